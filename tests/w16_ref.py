"""Builders, checks, plain-torch twins and mutants for the two 16-row kernels behind the 16-bit-weight and int8-weight ops:
f16_gemm_kernel (f16_gemm.cuh, tg_gemm_f16, the *_w_f16TC ops) and w8_gemm_kernel (w8_gemm.cuh, the 16-row path of tg_gemm_w8).

A plain helper module (not a conftest), in the style of tests/fused_ref.py.  Every check takes a callable and the device to build its
inputs on: tests/test_gpu_w16_f64.py passes the ops, tests/test_w16_ref_cpu.py a twin (which must pass) or a mutant (which must fail).

  16-bit weights   gemm(x [m][k], w [n][k]) -> y [m][>= n]                     (the callable packs w into its layout)
                   gemm(x, w, out=y) writes y [m][n] in place                  (the output guard)
  int8 weights     gemm(x [m][k], codes int32 [n][k], sz [k / g][n_pad][2], g) -> y [m][n_pad],  n_pad = n rounded up to gemm.pad

The contract is the project's own (tests/test_gpu_parity.py assert_gemm_close): y64 = x64 @ w64^T in float64 on the given 16-bit
values -- for int8 on oracle.dequant's RNE16(fma(b - 128, scale, zero)) -- and

    |y - y64| <= 0.5 ulp16(y64) (1 + 2^-7) + 4e-6 sum|x||w|

(fused_ref.contract: the same expression).  Nothing here is fitted to a kernel's output.

Loop regimes (read from the kernels; the shapes of F16_CASES / W8_CASES are the smallest that reach each):
  f16_gemm_kernel: 8 waves, wave v takes the 32-k steps v, v + 8, ... : nw = ceil((k / 32 - v) / 8) of them through a ring of 4.  The
    steady loop runs while base + 8 <= nw, the remainder (at most 7 steps) refills only where a step exists; a wave with nw = 0 loads its
    clamped last step four times and must add nothing.  A column's class is k mod 1024 = ring slot x wave x position in the step.
  w8_gemm_kernel: 8 waves = splitk slices x 8 / splitk row tiles per workgroup, steps of 64 k through a ring of 2; launch_w8 doubles the
    split while tiles x split < 4096 and 2 split <= nsteps = ceil(k / 64).
"""
from types import SimpleNamespace

import numpy as np
import torch

from tests.conftest import bits16, from_bits16
from tests.fused_ref import SENTINEL, contract, guard_intact, guarded

BF16, F16 = torch.bfloat16, torch.float16
DECOY = 2.0 ** 15   # finite and exact in both types


def dt_name(dtype):
    return "bf16" if dtype == BF16 else "fp16"


def _cdiv(a, b):
    return -(-a // b)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16).cpu(), b.contiguous().view(torch.int16).cpu())


# ---------------------------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------------------------
# f16_gemm_kernel: (k, regime, m, wrows on the right, wrows on the left).  Every k runs on the three layouts and both dtypes; every m and
# every wrows appears with a steady-loop k (k >= 2048).  nw per wave 0 ... 7 in the comment.
F16_SHAPES = [
    (32,        "one step; waves 1 ... 7 have nw = 0",                     1,   8, 16),   # nw 1 0 0 0 0 0 0 0
    (96,        "nw differs between waves, below one ring",                5,  24, 48),   # nw 1 1 1 0 0 0 0 0
    (288,       "nw differs between waves, below one ring",               17,  48, 16),   # nw 2 1 1 1 1 1 1 1
    (544,       "nw = 3 / 2: below one ring",                             16,  24, 16),   # nw 3 2 2 2 2 2 2 2
    (1024 + 32, "nw = 5 / 4: refills inside the remainder rounds",        33, 136, 48),   # nw 5 4 4 4 4 4 4 4
    (2048,      "nw = 8: exactly one steady round",                        1,   8, 16),   # nw 8 x 8
    (2048 + 32, "steady loop, ragged waves (nw = 9 / 8)",                  5,  24, 48),   # nw 9 8 8 8 8 8 8 8
    (2048 + 224, "steady loop, ragged waves (nw = 9 x 7, 8)",             17, 136, 48),   # nw 9 9 9 9 9 9 9 8
    (2592,      "one steady round, remainders of 7 and 6 steps",           5,   8, 48),   # nw 11 10 10 10 10 10 10 10
    (4096,      "the real layer (nw = 16)",                               33,  48, 16),   # nw 16 x 8
    (14336,     "nw = 56, long f32 sums",                                 16, 136, 48),   # nw 56 x 8
]
F16_LAYOUTS = [("B", 1), ("B", 2), ("A", 1)]   # (weight side: B = on the right, A = on the left; innerKTiles)
STEADY_K = 2048


def f16_cases():
    out = []
    for dtype in (BF16, F16):
        for side, inner in F16_LAYOUTS:
            for k, what, m, nr, nl in F16_SHAPES:
                out.append(SimpleNamespace(dtype=dtype, side=side, inner=inner, m=m, n=nr if side == "B" else nl, k=k, what=what, scale=1.0))
    # fp16, some outputs subnormal (|y| < 2^-14): x ~ 2^-7, w ~ 2^-10, y ~ 17 * 2^-17 = 1.3e-4 (a third of the outputs below 6.1e-5)
    out.append(SimpleNamespace(dtype=F16, side="B", inner=2, m=17, n=24, k=288, what="fp16 subnormal outputs", scale=2.0 ** -17))
    return out


def f16_id(c):
    return f"{dt_name(c.dtype)}-{c.side}{c.inner}-m{c.m}-n{c.n}-k{c.k}" + ("-subnormal" if c.scale != 1.0 else "")


F16_CASES = f16_cases()


def nw_f16(k, wave):
    """Steps of wave `wave` in f16_gemm_kernel."""
    return max(0, _cdiv(k // 32 - wave, 8))


def w8_split(m, wrows, k):
    """launch_w8 (tinygemm_hip.hip) restated: (split, row tiles, row tiles per workgroup, workgroups along the rows)."""
    tiles = _cdiv(wrows, 16) * _cdiv(m, 16)
    nsteps = (k // 16 + 3) // 4
    sk = 1
    while sk < 8 and tiles * sk < 256 * 16 and sk * 2 <= nsteps:
        sk *= 2
    tpb = 8 // sk
    return sk, _cdiv(wrows, 16), tpb, _cdiv(_cdiv(wrows, 16), tpb)


# w8_gemm_kernel: (m, n, k, side, innerKTiles, the split launch_w8 picks, what).  All m <= 16: the 16-row kernel (TG_TILE_W8_MIN_M = 17).
W8_SHAPES = [
    # 4097 row tiles >= 4096: split 1, 8 row tiles per workgroup, 513 workgroups; the last has ONE row tile (7 waves without one), half valid
    (5, 65544, 256, "B", 4, 1, "split 1, ragged last workgroup, half tile"),
    # 2049 tiles: 2049 < 4096 -> split 2, 4098 >= 4096 stops; 4 row tiles per workgroup, 513 workgroups, the last with one
    (5, 32776, 256, "B", 2, 2, "split 2, ragged last workgroup, half tile"),
    # 1025 tiles: split 4 (2 x 4 <= nsteps = 4 allows it, 4100 >= 4096 stops); 2 row tiles per workgroup, 513 workgroups, the last with one
    (5, 16400, 256, "A", 2, 4, "split 4, ragged last workgroup"),
    # nsteps = 1: split 1, 4 row tiles in one workgroup of 8 (waves 4 ... 7 without a row tile)
    (1, 64, 64, "B", 1, 1, "nsteps 1 caps the split at 1"),
    (1, 64, 64, "A", 1, 1, "nsteps 1 caps the split at 1"),
    # nsteps = 2: split 2, 5 row tiles (the last half valid on the right), 4 per workgroup, 2 workgroups, the last with one
    (16, 72, 128, "B", 2, 2, "nsteps 2 caps the split at 2"),
    (16, 72, 128, "A", 2, 2, "nsteps 2 caps the split at 2"),
    # 260 k-tiles, nsteps = 65: split 8, slice 0 takes 9 steps, the others 8 (steady rounds, a ragged remainder); k-tiles % 4 = 0 ...
    (16, 72, 4096 + 64, "B", 1, 8, "split 8, nw = 9 / 8"),
    (16, 72, 4096 + 64, "A", 1, 8, "split 8, nw = 9 / 8"),
    # (k = 4160 is no multiple of 128: g = 32 only.)  k = 4224: nsteps = 66, nw = 9 9 8 8 8 8 8 8, at g = 128 as well
    (16, 72, 4096 + 128, "B", 1, 8, "split 8, nw = 9 / 8, g = 128"),
    (16, 72, 4096 + 128, "A", 1, 8, "split 8, nw = 9 / 8, g = 128"),
    # ... and 262 k-tiles (k-tiles % 4 = 2): the last step's second K-slot is clamped and its scale forced to zero
    (16, 72, 4096 + 96, "B", 1, 8, "split 8, clamped half step"),
    (16, 72, 4096 + 96, "A", 1, 8, "split 8, clamped half step"),
]


def w8_cases():
    return [SimpleNamespace(dtype=dt, g=g, m=m, n=n, k=k, side=side, inner=inner, split=split, what=what)
            for (m, n, k, side, inner, split, what) in W8_SHAPES for dt in (BF16, F16) for g in (32, 128) if k % g == 0]


def w8_id(c):
    return f"{dt_name(c.dtype)}-{c.side}{c.inner}-g{c.g}-m{c.m}-n{c.n}-k{c.k}"


W8_CASES = w8_cases()
LARGE_N = 4096    # from here on a case samples its weight rows


def sample_rows(n, split):
    """Rows of the first, a middle and the last workgroup of a large-n launch (whole workgroups: 128 / split rows each), the last 24 rows
    included."""
    per_wg = 16 * (8 // split)
    wgs = _cdiv(_cdiv(n, 16), 8 // split)
    rows = np.concatenate([np.arange(w * per_wg, min(n, (w + 1) * per_wg)) for w in (0, wgs // 2, wgs - 2, wgs - 1)])
    rows = np.unique(np.concatenate([rows, np.arange(n - 24, n)]))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------

def f16_inputs(m, n, k, dtype, device, seed=0, scale=1.0):
    """x = randn, w = 0.05 randn (|y| ~ 0.05 sqrt(k): 6 at k = 14336, far from the fp16 range).  scale != 1 (the subnormal case):
    x = 2^-7 randn, w = 2^7 scale randn."""
    gen = torch.Generator().manual_seed(1000 * seed + m + n + k)
    sx, sw = (1.0, 0.05) if scale == 1.0 else (2.0 ** -7, scale * 2.0 ** 7)
    x = (torch.randn(m, k, generator=gen) * sx).to(dtype)
    w = (torch.randn(n, k, generator=gen) * sw).to(dtype)
    return x.to(device), w.to(device)


def w8_inputs(m, n, k, g, dtype, device, pad, seed=0):
    """test_gpu_parity._rand_int8_problem's recipe: codes [n][k] int32, x [m][k], sz [k / g][n_pad][2] with the padded rows' scale =
    zero = 0, on `device`.  Drawn on the CPU (the same inputs for a twin and a kernel) below LARGE_N rows, on `device` from there on."""
    src = device if n >= LARGE_N else "cpu"
    gen = torch.Generator(device=src).manual_seed(1000 * seed + m + n + k + g)
    codes = torch.randint(0, 256, (n, k), dtype=torch.int32, generator=gen, device=src).to(device)
    x = torch.randn(m, k, generator=gen, device=src).to(dtype).to(device)
    n_pad = _cdiv(n, pad) * pad
    sz = torch.zeros(k // g, n_pad, 2, dtype=dtype, device=device)
    sz[:, :n, 0] = (torch.rand(k // g, n, generator=gen, device=src) * 0.002 + 0.0005).to(dtype).to(device)
    sz[:, :n, 1] = (torch.randn(k // g, n, generator=gen, device=src) * 0.01).to(dtype).to(device)
    return codes, x, sz


def oracle_int8(oracle, codes, sz, g, dtype, rows=None):
    """oracle.dequant's weights (16-bit tensor [rows][k]) of the rows `rows` (None: all n)."""
    n = codes.shape[0]
    sel = slice(0, n) if rows is None else torch.from_numpy(rows).to(codes.device)
    c = codes[sel].cpu().contiguous().numpy()
    q = sz[:, sel].cpu().contiguous()
    w = oracle.dequant(c, g, oracle.Q_INT8, bits16(q), None, oracle.BF16 if dtype == BF16 else oracle.F16)
    return from_bits16(w, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# check 1: the float64 bound
# ---------------------------------------------------------------------------------------------------------------------------------

def f64_ratio(y, x, w):
    """max |y - y64| / allowance for y [m][n] against x [m][k], w [n][k] (16-bit tensors): the contract above."""
    x64, w64 = x.double().cpu(), w.double().cpu()
    y64 = (x64 @ w64.t()).numpy()
    S = (x64.abs() @ w64.abs().t()).numpy()
    return np.abs(y.double().cpu().numpy() - y64) / contract(y64, S, x.dtype)


def assert_f64(what, y, x, w, results=None):
    ratio = f64_ratio(y, x, w)
    worst = float(ratio.max())
    print(f"{what}: worst |y - y64| / allowance {worst:.3f}")
    if results is not None:
        results.append((what, worst))
    bad = ~(ratio <= 1)
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} outside the allowance, worst ratio {worst:.2f} at (row, column) {np.argwhere(bad)[:4].tolist()}"
    return worst


def check_f64_f16(gemm, c, device, results=None):
    x, w = f16_inputs(c.m, c.n, c.k, c.dtype, device, scale=c.scale)
    y = gemm(x, w)
    assert y.shape[0] == c.m and y.shape[1] >= c.n and y.dtype == c.dtype
    if c.scale != 1.0:
        y64 = (x.double() @ w.double().t()).abs()
        share = float(((y64 < 2.0 ** -14) & (y64 > 2.0 ** -24)).double().mean())
        assert share > 0.1, f"the subnormal case has {share:.2f} subnormal outputs"
    return assert_f64(f16_id(c), y[:, :c.n], x, w, results)


def check_f64_w8(gemm, oracle, c, device, results=None):
    """Large n (>= LARGE_N): the float64 comparison runs on sample_rows -- every row of the first, a middle and the last two workgroups and
    the last 24 rows -- so that the oracle dequantises a few hundred rows, not 16 M weights."""
    codes, x, sz = w8_inputs(c.m, c.n, c.k, c.g, c.dtype, device, gemm.pad)
    y = gemm(x, codes, sz, c.g)
    n_pad = sz.shape[1]
    assert y.shape == (c.m, n_pad) and y.dtype == c.dtype
    if n_pad > c.n:
        assert (y[:, c.n:] == 0).all()   # padded rows: code 0 with scale = zero = 0 -> exact zeros
    rows = sample_rows(c.n, c.split) if c.n >= LARGE_N else None
    w = oracle_int8(oracle, codes, sz, c.g, c.dtype, rows)
    ysel = y[:, :c.n] if rows is None else y[:, torch.from_numpy(rows).to(y.device)]
    return assert_f64(w8_id(c), ysel, x, w, results)


# ---------------------------------------------------------------------------------------------------------------------------------
# check 2: selection probes (exact)
# ---------------------------------------------------------------------------------------------------------------------------------

def selection_columns(n, k, seed=0, period=1024):
    """pi(r), r < n: the first C = min(k, period) rows hit every column class mod `period` once (at a random multiple of the period),
    the remaining rows alternate between the first and the last 32-k step."""
    C = min(k, period)
    assert n >= C + 2, "not enough rows for every column class and both end steps"
    rng = np.random.default_rng(seed)
    cls = rng.permutation(C)
    reps = (k - 1 - cls) // period + 1
    cols = cls + period * (rng.integers(0, 1 << 30, C) % reps)
    rest = np.arange(n - C)
    ends = np.where(rest % 2 == 0, rng.integers(0, 32, n - C), k - 32 + rng.integers(0, 32, n - C))
    pi = np.concatenate([cols, ends])
    assert pi.max() < k and len(np.unique(pi % period)) == C and (pi < 32).any() and (pi >= k - 32).any()
    return pi


def nonzero_x(m, k, dtype, device, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=gen)
    x = torch.where(x.abs() < 2.0 ** -6, torch.full_like(x, 0.37), x).to(dtype)   # non-zero (and normal) in both types
    assert (x != 0).all()
    return x.to(device)


def check_select_f16(gemm, m, n, k, dtype, device, seed=0):
    """One 1.0 per weight row at column pi(r): y[:, r] == x[:, pi(r)] bit for bit."""
    pi = torch.from_numpy(selection_columns(n, k, seed)).to(device)
    w = torch.zeros(n, k, dtype=dtype, device=device)
    w[torch.arange(n, device=device), pi] = 1.0
    x = nonzero_x(m, k, dtype, device, seed + 11)
    y = gemm(x, w)[:, :n]
    want = x[:, pi]
    bad = (y.view(torch.int16) != want.contiguous().view(torch.int16)).cpu()
    assert not bad.any(), f"selection probe: {int(bad.sum())} / {bad.numel()} outputs differ; (row, weight row) {torch.nonzero(bad)[:4].tolist()}, columns {pi[torch.nonzero(bad)[:4, 1]].tolist()}"


def onehot_columns(m, k, seed=0):
    """j(a), a < m: the first and the last column, the two sides of the first step boundary, then random columns."""
    rng = np.random.default_rng(seed + 5)
    fixed = [0, k - 1, 31, 32 % k, k - 32, k // 2 + 1]
    return np.array((fixed + rng.integers(0, k, m).tolist())[:m])


def check_onehot_f16(gemm, m, n, k, dtype, device, seed=0):
    """The transposed probe: activation row a is 1.0 at column j(a): y[a, r] == w[r, j(a)] bit for bit."""
    _, w = f16_inputs(m, n, k, dtype, device, seed=seed + 3)
    j = torch.from_numpy(onehot_columns(m, k, seed)).to(device)
    x = torch.zeros(m, k, dtype=dtype, device=device)
    x[torch.arange(m, device=device), j] = 1.0
    y = gemm(x, w)[:, :n]
    want = w[:, j].t()
    bad = (y.view(torch.int16) != want.contiguous().view(torch.int16)).cpu()
    assert not bad.any(), f"one-hot probe: {int(bad.sum())} / {bad.numel()} outputs differ; (row, weight row) {torch.nonzero(bad)[:4].tolist()}"


def check_select_w8(gemm, m, n, k, g, dtype, device, seed=0):
    """Code 129 at column pi(r) of row r with scale 1, zero 0 in that column's group; every other code 128, every zero 0, the other
    groups' scales random: w = RNE16(fma(1, 1, 0)) = 1 there and RNE16(fma(0, s, 0)) = 0 elsewhere, so y[:, r] == x[:, pi(r)] bit for bit."""
    pi = torch.from_numpy(selection_columns(n, k, seed)).to(device)
    r = torch.arange(n, device=device)
    codes = torch.full((n, k), 128, dtype=torch.int32, device=device)
    codes[r, pi] = 129
    n_pad = _cdiv(n, gemm.pad) * gemm.pad
    gen = torch.Generator().manual_seed(seed + 7)
    sz = torch.zeros(k // g, n_pad, 2, dtype=dtype, device=device)
    sz[:, :n, 0] = (torch.rand(k // g, n, generator=gen) * 3 + 1.5).to(dtype).to(device)
    sz[pi // g, r, 0] = 1.0
    x = nonzero_x(m, k, dtype, device, seed + 11)
    y = gemm(x, codes, sz, g)[:, :n]
    want = x[:, pi]
    bad = (y.view(torch.int16) != want.contiguous().view(torch.int16)).cpu()
    assert not bad.any(), f"int8 selection probe: {int(bad.sum())} / {bad.numel()} outputs differ; (row, weight row) {torch.nonzero(bad)[:4].tolist()}, columns {pi[torch.nonzero(bad)[:4, 1]].tolist()}"


def check_onehot_w8(gemm, oracle, m, n, k, g, dtype, device, seed=0):
    """One-hot activation rows against random codes / scales / zeros: y[a, r] == oracle.dequant's w[r, j(a)] bit for bit."""
    codes, _, sz = w8_inputs(m, n, k, g, dtype, device, gemm.pad, seed=seed + 3)
    j = torch.from_numpy(onehot_columns(m, k, seed)).to(device)
    x = torch.zeros(m, k, dtype=dtype, device=device)
    x[torch.arange(m, device=device), j] = 1.0
    y = gemm(x, codes, sz, g)[:, :n].cpu()
    want = oracle_int8(oracle, codes, sz, g, dtype)[:, j.cpu()].t()
    bad = y.view(torch.int16) != want.contiguous().view(torch.int16)
    assert not bad.any(), f"int8 one-hot probe: {int(bad.sum())} / {bad.numel()} outputs differ; (row, weight row) {torch.nonzero(bad)[:4].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------------------
# check 3: decoys
# ---------------------------------------------------------------------------------------------------------------------------------

def _decoyed(t):
    return (t.float() + DECOY).to(t.dtype)


def with_decoy_rows(x, extra=32):
    """x [m][k] as the leading rows of a buffer of m + extra rows whose other rows are random values + 2^15."""
    m, k = x.shape
    gen = torch.Generator().manual_seed(m + k)
    big = _decoyed(torch.randn(m + extra, k, generator=gen).to(x.dtype)).to(x.device)
    big[:m] = x
    view = big[:m]
    assert view.is_contiguous() and view.data_ptr() == big.data_ptr()
    return view, big


def check_decoy_f16(gemm, m, n, k, dtype, device):
    x, w = f16_inputs(m, n, k, dtype, device, seed=4)
    clean = gemm(x, w)[:, :n].clone()
    view, _big = with_decoy_rows(x)
    assert bits_equal(gemm(view, w)[:, :n], clean), "activation rows >= m were read"


def check_decoy_w8(gemm, m, n, k, g, dtype, device):
    """Rows >= m of the activation buffer and the scale / zero columns of the padded weight rows hold + 2^15: the outputs of the n real
    rows keep their bits (n is no multiple of gemm.pad)."""
    codes, x, sz = w8_inputs(m, n, k, g, dtype, device, gemm.pad, seed=4)
    assert sz.shape[1] > n
    clean = gemm(x, codes, sz, g)[:, :n].clone()
    view, _big = with_decoy_rows(x)
    assert bits_equal(gemm(view, codes, sz, g)[:, :n], clean), "activation rows >= m were read"
    sz2 = sz.clone()
    sz2[:, n:] = _decoyed(sz[:, n:])
    assert bits_equal(gemm(view, codes, sz2, g)[:, :n], clean), "a padded weight row's scale / zero reached a real row"


# ---------------------------------------------------------------------------------------------------------------------------------
# check 4: non-finite placement
# ---------------------------------------------------------------------------------------------------------------------------------

def _check_nonfinite(run_clean, run, x, w64_of, nan_w_row=None):
    """run_clean(x) / run(x) -> y [m][n] on the clean / the probed weights; w64_of: the float64 weights [n][k] (with the NaN weight in
    place).  One inf and one NaN in x, in different rows."""
    m, k = x.shape
    clean = run_clean(x).clone()
    a_inf, a_nan = (0, m - 1) if m > 1 else (0, None)
    x2 = x.clone()
    x2[a_inf, (3 * k) // 4 + 1] = float("inf")
    if a_nan is not None:
        x2[a_nan, k - 1] = float("nan")
    y = run(x2)
    with np.errstate(invalid="ignore"):
        y64 = x2.double().cpu().numpy() @ w64_of.numpy().T
    yf = y.float().cpu().numpy()
    assert np.array_equal(np.isnan(yf), np.isnan(y64)), "NaN placement differs from the float64 product"
    assert np.array_equal(np.isinf(yf), np.isinf(y64)) and np.array_equal(np.sign(yf[np.isinf(yf)]), np.sign(y64[np.isinf(y64)])), "inf placement differs"
    area = np.zeros(y64.shape, bool)     # where the probe's inputs reach
    area[a_inf] = True
    if a_nan is not None:
        area[a_nan] = True
    if nan_w_row is not None:
        area[:, nan_w_row] = True
    touched = ~np.isfinite(y64)
    assert not (touched & ~area).any() and touched[a_inf].any(), "the probe's own inputs overflow"
    keep = torch.from_numpy(~touched)
    same = (y.view(torch.int16).cpu() == clean.view(torch.int16).cpu()) | ~keep
    assert same.all(), f"{int((~same).sum())} finite outputs changed bits next to a non-finite input"


def check_nonfinite_f16(gemm, m, n, k, dtype, device):
    x, w = f16_inputs(m, n, k, dtype, device, seed=5)
    r = n - 3
    w2 = w.clone()
    w2[r, k // 3] = float("nan")
    _check_nonfinite(lambda xx: gemm(xx, w)[:, :n], lambda xx: gemm(xx, w2)[:, :n], x, w2.double().cpu(), nan_w_row=r)


def check_nonfinite_w8(gemm, oracle, m, n, k, g, dtype, device):
    codes, x, sz = w8_inputs(m, n, k, g, dtype, device, gemm.pad, seed=5)
    w = oracle_int8(oracle, codes, sz, g, dtype)
    run = lambda xx: gemm(xx, codes, sz, g)[:, :n]
    _check_nonfinite(run, run, x, w.double())


# ---------------------------------------------------------------------------------------------------------------------------------
# check 5: the output guard (16-bit weights; gemm(x, w, out=y))
# ---------------------------------------------------------------------------------------------------------------------------------

def check_guard_f16(gemm, m, n, k, dtype, device):
    """y [m][n] is a window of a sentinel-filled buffer: every element of it is written (the bits of the plain call), nothing around it."""
    x, w = f16_inputs(m, n, k, dtype, device, seed=6)
    want = gemm(x, w)[:, :n]
    out, whole = guarded(torch.zeros(m, n, dtype=dtype), device, fill=SENTINEL)
    out.view(torch.int16).fill_(0x7FC1)   # a NaN in both types
    gemm(x, w, out=out)
    assert guard_intact(out, whole), "the launch wrote outside its output"
    assert bits_equal(out, want), "the guarded output differs from the plain call"


# ---------------------------------------------------------------------------------------------------------------------------------
# check 6: determinism (graph capture is the GPU file's)
# ---------------------------------------------------------------------------------------------------------------------------------

def check_deterministic(run):
    a = run().clone()
    assert bits_equal(run(), a), "two calls differ"
    return a


# ---------------------------------------------------------------------------------------------------------------------------------
# twins and mutants (plain torch on the CPU)
# ---------------------------------------------------------------------------------------------------------------------------------

def _round16(acc, dtype, truncate=False):
    y = acc.to(dtype)
    if truncate:   # towards zero: step back where RNE went away from zero
        over = y.float().abs() > acc.abs()
        y = (y.view(torch.int16) - over.to(torch.int16)).view(dtype)
    return y


def _swap_1_8(t):
    """Columns 2Q + 1 and 2Q + 8 (Q = 0 ... 3) of every 16-k tile exchanged."""
    k = t.shape[1]
    idx = torch.arange(k).view(-1, 16).clone()
    for q in range(4):
        idx[:, [2 * q + 1, 2 * q + 8]] = idx[:, [2 * q + 8, 2 * q + 1]]
    return t[:, idx.reshape(-1)]


F16_MUTANTS = {
    "last_step_dropped": "the last 32-k step dropped",
    "last_step_twice": "the last step added twice (a clamped refill consumed)",
    "wrong_ring_slot": "the steady loop's activations taken from the wrong ring slot (steps s and s + 8 swapped for s >= 32)",
    "x_cols_swapped": "the x columns 2Q + 1 and 2Q + 8 swapped within a 32-k slot",
    "half_tile_previous_rows": "the last half tile (wrows % 16 = 8) reading the previous tile's rows",
    "idle_wave_adds": "waves with nw = 0 contributing their clamped step",
    "row_m_unmasked": "a row >= m unmasked",
    "partials_in_16_bit": "16-bit accumulation of the 8 wave partials (double rounding)",
    "truncation": "truncation in place of RNE",
}
W8_MUTANTS = {
    "zero_once_per_row": "int8: the zero applied once per row instead of per group",
    "byte_order_as_k_order": "int8: byte order k 2q, 2q+1, 2q+8, 2q+9 taken as stored order",
    "last_step_dropped": "int8: the last 64-k step dropped",
    "truncation": "int8: truncation in place of RNE",
}


class TwinF16:
    """f16_gemm_kernel in plain torch: wave v's f32 partial over the steps v, v + 8, ..., the 8 partials added in f32, ONE rounding
    (RNE).  pad: 8 (weights on the right) or 16 (left).  mutant: a key of F16_MUTANTS, or None."""

    def __init__(self, pad, mutant=None):
        assert mutant is None or mutant in F16_MUTANTS
        self.pad, self.mutant = pad, mutant

    def __call__(self, x, w, out=None):
        mu = self.mutant
        m, k = x.shape
        n = w.shape[0]
        assert k % 32 == 0
        n_real, n = n, _cdiv(n, self.pad) * self.pad      # the layout pads the rows with zeros
        xf, wf = x.float(), torch.cat([w.float(), torch.zeros(n - n_real, k)])
        steps = k // 32
        if mu == "x_cols_swapped":
            xf = _swap_1_8(xf)
        if mu == "wrong_ring_slot":
            idx = torch.arange(steps)
            for s in range(32, steps - 8):
                if (s // 8) % 2 == 0:
                    idx[s], idx[s + 8] = s + 8, s
            xf = xf.view(m, steps, 32)[:, idx].reshape(m, k)
        x3, w3 = xf.view(m, steps, 32), wf.view(n, steps, 32)
        last = steps - 1
        acc = torch.zeros(m, n)
        for wave in range(8):
            mine = list(range(wave, steps, 8))
            if mu == "last_step_dropped" and last in mine:
                mine.remove(last)
            if mu == "last_step_twice" and last in mine:
                mine.append(last)
            if mu == "idle_wave_adds" and not mine:
                mine = [last]
            if not mine:
                continue
            part = x3[:, mine].reshape(m, -1) @ w3[:, mine].reshape(n, -1).t()
            acc = (acc + part).to(x.dtype).float() if mu == "partials_in_16_bit" else acc + part
        y = _round16(acc, x.dtype, truncate=(mu == "truncation"))
        if mu == "half_tile_previous_rows" and n % 16 == 8 and n >= 16:
            y[:, n - 8:] = y[:, n - 16:n - 8]
        if out is None:
            return y
        rows = m + 1 if mu == "row_m_unmasked" else m
        dst = torch.as_strided(out, (rows, n), (n, 1))
        dst.copy_(torch.cat([y, y[-1:]])[:rows])      # (the clamped activation row m - 1 again)
        return out


class TwinW8:
    """w8_gemm_kernel in plain torch: w = RNE16(f32 (b - 128) * scale + zero) -- the product is exact in f32, so this is the fma --,
    an f32 matmul, one rounding.  side "B" pads the rows to 8, "A" to 16."""

    def __init__(self, side, mutant=None):
        assert mutant is None or mutant in W8_MUTANTS
        self.pad, self.mutant = (8 if side == "B" else 16), mutant

    def dequant(self, codes, sz, g):
        n, k = codes.shape
        sc = sz[:, :n, 0].float().repeat_interleave(g, dim=0).t()
        zz = sz[:, :n, 1].float()
        if self.mutant == "zero_once_per_row":
            zz = zz[:1].expand_as(zz)
        zz = zz.repeat_interleave(g, dim=0).t()
        b = (codes & 0xFF).float() - 128.0
        if self.mutant == "byte_order_as_k_order":
            b = _swap_1_8(b)
        return (b * sc + zz).to(sz.dtype)

    def __call__(self, x, codes, sz, g):
        n, k = codes.shape
        n_pad = sz.shape[1]
        assert n_pad == _cdiv(n, self.pad) * self.pad
        w = self.dequant(codes, sz, g).float()
        xf = x.float()
        if self.mutant == "last_step_dropped":
            xf = xf.clone()
            xf[:, (_cdiv(k, 64) - 1) * 64:] = 0
        y = torch.zeros(x.shape[0], n_pad, dtype=x.dtype)
        y[:, :n] = _round16(xf @ w.t(), x.dtype, truncate=(self.mutant == "truncation"))
        return y
