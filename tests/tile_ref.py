"""The launch plan restated, case tables, checks, a plain-torch twin and mutants for w4_gemm_tile_kernel (w4_gemm_tile.cuh, launched from
tg_tile.hip): the GEMM of every 4-bit call with more than 64 activation rows (from 17 with the op's workspace) and of tg_gemm_w8 from 17.

A plain helper module (not a conftest), in the style of tests/w16_ref.py.  Every check takes a callable gemm(P, bias=None, workspace=True)
-> y [m][wrows] (a CPU tensor) on a Problem P (below): tests/test_gpu_tile_f64.py passes the C ABI, tests/test_tile_ref_cpu.py the twin
(which must pass) or a mutant (which must fail the check named for it).

The contract is the project's own (tests/test_gpu_parity.py assert_gemm_close): y64 = x64 @ w64^T in float64 on the oracle's weights
RNE16(fma(lut, scale, zero)) (int8: RNE16(fma(b - 128, scale, zero))) and

    |y - y64| <= 0.5 ulp16(y64) (1 + 2^-7) + 4e-6 sum|x||w|

(fused_ref.contract: the same expression).  Nothing here is fitted to a kernel's output.

Regimes (read from the kernel and from tgx::tile / tgx::tile_w8 / tile_splits; tile_plan restates the three):
  tile shape   128 x 64 (65 rows or more, int8 from 17), 64 x 64 (17 ... 64 rows, only as a split launch), 128 x 128 (no mx4, no int8) once
               ceil(m / 128) ceil(wrows / 128) >= CUs -- the only flavour with DX = 3 stages of x, two packed words per dequantising
               thread, the consumers' "one half at a time" branch, and g = 128 / 256 at KS = 1
  KS           64-k super-tiles per step: 2 where the split's super-tiles are even (int8: and g >= 128), never on the 128 x 128 tile
  splits       1 / 2 / 4 / 8 k ranges (tile_splits), f32 partial tiles, tile_split_sum_kernel adds them in split order
  steps        ksteps = k / 64 / splits / KS per workgroup through the ring of packed words (4 slots) and the ring of scale / zero words
               (4 slots): steps mod 4 and steps > 4 decide whether a ring wraps and leaves a remainder
  groups       steps per group 1 / 2 / 4 (tables double-buffered by (step >> log2 steps per group) & 1), groups per step nsub 1 / 2 / 4
  grid         ntot = tiles_m tiles_n splits workgroups, dealt to the XCDs by ntot / 8 and ntot % 8
"""
import copy
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests.conftest import bits16, from_bits16
from tests.fused_ref import contract

BF16, F16 = torch.bfloat16, torch.float16
QT = {"int4": 0, "any4_global": 1, "any4_rowwise": 2, "mx4": 3}
DECOY = 2.0 ** 15   # finite and exact in both types
TILE_MIN_M_SPLIT, TILE_MIN_M, TILE_W8_MIN_M = 17, 65, 17   # tg_common.cuh
FP4 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def dt_name(dtype):
    return "bf16" if dtype == BF16 else "fp16"


def _cdiv(a, b):
    return -(-a // b)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16).cpu(), b.contiguous().view(torch.int16).cpu())


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch plan (tg_tile.hip restated)
# ---------------------------------------------------------------------------------------------------------------------------------

def tile_splits(tiles, ksuper, g64, cus, workspace=True):
    """tile_splits: as many splits (2 / 4 / 8) as keep tiles x splits <= CUs, whole groups, eight super-tiles or more per split."""
    splits = 1
    while splits < 8 and tiles * splits * 2 <= cus and ksuper % (splits * 2) == 0 and (ksuper // (splits * 2)) % g64 == 0 and ksuper // (splits * 2) >= 8:
        splits *= 2
    return splits if workspace else 1


def tile_plan(m, wrows, k, g, qtype, cus, workspace=True, int8=False, on_right=True, dtype=BF16):
    """(BM, BN, KS, splits, ksteps, steps_per_group, nsub, ntot) of the tile GEMM's launch for one problem of a call (batch 1, no fused
    norm / epilogue, innerKTiles 4 -- int8: 2), or None where tgx::tile / tgx::tile_w8 decline.  qtype: a key of QT (ignored for int8)."""
    gshift = {32: 5, 64: 6, 128: 7, 256: 8}[g]
    if k % 64 != 0 or k % g != 0:
        return None
    ksuper = k // 64
    if int8:
        if g < 64 or m < TILE_W8_MIN_M or wrows % (8 if on_right else 16) != 0:
            return None
        BM, BN = 128, 64
        tiles_m, tiles_n = _cdiv(m, 128), _cdiv(wrows, 64)
        splits = tile_splits(tiles_m * tiles_n, ksuper, g // 64, cus, workspace)
        KS = 2 if g >= 128 and (ksuper // splits) % 2 == 0 else 1
    else:
        if m < TILE_MIN_M_SPLIT or wrows % 8 != 0 or wrows < 8 or qtype not in QT:
            return None
        qmx = qtype == "mx4"
        if qmx and (dtype != BF16 or g != 32):
            return None
        small = m <= 64
        tiles_m = 1 if small else _cdiv(m, 128)
        wide = not small and not qmx and tiles_m * _cdiv(wrows, 128) >= cus
        tiles_n = _cdiv(wrows, 128 if wide else 64)
        splits = 1 if wide else tile_splits(tiles_m * tiles_n, ksuper, max(1, g // 64), cus, workspace)
        if splits == 1 and m < TILE_MIN_M:
            return None
        KS = 2 if not wide and (ksuper // splits) % 2 == 0 else 1
        BM, BN = (128, 128) if wide else (64, 64) if small else (128, 64)
    ksh = KS - 1
    ksteps = (ksuper // splits) >> ksh
    spg = 1 << (gshift - 6 - ksh) if gshift > 6 + ksh else 1
    nsub = 1 << (6 + ksh - gshift) if gshift < 6 + ksh else 1
    return BM, BN, KS, splits, ksteps, spg, nsub, tiles_m * tiles_n * splits


def regime(plan, kind="w4"):
    """What a case is there for: (words, BM x BN, KS, split or not, steps mod 4 (+ 4 from five steps on: a ring wraps), steps per group, groups per step)."""
    BM, BN, KS, splits, ksteps, spg, nsub, _ = plan
    return kind, f"{BM}x{BN}", KS, "split" if splits > 1 else "unsplit", ksteps % 4 + (4 if ksteps > 4 else 0), spg, nsub


def wide_shape(cus):
    """(m, wrows) of the smallest ragged launch on the 128 x 128 tile: ceil(sqrt(CUs)) tiles each way, m % 128 = 10, wrows % 128 = 120."""
    t = math.isqrt(cus - 1) + 1
    return t * 128 - 118, t * 128 - 8


def capped_rows(cus):
    """wrows (wrows % 64 = 8) of a 300-row launch whose 3 x tiles_n tiles allow split 4 and not 8: CUs / 8 < 3 tiles_n <= CUs / 4."""
    return (cus // 15) * 64 - 56


# ---------------------------------------------------------------------------------------------------------------------------------
# the case tables.  A row: (m, wrows, k, groups, (BM, BN, KS, splits, ksteps) it is there for).  Written for 256 CUs; the CU count enters at
# the wide shape and at the capped split, both derived from it; every other row holds from 64 CUs on (its tiles x 8 <= 64).
# ---------------------------------------------------------------------------------------------------------------------------------

def _w4_rows(cus):
    mw, nw = wide_shape(cus)
    return [
        # 128 x 64, KS = 1 (an odd number of super-tiles), unsplit: 1, 3, 5, 9 steps
        (65, 72, 64, (32, 64), (128, 64, 1, 1, 1)),
        (129, 104, 192, (32, 64), (128, 64, 1, 1, 3)),
        (130, 200, 320, (32, 64), (128, 64, 1, 1, 5)),
        (255, 72, 576, (32, 64), (128, 64, 1, 1, 9)),
        # 128 x 64, KS = 2, unsplit: 1, 2, 3, 5 steps; 10 and 18 steps at two steps per group (the group condition refuses the split)
        (65, 104, 128, (32, 64, 128), (128, 64, 2, 1, 1)),
        (130, 72, 256, (32, 64, 128, 256), (128, 64, 2, 1, 2)),
        (129, 136, 384, (32, 64, 128), (128, 64, 2, 1, 3)),      # 2 x 3 tiles: ntot % 8 = 6
        (255, 104, 640, (32, 64, 128), (128, 64, 2, 1, 5)),
        (65, 72, 1280, (256,), (128, 64, 2, 1, 10)),
        (130, 104, 2304, (256,), (128, 64, 2, 1, 18)),
        (300, 136, 256, (64,), (128, 64, 2, 1, 2)),              # 3 x 3 tiles: an odd ntot
        # split-K
        (65, 72, 1024, (32, 128, 256), (128, 64, 2, 2, 4)),
        (130, 200, 2048, (64, 256), (128, 64, 2, 4, 4)),
        (129, 104, 4096, (128,), (128, 64, 2, 8, 4)),
        (65, 200, 1536, (32, 128), (128, 64, 2, 2, 6)),
        (255, 72, 1280, (64, 128), (128, 64, 2, 2, 5)),
        (65, 104, 1152, (32, 64), (128, 64, 1, 2, 9)),
        (130, 72, 2304, (32, 64), (128, 64, 1, 4, 9)),
        (65, 136, 4608, (128,), (128, 64, 2, 4, 9)),             # ntot = 12: ntot % 8 = 4
        (300, capped_rows(cus), 4096, (128,), (128, 64, 2, 4, 8)),   # the tile count caps the split below what k allows
        # 64 x 64 (always split)
        (17, 72, 1024, (32, 128), (64, 64, 2, 2, 4)),
        (33, 104, 2048, (64, 256), (64, 64, 2, 4, 4)),
        (64, 72, 4096, (128,), (64, 64, 2, 8, 4)),
        (33, 200, 1152, (32, 64), (64, 64, 1, 2, 9)),
        (64, 104, 1536, (32,), (64, 64, 2, 2, 6)),
        # 128 x 128
        (mw, nw, 64, (32,), (128, 128, 1, 1, 1)),
        (mw, nw, 320, (64,), (128, 128, 1, 1, 5)),
        (mw, nw, 768, (32, 64, 128, 256), (128, 128, 1, 1, 12)),   # 1 / 1 / 2 / 4 steps per table buffer
    ]


def _mx4_rows(cus):
    mw, nw = wide_shape(cus)
    return [
        (65, 72, 64, (128, 64, 1, 1, 1)), (129, 104, 192, (128, 64, 1, 1, 3)), (130, 72, 256, (128, 64, 2, 1, 2)), (255, 104, 640, (128, 64, 2, 1, 5)),
        (65, 104, 1152, (128, 64, 1, 2, 9)), (130, 200, 2048, (128, 64, 2, 4, 4)), (33, 104, 1024, (64, 64, 2, 2, 4)), (33, 200, 1152, (64, 64, 1, 2, 9)),
        (mw, nw, 64, (128, 64, 1, 1, 1)),   # the 128 x 128 tile's shape: mx4 stays on 128 x 64
    ]


_W8_ROWS = [
    (17, 72, 192, (64,), (128, 64, 1, 1, 3)), (130, 104, 320, (64,), (128, 64, 1, 1, 5)), (17, 72, 1152, (64,), (128, 64, 1, 2, 9)),
    (130, 72, 256, (128, 256), (128, 64, 2, 1, 2)), (17, 104, 1024, (128, 256), (128, 64, 2, 2, 4)), (130, 72, 2048, (128, 256), (128, 64, 2, 4, 4)),
]


def _case(kind, qtype, dtype, side, g, m, wrows, k, want):
    if side == "A":
        wrows = _cdiv(wrows, 16) * 16      # (weights on the left: rows padded to 16; the same tiles)
    return SimpleNamespace(kind=kind, qtype=qtype, dtype=dtype, side=side, g=g, m=m, wrows=wrows, n=wrows - 3, k=k, want=want)


def cases(cus=256):
    """The float64 cases.  4-bit: the word flavour (int4, any4 global, any4 row-wise), the type and -- every fifth -- native
    weights-on-the-left words rotate over the rows; mx4: bf16, g = 32; int8: both word orders (Bint8 / Aint8) on every row."""
    out, i = [], 0
    for m, wrows, k, gs, want in _w4_rows(cus):
        for g in gs:
            side = "A" if i % 5 == 4 and want[1] == 64 else "B"      # (the 128 x 128 rows keep wrows % 128 = 120)
            out.append(_case("w4", ("int4", "any4_global", "any4_rowwise")[i % 3], (BF16, F16)[i % 2], side, g, m, wrows, k, want))
            i += 1
    for m, wrows, k, want in _mx4_rows(cus):
        out.append(_case("w4", "mx4", BF16, "B", 32, m, wrows, k, want))
    for m, wrows, k, gs, want in _W8_ROWS:
        for g in gs:
            for side in ("B", "A"):
                out.append(_case("w8", "int8", (BF16, F16)[i % 2], side, g, m, wrows, k, want))
                i += 1
    return out


def probe_cases(cus=256):
    """One representative of every (words, tile shape, KS, split or not) class and the 128 x 128 tile, with enough weight rows for every
    column class of the selection probe (select_columns) and enough activation rows for both ends of every group (onehot_columns); more
    than four steps wherever the class has such a k."""
    mw, nw = wide_shape(cus)
    w4 = [("int4", BF16, "B", 32, 130, 264, 576, (128, 64, 1, 1, 9)),
          ("any4_rowwise", F16, "B", 32, 65, 520, 640, (128, 64, 2, 1, 5)),
          ("any4_rowwise", BF16, "A", 32, 130, 528, 1152, (128, 64, 1, 2, 9)),
          ("int4", F16, "B", 64, 65, 1032, 1536, (128, 64, 2, 2, 6)),
          ("any4_global", BF16, "B", 64, 64, 520, 1152, (64, 64, 1, 2, 9)),
          ("any4_rowwise", F16, "B", 128, 64, 1032, 1536, (64, 64, 2, 2, 6)),
          ("any4_rowwise", BF16, "B", 64, mw, nw, 320, (128, 128, 1, 1, 5)),
          ("mx4", BF16, "B", 32, 130, 264, 576, (128, 64, 1, 1, 9)),
          ("mx4", BF16, "B", 32, 64, 1032, 1024, (64, 64, 2, 2, 4))]     # (g = 32: 64 rows hold both ends of 32 groups)
    w8 = [(BF16, "B", 64, 17, 264, 320, (128, 64, 1, 1, 5)), (F16, "A", 128, 33, 528, 640, (128, 64, 2, 1, 5)),
          (F16, "B", 64, 130, 520, 1152, (128, 64, 1, 2, 9)), (BF16, "A", 128, 33, 1040, 1536, (128, 64, 2, 2, 6))]
    out = [_case("w4", *r) for r in w4] + [_case("w8", "int8", *r) for r in w8]
    for c in out:
        c.n = c.wrows                      # (the selection probe uses every row; the other probes take wrows - 3 themselves)
    return out


def group_cases(cus=256):
    """One-hot activation rows where the table buffer turns: the 128 x 128 tile at 12 steps with 1 / 2 / 4 steps per group (three turns at
    g = 256), and 128 x 64 at KS = 2 with two steps per group (g = 256, 10 steps)."""
    mw, nw = wide_shape(cus)
    return [_case("w4", "any4_rowwise", BF16, "B", 32, mw, nw, 768, (128, 128, 1, 1, 12)), _case("w4", "int4", F16, "B", 128, mw, nw, 768, (128, 128, 1, 1, 12)),
            _case("w4", "any4_global", BF16, "B", 256, mw, nw, 768, (128, 128, 1, 1, 12)), _case("w4", "any4_rowwise", F16, "B", 256, 65, 72, 1280, (128, 64, 2, 1, 10))]


def placement_cases(cus=256):
    """A ragged launch on each tile shape (every output checked): 3 x 3 tiles unsplit (an odd ntot), a split launch, 64 x 64, 128 x 128, int8."""
    mw, nw = wide_shape(cus)
    return [_case("w4", "any4_rowwise", BF16, "B", 64, 300, 136, 256, (128, 64, 2, 1, 2)), _case("w4", "any4_rowwise", F16, "B", 64, 130, 200, 2048, (128, 64, 2, 4, 4)),
            _case("w4", "any4_rowwise", BF16, "A", 128, 33, 104, 1024, (64, 64, 2, 2, 4)), _case("w4", "any4_rowwise", F16, "B", 64, mw, nw, 320, (128, 128, 1, 1, 5)),
            _case("w4", "mx4", BF16, "B", 32, 130, 200, 2048, (128, 64, 2, 4, 4)), _case("w8", "int8", BF16, "B", 64, 130, 200, 1152, (128, 64, 1, 2, 9)),
            _case("w8", "int8", F16, "A", 128, 130, 200, 256, (128, 64, 2, 1, 2))]


def flavour(c):
    return "mx4" if c.qtype == "mx4" else c.kind


def case_regime(c, cus, workspace=True):
    return regime(plan_of(c, cus, workspace), flavour(c))


def wanted_regime(c):
    """The regime the table writes next to a case: its (BM, BN, KS, splits, ksteps) with the case's own group size."""
    bm, bn, ks, splits, ksteps = c.want
    return flavour(c), f"{bm}x{bn}", ks, "split" if splits > 1 else "unsplit", ksteps % 4 + (4 if ksteps > 4 else 0), max(1, c.g // (64 * ks)), max(1, 64 * ks // c.g)


def assert_regimes_reached(cs, cus):
    """The restated plan of every case lands in the regime the table writes next to it, and no regime is missing.  Returns the set."""
    reached, wanted = {case_regime(c, cus) for c in cs}, {wanted_regime(c) for c in cs}
    assert reached == wanted and len(reached) >= 50, sorted(reached ^ wanted)
    return reached


def case_id(c):
    return f"{c.qtype}-{dt_name(c.dtype)}-{c.side}-g{c.g}-m{c.m}-n{c.wrows}-k{c.k}"


def plan_of(c, cus, workspace=True):
    return tile_plan(c.m, c.wrows, c.k, c.g, c.qtype, cus, workspace, c.kind == "w8", c.side == "B", c.dtype)


def assert_regime(c, cus, workspace=True):
    """The precondition of every case: the restated plan is the one the case names (a case that drifts fails here, it does not pass elsewhere)."""
    plan = plan_of(c, cus, workspace)
    assert plan is not None and plan[:5] == c.want, f"{case_id(c)}: the launch plan is {plan}, the case is there for {c.want}"
    return plan


# ---------------------------------------------------------------------------------------------------------------------------------
# problems: CPU tensors, the quantisation info and row-wise LUT with one row per PADDED weight row
# ---------------------------------------------------------------------------------------------------------------------------------

def problem(c, seed=0):
    """test_gpu_parity.rand_problem's recipe (int8: _rand_int8_problem's) at c's shape: codes [n][k] int32, x [m][k], qinfo [k / g][wrows][2]
    (scale, zero; padded rows 0) -- mx4: uint8 exponents [wrows][k / 32] in 120 ... 130 (padded rows 127) --, lut None / [16] / [wrows][16]."""
    gen = torch.Generator().manual_seed(1000 * seed + c.m + c.wrows + c.k + c.g)
    n, k, g, dt = c.n, c.k, c.g, c.dtype
    P = SimpleNamespace(kind=c.kind, qtype=c.qtype, dtype=dt, side=c.side, g=g, m=c.m, n=n, wrows=c.wrows, k=k, lut=None, packed=None)
    P.codes = torch.randint(0, 256 if c.kind == "w8" else 16, (n, k), dtype=torch.int32, generator=gen)
    P.x = torch.randn(c.m, k, generator=gen).to(dt)
    if c.qtype == "mx4":
        P.qinfo = torch.full((c.wrows, k // 32), 127, dtype=torch.uint8)
        P.qinfo[:n] = torch.randint(120, 131, (n, k // 32), dtype=torch.uint8, generator=gen)
        return P
    s0, s1 = (0.002, 0.0005) if c.kind == "w8" else (0.02, 0.005)
    P.qinfo = torch.zeros(k // g, c.wrows, 2, dtype=dt)
    P.qinfo[:, :n, 0] = (torch.rand(k // g, n, generator=gen) * s0 + s1).to(dt)
    P.qinfo[:, :n, 1] = (torch.randn(k // g, n, generator=gen) * 0.01).to(dt)
    if c.qtype == "any4_global":
        P.lut = torch.randn(16, generator=gen).to(dt)
    elif c.qtype == "any4_rowwise":
        P.lut = torch.zeros(c.wrows, 16, dtype=dt)
        P.lut[:n] = torch.randn(n, 16, generator=gen).to(dt)
    return P


def vary(P, **kw):
    """P with some fields replaced (new codes drop the packed words an op cached on it)."""
    Q = copy.copy(P)
    for key, v in kw.items():
        setattr(Q, key, v)
    if "codes" in kw:
        Q.packed = None
    return Q


def oracle_w(oracle, P):
    """The oracle's weights of the n real rows: a 16-bit tensor [n][k]."""
    n = P.n
    if P.kind == "w8":
        w = oracle.dequant(P.codes.numpy(), P.g, oracle.Q_INT8, bits16(P.qinfo[:, :n].contiguous()), None, oracle.BF16 if P.dtype == BF16 else oracle.F16)
        return from_bits16(w, P.dtype)
    q = {"int4": oracle.Q_INT4, "any4_global": oracle.Q_ANY4_GLOBAL, "any4_rowwise": oracle.Q_ANY4_ROWWISE, "mx4": oracle.Q_MX4}[P.qtype]
    qi = P.qinfo[:n].contiguous().numpy() if P.qtype == "mx4" else bits16(P.qinfo[:, :n].contiguous())
    lut = None if P.lut is None else bits16(P.lut if P.lut.dim() == 1 else P.lut[:n].contiguous())
    w = oracle.dequant(P.codes.numpy(), P.g, q, qi, lut, oracle.BF16 if P.dtype == BF16 else oracle.F16)
    return from_bits16(w, P.dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# check 1: the float64 bound, the padded rows, the fused bias, the unsplit launch of a split case
# ---------------------------------------------------------------------------------------------------------------------------------

def f64_ratio(y, x, w):
    x64, w64 = x.double(), w.double()
    y64 = (x64 @ w64.t()).numpy()
    S = (x64.abs() @ w64.abs().t()).numpy()
    return np.abs(y.double().numpy() - y64) / contract(y64, S, x.dtype)


def assert_f64(what, y, x, w, results=None):
    assert not torch.isnan(y.float()).any(), f"{what}: NaN in y"
    ratio = f64_ratio(y, x, w)
    worst = float(ratio.max())
    print(f"{what}: worst |y - y64| / allowance {worst:.3f}")
    if results is not None:
        results.append((what, worst))
    bad = ~(ratio <= 1)
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} outside the allowance, worst ratio {worst:.2f} at (row, column) {np.argwhere(bad)[:4].tolist()}"
    return worst


def check_bias(gemm, P, y, what="", workspace=True):
    """A fused bias: RNE16(y + bias), the bits of the separate rounded add, on the direct store and on the split-sum store."""
    bias = torch.randn(P.wrows, generator=torch.Generator().manual_seed(5)).to(P.dtype)
    yb = gemm(P, bias=bias, workspace=workspace)
    assert bits_equal(yb, y + bias), f"{what}: the fused bias is not the separate rounded add"


def check_f64(gemm, oracle, c, cus, results=None):
    plan = assert_regime(c, cus)
    P = problem(c)
    w = oracle_w(oracle, P)
    what = f"{case_id(c)} {regime(plan, flavour(c))[1:]}"
    y = gemm(P)
    assert y.shape == (c.m, c.wrows) and y.dtype == c.dtype
    worst = assert_f64(what, y[:, :c.n], P.x, w, results)
    assert (y[:, c.n:] == 0).all(), "a padded weight row's output is not zero"
    check_bias(gemm, P, y, what)
    if plan[3] > 1 and plan_of(c, cus, workspace=False) is not None:     # the same problem unsplit: another summation order, the same contract
        p1 = plan_of(c, cus, workspace=False)
        assert p1[3] == 1 and p1[:2] == plan[:2]
        y1 = gemm(P, workspace=False)
        assert_f64(what + " no workspace " + str(regime(p1, flavour(c))[2:]), y1[:, :c.n], P.x, w, results)
        check_bias(gemm, P, y1, what, workspace=False)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# check 2: exact probes
# ---------------------------------------------------------------------------------------------------------------------------------

def select_columns(n, k, KS, splits, seed=0):
    """pi(r), r < n: one row per column class -- (split, column of the split mod 64 KS 4: position in the super-tile x plane of the step x
    ring slot), at a random turn of the ring --, then the first and the last column of every split, then random columns."""
    kl, per = k // splits, min(k // splits, 256 * KS)
    rng = np.random.default_rng(seed)
    s, j = np.divmod(np.arange(splits * per), per)
    reps = (kl - 1 - j) // per + 1
    cols = s * kl + j + per * (rng.integers(0, 1 << 30, len(j)) % reps)
    ends = np.array([[q * kl, q * kl + kl - 1] for q in range(splits)]).reshape(-1)
    assert n >= len(cols) + len(ends), f"{n} weight rows: {len(cols) + len(ends)} needed for every column class"
    pi = np.concatenate([rng.permutation(cols), ends, rng.integers(0, k, n - len(cols) - len(ends))])
    assert pi.max() < k and len(np.unique((pi // kl) * per + (pi % kl) % per)) == splits * per
    return pi


def nonzero_x(m, k, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=gen)
    x = torch.where(x.abs() < 2.0 ** -6, torch.full_like(x, 0.37), x).to(dtype)   # non-zero (and normal) in both types
    assert (x != 0).all()
    return x


def select_problem(c, plan, seed=0):
    """One weight 1.0 per row, at column pi(r), every other weight 0: int4 / int8 code 9 / 129 among 8s / 128s, any4 a LUT with a single
    1.0 (row-wise: at entry r % 16), mx4 code 2 (fp4 1.0) among 0s; scale 1 (mx4: exponent 127) in pi(r)'s group, random in the others,
    zero 0 everywhere."""
    n, k, g, dt = c.wrows, c.k, c.g, c.dtype
    P = problem(c, seed + 1)
    pi = torch.from_numpy(select_columns(n, k, plan[2], plan[3], seed))
    r = torch.arange(n)
    gen = torch.Generator().manual_seed(seed + 7)
    hot, cold = {"int8": (129, 128), "int4": (9, 8), "mx4": (2, 0)}.get(c.qtype, (None, None))
    if c.qtype == "any4_global":
        hot, cold, P.lut = 9, 4, torch.zeros(16, dtype=dt)
        P.lut[9] = 1.0
    if c.qtype == "any4_rowwise":
        hot, cold = r % 16, (r + 5) % 16
        P.lut = torch.zeros(n, 16, dtype=dt)
        P.lut[r, hot] = 1.0
        P.codes = cold.to(torch.int32)[:, None].repeat(1, k)
    else:
        P.codes = torch.full((n, k), cold, dtype=torch.int32)
    P.codes[r, pi] = hot if isinstance(hot, int) else hot.to(torch.int32)
    if c.qtype == "mx4":
        P.qinfo = torch.randint(120, 131, (n, k // 32), dtype=torch.uint8, generator=gen)
        P.qinfo[r, pi // 32] = 127
    else:
        P.qinfo = torch.zeros(k // g, n, 2, dtype=dt)
        P.qinfo[:, :, 0] = (torch.rand(k // g, n, generator=gen) * 3 + 1.5).to(dt)
        P.qinfo[pi // g, r, 0] = 1.0
    P.x, P.n, P.packed = nonzero_x(c.m, k, dt, seed + 11), n, None
    return P, pi


def check_select(gemm, c, cus, seed=0):
    """y[a, r] == x[a, pi(r)] bit for bit: the swizzle of both tiles, the x stage (step % NST), the w buffer, the ring slot, a split's ks0."""
    plan = assert_regime(c, cus)
    P, pi = select_problem(c, plan, seed)
    y = gemm(P)
    bad = y.view(torch.int16) != P.x[:, pi].contiguous().view(torch.int16)
    assert not bad.any(), (f"selection probe {case_id(c)}: {int(bad.sum())} / {bad.numel()} outputs differ; (row, weight row) {torch.nonzero(bad)[:4].tolist()}, "
                           f"columns {pi[torch.nonzero(bad)[:4, 1]].tolist()}")


def onehot_columns(m, k, g, splits, seed=0):
    """kappa(a), a < m: the first and the last k of every group (so of every split, and both 32-k halves of a g = 32 sub-group pair), then
    random columns."""
    rng = np.random.default_rng(seed + 5)
    ends = np.array([[q * g, q * g + g - 1] for q in range(k // g)]).reshape(-1)
    assert m >= len(ends), f"{m} activation rows: {len(ends)} needed for both ends of every group"
    return np.concatenate([rng.permutation(ends), rng.integers(0, k, m - len(ends))])


def check_onehot(gemm, oracle, c, cus, seed=0):
    """Activation row a is 1.0 at kappa(a): y[a, r] is the oracle's weight w[r, kappa(a)] bit for bit -- the table of the right (row, group),
    the table buffer's turn, the sub-group index, a split's g0.  Scales, zeros, LUT and codes are random."""
    plan = assert_regime(c, cus)
    P = problem(c, seed + 3)
    j = torch.from_numpy(onehot_columns(c.m, c.k, c.g, plan[3], seed))
    x = torch.zeros(c.m, c.k, dtype=c.dtype)
    x[torch.arange(c.m), j] = 1.0
    y = gemm(vary(P, x=x))[:, :c.n]
    want = (oracle_w(oracle, P)[:, j].t().float() + 0.0).to(c.dtype)     # (a weight of -0, mx4 code 8, among the +0 products: the sum is +0)
    bad = y.view(torch.int16) != want.contiguous().view(torch.int16)
    assert not bad.any(), (f"one-hot probe {case_id(c)}: {int(bad.sum())} / {bad.numel()} outputs differ; (row, weight row) {torch.nonzero(bad)[:4].tolist()}, "
                           f"columns {j[torch.nonzero(bad)[:4, 0]].tolist()}")


def _ident(i, k):
    """(1 + (i % 8) / 8) 2^((i / 8) % 13 - 12): 104 values in a row all different, 4 significant bits, so that k times one is exact in
    8 bits for every k = odd 2^j with odd <= 17 (the tables' k values), and at most 1.875 x 4608 in size."""
    return (1 + (i % 8) / 8) * np.exp2((i // 8) % 13 - 12.0)


def placement_problem(c, which):
    """Weight row r holds one value v_r in every column, activation row a one value c_a, so that y[a, r] = k c_a v_r exactly.  which = "x":
    c_a = _ident(a) names the activation row, v_r = 2^(r % 3); "w": v_r = _ident(r) names the weight row, c_a = 2^(a % 3).  v_r sits in
    the row's LUT (any4 row-wise: all 16 entries) under scale 1, zero 0; int8: code 129 under scale v_r; mx4 (powers of two and 1.5 x):
    code 2 or 3 under exponent 127 + log2."""
    n, k, g, dt = c.wrows, c.k, c.g, c.dtype
    P = problem(c)
    a, r = np.arange(c.m), np.arange(n)
    ca = _ident(a, k) if which == "x" else np.exp2(a % 3)
    if c.qtype == "mx4":
        vr = np.exp2(r % 3) if which == "x" else np.where(r % 2 == 1, 1.5, 1.0) * np.exp2((r // 2) % 13 - 12.0)
        P.codes = torch.from_numpy(np.where(vr / np.exp2(np.floor(np.log2(vr))) == 1.5, 3, 2).astype(np.int32))[:, None].repeat(1, k)
        P.qinfo = torch.from_numpy((127 + np.floor(np.log2(vr))).astype(np.uint8))[:, None].repeat(1, k // 32)
    else:
        vr = np.exp2(r % 3) if which == "x" else _ident(r, k)
        v16 = torch.from_numpy(vr).to(dt)
        P.qinfo = torch.zeros(k // g, n, 2, dtype=dt)
        if c.kind == "w8":
            P.codes = torch.full((n, k), 129, dtype=torch.int32)
            P.qinfo[:, :, 0] = v16[None, :]
        else:
            assert c.qtype == "any4_rowwise"
            P.qinfo[:, :, 0] = 1.0
            P.lut = v16[:, None].repeat(1, 16)
    P.x = torch.from_numpy(ca).to(dt)[:, None].repeat(1, k)
    P.n, P.packed = n, None
    want64 = k * ca[:, None] * vr[None, :]
    want = torch.from_numpy(want64).to(dt)
    assert torch.equal(want.double(), torch.from_numpy(want64)) and torch.equal(P.x.double()[:, 0], torch.from_numpy(ca)), "the placement values are not exact"
    return P, want


def check_placement(gemm, c, cus):
    """Every output of a ragged launch, once with the activation row's name in it and once with the weight row's: the tile -> (n tile,
    split, m tile) mapping, the store's row / column arithmetic, the XCD remap at ntot % 8 != 0."""
    assert_regime(c, cus)
    for which in ("x", "w"):
        P, want = placement_problem(c, which)
        y = gemm(P)
        bad = y.view(torch.int16) != want.view(torch.int16)
        assert not bad.any(), f"placement probe {case_id(c)} ({which}): {int(bad.sum())} / {bad.numel()} outputs differ; (row, weight row) {torch.nonzero(bad)[:4].tolist()}"


def _decoyed(t):
    return (t.float() + DECOY).to(t.dtype)


def check_decoy(gemm, c, cus):
    """+ 2^15 in the scale / zero, LUT (row-wise) and mx4 exponent (+ 15) entries of the padded weight rows, and in the activation rows
    directly behind row m - 1: no bit of the n real columns changes."""
    c = vary(c, n=c.wrows - 3)
    assert_regime(c, cus)
    P = problem(c, seed=4)
    n = c.n
    assert P.wrows > n
    clean = gemm(P)[:, :n].clone()
    q2 = P.qinfo.clone()
    if c.qtype == "mx4":
        q2[n:] = 142
    else:
        q2[:, n:] = _decoyed(torch.randn(q2.shape[0], P.wrows - n, 2).to(c.dtype))
    lut2 = P.lut
    if c.qtype == "any4_rowwise":
        lut2 = P.lut.clone()
        lut2[n:] = DECOY
    assert bits_equal(gemm(vary(P, qinfo=q2, lut=lut2))[:, :n], clean), "a padded weight row's scale / zero / LUT / exponent reached a real column"
    behind = _decoyed(torch.randn(32, c.k, generator=torch.Generator().manual_seed(3)).to(c.dtype))
    assert bits_equal(gemm(vary(P, x_behind=behind))[:, :n], clean), "activation rows >= m reached a stored output"


def check_nonfinite(gemm, oracle, c, cus):
    """One NaN in x[a, col] makes row a NaN; a NaN scale at (group, row) -- mx4: an exponent of 255 -- exactly that column; one inf in x
    appears where the float64 product has it; every other output keeps its bits."""
    c = vary(c, n=c.wrows - 3)
    assert_regime(c, cus)
    P = problem(c, seed=5)
    n, m, k = c.n, c.m, c.k
    clean = gemm(P)[:, :n].clone()
    a_inf, a_nan, r_nan, grp = 1, m - 1, n - 3, (k // c.g) // 2
    x2 = P.x.clone()
    x2[a_inf, (3 * k) // 4 + 1] = float("inf")
    x2[a_nan, k - 1] = float("nan")
    q2 = P.qinfo.clone()
    if c.qtype == "mx4":
        q2[r_nan, grp] = 255
    else:
        q2[grp, r_nan, 0] = float("nan")
    P2 = vary(P, x=x2, qinfo=q2)
    y = gemm(P2)[:, :n]
    with np.errstate(invalid="ignore"):
        y64 = x2.double().numpy() @ oracle_w(oracle, P2).double().numpy().T
    yf = y.float().numpy()
    assert np.array_equal(np.isnan(yf), np.isnan(y64)), "NaN placement differs from the float64 product"
    assert np.array_equal(np.isinf(yf), np.isinf(y64)) and np.array_equal(np.sign(yf[np.isinf(yf)]), np.sign(y64[np.isinf(y64)])), "inf placement differs"
    assert np.isnan(y64[a_nan]).all() and np.isnan(y64[:, r_nan]).all() and np.isinf(y64[a_inf]).any()
    area = np.zeros(y64.shape, bool)
    area[a_inf], area[a_nan], area[:, r_nan] = True, True, True
    touched = ~np.isfinite(y64)
    assert not (touched & ~area).any(), "the probe's own inputs overflow"
    same = (y.view(torch.int16) == clean.view(torch.int16)) | torch.from_numpy(touched)
    assert same.all(), f"{int((~same).sum())} finite outputs changed bits next to a non-finite input"


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin and its mutants (plain torch on the CPU)
# ---------------------------------------------------------------------------------------------------------------------------------

def _round16(acc, dtype, truncate=False):
    y = acc.to(dtype)
    if truncate:   # towards zero: step back where RNE went away from zero
        over = y.float().abs() > acc.abs()
        y = (y.view(torch.int16) - over.to(torch.int16)).view(dtype)
    return y


def _swap_1_8(t):
    """Columns 2Q + 1 and 2Q + 8 (Q = 0 ... 3) of every 16-k tile exchanged."""
    idx = torch.arange(t.shape[1]).view(-1, 16).clone()
    for q in range(4):
        idx[:, [2 * q + 1, 2 * q + 8]] = idx[:, [2 * q + 8, 2 * q + 1]]
    return t[:, idx.reshape(-1)]


# name -> (what it does, the check named for it, the regime it shows in)
MUTANTS = {
    "stale_ring_slot": ("the words of step s >= 4 taken from step s - 4", "select", "more than 4 steps"),
    "last_step_dropped": ("the last step of a split dropped", "select", "any"),
    # (a value mutant: it is DEFINED only where a group spans four steps -- the twin does not model the kernel's build-ahead schedule, so
    # that it changes nothing elsewhere is its definition, not a finding)
    "tables_overwritten_early": ("at 4 steps per group, the next group's tables written over a group before its last step", "onehot", "any"),
    "sub_groups_swapped": ("the g = 32 sub-groups of a step swapped", "onehot", "nsub > 1"),
    "split_scales_from_group_0": ("a split's scales taken from group 0 on", "onehot", "split"),
    "swizzle_without_row_term": ("x chunks without the row term of the swizzle", "select", "any"),
    "last_row_duplicated": ("row m - 1 duplicated into the stored row before it", "placement", "any"),
    "ragged_tile_previous_words": ("the ragged last 8-row tile reading the previous tile's words", "select", "wrows % 16 = 8"),
    "partials_in_16_bit": ("partials summed in 16 bits", "f64", "split"),
    "bias_once_per_split": ("the bias added once per split", "bias", "split"),
    "truncation": ("truncation in place of RNE", "f64", "any"),
    "int8_bytes_in_k_order": ("int8: the bytes of a word taken in k order", "select", "int8"),
}


class Twin:
    """The tile GEMM's schedule in plain torch: per split the f32 partial sums over its own k range, from 16-bit weights made per (row,
    group) as RNE16(f32 lut * scale + zero) (the product is exact in f32: this is the fma); the partials added in split order; ONE RNE
    rounding; the bias added and rounded again.  cus: the CU count it plans for; mutant: a key of MUTANTS, or None."""

    def __init__(self, cus=256, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.cus, self.mutant = cus, mutant

    def weights(self, P, plan):
        mu = self.mutant
        _, _, KS, splits, ksteps, spg, nsub, _ = plan
        k, g, wrows, dt = P.k, P.g, P.wrows, P.dtype
        kl, sw = k // splits, 64 * KS
        col = torch.arange(k)
        split, step = col // kl, (col % kl) // sw
        ccol, gcol = col.clone(), col // g
        if mu == "stale_ring_slot":
            ccol = torch.where(step >= 4, col - 4 * sw, col)
        if mu == "tables_overwritten_early" and spg == 4:
            last_group = (col % kl) // g == kl // g - 1
            gcol = torch.where((step % spg == spg - 1) & ~last_group, gcol + 1, gcol)
        if mu == "sub_groups_swapped" and nsub > 1:
            sub = (col % sw) // g
            gcol = gcol + (nsub - 1 - 2 * sub)
        if mu == "split_scales_from_group_0":
            gcol = gcol - split * (kl // g)
        C = torch.zeros(wrows, k, dtype=torch.int64)
        C[:P.codes.shape[0]] = P.codes
        if mu == "ragged_tile_previous_words" and wrows % 16 == 8 and wrows >= 16:
            C[wrows - 8:] = C[wrows - 16:wrows - 8].clone()
        if mu == "int8_bytes_in_k_order" and P.kind == "w8":
            C = _swap_1_8(C)
        C = C[:, ccol]
        if P.qtype == "mx4":
            e = P.qinfo[:, gcol].float()
            scale = torch.where(e == 255, torch.full_like(e, float("nan")), torch.exp2(e - 127))
            return (torch.tensor(FP4 + [-v for v in FP4])[C & 15] * scale).to(dt)
        sc, z = P.qinfo[:, :, 0].float()[gcol].t(), P.qinfo[:, :, 1].float()[gcol].t()
        if P.kind == "w8":
            v = (C & 255).float() - 128.0
        elif P.qtype == "int4":
            v = (C & 15).float() - 8.0
        elif P.lut.dim() == 1:
            v = P.lut.float()[C & 15]
        else:
            v = torch.gather(P.lut.float(), 1, C & 15)
        return (v * sc + z).to(dt)

    def __call__(self, P, bias=None, workspace=True):
        mu = self.mutant
        plan = tile_plan(P.m, P.wrows, P.k, P.g, P.qtype, self.cus, workspace, P.kind == "w8", P.side == "B", P.dtype)
        assert plan is not None, "the tile GEMM declines this call"
        _, _, KS, splits, ksteps, _, _, _ = plan
        m, k, dt = P.m, P.k, P.dtype
        kl, sw = k // splits, 64 * KS
        wf, xf = self.weights(P, plan).float(), P.x.float()
        col = torch.arange(k)
        if mu == "last_step_dropped":
            xf = xf.clone()
            xf[:, (col % kl) // sw == ksteps - 1] = 0
        if mu == "swizzle_without_row_term":
            chunk = (col % 64) // 8
            f = (torch.arange(m)[:, None] >> 1) & 7
            xf = torch.gather(xf, 1, col[None, :] - 8 * chunk[None, :] + 8 * (chunk[None, :] ^ f))
        acc = torch.zeros(m, P.wrows)
        for s in range(splits):
            part = xf[:, s * kl:(s + 1) * kl] @ wf[:, s * kl:(s + 1) * kl].t()
            acc = (acc + part).to(dt).float() if mu == "partials_in_16_bit" else acc + part
        y = _round16(acc, dt, truncate=(mu == "truncation"))
        if mu == "last_row_duplicated" and m >= 2:
            y[m - 2] = y[m - 1]
        if bias is not None:
            for _ in range(splits if mu == "bias_once_per_split" else 1):
                y = (y.float() + bias.float()).to(dt)
        return y


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes the tile GEMM's tests had before this suite: which of them let a mutant through (profiles/tile_f64_checks.txt)
# ---------------------------------------------------------------------------------------------------------------------------------
OLD_W4_SHAPES = [(65, 200, 512), (128, 64, 64), (130, 1008, 1024), (512, 528, 2048), (33, 200, 2048), (64, 528, 2048), (48, 1008, 4096), (130, 1008, 4096),
                 (256, 2056, 2048), (17, 72, 2048), (20, 4096, 2048)]                                    # test_tile_gemm_many_rows_against_oracle
OLD_W4_FLAVOURS = [("any4_rowwise", 128), ("any4_rowwise", 32), ("int4", 64), ("any4_global", 256)]
OLD_MX4_SHAPES = [(65, 200, 512), (130, 1008, 1024), (512, 528, 2048), (40, 264, 2048), (100, 4096, 4096)]   # test_tile_gemm_many_rows_mx4
OLD_W8_SHAPES = [(17, 200, 512, BF16), (33, 264, 2048, BF16), (64, 4096, 2048, F16), (130, 1008, 4096, BF16), (512, 528, 1024, F16), (100, 48, 192, BF16)]   # test_gemm_int8_many_rows_on_the_tile_gemm
OLD_NO_WORKSPACE = (128, 1008, 4096, 128)                                                                # test_tile_gemm_without_a_workspace: 32 steps unsplit


def old_cases():
    """Every (shape, flavour) the tile GEMM's tests ran before this suite, as (case, workspace): the 11 4-bit shapes at the four (words,
    group) flavours, the mx4 shapes, the int8 shapes at g = 64 / 128 / 256 (words on the right; the left runs the same plan), and the
    128-row call with and without a workspace."""
    mk = lambda kind, qtype, dt, g, m, n, k: SimpleNamespace(kind=kind, qtype=qtype, dtype=dt, side="B", g=g, m=m, wrows=_cdiv(n, 8) * 8, n=n, k=k, want=None)
    out = [(mk("w4", q, BF16, g, m, n, k), True) for m, n, k in OLD_W4_SHAPES for q, g in OLD_W4_FLAVOURS if g <= k]
    out += [(mk("w4", "mx4", BF16, 32, m, n, k), True) for m, n, k in OLD_MX4_SHAPES]
    out += [(mk("w8", "int8", dt, g, m, n, k), True) for m, n, k, dt in OLD_W8_SHAPES for g in (64, 128, 256) if k % g == 0]
    m, n, k, g = OLD_NO_WORKSPACE
    return out + [(mk("w4", "any4_rowwise", BF16, g, m, n, k), ws) for ws in (True, False)]


def old_shape_survivors(oracle, mutants=None, cus=256):
    """{mutant: [(case id, steps per workgroup, steps per group, passed)]}: the mutants under what the earlier tests check -- random data
    under the float64 contract and the fused bias's bits -- at every earlier case (old_cases).  The int8 mutant runs on the int8 cases only."""
    out = {name: [] for name in (mutants or MUTANTS)}
    for c, ws in old_cases():
        plan = plan_of(c, cus, ws)
        P = problem(c)
        w = oracle_w(oracle, P)
        bias = torch.randn(P.wrows, generator=torch.Generator().manual_seed(5)).to(P.dtype)
        for name in out:
            if name == "int8_bytes_in_k_order" and c.kind != "w8":
                continue
            twin = Twin(cus, name)
            y = twin(P, workspace=ws)
            ok = bool((f64_ratio(y[:, :c.n], P.x, w) <= 1).all()) and bits_equal(twin(P, bias=bias, workspace=ws), y + bias)
            out[name].append((case_id(c) + ("" if ws else "-no-workspace"), plan[4], plan[5], ok))
    return out
