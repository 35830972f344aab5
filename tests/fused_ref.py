"""Float64 references, input builders, the dry planner and the case table for the stages fused into the 4-bit GEMM launches
(tg_w4_gemm ABI 5: RMSNorm in the activation staging, the residual add and SwiGLU in the output store).

A plain helper module (not a conftest), in the style of tests/glue_ref.py.  tests/test_fused_ref_cpu.py checks the references, the
3 % condition and the case table against the library's dry planner on the CPU; tests/test_gpu_fused_f64.py runs the table against
the kernels.

Two fused-norm contracts (include/tinygemm_hip.h; GS = oracle.linear_group_scaled, the group-scaled contraction in double):

  "sum"   y = RNE16(rs * GS(x~)),  x~ = RNE16(x g)             w4_gemv_kernel at every m it takes (1 ... 8) and
                                                               w4_gemm_pair16_loop_kernel: 1 / rms multiplies the f32 sum in the store
  "act"   y = RNE16(GS(x')),  x' = RNE16(RNE16(x rs) g)        w4_gemm_pair16_kernel and w4_gemm_pair_kernel (chunk_rmsnorm, w4_helpers.cuh):
                                                               dg_add_rmsnorm's formula in the staging

with rs = rsqrt(mean(x^2) + eps).  Allowances (nothing here is fitted to a kernel's output):

  contract(ref, S) = 0.5 ulp16(ref) (1 + 2^-7) + 4e-6 S       the project's own for the group-scaled kernels (test_gpu_gemv.check),
                                                               S = sum_k |x_k w_k|
  "sum":  contract(ref, S) + 2^-18 S,  S = rs sum|x~ w|.  x~ is unambiguous (the product of two 16-bit values is exact in f32), so no
          per-activation rounding term.  2^-18 is for rs in f32: the kernels add the squares as chained v_dot2 steps per lane (16 in
          w4_gemv_kernel and the pair-table kernels, 32 in the loop kernel), a wave or quad sum (<= 6 steps), 8 or 16 partials, then
          multiply by the f32 1 / k (two roundings when k is no power of two), add eps, rsqrtf: at most 32 + 6 + 16 + 3 = 57
          roundings of 2^-24 each on the sum of squares (every term is positive, so relative errors do not amplify): 3.4e-6, halved by
          the square root, plus rsqrtf's own 2^-23: 1.8e-6, below 2^-19 = 1.9e-6 relative; 2^-18 doubles it.
  "act":  contract(ref, S) + A,  A = |x'(r+) - x'(r-)| @ |W|^T over r- = rs (1 - 2^-18), r+ = rs (1 + 2^-18).  Both roundings are
          monotone in r, so whatever rs the kernel computed inside that interval, each of its activations lies between x'(r-) and
          x'(r+).  The kernel's rs is an f32 number and it forms x rs with one f32 multiply, so the interval's ends are taken as the f32
          numbers just INSIDE it and x'(r) is evaluated with that same f32 multiply: the same monotone function on both sides, no wider
          than the float64 interval.  Condition: at most 3 % of a row's activations differ between the two ends (asserted on the CPU).
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests.conftest import bits16, from_bits16  # noqa: F401  (re-exported for the tests)
from tests.glue_ref import swiglu_ref64, two_roundings_bound
from tests.test_gpu_fast import QT, gs_reference
from tests.test_gpu_parity import oracle_weights, rand_problem, ulp16

RS_REL = 2.0 ** -18       # relative error allowed on the kernels' f32 1 / rms (derived above)
AMBIGUOUS_MAX = 0.03      # "act": share of a row's activations that may differ between the interval's ends
EPS = 1e-5
GUARD_BYTES = 4096
SENTINEL = 0x5A5A         # int16 pattern around `out` (finite in both types)
BF16, F16 = torch.bfloat16, torch.float16


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------

def make_inputs(m, n, k, dtype, seed):
    """The input recipe: x = 3 randn with row a scaled by 2^((a mod 5) - 2) (a neighbouring row's 1 / rms is off by a factor >= 2),
    g = 1 + 0.1 randn, residual = randn [m][n].  CPU tensors of `dtype`."""
    gen = torch.Generator().manual_seed(seed * 7919 + 5)
    x = 3 * torch.randn(m, k, generator=gen) * torch.exp2((torch.arange(m) % 5 - 2).float())[:, None]
    g = 1 + 0.1 * torch.randn(k, generator=gen)
    res = torch.randn(m, n, generator=gen)
    return x.to(dtype), g.to(dtype), res.to(dtype)


def guarded(t, device, fill=float("nan"), extra_cols=0):
    """`t` (a CPU tensor, 1-D or 2-D) inside a larger device allocation: at least GUARD_BYTES of `fill` on each side (int: that int16
    pattern, else the value; NaN by default), and for a 2-D tensor `extra_cols` columns of `fill` behind every row (a view into a wider
    tensor).  Returns (the view with t's values, the whole allocation)."""
    gelems = GUARD_BYTES // 2
    rows, cols = (1, t.numel()) if t.dim() == 1 else t.shape
    whole = torch.empty(2 * gelems + rows * (cols + extra_cols), dtype=t.dtype, device=device)
    if isinstance(fill, int):
        whole.view(torch.int16).fill_(fill if fill < 0x8000 else fill - 0x10000)
    else:
        whole.fill_(fill)
    view = whole[gelems:gelems + rows * (cols + extra_cols)].view(rows, cols + extra_cols)[:, :cols]
    view.copy_(t.view(rows, cols))
    return (view.reshape(-1) if t.dim() == 1 and not extra_cols else view), whole


def guard_intact(view, whole, fill=SENTINEL):
    """Everything of `whole` outside `view` (a contiguous view made by `guarded`) still holds the int16 pattern `fill`."""
    gelems = GUARD_BYTES // 2
    w = whole.view(torch.int16)
    pat = fill if fill < 0x8000 else fill - 0x10000
    return bool((w[:gelems] == pat).all()) and bool((w[gelems + view.numel():] == pat).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------

def rs64(x16, eps=EPS):
    """rsqrt(mean(x^2) + eps) per activation row in float64 (eps as the f32 number the struct carries)."""
    x = x16.double()
    return torch.rsqrt((x * x).mean(dim=1) + float(np.float32(eps)))


def mul16(a16, b16):
    """RNE16(a b) of two 16-bit tensors: the product is exact in f32 for both types, so this is ONE rounding."""
    return (a16.float() * b16.float()).to(a16.dtype)


def _f32_inside(v64, up):
    """The f32 number nearest to v64 on the side `up` says (up: >= v64, else <= v64)."""
    v64 = np.asarray(v64, np.float64)
    v32 = v64.astype(np.float32)
    wrong = (v32.astype(np.float64) < v64) if up else (v32.astype(np.float64) > v64)
    return np.where(wrong, np.nextafter(v32, np.float32(np.inf if up else -np.inf)), v32).astype(np.float32)


def act_norm16(x16, g16, r32):
    """x'(r) = RNE16(RNE16(x r) g) with r an f32 per row: x r is one f32 multiply, as chunk_rmsnorm forms it."""
    r = torch.from_numpy(np.ascontiguousarray(r32, np.float32))[:, None]
    return mul16((x16.float() * r).to(x16.dtype), g16[None, :].expand_as(x16))


def act_norm_bracket(x16, g16, eps=EPS):
    """(x'(rs), x'(r-), x'(r+), share): the "act" activations at the f32 nearest to rs and at the f32 ends just inside
    rs (1 -+ RS_REL), and per row the share of activations that differ between the two ends."""
    rs = rs64(x16, eps).numpy()
    mid = act_norm16(x16, g16, rs.astype(np.float32))
    lo = act_norm16(x16, g16, _f32_inside(rs * (1 - RS_REL), up=True))
    hi = act_norm16(x16, g16, _f32_inside(rs * (1 + RS_REL), up=False))
    share = (bits16(lo) != bits16(hi)).mean(axis=1)
    return mid, lo, hi, share


def contract(ref, S, dtype):
    """The project's allowance for a group-scaled kernel against oracle.linear_group_scaled (test_gpu_gemv.check)."""
    return 0.5 * ulp16(ref, dtype) * (1 + 2.0 ** -7) + 4e-6 * S + 1e-37


def _abs_w64(oracle, L, rows):
    sel = slice(None) if rows is None else torch.from_numpy(rows)
    codes, qinfo = L.codes[sel], (L.qinfo[sel] if L.qtype == "mx4" else L.qinfo[:, sel]).contiguous()
    lut = L.lut if L.lut is None or L.lut.dim() == 1 else L.lut[sel].contiguous()
    w = from_bits16(oracle_weights(oracle, codes, L.g, L.qtype, qinfo, lut, L.dtype), L.dtype).double().abs()
    return codes, qinfo, lut, w


def norm_gemv_ref(oracle, L, x16, g16, eps=EPS, rows=None):
    """The "sum" contract for layer L (see `layer`) on the weight rows `rows` (None: all): (ref, allowance) as float64 numpy [m][rows]."""
    codes, qinfo, lut, wabs = _abs_w64(oracle, L, rows)
    xt = mul16(x16, g16[None, :].expand_as(x16))
    rs = rs64(x16, eps).numpy()[:, None]
    ref = rs * gs_reference(oracle, codes, xt, qinfo, lut, L.g, L.qtype, L.dtype)
    S = rs * (xt.double().abs() @ wabs.t()).numpy()
    return ref, contract(ref, S, L.dtype) + RS_REL * S


def norm_pair_ref(oracle, L, x16, g16, eps=EPS, rows=None):
    """The "act" contract: (ref, allowance, share) with share the per-row ambiguous share of the activations."""
    codes, qinfo, lut, wabs = _abs_w64(oracle, L, rows)
    mid, lo, hi, share = act_norm_bracket(x16, g16, eps)
    ref = gs_reference(oracle, codes, mid, qinfo, lut, L.g, L.qtype, L.dtype)
    S = (mid.double().abs() @ wabs.t()).numpy()
    A = ((hi.double() - lo.double()).abs() @ wabs.t()).numpy()
    return ref, contract(ref, S, L.dtype) + A, share


def plain_ref(oracle, L, x16, rows=None):
    """No norm: the group-scaled kernels' own contract."""
    codes, qinfo, lut, wabs = _abs_w64(oracle, L, rows)
    ref = gs_reference(oracle, codes, x16, qinfo, lut, L.g, L.qtype, L.dtype)
    return ref, contract(ref, (x16.double().abs() @ wabs.t()).numpy(), L.dtype)


def norm_ref(oracle, L, x16, g16, formula, eps=EPS, rows=None):
    """(ref, allowance) under the contract `formula` names ("sum" / "act")."""
    if formula == "sum":
        return norm_gemv_ref(oracle, L, x16, g16, eps, rows)
    ref, tol, share = norm_pair_ref(oracle, L, x16, g16, eps, rows)
    assert share.max() <= AMBIGUOUS_MAX or (x16 != 0).sum(dim=1).max() <= 1, share.max()  # (one-hot probes: one activation per row)
    return ref, tol


def swiglu_of_sums(ref, tol, dtype):
    """The SwiGLU store on top of GEMM sums known to ref +- tol (rows in blocks of 8 gate + 8 up): (y_ref, allowance) [m][n / 2].
    The kernel computes RNE16(RNE16(silu(g16)) u16) from g16 / u16 = RNE16(sum) (tol already holds that rounding).  With
    |silu'| <= 1.1 everywhere and |silu(g)| <= |g|:  |silu(g) u - silu(g0) u0| <= 1.1 dg (|u0| + du) + |silu(g0)| du, and the two
    roundings of the store add glue_ref.two_roundings_bound of the (largest possible) result."""
    m, n = ref.shape
    r, t = ref.reshape(m, n // 16, 2, 8), tol.reshape(m, n // 16, 2, 8)
    g0, u0, dg, du = (torch.from_numpy(np.ascontiguousarray(a.reshape(m, n // 2))) for a in (r[:, :, 0], r[:, :, 1], t[:, :, 0], t[:, :, 1]))
    silu = g0 / (1.0 + torch.exp(-g0))
    y0 = swiglu_ref64(torch.cat([g0, u0], dim=1))
    prop = 1.1 * dg * (u0.abs() + du) + silu.abs() * du
    return y0.numpy(), (prop + two_roundings_bound(y0.abs() + prop, dtype)).numpy()


def split_gate_up(gu):
    """[m][n] GEMM output with rows in blocks of 8 gate + 8 up -> [gate | up] as decode_ops.swiglu takes it."""
    m = gu.shape[0]
    return gu.view(m, -1, 2, 8).transpose(1, 2).reshape(m, -1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# layers (weights of one case; shared by the cases of the same shape)
# ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def layer(n, k, g, qtype, dtype, seed=0):
    """rand_problem's weights for one layer (CPU): codes [n][k], qinfo, lut."""
    codes, _, qinfo, lut = rand_problem(n, k, g, 1, qtype, dtype=dtype, seed=seed + n + k + g)
    return SimpleNamespace(n=n, k=k, g=g, qtype=qtype, dtype=dtype, codes=codes, qinfo=qinfo, lut=lut)


# ---------------------------------------------------------------------------------------------------------------------------------
# the dry planner
# ---------------------------------------------------------------------------------------------------------------------------------

def fused_plan(m, n, k, g, qtype, dtype=BF16, inner=4, *, norm_weight=False, epilogue=0, bias=False, bias_row_stride=0, batch=1,
               numerics="fast"):
    """The kernel family tg_gemm_w4_plan names for the call ops.w4_linear_fused would make (dummy pointers as ops.gemm_w4_plan: nothing
    is dereferenced, no GPU needed; dry plans assume 256 CUs), or None where the library answers TG_E_FUSION."""
    from any4_amd import _lib, ops

    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63
    args = _lib.W4Gemm(x=p, w=p, qinfo=p, lut=(p if qtype.startswith("any4") else None), y=p, m=m, wrows=n, k=k, group=g, qtype=QT[qtype],
                       dtype=_lib.TG_BF16 if dtype == BF16 else _lib.TG_F16, w_on_right=1, inner_k_tiles=inner, batch=batch,
                       stride_x=16, stride_w=16, stride_qinfo=16, stride_lut=16, stride_y=16, stride_bias=16 if bias else 0,
                       numerics=ops._NUMERICS[numerics], bias=(p if bias else None), bias_row_stride=bias_row_stride,
                       norm_weight=(p if norm_weight else None), norm_eps=EPS, epilogue=epilogue)
    need = ops._L.tg_gemm_w4_workspace_bytes(ctypes.byref(args))
    if need == _lib.TG_E_FUSION:
        return None
    _lib.check(need if need < 0 else 0, "tg_gemm_w4_workspace_bytes")
    if need > 0:
        args.workspace, args.workspace_bytes = p, need
    rc = ops._L.tg_gemm_w4_plan(ctypes.byref(args), 0)
    if rc == _lib.TG_E_FUSION:
        return None
    _lib.check(rc if rc < 0 else 0, "tg_gemm_w4_plan")
    return ops._PLANS[rc].split("_")[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------
# kernel: the carrier read from the launch paths (tg_gemv.hip, tg_pair16.hip, tg_pair.hip); the planner names the family only
# ("gemv", or "pair" for every pair-table kernel), the formula follows the kernel.
FAMILY = {"gemv": "gemv", "pair16": "pair", "pair16_loop": "pair", "pair": "pair"}
FORMULA = {"gemv": "sum", "pair16_loop": "sum", "pair16": "act", "pair": "act"}


def Case(kernel, m, n, k, g, qtype="any4_rowwise", dtype=BF16, inner=4, numerics="fast", swiglu=False, sample=False, what=""):
    return SimpleNamespace(kernel=kernel, m=m, n=n, k=k, g=g, qtype=qtype, dtype=dtype, inner=inner, numerics=numerics, swiglu=swiglu,
                           sample=sample, what=what, family=FAMILY[kernel], formula=FORMULA[kernel])


def case_id(c):
    return (f"{c.kernel}-m{c.m}-n{c.n}-k{c.k}-g{c.g}-{c.qtype}-{'bf16' if c.dtype == BF16 else 'fp16'}" + (f"-i{c.inner}" if c.inner != 4 else "")
            + (f"-{c.numerics}" if c.numerics != "fast" else "") + ("-swiglu" if c.swiglu else ""))


def _norm_cases():
    out = []
    for dt in (BF16, F16):
        # w4_gemv_kernel, v_dot2 contraction (MF = 0): g = 32 (GPS = 2) / 64, M = 1 ... 4; 129 tiles: one tile per workgroup, 129 workgroups
        for g in (32, 64):
            for qt in ("any4_rowwise", "int4"):
                out += [Case("gemv", m, 1032, 2048, g, qt, dt, what="v_dot2") for m in (1, 2, 3, 4)]
        # ... matrix-core contraction (MF = 1): g = 128 / 256 (a global LUT at 256), M up to 8; m = 8 at k = 2048 / 4096: chunk staging
        for g, qt in ((128, "any4_rowwise"), (256, "any4_global")):
            for k in (2048, 4096):
                out += [Case("gemv", m, 1032, k, g, qt, dt, what="matrix core") for m in (1, 3, 4, 5, 8)]
        out += [Case("gemv", m, 1032, 8192, 128, "any4_rowwise", dt, what="ring of 8 (D = 8)") for m in (1, 4)]
        # ... 1281 tiles: ranges of 5 and 6 tiles, three 16-row passes, the LUT rows of the later passes staged through LDS
        out += [Case("gemv", m, 10248, 2048, 128, "any4_rowwise", dt, what="several passes") for m in (1, 4)]
        # w4_gemm_pair16_kernel<NORM>: what gemv declines (g = 32 / 64 above 4 rows, any g above 8 rows), one and 65 workgroups
        for n in (16, 1032):
            out += [Case("pair16", m, n, 2048, g, "any4_rowwise", dt) for g in (32, 64) for m in (5, 8)]
            out += [Case("pair16", m, n, 2048, g, "int4" if g == 256 else "any4_rowwise", dt) for g in (32, 64, 128, 256) for m in (9, 16)]
        out += [Case("pair16", m, 1032, 2048, 128, "any4_rowwise", dt, inner=2, what="innerKTiles 2") for m in (1, 16)]
        out += [Case("pair16", m, 1032, 4096, 64, "any4_rowwise", dt) for m in (5, 8)]
        # ... below 5 rows: TG_NUM_FAST_MFMA skips the gemv kernel
        out += [Case("pair16", m, 1032, 2048, 128, "any4_rowwise", dt, numerics="fast_mfma") for m in (1, 4)]
        # w4_gemm_pair16_loop_kernel<NORM>: k = 4096, more 16-row tiles than CUs (257: one workgroup with two; 385: 129 with two);
        # 5 rows at g = 128 / 256 stay on the gemv kernel (matrix core, up to 8 rows) -- the same contract either way
        for n in (4112, 6160):
            for g, qt in ((64, "any4_rowwise"), (128, "any4_rowwise"), (256, "any4_global")):
                out += [Case("gemv" if m == 5 and g >= 128 else "pair16_loop", m, n, 4096, g, qt, dt) for m in (5, 9, 16)]
    # two workgroups per CU, 7 SwiGLU units per CU dealt 5 + 2 (TG_GEMV_WG2_EXTRA): the smallest layer that gets there; a row sample
    out.append(Case("gemv", 1, 28672, 4096, 128, "any4_rowwise", BF16, swiglu=True, sample=True, what="two workgroups per CU, 5 + 2"))
    return out


NORM_CASES = _norm_cases()

# (what, m, n, k, g, qtype, dtype, inner, norm, swiglu, the line that refuses it)
REFUSED = [
    ("mx4 with a norm", 1, 1040, 2048, 32, "mx4", BF16, 4, True, False, "tg_pair16.hip launch_pair16: p.norm_w && QMX"),
    ("mx4 with a norm, 16 rows", 16, 1040, 2048, 32, "mx4", BF16, 4, True, False, "tg_pair16.hip launch_pair16: p.norm_w && QMX"),
    ("m k > 32768 on the 16-row kernel", 9, 512, 4096, 128, "any4_rowwise", BF16, 4, True, False, "tg_pair16.hip launch_pair16: m * k > 32768"),
    ("innerKTiles 8 with a norm", 1, 1040, 2048, 128, "any4_rowwise", BF16, 8, True, False, "tg_pair16.hip tgx::pair16: pick<2, 4>(p.inner)"),
    ("innerKTiles 8 with SwiGLU", 1, 1040, 2048, 128, "any4_rowwise", BF16, 8, False, True, "tg_pair16.hip tgx::pair16: pick<2, 4>(p.inner)"),
    ("the loop kernel's shape at g = 32 with a norm", 9, 4112, 4096, 32, "any4_rowwise", BF16, 4, True, False,
     "tg_pair16.hip launch_pair16_loop: p.norm_w && p.gshift == 5 (then launch_pair16: m * k > 32768)"),
    ("k = 3072 with a norm", 1, 1040, 3072, 128, "any4_rowwise", BF16, 4, True, False, "tinygemm_hip.hip check_gemm: k % 2048"),
]

# SwiGLU / residual composition: every carrier, both dtypes (n a multiple of 16: whole gate / up blocks).  The SwiGLU launch deals
# tile PAIRS, so its ranges are not the plain launch's; its bits are those of dg_swiglu on the plain launch's output where both add a
# row's partial sums in the same order -- w4_gemv_kernel's v_dot2 contraction does so for equal rows per pass (tg_gemv.hip, gp.P: 8 for
# one-tile ranges, else 16), hence 258 tiles there: two-tile ranges in the plain launch, one pair per workgroup with SwiGLU.
STAGE_CASES = [c for dt in (BF16, F16) for c in (
    Case("gemv", 2, 2064, 2048, 64, "int4", dt, what="v_dot2"),
    Case("gemv", 5, 1040, 4096, 128, "any4_rowwise", dt, what="matrix core"),
    Case("gemv", 1, 10256, 2048, 128, "any4_rowwise", dt, what="several passes, ranges of 2 and 3 SwiGLU units"),
    Case("pair16", 9, 1040, 2048, 128, "any4_rowwise", dt),
    Case("pair16", 4, 1040, 2048, 128, "any4_global", dt, numerics="fast_mfma"),
    Case("pair16_loop", 9, 4112, 4096, 128, "any4_rowwise", dt),
)]


def sample_rows(n):
    """The row sample of the one case too large for a float64 weight matrix: the first and last 160 rows and every row of every 37th
    8-row tile (whole 16-row gate / up blocks: a tile's partner tile comes along)."""
    tiles = np.unique(np.concatenate([np.arange(20), np.arange(n // 8 - 20, n // 8), np.arange(0, n // 8, 37)]))
    tiles = np.unique(np.concatenate([tiles, tiles ^ 1]))
    return (tiles[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)


def distinct_values(n, dtype, seed=0):
    """n distinct finite non-zero 16-bit values of both signs, in a scrambled order (neighbouring rows differ by far more than a
    rounding): magnitudes from 2^-60 (bf16) / 2^-8 (fp16) upwards, as few binades as n needs."""
    first = (127 - 60) * 128 if dtype == BF16 else (15 - 8) * 1024        # bit pattern of the smallest magnitude
    half = -(-n // 2)
    assert half <= (120 * 128 if dtype == BF16 else 16 * 1024), "not enough distinct values"
    mag = first + np.arange(half)
    bits = np.concatenate([mag, mag | 0x8000])[:n].astype(np.uint16)
    perm = np.random.default_rng(seed).permutation(n)
    return from_bits16(bits[perm], dtype)
