"""Case tables and float64 references of the two gradient GEMMs (tg_gemm_w4_dx: w4_gemm_dx.cuh / tg_dx.hip; tg_gemm_w4_dq: w4_gemm_dq.cuh /
tg_dq.hip).  A plain helper module (not a conftest), in the style of tests/lora_ref.py and tests/moe_ref.py: tests/test_dx_cpu.py and
tests/test_dq_cpu.py confirm the regimes the tables claim against the library (no GPU), tests/test_gpu_dx.py and tests/test_gpu_dq.py run
the kernels at them.

dx.  The launch splits the 64-row steps over the weight rows when the (m x k) tiles are few (tg_dx.hip).  Which regime a problem runs is
read from the library, never restated here: tg_gemm_w4_dx_workspace_bytes answers splits * m * k * 4, or 0 for an unsplit launch
(dx_splits).  A row of DX_SPLIT_CASES CLAIMS its regime -- tile counts, steps, splits, steps of every split, rows of the last step -- and
the CPU tests hold the claims to the library's answer and to plain arithmetic on wrows.

  bound     the project's GEMM bound, unchanged (test_gpu_parity.assert_gemm_close): 0.5 ulp16(want) (1 + 2^-7) + 4e-6 S + 1e-37,
            S = sum_r |dY[a][r] w[r][j]|, want = the float64 contraction of the 16-bit dY with the oracle's dequantised 16-bit weights.
            gemm_err_over_tol reports the largest err / tol under the same formula (a figure to print; the assertion stays
            assert_gemm_close's).
  identity  dY = I (m = wrows): every product is 1 w or 0 w and every f32 sum has at most one non-zero term, so dX is the dequantised
            weight matrix bit for bit in any summation order, split or not (-0 becomes +0: the accumulators start at +0).

dq.  dq_reference is the float64 evaluation of DESIGN section 14 (select by code, then sum); DQ_CASES claims the (row x k) tile counts
and the 64-row activation steps of each case.
"""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from tests.conftest import from_bits16
from tests.test_gpu_parity import ulp16

BF16, F16 = torch.bfloat16, torch.float16
DX_BK, DX_BR = 128, 64            # columns of dX per workgroup, weight rows per step (w4_gemm_dx.cuh)
DQ_BR, DQ_BK, DQ_BA = 128, 128, 64  # weight rows / columns of k per workgroup, activation rows per step (w4_gemm_dq.cuh)


def cdiv(a, b):
    return -(-a // b)


def _qtype_id(qtype):
    from any4_amd import _lib

    return {"int4": _lib.TG_Q_INT4, "any4_global": _lib.TG_Q_ANY4_GLOBAL, "any4_rowwise": _lib.TG_Q_ANY4_ROWWISE, "mx4": _lib.TG_Q_MX4}[qtype]


def w4_args(m, wrows, k, g, qtype, dtype, on_right, inner, **kw):
    """(W4Gemm, keep-alive buffer) of a valid problem with aligned dummy pointers (never dereferenced: the size queries need no GPU).
    Weights on the left: the native words (TG_WFMT_ROWS), `inner` is then the innerKTiles of their Bint4 order (ops._rows_inner)."""
    from any4_amd import _lib

    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 63) & ~63
    a = dict(x=p, w=p, qinfo=p, lut=(p if qtype.startswith("any4") else None), y=p, m=m, wrows=wrows, k=k, group=g, qtype=_qtype_id(qtype),
             dtype=_lib.TG_BF16 if dtype == BF16 else _lib.TG_F16, w_on_right=1 if on_right else 0, inner_k_tiles=inner, batch=1,
             w_format=_lib.TG_WFMT_M16N8K16 if on_right else _lib.TG_WFMT_ROWS)
    a.update(kw)
    return _lib.W4Gemm(**a), buf


def words_inner(k, on_right, inner):
    """innerKTiles of the packed words the kernels walk: the caller's on the right; on the left the native tensor's own (the convert op's
    innerKTiles argument only has to divide k there)."""
    from any4_amd import ops

    return inner if on_right else ops._rows_inner(k)


def dx_splits(m, wrows, k, g=32, qtype="int4", dtype=BF16, on_right=True, inner=2):
    """How many ways tg_gemm_w4_dx splits the weight rows of this problem when it is given its workspace: the library's own answer."""
    from any4_amd import _lib

    args, _buf = w4_args(m, wrows, k, g, qtype, dtype, on_right, words_inner(k, on_right, inner))
    need = _lib.load().tg_gemm_w4_dx_workspace_bytes(ctypes.byref(args))
    assert need >= 0 and need % (4 * m * k) == 0, need
    return need // (4 * m * k) or 1


def dq_workspace_bytes(m, wrows, k, g, qtype, dtype, on_right, inner):
    from any4_amd import _lib

    args, _buf = w4_args(m, wrows, k, g, qtype, dtype, on_right, words_inner(k, on_right, inner), y=None)
    return _lib.load().tg_gemm_w4_dq_workspace_bytes(ctypes.byref(args))


class Run(NamedTuple):
    """One launch of a case: weight kind, group, dtype, side and the innerKTiles handed to the convert op."""
    qtype: str
    g: int
    dtype: torch.dtype
    on_right: bool
    inner: int


class DxCase(NamedTuple):
    m: int
    wrows: int               # weights on the right
    wrows_left: int          # weights on the left: the nearest multiple of 16 with the same step count
    k: int
    bm: int                  # rows of dY per workgroup: 32 / 64 / 128 for m <= 32 / <= 64 / more
    tiles: tuple             # (m tiles, k tiles)
    steps: int               # 64-row steps over the weight rows
    splits: int
    sps: int                 # steps per split
    split_steps: tuple       # steps of every split: the short ones and the empty ones
    last_step_rows: int      # rows of the last step (weights on the right)
    last_k_cols: int         # columns of the last 128-column tile
    runs: tuple
    reaches: str


# Every qtype meets a split, on both dtypes (mx4: bf16 only), on both sides, at every innerKTiles the shape allows (k = 2080: 2 only).
DX_SPLIT_CASES = (
    DxCase(40, 712, 720, 256, 64, (1, 2), 12, 2, 6, (6, 6), 8, 128,
           (Run("int4", 32, F16, True, 2), Run("any4_global", 64, BF16, True, 4), Run("any4_rowwise", 128, F16, True, 8),
            Run("mx4", 32, BF16, False, 4)),
           "2 splits; BM 64; last step has 8 rows"),
    DxCase(33, 1032, 1040, 384, 64, (1, 3), 17, 4, 5, (5, 5, 5, 2), 8, 128,
           (Run("any4_rowwise", 32, BF16, True, 2), Run("mx4", 32, BF16, True, 4), Run("int4", 128, BF16, True, 8),
            Run("any4_global", 64, F16, False, 2)),
           "4 splits by the step limit; last split has 2 steps, the last of them 8 rows"),
    DxCase(130, 2112, 2112, 2080, 128, (2, 17), 33, 4, 9, (9, 9, 9, 6), 64, 32,
           (Run("any4_rowwise", 32, F16, True, 2), Run("mx4", 32, BF16, True, 2), Run("int4", 32, BF16, False, 1)),
           "4 splits by the tile limit; second row tile has 2 rows; last k tile has 32 columns; last split has 6 steps"),
    DxCase(16, 2112, 2112, 1024, 32, (1, 8), 33, 8, 5, (5, 5, 5, 5, 5, 5, 3, 0), 64, 128,
           (Run("any4_global", 32, F16, True, 2), Run("any4_rowwise", 256, BF16, True, 4), Run("mx4", 32, BF16, True, 8),
            Run("int4", 128, F16, False, 4)),
           "split 6 has 3 steps, split 7 has none"),
    DxCase(7, 4160, 4160, 128, 32, (1, 1), 65, 16, 5, (5,) * 13 + (0, 0, 0), 64, 128,
           (Run("mx4", 32, BF16, True, 2), Run("int4", 64, BF16, True, 4), Run("any4_global", 128, BF16, True, 8),
            Run("any4_rowwise", 32, BF16, False, 1)),
           "16 splits; splits 13, 14 and 15 have none"),
)

DX_SPLIT_RUNS = tuple((c, r) for c in DX_SPLIT_CASES for r in c.runs)


def dx_run_id(cr):
    c, r = cr
    return f"m{c.m}-r{c.wrows if r.on_right else c.wrows_left}-k{c.k}-{r.qtype}-g{r.g}-{'bf16' if r.dtype == BF16 else 'f16'}-{'R' if r.on_right else 'L'}{r.inner}"


def split_steps(steps, splits):
    """steps of every split when `steps` are dealt ceil(steps / splits) at a time"""
    sps = cdiv(steps, splits)
    return tuple(max(0, min(steps, (z + 1) * sps) - z * sps) for z in range(splits))


def dx_inner_and_split_shapes(inner):
    """The two problems of test_gpu_dx.test_dx_inner_and_split as (n, k, g, m, qtype, dtype, on_right, inner): many weight rows under
    few (m x k) tiles, so that the launch splits when it has its workspace (test_dx_cpu confirms it does)."""
    return ((2048, 1024, 128, 16, "int4", BF16, True, inner),
            (2048, 96 if inner == 2 else 1024, 32, 16, "any4_global", F16, True, inner if inner == 2 else 4))


# The identity probes: (wrows = m, k, splits).  Small: every word map; large: through a 4-way split of 17 x 2 tiles and 33 steps.
DX_IDENTITY_SMALL = (208, 512, 1)
DX_IDENTITY_LARGE = (2112, 256, 4)
# The non-finite dY probe: the 4-split case; row 32 is the last real row of a BM = 64 tile, r0 lies in the ragged last step.
DX_NONFINITE = dict(m=33, wrows=1032, k=384, splits=4, row=32, r0=1029)


def gemm_err_over_tol(got, x, w_bits, dtype=BF16):
    """largest |got - want| / tol under assert_gemm_close's bound (x [m][rows] 16-bit cpu, w_bits [cols][rows] uint16 bits)"""
    w = from_bits16(w_bits, dtype).double()
    x64 = x.double().cpu()
    want = (x64 @ w.t()).numpy()
    S = (x64.abs() @ w.abs().t()).numpy()
    tol = 0.5 * ulp16(want, dtype) * (1 + 2.0 ** -7) + 4e-6 * S + 1e-37
    return float((np.abs(got.detach().double().cpu().numpy() - want) / tol).max())


# ------------------------------------------------------------------------------------------------
# dq
# ------------------------------------------------------------------------------------------------

def _lut_rows(lut, n, dtype64=torch.float64):
    """the table of every row as [n][16] float64 (int4: code - 8; a global table: repeated)"""
    if lut is None:
        return (torch.arange(16, dtype=dtype64) - 8).expand(n, 16)
    lut = lut.detach().cpu().to(dtype64)
    return lut.expand(n, 16) if lut.dim() == 1 else lut


def dq_reference(codes, x, dy, qinfo, lut, g):
    """(d_qinfo [k/g][n][2], d_lut [n][16] / [16] / None) and the matching sums of absolute values, float64"""
    n, k = codes.shape
    x64, dy64 = x.detach().cpu().double(), dy.detach().cpu().double()
    onehot = torch.nn.functional.one_hot(codes.long(), 16).double().view(n, k // g, g, 16)
    lt = _lut_rows(lut, n)
    s = qinfo.detach().cpu()[..., 0].double().t()   # [n][k/g]
    out = []
    for G, l, sc in ((dy64.t() @ x64, lt, s), (dy64.abs().t() @ x64.abs(), lt.abs(), s.abs())):
        H = (G.view(n, k // g, g, 1) * onehot).sum(2)   # [n][k/g][16]
        dz = H.sum(2)
        ds = (H * l[:, None, :]).sum(2)
        dq = torch.stack([ds.t(), dz.t()], 2)            # [k/g][n][2]
        dl = (H * sc[:, :, None]).sum(1)                 # [n][16]
        if lut is None:
            dl = None
        elif lut.dim() == 1:
            dl = dl.sum(0)
        out.append((dq, dl))
    return out


class DqCase(NamedTuple):
    wrows: int
    k: int
    g: int
    m: int
    qtype: str
    dtype: torch.dtype
    on_right: bool
    inner: int
    tiles: tuple      # (row tiles, k tiles) of 128 x 128
    steps: int        # 64-row steps over the activation rows
    reaches: str


DQ_CASES = (
    DqCase(208, 160, 32, 65, "any4_rowwise", BF16, True, 2, (2, 2), 2, "two k tiles, the second 32 columns wide; m = 65: a step of one row"),
    DqCase(208, 160, 32, 63, "int4", F16, False, 1, (2, 2), 1, "the same k on the left (native words of k % 64 != 0); m = 63"),
    DqCase(200, 416, 32, 64, "any4_global", F16, True, 2, (2, 4), 1, "four k tiles, the last 32 wide; m = 64: one full step"),
    DqCase(208, 416, 32, 129, "any4_rowwise", BF16, False, 2, (2, 4), 3, "the same k on the left; m = 129: two steps and one row"),
    DqCase(136, 768, 256, 65, "any4_rowwise", F16, True, 4, (2, 6), 2, "three groups of 256, each in two halves over six tiles"),
    DqCase(144, 768, 256, 64, "int4", BF16, False, 4, (2, 6), 1, "the same groups on the left"),
    DqCase(264, 256, 64, 63, "any4_rowwise", BF16, True, 8, (3, 2), 1, "three row tiles, the last with 8 rows"),
    DqCase(264, 384, 128, 129, "int4", F16, True, 4, (3, 3), 3, "three row tiles, the last with 8 rows; three steps"),
    DqCase(272, 256, 64, 65, "any4_global", BF16, False, 2, (3, 2), 2, "three row tiles on the left, the last with 16 rows"),
    DqCase(2056, 128, 64, 65, "any4_global", BF16, True, 4, (17, 1), 2, "17 row tiles; the row sum's 16 chains have 129 and 128 rows"),
    DqCase(2056, 128, 32, 129, "any4_global", F16, True, 2, (17, 1), 3, "the same rows, fp16"),
)


def dq_case_id(c):
    return f"r{c.wrows}-k{c.k}-g{c.g}-m{c.m}-{c.qtype}-{'bf16' if c.dtype == BF16 else 'f16'}-{'R' if c.on_right else 'L'}{c.inner}"


# The non-finite probes of dq: any4 row-wise; r0 is the last row of a ragged row tile, row 64 the last activation row, alone in its step,
# column 159 the last column of the ragged k tile.
DQ_NONFINITE = dict(wrows=200, k=160, g=32, m=65, r0=199, a0=64, j0=159)
