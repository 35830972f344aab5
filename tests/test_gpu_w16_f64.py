"""GPU suite (-m gpu): the two 16-row kernels behind the 16-bit-weight and int8-weight ops -- f16_gemm_kernel (tg_gemm_f16, the
*_w_f16TC ops) and w8_gemm_kernel (the 16-row path of tg_gemm_w8) -- under the contract the 4-bit GEMMs have, at the smallest shapes
that reach every regime of their loops and launch geometry (tests/w16_ref.py states the contract, the regimes and the case tables;
tests/test_w16_ref_cpu.py proves on the CPU that the checks pass a correct twin and fail every mutant):

  1  the float64 bound on random data: every nw class of the 16-bit kernel's ring (idle waves, ragged waves below one ring, refills in
     the remainder, one steady round, steady rounds with ragged waves, k = 4096, k = 14336) on B layout innerKTiles 1 / 2 and A layout,
     both dtypes, fp16 subnormal outputs, the TC-layout ops; split-K 1 / 2 / 4 / 8 of launch_w8 with ragged last workgroups
  2  selection probes (exact): one 1.0 per weight row over every column class mod 1024 and both end steps; one-hot activation rows
  3  decoys: + 2^15 in activation rows >= m and in the padded weight rows' scales / zeros changes no bit
  4  non-finite placement: inf / NaN in x, a NaN weight: isnan / isinf as the float64 product, every other output keeps its bits
  5  tg_gemm_f16's output guard, its rejected calls and the op's clone path
  6  determinism and graph capture

Figures of one run on an MI355X (worst |y - y64| / allowance per test, wall time): profiles/w16_f64_checks.txt.
"""
import os

import pytest
import torch

from tests import w16_ref as R
from tests.test_gpu_parity import DEV, T  # noqa: F401  (T is a fixture)

pytestmark = pytest.mark.gpu

RESULTS = []  # (case id, worst |y - y64| / allowance): written to $W16_F64_REPORT when the module is done (profiles/w16_f64_checks.txt)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("W16_F64_REPORT")
    if path:
        with open(path, "w") as f:
            for cid, ratio in RESULTS:
                f.write(f"gpu  {cid:50s} {ratio:.3f}\n")


class OpF16:
    """tinygemm_y_f16RM_x_f16RM_w_f16TC behind w16_ref's gemm(x, w) / gemm(x, w, out=y): side "B" (weights on the right, innerKTiles
    1 / 2) or "A" (left, innerKTiles 1).  out: straight through the C ABI (any4_amd._lib), the op has no out argument."""

    def __init__(self, side, inner):
        self.side, self.inner, self.pad = side, inner, (8 if side == "B" else 16)

    def pack(self, w):
        t = torch.ops.tinygemm
        return t.convert_matrix_to_m16n8k16_B_layout(w, self.inner) if self.side == "B" else t.convert_matrix_to_m16n8k16_A_layout(w, 1)

    def run(self, x, wp):
        t = torch.ops.tinygemm
        return t.tinygemm_y_f16RM_x_f16RM_w_f16TC(x, wp, True) if self.side == "B" else t.tinygemm_y_f16RM_x_f16RM_w_f16TC(wp, x, False)

    def raw(self, x, wp, out, m, wrows, k, inner=None, w_offset=0):
        """tg_gemm_f16's return code for the call as given (nothing is checked on this side)."""
        from any4_amd import ops

        rc = ops._L.tg_gemm_f16(x.data_ptr(), wp.data_ptr() + w_offset, out.data_ptr(), m, wrows, k, ops._dt(x), 1 if self.side == "B" else 0,
                                self.inner if inner is None else inner, ops._dev(x), ops._stream(x))
        torch.cuda.synchronize()
        return rc

    def __call__(self, x, w, out=None):
        wp = self.pack(w.contiguous())
        if out is None:
            return self.run(x, wp)
        assert out.is_contiguous() and out.shape == (x.shape[0], w.shape[0]) and w.shape[0] % self.pad == 0
        assert self.raw(x, wp, out, x.shape[0], w.shape[0], x.shape[1]) == 0
        return out


class OpW8:
    """tinygemm_y_f16RM_x_f16RM_w_int8TC behind w16_ref's gemm(x, codes, sz, g)."""

    def __init__(self, side, inner):
        self.side, self.inner, self.pad = side, inner, (8 if side == "B" else 16)

    def pack(self, codes):
        t = torch.ops.tinygemm
        return t.convert_matrix_to_m16n8k16_Bint8_layout(codes, self.inner) if self.side == "B" else t.convert_matrix_to_m16n8k16_Aint8_layout(codes, self.inner)

    def run(self, x, wp, sz, g):
        t = torch.ops.tinygemm
        return t.tinygemm_y_f16RM_x_f16RM_w_int8TC(x, wp, g, sz, True) if self.side == "B" else t.tinygemm_y_f16RM_x_f16RM_w_int8TC(wp, x, g, sz, False)

    def __call__(self, x, codes, sz, g):
        return self.run(x, self.pack(codes), sz, g)


LAYOUT_IDS = [f"{s}{i}" for s, i in R.F16_LAYOUTS]
DTYPES = [R.BF16, R.F16]


def _n_half(side):
    """A row count with wrows % 16 == 8 on the right (the clamped half tile); three tiles on the left."""
    return 136 if side == "B" else 48


# ---------------------------------------------------------------------------------------------------------------------------------
# f16_gemm_kernel
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.F16_CASES, ids=R.f16_id)
def test_f16_float64(T, c):
    R.check_f64_f16(OpF16(c.side, c.inner), c, DEV, RESULTS)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("side", ["B", "A"])
def test_f16_tc_layout_ops_float64(T, side, dtype):
    """tinygemm_y_f16TC_x_f16TC_w_f16TC, both sides, at a steady-loop k with ragged waves; m and n no multiples of 16."""
    import tinygemm_lib.functional as F

    m, n, k = 21, 43, 2048 + 32
    x, w = R.f16_inputs(m, n, k, dtype, DEV, seed=2)
    y = F.linear_y_f16TC_x_f16TC_W_f16TC(x, w, 2) if side == "B" else F.linear_y_f16TC_W_f16TC_x_f16TC(x, w, 2)
    assert y.shape == (m, n)
    R.assert_f64(f"TC-{R.dt_name(dtype)}-{side}-m{m}-n{n}-k{k}", y, x, w, RESULTS)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("side,inner", R.F16_LAYOUTS, ids=LAYOUT_IDS)
def test_f16_selection_probe(T, side, inner, dtype):
    """k = 2272 (nw = 9 x 7, 8: one steady round) and k = 4320 (nw = 17 x 7, 16: three): 1024 rows hit every column class mod 1024 (ring
    slot x wave x position) at a random round, the others the first and the last step; wrows % 16 == 8 on the right.  k = 96: every
    column, five idle waves."""
    gemm = OpF16(side, inner)
    R.check_select_f16(gemm, 17, 1032 if side == "B" else 1040, 2272, dtype, DEV)
    R.check_select_f16(gemm, 17, 1032 if side == "B" else 1040, 4096 + 224, dtype, DEV, seed=2)
    R.check_select_f16(gemm, 5, 136 if side == "B" else 144, 96, dtype, DEV, seed=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("side,inner", R.F16_LAYOUTS, ids=LAYOUT_IDS)
def test_f16_onehot_probe(T, side, inner, dtype):
    gemm = OpF16(side, inner)
    R.check_onehot_f16(gemm, 33, _n_half(side), 2272, dtype, DEV)
    R.check_onehot_f16(gemm, 5, _n_half(side), 96, dtype, DEV, seed=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("side,inner", R.F16_LAYOUTS, ids=LAYOUT_IDS)
def test_f16_decoy_and_nonfinite(T, side, inner, dtype):
    gemm = OpF16(side, inner)
    R.check_decoy_f16(gemm, 17, _n_half(side), 2080, dtype, DEV)
    R.check_decoy_f16(gemm, 1, _n_half(side), 32, dtype, DEV)
    R.check_nonfinite_f16(gemm, 17, _n_half(side), 2080, dtype, DEV)
    R.check_nonfinite_f16(gemm, 5, _n_half(side), 96, dtype, DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("side,inner", R.F16_LAYOUTS, ids=LAYOUT_IDS)
def test_f16_output_guard(T, side, inner, dtype):
    """tg_gemm_f16 writes y [m][wrows] and nothing around it, at m % 16 != 0 and (on the right) wrows % 16 == 8."""
    gemm = OpF16(side, inner)
    for m, n, k in ((17, _n_half(side), 2080), (5, 24 if side == "B" else 16, 96), (33, 8 if side == "B" else 16, 32)):
        R.check_guard_f16(gemm, m, n, k, dtype, DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
def test_f16_rejected_calls_leave_y_untouched(T, dtype):
    E_INNER_K, E_K_DIV, E_SHAPE, E_ALIGN = -2, -3, -7, -8   # include/tinygemm_hip.h
    m, n, k = 5, 48, 96
    x, w = R.f16_inputs(m, n, k, dtype, DEV)
    right, right2, left = OpF16("B", 1), OpF16("B", 2), OpF16("A", 1)
    wb, wb2, wa = right.pack(w), right2.pack(w), left.pack(w)
    out, whole = R.guarded(torch.zeros(m, n, dtype=dtype), DEV, fill=R.SENTINEL)
    out.view(torch.int16).fill_(R.SENTINEL)
    calls = [("k % 32 != 0", right.raw(x, wb, out, m, n, k - 16), E_K_DIV),
             ("k % 32 != 0, left", left.raw(x, wa, out, m, n, k + 16), E_K_DIV),
             ("wrows % 8 != 0 on the right", right.raw(x, wb, out, m, n - 4, k), E_SHAPE),
             ("wrows % 16 != 0 on the left", left.raw(x, wa, out, m, n - 8, k), E_SHAPE),
             ("innerKTiles 2 on the left", left.raw(x, wa, out, m, n, k, inner=2), E_INNER_K),
             ("innerKTiles 4 on the right", right.raw(x, wb, out, m, n, k, inner=4), E_INNER_K),
             ("a misaligned w", right2.raw(x, wb2, out, m, n, k, w_offset=8), E_ALIGN)]
    for what, rc, want in calls:
        assert rc == want, (what, rc)
    assert (whole.view(torch.int16) == R.SENTINEL).all(), "a rejected call wrote to y"
    assert right.raw(x, wb, out, m, n, k) == 0 and R.bits_equal(out, right(x, w))      # the same arguments, accepted


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("side,inner", R.F16_LAYOUTS, ids=LAYOUT_IDS)
def test_f16_op_clones_misaligned_activations(T, side, inner, dtype):
    """x at an 8-byte-aligned, not 16-byte-aligned, data pointer (the kernel loads 16 bytes): the op's clone path gives the aligned call's bits."""
    gemm = OpF16(side, inner)
    m, n, k = 5, _n_half(side), 2080
    x, w = R.f16_inputs(m, n, k, dtype, DEV, seed=7)
    buf = torch.zeros(m * k + 8, dtype=dtype, device=DEV)
    xo = buf[4:4 + m * k].view(m, k)
    xo.copy_(x)
    assert xo.data_ptr() % 16 == 8 and xo.is_contiguous()
    assert R.bits_equal(gemm(xo, w), gemm(x, w))


def _captured(run):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
def test_f16_deterministic_and_captured(T, dtype):
    gemm = OpF16("B", 2)
    x, w = R.f16_inputs(17, 136, 2272, dtype, DEV, seed=8)
    wp = gemm.pack(w)
    eager = R.check_deterministic(lambda: gemm.run(x, wp))
    assert R.bits_equal(_captured(lambda: gemm.run(x, wp)), eager)


# ---------------------------------------------------------------------------------------------------------------------------------
# w8_gemm_kernel
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.W8_CASES, ids=R.w8_id)
def test_w8_float64(T, oracle, c):
    """Codes are drawn and packed on the device.  The cases with n >= 4096 compare a SAMPLE of the weight rows against float64
    (w16_ref.sample_rows: every row of the first, a middle and the last two workgroups, the last 24 rows included): the oracle then
    dequantises a few hundred rows instead of 16 M weights."""
    R.check_f64_w8(OpW8(c.side, c.inner), oracle, c, DEV, RESULTS)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("side,inner,m,n,k,g", [("B", 4, 5, 65544, 256, 32), ("B", 4, 5, 65544, 256, 128), ("B", 1, 16, 1032, 4160, 32), ("A", 1, 16, 1040, 4160, 32),
                                                 ("B", 1, 16, 1032, 4224, 128)])
def test_w8_selection_probe(T, side, inner, m, n, k, g, dtype):
    """At the split-1 shape (every column of k = 256, 513 workgroups) and at split 8 with nw = 9 / 8 (65 / 66 row tiles keep launch_w8 at
    split 8): every column class mod 1024 = ring slot x slice x position in the 64-k step."""
    wrows = -(-n // 16) * 16
    assert R.w8_split(m, wrows, k)[0] == (1 if k == 256 else 8)
    R.check_select_w8(OpW8(side, inner), m, n, k, g, dtype, DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("side,inner", [("B", 1), ("B", 2), ("B", 4), ("A", 1), ("A", 2)])
def test_w8_onehot_decoy_nonfinite(T, oracle, side, inner, dtype):
    gemm = OpW8(side, inner)
    R.check_onehot_w8(gemm, oracle, 16, 72, 4160, 32, dtype, DEV)
    R.check_onehot_w8(gemm, oracle, 5, 72, 128, 128, dtype, DEV, seed=1)
    R.check_decoy_w8(gemm, 5, 68, 4224, 128, dtype, DEV)
    R.check_decoy_w8(gemm, 1, 68, 64, 32, dtype, DEV)
    R.check_nonfinite_w8(gemm, oracle, 16, 72, 4160, 32, dtype, DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
def test_w8_deterministic_and_captured(T, dtype):
    gemm = OpW8("B", 1)
    codes, x, sz = R.w8_inputs(16, 72, 4160, 32, dtype, DEV, gemm.pad, seed=8)
    wp = gemm.pack(codes)
    eager = R.check_deterministic(lambda: gemm.run(x, wp, sz, 32))
    assert R.bits_equal(_captured(lambda: gemm.run(x, wp, sz, 32)), eager)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("side,inner,m,n,k,g", [("B", 1, 1, 64, 64, 32), ("B", 2, 16, 72, 128, 128), ("A", 2, 5, 16400, 256, 32), ("A", 1, 16, 72, 4160, 32)])
def test_w8_fused_bias_on_the_16_row_kernel(T, side, inner, m, n, k, g, dtype):
    """ops.fused_bias on the 16-row kernel's store (split 1 / 2 / 4 / 8): RNE16(RNE16(sum) + bias), the bits of the separate `y + bias`."""
    from any4_amd import ops

    gemm = OpW8(side, inner)
    codes, x, sz = R.w8_inputs(m, n, k, g, dtype, DEV, gemm.pad, seed=9)
    wp = gemm.pack(codes)
    y = gemm.run(x, wp, sz, g)
    bias = torch.randn(sz.shape[1], generator=torch.Generator().manual_seed(5)).to(dtype).to(DEV)
    with ops.fused_bias(bias) as fb:
        yb = gemm.run(x, wp, sz, g)
    assert fb.consumed and R.bits_equal(yb, y + bias)
