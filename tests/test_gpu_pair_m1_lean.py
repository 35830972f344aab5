"""GPU suite (-m gpu): the lean m = 1 pair kernel (w4_pair_m1_lean_kernel, any4_amd/csrc/w4_gemm_pair.cuh) -- the plain stacked launch of
one activation row at innerKTiles 4, g = 128 -- on batches of DIFFERENT problems, so that a workgroup's walk over its items shows: ranges
that cross a problem boundary (activations restaged, the LUT changes), one round and four rounds per wave, waves with an empty k-slice,
the last item of a range asking for its own rows again.  Which kernel a call takes is asked of the library (tg_gemm_w4_plan_detail).

Every problem of every batch is compared with the oracle's group-scaled restatement (oracle.linear_group_scaled, the same math in double)
at the tolerance of tests/test_gpu_fast.py:
        |y - y64| <= 0.5 ulp16(y64) (1 + 2^-7) + 4e-6 S,   S = sum_k |x_k w_k|
Calls that the lean kernel does not take (rows not a multiple of 64, a bias) run the general template; with an all-zero bias its result
must equal the lean kernel's as floats, which pins the two flavours to each other.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import bits16, from_bits16
from tests.test_gpu_parity import DEV, T, oracle_weights, ulp16  # noqa: F401  (T is a fixture)

pytestmark = [pytest.mark.gpu]

QT = {"int4": 0, "any4_global": 1, "any4_rowwise": 2}
G = 128

_problems = {}


def problems(oracle, n, k, batch, qtype, dtype):
    """`batch` different problems (one activation row each) and, per problem, the oracle's group-scaled result and S; made once per case."""
    key = (n, k, batch, qtype, dtype)
    if key in _problems:
        return _problems[key]
    gen = torch.Generator().manual_seed(n * 7 + k + batch + QT[qtype])
    codes = torch.randint(0, 16, (batch, n, k), dtype=torch.int32, generator=gen)
    x = torch.randn(batch, 1, k, generator=gen).to(dtype)
    scales = (torch.rand(batch, k // G, n, generator=gen) * 0.02 + 0.005).to(dtype)
    zeros = (torch.randn(batch, k // G, n, generator=gen) * 0.01).to(dtype)
    qinfo = torch.stack([scales, zeros], dim=3).contiguous()
    lut = {"int4": None, "any4_global": torch.randn(batch, 16, generator=gen).to(dtype),
           "any4_rowwise": torch.randn(batch, n, 16, generator=gen).to(dtype)}[qtype]
    q = {"int4": oracle.Q_INT4, "any4_global": oracle.Q_ANY4_GLOBAL, "any4_rowwise": oracle.Q_ANY4_ROWWISE}[qtype]
    dt = oracle.BF16 if dtype == torch.bfloat16 else oracle.F16
    y_gs = np.empty((batch, n), np.float64)
    S = np.empty((batch, n), np.float64)
    for b in range(batch):
        lb = None if lut is None else lut[b]
        _, y32 = oracle.linear_group_scaled(bits16(x[b]), codes[b].numpy(), G, q, bits16(qinfo[b]), None if lb is None else bits16(lb), dt)
        y_gs[b] = y32.astype(np.float64)[0]
        w = from_bits16(oracle_weights(oracle, codes[b], G, qtype, qinfo[b], lb, dtype), dtype).double()
        S[b] = (x[b].double().abs() @ w.abs().t()).numpy()[0]
    _problems[key] = (codes, x, qinfo, lut, y_gs, S)
    return _problems[key]


def run_stack(T, codes, x, qinfo, lut, qtype, bias=None):
    """One tg_gemm_w4 call over the batch; returns (y [batch][1][wrows], what tg_gemm_w4_plan_detail says of that very call)."""
    from any4_amd import _lib

    L = _lib.load()
    batch, n, k = codes.shape
    dt = x.dtype
    packed = torch.stack([T.convert_matrix_to_m16n8k16_Bint4_layout(codes[b].to(DEV), 4) for b in range(batch)]).contiguous()
    wrows = packed.shape[1] * 8
    if qinfo.shape[2] < wrows:  # the rows of the tile padding
        qinfo = torch.cat([qinfo, torch.zeros(batch, qinfo.shape[1], wrows - qinfo.shape[2], 2, dtype=qinfo.dtype)], dim=2)
    if lut is not None and lut.dim() == 3 and lut.shape[1] < wrows:
        lut = torch.cat([lut, torch.zeros(batch, wrows - lut.shape[1], 16, dtype=lut.dtype)], dim=1)
    xs, qs = x.to(DEV).contiguous(), qinfo.to(DEV).contiguous()
    luts = None if lut is None else lut.to(DEV).contiguous()
    bs = None if bias is None else bias.to(DEV).contiguous()
    ys = torch.full((batch, 1, wrows), float("nan"), dtype=dt, device=DEV)
    args = _lib.W4Gemm(x=xs.data_ptr(), w=packed.data_ptr(), qinfo=qs.data_ptr(), lut=(luts.data_ptr() if luts is not None else None),
                       y=ys.data_ptr(), m=1, wrows=wrows, k=k, group=G, qtype=QT[qtype],
                       dtype=_lib.TG_BF16 if dt == torch.bfloat16 else _lib.TG_F16, w_on_right=1, inner_k_tiles=4, batch=batch,
                       stride_x=xs.stride(0) * 2, stride_w=packed.stride(0) * 4, stride_qinfo=qs.stride(0) * 2,
                       stride_lut=(luts.stride(0) * 2 if luts is not None else 0), stride_y=ys.stride(0) * 2,
                       numerics=_lib.TG_NUM_FAST, bias=(bs.data_ptr() if bs is not None else None),
                       stride_bias=(bs.stride(0) * 2 if bs is not None else 0))
    assert L.tg_gemm_w4_workspace_bytes(ctypes.byref(args)) == 0
    plan = L.tg_gemm_w4_plan_detail(ctypes.byref(args), 0)
    assert L.tg_gemm_w4_plan(ctypes.byref(args), 0) == _lib.TG_PLAN_PAIR
    _lib.check(L.tg_gemm_w4(ctypes.byref(args), 0, torch.cuda.current_stream().cuda_stream), "stacked m = 1 launch")
    torch.cuda.synchronize()
    return ys, plan


def assert_close(ys, y_gs, S, dtype):
    n = y_gs.shape[1]
    got = ys.detach().double().cpu().numpy()[:, 0, :n]
    assert not np.isnan(got).any()
    tol = 0.5 * ulp16(y_gs, dtype) * (1 + 2.0 ** -7) + 4e-6 * S + 1e-37
    err = np.abs(got - y_gs)
    bad = err > tol
    print(f"max |y - y_gs| {err.max():.3e}, max err / tol {(err / tol).max():.3f}")
    assert not bad.any(), f"vs group-scaled oracle: {bad.sum()} / {bad.size} outside tolerance (problems {np.unique(np.nonzero(bad)[0])[:8]}); worst {err.max()}"


# (n, k, batch): 3 row blocks x 173 problems = 519 items on 512 workgroups (ranges of 1 and 2 items, some across a problem boundary; one
# round per wave) | every item a new problem, four rounds per wave | 192 items, the family's minimum: fewer items than workgroups, waves
# 4 ... 7 with an empty k-slice
CASES = [(192, 1024, 173), (64, 4096, 600), (128, 512, 96)]


@pytest.mark.parametrize("case", CASES)
def test_lean_kernel_vs_oracle(T, oracle, case):
    from any4_amd import _lib

    n, k, batch = case
    codes, x, qinfo, lut, y_gs, S = problems(oracle, n, k, batch, "any4_rowwise", torch.bfloat16)
    ys, plan = run_stack(T, codes, x, qinfo, lut, "any4_rowwise")
    assert plan == _lib.TG_PLAN_PAIR_M1_LEAN
    assert_close(ys, y_gs, S, torch.bfloat16)


@pytest.mark.parametrize("qtype,dtype", [("any4_global", torch.bfloat16), ("int4", torch.bfloat16), ("any4_rowwise", torch.float16),
                                         ("any4_global", torch.float16)])
def test_lean_kernel_other_tables(T, oracle, qtype, dtype):
    """The first case with a global LUT (one per problem: the table is kept across the items of a problem and rebuilt at a problem
    boundary), with int4 (one table for the launch), and in fp16."""
    from any4_amd import _lib

    n, k, batch = CASES[0]
    codes, x, qinfo, lut, y_gs, S = problems(oracle, n, k, batch, qtype, dtype)
    ys, plan = run_stack(T, codes, x, qinfo, lut, qtype)
    assert plan == _lib.TG_PLAN_PAIR_M1_LEAN
    assert_close(ys, y_gs, S, dtype)


def test_rows_not_a_multiple_of_64_take_the_general_kernel(T, oracle):
    from any4_amd import _lib

    codes, x, qinfo, lut, y_gs, S = problems(oracle, 200, 1024, 64, "any4_rowwise", torch.bfloat16)
    ys, plan = run_stack(T, codes, x, qinfo, lut, "any4_rowwise")
    assert plan == _lib.TG_PLAN_PAIR
    assert_close(ys, y_gs, S, torch.bfloat16)


def test_zero_bias_on_the_general_kernel_equals_the_lean_result(T, oracle):
    from any4_amd import _lib

    n, k, batch = CASES[0]
    codes, x, qinfo, lut, y_gs, S = problems(oracle, n, k, batch, "any4_rowwise", torch.bfloat16)
    y_lean, plan = run_stack(T, codes, x, qinfo, lut, "any4_rowwise")
    assert plan == _lib.TG_PLAN_PAIR_M1_LEAN
    y_bias, plan = run_stack(T, codes, x, qinfo, lut, "any4_rowwise", bias=torch.zeros(batch, n, dtype=torch.bfloat16))
    assert plan == _lib.TG_PLAN_PAIR
    assert_close(y_bias, y_gs, S, torch.bfloat16)
    assert torch.equal(y_bias.float(), y_lean.float())
