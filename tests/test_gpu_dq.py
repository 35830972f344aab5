"""Gradients of scales, zeros and LUT of the 4-bit GEMMs on the GPU (tg_gemm_w4_dq): the dq ops against a float64 evaluation of

    H[g][r][c] = sum_{j in group g, code(r, j) = c} sum_a dY[a][r] x[a][j],   dz = sum_c H,  ds = sum_c lut H,  dlut = sum_g s H

from the same 16-bit inputs, exact known answers that pin the word -> (row, k) maps, determinism, graph capture, autograd through the ops
and the modules under any4_amd.quant_param_grad, and tune_quant_params against a CPU twin.

Tolerance of the f32 op outputs: |got - want| <= 4e-6 * S + 1e-37, S = the same sum with every factor replaced by its absolute value
(4e-6: the project's f32-accumulation term, test_gpu_parity.assert_gemm_close; no 16-bit term, the outputs are f32).  Through autograd
into 16-bit .grads: plus 0.5 ulp16(want) (1 + 2^-7)."""
import numpy as np
import pytest
import torch

from tests import grad_ref
from tests.grad_ref import dq_reference as reference
from tests.test_gpu_parity import assert_gemm_close, oracle_weights, rand_problem, ulp16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def T():
    import tinygemm  # noqa: F401

    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    return torch.ops.tinygemm


def _pack(T, codes, on_right, inner):
    from any4_amd import ops

    if on_right:
        return T.convert_matrix_to_m16n8k16_Bint4_layout(codes.to(DEV), inner)
    with ops.weight_format("native"):
        return T.convert_matrix_to_m16n8k16_Aint4_layout(codes.to(DEV), inner)


def assert_close_f32(got, want, S, what):
    err = (got.detach().double().cpu() - want).abs()
    tol = 4e-6 * S + 1e-37
    print(f"{what}: max err / tol = {float((err / tol).max()):.4f}")
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.numel()} outside tolerance; worst err / tol {float((err / tol).max())}"
    return float((err / tol).max())


def assert_close_16(got, want, S, dtype, what):
    err = (got.detach().double().cpu() - want).abs()
    tol = 4e-6 * S + 1e-37 + torch.from_numpy(0.5 * ulp16(want.numpy(), dtype) * (1 + 2.0 ** -7))
    print(f"{what}: max err / tol = {float((err / tol).max()):.4f}")
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.numel()} outside tolerance; worst err / tol {float((err / tol).max())}"


def _dq(T, x, dy, w, g, qinfo, lut, on_right):
    if lut is None:
        return T.tinygemm_dq_f16RM_x_f16RM_w_int4TC(x, dy, w, g, qinfo, on_right), None
    return T.tinygemm_dq_f16RM_x_f16RM_w_any4TC(x, dy, w, g, qinfo, lut, on_right)


def _check_op(T, n, k, g, m, qtype, dtype, on_right, inner, seed=0):
    codes, x, qinfo, lut = rand_problem(n, k, g, m, qtype, dtype, seed=seed)
    dy = torch.randn(m, n, generator=torch.Generator().manual_seed(seed + 1)).to(dtype)
    w = _pack(T, codes, on_right, inner)
    d = lambda t: None if t is None else t.to(DEV)
    dq, dl = _dq(T, d(x), d(dy), w, g, d(qinfo), d(lut), on_right)
    assert dq.shape == qinfo.shape and dq.dtype == torch.float32
    (wq, wl), (sq, sl) = reference(codes, x, dy, qinfo, lut, g)
    worst = assert_close_f32(dq, wq, sq, "d_qinfo")
    if lut is None:
        assert dl is None
    else:
        assert dl.shape == lut.shape and dl.dtype == torch.float32
        worst = max(worst, assert_close_f32(dl, wl, sl, "d_lut"))
    return worst


QTYPES = [(q, d) for q in ("int4", "any4_global", "any4_rowwise") for d in (torch.bfloat16, torch.float16)]


@pytest.mark.parametrize("on_right", [True, False])
@pytest.mark.parametrize("qtype,dtype,g", [(q, d, g) for q, d in QTYPES for g in (32, 64, 128, 256)])
def test_dq_op_vs_float64(T, qtype, dtype, g, on_right):
    inner = {32: 2, 64: 4, 128: 8, 256: 4}[g] if on_right else {32: 1, 64: 2, 128: 4, 256: 2}[g]
    # 208 weight rows: not a multiple of 64 nor of 128 (the kernel's row tile)
    _check_op(T, 208, 512, g, 130, qtype, dtype, on_right, inner)


@pytest.mark.parametrize("on_right", [True, False])
@pytest.mark.parametrize("m", [1, 7, 31, 32, 33, 130, 512])
def test_dq_m_sweep(T, m, on_right):
    n = 200 if on_right else 208   # (weights on the left: rows padded to 16)
    _check_op(T, n, 256, 64, m, "any4_rowwise", torch.bfloat16, on_right, 4 if on_right else 2, seed=m)


def test_dq_edges(T):
    # k = 96: one ragged 128-column tile (innerKTiles 2 on the right; the native words of k % 64 != 0 on the left)
    _check_op(T, 64, 96, 32, 33, "int4", torch.bfloat16, True, 2)
    _check_op(T, 48, 96, 32, 33, "any4_rowwise", torch.bfloat16, False, 2)
    # fewer rows than a tile, innerKTiles 8, fp16
    _check_op(T, 8, 128, 64, 5, "any4_global", torch.float16, True, 8)
    # one group over the whole of k, wider than the kernel's column tile
    _check_op(T, 72, 256, 256, 40, "any4_rowwise", torch.bfloat16, True, 4)


DQ_WORST = {}   # case id -> its largest err / tol (printed; DESIGN section 14 records the maximum)


@pytest.mark.parametrize("case", grad_ref.DQ_CASES, ids=grad_ref.dq_case_id)
def test_dq_cases_vs_float64(T, case):
    """ragged k tiles among several, three and seventeen row tiles, the step boundary of the activation rows (tests/grad_ref.DQ_CASES;
    test_dq_cpu holds the claimed tile and step counts to the shapes)"""
    c = case
    DQ_WORST[grad_ref.dq_case_id(c)] = _check_op(T, c.wrows, c.k, c.g, c.m, c.qtype, c.dtype, c.on_right, c.inner, seed=c.m)
    print(f"dq {grad_ref.dq_case_id(c)}: max err / tol {DQ_WORST[grad_ref.dq_case_id(c)]:.4f}; largest so far {max(DQ_WORST.values()):.4f}")


def _nonfinite_problem(T):
    """any4 row-wise, fp16: code 5 is absent from group 2 of row r0 (present in its other groups), code 11 from the whole row"""
    N = grad_ref.DQ_NONFINITE
    n, k, g, m, r0 = N["wrows"], N["k"], N["g"], N["m"], N["r0"]
    codes, x, qinfo, lut = rand_problem(n, k, g, m, "any4_rowwise", torch.float16, seed=11)
    row = codes[r0]
    row[row == 11] = 12
    grp = row[2 * g:3 * g]
    grp[grp == 5] = 6
    row[0], row[4 * g] = 5, 5
    assert not (row == 11).any() and not (row[2 * g:3 * g] == 5).any() and (row == 5).any()
    dy = torch.randn(m, n, generator=torch.Generator().manual_seed(12)).half()
    w = _pack(T, codes, True, 2)
    run = lambda x_, dy_: tuple(t.cpu() for t in T.tinygemm_dq_f16RM_x_f16RM_w_any4TC(x_.to(DEV), dy_.to(DEV), w, g, qinfo.to(DEV), lut.to(DEV), True))
    return N, codes, x, dy, run


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_dq_nonfinite_dy_reaches_its_row_and_no_other(T, value):
    """dY[64][r0] non-finite, r0 = 199 the last row of a ragged row tile (rows 200 ... 255 of the tile load clamped copies of real rows),
    row 64 the last activation row, alone in its step.  By the definition (select by code, then sum) every G[r0][j] is non-finite, so
    every d_qinfo[g][r0] and every d_lut[r0][c] of a code present in the row is; a code absent from the row sums nothing and stays 0; no
    other row sees the value."""
    N, codes, x, dy, run = _nonfinite_problem(T)
    r0, a0 = N["r0"], N["a0"]
    dq0, dl0 = run(x, dy)
    assert torch.isfinite(dq0).all() and torch.isfinite(dl0).all()
    dy[a0, r0] = value
    dq, dl = run(x, dy)
    assert not torch.isfinite(dq[:, r0, :]).any(), dq[:, r0, :]
    present = torch.bincount(codes[r0], minlength=16) > 0
    assert int(present.sum()) == 15 and not present[11]
    assert not torch.isfinite(dl[r0][present]).any(), dl[r0]
    assert dl[r0][11] == 0.0
    others = torch.arange(N["wrows"]) != r0
    assert torch.equal(dq[:, others].view(torch.int32), dq0[:, others].view(torch.int32))
    assert torch.equal(dl[others].view(torch.int32), dl0[others].view(torch.int32))


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_dq_nonfinite_x_reaches_its_group_and_no_other(T, value):
    """x[64][159] non-finite: the last column of the ragged k tile (columns 160 ... 255 of the tile load clamped copies of real columns).
    G[r][159] is non-finite for every row, so d_qinfo[g(159)][r] is; every other group is untouched."""
    N, codes, x, dy, run = _nonfinite_problem(T)
    g0 = N["j0"] // N["g"]
    dq0, _ = run(x, dy)
    x[N["a0"], N["j0"]] = value
    dq, _ = run(x, dy)
    assert not torch.isfinite(dq[g0]).any(), f"{int(torch.isfinite(dq[g0]).sum())} finite values in group {g0}"
    others = torch.arange(N["k"] // N["g"]) != g0
    assert torch.equal(dq[others].view(torch.int32), dq0[others].view(torch.int32))


@pytest.mark.parametrize("on_right,inner", [(True, 2), (True, 4), (True, 8), (False, 2)])
def test_dq_known_answer_exact(T, on_right, inner):
    """x = 1, dY one-hot at (0, r0), s = 1, z = 0, lut[r][c] = c: d_lut[r0] counts the codes of row r0, every other row is zero,
    dz[g][r0] = g, ds[g][r0] = the sum of the group's codes -- small integers, exact in f32"""
    n, k, g, m = 208, 256, 64, 3
    codes = torch.randint(0, 16, (n, k), dtype=torch.int32, generator=torch.Generator().manual_seed(5))
    w = _pack(T, codes, on_right, inner)
    x = torch.ones(m, k, dtype=torch.bfloat16, device=DEV)
    qinfo = torch.stack([torch.ones(k // g, n), torch.zeros(k // g, n)], 2).bfloat16().to(DEV)
    lut = torch.arange(16, dtype=torch.float32).expand(n, 16).bfloat16().contiguous().to(DEV)
    for r0 in (0, 7, 8, 129, 207):
        dy = torch.zeros(m, n, dtype=torch.bfloat16, device=DEV)
        dy[0, r0] = 1
        dq, dl = T.tinygemm_dq_f16RM_x_f16RM_w_any4TC(x, dy, w, g, qinfo, lut, on_right)
        want_l = torch.zeros(n, 16)
        want_l[r0] = torch.bincount(codes[r0], minlength=16).float()
        assert torch.equal(dl.cpu(), want_l), r0
        want_q = torch.zeros(k // g, n, 2)
        want_q[:, r0, 0] = codes[r0].view(k // g, g).sum(1).float()
        want_q[:, r0, 1] = g
        assert torch.equal(dq.cpu(), want_q), r0


def _det_problem(T):
    codes, x, qinfo, lut = rand_problem(4096, 1024, 128, 16, "any4_rowwise")
    dy = torch.randn(16, 4096, generator=torch.Generator().manual_seed(3)).bfloat16()
    return x.to(DEV), dy.to(DEV), _pack(T, codes, True, 4), qinfo.to(DEV), lut.to(DEV)


def test_dq_deterministic(T):
    x, dy, w, q, l = _det_problem(T)
    a = T.tinygemm_dq_f16RM_x_f16RM_w_any4TC(x, dy, w, 128, q, l, True)
    b = T.tinygemm_dq_f16RM_x_f16RM_w_any4TC(x, dy, w, 128, q, l, True)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_dq_graph_capture_replays_eager_bits(T):
    x, dy, w, q, l = _det_problem(T)
    eager = T.tinygemm_dq_f16RM_x_f16RM_w_any4TC(x, dy, w, 128, q, l, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.tinygemm_dq_f16RM_x_f16RM_w_any4TC(x, dy, w, 128, q, l, True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = T.tinygemm_dq_f16RM_x_f16RM_w_any4TC(x, dy, w, 128, q, l, True)
    graph.replay()
    torch.cuda.synchronize()
    for u, v in zip(out, eager):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# autograd at op level
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("on_right", [True, False])
def test_autograd_op_fills_qinfo_and_lut_under_the_switch(T, on_right):
    import any4_amd

    n, k, g, m, dtype = 208, 256, 64, 37, torch.bfloat16
    codes, x, qinfo, lut = rand_problem(n, k, g, m, "any4_rowwise", dtype, seed=2)
    dy = torch.randn(m, n, generator=torch.Generator().manual_seed(7)).to(dtype)
    w = _pack(T, codes, on_right, 4 if on_right else 2)

    def run():
        xg, qg, lg = x.to(DEV).requires_grad_(True), qinfo.to(DEV).requires_grad_(True), lut.to(DEV).requires_grad_(True)
        A, B = (xg, w) if on_right else (w, xg)
        y = T.tinygemm_y_f16RM_x_f16RM_w_any4TC(A, B, g, qg, lg, on_right)
        return torch.autograd.grad(y, (xg, qg, lg), dy.to(DEV), allow_unused=True)

    dx_off, dq_off, dl_off = run()
    assert dq_off is None and dl_off is None   # the default: scales, zeros and LUT are constants of the graph
    with any4_amd.quant_param_grad():
        dx, dq, dl = run()
    assert torch.equal(dx.view(torch.int16), dx_off.view(torch.int16))
    assert dq.dtype == dtype and dl.dtype == dtype and dq.shape == qinfo.shape and dl.shape == lut.shape
    (wq, wl), (sq, sl) = reference(codes, x, dy, qinfo, lut, g)
    assert_close_16(dq, wq, sq, dtype, "qinfo.grad")
    assert_close_16(dl, wl, sl, dtype, "lut.grad")


# ------------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------------

def _module(cls, kernel, n, k, g, bias, per_row=True, seed=0, fmt="native"):
    import modules
    from any4_amd import ops

    gen = torch.Generator().manual_seed(seed)
    kw = dict(bias=bias, device=DEV, dtype=torch.bfloat16, group_size=g, kernel=kernel)
    if cls == "Any4Linear":
        kw["per_row"] = per_row
    mod = getattr(modules, cls)(k, n, **kw)
    codes = torch.randint(0, 16, (n, k), dtype=torch.int32, generator=gen)
    mod.weight.data = codes.to(DEV)
    if cls == "MX4Linear":
        mod.exponents.data = torch.randint(120, 131, (n, k // g), dtype=torch.uint8, generator=gen).to(DEV)
        qinfo, lut, qtype = None, None, "mx4"
    else:
        qinfo = torch.stack([(torch.rand(k // g, n, generator=gen) * 0.02 + 0.005), torch.randn(k // g, n, generator=gen) * 0.01], 2).bfloat16()
        mod.scales_and_zeros.data = qinfo.to(DEV)
        lut, qtype = None, "int4"
        if cls == "Any4Linear":
            lut = torch.randn(*((n, 16) if per_row else (16,)), generator=gen).bfloat16()
            qtype = "any4_rowwise" if per_row else "any4_global"
            mod.lut.data = lut.to(DEV)
        elif cls == "NF4Linear":
            lut, qtype = mod.lut.data.cpu(), "any4_global"
    if bias:
        mod.bias.data = torch.randn(n, generator=gen).bfloat16().to(DEV)
    with ops.weight_format(fmt):
        mod.reshape_weight()
    return mod, codes, qinfo, lut, qtype


MODULES = [("Int4Linear", "linear_y_f16RM_W_int4TC_x_f16RM", True), ("Int4Linear", "linear_y_f16RM_x_f16RM_W_int4TC", True),
           ("Any4Linear", "linear_y_f16RM_x_f16RM_W_any4TC", True), ("Any4Linear", "linear_y_f16RM_W_any4TC_x_f16RM", True),
           ("Any4Linear", "linear_y_f16RM_x_f16RM_W_any4TC", False), ("Any4Linear", "linear_y_f16RM_W_any4TC_x_f16RM", False),
           ("NF4Linear", "linear_y_f16RM_x_f16RM_W_any4TC", True)]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("cls,kernel,per_row", MODULES)
def test_module_backward_fills_quant_params(oracle, cls, kernel, per_row, bias):
    import any4_amd

    n, k, g, rows = 96, 256, 64, 37
    mod, codes, qinfo, lut, qtype = _module(cls, kernel, n, k, g, bias, per_row)
    x = torch.randn(rows, k, generator=torch.Generator().manual_seed(5)).bfloat16()
    dy = torch.randn(rows, n, generator=torch.Generator().manual_seed(6)).bfloat16()
    with torch.no_grad():
        y_ref = mod(x.to(DEV))
    xg = x.to(DEV).requires_grad_(True)
    with any4_amd.quant_param_grad():
        y = mod(xg)
    assert torch.equal(y.detach().view(torch.int16), y_ref.view(torch.int16))   # the same launches, the same bits
    y.backward(dy.to(DEV))   # (outside the context: the forward captured the switch)
    (wq, wl), (sq, sl) = reference(codes, x, dy, qinfo, lut, g)
    assert_close_16(mod.scales_and_zeros.grad, wq, sq, torch.bfloat16, "scales_and_zeros.grad")
    if lut is not None:
        assert_close_16(mod.lut.grad, wl, sl, torch.bfloat16, "lut.grad")
    wb = oracle_weights(oracle, codes, g, qtype, qinfo, lut)
    assert_gemm_close(xg.grad, dy, np.ascontiguousarray(wb.T))
    if bias:
        assert torch.equal(mod.bias.grad, dy.to(DEV).sum(0))


def test_module_quant_params_without_input_grad_and_frozen_lut():
    import any4_amd

    n, k, g, rows = 96, 256, 64, 21
    mod, codes, qinfo, lut, _ = _module("Any4Linear", "linear_y_f16RM_x_f16RM_W_any4TC", n, k, g, False)
    x = torch.randn(rows, k, generator=torch.Generator().manual_seed(8)).bfloat16()
    mod.lut.requires_grad_(False)
    mod(x.to(DEV))              # (switch off: records the launch plan of this shape; the next call must still build a graph)
    assert mod.__dict__.get("_plan") is not None
    with any4_amd.quant_param_grad():
        y = mod(x.to(DEV))
        assert y.grad_fn is not None
        y.sum().backward()
    assert mod.lut.grad is None
    (wq, _), (sq, _) = reference(codes, x, torch.ones(rows, n).bfloat16(), qinfo, lut, g)
    assert_close_16(mod.scales_and_zeros.grad, wq, sq, torch.bfloat16, "scales_and_zeros.grad")


def test_module_mx4_ignores_the_switch():
    import any4_amd

    mod, *_ = _module("MX4Linear", "linear_y_f16RM_x_f16RM_W_mx4TC", 64, 128, 32, False)
    xg = torch.randn(9, 128, generator=torch.Generator().manual_seed(1)).bfloat16().to(DEV).requires_grad_(True)
    with any4_amd.quant_param_grad():
        mod(xg).sum().backward()
    assert mod.exponents.grad is None and xg.grad is not None


def test_module_reference_aint4_words_name_relayout():
    import any4_amd

    mod, *_ = _module("Int4Linear", "linear_y_f16RM_W_int4TC_x_f16RM", 64, 256, 64, False, fmt="reference")
    x = torch.randn(4, 256, generator=torch.Generator().manual_seed(1)).bfloat16().to(DEV)
    with any4_amd.quant_param_grad(), pytest.raises(RuntimeError, match="relayout"):
        mod(x).sum().backward()


# ------------------------------------------------------------------------------------------------
# tune_quant_params
# ------------------------------------------------------------------------------------------------

def test_tune_quant_params_keeps_pace_with_a_cpu_twin():
    """100 Adam steps at lr 1e-3 on lut + scales_and_zeros against Y = X W^T.  The twin: the same optimisation of a float32 dense layer on
    the CPU with 16-bit-rounded parameters, weights and outputs, straight through every rounding; its ratio rho = loss_after / loss_before.
    The kernel path must reach at least half the twin's improvement: ratio <= (1 + rho) / 2 (the margin: bf16 parameter rounding sends
    the two runs along different trajectories)."""
    from any4_amd import ops
    from any4_amd.quantize import anyq_layer, tune_quant_params

    torch.manual_seed(0)
    n, k, g, m = 64, 256, 64, 256
    W = torch.randn(n, k) * 0.02
    X = torch.randn(m, k) * torch.exp(torch.randn(k))
    Y = X @ W.t()
    lin = torch.nn.Linear(k, n, bias=False, device=DEV, dtype=torch.bfloat16)
    lin.weight.data = W.bfloat16().to(DEV)
    mod = anyq_layer(lin, group_size=g)
    codes = ops.unpack_int4(mod.weight.data, n, k, "B").cpu().long()
    lut0, sz0 = mod.lut.detach().float().cpu(), mod.scales_and_zeros.detach().float().cpu()
    Xb, Yb = X.bfloat16(), Y.bfloat16()

    # the CPU twin
    ste = lambda t: t + (t.bfloat16().float() - t).detach()
    lut_m, sz_m = lut0.clone().requires_grad_(True), sz0.clone().requires_grad_(True)
    opt = torch.optim.Adam([lut_m, sz_m], lr=1e-3)

    def twin_loss():
        l16, s16 = ste(lut_m), ste(sz_m)
        s = s16[..., 0].t().repeat_interleave(g, 1)
        z = s16[..., 1].t().repeat_interleave(g, 1)
        w = ste(torch.gather(l16, 1, codes) * s + z)
        return (ste(Xb.float() @ w.t()) - Yb.float()).pow(2).mean()

    t_before = float(twin_loss().detach())
    for _ in range(100):
        opt.zero_grad()
        twin_loss().backward()
        opt.step()
    rho = float(twin_loss().detach()) / t_before

    before, after = tune_quant_params(mod, Xb.to(DEV), Yb.to(DEV), steps=100, lr=1e-3, params=("lut", "scales_and_zeros"))
    ratio = after / before
    print(f"tune_quant_params: loss {before:.4e} -> {after:.4e}, ratio {ratio:.3f}; CPU twin ratio {rho:.3f} (from {t_before:.4e})")
    assert rho < 1.0
    assert ratio <= (1 + rho) / 2, (ratio, rho)
