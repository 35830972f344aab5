"""Input gradient of the 4-bit GEMMs on the GPU: the dx ops against the oracle's weights contracted in float64, autograd through the
row-major ops and the modules, every split regime of tests/grad_ref.DX_SPLIT_CASES split and unsplit, the identity probe of the word maps
(exact), non-finite dY, determinism, mx4 NaN, a LoRA chain and graph capture."""
import warnings

import numpy as np
import pytest
import torch

from tests import grad_ref
from tests.conftest import from_bits16
from tests.test_gpu_parity import assert_gemm_close, oracle_weights, rand_problem

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def T():
    import tinygemm  # noqa: F401

    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    return torch.ops.tinygemm


class _NoWorkspace(dict):
    """stands in for ops._WS_BYTES (the cache of workspace bytes per entry point and shape): every call asks for no workspace, so the dx kernel runs unsplit"""

    def get(self, key, default=None):
        return 0


def _pack(T, codes, on_right, inner):
    from any4_amd import ops

    if on_right:
        return T.convert_matrix_to_m16n8k16_Bint4_layout(codes.to(DEV), inner)
    with ops.weight_format("native"):
        return T.convert_matrix_to_m16n8k16_Aint4_layout(codes.to(DEV), inner)


def _forward(T, w, x, g, qtype, qinfo, lut, on_right):
    A, B = (x, w) if on_right else (w, x)
    if qtype == "mx4":
        return T.tinygemm_y_f16RM_x_f16RM_w_mx4TC(A, B, g, qinfo, on_right)
    if qtype == "int4":
        return T.tinygemm_y_f16RM_x_f16RM_w_int4TC(A, B, g, qinfo, on_right)
    return T.tinygemm_y_f16RM_x_f16RM_w_any4TC(A, B, g, qinfo, lut, on_right)


def _dx(T, dy, w, g, qtype, qinfo, lut, on_right):
    if qtype == "mx4":
        return T.tinygemm_dx_f16RM_dy_f16RM_w_mx4TC(dy, w, g, qinfo, on_right)
    if qtype == "int4":
        return T.tinygemm_dx_f16RM_dy_f16RM_w_int4TC(dy, w, g, qinfo, on_right)
    return T.tinygemm_dx_f16RM_dy_f16RM_w_any4TC(dy, w, g, qinfo, lut, on_right)


def _check_grad(T, oracle, n, k, g, m, qtype, dtype, on_right, inner, seed=0):
    codes, x, qinfo, lut = rand_problem(n, k, g, m, qtype, dtype, seed=seed)
    w = _pack(T, codes, on_right, inner)
    d = lambda t: None if t is None else t.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    y = _forward(T, w, xg, g, qtype, d(qinfo), d(lut), on_right)
    assert y.shape == (m, n) and y.grad_fn is not None
    dy = torch.randn(m, n, generator=torch.Generator().manual_seed(seed + 1)).to(dtype)
    (dx,) = torch.autograd.grad(y, xg, dy.to(DEV))
    assert dx.shape == (m, k) and dx.dtype == dtype
    wb = oracle_weights(oracle, codes, g, qtype, qinfo, lut, dtype)
    assert_gemm_close(dx, dy, np.ascontiguousarray(wb.T), dtype)   # dX = dY . W: the contraction over the weight rows
    return dx


QTYPES = [("int4", torch.bfloat16), ("int4", torch.float16), ("any4_global", torch.bfloat16), ("any4_global", torch.float16),
          ("any4_rowwise", torch.bfloat16), ("any4_rowwise", torch.float16), ("mx4", torch.bfloat16)]


@pytest.mark.parametrize("on_right", [True, False])
@pytest.mark.parametrize("qtype,dtype,g", [(q, d, g) for q, d in QTYPES for g in (32, 64, 128, 256) if q != "mx4" or g == 32])  # (mx4: groups of 32)
def test_dx_op_vs_oracle(T, oracle, qtype, dtype, g, on_right):
    inner = {32: 2, 64: 4, 128: 8, 256: 4}[g] if on_right else {32: 1, 64: 2, 128: 4, 256: 2}[g]
    # 208 weight rows: not a multiple of 64 (the kernel's row step) nor of 128
    _check_grad(T, oracle, 208, 512, g, 130, qtype, dtype, on_right, inner)


@pytest.mark.parametrize("on_right", [True, False])
@pytest.mark.parametrize("m", [1, 7, 16, 17, 130, 512])
def test_dx_m_sweep(T, oracle, m, on_right):
    n = 200 if on_right else 208   # (weights on the left: rows padded to 16)
    _check_grad(T, oracle, n, 256, 64, m, "any4_rowwise", torch.bfloat16, on_right, 4 if on_right else 2, seed=m)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("inner", [2, 4, 8])
def test_dx_inner_and_split(T, oracle, inner, split, monkeypatch):
    from any4_amd import ops

    if not split:
        monkeypatch.setattr(ops, "_WS_BYTES", _NoWorkspace())
    # many k tiles (k = 1024) and 2048 weight rows: with the workspace the launch splits over the weight rows (m = 16 fills few CUs;
    # test_dx_cpu.test_dx_inner_and_split_shapes_really_split holds the library to it)
    for shape in grad_ref.dx_inner_and_split_shapes(inner):
        _check_grad(T, oracle, *shape)


def test_dx_k_of_one_step_and_ragged(T, oracle):
    # k = 96: one ragged 128-column tile; weights on the left with k % 64 != 0 (native words of innerKTiles 2)
    _check_grad(T, oracle, 64, 96, 32, 33, "int4", torch.bfloat16, True, 2)
    _check_grad(T, oracle, 48, 96, 32, 33, "any4_rowwise", torch.bfloat16, False, 2)
    _check_grad(T, oracle, 8, 128, 64, 5, "int4", torch.float16, True, 8)


def test_dx_deterministic(T):
    codes, _, qinfo, lut = rand_problem(4096, 1024, 128, 16, "any4_rowwise")
    w = _pack(T, codes, True, 4)
    dy = torch.randn(16, 4096, generator=torch.Generator().manual_seed(3)).bfloat16().to(DEV)
    a = _dx(T, dy, w, 128, "any4_rowwise", qinfo.to(DEV), lut.to(DEV), True)
    b = _dx(T, dy, w, 128, "any4_rowwise", qinfo.to(DEV), lut.to(DEV), True)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ------------------------------------------------------------------------------------------------
# every split regime (tests/grad_ref.DX_SPLIT_CASES; test_dx_cpu holds the table to the library), exact probes, non-finite dY
# ------------------------------------------------------------------------------------------------

def _dev_problem(T, n, k, m, run, seed=0):
    """(codes, dy on the CPU; packed words, qinfo, lut on the GPU) of one launch of a case"""
    codes, _, qinfo, lut = rand_problem(n, k, run.g, 1, run.qtype, run.dtype, seed=seed)
    dy = torch.randn(m, n, generator=torch.Generator().manual_seed(seed + 1)).to(run.dtype)
    d = lambda t: None if t is None else t.to(DEV)
    return codes, dy, qinfo, lut, _pack(T, codes, run.on_right, run.inner), d(qinfo), d(lut)


DX_WORST = {}   # case id -> the largest err / tol of its split and unsplit results (printed; DESIGN section 11 records the maximum)


@pytest.mark.parametrize("case,run", grad_ref.DX_SPLIT_RUNS, ids=[grad_ref.dx_run_id(cr) for cr in grad_ref.DX_SPLIT_RUNS])
def test_dx_split_regimes_vs_float64(T, oracle, case, run, monkeypatch):
    """each regime three ways: split (the op with its workspace), split again (the same bits), unsplit (no workspace); both results
    against the oracle's weights contracted in float64 under the project's GEMM bound"""
    from any4_amd import ops

    n = case.wrows if run.on_right else case.wrows_left
    assert grad_ref.dx_splits(case.m, n, case.k, run.g, run.qtype, run.dtype, run.on_right, run.inner) == case.splits
    codes, dy, qinfo, lut, w, q, l = _dev_problem(T, n, case.k, case.m, run, seed=case.m)
    split = _dx(T, dy.to(DEV), w, run.g, run.qtype, q, l, run.on_right)
    again = _dx(T, dy.to(DEV), w, run.g, run.qtype, q, l, run.on_right)
    monkeypatch.setattr(ops, "_WS_BYTES", _NoWorkspace())
    unsplit = _dx(T, dy.to(DEV), w, run.g, run.qtype, q, l, run.on_right)
    assert split.shape == (case.m, case.k) and split.dtype == run.dtype
    assert torch.equal(split.view(torch.int16), again.view(torch.int16))
    wt = np.ascontiguousarray(oracle_weights(oracle, codes, run.g, run.qtype, qinfo, lut, run.dtype).T)   # dX = dY . W
    worst = {name: grad_ref.gemm_err_over_tol(got, dy, wt, run.dtype) for name, got in (("split", split), ("unsplit", unsplit))}
    DX_WORST[grad_ref.dx_run_id((case, run))] = max(worst.values())
    print(f"dx {grad_ref.dx_run_id((case, run))} ({case.splits} splits): max err / tol split {worst['split']:.4f}, unsplit {worst['unsplit']:.4f}; "
          f"largest so far {max(DX_WORST.values()):.4f}")
    assert_gemm_close(split, dy, wt, run.dtype)
    assert_gemm_close(unsplit, dy, wt, run.dtype)


def _identity_probe(T, oracle, n, k, g, qtype, dtype, on_right, inner, splits):
    """dY = I: dX is the dequantised weight matrix itself, bit for bit (every product is 1 w or 0 w, every f32 sum is exact in any
    order); -0 weights come out as +0, the sums start at +0.  (rand_problem keeps the mx4 exponents in 120 ... 130: no NaN weight.)"""
    assert grad_ref.dx_splits(n, n, k, g, qtype, dtype, on_right, inner) == splits
    codes, _, qinfo, lut = rand_problem(n, k, g, 1, qtype, dtype, seed=n + k + g)
    d = lambda t: None if t is None else t.to(DEV)
    dx = _dx(T, torch.eye(n, dtype=dtype, device=DEV), _pack(T, codes, on_right, inner), g, qtype, d(qinfo), d(lut), on_right)
    want = from_bits16(oracle_weights(oracle, codes, g, qtype, qinfo, lut, dtype), dtype) + 0.0
    assert want.shape == (n, k) and torch.isfinite(want.float()).all()
    got = dx.cpu()
    bad = got.view(torch.int16) != want.view(torch.int16)
    assert not bad.any(), f"{int(bad.sum())} / {bad.numel()} weights differ; first at (row, column) {bad.nonzero()[0].tolist()}"


# the word maps: Bint4 innerKTiles 2 / 4 / 8 and the convert op's 1 / 2 / 4 on the left (k = 512: native words of innerKTiles 4); the
# last entry is the other native order, that of k % 64 != 0 (innerKTiles 2)
WORDS = [(True, 2, 512, 32), (True, 4, 512, 64), (True, 8, 512, 128), (False, 1, 512, 32), (False, 2, 512, 64), (False, 4, 512, 128),
         (False, 2, 224, 32)]


@pytest.mark.parametrize("on_right,inner,k,g", WORDS)
@pytest.mark.parametrize("qtype,dtype", QTYPES)
def test_dx_identity_is_the_weight_matrix_bit_for_bit(T, oracle, qtype, dtype, on_right, inner, k, g):
    n, _, splits = grad_ref.DX_IDENTITY_SMALL
    _identity_probe(T, oracle, n, k, 32 if qtype == "mx4" else g, qtype, dtype, on_right, inner, splits)


@pytest.mark.parametrize("qtype,inner", [("any4_rowwise", 4), ("mx4", 2)])
def test_dx_identity_through_a_split(T, oracle, qtype, inner):
    # 17 x 2 tiles, 33 steps, 4 splits (test_dx_cpu.test_dx_probe_shapes_run_the_regime_they_name)
    n, k, splits = grad_ref.DX_IDENTITY_LARGE
    _identity_probe(T, oracle, n, k, 32, qtype, torch.bfloat16, True, inner, splits)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_dx_nonfinite_dy_reaches_its_row_and_no_other(T, value, split, monkeypatch):
    """fp16 training: an Inf / NaN in dY must reach dX (the loss scaler looks for it) and must stay in its row.  m = 33 on a BM = 64
    tile: tile rows 33 ... 63 are clamped copies of row 32, computed and discarded."""
    from any4_amd import ops

    N = grad_ref.DX_NONFINITE
    m, n, k, row, r0 = N["m"], N["wrows"], N["k"], N["row"], N["r0"]
    run = grad_ref.Run("any4_rowwise", 64, torch.float16, True, 4)
    assert grad_ref.dx_splits(m, n, k, run.g, run.qtype, run.dtype, True, run.inner) == N["splits"]
    if not split:
        monkeypatch.setattr(ops, "_WS_BYTES", _NoWorkspace())
    _, dy, _, _, w, q, l = _dev_problem(T, n, k, m, run, seed=7)
    clean = _dx(T, dy.to(DEV), w, run.g, run.qtype, q, l, True).cpu()
    assert torch.isfinite(clean.float()).all()
    dy[row, r0] = value
    dx = _dx(T, dy.to(DEV), w, run.g, run.qtype, q, l, True).cpu()
    assert not torch.isfinite(dx[row].float()).any(), f"{int(torch.isfinite(dx[row].float()).sum())} finite columns in row {row}"
    assert torch.equal(dx[:row].view(torch.int16), clean[:row].view(torch.int16))


def test_dx_stride0_dy(T, oracle):
    """y.sum().backward() hands the op an expanded (stride-0) dY"""
    codes, x, qinfo, lut = rand_problem(64, 256, 64, 9, "int4")
    w = _pack(T, codes, True, 4)
    xg = x.to(DEV).requires_grad_(True)
    _forward(T, w, xg, 64, "int4", qinfo.to(DEV), None, True).sum().backward()
    wb = oracle_weights(oracle, codes, 64, "int4", qinfo, None)
    assert_gemm_close(xg.grad, torch.ones(9, 64, dtype=torch.bfloat16), np.ascontiguousarray(wb.T))


def test_dx_mx4_nan(T, oracle):
    n, k, g, m = 64, 256, 32, 20
    codes, x, qinfo, _ = rand_problem(n, k, g, m, "mx4")
    qinfo[5, 3] = 255     # row 5, k 96 ... 127: NaN weights
    qinfo[40, 7] = 255    # row 40, k 224 ... 255
    w = _pack(T, codes, True, 4)
    xg = x.to(DEV).requires_grad_(True)
    y = _forward(T, w, xg, g, "mx4", qinfo.to(DEV), None, True)
    dy = torch.randn(m, n, generator=torch.Generator().manual_seed(9)).bfloat16()
    (dx,) = torch.autograd.grad(y, xg, dy.to(DEV))
    wd = from_bits16(oracle_weights(oracle, codes, g, "mx4", qinfo, None), torch.bfloat16).double()
    dense = dy.double() @ wd
    assert torch.equal(torch.isnan(dx.cpu()), torch.isnan(dense))
    assert torch.isnan(dense).any()


def test_dx_reference_aint4_words_name_relayout(T):
    from any4_amd import ops

    codes, x, qinfo, _ = rand_problem(64, 256, 64, 4, "int4")
    with ops.weight_format("reference"):
        w = T.convert_matrix_to_m16n8k16_Aint4_layout(codes.to(DEV), 4)
    xg = x.to(DEV).requires_grad_(True)
    y = T.tinygemm_y_f16RM_x_f16RM_w_int4TC(w, xg, 64, qinfo.to(DEV), False)
    with pytest.raises(RuntimeError, match="relayout"):
        y.sum().backward()


def test_dx_graph_capture_replays_eager_bits(T):
    codes, _, qinfo, lut = rand_problem(4096, 1024, 128, 16, "any4_rowwise")
    w, q, l = _pack(T, codes, True, 4), qinfo.to(DEV), lut.to(DEV)
    dy = torch.randn(16, 4096, generator=torch.Generator().manual_seed(4)).bfloat16().to(DEV)
    eager = _dx(T, dy, w, 128, "any4_rowwise", q, l, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _dx(T, dy, w, 128, "any4_rowwise", q, l, True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _dx(T, dy, w, 128, "any4_rowwise", q, l, True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), eager.view(torch.int16))


# ------------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------------

def _module(cls, kernel, n, k, g, bias, seed=0):
    import modules

    gen = torch.Generator().manual_seed(seed)
    kw = dict(bias=bias, device=DEV, dtype=torch.bfloat16, group_size=g, kernel=kernel)
    mod = getattr(modules, cls)(k, n, **kw)
    codes = torch.randint(0, 16, (n, k), dtype=torch.int32, generator=gen)
    mod.weight.data = codes.to(DEV)
    if cls == "MX4Linear":
        qinfo = torch.randint(120, 131, (n, k // g), dtype=torch.uint8, generator=gen)
        mod.exponents.data = qinfo.to(DEV)
        lut, qtype = None, "mx4"
    else:
        qinfo = torch.stack([(torch.rand(k // g, n, generator=gen) * 0.02 + 0.005), torch.randn(k // g, n, generator=gen) * 0.01], 2).bfloat16()
        mod.scales_and_zeros.data = qinfo.to(DEV)
        lut, qtype = None, "int4"
        if cls == "Any4Linear":
            lut, qtype = torch.randn(n, 16, generator=gen).bfloat16(), "any4_rowwise"
            mod.lut.data = lut.to(DEV)
        elif cls == "NF4Linear":
            lut, qtype = mod.lut.data.cpu(), "any4_global"
    if bias:
        mod.bias.data = torch.randn(n, generator=gen).bfloat16().to(DEV)
    from any4_amd import ops

    with ops.weight_format("native"):
        mod.reshape_weight()
    return mod, codes, qinfo, lut, qtype


MODULES = [("Int4Linear", "linear_y_f16RM_W_int4TC_x_f16RM"), ("Int4Linear", "linear_y_f16RM_x_f16RM_W_int4TC"),
           ("Any4Linear", "linear_y_f16RM_x_f16RM_W_any4TC"), ("Any4Linear", "linear_y_f16RM_W_any4TC_x_f16RM"),
           ("NF4Linear", "linear_y_f16RM_x_f16RM_W_any4TC"), ("MX4Linear", "linear_y_f16RM_x_f16RM_W_mx4TC"),
           ("MX4Linear", "linear_y_f16RM_W_mx4TC_x_f16RM")]


@pytest.mark.parametrize("shape", [(37,), (3, 50)])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("cls,kernel", MODULES)
def test_module_backward_vs_dense_twin(oracle, cls, kernel, bias, shape):
    n, k = 96, 256
    g = 32 if cls == "MX4Linear" else 64
    mod, codes, qinfo, lut, qtype = _module(cls, kernel, n, k, g, bias)
    x = torch.randn(*shape, k, generator=torch.Generator().manual_seed(5)).bfloat16().to(DEV)
    with torch.no_grad():
        y_ref = mod(x)
    xg = x.clone().requires_grad_(True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        y = mod(xg)
        assert y.grad_fn is not None
        y.sum().backward()
    assert not [w for w in caught if "autograd" in str(w.message)], [str(w.message) for w in caught]
    assert torch.equal(y.detach().view(torch.int16), y_ref.view(torch.int16))   # grad mode: the same launches, the same bits
    rows = int(np.prod(shape))
    wb = oracle_weights(oracle, codes, g, qtype, qinfo, lut)
    assert_gemm_close(xg.grad.reshape(rows, k), torch.ones(rows, n, dtype=torch.bfloat16), np.ascontiguousarray(wb.T))
    if bias:
        assert torch.equal(mod.bias.grad.float().cpu(), torch.full((n,), float(rows)))
    for name in ("scales_and_zeros", "lut", "exponents"):
        p = getattr(mod, name, None)
        if p is not None:
            assert p.grad is None, name


def test_module_bias_only_grad(oracle):
    """x without grad, the bias a Parameter: the output still carries the graph to the bias (and the fused-bias launch)"""
    mod, *_ = _module("Int4Linear", "linear_y_f16RM_W_int4TC_x_f16RM", 64, 128, 64, True)
    x = torch.randn(7, 128, generator=torch.Generator().manual_seed(2)).bfloat16().to(DEV)
    mod(x).sum().backward()
    assert torch.equal(mod.bias.grad.float().cpu(), torch.full((64,), 7.0))


def test_lora_chain_first_adapter_matches_dense_twin(oracle):
    import modules

    k, n, r = 256, 256, 8
    gen = torch.Generator().manual_seed(11)
    layers, dense = [], []
    for i in range(2):
        mod, codes, qinfo, lut, qtype = _module("Any4Linear", "linear_y_f16RM_x_f16RM_W_any4TC", n, k, 64, False, seed=20 + i)
        layers.append(mod)
        dense.append(from_bits16(oracle_weights(oracle, codes, 64, qtype, qinfo, lut), torch.bfloat16).float().to(DEV))
    assert isinstance(layers[0], modules.Any4Linear)
    A = [(torch.randn(r, k, generator=gen) * 0.05).to(DEV) for _ in range(2)]
    B = [(torch.randn(n, r, generator=gen) * 0.05).to(DEV) for _ in range(2)]
    x = torch.randn(16, k, generator=gen).to(DEV)

    def run(base):
        a = [t.bfloat16().requires_grad_(True) for t in A]
        b = [t.bfloat16().requires_grad_(True) for t in B]
        h = x.bfloat16()
        for i in range(2):
            h = base(i, h) + (h @ a[i].t()) @ b[i].t()
        h.float().pow(2).sum().backward()
        return a[0].grad.float(), b[0].grad.float()

    ga, gb = run(lambda i, h: layers[i](h))
    ta, tb = run(lambda i, h: (h.float() @ dense[i].t()).bfloat16())
    for got, want in ((ga, ta), (gb, tb)):
        rel = (got - want).norm() / want.norm()
        assert rel < 3e-2, float(rel)
