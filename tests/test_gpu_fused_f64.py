"""GPU suite (-m gpu): the stages fused into the 4-bit GEMM launches (tg_w4_gemm ABI 5, any4_amd.ops.w4_linear_fused) on every kernel
that carries them -- w4_gemv_kernel, w4_gemm_pair16_kernel, w4_gemm_pair16_loop_kernel, w4_gemm_pair_kernel -- against the float64
references of tests/fused_ref.py (the two fused-norm contracts, their allowances and the case table are stated there; the table is
checked against the dry planner on the CPU by tests/test_fused_ref_cpu.py):

  a  the fused RMSNorm against float64 at every output row, per dtype, group size, row count, ring depth and contraction; the refusals
  b  SwiGLU / residual: the bits of the separate stage on the same launch's unfused output, whose float64 check closes the chain
  c  probes with exact inputs: the norm weight's index, the output's placement and the gate / up pairing, the residual passed through
  d  the persistent stacked kernel's fused paths through the C ABI

Every operand sits between NaN guard bands, `out` between sentinel bands that must come back intact.

Figures of one run on an MI355X (worst |y - ref| / allowance per group of cases, wall time): profiles/fused_f64_checks.txt.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import fused_ref as F
from tests.test_gpu_parity import DEV, T  # noqa: F401  (T is a fixture)

pytestmark = pytest.mark.gpu

RESULTS = []  # (group, case id, worst |y - ref| / allowance): written to $FUSED_F64_REPORT when the module is done (profiles/fused_f64_checks.txt)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("FUSED_F64_REPORT")
    if path:
        with open(path, "w") as f:
            for group, cid, ratio in RESULTS:
                f.write(f"{group:10s} {cid:70s} {ratio:.3f}\n")


@functools.lru_cache(maxsize=2)
def _dev_layer(n, k, g, qtype, dtype, inner):
    """F.layer's weights packed and on the device (shared by the cases of one shape: the table keeps them adjacent)."""
    L = F.layer(n, k, g, qtype, dtype)
    w = torch.ops.tinygemm.convert_matrix_to_m16n8k16_Bint4_layout(L.codes.to(DEV), inner)
    return L, w, L.qinfo.to(DEV), None if L.lut is None else L.lut.to(DEV)


def _launch(w, g, qinfo, lut, x, numerics="fast", norm=None, res=None, swiglu=False, inplace=False, res_extra=64):
    """One ops.w4_linear_fused call with every operand between guard bands (x, norm weight, residual: NaN; out: the sentinel; the
    residual additionally a view into rows `res_extra` columns wider, NaN there).  Returns y on the CPU, or None where the library
    refuses the stage.  inplace: out is the (contiguous) residual."""
    import any4_amd
    from any4_amd import ops

    m, n = x.shape[0], w.shape[0] * 8
    xd, _ = F.guarded(x, DEV)
    nd = None if norm is None else F.guarded(norm, DEV)[0]
    rd = whole = None
    if res is not None:
        rd, whole = F.guarded(res, DEV, extra_cols=0 if inplace else res_extra)
    if inplace:
        out, sentinel = rd, None
    else:
        out, sentinel = F.guarded(torch.zeros(m, n // 2 if swiglu else n, dtype=x.dtype), DEV, fill=F.SENTINEL)
        out.view(torch.int16).fill_(0x7FC1)   # a NaN in both types: every element must be written
    assert out.is_contiguous()
    with any4_amd.numerics(numerics):
        y = ops.w4_linear_fused(xd, w, g, qinfo, lut, residual=rd, norm_weight=nd, norm_eps=F.EPS, swiglu=swiglu, out=out)
    torch.cuda.synchronize()
    if y is None:
        return None
    assert y is out
    if sentinel is not None:
        assert F.guard_intact(out, sentinel), "the launch wrote outside its output"
    else:
        g2 = F.GUARD_BYTES // 2
        assert torch.isnan(whole[:g2].float()).all() and torch.isnan(whole[g2 + out.numel():].float()).all(), "the launch wrote outside its output"
    y = y.cpu()
    assert not torch.isnan(y.float()).any(), "an output element was not written, or a guard band was read"
    return y


def _run(c, x, **kw):
    L, w, qinfo, lut = _dev_layer(c.n, c.k, c.g, c.qtype, c.dtype, c.inner)
    return L, _launch(w, c.g, qinfo, lut, x, numerics=c.numerics, **kw)


def _assert_close(group, cid, got, ref, tol):
    ratio = np.abs(got - ref) / tol
    print(f"{cid}: worst |y - ref| / allowance {ratio.max():.3f}")
    RESULTS.append((group, cid, float(ratio.max())))
    bad = ratio > 1
    at = np.argwhere(bad)[:4]
    assert not bad.any(), (f"{cid}: {bad.sum()} / {bad.size} outside the allowance, worst ratio {ratio.max():.2f}; (row, column, got, ref, allowance): "
                           f"{[(int(a), int(r), float(got[a, r]), float(ref[a, r]), float(tol[a, r])) for a, r in at]}")


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _swiglu16(gu):
    """decode_ops.swiglu (dg_swiglu, float64-checked in test_gpu_glue_f64.py) of a GEMM output with rows in gate / up blocks."""
    from any4_amd import decode_ops as G

    return G.swiglu(F.split_gate_up(gu.to(DEV))).cpu()


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the fused norm against float64
# ---------------------------------------------------------------------------------------------------------------------------------

def _check_norm(oracle, group, c, x, gw, y):
    cid = F.case_id(c)
    L = F.layer(c.n, c.k, c.g, c.qtype, c.dtype)
    rows = np.sort(F.sample_rows(c.n)) if c.sample else None
    ref, tol = F.norm_ref(oracle, L, x, gw, c.formula, rows=rows)
    got = y.double().numpy()
    if c.swiglu:
        ref, tol = F.swiglu_of_sums(ref, tol, c.dtype)
        if rows is not None:
            blocks = rows.reshape(-1, 16)[:, 0] // 16
            got = got[:, (blocks[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)]
    elif rows is not None:
        got = got[:, rows]
    _assert_close(group, cid, got, ref, tol)


@pytest.mark.parametrize("c", F.NORM_CASES, ids=F.case_id)
def test_fused_norm_against_float64(T, oracle, c):
    """Every output row (the one 28672-row case: a row sample; its placement probe below checks every row) under the contract of the
    kernel that carries the case: "sum" without any per-activation rounding term, "act" with the interval term A."""
    assert F.fused_plan(c.m, c.n, c.k, c.g, c.qtype, c.dtype, c.inner, norm_weight=True, epilogue=int(c.swiglu), numerics=c.numerics) == c.family
    x, gw, _ = F.make_inputs(c.m, c.n, c.k, c.dtype, seed=c.m + c.g)
    _, y = _run(c, x, norm=gw, swiglu=c.swiglu)
    assert y is not None, "the dry plan names a kernel, the call found none"   # (tgx::gemv answers the dry plan before its template selection)
    _check_norm(oracle, "norm", c, x, gw, y)


@pytest.mark.parametrize("r", F.REFUSED, ids=[r[0] for r in F.REFUSED])
def test_documented_refusals(T, r):
    """TG_E_FUSION -> None from ops.w4_linear_fused, and the same call without the stage runs."""
    _, m, n, k, g, qtype, dtype, inner, norm, swiglu, _ = r
    c = F.Case("pair16", m, n, k, g, qtype, dtype, inner)
    x, gw, _ = F.make_inputs(m, n, k, dtype, seed=1)
    assert _run(c, x, norm=gw if norm else None, swiglu=swiglu)[1] is None
    assert _run(c, x)[1] is not None


# ---------------------------------------------------------------------------------------------------------------------------------
# b. SwiGLU and the residual add
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", F.STAGE_CASES, ids=F.case_id)
def test_stages_compose(T, oracle, c):
    """The bits of the separate stage applied to the same launch's unfused output -- with and without the norm, the residual as a view
    into wider rows and in place -- and that unfused output itself against float64."""
    x, gw, res = F.make_inputs(c.m, c.n, c.k, c.dtype, seed=c.m + c.k)
    L, plain = _run(c, x)
    _, normed = _run(c, x, norm=gw)
    assert plain is not None and normed is not None
    ref, tol = F.plain_ref(oracle, L, x)
    _assert_close("plain", F.case_id(c), plain.double().numpy(), ref, tol)
    _check_norm(oracle, "stages", c, x, gw, normed)
    for base, norm in ((plain, None), (normed, gw)):
        want = base + res                                              # 16 bit + 16 bit: one rounding
        assert _bits_equal(_run(c, x, norm=norm, res=res)[1], want), "residual, rows wider than n"
        assert _bits_equal(_run(c, x, norm=norm, res=res, inplace=True)[1], want), "residual, in place"
        act = _run(c, x, norm=norm, swiglu=True)[1]
        assert act is not None and act.shape == (c.m, c.n // 2)
        assert _bits_equal(act, _swiglu16(base)), "SwiGLU" + (" with the norm" if norm is not None else "")


@pytest.mark.parametrize("m", [1, 16])
def test_mx4_residual_and_swiglu_on_the_16_row_kernel(T, oracle, m):
    c = F.Case("pair16", m, 1040, 2048, 32, "mx4", F.BF16)
    x, _, res = F.make_inputs(m, c.n, c.k, c.dtype, seed=m)
    L, plain = _run(c, x)
    ref, tol = F.plain_ref(oracle, L, x)
    _assert_close("plain", F.case_id(c), plain.double().numpy(), ref, tol)
    assert _bits_equal(_run(c, x, res=res)[1], plain + res)
    assert _bits_equal(_run(c, x, res=res, inplace=True)[1], plain + res)
    assert _bits_equal(_run(c, x, swiglu=True)[1], _swiglu16(plain))


# ---------------------------------------------------------------------------------------------------------------------------------
# c. probes
# ---------------------------------------------------------------------------------------------------------------------------------

_INDEX_CARRIERS = [c for dt in (F.BF16, F.F16) for c in (
    F.Case("gemv", 4, 1032, 2048, 64, "any4_rowwise", dt), F.Case("gemv", 4, 1032, 8192, 128, "any4_rowwise", dt),
    F.Case("gemv", 8, 1032, 4096, 128, "any4_rowwise", dt), F.Case("pair16", 16, 1032, 2048, 128, "any4_rowwise", dt),
    F.Case("pair16", 4, 1032, 2048, 128, "any4_rowwise", dt, numerics="fast_mfma"), F.Case("pair16_loop", 16, 4112, 4096, 128, "any4_rowwise", dt),
)]


@functools.lru_cache(maxsize=1)
def _probe_layer(n, k, g, qtype, dtype, inner):
    """F.layer's weights with every zero point 0: a one-hot activation then leaves ONE product scale * lut * x per output.  (With a zero
    point the group-scaled kernels add scale * lut * x and zero * x as two f32 terms; where the two nearly cancel, the f32 rounding of
    the larger one -- 2^-24 of it -- exceeds 4e-6 |x w|, which only bounds it while S sums many terms.)"""
    L0 = F.layer(n, k, g, qtype, dtype)
    qinfo = L0.qinfo.clone()
    qinfo[:, :, 1] = 0
    L = F.SimpleNamespace(**{**vars(L0), "qinfo": qinfo})
    w = torch.ops.tinygemm.convert_matrix_to_m16n8k16_Bint4_layout(L.codes.to(DEV), inner)
    return L, w, qinfo.to(DEV), L.lut.to(DEV)


@pytest.mark.parametrize("c", _INDEX_CARRIERS, ids=F.case_id)
def test_norm_weight_index_probe(T, oracle, c):
    """Activation row a is one-hot at j_a (element 0, k - 1, the last element of a 32-chunk and the first of the next, one element in
    each of the eight k-slices); the norm weights (1 + (j mod 64) / 64) 2^((j div 64) mod 4) are exact in 16 bits and differ from
    their neighbours by 1 / 128 and more of their size, the allowance (S is one term) is half an output step."""
    k = c.k
    L, w, qinfo, lut = _probe_layer(c.n, c.k, c.g, c.qtype, c.dtype, c.inner)
    js = [0, k - 1, 31, 32] + [w * (k // 8) + 37 + w for w in range(8)]
    j = torch.arange(k)
    gw = ((1 + (j % 64) / 64.0) * torch.exp2(((j // 64) % 4).float())).to(c.dtype)
    assert torch.equal(gw.double(), (1 + (j % 64) / 64.0).double() * torch.exp2(((j // 64) % 4).double()))
    for b in range(0, len(js), c.m):
        x = torch.zeros(c.m, k)
        for a in range(c.m):
            x[a, js[(b + a) % len(js)]] = 1.5 * 2.0 ** (a % 3)
        x = x.to(c.dtype)
        y = _launch(w, c.g, qinfo, lut, x, numerics=c.numerics, norm=gw)
        assert y is not None
        ref, tol = F.norm_ref(oracle, L, x, gw, c.formula)
        _assert_close("index", f"{F.case_id(c)} j={[js[(b + a) % len(js)] for a in range(c.m)]}", y.double().numpy(), ref, tol)


def _placement_shapes():
    seen, out = set(), []
    for c in F.NORM_CASES + F.STAGE_CASES:
        key = (c.m, c.n, c.k, c.g, c.dtype, c.inner, c.numerics)
        if key not in seen:
            seen.add(key)
            out.append(F.Case(c.kernel, c.m, c.n, c.k, c.g, "any4_rowwise", c.dtype, c.inner, c.numerics))
    return out


@pytest.mark.parametrize("c", _placement_shapes(), ids=F.case_id)
def test_output_placement_and_gate_up_pairing_probe(T, c):
    """lut[row] holds ONE value v_row in all 16 entries (scale 1, zero 0) and x[a] = c_a e_0 with c_a a power of two: the accumulator of
    (a, row) is exactly c_a v_row whatever the codes are, the v_row distinct 16-bit values.  Plain and residual outputs must be that
    (plus the residual) in every column of every row, SwiGLU outputs the bits of dg_swiglu of the assembled [gate | up] values:
    every row of every range and pass, the 28672-row layer included."""
    m, n, k, dt = c.m, c.n, c.k, c.dtype
    gen = torch.Generator().manual_seed(n + k)
    w = torch.randint(-2 ** 31, 2 ** 31 - 1, (n // 8, k // (16 * c.inner), 32, c.inner // 2), dtype=torch.int64, generator=gen).to(torch.int32).to(DEV)
    v = F.distinct_values(n, dt, seed=n)
    lut = v[:, None].expand(n, 16).contiguous().to(DEV)
    qinfo = torch.stack([torch.ones(k // c.g, n), torch.zeros(k // c.g, n)], dim=2).to(dt).contiguous().to(DEV)
    ca = torch.exp2((torch.arange(m) % 3 - 1).float())
    x = torch.zeros(m, k)
    x[:, 0] = ca
    x = x.to(dt)
    want = (ca[:, None].double() * v[None, :].double()).to(dt)
    assert torch.equal(want.double(), ca[:, None].double() * v[None, :].double())   # exact
    res = torch.randn(m, n, generator=gen).to(dt)
    run = functools.partial(_launch, w, c.g, qinfo, lut, x, numerics=c.numerics)
    assert _bits_equal(run(), want), "plain"
    assert _bits_equal(run(res=res), want + res), "residual"
    if n % 16 == 0:
        assert _bits_equal(run(swiglu=True), _swiglu16(want)), "SwiGLU"


@pytest.mark.parametrize("c", F.STAGE_CASES, ids=F.case_id)
def test_residual_pass_through_probe(T, c):
    """x = 0: y is the residual bit for bit, with and without the norm (1 / rms = eps^-1/2 times a zero sum)."""
    x, gw, res = F.make_inputs(c.m, c.n, c.k, c.dtype, seed=3)
    x = torch.zeros_like(x)
    res[res == 0] = 1.0          # no -0: 0 + -0 = +0
    for norm in (None, gw):
        assert _bits_equal(_run(c, x, norm=norm, res=res)[1], res)
        assert _bits_equal(_run(c, x, norm=norm, res=res, inplace=True)[1], res)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. the persistent stacked kernel (w4_gemm_pair_kernel<.., NORM> and its SwiGLU store) through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------

def _stacked(layers, m, n, k, g, seed):
    import bench

    w, x, q, lut, y = bench.make_batch(layers, m, n, k, g, 4, torch.device(DEV), seed, "any4_rowwise", True)
    xs = torch.stack([F.make_inputs(m, n, k, F.BF16, seed=seed + b)[0] for b in range(layers)])
    x.copy_(xs)
    return w, x, q, lut, y, xs


def _stacked_call(w, x, q, lut, y, m, n, k, g, layers, norm=None, swiglu=False):
    import bench
    from any4_amd import _lib

    L = _lib.load()
    aa = bench.make_args(_lib, w, x, q, lut, y, m, n, k, g, "any4_rowwise", True, 4, layers)
    if norm is not None:
        aa.norm_weight, aa.norm_eps = norm.data_ptr(), F.EPS
    if swiglu:
        aa.epilogue = _lib.TG_EPI_SWIGLU
    ws = bench.attach_workspace(L, aa, torch.device(DEV))  # noqa: F841
    assert L.tg_gemm_w4_plan(ctypes.byref(aa), 0) == _lib.TG_PLAN_PAIR
    y.view(torch.int16).fill_(0x7FC1)
    assert _lib.check(L.tg_gemm_w4(ctypes.byref(aa), 0, torch.cuda.current_stream().cuda_stream), "tg_gemm_w4") is None
    torch.cuda.synchronize()
    assert not torch.isnan(y.float()).any()
    return y


@pytest.mark.parametrize("layers", [12, 13])
@pytest.mark.parametrize("m,k", [(1, 2048), (3, 2048), (1, 4096)])
def test_stacked_kernel_fused_norm_against_float64(oracle, layers, m, k):
    """192 and more items of 64 rows: w4_gemm_pair_kernel<.., NORM> (chunk_rmsnorm in x_stage: the "act" contract), one norm weight for
    all problems, every problem of the batch against float64."""
    n, g = 1024, 128
    w, x, q, lut, y, xs = _stacked(layers, m, n, k, g, seed=layers + m)
    gw = F.make_inputs(m, n, k, F.BF16, seed=99)[1]
    gd, _ = F.guarded(gw, DEV)
    y = _stacked_call(w, x, q, lut, y, m, n, k, g, layers, norm=gd).cpu()
    worst = 0.0
    for b in range(layers):
        codes = torch.from_numpy(oracle.unpack_Bint4(w[b].cpu().numpy(), n, k))
        Lb = F.SimpleNamespace(n=n, k=k, g=g, qtype="any4_rowwise", dtype=F.BF16, codes=codes, qinfo=q[b].cpu(), lut=lut[b].cpu())
        ref, tol = F.norm_ref(oracle, Lb, xs[b], gw, "act")
        ratio = np.abs(y[b].double().numpy() - ref) / tol
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1).all(), f"problem {b}: worst ratio {ratio.max():.2f} at {np.argwhere(ratio > 1)[:4].tolist()}"
    print(f"stacked m={m} k={k} x{layers}: worst |y - ref| / allowance {worst:.3f}")
    RESULTS.append(("stacked", f"pair-m{m}-n{n}-k{k}-g{g}-x{layers}", worst))


@pytest.mark.parametrize("layers", [12, 13])
@pytest.mark.parametrize("m", [1, 8])
def test_stacked_kernel_swiglu_store(layers, m):
    """The same kernel's SwiGLU store: the bits of dg_swiglu of the plain stacked launch's output, problem by problem."""
    n, k, g = 1024, 2048, 128
    w, x, q, lut, y, _ = _stacked(layers, m, n, k, g, seed=layers + m)
    plain = _stacked_call(w, x, q, lut, y, m, n, k, g, layers).cpu()
    act = _stacked_call(w, x, q, lut, torch.empty(layers, m, n // 2, dtype=torch.bfloat16, device=DEV), m, n, k, g, layers, swiglu=True).cpu()
    for b in range(layers):
        assert _bits_equal(act[b], _swiglu16(plain[b])), f"problem {b}"
