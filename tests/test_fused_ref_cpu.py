"""CPU suite: the helpers of tests/fused_ref.py themselves -- the two fused-norm references against a plain torch statement of each
formula, the 3 % condition of the interval argument at every case of the table, and the case table against the library's dry
planner (tg_gemm_w4_plan: no GPU needed), so that the table is known to be right before any GPU time is spent on it."""
import numpy as np
import pytest
import torch

from tests import fused_ref as F


def _tiny_layer(n, k, g, qtype, dtype):
    return F.layer(n, k, g, qtype, dtype, seed=3)


@pytest.mark.parametrize("dtype", [F.BF16, F.F16])
@pytest.mark.parametrize("qtype,g", [("any4_rowwise", 32), ("int4", 64), ("any4_global", 128)])
def test_norm_references_against_plain_torch(oracle, dtype, qtype, g):
    """Both contracts at a size small enough to write the sums out: dequantised weights in float64 (w = lut[code] * scale + zero, no
    rounding: the group-scaled arithmetic), activations normalised by torch in f32 / float64."""
    m, n, k = 3, 24, 256
    L = _tiny_layer(n, k, g, qtype, dtype)
    x, gw, _ = F.make_inputs(m, n, k, dtype, seed=1)
    lut = (torch.arange(16) - 8).to(dtype) if L.lut is None else L.lut
    lv = (lut[L.codes.long()] if lut.dim() == 1 else torch.gather(lut, 1, L.codes.long())).double()          # [n][k]
    sc = L.qinfo[:, :, 0].double().repeat_interleave(g, dim=0).t()                                             # [n][k]
    zz = L.qinfo[:, :, 1].double().repeat_interleave(g, dim=0).t()
    w = lv * sc + zz
    rs = torch.rsqrt(x.double().pow(2).mean(1) + float(np.float32(F.EPS)))
    # "sum": rs * sum RNE16(x g) w
    want = rs[:, None] * ((x.float() * gw.float()).to(dtype).double() @ w.t())
    ref, tol = F.norm_gemv_ref(oracle, L, x, gw)
    assert np.abs(ref - want.numpy()).max() <= 1e-6 * np.abs(want.numpy()).max()      # (the oracle returns its double sum as f32)
    assert (tol > 0).all() and (tol < 0.02 * np.abs(want.numpy()).max()).all()
    # "act": dg_add_rmsnorm's formula in f32, as transformers' LlamaRMSNorm states it for a 16-bit weight
    xn = ((x.float() * rs.float()[:, None]).to(dtype).float() * gw.float()).to(dtype)
    ref2, tol2, share = F.norm_pair_ref(oracle, L, x, gw)
    want2 = xn.double() @ w.t()
    assert np.abs(ref2 - want2.numpy()).max() <= 1e-6 * np.abs(want2.numpy()).max()
    mid, lo, hi, _ = F.act_norm_bracket(x, gw)
    assert torch.equal(mid, xn)
    assert ((lo.double() <= hi.double()) | (x.double() * gw.double() < 0)).all() and ((lo.double() >= hi.double()) | (x.double() * gw.double() > 0)).all()
    assert ((mid.double() - lo.double()) * (mid.double() - hi.double()) <= 0).all()  # the centre lies between the ends
    assert (tol2 >= F.contract(ref2, 0 * ref2, dtype)).all() and share.max() <= F.AMBIGUOUS_MAX


def test_interval_ends_are_f32_numbers_inside_the_interval():
    rs = np.array([0.3, 1.0, 7.123456789, 1e-3])
    lo, hi = F._f32_inside(rs * (1 - F.RS_REL), up=True), F._f32_inside(rs * (1 + F.RS_REL), up=False)
    assert lo.dtype == hi.dtype == np.float32
    assert (lo.astype(np.float64) >= rs * (1 - F.RS_REL)).all() and (hi.astype(np.float64) <= rs * (1 + F.RS_REL)).all()
    assert (np.nextafter(lo, np.float32(-np.inf)).astype(np.float64) < rs * (1 - F.RS_REL)).all()
    assert (np.nextafter(hi, np.float32(np.inf)).astype(np.float64) > rs * (1 + F.RS_REL)).all()


def test_ambiguous_share_is_at_most_3_percent_in_every_row_of_every_case(capsys):
    """The condition the "act" allowance rests on, at the inputs of every case that takes it (and, as a margin, at every other case's
    inputs too): printed as the measured maximum."""
    worst = {F.BF16: (0.0, 0.0), F.F16: (0.0, 0.0)}
    seen = set()
    for c in F.NORM_CASES + F.STAGE_CASES:
        key = (c.m, c.k, c.dtype)
        if key in seen:
            continue
        seen.add(key)
        x, gw, _ = F.make_inputs(c.m, 8, c.k, c.dtype, seed=c.m + c.k)
        mid, lo, hi, share = F.act_norm_bracket(x, gw)
        assert share.max() <= F.AMBIGUOUS_MAX, (F.case_id(c), share.max())
        rel = float(((hi.double() - lo.double()).abs().sum(1) / mid.double().abs().sum(1)).max())
        worst[c.dtype] = (max(worst[c.dtype][0], float(share.max())), max(worst[c.dtype][1], rel))
    with capsys.disabled():
        for dt, (s, r) in worst.items():
            print(f"\n  ambiguous share, {dt}: max {s:.4f} of a row's activations; sum|x'+ - x'-| / sum|x'| max {r:.2e}", end="")


@pytest.mark.parametrize("c", F.NORM_CASES, ids=F.case_id)
def test_plan_of_every_carried_case(c):
    got = F.fused_plan(c.m, c.n, c.k, c.g, c.qtype, c.dtype, c.inner, norm_weight=True, epilogue=1 if c.swiglu else 0, numerics=c.numerics)
    assert got == c.family, f"{F.case_id(c)}: the planner says {got!r}"


@pytest.mark.parametrize("r", F.REFUSED, ids=[r[0] for r in F.REFUSED])
def test_plan_of_every_refused_case(r):
    _, m, n, k, g, qtype, dtype, inner, norm, swiglu, _ = r
    assert F.fused_plan(m, n, k, g, qtype, dtype, inner, norm_weight=norm, epilogue=1 if swiglu else 0) is None
    assert F.fused_plan(m, n, k, g, qtype, dtype, inner) is not None      # the stage is what is refused, not the shape


@pytest.mark.parametrize("c", F.STAGE_CASES, ids=F.case_id)
def test_plan_of_every_stage_case(c):
    for norm, epi, bias in ((1, 0, 0), (1, 1, 0), (0, 1, 0), (1, 0, 1), (0, 0, 1), (0, 0, 0)):
        got = F.fused_plan(c.m, c.n, c.k, c.g, c.qtype, c.dtype, c.inner, norm_weight=bool(norm), epilogue=epi, bias=bool(bias),
                           bias_row_stride=c.n + 64 if bias else 0, numerics=c.numerics)
        assert got == c.family, (norm, epi, bias, got)
    for m in (1, 16):   # mx4 carries the residual and SwiGLU (no norm) on the 16-row kernel
        for epi, bias in ((0, 0), (1, 0), (0, 1)):
            assert F.fused_plan(m, 1040, 2048, 32, "mx4", F.BF16, 4, epilogue=epi, bias=bool(bias), bias_row_stride=1040 if bias else 0) == "pair"


def test_stacked_plan_takes_the_persistent_kernel():
    """The launches of test_gpu_fused_f64.py's stacked cases: 192 and more items of 64 rows."""
    for batch in (12, 13):
        for m, k, norm, epi in ((1, 2048, 1, 0), (3, 2048, 1, 0), (1, 4096, 1, 0), (1, 2048, 0, 1), (8, 2048, 0, 1)):
            assert F.fused_plan(m, 1024, k, 128, "any4_rowwise", F.BF16, 4, norm_weight=bool(norm), epilogue=epi, batch=batch) == "pair"


def test_every_template_axis_is_in_a_carried_case():
    """dtype, M, GPS, D, MF of w4_gemv_kernel<.., NORM>; CPG, I of w4_gemm_pair16_kernel<.., NORM>; CPG of the loop kernel's NORM."""
    gemv = [c for c in F.NORM_CASES if c.kernel == "gemv"]
    for dt in (F.BF16, F.F16):
        assert {c.m for c in gemv if c.dtype == dt} >= {1, 2, 3, 4, 5, 8}
        assert {c.g for c in gemv if c.dtype == dt} == {32, 64, 128, 256}                 # GPS = 2 / 1, MF = 0 / 1
        assert any(c.k == 8192 for c in gemv if c.dtype == dt)                            # D = 8
        p16 = [c for c in F.NORM_CASES if c.kernel == "pair16" and c.dtype == dt]
        assert {c.g for c in p16} == {32, 64, 128, 256} and {c.inner for c in p16} == {2, 4}
        assert {c.g for c in F.NORM_CASES if c.kernel == "pair16_loop" and c.dtype == dt} == {64, 128, 256}


def test_distinct_values_and_row_sample():
    for dt in (F.BF16, F.F16):
        v = F.distinct_values(28672, dt)
        assert len(set(F.bits16(v).tolist())) == 28672 and torch.isfinite(v.float()).all() and (v.float() != 0).all()
    rows = F.sample_rows(28672)
    assert rows.min() == 0 and rows.max() == 28671 and len(rows) % 16 == 0 and len(np.unique(rows)) == len(rows)
    assert (np.sort(rows).reshape(-1, 16)[:, 0] % 16 == 0).all()      # whole gate / up blocks


def test_swiglu_of_sums_contains_the_kernels_arithmetic():
    """Sums perturbed inside their allowance and pushed through dg_swiglu's rounding points stay inside the propagated allowance."""
    gen = torch.Generator().manual_seed(2)
    for dt in (F.BF16, F.F16):
        ref = (torch.randn(4, 64, generator=gen) * 3).double().numpy()
        tol = np.abs(ref) * 2.0 ** -8 + 1e-3
        y0, ytol = F.swiglu_of_sums(ref, tol, dt)
        for sgn in (-1, 1):
            s = torch.from_numpy(ref + sgn * tol * 0.4).to(dt)
            gu = F.split_gate_up(s)
            il = gu.shape[1] // 2
            g, u = gu[:, :il].float(), gu[:, il:].float()
            y = ((g / (1 + torch.exp(-g))).to(dt).float() * u).to(dt).double().numpy()
            assert (np.abs(y - y0) <= ytol).all()
