"""Checks of the checker (no GPU): the builders and float64 references of tests/glue_ref.py that tests/test_gpu_glue_f64.py relies on.

* the lookup / decoy builders meet their margin condition at every shape the GPU file uses;
* on lookup cases the float64 reference and the 16-bit torch formulations return the target V rows bit for bit;
* the float64 references agree with the existing torch formulations (any4_amd/decode.py) within derived bounds;
* the rope sample of the GPU file is large enough: at its element count, `decode._rope` and either single-FMA contraction of the
  same expression differ in at least 20 elements per type."""
import math

import pytest
import torch

from tests import glue_ref as R

DTYPES = [torch.bfloat16, torch.float16]


def _probe_shapes():
    """Every (bs, hl, kvl, d, S, T, p0, seed) the GPU file builds a lookup / decoy case at."""
    shapes = []
    for bs, (hl, kvl, d) in R.probe_geometries():
        for T, p0, S in R.prefill_chunks((hl, kvl, d), bs):
            shapes.append((bs, hl, kvl, d, S, T, p0, R.case_seed(T, p0)))
    for bs, (hl, kvl, d) in R.probe_geometries(decode=True):
        for pos, S, _ in R.decode_positions((hl, kvl, d), bs):
            shapes.append((bs, hl, kvl, d, S, 1, pos, R.case_seed(1, pos)))
    return shapes


def test_lookup_and_decoy_margins_at_every_gpu_shape():
    """attn_case asserts the margin itself; bf16 and fp16 hold the same +-1 / 2^-4 values, so one type covers the condition."""
    worst = {}
    shapes = _probe_shapes()
    assert len(shapes) > 100
    for bs, hl, kvl, d, S, T, p0, seed in shapes:
        for kind in ("lookup", "decoy"):
            c = R.attn_case(kind, torch.bfloat16, bs, hl, kvl, d, S, T, p0, seed)
            assert c.margin >= R.MARGIN and c.beta <= 16, (kind, bs, hl, kvl, d, S, T, p0)
            # off-target weight: at most (positions) e^-margin, times |V| <= 4, below half a bf16 spacing at the smallest |V| = 2^-4
            assert (p0 + T) * math.exp(-c.margin) * 4 <= 0.5 * 2.0 ** -4 * 2.0 ** -7 * (1 + 1e-9)
            key = (kind, d)
            worst[key] = min(worst.get(key, float("inf")), c.margin)
    print("smallest margins", worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,beta", [(64, 6), (128, 4)])
def test_lookup_rows_are_reproduced_bit_for_bit_by_both_references(dtype, d, beta):
    """bs = 2, 8 / 2 heads, S = 1024, T = 300, p0 = 257: attn_ref64 (rounded once), the 16-bit formulation of glue_ref and
    prefill_attention_torch all return V[target]; so does a decode-shaped case."""
    from any4_amd.decode import prefill_attention_torch

    c = R.attn_case("lookup", dtype, 2, 8, 2, d, 1024, 300, 257, seed=1, beta_min=beta)
    assert c.margin >= R.MARGIN
    want = c.want.view(c.bs, c.T, c.hl, c.d)
    assert R.same_bits(R.case_ref64(c).to(dtype), want)
    assert R.same_bits(R.case_torch16(c), want)
    kc, vc = c.kc0.clone(), c.vc0.clone()
    got = prefill_attention_torch(c.qkv, c.cos, c.sin, c.p0, kc, vc, c.hl, c.kvl, c.d, c.T)
    assert R.same_bits(got, c.want)
    ek, ev = R.expected_caches(c)
    assert R.same_bits(kc, ek) and R.same_bits(vc, ev)
    # targets really cycle through the edges: own, own - 1, 0, tile edges, chunk start, prefix end
    pos = torch.arange(c.p0, c.p0 + c.T).view(1, -1, 1)
    for edge in (pos, pos - 1, torch.zeros_like(pos), pos // 64 * 64, pos // 64 * 64 - 1, torch.full_like(pos, c.p0), torch.full_like(pos, c.p0 - 1),
                 pos // 32 * 32, pos // 256 * 256 - 1):
        assert (c.target == edge).any()
    assert (c.target <= pos).all() and (c.target >= 0).all()
    one = R.attn_case("lookup", dtype, 3, 6, 2, d, 1024, 1, 257, seed=2)
    assert R.same_bits(R.case_ref64(one).to(dtype), one.want.view(3, 1, 6, d)) and R.same_bits(R.case_torch16(one), one.want.view(3, 1, 6, d))


@pytest.mark.parametrize("dtype", DTYPES)
def test_decoy_rows_differ_grossly_from_the_hidden_row(dtype):
    """What a kernel that sees the decoy would return (V[p + 1]) misses the float64 expectation by O(1) of the row's size: far
    outside any allowance of the GPU file (which is a few 16-bit roundings)."""
    for T, p0 in ((40, 70), (1, 256)):
        c = R.attn_case("decoy", dtype, 2, 6, 2, 64, 512, T, p0, seed=3)
        ref = R.case_ref64(c)
        assert torch.isfinite(ref).all() and (c.target[:, :-1] == torch.arange(p0 + 1, p0 + T).view(1, -1, 1)).all()
        assert (c.target[:, -1] == p0 + T).all() and torch.isfinite(c.kc0[:, :, p0 + T].float()).all()
        assert torch.isnan(c.kc0[:, :, p0 + T + 1:].float()).all() and torch.isnan(c.kc0[:, :, p0:p0 + T].float()).all()
        kvh = torch.arange(c.hl) // c.rep
        seen = c.v_all[:, kvh][:, :, p0 + 1:p0 + T + 1].transpose(1, 2)          # [bs, T, hl, d]: the hidden rows
        assert R.row_err(seen, ref).min() > 0.25
    # a chunk that ends at max_seq has no row behind it: its last token looks itself up
    c = R.attn_case("decoy", dtype, 1, 2, 1, 64, 128, 8, 120, seed=4)
    assert (c.target[:, -1] == -1).all() and c.k_all.shape[2] == 128


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["peaked", "normal"])
def test_attention_references_agree(dtype, kind):
    """attn_torch16 is prefill_attention_torch's formulation (the same roundings; matmul shapes differ, so not the same bits), and
    both are within a few 16-bit roundings of attn_ref64.  Derived bound per row and element: the 16-bit score carries |score| u,
    which the exponential turns into a relative error of every weight and of their sum (2 max|score| u); the probability and the
    P . V accumulation add u each -- all of it times sum_s p_s |v_s| (there is cancellation in sum_s p_s v_s) -- and the output
    rounding adds u |ref|."""
    from any4_amd.decode import prefill_attention_torch

    u = R.unit_roundoff(dtype)
    c = R.attn_case(kind, dtype, 2, 4, 2, 64, 512, 130, 70, seed=5)
    ref, t16 = R.case_ref64(c), R.case_torch16(c)
    mass = R.attn_ref64(c.q16, c.k_all, c.v_all.abs(), c.visible, c.rep, c.scale)
    kc, vc = c.kc0.clone(), c.vc0.clone()
    pt = prefill_attention_torch(c.qkv, c.cos, c.sin, c.p0, kc, vc, c.hl, c.kvl, c.d, c.T).view(c.bs, c.T, c.hl, c.d)
    ek, ev = R.expected_caches(c)
    assert R.same_bits(kc, ek) and R.same_bits(vc, ev)
    kvh = torch.arange(c.hl) // c.rep
    smax = (torch.einsum("bthd,bhsd->bths", c.q16.double(), c.k_all[:, kvh].double()).abs().max() * c.scale).item()
    bound = u * ((2 + 2 * smax) * mass + ref.abs())
    for name, got in (("attn_torch16", t16), ("prefill_attention_torch", pt)):
        err = (got.double() - ref).abs()
        print(f"{kind} {dtype} {name}: max|score| {smax:.1f}, largest error / bound {(err / bound).max().item():.3f}, "
              f"largest row error {R.row_err(got, ref).max().item() / u:.2f} u")
        assert (err <= bound).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_and_swiglu_references_agree_with_the_torch_formulations(dtype):
    """The 16-bit torch formulations (decode.RMSNorm, silu * up) round twice, so they sit inside two_roundings_bound of the float64
    references -- the bound the kernels are held to."""
    from any4_amd.decode import RMSNorm

    gen = torch.Generator().manual_seed(0)
    for dim in (8, 64, 2040, 4096):
        h, dl = torch.randn(5, dim, generator=gen).to(dtype), torch.randn(5, dim, generator=gen).to(dtype)
        norm = RMSNorm(dim, 1e-5, "cpu", dtype)
        norm.weight.data = (torch.rand(dim, generator=gen) - 0.5).to(dtype)
        for delta in (dl, None):
            hs, y64 = R.rmsnorm_ref64(h, delta, norm.weight, 1e-5)
            assert R.same_bits(hs, h if delta is None else h + dl)
            assert ((norm(hs).double() - y64).abs() <= R.two_roundings_bound(y64, dtype)).all()
    gu = R.swiglu_input(dtype, 3, 512, "cpu")
    ref = R.swiglu_ref64(gu)
    want = torch.nn.functional.silu(gu[:, :512]) * gu[:, 512:]
    big = ref.abs() > torch.finfo(dtype).max
    assert (((want.double() - ref).abs() <= R.two_roundings_bound(ref, dtype)) | big).all()
    assert (want[big].double() == torch.sign(ref[big]) * float("inf")).all()
    if dtype == torch.float16:
        assert big.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_sample_is_large_enough_to_see_one_contracted_product(dtype):
    """At the element count of test_rope_bits_at_scale (per kernel and type; here the smallest of them), _rope and either single-FMA
    variant of the same expression differ in at least 20 elements after the rounding to 16 bit: a kernel compiled with one product
    contracted cannot pass that test by sample size."""
    n = min(R.rope_elements(kernel) for kernel in R.ROPE_KERNELS)
    assert n >= 1 << 22
    d, S = 128, 8192
    cos, sin = R.rope_tables(d, S)
    rows = n // d
    gen = torch.Generator().manual_seed(1)
    pos = torch.randint(0, S, (rows,), generator=gen)
    x = torch.randn(rows, d, generator=gen).to(dtype)
    want = R._rope(x, cos[pos], sin[pos])
    first, second = R.rope_fma_variants(x, cos[pos], sin[pos])
    n1 = int((first.view(torch.int16) != want.view(torch.int16)).sum())
    n2 = int((second.view(torch.int16) != want.view(torch.int16)).sum())
    print(f"{dtype}: {rows * d} elements, mismatches fma-first {n1}, fma-second {n2}")
    assert n1 >= 20 and n2 >= 20
