"""CPU suite: LoRA adapters on the decode stack (any4_amd/lora.py) in their plain-torch formulation -- the float64 reference of
tests/lora_ref.py, AdapterSet's loading rules, a `fused=False` stack on dense linears with an adapter per sequence, and LoRALinear's
gradients.  No HIP compute."""
import numpy as np
import pytest
import torch

from any4_amd.decode import DecodeConfig, DecodeStack, DenseFactory, shard_rows
from any4_amd.lora import AdapterSet, LoRALinear, fuse_projections, lora_ref
from tests import lora_ref as R

CFG = dict(hidden=64, inter=96, layers=2, heads=4, kv_heads=2, head_dim=16, vocab=50, max_seq=16, group_size=32, gate_up_interleave=8)
ATOL = 1e-4  # tests/test_decode_cpu.py's tolerance for logits of a float32 stack
BS, RANK, NA = 3, 8, 3


def test_reference_against_a_hand_computed_2x2_case():
    """x = [[1, 2], [3, 4]], A = [[1, 0], [1, 1]] -> t = [[1, 3], [3, 7]]; B = [[1, 1], [0, 2]] -> B t = [[4, 6], [10, 14]]; scale 1/2,
    y_in = 1: row 0 (adapter 0) = [3, 4], row 1 (no adapter) keeps [1, 1].  With ids [0, 0]: row 1 = [6, 8]."""
    x = torch.tensor([[1., 2.], [3., 4.]], dtype=torch.bfloat16)
    A = torch.tensor([[[1., 0.], [1., 1.]]], dtype=torch.bfloat16)
    B = torch.tensor([[[1., 1.], [0., 2.]]], dtype=torch.bfloat16)
    scale = torch.tensor([0.5])
    y = torch.ones(2, 2, dtype=torch.bfloat16)
    for ids, want in (([0, -1], [[3., 4.], [1., 1.]]), ([0, 0], [[3., 4.], [6., 8.]]), ([1, -5], [[1., 1.], [1., 1.]])):
        ref, tol, adapted, t, _ = R.lora_ref64(x, A, B, scale, ids, 1, y)
        assert ref.tolist() == want and adapted.tolist() == [0 <= i < 1 for i in ids]
        assert (tol[~adapted] == 0).all() and (tol[adapted] > 0).all() and (tol < 0.04).all()  # (half a bf16 ulp at 8 is 2^-5)
        got = lora_ref(x, A, B, scale, torch.tensor(ids, dtype=torch.int32), 1, y.clone())
        assert got.tolist() == want
    assert R.lora_ref64(x, A, B, scale, [0], 2, y)[0].tolist() == [[3., 4.], [6., 8.]]  # rows_per_id = 2: one id for both rows
    assert R.shrink_ref64(x, A, [0, -1], 1)[0].tolist() == [[1., 3.], [0., 0.]]


def test_reference_norm_flavour_is_the_sum_convention():
    """t = rs A RNE16(x g): against the formula spelled out in float64 on a random case, and the torch definition inside the bound."""
    x, g, A, B, scale, y = R.make_case(5, 64, 8, 16, torch.bfloat16)
    ids = [0, -1, 2, 1, 3]
    ref, tol, adapted, t, t_tol = R.lora_ref64(x, A, B, scale, ids, 1, y, g)
    xt = (x.float() * g.float()).to(torch.bfloat16).double()
    rs = torch.rsqrt((x.double() ** 2).mean(1) + float(np.float32(R.EPS)))
    for i, a in enumerate(ids):
        if 0 <= a < 3:
            np.testing.assert_allclose(t[i], (rs[i] * (A[a].double() @ xt[i])).numpy(), rtol=1e-12)
    got = lora_ref(x, A, B, scale, torch.tensor(ids, dtype=torch.int32), 1, y.clone(), g, R.EPS)
    assert (np.abs(got.double().numpy() - ref) <= tol).all()
    assert torch.equal(got[~torch.from_numpy(adapted)], y[~torch.from_numpy(adapted)])


def _adapter(cfg, rank, seed, targets=("qkv", "o", "gate_up", "down"), dtype=torch.float32, gain=1.0):
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for layer in range(cfg.layers):
        for name, n, k in cfg.linear_shapes():
            if name in targets:
                out[layer, name] = ((torch.randn(rank, k, generator=gen) / k ** 0.5).to(dtype), (gain * torch.randn(n, rank, generator=gen) / rank ** 0.5).to(dtype))
    return out


def test_adapter_set_load_pads_permutes_and_clears():
    cfg = DecodeConfig(**CFG)
    aset = AdapterSet(cfg, NA, RANK, "cpu", torch.bfloat16)
    w = _adapter(cfg, 3, seed=1, dtype=torch.bfloat16)
    aset.load(1, w, alpha=6.0)
    perm = shard_rows(cfg, "gate_up", 0, 1)
    assert not torch.equal(perm, torch.arange(2 * cfg.inter))  # (the 8 + 8 interleave is a real permutation here)
    for (layer, name), (A, B) in w.items():
        dA, dB, ds = aset.tensors(layer, name)
        assert dA.shape == (NA, RANK, A.shape[1]) and dB.shape == (NA, B.shape[0], RANK) and ds.tolist() == [0, 2.0, 0]  # alpha / r'
        assert torch.equal(dA[1, :3], A) and not dA[1, 3:].any() and not dA[0].any() and not dA[2].any()
        assert torch.equal(dB[1, :, :3], B[perm] if name == "gate_up" else B) and not dB[1, :, 3:].any() and not dB[0].any()
    ptr = aset.tensors(0, "qkv")[0].data_ptr()
    aset.load(1, {(0, "o"): w[0, "o"]}, alpha={(0, "o"): 3.0})  # a re-load replaces the slot, in place
    assert aset.tensors(0, "qkv")[0].data_ptr() == ptr and not aset.tensors(0, "qkv")[0].any()
    assert aset.tensors(0, "o")[2].tolist() == [0, 1.0, 0]
    aset.clear(1)
    assert all(not t.any() for key in w for t in aset.tensors(*key))
    with pytest.raises(ValueError):
        aset.load(3, w, 1.0)
    with pytest.raises(ValueError):
        aset.load(0, {(0, "qkv"): (torch.zeros(RANK + 1, cfg.hidden), torch.zeros(128, RANK + 1))}, 1.0)
    with pytest.raises(ValueError):
        aset.load(0, {(5, "qkv"): w[0, "qkv"]}, 1.0)
    with pytest.raises(ValueError):
        AdapterSet(cfg, NA, 12, "cpu")


def test_fuse_projections_equals_separate_projections():
    gen = torch.Generator().manual_seed(3)
    k, parts = 32, []
    for n, r in ((24, 2), (8, 3), (8, 1)):
        parts.append((torch.randn(r, k, generator=gen, dtype=torch.float64), torch.randn(n, r, generator=gen, dtype=torch.float64)))
    A, B = fuse_projections(parts)
    assert A.shape == (6, k) and B.shape == (40, 6)
    x = torch.randn(5, k, generator=gen, dtype=torch.float64)
    want = torch.cat([(x @ a.t()) @ b.t() for a, b in parts], dim=1)
    assert torch.allclose((x @ A.t()) @ B.t(), want, rtol=1e-12, atol=1e-12)


def _stacks(dtype=torch.float32, bs=BS, **kw):
    cfg = DecodeConfig(**CFG)
    aset = AdapterSet(cfg, NA, RANK, "cpu", dtype)
    plain = DecodeStack(cfg, DenseFactory(cfg, "cpu", dtype, seed=3), "cpu", dtype, bs=bs, seed=7, fused=False, **kw)
    adapted = DecodeStack(cfg, DenseFactory(cfg, "cpu", dtype, seed=3), "cpu", dtype, bs=bs, seed=7, fused=False, adapters=aset, **kw)
    return cfg, aset, plain, adapted


def _tokens(cfg, bs, T, seed=0):
    return torch.randint(0, cfg.vocab, (bs, T), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stack_without_an_adapter_is_the_plain_stack_bit_for_bit(dtype):
    """All ids -1, and a loaded adapter whose B is zero: logits bit for bit those of a stack built without `adapters=`."""
    cfg, aset, plain, adapted = _stacks(dtype)
    zero_b = {key: (A, torch.zeros_like(B)) for key, (A, B) in _adapter(cfg, RANK, 2, dtype=dtype).items()}
    aset.load(0, _adapter(cfg, RANK, 1, dtype=dtype), alpha=16.0)
    aset.load(2, zero_b, alpha=16.0)
    toks = _tokens(cfg, BS, 4)
    assert adapted.adapter_ids.tolist() == [-1] * BS and adapted.adapter_ids.dtype == torch.int32
    for i in range(4):
        want = plain.decode(toks[:, i], i)
        assert torch.equal(adapted.decode(toks[:, i], i, adapters=[-1, -1, -1] if i == 0 else None), want)
    _, _, _, zb = _stacks(dtype)
    zb.adapters.load(2, zero_b, alpha=16.0)
    _, _, plain2, _ = _stacks(dtype)
    for i in range(4):
        assert torch.equal(zb.decode(toks[:, i], i, adapters=[2, -1, 2]), plain2.decode(toks[:, i], i))


def test_stack_adapter_is_per_sequence():
    """ids [a, -1, b]: row 0 is bit for bit the run with [a, a, a], row 1 the plain stack's, row 2 the run with [b, b, b]; and the adapter
    matters (the logits move by far more than the float32 noise)."""
    cfg, aset, plain, mixed = _stacks()
    _, _, _, all_a = _stacks()
    _, _, _, all_b = _stacks()
    for s in (aset, all_a.adapters, all_b.adapters):
        s.load(0, _adapter(cfg, RANK, 1), alpha=16.0)
        s.load(2, _adapter(cfg, 5, 2), alpha=10.0)
    toks = _tokens(cfg, BS, 3)
    for i in range(3):
        got = mixed.decode(toks[:, i], i, adapters=[0, -1, 2])
        a, b, p = all_a.decode(toks[:, i], i, adapters=[0, 0, 0]), all_b.decode(toks[:, i], i, adapters=[2, 2, 2]), plain.decode(toks[:, i], i)
        assert torch.equal(got[0], a[0]) and torch.equal(got[1], p[1]) and torch.equal(got[2], b[2])
        assert (got[0] - p[0]).abs().max() > 100 * ATOL and (got[2] - p[2]).abs().max() > 100 * ATOL


def test_prefill_then_decode_equals_token_by_token_decode():
    cfg, aset, _, a = _stacks()
    _, _, _, b = _stacks()
    for s in (aset, b.adapters):
        s.load(0, _adapter(cfg, RANK, 1), alpha=16.0)
        s.load(1, _adapter(cfg, 4, 2), alpha=8.0)
    ids, T = [1, -1, 0], 5
    toks = _tokens(cfg, BS, T + 2)
    got = a.prefill(toks[:, :T], adapters=ids)
    assert a.adapter_ids.tolist() == ids and a.prefill_adapter_ids.tolist() == ids
    for i in range(T):
        want = b.decode(toks[:, i], i, adapters=ids)
    assert torch.allclose(got, want, atol=ATOL), (got - want).abs().max()
    for i in range(T, T + 2):  # the decode steps behind the prefill keep its adapters without being told
        got, want = a.decode(toks[:, i], i), b.decode(toks[:, i], i)
        assert torch.allclose(got, want, atol=ATOL), (i, (got - want).abs().max())
    chunked = _stacks()[3]
    chunked.adapters.load(0, _adapter(cfg, RANK, 1), alpha=16.0)
    chunked.adapters.load(1, _adapter(cfg, 4, 2), alpha=8.0)
    got = chunked.prefill(toks[:, :T], adapters=ids, chunk=2)
    want = a.prefill(toks[:, :T], adapters=ids)
    assert torch.allclose(got, want, atol=ATOL)


def test_generate_and_prefill_slots_keep_the_ids():
    cfg, aset, _, a = _stacks(ragged=True)
    _, _, _, b = _stacks(ragged=True)
    for s in (aset, b.adapters):
        s.load(0, _adapter(cfg, RANK, 1), alpha=16.0)
        s.load(2, _adapter(cfg, 4, 2), alpha=8.0)
    prompts = [_tokens(cfg, 1, n, seed=n)[0] for n in (4, 2, 5)]
    ids = [2, 0, -1]
    out = a.generate(prompts, 4, adapters=ids)
    assert a.adapter_ids.tolist() == ids
    # the manual loop: a prefill with slots in another order, then decode steps that are never told an adapter
    order = [2, 0, 1]
    T = max(p.numel() for p in prompts)
    padded = torch.zeros(BS, T, dtype=torch.long)
    for row, sl in enumerate(order):
        padded[row, : prompts[sl].numel()] = prompts[sl]
    logits = b.prefill(padded, position=0, lengths=[prompts[sl].numel() for sl in order], slots=order, adapters=[ids[sl] for sl in order])
    assert b.adapter_ids.tolist() == ids
    tok = torch.empty(BS, dtype=torch.long)
    tok[order] = logits.argmax(-1)
    want = [tok.clone()]
    for i in range(3):
        tok = b.decode(tok, [p.numel() + i for p in prompts]).argmax(-1)
        want.append(tok.clone())
    assert torch.equal(out, torch.stack(want, dim=1))
    # and the adapters did something: the same prompts without them continue differently somewhere, or the logits differ
    plain = _stacks(ragged=True)[2]
    assert not torch.allclose(plain.prefill(padded, position=0, lengths=[prompts[sl].numel() for sl in order], slots=order), logits, atol=100 * ATOL)


def test_host_refusals():
    cfg, aset, plain, adapted = _stacks()
    toks = _tokens(cfg, BS, 2)
    with pytest.raises(ValueError):
        plain.decode(toks[:, 0], 0, adapters=[0, 0, 0])      # a stack without an AdapterSet
    with pytest.raises(ValueError):
        adapted.decode(toks[:, 0], 0, adapters=[0, NA, 0])   # id >= n_adapters
    with pytest.raises(ValueError):
        adapted.decode(toks[:, 0], 0, adapters=[0, 0])       # one id per sequence
    with pytest.raises(ValueError):
        adapted.prefill(toks, adapters=[0, 1, 7])
    with pytest.raises(ValueError):
        adapted.generate(toks, 2, adapters=[0])
    with pytest.raises(ValueError):
        adapted.set_adapters([0, 1, NA])
    assert adapted.adapter_ids.tolist() == [-1] * BS          # nothing was written by a refused call
    adapted.set_adapters([0, -7, 2])
    assert adapted.adapter_ids.tolist() == [0, -1, 2]
    adapted.set_adapters([-1] * BS)
    with pytest.raises(ValueError):
        DecodeStack(cfg, DenseFactory(cfg, "cpu", torch.float32), "cpu", torch.float32, bs=BS, fused=False, adapters=aset, rank=0, world=2)
    other = AdapterSet(DecodeConfig(**dict(CFG, inter=128)), NA, RANK, "cpu", torch.float32)
    with pytest.raises(ValueError):
        DecodeStack(cfg, DenseFactory(cfg, "cpu", torch.float32), "cpu", torch.float32, bs=BS, fused=False, adapters=other)


def test_scratch_never_releases_a_buffer_it_handed_out():
    """A captured step holds the address of the scratch it was captured on (bs rows) and writes there at every replay; a later prefill
    brings more rows.  The set must grow WITHOUT giving the earlier buffer back to the allocator, and rows that fit reuse a buffer."""
    import gc
    import weakref

    cfg = DecodeConfig(**CFG)
    aset = AdapterSet(cfg, NA, RANK, "cpu", torch.float32)
    first = aset.scratch(BS)
    assert first.shape == (BS, RANK) and first.dtype == torch.float32
    alive, ptr = weakref.ref(first._base), first.data_ptr()
    del first
    assert aset.scratch(BS - 1).data_ptr() == ptr       # fits: the same memory
    big = aset.scratch(40 * BS)                          # a prefill's rows
    assert big.shape == (40 * BS, RANK) and big.data_ptr() != ptr
    gc.collect()
    assert alive() is not None and alive().data_ptr() == ptr, "the buffer a captured step may have seen was released"
    assert aset.scratch(BS).data_ptr() == big.data_ptr() == aset.scratch(40 * BS).data_ptr()  # no further growth, no further buffers
    assert len(aset._buffers) == 2


def test_lora_linear_refuses_a_base_whose_output_is_not_contiguous():
    """The delta lands in place through a 2-D view of the base's output; a non-contiguous output would be updated in a copy and returned
    without the delta, so it is refused on the CPU as on the GPU."""
    class Strided(torch.nn.Linear):
        def forward(self, x):
            return super().forward(x).t().contiguous().t()  # the right values, column-major

    mod = LoRALinear(Strided(16, 8, bias=False), rank=8, alpha=8.0)
    with torch.no_grad():
        mod.B.normal_()
        x = torch.randn(4, 16)
        assert not mod.base(x).is_contiguous()
        with pytest.raises(RuntimeError):
            mod(x)
        x3 = torch.randn(2, 3, 16)  # a contiguous 3-D output: in place through the view
        ok = LoRALinear(torch.nn.Linear(16, 8, bias=False), rank=8, alpha=8.0)
        ok.B.normal_()
        assert torch.allclose(ok(x3), ok.base(x3) + (x3 @ ok.A.t()) @ ok.B.t(), atol=1e-5)


def test_adapter_set_on_another_device_is_refused():
    cfg = DecodeConfig(**CFG)
    elsewhere = AdapterSet(cfg, NA, RANK, "meta", torch.float32)
    with pytest.raises(ValueError):
        DecodeStack(cfg, DenseFactory(cfg, "cpu", torch.float32), "cpu", torch.float32, bs=BS, fused=False, adapters=elsewhere)


def test_launch_counts_with_adapters():
    cfg, aset, plain, adapted = _stacks()
    assert plain.layers[0].launches() + 8 == adapted.layers[0].launches()
    two = AdapterSet(cfg, NA, RANK, "cpu", torch.float32, targets=("qkv", "down"))
    s = DecodeStack(cfg, DenseFactory(cfg, "cpu", torch.float32), "cpu", torch.float32, bs=BS, fused=False, adapters=two)
    assert s.layers[0].launches() == plain.layers[0].launches() + 4


def test_lora_linear_gradients_against_the_dense_formula():
    """dA, dB (and dx) of y = base(x) + s B A x against autograd on the dense twin y = x (W + s B A)^T, float64."""
    gen = torch.Generator().manual_seed(5)
    base = torch.nn.Linear(24, 40, bias=False, dtype=torch.float64)
    base.weight.requires_grad_(False)
    mod = LoRALinear(base, rank=8, alpha=16.0)
    assert mod.A.dtype == torch.float64 and not mod.B.any()
    with torch.no_grad():
        mod.B.copy_(torch.randn(40, 8, generator=gen, dtype=torch.float64))
    x = torch.randn(6, 24, generator=gen, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(6, 40, generator=gen, dtype=torch.float64)
    (mod(x) * dy).sum().backward()
    A2, B2, x2 = (t.detach().clone().requires_grad_(True) for t in (mod.A, mod.B, x))
    ((x2 @ (base.weight + 2.0 * B2 @ A2).t()) * dy).sum().backward()
    for got, want in ((mod.A.grad, A2.grad), (mod.B.grad, B2.grad), (x.grad, x2.grad)):
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-12), (got - want).abs().max()
    with torch.no_grad():  # the serving form of the same module (lora_ref on the CPU: f32 sums) agrees with the training form
        assert torch.allclose(mod(x), mod.base(x) + 2.0 * (x @ mod.A.t()) @ mod.B.t(), rtol=1e-5, atol=1e-5)


def test_load_modules_serves_what_was_trained():
    cfg = DecodeConfig(**CFG)
    aset = AdapterSet(cfg, NA, RANK, "cpu", torch.float32)
    base = torch.nn.Linear(cfg.hidden, cfg.hidden, bias=False)
    mod = LoRALinear(base, rank=4, alpha=8.0, seed=2)
    with torch.no_grad():
        mod.B.normal_()
    aset.load_modules(2, {(1, "o"): mod})
    A, B, s = aset.tensors(1, "o")
    assert torch.equal(A[2, :4], mod.A) and torch.equal(B[2, :, :4], mod.B) and s.tolist() == [0, 0, 2.0]


def test_abi_preconditions_fail_before_any_launch():
    """dg_lora_shrink / dg_lora_expand answer a TG_E_* code for anything outside their contract without touching HIP."""
    from any4_amd import _lib

    L = _lib.load()
    p = 4096

    def shrink(x=p, g=None, A=p, idx=p, t=p, m=1, k=64, r=8, na=1, rpi=1, dt=0):
        return L.dg_lora_shrink(x, g, A, idx, t, m, k, r, na, rpi, 1e-5, dt, -1, None)

    def expand(t=p, B=p, sc=p, idx=p, y=p, m=1, n=64, r=8, ldy=64, na=1, rpi=1, dt=0):
        return L.dg_lora_expand(t, B, sc, idx, y, m, n, r, ldy, na, rpi, dt, -1, None)

    assert shrink(x=None) == shrink(A=None) == shrink(idx=None) == shrink(t=None) == -1
    assert expand(t=None) == expand(B=None) == expand(sc=None) == expand(idx=None) == expand(y=None) == -1
    assert shrink(dt=2) == expand(dt=2) == -5
    for bad in (dict(m=0), dict(r=4), dict(r=12), dict(r=72), dict(na=0), dict(rpi=0)):
        assert shrink(**bad) == -7 and expand(**bad) == -7, bad
    assert shrink(k=0) == -7 and shrink(k=68) == -3 and shrink(k=(1 << 17) + 8) == -10 and shrink(m=1 << 31) == -10
    assert expand(n=0) == -7 and expand(n=68, ldy=72) == -7 and expand(ldy=56) == -7 and expand(ldy=68) == -7
    assert shrink(x=p + 8) == shrink(A=p + 2) == shrink(t=p + 4) == shrink(g=p + 8) == shrink(idx=p + 2) == -8
    assert expand(t=p + 4) == expand(B=p + 8) == expand(y=p + 2) == expand(sc=p + 2) == expand(idx=p + 1) == -8
