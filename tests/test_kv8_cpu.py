"""CPU suite: the mx8 KV-cache format (any4_amd/kvcache.py: E4M3 codes, one E8M0 exponent byte per 32 elements) -- the properties of
the host encoder that defines it -- and DecodeStack(..., kv_cache="mx8") in its plain-torch formulation: prefill + decode, ragged and
not, cache slots, generate with eos, host refusals, and the C ABI of the four mx8 entry points (declared, exported, bound).
Float32 stack on the tests-only dense linears of tests/test_decode_cpu.py; no HIP compute."""
import os

import pytest
import torch

from any4_amd.decode import DecodeConfig, DecodeStack
from any4_amd.kvcache import F8, mx8_decode, mx8_encode, mx8_scale
from tests.test_decode_cpu import CFG, SeededDense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG8 = dict(CFG, head_dim=32)  # (the suite's tiny configuration has head_dim 16: below one block)
ENTRIES = ("dg_rope_attn_split_mx8", "dg_rope_attn_split_mx8_seq", "dg_prefill_attn_mx8", "dg_prefill_attn_mx8_seq")


def _rows(dtype, n=2048, d=128, seed=0):
    """Log-normally scaled rows (row scales over ~ +-13 binades), inside fp16's range."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=gen) * torch.exp(torch.randn(n, 1, generator=gen).clamp(-3, 3) * 1.5)
    return x.to(dtype)


def _blocks(x):
    return x.float().reshape(*x.shape[:-1], x.shape[-1] // 32, 32)


# ---------------------------------------------------------------- the encoder
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_encoder_never_clips_and_errs_at_most_a_sixteenth_of_the_block_maximum(dtype):
    x = _rows(dtype)
    codes, exps = mx8_encode(x)
    assert codes.dtype == F8 and codes.shape == x.shape and exps.dtype == torch.uint8 and exps.shape == (x.shape[0], x.shape[1] // 32)
    amax = _blocks(x).abs().amax(-1)
    scaled = amax.double() / mx8_scale(exps).double()
    assert (scaled <= 448).all(), scaled.max()
    assert (scaled[amax > 0] > 224).all()  # ... and it is the SMALLEST such power of two
    y = mx8_decode(codes, exps, torch.float32)
    err = (_blocks(y) - _blocks(x)).abs().amax(-1) / amax
    assert err.max() <= 1 / 16, err.max()
    # the codes themselves: nearest E4M3 value to the scaled element (ties to even is torch's cast; here: no other code is closer)
    grid = torch.arange(256, dtype=torch.uint8).view(F8).float()
    grid = grid[torch.isfinite(grid)]
    s = (_blocks(x) / mx8_scale(exps).unsqueeze(-1))[:64].reshape(-1, 1).double()
    best = (s - grid.double().view(1, -1)).abs().min(-1).values
    mine = (s.view(-1) - codes[:64].float().view(-1).double()).abs()
    assert torch.equal(mine, best)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_decoded_values_are_exact_in_the_16_bit_type_and_re_encoding_keeps_them(dtype):
    x = _rows(dtype, seed=1)
    codes, exps = mx8_encode(x)
    y32, y16 = mx8_decode(codes, exps, torch.float32), mx8_decode(codes, exps, dtype)
    assert torch.equal(y16.float(), y32)
    c2, e2 = mx8_encode(y16)
    assert torch.equal(mx8_decode(c2, e2, dtype).view(torch.int16), y16.view(torch.int16))  # the same values ...
    assert (e2.int() - exps.int()).abs().max() <= 1 and (e2 <= exps).all()                     # ... from an exponent at most one lower
    c3, e3 = mx8_encode(mx8_decode(c2, e2, dtype))
    assert torch.equal(mx8_decode(c3, e3, dtype).view(torch.int16), y16.view(torch.int16))


def test_zero_blocks_nan_blocks_clamped_exponents_and_the_clamp_before_the_cast():
    x = torch.randn(4, 64)
    x[0, :32] = 0
    x[1, 40] = float("nan")
    x[2, 3] = float("inf")
    x[3, :32] = torch.randn(32) * 2.0 ** -140  # far below 2^-127 * 2^-9: the exponent byte clamps at 0
    x[3, 32:] = torch.randn(32) * 2.0 ** 120
    codes, exps = mx8_encode(x)
    y = mx8_decode(codes, exps, torch.float32)
    assert exps[0, 0] == 0 and (codes[0, :32].view(torch.uint8) == 0).all() and (y[0, :32] == 0).all()
    assert exps[1, 1] == 255 and torch.isnan(y[1, 32:]).all() and torch.isfinite(y[1, :32]).all() and exps[1, 0] < 255
    assert exps[2, 0] == 255 and torch.isnan(y[2, :32]).all() and torch.isfinite(y[2, 32:]).all()
    assert (codes[1, 32:].view(torch.uint8) == 0x7F).all()
    assert exps[3, 0] == 0 and torch.isfinite(y[3]).all() and 239 <= exps[3, 1] <= 254
    # a code of an exponent-255 block decodes to NaN whatever its bits; an exponent of 0 is 2^-127
    one = torch.full((1, 32), 1.0).to(F8)
    assert torch.isnan(mx8_decode(one, torch.tensor([[255]], dtype=torch.uint8), torch.float32)).all()
    assert (mx8_decode(one, torch.tensor([[0]], dtype=torch.uint8), torch.float32) == 2.0 ** -127).all()
    # 465 would become NaN in torch's own cast; a block maximum just above a power of two puts elements there without the clamp
    assert torch.isnan(torch.tensor([465.0]).to(F8).float()).all()
    b = torch.full((1, 32), 0.8751)  # m > 0.875: the rule steps one exponent up instead of clipping
    c, e = mx8_encode(b)
    assert e[0, 0] == 127 - 8 and torch.isfinite(c.float()).all() and mx8_decode(c, e, torch.float32)[0, 0] == 0.875
    with pytest.raises(ValueError, match="multiple of 32"):
        mx8_encode(torch.zeros(2, 48))
    with pytest.raises(ValueError, match="belong together"):
        mx8_decode(codes, exps[:, :1], torch.float32)


def test_textbook_exponent_rule_would_clip():
    """Why e is not floor(log2 amax) - 8: with it, a maximum of 1.9 * 2^k is scaled to 486 and clips to 448 (8 %)."""
    amax = torch.tensor([1.9])
    e_textbook = torch.floor(torch.log2(amax)) - 8
    assert (amax / 2.0 ** e_textbook > 448).all()
    c, e = mx8_encode(torch.full((1, 32), 1.9))
    assert abs(mx8_decode(c, e, torch.float32)[0, 0] - 1.9) <= 1.9 / 16


# ---------------------------------------------------------------- the plain-torch mx8 stack
def _stack(cfg, bs, ragged=False, kv_cache="mx8"):
    return DecodeStack(cfg, SeededDense(cfg, 0, 1), "cpu", torch.float32, bs=bs, seed=7, ragged=ragged, kv_cache=kv_cache)


def _tokens(cfg, bs, T, seed=0):
    return torch.randint(0, cfg.vocab, (bs, T), generator=torch.Generator().manual_seed(seed))


def _cache_state(stack):
    return [tuple(t.view(torch.uint8).clone() for t in (l.k_cache, l.v_cache, l.k_exp, l.v_exp)) for l in stack.layers]


def test_mx8_stack_tensors_and_bytes():
    cfg = DecodeConfig(**CFG8)
    s8, s16 = _stack(cfg, 2), _stack(cfg, 2, kv_cache=None)
    for layer in s8.layers:
        assert layer.k_cache.dtype == F8 and layer.v_cache.dtype == F8 and layer.k_exp.dtype == torch.uint8
        assert layer.k_cache.shape == (2, cfg.kv_heads, cfg.max_seq, 32) and layer.k_exp.shape == (2, cfg.kv_heads, cfg.max_seq, 1)
        assert all(t.element_size() == 1 for t in (layer.k_cache, layer.v_cache, layer.k_exp, layer.v_exp))
    assert s16.layers[0].k_exp is None and s16.layers[0].k_cache.dtype == torch.float32
    # against a 16-bit cache of the same shape: (1 + 1/32) / 2
    assert s8.kv_cache_bytes() * 4 * 32 == s16.kv_cache_bytes() * 33  # (the float32 twin holds 4 bytes per element)


def test_mx8_prefill_then_decode_equals_token_by_token_and_stays_near_the_unquantised_stack():
    cfg = DecodeConfig(**CFG8)
    bs, T, steps = 2, 7, 3
    toks = _tokens(cfg, bs, T + steps, seed=3)
    a, b, ref = _stack(cfg, bs), _stack(cfg, bs), _stack(cfg, bs, kv_cache=None)
    la = a.prefill(toks[:, :T])
    for t in range(T):
        lb = b.decode(toks[:, t], t)
    lr = ref.prefill(toks[:, :T])
    assert torch.allclose(la, lb, atol=1e-4), (la - lb).abs().max()
    for x, y in zip(_cache_state(a), _cache_state(b)):
        for p, q in zip(x, y):
            # (the two formulations round differently in f32: a code may land on the neighbouring value; their exponents may not)
            assert (p[:, :, :T].int() - q[:, :, :T].int()).abs().max() <= 1 and not p[:, :, T:].any() and not q[:, :, T:].any()
    for i in range(steps):
        la, lb, lr = a.decode(toks[:, T + i], T + i), b.decode(toks[:, T + i], T + i), ref.decode(toks[:, T + i], T + i)
        assert torch.allclose(la, lb, atol=1e-3), (i, (la - lb).abs().max())
        gap = (la - lr).abs().max() / lr.abs().max()
        assert 0 < gap < 0.1, gap  # quantised, and nowhere near broken (elements err by <= 1/16 of their block maximum)
    # chunked prefill reads earlier chunks through the cache, as the one-pass prefill reads its own rows: decoded values both ways
    lc, lw = _stack(cfg, bs).prefill(toks[:, :T], chunk=3), _stack(cfg, bs).prefill(toks[:, :T])
    assert torch.allclose(lc, lw, atol=1e-4), (lc - lw).abs().max()


def test_mx8_ragged_stack_equals_each_sequence_alone_and_equal_positions_reproduce_the_non_ragged_stack():
    cfg = DecodeConfig(**CFG8)
    lengths, steps = [1, 4, 7], 2
    toks = _tokens(cfg, 3, max(lengths) + steps + 1, seed=11)
    T = max(lengths)
    r = _stack(cfg, 3, ragged=True)
    got = r.prefill(toks[:, :T], lengths=lengths)
    outs = [r.decode(torch.stack([toks[b, n + i] for b, n in enumerate(lengths)]), [n + i for n in lengths]).clone() for i in range(steps)]
    for b, n in enumerate(lengths):
        s = _stack(cfg, 1)
        want = s.prefill(toks[b: b + 1, :n])
        assert torch.allclose(got[b], want[0], atol=1e-4), b
        for i in range(steps):
            want = s.decode(toks[b: b + 1, n + i], n + i)
            assert torch.allclose(outs[i][b], want[0], atol=1e-3), (b, i, (outs[i][b] - want[0]).abs().max())
        for lr, l1 in zip(r.layers, s.layers):
            for name in ("k_cache", "v_cache", "k_exp", "v_exp"):
                tr, t1 = getattr(lr, name).view(torch.uint8)[b], getattr(l1, name).view(torch.uint8)[0]
                assert (tr[:, :n + steps].int() - t1[:, :n + steps].int()).abs().max() <= 1 and not tr[:, n + steps:].any(), (b, name)
    # equal positions: the ragged addressing gives the bits of the other
    e, p = _stack(cfg, 3, ragged=True), _stack(cfg, 3)
    assert torch.equal(e.prefill(toks[:, :4], position=[0] * 3, lengths=[4] * 3), p.prefill(toks[:, :4]))
    assert torch.equal(e.decode(toks[:, 4], [4, 4, 4]), p.decode(toks[:, 4], 4))
    for x, y in zip(_cache_state(e), _cache_state(p)):
        assert all(torch.equal(u, v) for u, v in zip(x, y))


def test_mx8_prefill_into_one_slot_of_a_running_batch_and_inactive_sequences_leave_the_rest_untouched():
    cfg = DecodeConfig(**CFG8)
    toks = _tokens(cfg, 3, 10, seed=5)
    s = _stack(cfg, 3, ragged=True)
    s.prefill(toks[:, :4], lengths=[4, 2, 3])
    before = _cache_state(s)
    s.prefill(toks[1:2, 4:9], position=[0], lengths=[5], slots=[1])  # a new sequence takes slot 1
    for x, y in zip(before, _cache_state(s)):
        for name, u, v in zip(("k_cache", "v_cache", "k_exp", "v_exp"), x, y):
            assert torch.equal(u[0], v[0]) and torch.equal(u[2], v[2]), name
            assert not torch.equal(u[1], v[1]) and not v[1][:, 5:].any(), name
    before = _cache_state(s)
    s.decode(toks[:, 9], [4, -1, 3])
    for x, y in zip(before, _cache_state(s)):
        for name, u, v in zip(("k_cache", "v_cache", "k_exp", "v_exp"), x, y):
            assert torch.equal(u[1], v[1]), name
            assert torch.equal(u[0][:, :4], v[0][:, :4]) and torch.equal(u[0][:, 5:], v[0][:, 5:]), name
            assert name.endswith("exp") and v[0][:, 4].all() or v[0][:, 4].any(), name


def test_mx8_generate_with_eos():
    cfg = DecodeConfig(**CFG8)
    toks = _tokens(cfg, 2, 6, seed=9)
    prompts = [toks[0, :3], toks[1, :6]]
    free = _stack(cfg, 2, ragged=True).generate(prompts, 6)
    assert free.shape == (2, 6) and (free >= 0).all()
    eos = int(free[0, 2])
    first = (free[0] == eos).nonzero()[0].item()
    out = _stack(cfg, 2, ragged=True).generate(prompts, 6, eos=eos)
    assert torch.equal(out[0, :first + 1], free[0, :first + 1]) and (out[0, first + 1:] == eos).all()
    stop1 = (free[1] == eos).nonzero()
    n1 = stop1[0].item() + 1 if stop1.numel() else 6
    assert torch.equal(out[1, :n1], free[1, :n1])
    # a non-ragged mx8 stack generates too, and the same tokens as the ragged one on equal prompts
    same = [toks[0, :4], toks[1, :4]]
    assert torch.equal(_stack(cfg, 2).generate(torch.stack(same), 4), _stack(cfg, 2, ragged=True).generate(same, 4))


# ---------------------------------------------------------------- refusals and the C ABI
def test_host_refusals():
    from any4_amd import decode_ops as G

    with pytest.raises(ValueError, match="head_dim % 32"):
        _stack(DecodeConfig(**CFG), 1)  # head_dim 16
    with pytest.raises(ValueError, match="kv_cache must be"):
        _stack(DecodeConfig(**CFG8), 1, kv_cache="fp8")
    kc, ke = torch.zeros(1, 1, 8, 32, dtype=torch.uint8).view(F8), torch.zeros(1, 1, 8, 1, dtype=torch.uint8)
    k16 = torch.zeros(1, 1, 8, 32, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="an mx8 cache is"):
        G._mx8_exps("t", kc, kc, None, None, 32)
    with pytest.raises(RuntimeError, match="an mx8 cache is"):
        G._mx8_exps("t", kc, k16, ke, ke, 32)
    with pytest.raises(RuntimeError, match="belong to float8_e4m3fn"):
        G._mx8_exps("t", k16, k16, ke, ke, 32)
    with pytest.raises(RuntimeError, match="exponents must be uint8"):
        G._mx8_exps("t", kc, kc, ke, ke.view(1, 1, 4, 2), 32)
    with pytest.raises(RuntimeError, match="exponents must be uint8"):
        G._mx8_exps("t", kc, kc, ke.int(), ke, 32)
    assert G._mx8_exps("t", kc, kc, ke, ke, 32) == (ke, ke) and G._mx8_exps("t", k16, k16, None, None, 32) == ()
    with pytest.raises(RuntimeError, match="ROCm device"):  # no CPU fallback for the kernels
        G.rope_attn_split(torch.zeros(1, 96, dtype=torch.bfloat16), torch.zeros(8, 32), torch.zeros(8, 32), torch.zeros(1, dtype=torch.long),
                          kc, kc, 1, 1, 32, 1.0, torch.zeros(64, dtype=torch.int32), 1, k_exp=ke, v_exp=ke)


def test_mx8_flavours_refuse_null_tensors_before_any_launch():
    """The four DG_ATTN_MX8 flavours of the split and the prefill kernel: preconditions come before any launch -- null tensors are TG_E_NULL
    (-1), no device is touched; the flag is what asks for the exponents, so a call that says MX8 and brings none stays TG_E_NULL."""
    import ctypes
    import re

    from any4_amd import _lib
    from tests import attn_abi

    assert _lib.TG_ABI_VERSION == 10 and re.search(r"#define\s+TG_ABI_VERSION\s+10\b", open(os.path.join(ROOT, "include", "tinygemm_hip.h")).read())
    lib = _lib.load()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    ok = dict(qkv=p, cos=p, sin=p, pos=p, k_cache=p, v_cache=p, k_exp=p, v_exp=p, out=p, scratch=p, scratch_bytes=1 << 20, bs=2, T=4, hl=4,
              kvl=2, d=64, max_seq=128, scale=0.125, nsplit=4, dtype=2)
    for name in ENTRIES:
        assert attn_abi.launch(lib, name) == -1, name
        assert attn_abi.launch(lib, name, **ok) == -5, name                    # (every pointer there: on to the dtype, which is none)
        for exp in ("k_exp", "v_exp"):
            assert attn_abi.launch(lib, name, **dict(ok, **{exp: None})) == -1, (name, exp)
