"""CPU suite: the one-barrier kernel on an mx8 cache, the dg_rope_attn_online_mx8 / _mx8_seq flavours of dg_attn_launch, up to where a GPU
is needed -- which (kernel, flags) pairs they are, the ABI version, every argument check before the first HIP call (null stream, no GPU) -- and DecodeStack(..., kv_cache="mx8", mx8_attention=...):
the constructor's refusals, and the plain-torch formulation, which is the same for "split" and "online"."""
import ctypes

import pytest
import torch

from any4_amd.decode import DecodeConfig, DecodeLayer, DecodeStack
from tests.test_decode_cpu import CFG, SeededDense

NAMES = ("dg_rope_attn_online_mx8", "dg_rope_attn_online_mx8_seq")
TG_E_NULL, TG_E_DTYPE, TG_E_SHAPE, TG_E_ALIGN = -1, -5, -7, -8
CFG8 = dict(CFG, head_dim=32, max_seq=256)  # (the suite's tiny configuration has head_dim 16: below one mx8 block)


def test_the_flavours_are_the_split_kind_held_to_the_one_barrier_kernel():
    """DG_ATTN_SPLIT | DG_ATTN_MX8 | DG_ATTN_ONE_BARRIER, with or without DG_ATTN_SEQ; the plain one-barrier kind (DG_ATTN_ONLINE: no
    scratch, no split) has no mx8 flavour, and the library is what refuses it."""
    from any4_amd import _lib, decode_ops
    from tests import attn_abi

    L = _lib.load()
    assert L.tg_abi_version() == _lib.TG_ABI_VERSION == 10
    held = _lib.DG_ATTN_MX8 | _lib.DG_ATTN_ONE_BARRIER
    assert [attn_abi.PAIR[name] for name in NAMES] == [(_lib.DG_ATTN_SPLIT, held), (_lib.DG_ATTN_SPLIT, held | _lib.DG_ATTN_SEQ)]
    assert callable(decode_ops.rope_attn_online_mx8)
    for flags in (_lib.DG_ATTN_MX8, _lib.DG_ATTN_MX8 | _lib.DG_ATTN_SEQ, held, held | _lib.DG_ATTN_SEQ):
        assert attn_abi.launch(L, (_lib.DG_ATTN_ONLINE, flags)) == _lib.TG_E_LAYOUT, flags


def test_argument_checks_return_their_codes_before_any_launch():
    from any4_amd import _lib, decode_ops
    from tests import attn_abi

    L = _lib.load()
    buf = (ctypes.c_int32 * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)      # 16-byte aligned
    odd = ctypes.c_void_p(p.value + 4)
    ok = dict(qkv=p, cos=p, sin=p, pos=p, k_cache=p, v_cache=p, k_exp=p, v_exp=p, out=p, scratch=p, scratch_bytes=1 << 20, bs=2, hl=4, kvl=2,
              d=64, max_seq=256, scale=0.125, nsplit=4, dtype=0, device=0, stream=None)

    def call(name, **kw):
        a = dict(ok, **kw)
        return attn_abi.launch(L, name, a.pop("device"), a.pop("stream"), **a)

    need = L.dg_rope_attn_split_scratch_bytes(2, 4, 64, 4)
    for name in NAMES:
        for arg in ("qkv", "cos", "sin", "pos", "k_cache", "v_cache", "k_exp", "v_exp", "out", "scratch"):
            assert call(name, **{arg: None}) == TG_E_NULL, (name, arg)
        assert call(name, dtype=2) == TG_E_DTYPE, name
        for kw in (dict(d=96), dict(d=32), dict(d=256), dict(d=16), dict(nsplit=0), dict(nsplit=65), dict(nsplit=-1), dict(max_seq=65537),
                   dict(max_seq=131072), dict(scratch_bytes=need - 1), dict(scratch_bytes=0), dict(bs=0), dict(hl=3)):
            assert call(name, **kw) == TG_E_SHAPE, (name, kw)
        for arg in ("k_cache", "v_cache", "k_exp", "v_exp", "scratch", "qkv", "cos", "sin"):
            assert call(name, **{arg: odd}) == TG_E_ALIGN, (name, arg)
        # the order of precedence: null, (dtype,) shape -- the scratch size last of it --, alignment
        assert call(name, k_exp=None, d=96, qkv=odd) == TG_E_NULL and call(name, d=96, k_exp=odd) == TG_E_SHAPE, name
        assert call(name, scratch_bytes=16, v_exp=odd) == TG_E_SHAPE and call(name, nsplit=65, scratch_bytes=1 << 30, cos=odd) == TG_E_SHAPE, name
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        z = torch.zeros(2, 8 * 64, dtype=torch.bfloat16)
        c = torch.zeros(2, 2, 256, 64, dtype=torch.uint8).view(torch.float8_e4m3fn)
        e = torch.zeros(2, 2, 256, 2, dtype=torch.uint8)
        decode_ops.rope_attn_online_mx8(z, torch.zeros(256, 64), torch.zeros(256, 64), torch.zeros(1, dtype=torch.long), c, c.clone(), e, e.clone(),
                                        4, 2, 64, 0.125, torch.zeros(1024, dtype=torch.int32), 1)
    with pytest.raises(RuntimeError, match="mx8"):   # 16-bit caches do not belong here (checked on the host, before the device check)
        c16 = torch.zeros(2, 2, 256, 64, dtype=torch.bfloat16)
        decode_ops.rope_attn_online_mx8(z, torch.zeros(256, 64), torch.zeros(256, 64), torch.zeros(1, dtype=torch.long), c16, c16.clone(), None, None,
                                        4, 2, 64, 0.125, torch.zeros(1024, dtype=torch.int32), 1)


def _stack(cfg, **kw):
    return DecodeStack(cfg, SeededDense(cfg, 0, 1), "cpu", torch.float32, bs=3, seed=7, **kw)


def test_constructor_refusals():
    cfg = DecodeConfig(**CFG8)
    for bad in ("Online", "one-barrier", None, ""):
        with pytest.raises(ValueError, match="mx8_attention"):
            _stack(cfg, kv_cache="mx8", mx8_attention=bad)
    with pytest.raises(ValueError, match="kv_cache='mx8'"):
        _stack(cfg, mx8_attention="online")                                 # a 16-bit cache
    with pytest.raises(ValueError, match="kv_cache='mx8'"):
        DecodeLayer(cfg, 0, SeededDense(cfg, 0, 1), 0, 1, "cpu", torch.float32, 3, mx8_attention="online")
    with pytest.raises(ValueError, match="mx8_attention"):
        DecodeLayer(cfg, 0, SeededDense(cfg, 0, 1), 0, 1, "cpu", torch.float32, 3, kv_cache="mx8", mx8_attention="both")
    with pytest.raises(ValueError, match="64 or 128"):
        _stack(cfg, kv_cache="mx8", mx8_attention="online", fused=True)     # head_dim 32: the one-barrier kernel has 64 / 128
    with pytest.raises(ValueError, match="not built yet"):
        _stack(cfg, ragged=True, kv_pages=4, kv_cache="mx8", mx8_attention="online")   # paging an mx8 cache stays refused
    for kw in (dict(), dict(kv_cache="mx8"), dict(kv_cache="mx8", mx8_attention="split"), dict(mx8_attention="split")):
        s = _stack(cfg, **kw)
        assert s.mx8_attention == "split" and all(layer.mx8_attention == "split" for layer in s.layers)
    s = _stack(cfg, kv_cache="mx8", mx8_attention="online")                  # unfused: any head_dim an mx8 cache takes
    assert s.mx8_attention == "online" and all(layer.mx8_attention == "online" for layer in s.layers)


def test_plain_torch_stack_is_the_same_for_both_values():
    """Unfused float32 stack: prefill of lengths 130 / 1 / 65 and four ragged decode steps, "online" against "split": the same logits and
    the same cache bytes (the keyword picks a kernel of the fused path, nothing else)."""
    cfg = DecodeConfig(**CFG8)
    lengths = [130, 1, 65]
    a, b = (_stack(cfg, ragged=True, kv_cache="mx8", mx8_attention=m) for m in ("online", "split"))
    toks = torch.randint(0, cfg.vocab, (3, 130 + 4), generator=torch.Generator().manual_seed(0))
    assert torch.equal(a.prefill(toks[:, :130], position=0, lengths=lengths), b.prefill(toks[:, :130], position=0, lengths=lengths))
    for i in range(4):
        position = [n + i for n in lengths]
        tok = torch.stack([toks[s, min(lengths[s] + i, 133)] for s in range(3)])
        assert torch.equal(a.decode(tok, position), b.decode(tok, position)), i
    for la, lb in zip(a.layers, b.layers):
        for name in ("k_cache", "v_cache", "k_exp", "v_exp"):
            assert torch.equal(getattr(la, name).view(torch.uint8), getattr(lb, name).view(torch.uint8)), name
        assert la.k_exp[0, :, 133].any() and not la.k_exp[0, :, 134:].any()
