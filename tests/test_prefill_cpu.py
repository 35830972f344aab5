"""CPU suite: prompt prefill of the decode harness (DecodeStack.prefill / generate, any4_amd/decode.py) in its plain-torch
formulation -- a chunk of T tokens at once against T one-token `decode()` calls, chunking, the greedy loop, host refusals,
tensor-parallel sharding over gloo -- and the C ABI of dg_prefill_attn (exported, bound, preconditions before any launch).
Float32 stack on the tests-only dense linears of tests/test_decode_cpu.py; no HIP compute."""
import ctypes
import os

import pytest
import torch

from any4_amd.decode import DecodeConfig, DecodeStack
from tests.test_decode_cpu import CFG, SeededDense

ATOL = 1e-4  # tests/test_decode_cpu.py's tolerance for logits of the float32 stack


def _stack(cfg, bs, rank=0, world=1):
    return DecodeStack(cfg, SeededDense(cfg, rank, world), "cpu", torch.float32, bs=bs, rank=rank, world=world, seed=7)


def _tokens(cfg, bs, T, seed=0):
    return torch.randint(0, cfg.vocab, (bs, T), generator=torch.Generator().manual_seed(seed))


def _caches_close(a, b, atol=1e-5):
    for la, lb in zip(a.layers, b.layers):
        assert torch.allclose(la.k_cache, lb.k_cache, atol=atol), (la.k_cache - lb.k_cache).abs().max()
        assert torch.allclose(la.v_cache, lb.v_cache, atol=atol), (la.v_cache - lb.v_cache).abs().max()


@pytest.mark.parametrize("bs", [1, 3])
@pytest.mark.parametrize("T", [1, 5, CFG["max_seq"]])
def test_prefill_equals_token_by_token_decode(bs, T):
    """prefill(toks[:, :T]) == the logits of the last of T decode() calls on a fresh stack; the caches of every layer agree."""
    cfg = DecodeConfig(**CFG)
    toks = _tokens(cfg, bs, T)
    a, b = _stack(cfg, bs), _stack(cfg, bs)
    got = a.prefill(toks)
    for i in range(T):
        want = b.decode(toks[:, i], i)
    assert got.shape == (bs, cfg.vocab)
    assert torch.allclose(got, want, atol=ATOL), (got - want).abs().max()
    _caches_close(a, b)


def test_prefill_chunking_and_decode_continues():
    """One pass of T tokens == two calls (T1 at 0, the rest at T1) == chunk=3; decode() then continues identically from each."""
    cfg = DecodeConfig(**CFG)
    bs, T, T1 = 2, 11, 4
    toks = _tokens(cfg, bs, T + 3, seed=1)
    whole, two, chunked = _stack(cfg, bs), _stack(cfg, bs), _stack(cfg, bs)
    lw = whole.prefill(toks[:, :T])
    assert two.prefill(toks[:, :T1], 0).shape == (bs, cfg.vocab)
    lt = two.prefill(toks[:, T1:T], T1)
    lc = chunked.prefill(toks[:, :T], chunk=3)
    assert torch.allclose(lt, lw, atol=ATOL) and torch.allclose(lc, lw, atol=ATOL), ((lt - lw).abs().max(), (lc - lw).abs().max())
    _caches_close(whole, two)
    _caches_close(whole, chunked)
    for i in range(3):
        dw = whole.decode(toks[:, T + i], T + i).clone()
        for other in (two, chunked):
            do = other.decode(toks[:, T + i], T + i)
            assert torch.allclose(do, dw, atol=ATOL), (i, (do - dw).abs().max())


def test_generate_equals_manual_greedy_loop():
    cfg = DecodeConfig(**CFG)
    bs, T, new = 2, 6, 5
    prompt = _tokens(cfg, bs, T, seed=2)
    got = _stack(cfg, bs).generate(prompt, new)
    ref = _stack(cfg, bs)
    for i in range(T):
        logits = ref.decode(prompt[:, i], i)
    want = []
    for i in range(new):
        tok = logits.argmax(-1)
        want.append(tok.clone())
        if i + 1 < new:
            logits = ref.decode(tok, T + i)
    assert got.shape == (bs, new) and torch.equal(got, torch.stack(want, dim=1))


def test_prefill_host_refusals():
    cfg = DecodeConfig(**CFG)
    stack = _stack(cfg, 2)
    toks = _tokens(cfg, 2, 5)
    with pytest.raises(ValueError, match="outside the KV cache"):
        stack.prefill(toks, cfg.max_seq - 4)          # position + T > max_seq
    with pytest.raises(ValueError, match="outside the KV cache"):
        stack.prefill(toks, -1)
    with pytest.raises(ValueError, match="outside the KV cache"):
        stack.prefill(_tokens(cfg, 2, cfg.max_seq + 1))
    for bad in (toks[0], toks[:1], toks[:, :0], toks.unsqueeze(0)):  # [T], wrong bs, T = 0, three dimensions
        with pytest.raises(ValueError, match="tokens must be"):
            stack.prefill(bad)
    with pytest.raises(ValueError, match="chunk"):
        stack.prefill(toks, chunk=0)
    assert stack.prefill(toks, cfg.max_seq - 5).shape == (2, cfg.vocab)  # position + T == max_seq is the last legal place


def _tp_worker(rank, world, port, results):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = DecodeConfig(**CFG)
        toks = _tokens(cfg, 3, 7, seed=3)
        full, tp = _stack(cfg, 3), _stack(cfg, 3, rank, world)
        err = (tp.prefill(toks[:, :5]) - full.prefill(toks[:, :5])).abs().max()
        err = max(err, (tp.prefill(toks[:, 5:], 5) - full.prefill(toks[:, 5:], 5)).abs().max())  # a second chunk over the first one's rows
        err = max(err, (tp.decode(toks[:, 0], 7) - full.decode(toks[:, 0], 7)).abs().max())
        results[rank] = float(err)
    finally:
        dist.destroy_process_group()


def test_tensor_parallel_prefill_gloo():
    """Heads / rows split over two ranks, the four exchanges of a layer as all_gathers at bs * T rows == the unsharded stack."""
    import torch.multiprocessing as mp

    world = 2
    port = 33500 + (os.getpid() % 2000)
    results = mp.Manager().dict()
    mp.spawn(_tp_worker, args=(world, port, results), nprocs=world, join=True)
    assert set(results.keys()) == {0, 1}
    assert max(results.values()) < ATOL, dict(results)


def test_dg_prefill_attn_abi_preconditions_fail_before_any_launch():
    """DG_ATTN_PREFILL with no flags: argument validation returns its TG_E_* code before the first HIP call (null stream, no GPU)."""
    from any4_amd import _lib, decode_ops
    from tests import attn_abi

    assert callable(decode_ops.prefill_attn)
    L = _lib.load()
    buf = (ctypes.c_int32 * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)      # 16-byte aligned
    odd = ctypes.c_void_p(p.value + 2)
    ok = dict(qkv=p, cos=p, sin=p, pos=p, k=p, v=p, out=p, bs=1, T=4, hl=4, kvl=2, d=64, max_seq=128, scale=0.125, dtype=0)

    def call(**kw):
        return attn_abi.launch(L, "dg_prefill_attn", **dict(ok, **kw))

    for name in ("qkv", "cos", "sin", "pos", "k", "v", "out"):
        assert call(**{name: None}) == -1, name                      # TG_E_NULL
    assert call(dtype=2) == -5                                       # TG_E_DTYPE
    for kw in (dict(bs=0), dict(T=0), dict(T=-3), dict(hl=0), dict(kvl=0), dict(hl=4, kvl=3), dict(d=32), dict(d=96), dict(d=256),
               dict(max_seq=0), dict(max_seq=8193), dict(bs=1 << 20, T=1 << 20)):
        assert call(**kw) == -7, kw                                  # TG_E_SHAPE
    for name in ("qkv", "cos", "sin", "k", "v", "out"):
        assert call(**{name: odd}) == -8, name                       # TG_E_ALIGN
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        z = torch.zeros(4, 8 * 64, dtype=torch.bfloat16)
        c = torch.zeros(2, 4, 128, 64, dtype=torch.bfloat16)
        decode_ops.prefill_attn(z, torch.zeros(128, 64), torch.zeros(128, 64), torch.zeros(1, dtype=torch.long), c, c.clone(), 4, 2, 64,
                                0.125, 4)
