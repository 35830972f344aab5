"""CPU suite: a position per sequence in the decode harness (DecodeStack(..., ragged=True), any4_amd/decode.py) in its plain-torch
formulation -- a ragged batch against each sequence alone, equal positions against the non-ragged stack, inactive sequences, cache
slots, chunking, generate() over prompts of different lengths, host refusals, tensor-parallel sharding over gloo -- and the C ABI of
the four per-sequence entry points (declared, exported, bound, preconditions before any launch).
Float32 stack on the tests-only dense linears of tests/test_decode_cpu.py; no HIP compute."""
import ctypes
import os

import pytest
import torch

from any4_amd.decode import DecodeConfig, DecodeStack
from tests.test_decode_cpu import CFG, SeededDense

ATOL = 1e-4  # tests/test_decode_cpu.py's tolerance for logits of the float32 stack
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stack(cfg, bs, ragged=True, rank=0, world=1):
    return DecodeStack(cfg, SeededDense(cfg, rank, world), "cpu", torch.float32, bs=bs, rank=rank, world=world, seed=7, ragged=ragged)


def _tokens(cfg, bs, T, seed=0):
    return torch.randint(0, cfg.vocab, (bs, T), generator=torch.Generator().manual_seed(seed))


def _pad(toks, lengths):
    """Rows of `toks` beyond each length replaced by another token: padding must not matter."""
    out = toks.clone()
    for b, n in enumerate(lengths):
        out[b, n:] = (toks[b, n:] + 1) % 7
    return out


def _caches(stack):
    return [(layer.k_cache.clone(), layer.v_cache.clone()) for layer in stack.layers]


def _alone(cfg, toks, lengths, steps):
    """Each sequence on a bs = 1 non-ragged stack: prefill of its own tokens, then `steps` decode steps fed toks[b, len_b + i].
    Returns (stacks, prefill logits [bs, vocab], step logits [steps][bs, vocab])."""
    stacks, pl, sl = [], [], [[] for _ in range(steps)]
    for b, n in enumerate(lengths):
        s = _stack(cfg, 1, ragged=False)
        pl.append(s.prefill(toks[b: b + 1, :n]).clone())
        for i in range(steps):
            sl[i].append(s.decode(toks[b: b + 1, n + i], n + i).clone())
        stacks.append(s)
    return stacks, torch.cat(pl), [torch.cat(x) for x in sl]


def _rows_agree(ragged, singles, rows, atol=1e-5, slots=None):
    """Cache rows [0, rows[b]) of slot b agree with the single stack's; every other row of the slot is still exactly zero."""
    for lr, *ls in zip(ragged.layers, *[s.layers for s in singles]):
        for b, (l1, n) in enumerate(zip(ls, rows)):
            sl = b if slots is None else slots[b]
            for got, want in ((lr.k_cache[sl], l1.k_cache[0]), (lr.v_cache[sl], l1.v_cache[0])):
                assert torch.allclose(got[:, :n], want[:, :n], atol=atol), (b, (got[:, :n] - want[:, :n]).abs().max())
                assert not got[:, n:].any(), b


def test_ragged_equals_each_sequence_alone():
    cfg = DecodeConfig(**CFG)
    lengths, steps = [1, 4, 7], 3
    toks = _tokens(cfg, 3, max(lengths) + steps + 1, seed=11)
    singles, want_p, want_s = _alone(cfg, toks, lengths, steps)
    T = max(lengths)
    stack = _stack(cfg, 3)
    got = stack.prefill(_pad(toks[:, :T], lengths), lengths=lengths)
    assert got.shape == (3, cfg.vocab)
    assert torch.allclose(got, want_p, atol=ATOL), (got - want_p).abs().max()
    for i in range(steps):
        fed = torch.stack([toks[b, n + i] for b, n in enumerate(lengths)])
        got = stack.decode(fed, [n + i for n in lengths])
        assert torch.allclose(got, want_s[i], atol=ATOL), (i, (got - want_s[i]).abs().max())
    _rows_agree(stack, singles, [n + steps for n in lengths])


def test_equal_positions_reproduce_the_non_ragged_stack_exactly():
    cfg = DecodeConfig(**CFG)
    bs, T = 3, 5
    toks = _tokens(cfg, bs, T + 2, seed=12)
    a, b = _stack(cfg, bs), _stack(cfg, bs, ragged=False)
    assert torch.equal(a.prefill(toks[:, :T], position=[0] * bs, lengths=[T] * bs), b.prefill(toks[:, :T]))
    for i, position in enumerate(([T] * bs, torch.full((bs,), T + 1))):  # a list, a tensor
        assert torch.equal(a.decode(toks[:, T + i], position), b.decode(toks[:, T + i], T + i)), i
    assert torch.equal(a.decode(toks[:, 0], T + 2), b.decode(toks[:, 0], T + 2))  # an int: all sequences
    for la, lb in zip(a.layers, b.layers):
        assert torch.equal(la.k_cache, lb.k_cache) and torch.equal(la.v_cache, lb.v_cache)
    # the chunk loop: positions and lengths named per sequence against the plain call, three chunks of 3 / 3 / 1 tokens from position 2
    T = 7
    a, b = _stack(cfg, bs), _stack(cfg, bs, ragged=False)
    assert torch.equal(a.prefill(toks[:, :T], position=[2] * bs, lengths=[T] * bs, chunk=3), b.prefill(toks[:, :T], position=2, chunk=3))
    for la, lb in zip(a.layers, b.layers):
        assert torch.equal(la.k_cache, lb.k_cache) and torch.equal(la.v_cache, lb.v_cache)


def test_inactive_sequence_writes_nothing_and_disturbs_nobody():
    cfg = DecodeConfig(**CFG)
    lengths = [3, 5, 2]
    toks = _tokens(cfg, 3, 8, seed=13)
    a, b = _stack(cfg, 3), _stack(cfg, 3)
    for s in (a, b):
        s.prefill(_pad(toks[:, :5], lengths), lengths=lengths)
    before = _caches(a)
    for i in range(2):
        fed = toks[:, 5 + i]
        got = a.decode(fed, [lengths[0] + i, -1, lengths[2] + i]).clone()
        want = b.decode(fed, [n + i for n in lengths])
        assert torch.allclose(got[[0, 2]], want[[0, 2]], atol=ATOL), (i, (got[[0, 2]] - want[[0, 2]]).abs().max())
    for (k0, v0), la, lb in zip(before, a.layers, b.layers):
        assert torch.equal(la.k_cache[1], k0[1]) and torch.equal(la.v_cache[1], v0[1])
        for sl in (0, 2):
            assert torch.allclose(la.k_cache[sl], lb.k_cache[sl], atol=1e-5) and torch.allclose(la.v_cache[sl], lb.v_cache[sl], atol=1e-5)
            assert la.k_cache[sl, :, lengths[sl] + 1].any()  # (the active ones did write)


def test_prefill_into_one_slot_of_a_running_batch():
    cfg = DecodeConfig(**CFG)
    lengths = [3, 4, 2]
    toks = _tokens(cfg, 3, 6, seed=14)
    new = _tokens(cfg, 1, 5, seed=15)
    stack = _stack(cfg, 3)
    stack.prefill(_pad(toks[:, :4], lengths), lengths=lengths)
    before = _caches(stack)
    got = stack.prefill(new, position=0, slots=[2])
    # the references: sequences 0 and 1 as they were, the newcomer alone
    singles, _, want_s = _alone(cfg, torch.cat([toks[:2], torch.cat([new, toks[2:3, :1]], dim=1)]), [3, 4, 5], 1)
    fresh = _stack(cfg, 1, ragged=False)
    want = fresh.prefill(new)
    assert got.shape == (1, cfg.vocab) and torch.allclose(got, want, atol=ATOL), (got - want).abs().max()
    for (k0, v0), layer in zip(before, stack.layers):
        for sl in (0, 1):
            assert torch.equal(layer.k_cache[sl], k0[sl]) and torch.equal(layer.v_cache[sl], v0[sl])
        assert not torch.equal(layer.k_cache[2], k0[2])
    fed = torch.stack([toks[0, 3], toks[1, 4], toks[2, 0]])
    got = stack.decode(fed, [3, 4, 5])
    assert torch.allclose(got, want_s[0], atol=ATOL), (got - want_s[0]).abs().max()
    _rows_agree(stack, singles, [4, 5, 6])


def test_chunked_ragged_prefill_equals_the_single_pass():
    cfg = DecodeConfig(**CFG)
    lengths = [2, 7, 11]  # with chunk = 3 the last valid tokens lie in chunks 0, 2 and 3
    toks = _pad(_tokens(cfg, 3, 11, seed=16), lengths)
    whole, chunked = _stack(cfg, 3), _stack(cfg, 3)
    lw = whole.prefill(toks, lengths=lengths)
    lc = chunked.prefill(toks, lengths=lengths, chunk=3)
    assert torch.allclose(lc, lw, atol=ATOL), (lc - lw).abs().max()
    _, want, _ = _alone(cfg, toks, lengths, 0)
    assert torch.allclose(lc, want, atol=ATOL), (lc - want).abs().max()
    for la, lb in zip(whole.layers, chunked.layers):
        assert torch.allclose(la.k_cache, lb.k_cache, atol=1e-5) and torch.allclose(la.v_cache, lb.v_cache, atol=1e-5)
        for b, n in enumerate(lengths):
            assert not lb.k_cache[b, :, n:].any() and not lb.v_cache[b, :, n:].any()


def test_generate_over_prompts_of_different_lengths_and_eos():
    cfg = DecodeConfig(**CFG)
    lengths, new = [2, 5, 3], 6
    toks = _tokens(cfg, 3, 5, seed=17)
    prompts = [toks[b, :n] for b, n in enumerate(lengths)]
    want = torch.cat([_stack(cfg, 1, ragged=False).generate(p.view(1, -1), new) for p in prompts])
    got = _stack(cfg, 3).generate(prompts, new)
    assert got.shape == (3, new) and torch.equal(got, want)
    # sequence 0 stops at the token it emits at step 2
    eos = int(want[0, 2])
    first = [int((want[b] == eos).nonzero()[0]) if (want[b] == eos).any() else new for b in range(3)]
    assert first[0] <= 2
    stack = _stack(cfg, 3)
    got = stack.generate(prompts, new, eos=eos)
    for b in range(3):
        assert torch.equal(got[b, : first[b] + 1], want[b, : first[b] + 1]), b
        assert (got[b, first[b]:] == eos).all(), b
        # the token emitted at step i is fed at position len + i; the eos token is never fed
        written = lengths[b] + min(first[b], new - 1)
        for layer in stack.layers:
            assert layer.k_cache[b, :, written - 1].any() and not layer.k_cache[b, :, written:].any(), b
            assert not layer.v_cache[b, :, written:].any(), b
    # eos = None: a sequence goes inactive where the cache ends, its remaining outputs are -1
    stack = _stack(cfg, 2)
    long = [_tokens(cfg, 1, cfg.max_seq - 2, seed=18)[0], toks[0, :3]]
    got = stack.generate(long, 5)
    assert (got[0, :3] >= 0).all() and (got[0, 3:] == -1).all() and (got[1] >= 0).all()


def test_host_refusals():
    cfg = DecodeConfig(**CFG)
    stack, plain = _stack(cfg, 3), _stack(cfg, 3, ragged=False)
    toks = _tokens(cfg, 3, 5)
    for kw in (dict(lengths=[1, 6, 2]), dict(lengths=[1, -1, 2]), dict(lengths=[1, 2]),          # a length outside [0, T]; too few
               dict(position=[0, cfg.max_seq - 4, 0]), dict(position=[0, -1, 0]),              # position + length > max_seq; negative
               dict(slots=[0, 1, 1]), dict(slots=[0, 1, 3]), dict(slots=[0, -1, 2])):           # duplicate / out-of-range slots
        with pytest.raises(ValueError):
            stack.prefill(toks, **kw)
    assert stack.prefill(toks, position=[0, cfg.max_seq - 4, 0], lengths=[5, 4, 5]).shape == (3, cfg.vocab)  # ends at max_seq: legal
    with pytest.raises(ValueError, match="slots"):
        stack.prefill(toks[:2], lengths=[1, 2])                    # n != bs without slots
    with pytest.raises(ValueError):
        stack.prefill(toks, position=None, lengths=[1, 2, 3])
    with pytest.raises(ValueError):
        stack.prefill(toks, lengths=[1, 2, 3], chunk=0)
    for kw in (dict(lengths=[1, 2, 3]), dict(slots=[0, 1, 2]), dict(position=[0, 0, 0])):
        with pytest.raises(ValueError, match="ragged=True"):
            plain.prefill(toks, **kw)
    for position in ([0, 0, 0], torch.zeros(3, dtype=torch.long), 1.5):
        with pytest.raises(ValueError):
            plain.decode(toks[:, 0], position)
    with pytest.raises(ValueError, match="ragged=True"):
        plain.generate([toks[0], toks[1, :2], toks[2]], 2)
    for position in ([0, 1], [0, 1, cfg.max_seq], [0, -2, 1], cfg.max_seq, [0.5, 1, 2]):
        with pytest.raises(ValueError):
            stack.decode(toks[:, 0], position)
    assert not hasattr(plain, "pos_seq") and stack.pos_seq.shape == (3,) and stack.pos.shape == (1,)


def _tp_worker(rank, world, port, results):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = DecodeConfig(**CFG)
        lengths = [2, 6, 4]
        toks = _pad(_tokens(cfg, 3, 8, seed=19), lengths)
        full, tp = _stack(cfg, 3), _stack(cfg, 3, rank=rank, world=world)
        err = (tp.prefill(toks[:, :6], lengths=lengths) - full.prefill(toks[:, :6], lengths=lengths)).abs().max()
        for i, position in enumerate(([2, 6, 4], [3, -1, 5])):
            d = (tp.decode(toks[:, 6 + i], position) - full.decode(toks[:, 6 + i], position)).abs()
            err = max(err, d[[0, 2]].max() if i else d.max())
        results[rank] = float(err)
    finally:
        dist.destroy_process_group()


def test_tensor_parallel_ragged_gloo():
    """Heads / rows split over two ranks: ragged prefill and two decode steps (the second with an inactive sequence) == unsharded."""
    import torch.multiprocessing as mp

    world = 2
    port = 35500 + (os.getpid() % 2000)
    results = mp.Manager().dict()
    mp.spawn(_tp_worker, args=(world, port, results), nprocs=world, join=True)
    assert set(results.keys()) == {0, 1}
    assert max(results.values()) < ATOL, dict(results)


SEQ_SYMBOLS = ("dg_rope_attn_seq", "dg_rope_attn_online_seq", "dg_rope_attn_split_seq", "dg_prefill_attn_seq")


def test_per_sequence_abi_preconditions_fail_before_any_launch():
    """The four per-sequence flavours of dg_attn_launch (DG_ATTN_SEQ on each kernel): argument validation returns its TG_E_* code before
    the first HIP call (null stream, no GPU)."""
    import inspect

    from any4_amd import _lib, decode_ops
    from tests import attn_abi

    L = _lib.load()
    for fn in (decode_ops.rope_attn, decode_ops.rope_attn_online, decode_ops.rope_attn_split, decode_ops.prefill_attn):
        assert inspect.signature(fn).parameters["per_sequence"].default is False
    for name in ("lengths", "slots"):
        assert inspect.signature(decode_ops.prefill_attn).parameters[name].default is None

    buf = (ctypes.c_int32 * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)      # 16-byte aligned
    odd = ctypes.c_void_p(p.value + 2)

    ok = dict(qkv=p, cos=p, sin=p, pos=p, len=p, slot=p, k=p, v=p, out=p, n=2, T=4, cache_bs=3, hl=4, kvl=2, d=64, max_seq=128, scale=0.125,
              dtype=0)

    def prefill(**kw):
        return attn_abi.launch(L, "dg_prefill_attn_seq", **dict(ok, **kw))

    for name in ("qkv", "cos", "sin", "pos", "k", "v", "out"):
        assert prefill(**{name: None}) == -1, name                   # TG_E_NULL
    assert prefill(dtype=2) == -5                                    # TG_E_DTYPE
    for kw in (dict(d=96), dict(d=32), dict(n=0), dict(T=0), dict(cache_bs=0), dict(max_seq=8193), dict(hl=4, kvl=3),
               dict(slot=None), dict(slot=None, n=4)):               # slot == NULL with n != cache_bs
        assert prefill(**kw) == -7, kw                               # TG_E_SHAPE
    for name in ("qkv", "cos", "sin", "k", "v", "out"):
        assert prefill(**{name: odd}) == -8, name                    # TG_E_ALIGN

    def step(name, **kw):
        return attn_abi.launch(L, name, **dict(dict(ok, bs=2, scratch=p, scratch_bytes=1 << 20, nsplit=4), **kw))

    for name in SEQ_SYMBOLS[:3]:
        assert step(name, pos=None) == -1, name
        assert step(name, dtype=2) == -5, name
        assert step(name, d=96) == -7 and step(name, bs=0) == -7, name
        assert step(name, k=odd) == -8, name
    assert step("dg_rope_attn_online_seq", qkv=odd) == -8
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        z = torch.zeros(8, 8 * 64, dtype=torch.bfloat16)
        c = torch.zeros(3, 2, 128, 64, dtype=torch.bfloat16)
        decode_ops.prefill_attn(z, torch.zeros(128, 64), torch.zeros(128, 64), torch.zeros(2, dtype=torch.long), c, c.clone(), 4, 2, 64,
                                0.125, 4, lengths=torch.ones(2, dtype=torch.long), slots=torch.zeros(2, dtype=torch.long))
