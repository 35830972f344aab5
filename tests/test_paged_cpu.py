"""CPU suite: the paged KV cache of the decode harness (DecodeStack(..., ragged=True, kv_pages=N), any4_amd/decode.py) in its plain-torch
formulation -- a pool of 12 pages with a scrambled free list against the contiguous ragged stack (which would hold 32 pages' worth),
release and reuse, prefix sharing with fork(), the host refusals, tensor-parallel sharding over gloo -- with the page pool's bookkeeping
(any4_amd/kvcache.py) and the C ABI of the three paged entry points (declared, exported, bound, preconditions before any launch).
Float32 stack on the tests-only dense linears of tests/test_decode_cpu.py; no HIP compute."""
import ctypes
import os
import re

import pytest
import torch

from any4_amd.decode import DecodeConfig, DecodeStack
from any4_amd.kvcache import PagePool
from tests.test_decode_cpu import CFG, SeededDense

ATOL = 1e-4  # tests/test_decode_cpu.py's tolerance for logits of the float32 stack (rows that were computed in batches of other shapes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCFG = dict(CFG, max_seq=512)
BS, PAGES, PS = 4, 12, 64
LENGTHS = [130, 1, 65, 200]
SCRAMBLED = [5, 0, 11, 3, 7, 1, 9, 2, 10, 4, 8, 6]


def _stack(cfg, kv_pages=None, rank=0, world=1, **kw):
    s = DecodeStack(cfg, SeededDense(cfg, rank, world), "cpu", torch.float32, bs=BS, rank=rank, world=world, seed=7, ragged=True,
                    kv_pages=kv_pages, **kw)
    if kv_pages == PAGES:
        s.page_pool._free = list(SCRAMBLED)  # physical order has nothing to do with logical order
    return s


def _tokens(cfg, n, T, seed=0):
    return torch.randint(0, cfg.vocab, (n, T), generator=torch.Generator().manual_seed(seed))


def test_page_pool_counts_and_exhaustion():
    pool = PagePool(4)
    assert pool.free_pages == 4 and pool.refs == [0, 0, 0, 0]
    a = pool.alloc(3)
    assert sorted(a) == [0, 1, 2] and pool.free_pages == 1 and [pool.refs[i] for i in a] == [1, 1, 1]
    pool.retain(a[:2])
    assert [pool.refs[i] for i in a] == [2, 2, 1]
    before = (list(pool.refs), list(pool._free))
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        pool.alloc(2)
    assert (pool.refs, pool._free) == before                       # nothing changed
    pool.release(a)
    assert [pool.refs[i] for i in a] == [1, 1, 0] and pool.free_pages == 2
    pool.release(a[:2])
    assert pool.refs == [0, 0, 0, 0] and pool.free_pages == 4 and sorted(pool._free) == [0, 1, 2, 3]
    for bad in (lambda: pool.release([0]), lambda: pool.retain([1]), lambda: pool.retain([7]), lambda: PagePool(0)):
        with pytest.raises(ValueError):
            bad()
    assert pool.alloc(0) == [] and pool.free_pages == 4


@pytest.fixture(scope="module")
def scenario():
    """The paged stack and the contiguous one after the same prefill (lengths 130 / 1 / 65 / 200) and 64 decode steps: slot 1 crosses
    position 64 and slot 2 position 128 (each maps a page on the way), slot 3 runs ten steps, slot 0 none -- 12 pages in the end."""
    cfg = DecodeConfig(**PCFG)
    paged, flat = _stack(cfg, PAGES), _stack(cfg)
    toks = _tokens(cfg, BS, 200)
    logits = [(paged.prefill(toks, position=0, lengths=LENGTHS).clone(), flat.prefill(toks, position=0, lengths=LENGTHS).clone())]
    mapped_after_prefill = [paged._mapped(b) for b in range(BS)]
    steps = _tokens(cfg, 64, BS, seed=1)
    for i in range(64):
        position = [-1, 1 + i, 65 + i, 200 + i if i < 10 else -1]
        logits.append((paged.decode(steps[i], position).clone(), flat.decode(steps[i], position).clone(), position))
    return cfg, paged, flat, logits, mapped_after_prefill


def test_paged_stack_equals_the_contiguous_stack_bit_for_bit(scenario):
    cfg, paged, flat, logits, mapped = scenario
    assert mapped == [3, 1, 2, 4]
    assert paged.kv_cache_bytes() * 32 == flat.kv_cache_bytes() * PAGES
    assert torch.equal(logits[0][0], logits[0][1])
    for got, want, position in logits[1:]:
        active = [b for b, p in enumerate(position) if p >= 0]
        assert torch.equal(got[active], want[active]), position
    assert [paged._mapped(b) for b in range(BS)] == [3, 2, 3, 4] and paged.page_pool.free_pages == 0
    table = paged.block_table.tolist()
    assert table == paged._table and sorted(p for row in table for p in row if p >= 0) == list(range(PAGES))
    assert table[0][:3] != sorted(table[0][:3]) or table[3][:4] != sorted(table[3][:4])  # scrambled: not the identity layout
    # every row of every slot is where the table says
    for lp, lf in zip(paged.layers, flat.layers):
        for b, n in enumerate([130, 65, 129, 210]):
            for pool, cache in ((lp.k_pool, lf.k_cache), (lp.v_pool, lf.v_cache)):
                rows = torch.stack([pool[table[b][p // PS], :, p % PS] for p in range(n)], dim=1)
                assert torch.equal(rows, cache[b, :, :n]), b


def test_exhaustion_raises_before_anything_is_mapped_or_launched(scenario):
    cfg, paged, flat, _, _ = scenario
    assert paged.page_pool.free_pages == 0
    table, refs, caches = [list(r) for r in paged._table], list(paged.page_pool.refs), [layer.k_pool.clone() for layer in paged.layers]
    pos_before = paged.pos_seq.clone()
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        paged.reserve(0, 200)
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        paged.decode(_tokens(cfg, 1, BS)[0], [130, 65, 129, 256])          # slot 3 would need a fifth page
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        paged.prefill(_tokens(cfg, 1, 70), position=[130], slots=[0])      # 200 positions: a fourth page for slot 0
    assert paged._table == table and paged.block_table.tolist() == table and paged.page_pool.refs == refs
    assert torch.equal(paged.pos_seq, pos_before)
    assert all(torch.equal(layer.k_pool, c) for layer, c in zip(paged.layers, caches))
    paged.reserve(0, 130)                                                  # what is mapped already: idempotent
    assert paged._table == table


def test_release_then_prefill_into_the_recycled_pages(scenario):
    cfg, paged, _, _, _ = scenario
    held = set(paged._table[3][:4])
    paged.release(3)
    assert paged._table[3] == [-1] * 8 and paged.block_table[3].tolist() == [-1] * 8 and paged.page_pool.free_pages == 4
    prompt = _tokens(cfg, 1, 150, seed=5)
    got = paged.prefill(prompt, position=[0], slots=[3])
    assert set(paged._table[3][:3]) <= held and paged._mapped(3) == 3       # the recycled pages, stale rows and all
    fresh = _stack(cfg)
    assert torch.equal(got, fresh.prefill(prompt, position=[0], slots=[3]))
    tok = _tokens(cfg, 1, BS, seed=6)[0]
    position = [-1, -1, -1, 150]
    assert torch.equal(paged.decode(tok, position)[3], fresh.decode(tok, position)[3])


@pytest.mark.parametrize("t", [128, 70])
def test_fork_shares_a_prefix(t):
    """fork(src, dst, t): whole pages shared (t = 128: two of them, nothing copied; t = 70: one, and six rows copied into a fresh page).
    dst then decodes like a slot that prefilled the first t tokens itself, and src goes on undisturbed."""
    cfg = DecodeConfig(**PCFG)
    paged, flat = _stack(cfg, PAGES), _stack(cfg)
    prompt = _tokens(cfg, 1, 130, seed=3)
    for s in (paged, flat):
        s.prefill(prompt, position=[0], slots=[0])
    flat.prefill(prompt[:, :t], position=[0], slots=[2])
    paged.reserve(2, 10)                                                   # dst is released first
    paged.fork(0, 2, t)
    full = t // PS
    assert paged._table[2][:full] == paged._table[0][:full] and paged._mapped(2) == -(-t // PS) and paged._mapped(0) == 3
    assert [paged.page_pool.refs[p] for p in paged._table[0][:3]] == [2] * full + [1] * (3 - full)
    assert paged.page_pool.free_pages == PAGES - 3 - (1 if t % PS else 0) and paged.block_table.tolist() == paged._table
    steps = _tokens(cfg, 3, BS, seed=4)
    for i in range(3):
        position = [130 + i, -1, t + i, -1]
        got, want = paged.decode(steps[i], position), flat.decode(steps[i], position)
        assert torch.equal(got[0], want[0]), i                            # src: unchanged by the fork
        assert torch.allclose(got[2], want[2], atol=ATOL), (i, (got[2] - want[2]).abs().max())
    # a write into a page that two slots hold is refused, by decode and by prefill, and nothing is mapped on the way
    table = [list(r) for r in paged._table]
    with pytest.raises(ValueError, match="share"):
        paged.decode(steps[0], [10, -1, -1, -1])
    with pytest.raises(ValueError, match="share"):
        paged.prefill(prompt[:, :4], position=[60], slots=[2])
    assert paged._table == table
    paged.release(0)                                                       # dst keeps the shared pages alive
    assert [paged.page_pool.refs[p] for p in paged._table[2][:full]] == [1] * full
    got, want = paged.decode(steps[0], [-1, -1, t + 3, -1]), flat.decode(steps[0], [-1, -1, t + 3, -1])
    assert torch.allclose(got[2], want[2], atol=ATOL)
    for bad in ((2, 2, 10), (2, 1, 300), (2, 4, 10), (1, 3, 1)):           # same slot; beyond what src has mapped; no such slot; src unmapped
        with pytest.raises(ValueError):
            paged.fork(*bad)


def test_constructor_refusals_and_generate():
    cfg = DecodeConfig(**PCFG)
    make = lambda **kw: DecodeStack(cfg, SeededDense(cfg, 0, 1), "cpu", torch.float32, bs=2, seed=7, **kw)
    with pytest.raises(ValueError, match="ragged=True"):
        make(kv_pages=4)
    with pytest.raises(ValueError, match="not built yet"):
        make(ragged=True, kv_pages=4, kv_cache="mx8")
    for ps in (48, 32, 96, 1024):
        with pytest.raises(ValueError, match="page_size"):
            make(ragged=True, kv_pages=4, page_size=ps)
    with pytest.raises(ValueError, match="64 or 128"):
        make(ragged=True, kv_pages=4, fused=True)                          # head_dim 16 has no paged kernel
    with pytest.raises(ValueError):
        make(ragged=True, kv_pages=0)
    plain = make(ragged=True)
    assert not plain.paged and not hasattr(plain, "block_table")
    for call in (lambda: plain.reserve(0, 1), lambda: plain.release(0), lambda: plain.fork(0, 1, 1)):
        with pytest.raises(ValueError, match="kv_pages"):
            call()
    # generate reserves len_b + new_tokens per slot up front, and releases nothing
    paged = make(ragged=True, kv_pages=4, page_size=128)
    prompts = [_tokens(cfg, 1, 120, seed=8)[0], _tokens(cfg, 1, 3, seed=9)[0]]
    out = paged.generate(prompts, 12)
    assert torch.equal(out, plain.generate(prompts, 12))
    assert [paged._mapped(b) for b in range(2)] == [2, 1] and paged.page_pool.free_pages == 1
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        paged.generate([prompts[0], prompts[0]], 140)   # three pages each, one free
    with pytest.raises(ValueError):
        paged.reserve(2, 1)
    with pytest.raises(ValueError):
        paged.reserve(0, 513)


def _tp_worker(rank, world, port, results):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = DecodeConfig(**PCFG)
        lengths = [70, 1, 65, 3]
        toks = _tokens(cfg, BS, 72, seed=19)
        full, tp = _stack(cfg, PAGES), _stack(cfg, PAGES, rank=rank, world=world)
        err = (tp.prefill(toks[:, :70], lengths=lengths) - full.prefill(toks[:, :70], lengths=lengths)).abs().max()
        for i, position in enumerate(([70, 1, 65, 3], [71, -1, 66, 4])):
            d = (tp.decode(toks[:, 70 + i], position) - full.decode(toks[:, 70 + i], position)).abs()
            err = max(err, d[[0, 2, 3]].max() if i else d.max())
        same = tp._table == full._table and tp.page_pool.refs == full.page_pool.refs and tp.layers[0].k_pool.shape[1] * world == cfg.kv_heads
        results[rank] = float(err) if same else float("inf")
    finally:
        dist.destroy_process_group()


def test_tensor_parallel_paged_gloo():
    """Heads / rows split over two ranks, the table and the pool's decisions replicated, the pools per rank == the unsharded paged stack."""
    import torch.multiprocessing as mp

    world = 2
    port = 37500 + (os.getpid() % 2000)
    results = mp.Manager().dict()
    mp.spawn(_tp_worker, args=(world, port, results), nprocs=world, join=True)
    assert set(results.keys()) == {0, 1}
    assert max(results.values()) < ATOL, dict(results)


PAGED_FLAVOURS = ("dg_rope_attn_online_paged", "dg_rope_attn_split_paged", "dg_prefill_attn_paged")


def test_paged_abi_preconditions_fail_before_any_launch():
    """The three paged 16-bit flavours of dg_attn_launch (DG_ATTN_SEQ | DG_ATTN_PAGED on the one-barrier, the split and the prefill kernel):
    argument validation returns its TG_E_* code before the first HIP call (null stream, no GPU)."""
    from any4_amd import _lib, decode_ops
    from tests import attn_abi

    L = _lib.load()
    for name in PAGED_FLAVOURS:
        assert callable(getattr(decode_ops, name[3:])), name
    paged = _lib.DG_ATTN_SEQ | _lib.DG_ATTN_PAGED
    assert attn_abi.launch(L, (_lib.DG_ATTN_GENERAL, paged)) == _lib.TG_E_LAYOUT               # no paged flavour of the 256-thread kernels
    assert attn_abi.launch(L, (_lib.DG_ATTN_GENERAL, paged | _lib.DG_ATTN_MX8)) == _lib.TG_E_LAYOUT   # nor of their mx8 caches

    buf = (ctypes.c_int32 * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)      # 16-byte aligned
    odd = ctypes.c_void_p(p.value + 4)
    ok = dict(qkv=p, cos=p, sin=p, pos=p, len=p, slot=p, table=p, k_pool=p, v_pool=p, out=p, scratch=p, scratch_bytes=1 << 20, bs=2, T=4,
              cache_bs=3, hl=4, kvl=2, d=64, max_seq=256, page_size=64, num_pages=5, scale=0.125, nsplit=4, dtype=0, device=0, stream=None)

    def call(name, **kw):
        a = dict(ok, **kw)
        return attn_abi.launch(L, name, a.pop("device"), a.pop("stream"), **a)

    for name in PAGED_FLAVOURS:
        for arg in ("table", "qkv", "pos", "k_pool", "v_pool", "out"):
            assert call(name, **{arg: None}) == -1, (name, arg)             # TG_E_NULL
        assert call(name, dtype=2) == -5, name                              # TG_E_DTYPE
        for kw in (dict(d=96), dict(d=32), dict(d=256), dict(page_size=48), dict(page_size=32), dict(page_size=96), dict(page_size=512),
                   dict(page_size=0), dict(max_seq=320, page_size=128), dict(num_pages=0), dict(num_pages=-3), dict(bs=0)):
            assert call(name, **kw) == -7, (name, kw)                       # TG_E_SHAPE
        for arg in ("table", "qkv", "cos", "sin", "k_pool", "v_pool"):
            assert call(name, **{arg: odd}) == -8, (name, arg)              # TG_E_ALIGN
        assert call(name, table=None, d=96, qkv=odd) == -1 and call(name, d=96, table=odd) == -7, name   # null before shape before alignment
    assert call("dg_rope_attn_online_paged", max_seq=131072) == -7 and call("dg_rope_attn_split_paged", max_seq=131072) == -7
    assert call("dg_prefill_attn_paged", max_seq=16384) == -7 and call("dg_prefill_attn_paged", slot=None) == -7   # n != cache_bs without slots
    assert call("dg_rope_attn_split_paged", nsplit=65) == -7 and call("dg_rope_attn_split_paged", scratch_bytes=16) == -7
    assert call("dg_rope_attn_split_paged", scratch=None) == -1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        z = torch.zeros(2, 8 * 64, dtype=torch.bfloat16)
        pool = torch.zeros(5, 2, 64, 64, dtype=torch.bfloat16)
        decode_ops.rope_attn_online_paged(z, torch.zeros(256, 64), torch.zeros(256, 64), torch.zeros(2, dtype=torch.long),
                                          torch.zeros(2, 4, dtype=torch.int32), pool, pool.clone(), 4, 2, 64, 0.125)
