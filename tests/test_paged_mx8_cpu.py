"""CPU suite: the paged mx8 KV cache, DecodeStack(..., ragged=True, kv_cache="mx8", kv_pages=N) -- four pools (E4M3 codes and exponent
bytes) behind the one block table -- up to where a GPU is needed.  The two flavours dg_rope_attn_online_mx8_paged and
dg_prefill_attn_mx8_paged of dg_attn_launch: which (kernel, flags) pairs they are, every argument check before the first HIP call (null stream, no GPU; the cases of
tests/test_paged_cpu.py and tests/test_kv8_online_cpu.py, merged).  The unfused float32 stack at head_dim 64 in the scenario of
tests/test_paged_cpu.py against the contiguous ragged mx8 stack, bit for bit; release and reuse, fork, exhaustion, the shared-page
refusal, tensor parallelism over gloo; and the refusal that stays (head_dim 16 / 32)."""
import ctypes
import os

import pytest
import torch

from any4_amd.decode import DecodeConfig, DecodeLayer, DecodeStack
from tests.test_decode_cpu import CFG, SeededDense

NAMES = ("dg_rope_attn_online_mx8_paged", "dg_prefill_attn_mx8_paged")
TG_E_NULL, TG_E_DTYPE, TG_E_SHAPE, TG_E_ALIGN = -1, -5, -7, -8
ATOL = 1e-4  # tests/test_decode_cpu.py's tolerance for logits of the float32 stack (rows that were computed in batches of other shapes)
PCFG = dict(CFG, head_dim=64, max_seq=512)  # (paged mx8 pools exist for head_dim 64 / 128; the rest is the suite's tiny configuration)
BS, PAGES, PS = 4, 12, 64
LENGTHS = [130, 1, 65, 200]
SCRAMBLED = [5, 0, 11, 3, 7, 1, 9, 2, 10, 4, 8, 6]
POOLS = ("k_pool", "v_pool", "k_exp_pool", "v_exp_pool")
FLAT = ("k_cache", "v_cache", "k_exp", "v_exp")


def test_the_flavours_and_the_pairs_next_to_them_that_the_library_refuses():
    """DG_ATTN_SEQ | DG_ATTN_PAGED | DG_ATTN_MX8 on the prefill kernel and, held to the one-barrier kernel, on the split kind; what lies
    next to them does not exist, and the library is what refuses it."""
    from any4_amd import _lib, decode_ops
    from tests import attn_abi

    L = _lib.load()
    assert L.tg_abi_version() == _lib.TG_ABI_VERSION == 10
    pools8 = _lib.DG_ATTN_SEQ | _lib.DG_ATTN_PAGED | _lib.DG_ATTN_MX8
    assert [attn_abi.PAIR[name] for name in NAMES] == [(_lib.DG_ATTN_SPLIT, pools8 | _lib.DG_ATTN_ONE_BARRIER), (_lib.DG_ATTN_PREFILL, pools8)]
    for name in NAMES:
        assert callable(getattr(decode_ops, name[3:])), name
    for pair in ((_lib.DG_ATTN_SPLIT, pools8),                              # no paged-mx8 flavour of the 256-thread split kernel
                 (_lib.DG_ATTN_ONLINE, pools8), (_lib.DG_ATTN_ONLINE, _lib.DG_ATTN_MX8),   # no mx8 flavour of the plain one-barrier kind
                 (_lib.DG_ATTN_GENERAL, pools8), (_lib.DG_ATTN_GENERAL, pools8 | _lib.DG_ATTN_ONE_BARRIER),
                 (_lib.DG_ATTN_PREFILL, pools8 | _lib.DG_ATTN_ONE_BARRIER), (_lib.DG_ATTN_PREFILL, pools8 & ~_lib.DG_ATTN_SEQ)):
        assert attn_abi.launch(L, pair) == _lib.TG_E_LAYOUT, pair


def test_argument_checks_return_their_codes_before_any_launch():
    from any4_amd import _lib, decode_ops
    from tests import attn_abi

    L = _lib.load()
    buf = (ctypes.c_int32 * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)      # 16-byte aligned
    odd = ctypes.c_void_p(p.value + 4)
    ok = dict(qkv=p, cos=p, sin=p, pos=p, len=p, slot=p, table=p, k_pool=p, v_pool=p, k_exp=p, v_exp=p, out=p, scratch=p, scratch_bytes=1 << 20,
              bs=2, T=4, cache_bs=3, hl=4, kvl=2, d=64, max_seq=256, page_size=64, num_pages=5, scale=0.125, nsplit=4, dtype=0, device=0,
              stream=None)

    def call(name, **kw):
        a = dict(ok, **kw)
        return attn_abi.launch(L, name, a.pop("device"), a.pop("stream"), **a)

    decode, prefill = NAMES
    need = L.dg_rope_attn_split_scratch_bytes(2, 4, 64, 4)
    for name in NAMES:
        for arg in ("table", "qkv", "cos", "sin", "pos", "k_pool", "v_pool", "k_exp", "v_exp", "out"):
            assert call(name, **{arg: None}) == TG_E_NULL, (name, arg)
        assert call(name, dtype=2) == TG_E_DTYPE, name
        for kw in (dict(d=96), dict(d=32), dict(d=256), dict(d=16), dict(page_size=48), dict(page_size=32), dict(page_size=96), dict(page_size=0),
                   dict(page_size=512), dict(max_seq=320, page_size=128), dict(num_pages=0), dict(num_pages=-3), dict(bs=0), dict(hl=3)):
            assert call(name, **kw) == TG_E_SHAPE, (name, kw)      # (page_size 512: above max_seq 256)
        for arg in ("table", "qkv", "cos", "sin", "k_pool", "v_pool", "k_exp", "v_exp"):
            assert call(name, **{arg: odd}) == TG_E_ALIGN, (name, arg)
        # the order of precedence: null, (dtype,) shape, alignment
        assert call(name, table=None, d=96, qkv=odd) == TG_E_NULL and call(name, d=96, table=odd) == TG_E_SHAPE, name
        assert call(name, k_exp=None, d=96, qkv=odd) == TG_E_NULL and call(name, page_size=48, k_exp=odd) == TG_E_SHAPE, name
        assert call(name, v_exp=None, dtype=2) == TG_E_NULL and call(name, dtype=2, d=96) == TG_E_DTYPE, name
    assert call(decode, scratch=None) == TG_E_NULL and call(decode, scratch=odd) == TG_E_ALIGN
    for kw in (dict(nsplit=0), dict(nsplit=65), dict(nsplit=-1), dict(scratch_bytes=need - 1), dict(scratch_bytes=0), dict(max_seq=131072)):
        assert call(decode, **kw) == TG_E_SHAPE, kw
    assert call(decode, scratch_bytes=16, v_exp=odd) == TG_E_SHAPE and call(decode, nsplit=65, scratch_bytes=1 << 30, cos=odd) == TG_E_SHAPE
    assert call(prefill, max_seq=16384) == TG_E_SHAPE and call(prefill, slot=None) == TG_E_SHAPE   # n != cache_bs without slots
    assert call(prefill, out=odd) == TG_E_ALIGN

    z = torch.zeros(2, 8 * 64, dtype=torch.bfloat16)
    tabs = (torch.zeros(256, 64), torch.zeros(256, 64))
    pool = torch.zeros(5, 2, 64, 64, dtype=torch.uint8).view(torch.float8_e4m3fn)
    exp = torch.zeros(5, 2, 64, 2, dtype=torch.uint8)
    pool16 = torch.zeros(5, 2, 64, 64, dtype=torch.bfloat16)
    table, scratch = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(1024, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode_ops.rope_attn_online_mx8_paged(z, *tabs, torch.zeros(2, dtype=torch.long), table, pool, pool.clone(), exp, exp.clone(), 4, 2, 64,
                                              0.125, scratch, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode_ops.prefill_attn_mx8_paged(z, *tabs, torch.zeros(2, dtype=torch.long), table, pool, pool.clone(), exp, exp.clone(), 4, 2, 64, 0.125, 1)
    # 16-bit pools do not belong here (checked on the host, before the device check), nor do exponents of another type
    with pytest.raises(RuntimeError, match="mx8"):
        decode_ops.rope_attn_online_mx8_paged(z, *tabs, torch.zeros(2, dtype=torch.long), table, pool16, pool16.clone(), None, None, 4, 2, 64,
                                              0.125, scratch, 1)
    with pytest.raises(RuntimeError, match="mx8"):
        decode_ops.prefill_attn_mx8_paged(z, *tabs, torch.zeros(2, dtype=torch.long), table, pool16, pool16.clone(), None, None, 4, 2, 64, 0.125, 1)
    with pytest.raises(RuntimeError, match="uint8"):
        decode_ops.rope_attn_online_mx8_paged(z, *tabs, torch.zeros(2, dtype=torch.long), table, pool, pool.clone(), exp.to(torch.int8), exp.clone(),
                                              4, 2, 64, 0.125, scratch, 1)


def _stack(cfg, kv_pages=None, rank=0, world=1, **kw):
    s = DecodeStack(cfg, SeededDense(cfg, rank, world), "cpu", torch.float32, bs=BS, rank=rank, world=world, seed=7, ragged=True,
                    kv_cache="mx8", kv_pages=kv_pages, **kw)
    if kv_pages == PAGES:
        s.page_pool._free = list(SCRAMBLED)  # physical order has nothing to do with logical order
    return s


def _tokens(cfg, n, T, seed=0):
    return torch.randint(0, cfg.vocab, (n, T), generator=torch.Generator().manual_seed(seed))


def _bytes(t):
    return t.view(torch.uint8)


@pytest.fixture(scope="module")
def scenario():
    """tests/test_paged_cpu.py's: the paged stack and the contiguous one after the same prefill (lengths 130 / 1 / 65 / 200) and 64 decode
    steps -- slot 1 crosses position 64 and slot 2 position 128 (each maps a page on the way), slot 3 runs ten steps, slot 0 none."""
    cfg = DecodeConfig(**PCFG)
    paged, flat = _stack(cfg, PAGES), _stack(cfg)
    toks = _tokens(cfg, BS, 200)
    logits = [(paged.prefill(toks, position=0, lengths=LENGTHS).clone(), flat.prefill(toks, position=0, lengths=LENGTHS).clone())]
    steps = _tokens(cfg, 64, BS, seed=1)
    for i in range(64):
        position = [-1, 1 + i, 65 + i, 200 + i if i < 10 else -1]
        logits.append((paged.decode(steps[i], position).clone(), flat.decode(steps[i], position).clone(), position))
    return cfg, paged, flat, logits


def test_paged_mx8_stack_equals_the_contiguous_mx8_stack_bit_for_bit(scenario):
    cfg, paged, flat, logits = scenario
    assert paged.paged and paged.kv_cache == "mx8"
    for layer in paged.layers:
        assert layer.k_pool.dtype == layer.v_pool.dtype == torch.float8_e4m3fn and tuple(layer.k_pool.shape) == (PAGES, cfg.kv_heads, PS, 64)
        assert layer.k_exp_pool.dtype == layer.v_exp_pool.dtype == torch.uint8 and tuple(layer.v_exp_pool.shape) == (PAGES, cfg.kv_heads, PS, 2)
        assert layer.k_cache is None and layer.k_exp is None               # the contiguous views exist only inside _paged_view
    # (1 + 1/32) / 2 of a 16-bit pool of the same pages at 2 bytes per element (whatever the stack's dtype: codes are bytes)
    pool16 = cfg.layers * 2 * PAGES * cfg.kv_heads * PS * cfg.head_dim * 2
    assert paged.kv_cache_bytes() * 64 == pool16 * 33
    assert paged.kv_cache_bytes() * 32 == flat.kv_cache_bytes() * PAGES    # 12 of the 32 pages the contiguous mx8 stack holds
    assert torch.equal(logits[0][0], logits[0][1])
    for got, want, position in logits[1:]:
        active = [b for b, p in enumerate(position) if p >= 0]
        assert torch.equal(got[active], want[active]), position
    assert [paged._mapped(b) for b in range(BS)] == [3, 2, 3, 4] and paged.page_pool.free_pages == 0
    table = paged.block_table.tolist()
    assert table == paged._table and sorted(p for row in table for p in row if p >= 0) == list(range(PAGES))
    assert table[0][:3] != sorted(table[0][:3]) or table[3][:4] != sorted(table[3][:4])  # scrambled: not the identity layout
    # every code row and every exponent row of every slot is where the table says, and what the contiguous stack holds there
    for lp, lf in zip(paged.layers, flat.layers):
        for b, n in enumerate([130, 65, 129, 210]):
            for pool, cache in zip(POOLS, FLAT):
                pool, cache = _bytes(getattr(lp, pool)), _bytes(getattr(lf, cache))
                rows = torch.stack([pool[table[b][p // PS], :, p % PS] for p in range(n)], dim=1)
                assert torch.equal(rows, cache[b, :, :n]) and rows.any(), b
        # rows of a mapped page above its slot's last position were never written: zero bytes
        for b, n in enumerate([130, 65, 129, 210]):
            for pool in POOLS:
                assert not _bytes(getattr(lp, pool))[table[b][n // PS], :, n % PS:].any(), (b, pool)


def test_unmapped_pages_keep_their_zero_bytes():
    cfg = DecodeConfig(**PCFG)
    paged = _stack(cfg, PAGES)
    paged.prefill(_tokens(cfg, BS, 200), position=0, lengths=LENGTHS)      # 3 + 1 + 2 + 4 = 10 pages
    paged.decode(_tokens(cfg, 1, BS, seed=1)[0], [130, 1, 65, 200])
    used = {p for row in paged._table for p in row if p >= 0}
    spare = sorted(set(range(PAGES)) - used)
    assert len(used) == 10 and len(spare) == 2
    for layer in paged.layers:
        for pool in POOLS:
            assert not _bytes(getattr(layer, pool))[spare].any(), pool
            assert _bytes(getattr(layer, pool))[sorted(used)].any(), pool


def test_exhaustion_raises_before_anything_is_mapped_or_launched(scenario):
    cfg, paged, flat, _ = scenario
    assert paged.page_pool.free_pages == 0
    table, refs = [list(r) for r in paged._table], list(paged.page_pool.refs)
    pools = [[_bytes(getattr(layer, name)).clone() for name in POOLS] for layer in paged.layers]
    pos_before = paged.pos_seq.clone()
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        paged.reserve(0, 200)
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        paged.decode(_tokens(cfg, 1, BS)[0], [130, 65, 129, 256])          # slot 3 would need a fifth page
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        paged.prefill(_tokens(cfg, 1, 70), position=[130], slots=[0])      # 200 positions: a fourth page for slot 0
    assert paged._table == table and paged.block_table.tolist() == table and paged.page_pool.refs == refs
    assert torch.equal(paged.pos_seq, pos_before)
    assert all(torch.equal(_bytes(getattr(layer, name)), c) for layer, cs in zip(paged.layers, pools) for name, c in zip(POOLS, cs))
    paged.reserve(0, 130)                                                  # what is mapped already: idempotent
    assert paged._table == table


def test_release_then_prefill_into_the_recycled_pages(scenario):
    cfg, paged, _, _ = scenario
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
    """fork(src, dst, t): whole pages shared (t = 128: two of them, nothing copied; t = 70: one, and six rows of codes AND exponents copied
    into a fresh page).  dst then decodes like a slot that prefilled the first t tokens itself, and src goes on undisturbed."""
    cfg = DecodeConfig(**PCFG)
    paged, flat = _stack(cfg, PAGES), _stack(cfg)
    prompt = _tokens(cfg, 1, 130, seed=3)
    for s in (paged, flat):
        s.prefill(prompt, position=[0], slots=[0])
    flat.prefill(prompt[:, :t], position=[0], slots=[2])
    paged.reserve(2, 10)                                                   # dst is released first
    src_before = [[_bytes(getattr(layer, name))[paged._table[0][:3]].clone() for name in POOLS] for layer in paged.layers]
    paged.fork(0, 2, t)
    full, part = divmod(t, PS)
    assert paged._table[2][:full] == paged._table[0][:full] and paged._mapped(2) == -(-t // PS) and paged._mapped(0) == 3
    assert [paged.page_pool.refs[p] for p in paged._table[0][:3]] == [2] * full + [1] * (3 - full)
    assert paged.page_pool.free_pages == PAGES - 3 - (1 if part else 0) and paged.block_table.tolist() == paged._table
    for layer, before in zip(paged.layers, src_before):
        for name, b in zip(POOLS, before):
            pool = _bytes(getattr(layer, name))
            assert torch.equal(pool[paged._table[0][:3]], b), name         # src: undisturbed
            if part:                                                        # six rows copied, the rest of the fresh page untouched (zero)
                fresh, src = pool[paged._table[2][full]], pool[paged._table[0][full]]
                assert part == 6 and torch.equal(fresh[:, :part], src[:, :part]) and fresh[:, :part].any() and not fresh[:, part:].any(), name
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


def test_the_refusal_that_stays_and_what_is_built():
    """head_dim 16 / 32: kv_pages with kv_cache="mx8" keeps raising `not built yet`, from the stack and from the layer, ahead of the
    head_dim % 32 check; head_dim 64 builds, with either mx8_attention, and generate works on top."""
    for hd in (16, 32):
        cfg = DecodeConfig(**dict(CFG, head_dim=hd, max_seq=512))
        for kw in (dict(), dict(mx8_attention="online"), dict(fused=True)):
            with pytest.raises(ValueError, match="not built yet"):
                DecodeStack(cfg, SeededDense(cfg, 0, 1), "cpu", torch.float32, bs=2, seed=7, ragged=True, kv_pages=4, kv_cache="mx8", **kw)
        with pytest.raises(ValueError, match="not built yet"):
            DecodeLayer(cfg, 0, SeededDense(cfg, 0, 1), 0, 1, "cpu", torch.float32, 2, kv_cache="mx8", kv_pages=4)
    cfg = DecodeConfig(**PCFG)
    make = lambda **kw: DecodeStack(cfg, SeededDense(cfg, 0, 1), "cpu", torch.float32, bs=2, seed=7, kv_cache="mx8", **kw)
    with pytest.raises(ValueError, match="ragged=True"):
        make(kv_pages=4)
    for ps in (48, 32, 96, 1024):
        with pytest.raises(ValueError, match="page_size"):
            make(ragged=True, kv_pages=4, page_size=ps)
    plain = make(ragged=True)
    outs = []
    for m in ("split", "online"):                                           # a paged mx8 stack accepts either value
        paged = make(ragged=True, kv_pages=4, page_size=128, mx8_attention=m)
        prompts = [_tokens(cfg, 1, 120, seed=8)[0], _tokens(cfg, 1, 3, seed=9)[0]]
        outs.append(paged.generate(prompts, 12))
        assert [paged._mapped(b) for b in range(2)] == [2, 1] and paged.page_pool.free_pages == 1
        with pytest.raises(RuntimeError, match="KV page pool exhausted"):
            paged.generate([prompts[0], prompts[0]], 140)   # three pages each, one free
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], plain.generate(prompts, 12))


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
        same = tp._table == full._table and tp.page_pool.refs == full.page_pool.refs and \
            all(getattr(tp.layers[0], name).shape[1] * world == cfg.kv_heads for name in POOLS)
        results[rank] = float(err) if same else float("inf")
    finally:
        dist.destroy_process_group()


def test_tensor_parallel_paged_mx8_gloo():
    """Heads / rows split over two ranks, the table and the pool's decisions replicated, the four pools per rank == the unsharded paged
    mx8 stack."""
    import torch.multiprocessing as mp

    world = 2
    port = 39500 + (os.getpid() % 2000)
    results = mp.Manager().dict()
    mp.spawn(_tp_worker, args=(world, port, results), nprocs=world, join=True)
    assert set(results.keys()) == {0, 1}
    assert max(results.values()) < ATOL, dict(results)
