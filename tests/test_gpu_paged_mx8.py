"""GPU suite: the paged mx8 KV cache -- dg_rope_attn_online_mx8_paged (nsplit 1 / 4) and dg_prefill_attn_mx8_paged bit for bit against
dg_rope_attn_online_mx8_seq / dg_prefill_attn_mx8_seq on contiguous mx8 caches that hold the same bytes (pages in reverse physical order,
two spare pages, guard bytes on both sides of each of the FOUR buffers: every byte of codes and exponents is compared), the table guards,
and DecodeStack(..., ragged=True, kv_cache="mx8", kv_pages=N) on the HIP linears: torch.equal to the contiguous ragged fused mx8 stack
(mx8_attention="online") over prefill, steps across page edges, release / reuse and fork, through a captured graph with a page mapped
between replays, and against the dense twin's plain-torch paged mx8 path under the contract of tests/test_gpu_decode.py.
The comparison is bit for bit (NaN == NaN): no tolerance is involved."""
import math

import numpy as np
import pytest
import torch

from tests.conftest import bits16
from tests.test_gpu_decode import CFG, _PairedFactories

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_numerics")]
DEV = "cuda:0"
F8 = torch.float8_e4m3fn
SENTINEL = 7.0
SPARE, GUARD = 0x33, 0xA5                            # bytes of the spare pages and of the guards (codes and exponents alike)
GUARD_BYTES = 4096                                   # (a multiple of 16: the pools stay 16-byte aligned)
GEOMETRIES = [(4, 1, 128), (4, 2, 64), (8, 8, 128)]  # (8, 8, 128): the online kernel's head remap
S = 512                                              # both 256-position chunks of the one-barrier kernel


def _tables(d, max_seq):
    from any4_amd.decode import DecodeConfig, _rope_tables

    return _rope_tables(DecodeConfig(head_dim=d, max_seq=max_seq), DEV)


def _same(a, b):
    """Bit for bit (NaN == NaN)."""
    return np.array_equal(bits16(a), bits16(b))


def _dev(vals):
    return torch.tensor(vals, dtype=torch.long, device=DEV)


def _caches(gen, dtype, prefixes, kvl, d):
    """Contiguous mx8 caches as bytes -- (k codes, v codes, k exps, v exps), uint8 [n][kvl][S][d] and [n][kvl][S][d / 32]: mx8_encode of a
    standard-normal prefix per slot; above it exponent 255 and code 0x7f, the format's NaN block."""
    from any4_amd.kvcache import mx8_encode

    n = len(prefixes)
    out = []
    for _ in range(2):
        codes = torch.full((n, kvl, S, d), 0x7F, device=DEV, dtype=torch.uint8)
        exps = torch.full((n, kvl, S, d // 32), 255, device=DEV, dtype=torch.uint8)
        for b, p in enumerate(prefixes):
            if p:
                c, e = mx8_encode(torch.randn(kvl, p, d, device=DEV, generator=gen).to(dtype))
                codes[b, :, :p], exps[b, :, :p] = c.view(torch.uint8), e
        out.append((codes, exps))
    (kc, ke), (vc, ve) = out
    return kc, vc, ke, ve


class _Pools:
    """The rows of contiguous caches [n][kvl][S][w] (bytes) in pools [num_pages][kvl][ps][w]: entry e of sequence b is the (e * n + b)-th
    page in REVERSE physical order, two spare pages (physical 0 and the middle one) hold SPARE, and each pool sits between GUARD_BYTES guard
    bytes in one buffer.  One table serves the code pools (w = d) and the exponent pools (w = d / 32)."""

    def __init__(self, n, kvl, ps):
        self.n, self.kvl, self.ps, self.entries = n, kvl, ps, S // ps
        self.num_pages = n * self.entries + 2
        spare = {0, self.num_pages // 2}
        order = [p for p in reversed(range(self.num_pages)) if p not in spare]
        self.spare = sorted(spare)
        self.table = torch.tensor([[order[e * n + b] for e in range(self.entries)] for b in range(n)], dtype=torch.int32, device=DEV)

    def fill(self, cache):
        """(buffer, pool view) holding `cache`'s rows"""
        shape = (self.num_pages, self.kvl, self.ps, cache.shape[-1])
        numel = math.prod(shape)
        buf = torch.full((numel + 2 * GUARD_BYTES,), GUARD, device=DEV, dtype=torch.uint8)
        pool = buf[GUARD_BYTES: GUARD_BYTES + numel].view(shape)
        pool[self.spare] = SPARE
        pages = cache.view(self.n, self.kvl, self.entries, self.ps, -1).permute(0, 2, 1, 3, 4)  # [n][entries][kvl][ps][w]
        pool[self.table.long()] = pages
        return buf, pool

    def fill4(self, caches):
        """the four buffers and the four pool views as the wrappers take them (codes as float8_e4m3fn)"""
        bufs, pools = zip(*[self.fill(c) for c in caches])
        return list(bufs), [pools[0].view(F8), pools[1].view(F8), pools[2], pools[3]]

    def same4(self, bufs, caches):
        return [torch.equal(b, self.fill(c)[0]) for b, c in zip(bufs, caches)]


def _f8(caches):
    return [caches[0].view(F8), caches[1].view(F8), caches[2], caches[3]]


POSITIONS = [[0, 63, 64], [65, 127, 128], [255, 256, 257], [511, -1, 5]]  # page edges, iteration edges, the chunk edge, the end; inactive


@pytest.mark.parametrize("page_size", [64, 128, 512])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_paged_mx8_decode_equals_the_contiguous_mx8_kernel_bit_for_bit(dtype, geometry, page_size):
    """Outputs and the four pools (the written row of codes and of exponents, every other byte, the spare pages, the guards) of
    dg_rope_attn_online_mx8_paged at nsplit 1 / 4 are those of dg_rope_attn_online_mx8_seq at the same nsplit on the contiguous caches."""
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    bs, scale = 3, 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(hl * 100 + d + page_size)
    pools = _Pools(bs, kvl, page_size)
    scratch = {ns: G.rope_attn_split_scratch(bs, hl, d, ns, DEV) for ns in (1, 4)}
    for positions in POSITIONS:
        caches = _caches(gen, dtype, [max(p, 0) for p in positions], kvl, d)
        qkv = torch.randn(bs, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
        pos = _dev(positions)
        for ns in (1, 4):
            what = (positions, ns)
            flat = [c.clone() for c in caches]
            want = torch.full((bs, hl * d), SENTINEL, device=DEV, dtype=dtype)
            got = want.clone()
            bufs, views = pools.fill4(caches)
            G.rope_attn_online_mx8(qkv, cos, sin, pos, *_f8(flat), hl, kvl, d, scale, scratch[ns], ns, per_sequence=True, out=want)
            G.rope_attn_online_mx8_paged(qkv, cos, sin, pos, pools.table, *views, hl, kvl, d, scale, scratch[ns], ns, out=got)
            active = [b for b, p in enumerate(positions) if p >= 0]
            # never vacuous: the contiguous kernel gave finite outputs and did write a row of codes and of exponents
            assert torch.isfinite(want[active].float()).all(), what
            assert not any(torch.equal(a, b) for a, b in zip(flat, caches)), what
            assert _same(got, want), what
            for b, p in enumerate(positions):
                if p < 0:
                    assert (got[b] == SENTINEL).all(), what
            # the whole buffers: guards, spare pages, untouched rows, and the one written row per active sequence
            assert pools.same4(bufs, flat) == [True] * 4, what


PREFILL_LEN, PREFILL_SLOT, T = [130, 1, 65, 0], [2, 0, 3, -1], 130


@pytest.mark.parametrize("p0", [0, 70, S - 3])  # 70: the chunk's rows cross positions 128 and 192 mid-chunk; S - 3: three tokens fit
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_paged_mx8_prefill_equals_the_contiguous_mx8_kernel_bit_for_bit(dtype, geometry, p0):
    """len 130 / 1 / 65 / 0 into slots 2 / 0 / 3 / -1 of 4, 64-position pages, NaN blocks above the prefixes: the outputs (the sentinel
    where no token exists) and the four whole pool buffers are dg_prefill_attn_mx8_seq's on the contiguous caches."""
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    n, cache_bs, scale = 4, 4, 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(hl + d + p0)
    qkv = torch.randn(n * T, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    caches = _caches(gen, dtype, [p0] * cache_bs, kvl, d)
    pools = _Pools(cache_bs, kvl, 64)
    bufs, views = pools.fill4(caches)
    pos, lens, slots = _dev([p0] * n), _dev(PREFILL_LEN), _dev(PREFILL_SLOT)
    want = torch.full((n * T, hl * d), SENTINEL, device=DEV, dtype=dtype)
    got = want.clone()
    flat = [c.clone() for c in caches]
    k1, v1, ke1, ve1 = _f8(flat)
    G.prefill_attn(qkv, cos, sin, pos, k1, v1, hl, kvl, d, scale, T, out=want, lengths=lens, slots=slots, k_exp=ke1, v_exp=ve1)
    G.prefill_attn_mx8_paged(qkv, cos, sin, pos, pools.table, *views, hl, kvl, d, scale, T, out=got, lengths=lens, slots=slots)
    w3 = want.view(n, T, -1)
    for i, L in enumerate(PREFILL_LEN):
        inside = max(0, min(L, S - p0))
        assert torch.isfinite(w3[i, :inside].float()).all() and (w3[i, inside:] == SENTINEL).all(), i
    assert not any(torch.equal(a, b) for a, b in zip(flat, caches)) and all(torch.equal(a[1], b[1]) for a, b in zip(flat, caches))
    assert _same(got, want)
    assert pools.same4(bufs, flat) == [True] * 4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_table_guards(dtype):
    """(a) Entries above a sequence's last used page at -1 -- the normal case -- change nothing.  (b) A sequence whose own write page is -1
    leaves all four buffers byte-identical, in the decode kernel and in prefill.  (c) d = 96 and page_size = 48 are TG_E_SHAPE and touch
    nothing."""
    from any4_amd import decode_ops as G

    hl, kvl, d = 4, 2, 64
    bs, ps, scale = 3, 64, 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(11)
    pools = _Pools(bs, kvl, ps)
    positions = [70, 256, 5]
    caches = _caches(gen, dtype, positions, kvl, d)
    qkv = torch.randn(bs, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    scr = {ns: G.rope_attn_split_scratch(bs, hl, d, ns, DEV) for ns in (1, 4)}
    trimmed, unmapped = pools.table.clone(), pools.table.clone()
    for b, p in enumerate(positions):
        trimmed[b, p // ps + 1:] = -1
        unmapped[b, p // ps] = -1
    untouched = [pools.fill(c)[0] for c in caches]
    runs = {}
    for name, table in (("full", pools.table), ("trimmed", trimmed), ("unmapped", unmapped)):
        for ns in (1, 4):
            bufs, views = pools.fill4(caches)
            out = torch.full((bs, hl * d), SENTINEL, device=DEV, dtype=dtype)
            G.rope_attn_online_mx8_paged(qkv, cos, sin, _dev(positions), table, *views, hl, kvl, d, scale, scr[ns], ns, out=out)
            runs[name, ns] = (out, bufs)
    # prefill: sequence 0 appends 70 ... 89 (page 1 of its row), sequence 1 at 256; their write pages unmapped -> the pools unchanged
    n, Tp = 2, 20
    pq = torch.randn(n * Tp, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    for name, table in (("full", pools.table), ("trimmed", trimmed), ("unmapped", unmapped)):
        bufs, views = pools.fill4(caches)
        out = torch.full((n * Tp, hl * d), SENTINEL, device=DEV, dtype=dtype)
        G.prefill_attn_mx8_paged(pq, cos, sin, _dev(positions[:2]), table, *views, hl, kvl, d, scale, Tp, out=out, slots=_dev([0, 1]))
        runs[name, "prefill"] = (out, bufs)
    for key in (1, 4, "prefill"):
        out, bufs = runs["full", key]
        assert torch.isfinite(out.float()).all() and not any(torch.equal(a, b) for a, b in zip(bufs, untouched)), key
        assert _same(runs["trimmed", key][0], out) and all(torch.equal(a, b) for a, b in zip(runs["trimmed", key][1], bufs)), key
        assert all(torch.equal(a, b) for a, b in zip(runs["unmapped", key][1], untouched)), key
    # (c) refused shapes: nothing is launched
    for dd, pp, ss in ((96, 64, S), (64, 48, 480)):
        c, s = _tables(dd, ss)
        kp = torch.full((4, kvl, pp, dd), SPARE, device=DEV, dtype=torch.uint8)
        ke = torch.full((4, kvl, pp, dd // 32), SPARE, device=DEV, dtype=torch.uint8)
        vp, ve, out = kp.clone(), ke.clone(), torch.full((bs, hl * dd), SENTINEL, device=DEV, dtype=dtype)
        table = torch.zeros(bs, ss // pp, dtype=torch.int32, device=DEV)
        q = torch.randn(bs, (hl + 2 * kvl) * dd, device=DEV, generator=gen).to(dtype)
        sc = G.rope_attn_split_scratch(bs, hl, dd, 4, DEV)
        args = (q, c, s, _dev([1, 2, 3]), table, kp.view(F8), vp.view(F8), ke, ve, hl, kvl, dd, 1.0)
        for call in (lambda: G.rope_attn_online_mx8_paged(*args, sc, 4, out=out), lambda: G.prefill_attn_mx8_paged(*args, 1, out=out)):
            with pytest.raises(RuntimeError, match=r"code -7"):
                call()
        assert all((t == SPARE).all() for t in (kp, vp, ke, ve)) and (out == SENTINEL).all()


# ---------------------------------------------------------------- the stack
def _contract(a, b, what):
    a, b = a.float(), b.float()
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    print(f"{what}: err {err:.4e} allowed {0.03 * ref + 1e-3:.4e}")
    assert torch.isfinite(a).all() and err <= 0.03 * ref + 1e-3, (what, err, ref)


PAGES, PS, BS = 12, 64, 4
LENGTHS = [130, 1, 65, 200]
SCRAMBLED = [5, 0, 11, 3, 7, 1, 9, 2, 10, 4, 8, 6]
FLAT = ("k_cache", "v_cache", "k_exp", "v_exp")
POOLS = ("k_pool", "v_pool", "k_exp_pool", "v_exp_pool")


@pytest.mark.parametrize("fuse_gemm_stages", [True, False])
def test_paged_mx8_fused_stack_equals_the_contiguous_mx8_fused_stack(oracle, fuse_gemm_stages):
    """bs 4, max_seq 512, head_dim 64, 12 pages of 64 with a scrambled free list, five and eight launches: prefill with lengths, 64 steps
    across page edges, release and reuse, fork at 128 and at 70 -- logits torch.equal to the contiguous ragged fused stack with
    kv_cache="mx8", mx8_attention="online" -- and the contract against the dense twin's plain-torch paged mx8 path."""
    from any4_amd.decode import DecodeConfig, DecodeStack

    cfg = DecodeConfig(**dict(CFG, max_seq=512))
    assert cfg.head_dim == 64
    fac = _PairedFactories(oracle, cfg, "linear_y_f16RM_x_f16RM_W_any4TC")
    kw = dict(bs=BS, seed=5, ragged=True, kv_cache="mx8")
    paged = DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, fused=True, fuse_gemm_stages=fuse_gemm_stages, kv_pages=PAGES, page_size=PS, **kw)
    flat = DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, fused=True, fuse_gemm_stages=fuse_gemm_stages, mx8_attention="online", **kw)
    twin = DecodeStack(cfg, fac.dense, DEV, torch.bfloat16, fused=False, kv_pages=PAGES, page_size=PS, **kw)
    assert paged.kv_cache_bytes() * 32 == flat.kv_cache_bytes() * PAGES and paged._five_launch() == fuse_gemm_stages
    assert paged.kv_cache_bytes() * 64 == cfg.layers * 2 * PAGES * cfg.kv_heads * PS * cfg.head_dim * 2 * 33
    for s in (paged, twin):
        s.page_pool._free = list(SCRAMBLED)
    toks = torch.randint(0, cfg.vocab, (BS, 200 + 64), generator=torch.Generator().manual_seed(1)).to(DEV)
    a, b, c = [s.prefill(toks[:, :200], position=0, lengths=LENGTHS) for s in (paged, flat, twin)]
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    _contract(a, c, "paged mx8 prefill any4 vs dense twin")
    for i in range(64):
        position = [-1, 1 + i, 65 + i, 200 + i if i < 10 else -1]
        active = [s for s, p in enumerate(position) if p >= 0]
        a, b = paged.decode(toks[:, 200 + i], position), flat.decode(toks[:, 200 + i], position)
        assert torch.equal(a[active], b[active]), i
        c = twin.decode(toks[:, 200 + i], position)
        if i % 9 == 0 or i == 63:
            _contract(a[active], c[active], f"paged mx8 decode {i} any4 vs dense twin")
    assert paged.page_pool.free_pages == 0 and paged._table == twin._table and paged.block_table.tolist() == paged._table
    # every code and exponent row is where the table says, and what the contiguous stack holds
    for lp, lf in zip(paged.layers, flat.layers):
        for b, n in enumerate([130, 65, 129, 210]):
            pages = torch.tensor([paged._table[b][p // PS] for p in range(n)], device=DEV)
            rows = torch.arange(n, device=DEV) % PS
            for pool, cache in zip(POOLS, FLAT):
                got = getattr(lp, pool).view(torch.uint8)[pages, :, rows].transpose(0, 1)
                assert torch.equal(got, getattr(lf, cache).view(torch.uint8)[b, :, :n]), (b, pool)
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        paged.decode(toks[:, 0], [130, -1, -1, 210 + 46])
    # release and reuse: a new prompt into slot 3's recycled pages
    prompt = torch.randint(0, cfg.vocab, (1, 150), generator=torch.Generator().manual_seed(2)).to(DEV)
    paged.release(3)
    assert torch.equal(paged.prefill(prompt, position=[0], slots=[3]), flat.prefill(prompt, position=[0], slots=[3]))
    # fork: the contiguous stack copies the prefix rows, the paged one shares pages (t = 128) or shares one and copies six rows (t = 70)
    for src, dst, t, position in ((0, 1, 128, [130, 128, 129, 150]), (2, 1, 70, [131, 70, 130, 151])):
        paged.fork(src, dst, t)
        for layer in flat.layers:
            for name in FLAT:
                cache = getattr(layer, name).view(torch.uint8)
                cache[dst, :, :t] = cache[src, :, :t]
        assert paged._table[dst][: t // PS] == paged._table[src][: t // PS] and paged._mapped(dst) == -(-t // PS)
        a, b = paged.decode(toks[:, t], position), flat.decode(toks[:, t], position)
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), t
    with pytest.raises(ValueError, match="share"):
        paged.decode(toks[:, 0], [-1, -1, 10, -1])


def test_paged_mx8_graph_replays_with_a_page_mapped_between_replays():
    """A captured paged mx8 step (max_seq 2048: the split launch, four blocks per head) replayed with three position vectors -- one with
    an inactive sequence, the last a device tensor that crosses a page edge, its page mapped by hand between two replays -- gives the
    eager contiguous ragged mx8 stack's (mx8_attention="online") logits in bits."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**dict(CFG, max_seq=2048))
    bs = 3
    kw = dict(bs=bs, seed=9, ragged=True, kv_cache="mx8")
    eager = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, mx8_attention="online", **kw)
    graph = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, kv_pages=8, page_size=64, **kw)
    assert graph._attn_split == 4 and graph._attn_scratch is not None and eager._attn_split == 4
    graph.capture()  # (nothing is mapped yet: the warm-up steps write nothing)
    assert graph._graph is not None
    assert not any(getattr(layer, name).view(torch.uint8).any() for layer in graph.layers for name in POOLS)
    toks = torch.randint(0, cfg.vocab, (bs, 70), generator=torch.Generator().manual_seed(2)).to(DEV)
    lengths = [62, 9, 5]
    for stack in (eager, graph):
        stack.prefill(toks[:, :62], lengths=lengths)
    assert [graph._mapped(b) for b in range(bs)] == [1, 1, 1]
    for i, position in enumerate(([62, 9, 5], [63, -1, 6], _dev([64, 10, 7]))):
        if i == 2:
            graph.reserve(0, 65)  # a device position: reservation is the caller's
            assert graph._mapped(0) == 2
        a, b = eager.decode(toks[:, 62 + i], position), graph.decode(toks[:, 62 + i], position).clone()
        rows = [s for s in range(bs) if i != 1 or s != 1]
        assert torch.isfinite(a[rows].float()).all() and torch.equal(a[rows], b[rows]), i
    for le, lg in zip(eager.layers, graph.layers):
        for b, n in enumerate([65, 11, 8]):
            for pool, cache in zip(POOLS, FLAT):
                p8 = getattr(lg, pool).view(torch.uint8)
                rows = torch.stack([p8[graph._table[b][p // 64], :, p % 64] for p in range(n)], dim=1)
                assert torch.equal(rows, getattr(le, cache).view(torch.uint8)[b, :, :n]), (b, pool)
