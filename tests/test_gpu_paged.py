"""GPU suite: the paged KV cache -- dg_rope_attn_online_paged / dg_rope_attn_split_paged / dg_prefill_attn_paged bit for bit against their
_seq namesakes on a contiguous cache that holds the same rows (pages interleaved in reverse physical order, spare pages and guard bytes
around the pools untouched), the table guards, and DecodeStack(..., ragged=True, kv_pages=N) on the HIP linears: torch.equal to the
contiguous ragged fused stack over prefill, steps across page edges, release / reuse and fork, through a captured graph with a page
mapped between replays, and against the dense twin's plain-torch paged path under the contract of tests/test_gpu_decode.py."""
import math

import numpy as np
import pytest
import torch

from tests.conftest import bits16
from tests.test_gpu_decode import CFG, _PairedFactories

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_numerics")]
DEV = "cuda:0"
SENTINEL, SPARE, GUARD = 7.0, 3.0, -5.0
GUARD_ELEMS = 4096                                   # (a multiple of 8: the pools stay 16-byte aligned)
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
    """[len(prefixes)][kvl][S][d] x 2, NaN above a standard-normal prefix per slot."""
    n = len(prefixes)
    kc = torch.full((n, kvl, S, d), float("nan"), device=DEV, dtype=dtype)
    vc = torch.full((n, kvl, S, d), float("nan"), device=DEV, dtype=dtype)
    for b, p in enumerate(prefixes):
        kc[b, :, :p] = torch.randn(kvl, p, d, device=DEV, generator=gen).to(dtype)
        vc[b, :, :p] = torch.randn(kvl, p, d, device=DEV, generator=gen).to(dtype)
    return kc, vc


class _Pools:
    """The rows of contiguous caches [n][kvl][S][d] in pools [num_pages][kvl][ps][d]: entry e of sequence b is the (e * n + b)-th page in
    REVERSE physical order, two spare pages (physical 0 and the middle one) hold SPARE, and each pool sits between GUARD_ELEMS guard
    elements in one buffer."""

    def __init__(self, n, kvl, d, ps, dtype):
        self.n, self.ps, self.entries = n, ps, S // ps
        self.num_pages = n * self.entries + 2
        spare = {0, self.num_pages // 2}
        order = [p for p in reversed(range(self.num_pages)) if p not in spare]
        self.spare = sorted(spare)
        self.table = torch.tensor([[order[e * n + b] for e in range(self.entries)] for b in range(n)], dtype=torch.int32, device=DEV)
        self.shape, self.dtype = (self.num_pages, kvl, ps, d), dtype

    def fill(self, cache):
        """(buffer, pool view) holding `cache`'s rows"""
        numel = math.prod(self.shape)
        buf = torch.full((numel + 2 * GUARD_ELEMS,), GUARD, device=DEV, dtype=self.dtype)
        pool = buf[GUARD_ELEMS: GUARD_ELEMS + numel].view(self.shape)
        pool[self.spare] = SPARE
        pages = cache.view(self.n, cache.shape[1], self.entries, self.ps, -1).permute(0, 2, 1, 3, 4)  # [n][entries][kvl][ps][d]
        pool[self.table.long()] = pages
        return buf, pool


POSITIONS = [[0, 63, 64], [65, 127, 128], [255, 256, 257], [511, -1, 5]]  # page edges, iteration edges, the chunk edge, the end; inactive


@pytest.mark.parametrize("page_size", [64, 128, 512])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_paged_decode_kernels_equal_the_seq_kernels_bit_for_bit(dtype, geometry, page_size):
    """Outputs and pools (written rows, every other byte, the spare pages, the guards) of dg_rope_attn_online_paged and of
    dg_rope_attn_split_paged at nsplit 1 / 4 are those of dg_rope_attn_online_seq / dg_rope_attn_split_seq on the contiguous cache."""
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    bs, scale = 3, 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(hl * 100 + d + page_size)
    pools = _Pools(bs, kvl, d, page_size, dtype)
    scratch = {ns: G.rope_attn_split_scratch(bs, hl, d, ns, DEV) for ns in (1, 4)}
    for positions in POSITIONS:
        kc, vc = _caches(gen, dtype, [max(p, 0) for p in positions], kvl, d)
        qkv = torch.randn(bs, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
        pos = _dev(positions)
        for ns in (None, 1, 4):
            what = (positions, ns)
            k1, v1 = kc.clone(), vc.clone()
            want = torch.full((bs, hl * d), SENTINEL, device=DEV, dtype=dtype)
            (kbuf, kp), (vbuf, vp) = pools.fill(kc), pools.fill(vc)
            got = want.clone()
            if ns is None:
                G.rope_attn_online(qkv, cos, sin, pos, k1, v1, hl, kvl, d, scale, per_sequence=True, out=want)
                G.rope_attn_online_paged(qkv, cos, sin, pos, pools.table, kp, vp, hl, kvl, d, scale, out=got)
            else:
                G.rope_attn_split(qkv, cos, sin, pos, k1, v1, hl, kvl, d, scale, scratch[ns], ns, per_sequence=True, out=want)
                G.rope_attn_split_paged(qkv, cos, sin, pos, pools.table, kp, vp, hl, kvl, d, scale, scratch[ns], ns, out=got)
            active = [b for b, p in enumerate(positions) if p >= 0]
            assert torch.isfinite(want[active].float()).all() and not _same(k1, kc), what
            assert _same(got, want), what
            for b, p in enumerate(positions):
                if p < 0:
                    assert (got[b] == SENTINEL).all(), what
            # the whole buffer: guards, spare pages, untouched rows, and the one written row per active sequence
            assert _same(kbuf, pools.fill(k1)[0]) and _same(vbuf, pools.fill(v1)[0]), what


PREFILL_LEN, PREFILL_SLOT, T = [130, 1, 65, 0], [2, 0, 3, -1], 130


@pytest.mark.parametrize("p0", [0, 70, S - 3])  # 70: the chunk's rows cross positions 128 and 192 mid-chunk; S - 3: three tokens fit
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_paged_prefill_equals_the_seq_kernel_bit_for_bit(dtype, geometry, p0):
    """len 130 / 1 / 65 / 0 into slots 2 / 0 / 3 / -1 of 4, 64-position pages, NaN above the prefixes: the outputs (the sentinel where no
    token exists) and the whole pool buffers are dg_prefill_attn_seq's on the contiguous caches."""
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    n, cache_bs, scale = 4, 4, 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(hl + d + p0)
    qkv = torch.randn(n * T, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    kc, vc = _caches(gen, dtype, [p0] * cache_bs, kvl, d)
    pools = _Pools(cache_bs, kvl, d, 64, dtype)
    (kbuf, kp), (vbuf, vp) = pools.fill(kc), pools.fill(vc)
    pos, lens, slots = _dev([p0] * n), _dev(PREFILL_LEN), _dev(PREFILL_SLOT)
    want = torch.full((n * T, hl * d), SENTINEL, device=DEV, dtype=dtype)
    got = want.clone()
    k1, v1 = kc.clone(), vc.clone()
    G.prefill_attn(qkv, cos, sin, pos, k1, v1, hl, kvl, d, scale, T, out=want, lengths=lens, slots=slots)
    G.prefill_attn_paged(qkv, cos, sin, pos, pools.table, kp, vp, hl, kvl, d, scale, T, out=got, lengths=lens, slots=slots)
    w3 = want.view(n, T, -1)
    for i, L in enumerate(PREFILL_LEN):
        inside = max(0, min(L, S - p0))
        assert torch.isfinite(w3[i, :inside].float()).all() and (w3[i, inside:] == SENTINEL).all(), i
    assert not _same(k1, kc) and _same(k1[1], kc[1])
    assert _same(got, want)
    assert _same(kbuf, pools.fill(k1)[0]) and _same(vbuf, pools.fill(v1)[0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_table_guards(dtype):
    """(a) Entries above a sequence's last used page at -1 -- the normal case -- change nothing.  (b) A sequence whose own write page is -1
    leaves both pools byte-identical, in the decode kernels and in prefill.  (c) d = 96 and page_size = 48 are TG_E_SHAPE and touch nothing."""
    from any4_amd import decode_ops as G

    hl, kvl, d = 4, 2, 64
    bs, ps, scale = 3, 64, 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(11)
    pools = _Pools(bs, kvl, d, ps, dtype)
    positions = [70, 256, 5]
    kc, vc = _caches(gen, dtype, positions, kvl, d)
    qkv = torch.randn(bs, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    scr = G.rope_attn_split_scratch(bs, hl, d, 4, DEV)
    trimmed, unmapped = pools.table.clone(), pools.table.clone()
    for b, p in enumerate(positions):
        trimmed[b, p // ps + 1:] = -1
        unmapped[b, p // ps] = -1
    runs = {}
    for name, table in (("full", pools.table), ("trimmed", trimmed), ("unmapped", unmapped)):
        for ns in (None, 4):
            (kbuf, kp), (vbuf, vp) = pools.fill(kc), pools.fill(vc)
            out = torch.full((bs, hl * d), SENTINEL, device=DEV, dtype=dtype)
            if ns is None:
                G.rope_attn_online_paged(qkv, cos, sin, _dev(positions), table, kp, vp, hl, kvl, d, scale, out=out)
            else:
                G.rope_attn_split_paged(qkv, cos, sin, _dev(positions), table, kp, vp, hl, kvl, d, scale, scr, ns, out=out)
            runs[name, ns] = (out, kbuf, vbuf)
    untouched = (pools.fill(kc)[0], pools.fill(vc)[0])
    for ns in (None, 4):
        assert torch.isfinite(runs["full", ns][0].float()).all() and not _same(runs["full", ns][1], untouched[0])
        assert all(_same(a, b) for a, b in zip(runs["trimmed", ns], runs["full", ns])), ns
        assert _same(runs["unmapped", ns][1], untouched[0]) and _same(runs["unmapped", ns][2], untouched[1]), ns
    # prefill: sequence 0 appends 70 ... 89 (pages 1 of its row), sequence 1 at 256; their write pages unmapped -> both pools unchanged
    n, Tp = 2, 20
    pq = torch.randn(n * Tp, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    for name, table in (("full", pools.table), ("trimmed", trimmed), ("unmapped", unmapped)):
        (kbuf, kp), (vbuf, vp) = pools.fill(kc), pools.fill(vc)
        out = torch.full((n * Tp, hl * d), SENTINEL, device=DEV, dtype=dtype)
        G.prefill_attn_paged(pq, cos, sin, _dev(positions[:2]), table, kp, vp, hl, kvl, d, scale, Tp, out=out, slots=_dev([0, 1]))
        runs[name, "prefill"] = (out, kbuf, vbuf)
    assert torch.isfinite(runs["full", "prefill"][0].float()).all() and not _same(runs["full", "prefill"][1], untouched[0])
    assert all(_same(a, b) for a, b in zip(runs["trimmed", "prefill"], runs["full", "prefill"]))
    assert _same(runs["unmapped", "prefill"][1], untouched[0]) and _same(runs["unmapped", "prefill"][2], untouched[1])
    # (c) refused shapes: nothing is launched
    for dd, pp, ss in ((96, 64, S), (64, 48, 480)):
        c, s = _tables(dd, ss)
        kp = torch.full((4, kvl, pp, dd), SPARE, device=DEV, dtype=dtype)
        vp, out = kp.clone(), torch.full((bs, hl * dd), SENTINEL, device=DEV, dtype=dtype)
        table = torch.zeros(bs, ss // pp, dtype=torch.int32, device=DEV)
        q = torch.randn(bs, (hl + 2 * kvl) * dd, device=DEV, generator=gen).to(dtype)
        scr = G.rope_attn_split_scratch(bs, hl, dd, 4, DEV)
        for call in (lambda: G.rope_attn_online_paged(q, c, s, _dev([1, 2, 3]), table, kp, vp, hl, kvl, dd, 1.0, out=out),
                     lambda: G.rope_attn_split_paged(q, c, s, _dev([1, 2, 3]), table, kp, vp, hl, kvl, dd, 1.0, scr, 4, out=out),
                     lambda: G.prefill_attn_paged(q, c, s, _dev([1, 2, 3]), table, kp, vp, hl, kvl, dd, 1.0, 1, out=out)):
            with pytest.raises(RuntimeError, match=r"code -7"):
                call()
        assert (kp == SPARE).all() and (vp == SPARE).all() and (out == SENTINEL).all()


# ---------------------------------------------------------------- the stack
def _contract(a, b, what):
    a, b = a.float(), b.float()
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    print(f"{what}: err {err:.4e} allowed {0.03 * ref + 1e-3:.4e}")
    assert torch.isfinite(a).all() and err <= 0.03 * ref + 1e-3, (what, err, ref)


PAGES, PS, BS = 12, 64, 4
LENGTHS = [130, 1, 65, 200]
SCRAMBLED = [5, 0, 11, 3, 7, 1, 9, 2, 10, 4, 8, 6]


@pytest.mark.parametrize("fuse_gemm_stages", [True, False])
def test_paged_fused_stack_equals_the_contiguous_fused_stack(oracle, fuse_gemm_stages):
    """bs 4, max_seq 512, 12 pages of 64 with a scrambled free list (the contiguous stack holds 32 pages' worth), five and eight launches:
    prefill with lengths, 64 steps across page edges, release and reuse, fork at 128 and at 70 -- logits torch.equal to the contiguous
    ragged fused stack -- and the contract against the dense twin's plain-torch paged path."""
    from any4_amd.decode import DecodeConfig, DecodeStack

    cfg = DecodeConfig(**dict(CFG, max_seq=512))
    fac = _PairedFactories(oracle, cfg, "linear_y_f16RM_x_f16RM_W_any4TC")
    kw = dict(bs=BS, seed=5, ragged=True)
    paged = DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, fused=True, fuse_gemm_stages=fuse_gemm_stages, kv_pages=PAGES, page_size=PS, **kw)
    flat = DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, fused=True, fuse_gemm_stages=fuse_gemm_stages, **kw)
    twin = DecodeStack(cfg, fac.dense, DEV, torch.bfloat16, fused=False, kv_pages=PAGES, page_size=PS, **kw)
    assert paged.kv_cache_bytes() * 32 == flat.kv_cache_bytes() * PAGES and paged._five_launch() == fuse_gemm_stages
    for s in (paged, twin):
        s.page_pool._free = list(SCRAMBLED)
    toks = torch.randint(0, cfg.vocab, (BS, 200 + 64), generator=torch.Generator().manual_seed(1)).to(DEV)
    a, b, c = [s.prefill(toks[:, :200], position=0, lengths=LENGTHS) for s in (paged, flat, twin)]
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    _contract(a, c, "paged prefill any4 vs dense twin")
    for i in range(64):
        position = [-1, 1 + i, 65 + i, 200 + i if i < 10 else -1]
        active = [s for s, p in enumerate(position) if p >= 0]
        a, b = paged.decode(toks[:, 200 + i], position), flat.decode(toks[:, 200 + i], position)
        assert torch.equal(a[active], b[active]), i
        c = twin.decode(toks[:, 200 + i], position)
        if i % 9 == 0 or i == 63:
            _contract(a[active], c[active], f"paged decode {i} any4 vs dense twin")
    assert paged.page_pool.free_pages == 0 and paged._table == twin._table and paged.block_table.tolist() == paged._table
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
            for cache in (layer.k_cache, layer.v_cache):
                cache[dst, :, :t] = cache[src, :, :t]
        assert paged._table[dst][: t // PS] == paged._table[src][: t // PS] and paged._mapped(dst) == -(-t // PS)
        a, b = paged.decode(toks[:, t], position), flat.decode(toks[:, t], position)
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), t
    with pytest.raises(ValueError, match="share"):
        paged.decode(toks[:, 0], [-1, -1, 10, -1])


def test_paged_graph_replays_with_a_page_mapped_between_replays():
    """A captured paged step (max_seq 2048: the split launch, four blocks per head) replayed with three position vectors -- one with an
    inactive sequence, the last a device tensor that crosses a page edge, its page mapped by hand between two replays -- gives the eager
    contiguous ragged stack's logits in bits."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**dict(CFG, max_seq=2048))
    bs = 3
    eager = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=bs, seed=9, ragged=True)
    graph = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=bs, seed=9, ragged=True, kv_pages=8, page_size=64)
    assert graph._attn_split == 4 and graph._attn_scratch is not None
    graph.capture()  # (nothing is mapped yet: the warm-up steps write nothing)
    assert graph._graph is not None and not any(layer.k_pool.any() for layer in graph.layers)
    toks = torch.randint(0, cfg.vocab, (bs, 70), generator=torch.Generator().manual_seed(2)).to(DEV)
    lengths = [62, 9, 5]
    for layer in eager.layers:
        layer.k_cache.zero_()
        layer.v_cache.zero_()
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
            rows = torch.stack([lg.k_pool[graph._table[b][p // 64], :, p % 64] for p in range(n)], dim=1)
            assert torch.equal(rows, le.k_cache[b, :, :n]), b
