"""GPU suite: a position per sequence -- dg_rope_attn_seq / dg_rope_attn_online_seq / dg_rope_attn_split_seq and dg_prefill_attn_seq bit
for bit against their scalar namesakes run on one sequence at a time, dg_prefill_attn_seq against the plain-torch formulation under
the bound of tests/test_gpu_prefill.py, and DecodeStack(..., ragged=True) on the HIP linears against the dense twin's plain-torch
ragged path, against the non-ragged stack at equal positions, and through a captured graph."""
import math

import numpy as np
import pytest
import torch

from tests.conftest import bits16
from tests.test_gpu_decode import CFG, _PairedFactories

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_numerics")]
DEV = "cuda:0"
SENTINEL = 7.0


def _ulp(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def _tables(d, max_seq):
    from any4_amd.decode import DecodeConfig, _rope_tables

    return _rope_tables(DecodeConfig(head_dim=d, max_seq=max_seq), DEV)


def _same(a, b):
    """Bit for bit (NaN == NaN)."""
    return np.array_equal(bits16(a), bits16(b))


def _caches(gen, dtype, prefixes, kvl, S, d):
    """[len(prefixes)][kvl][S][d] x 2, NaN above a standard-normal prefix per slot."""
    n = len(prefixes)
    kc = torch.full((n, kvl, S, d), float("nan"), device=DEV, dtype=dtype)
    vc = torch.full((n, kvl, S, d), float("nan"), device=DEV, dtype=dtype)
    for b, p in enumerate(prefixes):
        kc[b, :, :p] = torch.randn(kvl, p, d, device=DEV, generator=gen).to(dtype)
        vc[b, :, :p] = torch.randn(kvl, p, d, device=DEV, generator=gen).to(dtype)
    return kc, vc


def _dev(vals):
    return torch.tensor(vals, dtype=torch.long, device=DEV)


# ---------------------------------------------------------------- decode step: one new token per sequence
GEOMETRIES = [(4, 2, 64), (16, 8, 128), (6, 2, 32)]  # (16, 8, 128): the online kernel's head remap; d = 32: the general kernels only
POSITIONS = [[0, 31, 32, 700], [255, 256, 257, 1023], [5, -1, 1024, 64]]  # 32- / 64-row iterations, 256-row chunks; two inactive


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_decode_seq_kernels_equal_the_scalar_kernels_per_sequence(dtype, geometry):
    """For every active sequence the output row and both caches are, in bits, what the scalar namesake gives for that sequence alone
    (bs = 1 on slices of identical initial state); an inactive sequence keeps its sentinel row and its caches."""
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    bs, S, ns, scale = 4, 1024, 4, 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(hl * 100 + d)
    scr4, scr1 = G.rope_attn_split_scratch(bs, hl, d, ns, DEV), G.rope_attn_split_scratch(1, hl, d, ns, DEV)
    entries = {"rope_attn": (G.rope_attn, (), ()), "rope_attn_split": (G.rope_attn_split, (scr4, ns), (scr1, ns))}
    if d in (64, 128):
        entries["rope_attn_online"] = (G.rope_attn_online, (), ())
    for name, (fn, more4, more1) in entries.items():
        for positions in POSITIONS:
            active = [0 <= p < S for p in positions]
            kc, vc = _caches(gen, dtype, [p if a else 9 for p, a in zip(positions, active)], kvl, S, d)
            qkv = torch.randn(bs, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
            k2, v2 = kc.clone(), vc.clone()
            out = torch.full((bs, hl * d), SENTINEL, device=DEV, dtype=dtype)
            fn(qkv, cos, sin, _dev(positions), k2, v2, hl, kvl, d, scale, *more4, per_sequence=True, out=out)
            for b, p in enumerate(positions):
                what = (name, positions, b)
                if not active[b]:
                    assert (out[b] == SENTINEL).all() and _same(k2[b], kc[b]) and _same(v2[b], vc[b]), what
                    continue
                k1, v1 = kc[b: b + 1].clone(), vc[b: b + 1].clone()
                want = fn(qkv[b: b + 1].contiguous(), cos, sin, _dev([p]), k1, v1, hl, kvl, d, scale, *more1)
                assert torch.isfinite(want.float()).all(), what
                assert _same(out[b], want[0]), what
                assert _same(k2[b], k1[0]) and _same(v2[b], v1[0]), what
    with pytest.raises(RuntimeError, match="per_sequence"):
        G.rope_attn(qkv, cos, sin, _dev([3]), k2, v2, hl, kvl, d, scale, per_sequence=True)


# ---------------------------------------------------------------- prefill chunk
PREFILL_GEOMETRIES = [(4, 4, 128), (8, 2, 128), (4, 2, 64)]  # T = 130: two query blocks at hl / kvl = 1, five at hl / kvl = 4


def _prefill_case(dtype, geometry, seed):
    hl, kvl, d = geometry
    n, cache_bs, S, T = 3, 4, 512, 130
    gen = torch.Generator(device=DEV).manual_seed(seed + hl + d)
    cos, sin = _tables(d, S)
    qkv = torch.randn(n * T, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    return hl, kvl, d, n, cache_bs, S, T, gen, cos, sin, qkv, 1.0 / math.sqrt(d)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("geometry", PREFILL_GEOMETRIES)
def test_prefill_seq_equals_the_scalar_kernel_per_sequence_and_torch(dtype, geometry):
    """len = [130, 1, 65], pos = [0, 41, 257], slot = [2, 0, 3] of 4: rows t < len_i and the written cache rows are dg_prefill_attn's bits
    for that sequence alone (T = len_i, p0 = pos_i, its slot's slice); rows t >= len_i keep the sentinel; slot 1 and every cache
    row outside [pos_i, pos_i + len_i) are bit-unchanged.  And per sequence max|got - want| <= 4 ulp max|want| against
    prefill_attention_torch at T = len_i (a reference that does not rest on the project's kernels)."""
    from any4_amd import decode_ops as G
    from any4_amd.decode import prefill_attention_torch

    hl, kvl, d, n, cache_bs, S, T, gen, cos, sin, qkv, scale = _prefill_case(dtype, geometry, 1)
    lens, pos, slot = [130, 1, 65], [0, 41, 257], [2, 0, 3]
    prefix = [20] * cache_bs
    for i in range(n):
        prefix[slot[i]] = pos[i]
    kc, vc = _caches(gen, dtype, prefix, kvl, S, d)
    k2, v2 = kc.clone(), vc.clone()
    out = torch.full((n * T, hl * d), SENTINEL, device=DEV, dtype=dtype)
    got = G.prefill_attn(qkv, cos, sin, _dev(pos), k2, v2, hl, kvl, d, scale, T, out=out, lengths=_dev(lens), slots=_dev(slot))
    assert got is out
    o3, q3 = out.view(n, T, -1), qkv.view(n, T, -1)
    assert _same(k2[1], kc[1]) and _same(v2[1], vc[1])
    for i in range(n):
        L, p0, sl = lens[i], pos[i], slot[i]
        part = q3[i, :L].contiguous()
        k1, v1 = kc[sl: sl + 1].clone(), vc[sl: sl + 1].clone()
        want = G.prefill_attn(part, cos, sin, _dev([p0]), k1, v1, hl, kvl, d, scale, L)
        assert torch.isfinite(want.float()).all(), i
        assert _same(o3[i, :L], want), i
        assert (o3[i, L:] == SENTINEL).all(), i
        assert _same(k2[sl], k1[0]) and _same(v2[sl], v1[0]), i
        for cache, init in ((k2, kc), (v2, vc)):
            assert _same(cache[sl, :, :p0], init[sl, :, :p0]) and _same(cache[sl, :, p0 + L:], init[sl, :, p0 + L:]), i
            assert torch.isfinite(cache[sl, :, p0: p0 + L].float()).all(), i
        kt, vt = kc[sl: sl + 1].clone(), vc[sl: sl + 1].clone()
        ref = prefill_attention_torch(part, cos, sin, p0, kt, vt, hl, kvl, d, L)
        err, top = (o3[i, :L].float() - ref.float()).abs().max().item(), ref.float().abs().max().item()
        print(f"prefill_attn_seq {dtype} {geometry} sequence {i}: err {err:.3e} bound {4 * _ulp(dtype) * top:.3e}")
        assert err <= 4 * _ulp(dtype) * top, (i, err, 4 * _ulp(dtype) * top)
        assert torch.equal(k2[sl, :, p0: p0 + L], kt[0, :, p0: p0 + L]) and torch.equal(v2[sl, :, p0: p0 + L], vt[0, :, p0: p0 + L]), i


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("geometry", PREFILL_GEOMETRIES)
def test_prefill_seq_no_op_sequences_and_the_end_of_the_cache(dtype, geometry):
    """Defined behaviour, not a fault test: len = [0, 130, 7], slot = [-1, 4, 1] of 4, pos[2] = max_seq - 3.  A length of 0 and a slot
    outside the caches make a sequence a no-op; of sequence 2 only the three tokens inside the cache have any effect.  The caches
    are views into the front of larger buffers whose tails hold a pattern: nothing behind them is touched."""
    from any4_amd import decode_ops as G

    hl, kvl, d, n, cache_bs, S, T, gen, cos, sin, qkv, scale = _prefill_case(dtype, geometry, 2)
    lens, pos, slot, inside, guard = [0, 130, 7], [0, 10, S - 3], [-1, 4, 1], 3, 4096
    kc, vc = _caches(gen, dtype, [20, S - 3, 20, 20], kvl, S, d)
    numel = kc.numel()
    kbuf = torch.full((numel + guard,), 1.5, device=DEV, dtype=dtype)
    vbuf = torch.full((numel + guard,), -2.5, device=DEV, dtype=dtype)
    k2, v2 = kbuf[:numel].view_as(kc), vbuf[:numel].view_as(vc)
    k2.copy_(kc)
    v2.copy_(vc)
    out = torch.full((n * T, hl * d), SENTINEL, device=DEV, dtype=dtype)
    G.prefill_attn(qkv, cos, sin, _dev(pos), k2, v2, hl, kvl, d, scale, T, out=out, lengths=_dev(lens), slots=_dev(slot))
    assert (kbuf[numel:] == 1.5).all() and (vbuf[numel:] == -2.5).all()
    o3 = out.view(n, T, -1)
    assert (o3[:2] == SENTINEL).all() and (o3[2, inside:] == SENTINEL).all()
    for sl in (0, 2, 3):
        assert _same(k2[sl], kc[sl]) and _same(v2[sl], vc[sl]), sl
    k1, v1 = kc[1:2].clone(), vc[1:2].clone()
    want = G.prefill_attn(qkv.view(n, T, -1)[2, :inside].contiguous(), cos, sin, _dev([pos[2]]), k1, v1, hl, kvl, d, scale, inside)
    assert torch.isfinite(want.float()).all()
    assert _same(o3[2, :inside], want) and _same(k2[1], k1[0]) and _same(v2[1], v1[0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("geometry", PREFILL_GEOMETRIES)
def test_prefill_seq_without_lengths_and_slots_is_the_scalar_kernel(dtype, geometry):
    from any4_amd import decode_ops as G

    hl, kvl, d, _, n, S, T, gen, cos, sin, _, scale = _prefill_case(dtype, geometry, 3)
    p0 = 41
    qkv = torch.randn(n * T, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    kc, vc = _caches(gen, dtype, [p0] * n, kvl, S, d)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    want = G.prefill_attn(qkv, cos, sin, _dev([p0]), k1, v1, hl, kvl, d, scale, T)
    got = G.prefill_attn(qkv, cos, sin, _dev([p0] * n), k2, v2, hl, kvl, d, scale, T, per_sequence=True)
    assert torch.isfinite(want.float()).all() and _same(got, want) and _same(k2, k1) and _same(v2, v1)


# ---------------------------------------------------------------- the stack
def _contract(a, b, what):
    a, b = a.float(), b.float()
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    print(f"{what}: err {err:.4e} allowed {0.03 * ref + 1e-3:.4e}")
    assert torch.isfinite(a).all() and err <= 0.03 * ref + 1e-3, (what, err, ref)


@pytest.mark.parametrize("fuse_gemm_stages", [True, False])
def test_ragged_stack_any4_vs_dense_and_vs_the_non_ragged_stack(oracle, fuse_gemm_stages):
    """bs = 3, lengths [6, 24, 1]: ragged prefill + four decode steps of the fused any4 stack vs the dense twin's plain-torch ragged path
    (contract of tests/test_gpu_decode.py: max|a - b| <= 0.03 max|b| + 1e-3); nothing beyond a sequence's own rows is written; and
    at equal positions the ragged fused stack gives the non-ragged fused stack's logits in bits."""
    from any4_amd.decode import DecodeConfig, DecodeStack

    cfg = DecodeConfig(**CFG)
    bs, lengths, steps = 3, [6, 24, 1], 4
    fac = _PairedFactories(oracle, cfg, "linear_y_f16RM_x_f16RM_W_any4TC")
    kw = dict(bs=bs, seed=5, fused=True, fuse_gemm_stages=fuse_gemm_stages)
    q = DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, ragged=True, **kw)
    dn = DecodeStack(cfg, fac.dense, DEV, torch.bfloat16, bs=bs, seed=5, fused=False, ragged=True)
    T = max(lengths)
    toks = torch.randint(0, cfg.vocab, (bs, T + steps), generator=torch.Generator().manual_seed(1)).to(DEV)
    a, b = q.prefill(toks[:, :T], lengths=lengths), dn.prefill(toks[:, :T], lengths=lengths)
    assert a.shape == (bs, cfg.vocab)
    _contract(a, b, "ragged prefill any4 vs dense")
    for i in range(steps):
        position = [n + i for n in lengths]
        a, b = q.decode(toks[:, T + i], position), dn.decode(toks[:, T + i], _dev(position))
        _contract(a, b, f"ragged decode {i} any4 vs dense")
    for stack in (q, dn):
        for layer in stack.layers:
            for s, n in enumerate(lengths):
                assert (layer.k_cache[s, :, n + steps:] == 0).all() and (layer.v_cache[s, :, n + steps:] == 0).all()
                assert layer.k_cache[s, :, n + steps - 1].any()
    # equal positions: the bits of the non-ragged stack
    r, p = DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, ragged=True, **kw), DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, **kw)
    T = 6
    assert torch.equal(r.prefill(toks[:, :T], position=[0] * bs, lengths=[T] * bs), p.prefill(toks[:, :T]))
    for i in range(2):
        assert torch.equal(r.decode(toks[:, T + i], [T + i] * bs), p.decode(toks[:, T + i], T + i)), i
    for lr, lp in zip(r.layers, p.layers):
        assert torch.equal(lr.k_cache, lp.k_cache) and torch.equal(lr.v_cache, lp.v_cache)


def test_ragged_graph_replays_with_new_positions():
    """A captured ragged step replayed with three position vectors (one with an inactive sequence) == the eager step, in bits."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**CFG)
    bs = 3
    eager = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=bs, seed=9, ragged=True)
    graph = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=bs, seed=9, ragged=True)
    graph.capture()
    assert graph._graph is not None
    toks = torch.randint(0, cfg.vocab, (bs, 12), generator=torch.Generator().manual_seed(2)).to(DEV)
    lengths = [2, 9, 5]
    for stack in (eager, graph):
        for layer in stack.layers:  # (capture's warm-up steps wrote position 0)
            layer.k_cache.zero_()
            layer.v_cache.zero_()
        stack.prefill(toks[:, :9], lengths=lengths)
    for i, position in enumerate(([2, 9, 5], [3, -1, 6], _dev([4, 10, 7]))):
        a, b = eager.decode(toks[:, 9 + i], position), graph.decode(toks[:, 9 + i], position).clone()
        rows = [s for s in range(bs) if i != 1 or s != 1]
        assert torch.isfinite(a[rows].float()).all() and torch.equal(a[rows], b[rows]), i
        for le, lg in zip(eager.layers, graph.layers):
            assert torch.equal(le.k_cache, lg.k_cache) and torch.equal(le.v_cache, lg.v_cache), i
            if i == 1:  # the inactive sequence wrote nothing: its last row is still the one of the step before
                assert lg.k_cache[1, :, 9].any() and not lg.k_cache[1, :, 10:].any() and not lg.v_cache[1, :, 10:].any()
