"""GPU suite: prompt prefill -- dg_prefill_attn (rope + KV-cache append + causal flash attention for a chunk of tokens) against the
plain-torch formulation of any4_amd/decode.py under the attention contract of tests/test_gpu_decode.py, and
DecodeStack.prefill / generate on the HIP linears against the dense twin and against token-by-token decode."""
import math

import pytest
import torch

from tests.test_gpu_decode import CFG, _PairedFactories

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_numerics")]
DEV = "cuda:0"
HEADS = [(4, 2, 64), (8, 2, 128), (4, 4, 128), (32, 8, 128)]
# (T, p0) with max_seq 1024; the last one ends exactly at max_seq
CASES = [(1, 0), (1, 5), (17, 0), (63, 1), (64, 0), (65, 17), (200, 0), (300, 257), (512, 0), (17, 1007), (24, 1000)]


def _ulp(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def _tables(d, max_seq):
    from any4_amd.decode import DecodeConfig, _rope_tables

    return _rope_tables(DecodeConfig(head_dim=d, max_seq=max_seq), DEV)


def _setup(gen, dtype, bs, hl, kvl, d, S, T, p0):
    """NaN-filled caches whose prefix [0, p0) holds standard-normal rows, and a standard-normal qkv chunk."""
    kc = torch.full((bs, kvl, S, d), float("nan"), device=DEV, dtype=dtype)
    vc = torch.full((bs, kvl, S, d), float("nan"), device=DEV, dtype=dtype)
    kc[:, :, :p0] = torch.randn(bs, kvl, p0, d, device=DEV, generator=gen).to(dtype)
    vc[:, :, :p0] = torch.randn(bs, kvl, p0, d, device=DEV, generator=gen).to(dtype)
    qkv = torch.randn(bs * T, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    return kc, vc, qkv


def _bound_ok(got, want, dtype):
    err, ref = (got.float() - want.float()).abs().max().item(), want.float().abs().max().item()
    return err <= 4 * _ulp(dtype) * ref, (err, 4 * _ulp(dtype) * ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("bs", [1, 3])
def test_prefill_attn_vs_torch(dtype, heads, bs):
    """Caches torch.equal to `_rope`'s rows, everything outside [p0, p0 + T) bit-untouched (NaN beyond the written prefix stays NaN,
    the output is finite), max|got - want| <= 4 ulp max|want| against the plain-torch formulation."""
    from any4_amd import decode_ops as G
    from any4_amd.decode import _rope, prefill_attention_torch

    hl, kvl, d = heads
    S, scale = 1024, 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(hl * 1000 + d + bs)
    for T, p0 in CASES:
        kc, vc, qkv = _setup(gen, dtype, bs, hl, kvl, d, S, T, p0)
        k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
        want = prefill_attention_torch(qkv, cos, sin, p0, k1, v1, hl, kvl, d, T)
        got = G.prefill_attn(qkv, cos, sin, torch.tensor([p0], device=DEV), k2, v2, hl, kvl, d, scale, T)
        # the rows written are _rope's bits (two rounded products, a rounded sum, one rounding to 16 bit)
        c, s_ = cos[p0:p0 + T].view(1, T, 1, d), sin[p0:p0 + T].view(1, T, 1, d)
        want_k = _rope(qkv[:, hl * d:(hl + kvl) * d].reshape(bs, T, kvl, d), c, s_).transpose(1, 2)
        want_v = qkv[:, (hl + kvl) * d:].reshape(bs, T, kvl, d).transpose(1, 2)
        assert torch.equal(k2[:, :, p0:p0 + T], want_k) and torch.equal(v2[:, :, p0:p0 + T], want_v), (T, p0)
        assert torch.equal(k2[:, :, :p0 + T], k1[:, :, :p0 + T]) and torch.equal(v2[:, :, :p0 + T], v1[:, :, :p0 + T]), (T, p0)
        assert torch.equal(k2[:, :, :p0], kc[:, :, :p0]) and torch.equal(v2[:, :, :p0], vc[:, :, :p0]), (T, p0)
        assert torch.isnan(k2[:, :, p0 + T:].float()).all() and torch.isnan(v2[:, :, p0 + T:].float()).all(), (T, p0)
        assert torch.isfinite(got.float()).all(), (T, p0)
        ok, figures = _bound_ok(got, want, dtype)
        print(f"prefill_attn {dtype} heads={heads} bs={bs} T={T} p0={p0}: err {figures[0]:.3e} bound {figures[1]:.3e}")
        assert ok, (T, p0, figures)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_prefill_attn_one_token_agrees_with_the_decode_kernel(dtype):
    from any4_amd import decode_ops as G

    bs, hl, kvl, d, S = 2, 8, 2, 128, 512
    scale = 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(7)
    for p in (0, 1, 63, 64, 300, 511):
        kc, vc, qkv = _setup(gen, dtype, bs, hl, kvl, d, S, 1, p)
        k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
        pos = torch.tensor([p], device=DEV)
        want = G.rope_attn_online(qkv, cos, sin, pos, k1, v1, hl, kvl, d, scale)
        got = G.prefill_attn(qkv, cos, sin, pos, k2, v2, hl, kvl, d, scale, 1)
        assert torch.equal(k1[:, :, :p + 1], k2[:, :, :p + 1]) and torch.equal(v1[:, :, :p + 1], v2[:, :, :p + 1]), p
        assert torch.isnan(k2[:, :, p + 1:].float()).all(), p
        ok, figures = _bound_ok(got, want, dtype)
        assert ok, (p, figures)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("p0", [0, 41])
def test_prefill_attn_chunk_invariance_and_determinism(dtype, p0):
    """One call of T = 300 vs calls of 100 + 200 and of 37 x 8 + 4: caches bit-equal, outputs within the bound of each other; the same
    call repeated gives the same bits."""
    from any4_amd import decode_ops as G

    bs, hl, kvl, d, S, T = 2, 8, 2, 128, 512, 300
    scale = 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(11)
    kc, vc, qkv = _setup(gen, dtype, bs, hl, kvl, d, S, T, p0)
    q3 = qkv.view(bs, T, -1)

    def run(pieces):
        k, v = kc.clone(), vc.clone()
        outs, t0 = [], 0
        for n in pieces:
            part = q3[:, t0:t0 + n].reshape(bs * n, -1).contiguous()
            o = G.prefill_attn(part, cos, sin, torch.tensor([p0 + t0], device=DEV), k, v, hl, kvl, d, scale, n)
            outs.append(o.view(bs, n, -1))
            t0 += n
        return torch.cat(outs, dim=1).reshape(bs * T, -1), k, v

    one, k1, v1 = run([T])
    again, k1b, v1b = run([T])
    assert torch.equal(one, again) and torch.equal(k1[:, :, :p0 + T], k1b[:, :, :p0 + T]) and torch.equal(v1[:, :, :p0 + T], v1b[:, :, :p0 + T])
    for pieces in ([100, 200], [37] * 8 + [4]):
        got, k2, v2 = run(pieces)
        assert torch.equal(k2[:, :, :p0 + T], k1[:, :, :p0 + T]) and torch.equal(v2[:, :, :p0 + T], v1[:, :, :p0 + T]), pieces
        assert torch.isnan(k2[:, :, p0 + T:].float()).all(), pieces
        ok, figures = _bound_ok(got, one, dtype)
        assert ok, (pieces, figures)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("heads", [(4, 2, 64), (8, 2, 128)])
def test_prefill_attn_out_of_range_positions(dtype, heads):
    """Defined behaviour, not a fault test: tokens whose position is outside [0, max_seq) write no cache row and leave their output
    row as it was; the in-range tokens of the same call are computed normally.  The caches are views into the front of larger
    buffers whose tails hold a pattern: nothing behind the caches is touched."""
    from any4_amd import decode_ops as G
    from any4_amd.decode import prefill_attention_torch

    hl, kvl, d = heads
    bs, S, T, guard = 2, 128, 40, 4096
    scale = 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(5)
    n = bs * kvl * S * d
    for p0, lo, hi in ((S - T + 3, 0, T - 3), (-2, 2, T), (S + 7, 0, 0), (-T, 0, 0)):  # tokens [lo, hi) are in range
        pfx = max(p0, 0)
        kc, vc, qkv = _setup(gen, dtype, bs, hl, kvl, d, S, T, min(pfx, S))
        kbuf = torch.full((n + guard,), 1.5, device=DEV, dtype=dtype)
        vbuf = torch.full((n + guard,), -2.5, device=DEV, dtype=dtype)
        k2, v2 = kbuf[:n].view(bs, kvl, S, d), vbuf[:n].view(bs, kvl, S, d)
        k2.copy_(kc)
        v2.copy_(vc)
        out = torch.full((bs * T, hl * d), 7.0, device=DEV, dtype=dtype)
        G.prefill_attn(qkv, cos, sin, torch.tensor([p0], device=DEV), k2, v2, hl, kvl, d, scale, T, out=out)
        assert (kbuf[n:] == 1.5).all() and (vbuf[n:] == -2.5).all(), p0
        o3 = out.view(bs, T, -1)
        assert (o3[:, :lo] == 7.0).all() and (o3[:, hi:] == 7.0).all(), p0
        if hi > lo:
            k1, v1 = kc.clone(), vc.clone()
            part = qkv.view(bs, T, -1)[:, lo:hi].reshape(bs * (hi - lo), -1).contiguous()
            want = prefill_attention_torch(part, cos, sin, p0 + lo, k1, v1, hl, kvl, d, hi - lo)
            end = p0 + hi
            assert torch.equal(k2[:, :, :end], k1[:, :, :end]) and torch.equal(v2[:, :, :end], v1[:, :, :end]), p0
            assert torch.isnan(k2[:, :, end:].float()).all(), p0
            ok, figures = _bound_ok(o3[:, lo:hi].reshape(bs * (hi - lo), -1), want, dtype)
            assert ok, (p0, figures)
        else:  # nothing in range: the caches are exactly as they were
            same = lambda a, b: torch.equal(a.view(torch.int16), b.view(torch.int16))
            assert same(k2, kc) and same(v2, vc), p0


def test_prefill_attn_graph_capture_replays_with_a_new_position():
    from any4_amd import decode_ops as G

    dtype, bs, hl, kvl, d, S, T = torch.bfloat16, 2, 8, 2, 128, 512, 70
    scale = 1.0 / math.sqrt(d)
    cos, sin = _tables(d, S)
    gen = torch.Generator(device=DEV).manual_seed(3)
    kc, vc, qkv = _setup(gen, dtype, bs, hl, kvl, d, S, T, 100)
    pos = torch.zeros(1, dtype=torch.long, device=DEV)
    ks, vs = kc.clone(), vc.clone()
    out = torch.zeros(bs * T, hl * d, device=DEV, dtype=dtype)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        G.prefill_attn(qkv, cos, sin, pos, ks, vs, hl, kvl, d, scale, T, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        G.prefill_attn(qkv, cos, sin, pos, ks, vs, hl, kvl, d, scale, T, out=out)
    for p in (0, 100):
        ks.copy_(kc)
        vs.copy_(vc)
        pos.fill_(p)
        g.replay()
        k1, v1 = kc.clone(), vc.clone()
        want = G.prefill_attn(qkv, cos, sin, torch.tensor([p], device=DEV), k1, v1, hl, kvl, d, scale, T)
        assert torch.equal(out, want), p
        assert torch.equal(ks[:, :, :p + T], k1[:, :, :p + T]) and torch.equal(vs[:, :, :p + T], v1[:, :, :p + T]), p


def _contract(a, b, what):
    a, b = a.float(), b.float()
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    print(f"{what}: err {err:.4e} allowed {0.03 * ref + 1e-3:.4e}")
    assert torch.isfinite(a).all() and err <= 0.03 * ref + 1e-3, (what, err, ref)


@pytest.mark.parametrize("max_seq,T", [(32, 6), (32, 24), (256, 200)])
def test_stack_prefill_any4_vs_dense_and_vs_token_by_token(oracle, max_seq, T):
    """any4 stack `prefill` (fused: HIP glue + dg_prefill_attn + the library's many-rows GEMM) vs the dense twin's plain-torch `prefill`,
    then 4 decode steps on both; and any4 prefill + decode vs the same any4 stack fed token by token.  Contract of
    tests/test_gpu_decode.py: max|a - b| <= 0.03 max|b| + 1e-3."""
    from any4_amd.decode import DecodeConfig, DecodeStack

    cfg = DecodeConfig(**{**CFG, "max_seq": max_seq})
    bs = 2
    fac = _PairedFactories(oracle, cfg, "linear_y_f16RM_x_f16RM_W_any4TC")
    q = DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, bs=bs, seed=5, fused=True)
    q1 = DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, bs=bs, seed=5, fused=True)
    dn = DecodeStack(cfg, fac.dense, DEV, torch.bfloat16, bs=bs, seed=5, fused=False)
    toks = torch.randint(0, cfg.vocab, (bs, T + 4), generator=torch.Generator().manual_seed(1)).to(DEV)
    a, b = q.prefill(toks[:, :T]), dn.prefill(toks[:, :T])
    for i in range(T):
        c = q1.decode(toks[:, i], i)
    assert a.shape == (bs, cfg.vocab)
    _contract(a, b, f"prefill T={T} any4 vs dense")
    _contract(a, c, f"prefill T={T} any4 vs token by token")
    for layer_a, layer_c in zip(q.layers, q1.layers):  # nothing beyond the prompt was written
        assert (layer_a.k_cache[:, :, T:] == 0).all() and (layer_a.v_cache[:, :, T:] == 0).all()
        assert layer_a.k_cache.shape == layer_c.k_cache.shape
    for i in range(T, T + 4):
        a, b, c = q.decode(toks[:, i], i), dn.decode(toks[:, i], i), q1.decode(toks[:, i], i)
        _contract(a, b, f"decode {i} after prefill, any4 vs dense")
        _contract(a, c, f"decode {i} after prefill vs token by token")


def test_captured_decode_survives_a_prefill():
    """capture(), prefill(), decode() replays == an uncaptured twin: prefill keeps its own position buffer and the caches it fills are
    the ones the captured graph reads."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**CFG)
    eager = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=2, seed=9)
    graph = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=2, seed=9)
    graph.capture()
    T = 9
    toks = torch.randint(0, cfg.vocab, (2, T + 5), generator=torch.Generator().manual_seed(2)).to(DEV)
    graph.pos.fill_(3)
    a, b = eager.prefill(toks[:, :T]), graph.prefill(toks[:, :T])
    assert int(graph.pos) == 3 and torch.equal(a, b)
    for i in range(T, T + 5):
        a, b = eager.decode(toks[:, i], i), graph.decode(toks[:, i], i).clone()
        assert torch.equal(a, b), i
    # generate() on the captured stack == the manual loop on the eager one
    got = graph.generate(toks[:, :T], 4)
    logits = eager.prefill(toks[:, :T])
    for i in range(4):
        tok = logits.argmax(-1)
        assert torch.equal(got[:, i], tok), i
        logits = eager.decode(tok, T + i) if T + i < cfg.max_seq else None


def test_prefill_llama3_8b_geometry_smoke():
    """Two layers of Llama-3-8B's geometry, T = 512, bs = 1: finite logits, caches written exactly on [0, 512)."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig.llama3_8b(layers=2, max_seq=1024, vocab=4096)
    stack = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=1), DEV, bs=1, seed=2)
    for layer in stack.layers:
        layer.k_cache.fill_(float("nan"))
        layer.v_cache.fill_(float("nan"))
    T = 512
    toks = torch.randint(0, cfg.vocab, (1, T), generator=torch.Generator().manual_seed(4)).to(DEV)
    logits = stack.prefill(toks)
    assert logits.shape == (1, cfg.vocab) and torch.isfinite(logits.float()).all()
    for layer in stack.layers:
        for cache in (layer.k_cache, layer.v_cache):
            assert torch.isfinite(cache[:, :, :T].float()).all() and torch.isnan(cache[:, :, T:].float()).all()
    nxt = stack.decode(logits.argmax(-1), T)
    assert torch.isfinite(nxt.float()).all()
