"""GPU suite: the one-barrier decode attention kernel on an mx8 KV cache -- the dg_rope_attn_online_mx8 / _mx8_seq flavours of dg_attn_launch, decode_ops.rope_attn_online_mx8,
DecodeStack(..., kv_cache="mx8", mx8_attention="online"):
  1. the bytes it writes are mx8_encode's (codes and exponents), nothing else is written, guard bytes behind all four tensors stay;
  2. its outputs equal the 16-bit one-barrier kernel's bit for bit on a 16-bit cache that holds the decoded values (identity rope tables,
     16-byte aligned, so that dg_rope_attn_online / dg_rope_attn_split run that kernel; a new token whose rows are decoded values);
  3. real rope tables: float64 attention over the DECODED cache under the contract of tests/test_gpu_kv8.py (_f64_check);
  4. a block with exponent byte 255 is never read above a sequence's prefix and makes exactly the affected outputs NaN inside it;
  5. a split launch repeated on one scratch buffer, nothing cleared in between, gives the same bits (the counters reset themselves);
  6. rejected calls return their code and touch nothing;
  7. the stack: fused against its plain-torch twin, ragged vs not, a captured split step replayed with new positions.
Positions are the edges of the 32- / 64-row iteration, of the 256-row chunk and of the cache; with nsplit = 8 short positions leave
blocks of a head without rows."""
import math

import pytest
import torch

from any4_amd.kvcache import F8
from tests import glue_ref as R
from tests.test_gpu_decode import CFG, _PairedFactories
from tests.test_gpu_kv8 import (CODE_FILL, DEV, DTYPES, EXP_FILL, GEOMETRIES, SENTINEL, TAILS, Cache8, S, _case8, _contract, _decoded_rows, _dev,
                                _f64_check, _put, _rope, _same, _split_k_v, _tables)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_numerics")]
POSITIONS = [0, 31, 32, 63, 64, 65, 255, 256, 257, S - 1]
NSPLITS = (1, 4, 8)


def _online8(G, qkv, cos, sin, pos, c, hl, kvl, d, scale, scr, ns, **kw):
    kc, vc, ke, ve = c.tensors
    return G.rope_attn_online_mx8(qkv, cos, sin, pos, kc, vc, ke, ve, hl, kvl, d, scale, scr, ns, **kw)


# ---------------------------------------------------------------- 1. bytes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_writes_the_encoders_bytes_and_nothing_else(dtype, geometry):
    """Real rope tables.  The scalar entry point at three positions (the last row of the cache among them) and the _seq one at every edge
    position with an inactive sequence and one outside the cache, nsplit 1, 4 and 8: the row written is mx8_encode(decode._rope(k)) /
    mx8_encode(v) byte for byte, every other byte keeps its sentinel, the guards behind all four tensors are intact, inactive sequences
    keep their output row."""
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    scale = 1.0 / math.sqrt(d)
    cos, sin = _tables(d)
    gen = torch.Generator(device=DEV).manual_seed(hl * 10 + kvl + d + 10)
    for ns in NSPLITS:
        for positions, per_sequence in (([0] * 2, False), ([257] * 2, False), ([S - 1] * 2, False), (POSITIONS + [-1, S], True)):
            bs = len(positions)
            scratch = G.rope_attn_split_scratch(bs, hl, d, ns, DEV)
            active = [0 <= p < S for p in positions]
            c = Cache8(gen, dtype, [p if a else 5 for p, a in zip(positions, active)], kvl, d)
            qkv = torch.randn(bs, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
            out = torch.full((bs, hl * d), SENTINEL, device=DEV, dtype=dtype)
            pos = _dev(positions) if per_sequence else _dev(positions[:1])
            _online8(G, qkv, cos, sin, pos, c, hl, kvl, d, scale, scratch, ns, per_sequence=per_sequence, out=out)
            _, k, v = _split_k_v(qkv, hl, kvl, d)
            kr = _rope(k, cos, sin, [p if a else 0 for p, a in zip(positions, active)])
            want = {n: t.clone() for n, t in c.initial.items()}
            for b, p in enumerate(positions):
                if active[b]:
                    _put(want, b, p, kr[b].unsqueeze(1), v[b].unsqueeze(1))
            what = (ns, positions, per_sequence)
            c.expect(want, what)
            for b in range(bs):
                assert torch.isfinite(out[b].float()).all() if active[b] else (out[b] == SENTINEL).all(), (what, b)
            assert not scratch[: bs * hl].any(), what  # the counters are back at zero


# ---------------------------------------------------------------- 2. the 16-bit one-barrier kernel's arithmetic, no tolerance
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_equals_the_16_bit_one_barrier_kernel_bit_for_bit(dtype, geometry):
    """nsplit = 1 against rope_attn_online(_seq), nsplit 4 / 8 against rope_attn_split(_seq) -- with aligned tables and head_dim 64 / 128
    the one-barrier kernel with that many blocks per head -- on a 16-bit cache holding mx8_decode of the same bytes; afterwards the two
    caches decode to the same values.  The per-sequence form carries an inactive sequence, whose output row nobody writes."""
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    scale = 1.0 / math.sqrt(d)
    cos, sin = _tables(d, identity=True)
    assert cos.data_ptr() % 16 == 0 and sin.data_ptr() % 16 == 0
    gen = torch.Generator(device=DEV).manual_seed(hl * 10 + kvl + d + 11)
    seq_positions = POSITIONS + [-1]
    bs = len(seq_positions)
    c0 = Cache8(gen, dtype, [p if p >= 0 else 5 for p in seq_positions], kvl, d)
    q = torch.randn(bs, hl * d, device=DEV, generator=gen).to(dtype)
    qkv = torch.cat([q, _decoded_rows(gen, dtype, bs, 2 * kvl * d // 32, 32).view(bs, -1)], dim=1).contiguous()
    assert qkv.data_ptr() % 16 == 0
    for ns in NSPLITS:
        scr = G.rope_attn_split_scratch(bs, hl, d, ns, DEV)
        for per_sequence in (True, False):
            for p in ([None] if per_sequence else POSITIONS):
                for name in TAILS:
                    getattr(c0, name).copy_(c0.initial[name])
                k16, v16 = c0.decoded(dtype)
                # (the scalar entry points put every sequence at p: rows of the slots whose prefix is shorter are the finite sentinel rows)
                pos = _dev(seq_positions) if per_sequence else _dev([p])
                got, want = (torch.full((bs, hl * d), SENTINEL, device=DEV, dtype=dtype) for _ in range(2))
                _online8(G, qkv, cos, sin, pos, c0, hl, kvl, d, scale, scr, ns, per_sequence=per_sequence, out=got)
                if ns == 1:
                    G.rope_attn_online(qkv, cos, sin, pos, k16, v16, hl, kvl, d, scale, per_sequence=per_sequence, out=want)
                else:
                    G.rope_attn_split(qkv, cos, sin, pos, k16, v16, hl, kvl, d, scale, scr, ns, per_sequence=per_sequence, out=want)
                what = (ns, per_sequence, p)
                assert torch.isfinite(want.float()).all(), what
                if per_sequence:
                    assert (want[-1] == SENTINEL).all() and not (want[:-1] == SENTINEL).all(dim=1).any(), what
                assert _same(got, want), (what, (got.float() - want.float()).abs().max().item())
                kd, vd = c0.decoded(dtype)
                assert _same(kd, k16) and _same(vd, v16), what  # and the caches hold the same values afterwards


# ---------------------------------------------------------------- 3. real rope tables: float64 over the decoded cache
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_real_rope_tables_vs_float64_on_the_decoded_cache(dtype, geometry):
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    bs = 2
    for kind, pos, ns in (("peaked", 257, 4), ("normal", S - 1, 1), ("peaked", 31, 4)):
        c, cache = _case8(kind, dtype, bs, geometry, 1, pos, R.case_seed(1, pos))
        scr = G.rope_attn_split_scratch(bs, hl, d, ns, DEV)
        out = _online8(G, c.qkv, c.cos, c.sin, _dev([pos]), cache, hl, kvl, d, c.scale, scr, ns)
        k16, v16 = cache.decoded(dtype)
        _f64_check(c, out, k16, v16, f"online {kind} pos {pos} nsplit {ns}")


# ---------------------------------------------------------------- 4. NaN isolation
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", [(4, 2, 64), (8, 8, 128)])
def test_a_nan_block_is_never_read_above_the_prefix_and_poisons_exactly_its_outputs_inside(dtype, geometry):
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    rep, scale, bs = hl // kvl, 1.0 / math.sqrt(d), 3
    cos, sin = _tables(d)
    gen = torch.Generator(device=DEV).manual_seed(hl + d + 12)
    positions = [100, 300, 200]
    c = Cache8(gen, dtype, positions, kvl, d)
    qkv = torch.randn(bs, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    blk = d // 32 - 1  # the block that is poisoned: the row's last

    def decode(ns, poison):
        for name in TAILS:
            getattr(c, name).copy_(c.initial[name])
        for name, b, kv, row in poison:
            getattr(c, name)[b, kv, row, blk] = 255
        scr = G.rope_attn_split_scratch(bs, hl, d, ns, DEV)
        return _online8(G, qkv, cos, sin, _dev(positions), c, hl, kvl, d, scale, scr, ns, per_sequence=True)

    for ns in NSPLITS:
        clean = decode(ns, [])
        assert torch.isfinite(clean.float()).all()
        # above every sequence's own position (their new rows sit at 100 / 300 / 200): the row behind it, and the last row of the cache --
        # rows the speculative requests and the clamped ones do read, and mask
        above = [(name, b, kv, row) for name in ("ke", "ve") for b in range(bs) for kv in range(kvl) for row in (positions[b] + 1, S - 1)]
        assert _same(decode(ns, above), clean), ns
        # inside: K of (sequence 1, kv head 0) at row 37 -> every output of that head group is NaN, nothing else changes
        got = decode(ns, [("ke", 1, 0, 37)]).view(bs, hl, d)
        nan = torch.zeros(bs, hl, d, dtype=torch.bool, device=DEV)
        nan[1, :rep] = True
        assert torch.equal(torch.isnan(got), nan) and _same(got[~nan], clean.view(bs, hl, d)[~nan]), ("k", ns)
        # ... and rows 64 ... 127 of it, all of them: at nsplit = 8 whole blocks of the head then have no finite score at all
        got = decode(ns, [("ke", 1, 0, row) for row in range(64, 128)]).view(bs, hl, d)
        assert torch.equal(torch.isnan(got), nan) and _same(got[~nan], clean.view(bs, hl, d)[~nan]), ("k rows", ns)
        # V of (sequence 2, last kv head) at row 199: the 32 columns of the block, in the heads of that group
        got = decode(ns, [("ve", 2, kvl - 1, 199)]).view(bs, hl, d)
        nan.zero_()
        nan[2, hl - rep:, blk * 32:] = True
        assert torch.equal(torch.isnan(got), nan) and _same(got[~nan], clean.view(bs, hl, d)[~nan]), ("v", ns)


# ---------------------------------------------------------------- 5. replay on one scratch buffer
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", [(4, 2, 64), (8, 8, 128)])
def test_a_split_launch_repeated_on_one_scratch_gives_the_same_bits(dtype, geometry):
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    scale, ns = 1.0 / math.sqrt(d), 4
    cos, sin = _tables(d)
    gen = torch.Generator(device=DEV).manual_seed(hl + d + 13)
    positions = [257, 31, -1, S - 1]
    bs = len(positions)
    c = Cache8(gen, dtype, [max(p, 0) for p in positions], kvl, d)
    qkv = torch.randn(bs, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    scr = G.rope_attn_split_scratch(bs, hl, d, ns, DEV)
    outs = [torch.full((bs, hl * d), SENTINEL, device=DEV, dtype=dtype) for _ in range(2)]
    for out in outs:  # (the second launch re-encodes the same row over itself; nothing is cleared in between)
        _online8(G, qkv, cos, sin, _dev(positions), c, hl, kvl, d, scale, scr, ns, per_sequence=True, out=out)
    assert torch.isfinite(outs[0][[0, 1, 3]].float()).all() and (outs[0][2] == SENTINEL).all()
    assert _same(outs[0], outs[1])
    assert not scr[: bs * hl].any()


# ---------------------------------------------------------------- 6. rejected calls
@pytest.mark.parametrize("dtype", DTYPES)
def test_rejected_calls_return_their_code_and_touch_nothing(dtype):
    """head_dim 96 and nsplit 65 (TG_E_SHAPE), exponent tensors 4 bytes off a 16-byte boundary (TG_E_ALIGN); raw calls of both flavours."""
    from any4_amd import _lib
    from any4_amd import decode_ops as G
    from tests import attn_abi

    lib = _lib.load()
    TG_E_SHAPE, TG_E_ALIGN = -7, -8
    hl, kvl, bs = 4, 2, 2
    dt = _lib.TG_BF16 if dtype == torch.bfloat16 else _lib.TG_F16
    for entry in ("dg_rope_attn_online_mx8", "dg_rope_attn_online_mx8_seq"):
        for d, ns, off, code in ((96, 2, 0, TG_E_SHAPE), (64, 65, 0, TG_E_SHAPE), (64, 2, 4, TG_E_ALIGN), (128, 2, 4, TG_E_ALIGN)):
            nb = d // 32
            qkv = torch.ones(bs, (hl + 2 * kvl) * d, device=DEV, dtype=dtype)
            cos, sin = torch.ones(S, d, device=DEV), torch.zeros(S, d, device=DEV)
            pos = _dev([3] * bs)
            kc, vc = (torch.full((bs, kvl, S, d), CODE_FILL, dtype=torch.uint8, device=DEV) for _ in range(2))
            ebuf = [torch.full((bs * kvl * S * nb + 16,), EXP_FILL, dtype=torch.uint8, device=DEV) for _ in range(2)]
            ke, ve = (b[off: off + bs * kvl * S * nb].view(bs, kvl, S, nb) for b in ebuf)
            assert ke.data_ptr() % 16 == off and ve.data_ptr() % 16 == off
            out = torch.full((bs, hl * d), SENTINEL, device=DEV, dtype=dtype)
            scr = G.rope_attn_split_scratch(bs, hl, 128, 64, DEV)
            st = torch.cuda.current_stream().cuda_stream
            rc = attn_abi.launch(lib, entry, 0, st, qkv=qkv.data_ptr(), cos=cos.data_ptr(), sin=sin.data_ptr(), pos=pos.data_ptr(),
                                 k_cache=kc.data_ptr(), v_cache=vc.data_ptr(), k_exp=ke.data_ptr(), v_exp=ve.data_ptr(), out=out.data_ptr(),
                                 scratch=scr.data_ptr(), scratch_bytes=scr.numel() * 4, bs=bs, hl=hl, kvl=kvl, d=d, max_seq=S, scale=0.125,
                                 nsplit=ns, dtype=dt)
            torch.cuda.synchronize()
            assert rc == code, (entry, d, ns, off, rc)
            assert (kc == CODE_FILL).all() and (vc == CODE_FILL).all() and all((b == EXP_FILL).all() for b in ebuf), (entry, d, ns, off)
            assert (out == SENTINEL).all() and not scr.any(), (entry, d, ns, off)


# ---------------------------------------------------------------- 7. the stack
@pytest.mark.parametrize("fuse_gemm_stages", [True, False])
@pytest.mark.parametrize("ragged", [False, True])
def test_online_stack_fused_vs_its_plain_torch_twin(oracle, fuse_gemm_stages, ragged):
    """Five and eight launches, ragged and not: prefill + four decode steps of the fused any4 mx8 stack with mx8_attention="online"
    against the dense twin's plain-torch mx8 path, under the contract of tests/test_gpu_kv8.py."""
    from any4_amd.decode import DecodeConfig, DecodeStack

    cfg = DecodeConfig(**CFG)
    bs, steps = 3, 4
    lengths = [6, 24, 1] if ragged else [6, 6, 6]
    fac = _PairedFactories(oracle, cfg, "linear_y_f16RM_x_f16RM_W_any4TC")
    kw8 = dict(kv_cache="mx8", mx8_attention="online")
    q = DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, bs=bs, seed=5, fused=True, fuse_gemm_stages=fuse_gemm_stages, ragged=ragged, **kw8)
    dn = DecodeStack(cfg, fac.dense, DEV, torch.bfloat16, bs=bs, seed=5, fused=False, ragged=ragged, **kw8)
    assert q._attn_scratch is not None and q._attn_split >= 1 and q._five_launch() == fuse_gemm_stages
    assert all(layer.mx8_attention == "online" for layer in q.layers)
    T = max(lengths)
    toks = torch.randint(0, cfg.vocab, (bs, T + steps), generator=torch.Generator().manual_seed(1)).to(DEV)
    kw = dict(lengths=lengths) if ragged else {}
    _contract(q.prefill(toks[:, :T], **kw), dn.prefill(toks[:, :T], **kw), "online prefill")
    for i in range(steps):
        position = [n + i for n in lengths] if ragged else T + i
        _contract(q.decode(toks[:, T + i], position), dn.decode(toks[:, T + i], position), f"online decode {i}")
    for stack in (q, dn):
        for layer in stack.layers:
            tensors = (layer.k_cache, layer.v_cache, layer.k_exp, layer.v_exp)
            assert all(t.element_size() == 1 for t in tensors) and layer.k_cache.dtype == F8 and layer.k_exp.dtype == torch.uint8
            for s, n in enumerate(lengths):
                for t in tensors:
                    assert not t.view(torch.uint8)[s, :, n + steps:].any() and t.view(torch.uint8)[s, :, n + steps - 1].any()


def test_online_ragged_stack_at_equal_positions_is_the_non_ragged_stack(monkeypatch):
    """... in logits and in cache bytes; and every decode step's attention launch is rope_attn_online_mx8 (none the split entry point)."""
    from any4_amd import decode_ops as G
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    calls = {"online": 0, "split": 0}
    online, split = G.rope_attn_online_mx8, G.rope_attn_split
    monkeypatch.setattr(G, "rope_attn_online_mx8", lambda *a, **k: (calls.__setitem__("online", calls["online"] + 1), online(*a, **k))[1])
    monkeypatch.setattr(G, "rope_attn_split", lambda *a, **k: (calls.__setitem__("split", calls["split"] + 1), split(*a, **k))[1])
    cfg = DecodeConfig(**CFG)
    bs, T = 3, 6
    mk = lambda **kw: DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=bs, seed=9, kv_cache="mx8", mx8_attention="online", **kw)  # noqa: E731
    r, p = mk(ragged=True), mk()
    toks = torch.randint(0, cfg.vocab, (bs, T + 2), generator=torch.Generator().manual_seed(2)).to(DEV)
    assert torch.equal(r.prefill(toks[:, :T], position=[0] * bs, lengths=[T] * bs), p.prefill(toks[:, :T]))
    for i in range(2):
        a, b = r.decode(toks[:, T + i], [T + i] * bs), p.decode(toks[:, T + i], T + i)
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), i
    assert calls == {"online": 2 * 2 * cfg.layers, "split": 0}
    for lr, lp in zip(r.layers, p.layers):
        for name in ("k_cache", "v_cache", "k_exp", "v_exp"):
            assert torch.equal(getattr(lr, name).view(torch.uint8), getattr(lp, name).view(torch.uint8)), name
            assert getattr(lr, name).view(torch.uint8)[:, :, T + 1].any() and not getattr(lr, name).view(torch.uint8)[:, :, T + 2:].any(), name


def test_online_graph_at_max_seq_2048_replays_with_new_positions():
    """max_seq 2048: the stack splits every head four ways, so the captured launch is the split one (partials, counters, the combine).  A
    captured ragged step replayed with three position vectors (one with an inactive sequence) == the eager step, in bits."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**dict(CFG, max_seq=2048))
    bs = 3
    mk = lambda: DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=bs, seed=9, ragged=True, kv_cache="mx8", mx8_attention="online")  # noqa: E731
    eager, graph = mk(), mk()
    assert eager._attn_split == 4 and graph._attn_scratch is not None
    graph.capture()
    assert graph._graph is not None
    lengths = [2, 300, 70]
    toks = torch.randint(0, cfg.vocab, (bs, 303), generator=torch.Generator().manual_seed(2)).to(DEV)
    names = ("k_cache", "v_cache", "k_exp", "v_exp")
    for stack in (eager, graph):
        for layer in stack.layers:  # (capture's warm-up steps wrote position 0)
            for name in names:
                getattr(layer, name).view(torch.uint8).zero_()
        stack.prefill(toks[:, :300], lengths=lengths)
    for i, position in enumerate(([2, 300, 70], [3, -1, 71], _dev([4, 301, 72]))):
        a, b = eager.decode(toks[:, 300 + i], position), graph.decode(toks[:, 300 + i], position).clone()
        rows = [s for s in range(bs) if i != 1 or s != 1]
        assert torch.isfinite(a[rows].float()).all() and torch.equal(a[rows], b[rows]), i
        for le, lg in zip(eager.layers, graph.layers):
            for name in names:
                assert torch.equal(getattr(le, name).view(torch.uint8), getattr(lg, name).view(torch.uint8)), (i, name)
            if i == 1:  # the inactive sequence wrote nothing
                assert lg.k_exp[1, :, 300].any() and not lg.k_exp[1, :, 301:].any() and not lg.v_cache.view(torch.uint8)[1, :, 301:].any()
