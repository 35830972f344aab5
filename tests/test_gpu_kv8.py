"""GPU suite: the mx8 KV cache (any4_amd/kvcache.py) on the HIP kernels -- the dg_rope_attn_split_mx8 / _mx8_seq and dg_prefill_attn_mx8 / _mx8_seq flavours of dg_attn_launch:
  1. the bytes they write are mx8_encode's (codes and exponents), nothing else is written, guard bytes behind all four tensors stay;
  2. their outputs equal their 16-bit namesakes' bit for bit on a 16-bit cache that holds the decoded values (identity rope tables and a
     new token whose rows are decoded values themselves, so re-quantising changes nothing).  At head_dim 64 / 128 dg_rope_attn_split
     would take the one-barrier kernel, whose arithmetic is another; it is handed rope tables that are 4 bytes off a 16-byte boundary,
     for which the ABI runs the 256-thread split kernel -- the one the mx8 entry points always run;
  3. real rope tables: float64 attention over the DECODED cache under the contract of tests/test_gpu_glue_f64.py
     (2 max(e of the 16-bit torch formulation, 2 u));
  4. a block with exponent byte 255 is never read above a sequence's prefix and makes exactly the affected outputs NaN inside it;
  5. DecodeStack(..., kv_cache="mx8") fused against its plain-torch twin (max|a - b| <= 0.03 max|b| + 1e-3), ragged vs not, a captured
     step, and the cache's bytes;
  6. rejected shapes return TG_E_SHAPE and touch nothing."""
import math

import pytest
import torch

from any4_amd.kvcache import F8, mx8_decode, mx8_encode
from tests import glue_ref as R
from tests.test_gpu_decode import CFG, _PairedFactories

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_numerics")]
DEV = "cuda:0"
SENTINEL = 7.0
GEOMETRIES = [(4, 1, 64), (4, 2, 64), (8, 8, 64), (4, 1, 128), (4, 2, 128), (8, 8, 128)]
DTYPES = [torch.bfloat16, torch.float16]
S = 512
POSITIONS = [0, 31, 32, 255, 256, 257, S - 1]
CODE_FILL, EXP_FILL, GUARD = 0x5A, 0x7B, 4096  # unwritten rows: code 20.0 times 2^-4, finite in both types
TAILS = {"kc": 0xA1, "ke": 0xB2, "vc": 0xC3, "ve": 0xD4}


def _dev(vals):
    return torch.tensor(vals, dtype=torch.long, device=DEV)


def _tables(d, identity=False, misaligned=False):
    """float32 [S, d] rope tables on the device; misaligned: the same values 4 bytes behind a 16-byte boundary."""
    cos, sin = R.rope_tables(d, S, DEV, identity=identity)
    if misaligned:
        out = []
        for t in (cos, sin):
            buf = torch.empty(t.numel() + 4, device=DEV)
            v = buf[1: 1 + t.numel()].view_as(t)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4 and v.is_contiguous()
            out.append(v)
        cos, sin = out
    return cos, sin


class Cache8:
    """An mx8 cache [n][kvl][S][d] at the front of four larger byte buffers whose tails hold a pattern.  Slot b holds encoded
    standard-normal rows in [0, prefixes[b]) and a sentinel in every byte above."""

    def __init__(self, gen, dtype, prefixes, kvl, d):
        n = len(prefixes)
        self.buf, self.numel = {}, {}
        for name, width, fill in (("kc", d, CODE_FILL), ("ke", d // 32, EXP_FILL), ("vc", d, CODE_FILL), ("ve", d // 32, EXP_FILL)):
            numel = n * kvl * S * width
            buf = torch.full((numel + GUARD,), TAILS[name], dtype=torch.uint8, device=DEV)
            buf[:numel] = fill
            self.buf[name], self.numel[name] = buf, numel
            setattr(self, name, buf[:numel].view(n, kvl, S, width))
        for b, p in enumerate(prefixes):
            for c, e in ((self.kc, self.ke), (self.vc, self.ve)):
                codes, exps = mx8_encode(torch.randn(kvl, p, d, device=DEV, generator=gen).to(dtype))
                c[b, :, :p], e[b, :, :p] = codes.view(torch.uint8), exps
        self.initial = {name: getattr(self, name).clone() for name in TAILS}

    @property
    def tensors(self):
        """(k_cache, v_cache, k_exp, v_exp) as the entry points take them"""
        return self.kc.view(F8), self.vc.view(F8), self.ke, self.ve

    def decoded(self, dtype):
        return mx8_decode(self.kc.view(F8), self.ke, dtype), mx8_decode(self.vc.view(F8), self.ve, dtype)

    def guards_intact(self):
        return all((self.buf[name][self.numel[name]:] == TAILS[name]).all() for name in TAILS)

    def expect(self, want, what):
        """Every byte of the four tensors equals `want` (a dict like self.initial), and the guards are intact."""
        for name in TAILS:
            got = getattr(self, name)
            if not torch.equal(got, want[name]):
                bad = (got != want[name]).nonzero()
                pytest.fail(f"{what}: {name} differs in {bad.shape[0]} bytes, first at {bad[0].tolist()}: got {int(got[tuple(bad[0])])}, "
                            f"want {int(want[name][tuple(bad[0])])}")
        assert self.guards_intact(), what


def _put(want, b, p, k16, v16):
    """rows k16 / v16 [kvl, T, d] of slot b at positions p ... in the expected bytes"""
    T = k16.shape[1]
    for c, e, x in (("kc", "ke", k16), ("vc", "ve", v16)):
        codes, exps = mx8_encode(x)
        want[c][b, :, p: p + T], want[e][b, :, p: p + T] = codes.view(torch.uint8), exps
    return want


def _split_k_v(qkv, hl, kvl, d):
    """qkv [rows, (hl + 2 kvl) d] -> q [rows, hl, d], k, v [rows, kvl, d]"""
    rows = qkv.shape[0]
    return (qkv[:, : hl * d].reshape(rows, hl, d), qkv[:, hl * d: (hl + kvl) * d].reshape(rows, kvl, d),
            qkv[:, (hl + kvl) * d:].reshape(rows, kvl, d))


def _rope(x, cos, sin, positions):
    """x [rows, heads, d] at `positions` [rows] -> decode._rope's bits"""
    from any4_amd.decode import _rope as rope

    idx = torch.as_tensor(positions, device=x.device)
    return rope(x, cos[idx].unsqueeze(1), sin[idx].unsqueeze(1))


def _decoded_rows(gen, dtype, *shape):
    """Rows whose values are decoded mx8 values: encoding them again changes nothing."""
    x = torch.randn(*shape, device=DEV, generator=gen).to(dtype)
    return mx8_decode(*mx8_encode(x), dtype)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---------------------------------------------------------------- 1. bytes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_split_writes_the_encoders_bytes_and_nothing_else(dtype, geometry):
    """Real rope tables.  Scalar entry point at three positions (the last row of the cache among them) and the _seq one with an inactive
    sequence and one outside the cache, nsplit 1 and 4: the row written is mx8_encode(decode._rope(k)) / mx8_encode(v) byte for byte,
    every other byte keeps its sentinel, the guards behind all four tensors are intact, inactive sequences keep their output row."""
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    bs, scale = 4, 1.0 / math.sqrt(d)
    cos, sin = _tables(d)
    gen = torch.Generator(device=DEV).manual_seed(hl * 10 + kvl + d)
    for ns in (1, 4):
        scratch = G.rope_attn_split_scratch(bs, hl, d, ns, DEV)
        for positions, per_sequence in (([0] * bs, False), ([257] * bs, False), ([S - 1] * bs, False), ([31, -1, S - 1, S], True),
                                        ([256, 0, 32, -1], True)):
            active = [0 <= p < S for p in positions]
            c = Cache8(gen, dtype, [p if a else 5 for p, a in zip(positions, active)], kvl, d)
            qkv = torch.randn(bs, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
            out = torch.full((bs, hl * d), SENTINEL, device=DEV, dtype=dtype)
            kc, vc, ke, ve = c.tensors
            pos = _dev(positions) if per_sequence else _dev(positions[:1])
            G.rope_attn_split(qkv, cos, sin, pos, kc, vc, hl, kvl, d, scale, scratch, ns, per_sequence=per_sequence, out=out, k_exp=ke, v_exp=ve)
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


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_prefill_writes_the_encoders_bytes_and_nothing_else(dtype, geometry):
    """Real rope tables, T = 130.  dg_prefill_attn_mx8 at p0 = 0, 70 and at the end of the cache (S - 3: three tokens exist), and
    dg_prefill_attn_mx8_seq with len = [130, 1, 65, 0], slot = [2, 0, 3, -1] of 4 (slot 1 is nobody's; the last sequence is a no-op)."""
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    T, scale = 130, 1.0 / math.sqrt(d)
    cos, sin = _tables(d)
    gen = torch.Generator(device=DEV).manual_seed(hl * 10 + kvl + d + 1)
    for p0 in (0, 70, S - 3):
        bs = 2
        c = Cache8(gen, dtype, [p0] * bs, kvl, d)
        qkv = torch.randn(bs * T, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
        out = torch.full((bs * T, hl * d), SENTINEL, device=DEV, dtype=dtype)
        kc, vc, ke, ve = c.tensors
        G.prefill_attn(qkv, cos, sin, _dev([p0]), kc, vc, hl, kvl, d, scale, T, out=out, k_exp=ke, v_exp=ve)
        Tin = min(T, S - p0)
        _, k, v = _split_k_v(qkv, hl, kvl, d)
        pos = (torch.arange(T, device=DEV) + p0).clamp_max(S - 1).repeat(bs)
        kr = _rope(k, cos, sin, pos).view(bs, T, kvl, d)
        want = {n: t.clone() for n, t in c.initial.items()}
        for b in range(bs):
            _put(want, b, p0, kr[b, :Tin].transpose(0, 1), v.view(bs, T, kvl, d)[b, :Tin].transpose(0, 1))
        c.expect(want, ("scalar", p0))
        o = out.view(bs, T, -1)
        assert torch.isfinite(o[:, :Tin].float()).all() and (o[:, Tin:] == SENTINEL).all(), p0
    n, lens, pos0, slot = 4, [130, 1, 65, 0], [0, 41, 257, 9], [2, 0, 3, -1]
    prefix = [20] * 4
    for i in range(3):
        prefix[slot[i]] = pos0[i]
    c = Cache8(gen, dtype, prefix, kvl, d)
    qkv = torch.randn(n * T, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    out = torch.full((n * T, hl * d), SENTINEL, device=DEV, dtype=dtype)
    kc, vc, ke, ve = c.tensors
    G.prefill_attn(qkv, cos, sin, _dev(pos0), kc, vc, hl, kvl, d, scale, T, out=out, lengths=_dev(lens), slots=_dev(slot), k_exp=ke, v_exp=ve)
    _, k, v = _split_k_v(qkv, hl, kvl, d)
    want = {name: t.clone() for name, t in c.initial.items()}
    o = out.view(n, T, -1)
    for i in range(n):
        L = lens[i]
        if L > 0 and slot[i] >= 0:
            ki, vi = k.view(n, T, kvl, d)[i, :L], v.view(n, T, kvl, d)[i, :L]
            _put(want, slot[i], pos0[i], _rope(ki, cos, sin, torch.arange(L) + pos0[i]).transpose(0, 1), vi.transpose(0, 1))
            assert torch.isfinite(o[i, :L].float()).all(), i
        assert (o[i, max(L, 0):] == SENTINEL).all(), i
    c.expect(want, "per sequence")


# ---------------------------------------------------------------- 2. the 16-bit kernels' arithmetic, no tolerance
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_split_equals_the_16_bit_split_kernel_bit_for_bit(dtype, geometry):
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    scale = 1.0 / math.sqrt(d)
    cos, sin = _tables(d, identity=True, misaligned=True)
    gen = torch.Generator(device=DEV).manual_seed(hl * 10 + kvl + d + 2)
    bs = len(POSITIONS)
    c0 = Cache8(gen, dtype, POSITIONS, kvl, d)
    q = torch.randn(bs, hl * d, device=DEV, generator=gen).to(dtype)
    qkv = torch.cat([q, _decoded_rows(gen, dtype, bs, 2 * kvl * d // 32, 32).view(bs, -1)], dim=1).contiguous()
    for ns in (1, 4):
        scr = G.rope_attn_split_scratch(bs, hl, d, ns, DEV)
        for per_sequence in (True, False):
            for p in ([None] if per_sequence else POSITIONS):
                for name in TAILS:
                    getattr(c0, name).copy_(c0.initial[name])
                kc, vc, ke, ve = c0.tensors
                k16, v16 = c0.decoded(dtype)
                # (the scalar entry points put every sequence at p: rows of the slots whose prefix is shorter are the finite sentinel rows)
                pos = _dev(POSITIONS) if per_sequence else _dev([p])
                got = G.rope_attn_split(qkv, cos, sin, pos, kc, vc, hl, kvl, d, scale, scr, ns, per_sequence=per_sequence, k_exp=ke, v_exp=ve)
                want = G.rope_attn_split(qkv, cos, sin, pos, k16, v16, hl, kvl, d, scale, scr, ns, per_sequence=per_sequence)
                what = (ns, per_sequence, p)
                assert torch.isfinite(want.float()).all(), what
                assert _same(got, want), (what, (got.float() - want.float()).abs().max().item())
                kd, vd = c0.decoded(dtype)
                assert _same(kd, k16) and _same(vd, v16), what  # and the caches hold the same values afterwards


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_prefill_equals_the_16_bit_prefill_kernel_bit_for_bit(dtype, geometry):
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    T, scale = 130, 1.0 / math.sqrt(d)
    cos, sin = _tables(d, identity=True)
    gen = torch.Generator(device=DEV).manual_seed(hl * 10 + kvl + d + 3)

    def chunk(rows):
        q = torch.randn(rows, hl * d, device=DEV, generator=gen).to(dtype)
        return torch.cat([q, _decoded_rows(gen, dtype, rows, 2 * kvl * d // 32, 32).view(rows, -1)], dim=1).contiguous()

    for p0 in (0, 70):
        c = Cache8(gen, dtype, [p0, p0], kvl, d)
        qkv = chunk(2 * T)
        kc, vc, ke, ve = c.tensors
        k16, v16 = c.decoded(dtype)
        got = G.prefill_attn(qkv, cos, sin, _dev([p0]), kc, vc, hl, kvl, d, scale, T, k_exp=ke, v_exp=ve)
        want = G.prefill_attn(qkv, cos, sin, _dev([p0]), k16, v16, hl, kvl, d, scale, T)
        assert torch.isfinite(want.float()).all(), p0
        assert _same(got, want), (p0, (got.float() - want.float()).abs().max().item())
        kd, vd = c.decoded(dtype)
        assert _same(kd, k16) and _same(vd, v16), p0
    n, lens, pos0, slot = 3, [130, 1, 65], [0, 41, 257], [2, 0, 3]
    prefix = [20] * 4
    for i in range(n):
        prefix[slot[i]] = pos0[i]
    c = Cache8(gen, dtype, prefix, kvl, d)
    qkv = chunk(n * T)
    kc, vc, ke, ve = c.tensors
    k16, v16 = c.decoded(dtype)
    outs = [torch.full((n * T, hl * d), SENTINEL, device=DEV, dtype=dtype) for _ in range(2)]
    kw = dict(lengths=_dev(lens), slots=_dev(slot))
    G.prefill_attn(qkv, cos, sin, _dev(pos0), kc, vc, hl, kvl, d, scale, T, out=outs[0], k_exp=ke, v_exp=ve, **kw)
    G.prefill_attn(qkv, cos, sin, _dev(pos0), k16, v16, hl, kvl, d, scale, T, out=outs[1], **kw)
    assert torch.isfinite(outs[1].float()).all() and _same(outs[0], outs[1])
    kd, vd = c.decoded(dtype)
    assert _same(kd, k16) and _same(vd, v16)


# ---------------------------------------------------------------- 3. real rope tables: float64 over the decoded cache
def _f64_check(c, out, k16, v16, what):
    ref = R.attn_ref64(c.q16, k16, v16, c.visible, c.rep, c.scale)
    e16 = R.row_err(R.attn_torch16(c.q16, k16, v16, c.visible, c.rep, c.scale), ref).max().item()
    u = R.unit_roundoff(c.dtype)
    allow = 2 * max(e16, 2 * u)
    assert torch.isfinite(out.float()).all(), what
    worst = R.row_err(out.view(c.bs, c.T, c.hl, c.d), ref).max().item()
    print(f"KV8_F64 {what}: e {worst / u:.2f} u, allowed {allow / u:.2f} u (torch16 {e16 / u:.2f} u)")
    assert worst <= allow, (what, worst / u, allow / u)


def _case8(kind, dtype, bs, geometry, T, p0, seed):
    """A glue_ref case (its q, k, v and rope tables) on an mx8 cache: the prefix rows [0, p0) encoded, sentinel bytes above."""
    hl, kvl, d = geometry
    c = R.attn_case(kind, dtype, bs, hl, kvl, d, S, T, p0, seed=seed).to(DEV)
    cache = Cache8(torch.Generator(device=DEV).manual_seed(seed), dtype, [0] * bs, kvl, d)
    if p0:
        for codes, exps, rows in ((cache.kc, cache.ke, c.k_all), (cache.vc, cache.ve, c.v_all)):
            cd, ex = mx8_encode(rows[:, :, :p0])
            codes[:, :, :p0], exps[:, :, :p0] = cd.view(torch.uint8), ex
    return c, cache


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_real_rope_tables_vs_float64_on_the_decoded_cache(dtype, geometry):
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    bs = 2
    for kind, pos, ns in (("peaked", 257, 4), ("normal", S - 1, 1), ("peaked", 31, 4)):
        c, cache = _case8(kind, dtype, bs, geometry, 1, pos, R.case_seed(1, pos))
        kc, vc, ke, ve = cache.tensors
        scr = G.rope_attn_split_scratch(bs, hl, d, ns, DEV)
        out = G.rope_attn_split(c.qkv, c.cos, c.sin, _dev([pos]), kc, vc, hl, kvl, d, c.scale, scr, ns, k_exp=ke, v_exp=ve)
        k16, v16 = cache.decoded(dtype)
        _f64_check(c, out, k16, v16, f"split {kind} pos {pos} nsplit {ns}")
    for kind, T, p0 in (("peaked", 130, 70), ("normal", 130, 0)):
        c, cache = _case8(kind, dtype, bs, geometry, T, p0, R.case_seed(T, p0))
        kc, vc, ke, ve = cache.tensors
        out = G.prefill_attn(c.qkv, c.cos, c.sin, _dev([p0]), kc, vc, hl, kvl, d, c.scale, T, k_exp=ke, v_exp=ve)
        k16, v16 = cache.decoded(dtype)
        _f64_check(c, out, k16, v16, f"prefill {kind} T {T} p0 {p0}")


# ---------------------------------------------------------------- 4. NaN isolation
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", [(4, 2, 64), (8, 8, 128)])
def test_a_nan_block_is_never_read_above_the_prefix_and_poisons_exactly_its_outputs_inside(dtype, geometry):
    from any4_amd import decode_ops as G

    hl, kvl, d = geometry
    rep, scale, bs = hl // kvl, 1.0 / math.sqrt(d), 3
    cos, sin = _tables(d)
    gen = torch.Generator(device=DEV).manual_seed(hl + d + 4)
    positions = [100, 300, 200]
    c = Cache8(gen, dtype, positions, kvl, d)
    qkv = torch.randn(bs, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    blk = d // 32 - 1  # the block that is poisoned: the row's last

    def decode(ns, poison):
        for name in TAILS:
            getattr(c, name).copy_(c.initial[name])
        for name, b, kv, row in poison:
            getattr(c, name)[b, kv, row, blk] = 255
        kc, vc, ke, ve = c.tensors
        scr = G.rope_attn_split_scratch(bs, hl, d, ns, DEV)
        return G.rope_attn_split(qkv, cos, sin, _dev(positions), kc, vc, hl, kvl, d, scale, scr, ns, per_sequence=True, k_exp=ke, v_exp=ve)

    for ns in (1, 4):
        clean = decode(ns, [])
        assert torch.isfinite(clean.float()).all()
        # above every sequence's own position (their new rows sit at 100 / 300 / 200): the row behind it, and the last row of the cache
        above = [(name, b, kv, row) for name in ("ke", "ve") for b in range(bs) for kv in range(kvl) for row in (positions[b] + 1, S - 1)]
        assert _same(decode(ns, above), clean), ns
        # inside: K of (sequence 1, kv head 0) at row 37 -> every output of that head group is NaN, nothing else changes
        got = decode(ns, [("ke", 1, 0, 37)]).view(bs, hl, d)
        nan = torch.zeros(bs, hl, d, dtype=torch.bool, device=DEV)
        nan[1, :rep] = True
        assert torch.equal(torch.isnan(got), nan) and _same(got[~nan], clean.view(bs, hl, d)[~nan]), ("k", ns)
        # V of (sequence 2, last kv head) at row 199: the 32 columns of the block, in the heads of that group
        got = decode(ns, [("ve", 2, kvl - 1, 199)]).view(bs, hl, d)
        nan.zero_()
        nan[2, hl - rep:, blk * 32:] = True
        assert torch.equal(torch.isnan(got), nan) and _same(got[~nan], clean.view(bs, hl, d)[~nan]), ("v", ns)

    # prefill: T = 40 tokens behind a prefix of 70; a block in the prefix is seen by every token, one behind the chunk by nobody
    T, p0 = 40, 70
    qkv = torch.randn(bs * T, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
    c = Cache8(gen, dtype, [p0] * bs, kvl, d)

    def prefill(poison):
        for name in TAILS:
            getattr(c, name).copy_(c.initial[name])
        for name, b, kv, row in poison:
            getattr(c, name)[b, kv, row, blk] = 255
        kc, vc, ke, ve = c.tensors
        return G.prefill_attn(qkv, cos, sin, _dev([p0]), kc, vc, hl, kvl, d, scale, T, k_exp=ke, v_exp=ve).view(bs, T, hl, d)

    clean = prefill([])
    assert torch.isfinite(clean.float()).all()
    assert _same(prefill([(name, b, kv, row) for name in ("ke", "ve") for b in range(bs) for kv in range(kvl) for row in (p0 + T, S - 1)]), clean)
    got = prefill([("ke", 1, 0, 37)])
    nan = torch.zeros(bs, T, hl, d, dtype=torch.bool, device=DEV)
    nan[1, :, :rep] = True
    assert torch.equal(torch.isnan(got), nan) and _same(got[~nan], clean[~nan])
    got = prefill([("ve", 2, kvl - 1, 69)])
    nan.zero_()
    nan[2, :, hl - rep:, blk * 32:] = True
    assert torch.equal(torch.isnan(got), nan) and _same(got[~nan], clean[~nan])


# ---------------------------------------------------------------- 5. the stack
def _contract(a, b, what):
    a, b = a.float(), b.float()
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    print(f"KV8_STACK {what}: err {err:.4e} allowed {0.03 * ref + 1e-3:.4e}")
    assert torch.isfinite(a).all() and err <= 0.03 * ref + 1e-3, (what, err, ref)


@pytest.mark.parametrize("fuse_gemm_stages", [True, False])
@pytest.mark.parametrize("ragged", [False, True])
def test_mx8_stack_fused_vs_its_plain_torch_twin(oracle, fuse_gemm_stages, ragged):
    """Five and eight launches, ragged and not: prefill + four decode steps of the fused any4 mx8 stack against the dense twin's
    plain-torch mx8 path; rows that no sequence wrote keep their zero bytes; and the cache tensors are one byte per element."""
    from any4_amd.decode import DecodeConfig, DecodeStack

    cfg = DecodeConfig(**CFG)
    bs, steps = 3, 4
    lengths = [6, 24, 1] if ragged else [6, 6, 6]
    fac = _PairedFactories(oracle, cfg, "linear_y_f16RM_x_f16RM_W_any4TC")
    q = DecodeStack(cfg, fac.any4, DEV, torch.bfloat16, bs=bs, seed=5, fused=True, fuse_gemm_stages=fuse_gemm_stages, ragged=ragged, kv_cache="mx8")
    dn = DecodeStack(cfg, fac.dense, DEV, torch.bfloat16, bs=bs, seed=5, fused=False, ragged=ragged, kv_cache="mx8")
    assert q._attn_scratch is not None and q._attn_split >= 1 and q._five_launch() == fuse_gemm_stages
    T = max(lengths)
    toks = torch.randint(0, cfg.vocab, (bs, T + steps), generator=torch.Generator().manual_seed(1)).to(DEV)
    kw = dict(lengths=lengths) if ragged else {}
    _contract(q.prefill(toks[:, :T], **kw), dn.prefill(toks[:, :T], **kw), "prefill")
    for i in range(steps):
        position = [n + i for n in lengths] if ragged else T + i
        _contract(q.decode(toks[:, T + i], position), dn.decode(toks[:, T + i], position), f"decode {i}")
    for stack in (q, dn):
        for layer in stack.layers:
            tensors = (layer.k_cache, layer.v_cache, layer.k_exp, layer.v_exp)
            assert all(t.element_size() == 1 for t in tensors) and layer.k_cache.dtype == F8 and layer.k_exp.dtype == torch.uint8
            for s, n in enumerate(lengths):
                for t in tensors:
                    assert not t.view(torch.uint8)[s, :, n + steps:].any() and t.view(torch.uint8)[s, :, n + steps - 1].any()


def test_mx8_ragged_stack_at_equal_positions_is_the_non_ragged_stack_and_cache_bytes():
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**CFG)
    bs, T = 3, 6
    mk = lambda **kw: DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=bs, seed=9, **kw)  # noqa: E731
    r, p, full = mk(ragged=True, kv_cache="mx8"), mk(kv_cache="mx8"), mk()
    toks = torch.randint(0, cfg.vocab, (bs, T + 2), generator=torch.Generator().manual_seed(2)).to(DEV)
    assert torch.equal(r.prefill(toks[:, :T], position=[0] * bs, lengths=[T] * bs), p.prefill(toks[:, :T]))
    for i in range(2):
        assert torch.equal(r.decode(toks[:, T + i], [T + i] * bs), p.decode(toks[:, T + i], T + i)), i
    for lr, lp in zip(r.layers, p.layers):
        for name in ("k_cache", "v_cache", "k_exp", "v_exp"):
            assert torch.equal(getattr(lr, name).view(torch.uint8), getattr(lp, name).view(torch.uint8)), name
    assert p.kv_cache_bytes() * 64 == full.kv_cache_bytes() * 33  # (1 + 1/32) / 2 of the 16-bit stack's
    assert full.layers[0].k_cache.element_size() == 2 and full.layers[0].k_exp is None


def test_mx8_graph_replays_with_new_positions():
    """A captured ragged mx8 step replayed with three position vectors (one with an inactive sequence) == the eager step, in bits."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**CFG)
    bs = 3
    eager = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=bs, seed=9, ragged=True, kv_cache="mx8")
    graph = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=bs, seed=9, ragged=True, kv_cache="mx8")
    graph.capture()
    assert graph._graph is not None
    toks = torch.randint(0, cfg.vocab, (bs, 12), generator=torch.Generator().manual_seed(2)).to(DEV)
    lengths = [2, 9, 5]
    names = ("k_cache", "v_cache", "k_exp", "v_exp")
    for stack in (eager, graph):
        for layer in stack.layers:  # (capture's warm-up steps wrote position 0)
            for name in names:
                getattr(layer, name).view(torch.uint8).zero_()
        stack.prefill(toks[:, :9], lengths=lengths)
    for i, position in enumerate(([2, 9, 5], [3, -1, 6], _dev([4, 10, 7]))):
        a, b = eager.decode(toks[:, 9 + i], position), graph.decode(toks[:, 9 + i], position).clone()
        rows = [s for s in range(bs) if i != 1 or s != 1]
        assert torch.isfinite(a[rows].float()).all() and torch.equal(a[rows], b[rows]), i
        for le, lg in zip(eager.layers, graph.layers):
            for name in names:
                assert torch.equal(getattr(le, name).view(torch.uint8), getattr(lg, name).view(torch.uint8)), (i, name)
            if i == 1:  # the inactive sequence wrote nothing
                assert lg.k_exp[1, :, 9].any() and not lg.k_exp[1, :, 10:].any() and not lg.v_cache.view(torch.uint8)[1, :, 10:].any()


# ---------------------------------------------------------------- 6. rejected shapes
@pytest.mark.parametrize("dtype", DTYPES)
def test_rejected_shapes_return_tg_e_shape_and_touch_nothing(dtype):
    """head_dim 16 (a multiple of 8 the 16-bit split kernel takes, not of 32) at the split flavours; head_dim 32 and 96 at the
    prefill ones (64 / 128 only).  Raw calls: the Python front end refuses these before the library sees them."""
    from any4_amd import _lib
    from any4_amd import decode_ops as G
    from tests import attn_abi

    lib = _lib.load()
    TG_E_SHAPE = -7
    hl, kvl, bs, T = 4, 2, 2, 3
    dt = _lib.TG_BF16 if dtype == torch.bfloat16 else _lib.TG_F16
    for entry, d in (("dg_rope_attn_split_mx8", 16), ("dg_rope_attn_split_mx8_seq", 16), ("dg_rope_attn_split_mx8", 48),
                     ("dg_prefill_attn_mx8", 32), ("dg_prefill_attn_mx8_seq", 32), ("dg_prefill_attn_mx8", 96)):
        prefill = "prefill" in entry
        rows = bs * T if prefill else bs
        nb = max(1, d // 32)
        qkv = torch.ones(rows, (hl + 2 * kvl) * d, device=DEV, dtype=dtype)
        cos, sin = torch.ones(S, d, device=DEV), torch.zeros(S, d, device=DEV)
        pos = _dev([3] * bs)
        kc, vc = (torch.full((bs, kvl, S, d), CODE_FILL, dtype=torch.uint8, device=DEV) for _ in range(2))
        ke, ve = (torch.full((bs, kvl, S, nb), EXP_FILL, dtype=torch.uint8, device=DEV) for _ in range(2))
        out = torch.full((rows, hl * d), SENTINEL, device=DEV, dtype=dtype)
        scr = G.rope_attn_split_scratch(bs, hl, 64, 2, DEV)
        st = torch.cuda.current_stream().cuda_stream
        # (the split kernel's fields, the prefill kernel's -- len = slot = NULL, the caches' own batch -- and what they share; a flavour
        #  reads its own)
        rc = attn_abi.launch(lib, entry, 0, st, qkv=qkv.data_ptr(), cos=cos.data_ptr(), sin=sin.data_ptr(), pos=pos.data_ptr(),
                             k_cache=kc.data_ptr(), v_cache=vc.data_ptr(), k_exp=ke.data_ptr(), v_exp=ve.data_ptr(), out=out.data_ptr(),
                             scratch=scr.data_ptr(), scratch_bytes=scr.numel() * 4, nsplit=2, bs=bs, T=T, cache_bs=bs, hl=hl, kvl=kvl, d=d,
                             max_seq=S, scale=0.125, dtype=dt)
        torch.cuda.synchronize()
        assert rc == TG_E_SHAPE, (entry, d, rc)
        assert (kc == CODE_FILL).all() and (vc == CODE_FILL).all() and (ke == EXP_FILL).all() and (ve == EXP_FILL).all(), (entry, d)
        assert (out == SENTINEL).all() and not scr.any(), (entry, d)
