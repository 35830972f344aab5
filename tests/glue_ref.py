"""Input builders and float64 references for the non-GEMM kernels of the decode stack (include/decode_glue_hip.h).

A plain helper module (not a conftest): it runs on any device and never touches the HIP library.  tests/test_glue_ref_cpu.py checks
the builders and the references themselves on the CPU; tests/test_gpu_glue_f64.py uses them against the kernels, and
tests/test_gpu_ragged_f64.py against the per-sequence and paged ones (`ragged_case`: several cases with positions of their own in one
launch; `page_layout` / `to_pools` / `from_pools`: the same caches as page pools behind a scrambled block table).

Attention cases are built on the CPU from a seeded generator (the same bits whichever device runs the test) and moved with `.to()`.
A case describes ONE call of an attention entry point: a chunk of T tokens per sequence at positions p0 ... p0 + T - 1 (T = 1: a
decode step at position p0) on top of a cache prefix [0, p0).

  kind "lookup"   identity rope tables; every key row is an independent random +-1 vector, V entries are odd multiples of 2^-4 inside
                  +-4 (exact in bf16 and fp16, never zero); query (b, t, h) is beta times the key at a chosen visible target position,
                  so softmax is one-hot up to e^-20 and the expected output row is V[b, kv(h), target] BIT FOR BIT: an indexing,
                  masking or staging error returns another V row (or a mixture).
  kind "decoy"    as lookup, but the query points at the key of position p + 1, which the row must NOT see (a later token of the chunk,
                  or a stale finite cache row behind the chunk); the expected output is the float64 attention over the visible rows.
  kind "peaked"   the project's rope tables, standard-normal k and v, q = 4 * standard normal: raw scores have a standard deviation of
                  about 4, a few keys dominate a row, and a lost or misplaced key moves the row by O(1) of its own size.
  kind "normal"   standard-normal q, k, v.
"""
import math
from types import SimpleNamespace

import torch

MARGIN = 20.0  # lookup / decoy: the pointed-at key's score exceeds every other (visible) score by at least this much


def unit_roundoff(dtype):
    """u: half the relative spacing of the 16-bit type (8 significant bits in bf16, 11 in fp16)."""
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def rope_tables(d, max_seq, device="cpu", identity=False):
    """float32 [max_seq, d] cos / sin tables: the project's (theta 5e5), or cos = 1, sin = 0."""
    if identity:
        return torch.ones(max_seq, d, device=device), torch.zeros(max_seq, d, device=device)
    from any4_amd.decode import DecodeConfig, _rope_tables

    return _rope_tables(DecodeConfig(head_dim=d, max_seq=max_seq), device)


def _rope(x, cos, sin):
    from any4_amd.decode import _rope as rope

    return rope(x, cos, sin)


def _target_candidates(pos, p0, rnd):
    """[T, NC] candidate target positions of the query rows at positions `pos` [T] (all clamped into [0, pos]): the edges at which
    the kernels change tile, chunk or code path."""
    t64, t32, t256 = pos // 64 * 64, pos // 32 * 32, pos // 256 * 256
    p0v = torch.full_like(pos, p0)
    cols = [pos, pos - 1, torch.zeros_like(pos),
            t64, t64 + 63, t64 - 64, t64 - 1,           # first / last position of the row's 64-position tile and of the tile before
            p0v, p0v - 1,                               # first position of the chunk, last position of the cache prefix
            t32, t32 - 1, t256, t256 - 1,               # 32-row iterations and 256-row chunks of the decode kernels
            rnd]
    c = torch.stack(cols, dim=1)
    return torch.minimum(c.clamp_min(0), pos[:, None])


def attn_case(kind, dtype, bs, hl, kvl, d, S, T, p0, seed=0, beta_min=4, prefix_from=None):
    """One call of an attention entry point (see the module docstring).  Fields of the returned namespace (CPU tensors; `.to(device)`):
      qkv [bs * T, (hl + 2 kvl) d]   the call's input (row b * T + t), cos / sin [S, d] float32
      kc0 / vc0 [bs, kvl, S, d]      the caches before the call: rows [0, p0) hold the prefix, everything else NaN (decoy: the one
                                     stale row p0 + T is finite)
      k_all / v_all [bs, kvl, P, d]  the finite rows the caches must hold after the call, P = p0 + T (+ 1 with a stale row)
      q16 [bs, T, hl, d]             the roped, 16-bit query the kernels form
      visible [T]                    positions row t may see: p0 + t + 1
      target [bs, T, hl]             lookup: the position whose V row is the expected output; decoy: the hidden position pointed at
                                     (-1 where there is none and the row is a lookup of its own position)
      want [bs * T, hl * d]          lookup only: the expected output, bit for bit
      beta, margin                   lookup / decoy: the query scale used and the smallest score margin it gives (>= MARGIN)
    prefix_from: a case of the same kind, type and geometry whose first min(p0, its p0) cache rows this case takes over (two sequences
    that share a prefix, as forked sequences of a paged cache do); everything else is drawn as without it."""
    assert kind in ("lookup", "decoy", "peaked", "normal") and hl % kvl == 0 and 0 <= p0 and p0 + T <= S and T >= 1
    rep, scale = hl // kvl, 1.0 / math.sqrt(d)
    gen = torch.Generator().manual_seed(seed * 7919 + 13)
    probe = kind in ("lookup", "decoy")
    stale = 1 if (kind == "decoy" and p0 + T < S) else 0
    P = p0 + T + stale
    cos, sin = rope_tables(d, S, identity=probe)
    pos = torch.arange(p0, p0 + T)
    case = SimpleNamespace(kind=kind, dtype=dtype, bs=bs, hl=hl, kvl=kvl, d=d, S=S, T=T, p0=p0, rep=rep, scale=scale, seed=seed,
                           cos=cos, sin=sin, visible=pos + 1, target=None, want=None, beta=None, margin=None)
    if probe:
        assert d >= 64, "+-1 key codes collide at small head dimensions"
        keys = (torch.randint(0, 2, (bs, kvl, P, d), generator=gen) * 2 - 1).float()
        vals = (torch.randint(-32, 32, (bs, kvl, P, d), generator=gen) * 2 + 1).float() / 16.0
        if prefix_from is not None:  # (lookup / decoy prefixes are un-roped +-1 codes: k_all holds them exactly)
            n = min(p0, prefix_from.p0)
            keys[:, :, :n], vals[:, :, :n] = prefix_from.k_all[:, :, :n].float(), prefix_from.v_all[:, :, :n].float()
        if kind == "lookup":
            rnd = (torch.rand(T, generator=gen) * (pos + 1)).long()
            cand = _target_candidates(pos, p0, torch.minimum(rnd, pos))
            nc = cand.shape[1]
            which = (torch.arange(T).view(1, T, 1) + 3 * torch.arange(hl).view(1, 1, hl) + 5 * torch.arange(bs).view(bs, 1, 1) + seed) % nc
            target = torch.gather(cand.view(1, T, nc).expand(bs, T, nc), 2, which)             # [bs, T, hl]
            point = target
        else:
            hidden = (pos + 1).view(1, T, 1).expand(bs, T, hl)
            target = torch.where(hidden < P, hidden, torch.full_like(hidden, -1))
            point = torch.where(hidden < P, hidden, pos.view(1, T, 1).expand(bs, T, hl))       # no hidden row: the row looks itself up
        kvh = (torch.arange(hl) // rep).view(1, 1, hl).expand(bs, T, hl)
        bi = torch.arange(bs).view(bs, 1, 1).expand(bs, T, hl)
        qkey = keys[bi, kvh, point]                                                             # [bs, T, hl, d]
        # margin: key[point] . key[point] = d against the largest key[point] . key[s] over the visible s != point; all of it exact in f32
        # at least MARGIN, and enough that (positions) e^-margin max|V| stays below half a bf16 spacing at the smallest |V| = 2^-4
        need = max(MARGIN, math.log((p0 + T) * 4 / (0.5 * 2.0 ** -4 * 2.0 ** -7)))
        gap = float("inf")
        for b in range(bs):
            for kv in range(kvl):
                qk = qkey[b, :, kv * rep:(kv + 1) * rep].reshape(T * rep, d)
                g = qk @ keys[b, kv, :p0 + T].t()                                               # [T * rep, p0 + T]
                srange = torch.arange(p0 + T).view(1, -1)
                rowpos = pos.repeat_interleave(rep).view(-1, 1)
                pt = point[b, :, kv * rep:(kv + 1) * rep].reshape(-1, 1)
                g = g.masked_fill((srange > rowpos) | (srange == pt), float("-inf"))
                gap = min(gap, d - g.max().item())                                             # (-inf: nothing else visible)
        if gap == float("inf"):  # a single visible position everywhere: nothing to compete with
            beta = beta_min
        else:
            assert gap > 0, f"seed {seed}: a key code collides with the pointed-at key; pick another seed"
            beta = max(beta_min, math.ceil(need / (scale * gap)))
        assert beta <= 16, f"seed {seed}: beta {beta} (gap {gap}); pick another seed"
        margin = beta * scale * gap
        assert margin >= need, (margin, beta, gap)
        case.beta, case.margin, case.target = beta, margin, target
        q = (beta * qkey).to(dtype)
        k_all, v_all = keys.to(dtype), vals.to(dtype)
        assert torch.equal(k_all.float(), keys) and torch.equal(v_all.float(), vals) and torch.equal(q.float(), beta * qkey)
        if kind == "lookup":
            case.want = v_all[bi, kvh, target].reshape(bs * T, hl * d)
    else:
        k_all = torch.randn(bs, kvl, P, d, generator=gen).to(dtype)
        v_all = torch.randn(bs, kvl, P, d, generator=gen).to(dtype)
        q = (torch.randn(bs, T, hl, d, generator=gen) * (4.0 if kind == "peaked" else 1.0)).to(dtype)
        if prefix_from is not None:
            n = min(p0, prefix_from.p0)
            k_all[:, :, :n], v_all[:, :, :n] = prefix_from.k_all[:, :, :n], prefix_from.v_all[:, :, :n]
    kraw = k_all[:, :, p0:p0 + T].transpose(1, 2)                                               # [bs, T, kvl, d]: the chunk's un-roped k
    vraw = v_all[:, :, p0:p0 + T].transpose(1, 2)
    case.qkv = torch.cat([q.reshape(bs * T, hl * d), kraw.reshape(bs * T, kvl * d), vraw.reshape(bs * T, kvl * d)], dim=1).contiguous()
    c, s_ = cos[p0:p0 + T].view(1, T, 1, d), sin[p0:p0 + T].view(1, T, 1, d)
    case.q16 = _rope(q, c, s_)
    k_all = k_all.clone()
    k_all[:, :, p0:p0 + T] = _rope(kraw, c, s_).transpose(1, 2)
    case.k_all, case.v_all = k_all, v_all
    kc0 = torch.full((bs, kvl, S, d), float("nan"), dtype=dtype)
    vc0 = torch.full((bs, kvl, S, d), float("nan"), dtype=dtype)
    kc0[:, :, :p0], vc0[:, :, :p0] = k_all[:, :, :p0], v_all[:, :, :p0]
    if stale:
        kc0[:, :, p0 + T], vc0[:, :, p0 + T] = k_all[:, :, p0 + T], v_all[:, :, p0 + T]
    case.kc0, case.vc0 = kc0, vc0

    def to(device):
        moved = SimpleNamespace(**vars(case))
        for name, val in vars(case).items():
            if torch.is_tensor(val):
                setattr(moved, name, val.to(device))
        return moved

    case.to = to
    return case


def expected_caches(case):
    """The caches after the call, bit for bit: the rows before it with rows [p0, p0 + T) replaced by the roped k / the raw v."""
    kc, vc = case.kc0.clone(), case.vc0.clone()
    kc[:, :, case.p0:case.p0 + case.T] = case.k_all[:, :, case.p0:case.p0 + case.T]
    vc[:, :, case.p0:case.p0 + case.T] = case.v_all[:, :, case.p0:case.p0 + case.T]
    return kc, vc


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16), b.view(torch.int16))


def _row_blocks(R, width, limit=1 << 24):
    step = max(1, limit // max(1, width))
    return [(r0, min(R, r0 + step)) for r0 in range(0, R, step)]


def attn_ref64(q16, k16, v16, visible, rep, scale):
    """softmax(q . k^T * scale) . v in float64 from the 16-bit operands a kernel actually sees.  q16 [bs, R, hl, d] (roped), k16 / v16
    [bs, kvl, >= max(visible), d] (the cache contents), visible [R]: query row r sees cache rows [0, visible[r]).  Returns float64
    [bs, R, hl, d].  Works per (sequence, kv head) and in blocks of query rows, so T = 2048 over 8192 positions stays below 1 GiB."""
    bs, R, hl, d = q16.shape
    kvl = hl // rep
    visible = torch.as_tensor(visible, device=q16.device)
    P = int(visible.max())
    out = torch.empty(bs, R, hl, d, dtype=torch.float64, device=q16.device)
    srange = torch.arange(P, device=q16.device).view(1, 1, P)
    for b in range(bs):
        for kv in range(kvl):
            k, v = k16[b, kv, :P].double(), v16[b, kv, :P].double()
            for r0, r1 in _row_blocks(R, rep * P):
                q = q16[b, r0:r1, kv * rep:(kv + 1) * rep].double()                    # [r, rep, d]
                s = torch.matmul(q, k.t()) * scale                                      # [r, rep, P]
                s = s.masked_fill(srange >= visible[r0:r1].view(-1, 1, 1), float("-inf"))
                out[b, r0:r1, kv * rep:(kv + 1) * rep] = torch.matmul(torch.softmax(s, dim=-1), v)
    return out


def attn_torch16(q16, k16, v16, visible, rep, scale):
    """The 16-bit torch formulation of the same attention (any4_amd/decode.py: 16-bit score matmul, f32 scale and softmax, 16-bit
    probabilities, 16-bit P . V), same arguments as attn_ref64; returns a 16-bit [bs, R, hl, d]."""
    bs, R, hl, d = q16.shape
    kvl = hl // rep
    visible = torch.as_tensor(visible, device=q16.device)
    P = int(visible.max())
    out = torch.empty(bs, R, hl, d, dtype=q16.dtype, device=q16.device)
    srange = torch.arange(P, device=q16.device).view(1, 1, P)
    for b in range(bs):
        for kv in range(kvl):
            k, v = k16[b, kv, :P], v16[b, kv, :P]
            for r0, r1 in _row_blocks(R, rep * P):
                q = q16[b, r0:r1, kv * rep:(kv + 1) * rep]
                s = torch.matmul(q, k.t()).float() * scale
                s = s.masked_fill(srange >= visible[r0:r1].view(-1, 1, 1), float("-inf"))
                out[b, r0:r1, kv * rep:(kv + 1) * rep] = torch.matmul(torch.softmax(s, dim=-1).to(q16.dtype), v)
    return out


def row_err(got, ref64):
    """Per (sequence, row, head): max_d |got - ref64| / max_d |ref64|.  got / ref64 [bs, R, hl, d]."""
    return (got.double() - ref64).abs().amax(-1) / ref64.abs().amax(-1)


def case_ref64(case):
    return attn_ref64(case.q16, case.k_all, case.v_all, case.visible, case.rep, case.scale)


def case_torch16(case):
    return attn_torch16(case.q16, case.k_all, case.v_all, case.visible, case.rep, case.scale)


def returned_rows(case, got, limit=5):
    """Lookup failure report: for the first wrong output rows, which V row (position) of the head's kv head came back, if any."""
    bs, T, hl, d = case.bs, case.T, case.hl, case.d
    g, w = got.view(bs, T, hl, d), case.want.view(bs, T, hl, d)
    bad = (g.view(torch.int16) != w.view(torch.int16)).any(-1).nonzero()
    lines = [f"{bad.shape[0]} of {bs * T * hl} rows wrong"]
    for b, t, h in bad[:limit].tolist():
        hit = (case.v_all[b, h // case.rep].view(torch.int16) == g[b, t, h].view(torch.int16)).all(-1).nonzero().flatten().tolist()
        lines.append(f"(b {b}, position {case.p0 + t}, head {h}): wanted V[{int(case.target[b, t, h])}], got "
                     + (f"V[{hit}]" if hit else f"no V row (first elements {g[b, t, h, :4].tolist()}, wanted {w[b, t, h, :4].tolist()})"))
    return "; ".join(lines)


# ---- RMSNorm / SwiGLU ----

def rmsnorm_ref64(h16, delta16, w16, eps):
    """(h', y): h' = h + delta rounded to 16 bit first (include/decode_glue_hip.h; delta may be None), then the documented formula
    y = h' * rsqrt(mean(h'^2) + eps) * w in float64 from the 16-bit h' and w."""
    hs = h16 if delta16 is None else h16 + delta16
    x = hs.double()
    return hs, x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w16.double()


def swiglu_ref64(gu16):
    """silu(gate) * up in float64 from the 16-bit gu = [gate | up]."""
    il = gu16.shape[1] // 2
    g, u = gu16[:, :il].double(), gu16[:, il:].double()
    return g / (1.0 + torch.exp(-g)) * u


def two_roundings_bound(ref64, dtype):
    """|got - ref64| allowed for a kernel that rounds to 16 bit twice: (1 + u)^2 - 1 = 2u + u^2 relative, 1e-5 relative for the f32
    arithmetic in between, and the type's smallest normal as an absolute floor (results below it lose bits or flush)."""
    u = unit_roundoff(dtype)
    return (2 * u + u * u + 1e-5) * ref64.abs() + torch.finfo(dtype).tiny


def rope_fma_variants(x, cos, sin):
    """The two ways a compiler can contract x * cos + rotate_half(x) * sin into one rounded product and one FMA, emulated in float64
    (an exact product plus an f32 addend fits a double; the double rounding double -> f32 is negligible next to the effect looked
    for).  Returns (fma(x, cos, RN(rot * sin)), fma(rot, sin, RN(x * cos))) rounded to f32 and then to x's type."""
    d2 = x.shape[-1] // 2
    rot = torch.cat([-x[..., d2:], x[..., :d2]], dim=-1)
    p1, p2 = x.float() * cos, rot.float() * sin
    first = (x.double() * cos.double() + p2.double()).float().to(x.dtype)
    second = (p1.double() + rot.double() * sin.double()).float().to(x.dtype)
    return first, second


# ---- the shapes of tests/test_gpu_glue_f64.py (kept here so that tests/test_glue_ref_cpu.py can check the builders at every one) ----

# (hl, kvl, d): hl / kvl = 1, 2, 3, 3, 4, 4, 8; ratio 3 leaves the prefill kernel's head group of 4 partly filled
PROBE_GEOMS = [(2, 2, 64), (4, 2, 128), (6, 2, 64), (3, 1, 128), (4, 1, 64), (32, 8, 128), (8, 1, 128)]
GENERIC_PROBE_GEOM = (4, 2, 256)   # lookup probes of the generic kernels (the only ones that take d = 256)
# decode positions (pos, max_seq): around the 32-row iterations and 256-row chunks of the decode kernels, and the end of the largest cache
DECODE_POSITIONS = [(0, 1024), (31, 1024), (32, 1024), (33, 1024), (255, 1024), (256, 1024), (257, 1024), (700, 1024), (1023, 1024),
                    (8190, 8192), (8191, 8192)]
SPLIT_LONG = [(32767, 32768)]      # split kernel only (nsplit 8), on SPLIT_LONG_GEOMS at bs = 1
SPLIT_LONG_GEOMS = [(4, 2, 128), (6, 2, 64), GENERIC_PROBE_GEOM]
SPLITS = (2, 3, 5, 8)
# prefill chunks (T, p0, max_seq): T around 16 / 32 / 64 / 128, p0 off the 64-position tiles, a chunk that ends at max_seq
PREFILL_CHUNKS = [(15, 0, 1024), (16, 5, 1024), (17, 100, 1024), (31, 0, 1024), (32, 33, 1024), (33, 64, 1024), (63, 1, 1024),
                  (64, 0, 1024), (65, 17, 1024), (127, 0, 1024), (128, 70, 1024), (129, 257, 1024), (300, 257, 1024), (17, 1007, 1024)]
PREFILL_LONG = (2048, 6144, 8192)  # on PREFILL_LONG_GEOMS at bs = 1
PREFILL_LONG_GEOMS = [(32, 8, 128), (6, 2, 64)]


def probe_geometries(decode=False):
    geoms = PROBE_GEOMS + ([GENERIC_PROBE_GEOM] if decode else [])
    return [(bs, g) for g in geoms for bs in (1, 3)]


def prefill_chunks(geom, bs):
    return PREFILL_CHUNKS + ([PREFILL_LONG] if bs == 1 and geom in PREFILL_LONG_GEOMS else [])


def decode_positions(geom, bs):
    """(pos, max_seq, split_only)"""
    return [(p, S, False) for p, S in DECODE_POSITIONS] + ([(p, S, True) for p, S in SPLIT_LONG] if bs == 1 and geom in SPLIT_LONG_GEOMS else [])


def case_seed(T, p0):
    return 131 * T + p0


# rope bits at scale: per kernel a list of plans.  Decode kernels: one launch per position of ROPE_POSITIONS with a fresh qkv; what
# can be compared is q_out (rope_kv only) and the k row written, so a launch contributes bs (hl + kvl) d resp. bs kvl d roped elements.
ROPE_KERNELS = ("rope_kv", "rope_attn", "rope_attn_split", "rope_attn_online", "prefill_attn")
ROPE_POSITIONS = [0, 1, 2, 31, 32, 63, 64, 255, 256, 1023, 2047, 4095, 4096, 4097, 5000, 6143, 6144, 7000, 8190, 8191]
ROPE_MAX_SEQ = 8192
ROPE_MIN_ELEMENTS = 1 << 22


def rope_plan(kernel):
    """[dict(d, bs, hl, kvl, S, calls)]; calls = [(T, p0)] (T = 1 for the decode kernels)."""
    n = len(ROPE_POSITIONS)
    steps = [(1, p) for p in ROPE_POSITIONS]

    def decode_plan(d, hl, kvl, per_launch, want):
        bs = -(-want // (n * per_launch))
        return dict(d=d, bs=bs, hl=hl, kvl=kvl, S=ROPE_MAX_SEQ, calls=steps)

    q = ROPE_MIN_ELEMENTS // 4 + 1
    if kernel == "rope_kv":
        return [decode_plan(d, 4, 4, 8 * d, q) for d in (32, 64, 128, 256)]
    if kernel == "rope_attn":
        return [decode_plan(d, 4, 4, 4 * d, q) for d in (32, 64, 128, 256)]
    if kernel == "rope_attn_split":  # d = 32 / 256 run the generic split kernel (d = 64 / 128: rope_attn_online's, split): the full count on it
        return [decode_plan(d, 8, 8, 8 * d, 2 * q) for d in (32, 256)] + [decode_plan(d, 8, 8, 8 * d, q // 8) for d in (64, 128)]
    if kernel == "rope_attn_online":
        return [decode_plan(d, 8, 8, 8 * d, 2 * q) for d in (64, 128)]
    if kernel == "prefill_attn":
        calls = [(2048, 0), (2048, 6144)]
        return [dict(d=64, bs=2, hl=8, kvl=8, S=ROPE_MAX_SEQ, calls=calls), dict(d=128, bs=1, hl=8, kvl=8, S=ROPE_MAX_SEQ, calls=calls)]
    raise ValueError(kernel)


def rope_elements(kernel):
    """Roped elements test_rope_bits_at_scale compares for `kernel` (per type)."""
    total = 0
    for p in rope_plan(kernel):
        heads = p["hl"] + p["kvl"] if kernel == "rope_kv" else p["kvl"]
        total += sum(T for T, _ in p["calls"]) * p["bs"] * heads * p["d"]
    return total


def swiglu_input(dtype, bs, il, device, seed=0):
    """gu [bs, 2 il]: gates and ups 3 * standard normal, with the gates 0, +-30, +-100 and +-(largest finite fp16) in the first and
    the last columns against ups from {+-0.5, +-1, +-1.5, +-2} (so no product lands between the largest finite value and the
    overflow threshold, where round-to-nearest still returns the finite value)."""
    gen = torch.Generator().manual_seed(1000 + seed + il)
    gu = (torch.randn(bs, 2 * il, generator=gen) * 3).to(dtype)
    gates = torch.tensor([0.0, 30.0, -30.0, 100.0, -100.0, 65504.0, -65504.0])
    ups = torch.tensor([0.5, -1.0, 1.5, -2.0, 2.0, -0.5, 1.0, -1.5])
    cols = list(range(7)) + ([il - 7 + j for j in range(7)] if il >= 16 else [])
    for i, col in enumerate(cols):
        gu[:, col] = gates[i % 7].to(dtype)
        gu[:, il + col] = ups[(torch.arange(bs) + i) % 8].to(dtype)
    return gu.to(device)


# ---- ragged launches: several scalar cases in one call of a per-sequence (_seq) or paged entry point ----

def ragged_case(cases, T=None, slots=None, cache_bs=None, caches=True):
    """One launch made of `attn_case` results built with bs = 1 that share kind, type, geometry and S and may differ in p0 and T; None
    is an inactive sequence.  A launch whose common T is 1 is a decode step (inactive: pos = -1, the sequence keeps its own slot);
    otherwise a prefill chunk (inactive: len = 0, slot = -1, pos = 0).  Fields (CPU tensors; `.to(device)` moves them):
      qkv [n * T, (hl + 2 kvl) d]   row i * T + t; rows t >= T_i (and every row of an inactive sequence) hold finite random filler
      pos / lengths / slots [n]     int64
      kc0 / vc0 [cache_bs, kvl, S, d]   before the call: slot slots[i] is case i's cache; a slot nobody uses holds a finite random prefix
                                    of its own (rows[slot] rows) under NaN, so that a read of the wrong slot returns wrong finite data
      kc1 / vc1                     after the call, bit for bit
      rows [cache_bs]               finite rows per slot after the call (what a live block table has to map)
      seqs [n]                      the scalar cases (None: inactive), each with `ref64` [1, T_i, hl, d] added: want, q16, k_all, v_all,
                                    visible, target are theirs
    caches = False leaves out kc0 / vc0 / kc1 / vc1 (launches whose caches are too large to build on the host)."""
    live = [c for c in cases if c is not None]
    f = live[0]
    for c in live:
        assert c.bs == 1 and (c.kind, c.dtype, c.hl, c.kvl, c.d, c.S) == (f.kind, f.dtype, f.hl, f.kvl, f.d, f.S)
    n = len(cases)
    T = max(c.T for c in live) if T is None else T
    assert all(c.T <= T for c in live)
    decode = T == 1
    if slots is None:
        slots = [i if (c is not None or decode) else -1 for i, c in enumerate(cases)]
    assert len(slots) == n and all((c is None and not decode) == (s < 0) for c, s in zip(cases, slots))
    used = [s for s in slots if s >= 0]
    assert len(set(used)) == len(used)
    cache_bs = max(n if decode else 0, max(used) + 1) if cache_bs is None else cache_bs
    assert cache_bs > max(used) and (not decode or (cache_bs == n and slots == list(range(n))))
    width = (f.hl + 2 * f.kvl) * f.d
    gen = torch.Generator().manual_seed(977 + sum(c.seed for c in live))
    qkv = torch.randn(n, T, width, generator=gen).to(f.dtype)
    for i, c in enumerate(cases):
        if c is not None:
            qkv[i, :c.T] = c.qkv
            c.ref64 = case_ref64(c)
    rc = SimpleNamespace(kind=f.kind, dtype=f.dtype, hl=f.hl, kvl=f.kvl, d=f.d, S=f.S, rep=f.rep, scale=f.scale, cos=f.cos, sin=f.sin,
                         n=n, T=T, decode=decode, cache_bs=cache_bs, seqs=list(cases), qkv=qkv.view(n * T, width).contiguous(),
                         pos=torch.tensor([-1 if c is None and decode else 0 if c is None else c.p0 for c in cases]),
                         lengths=torch.tensor([0 if c is None else c.T for c in cases]), slots=torch.tensor(slots))
    rows = [0] * cache_bs
    for c, s in zip(cases, slots):
        if c is not None:
            rows[s] = c.k_all.shape[2]
    if caches:
        kc0 = torch.full((cache_bs, f.kvl, f.S, f.d), float("nan"), dtype=f.dtype)
        vc0 = kc0.clone()
        for s in range(cache_bs):
            if s not in used or cases[slots.index(s)] is None:  # nobody's slot (decode: an inactive sequence's)
                rows[s] = min(f.S, 40 + 37 * s)
                kc0[s, :, :rows[s]] = torch.randn(f.kvl, rows[s], f.d, generator=gen).to(f.dtype)
                vc0[s, :, :rows[s]] = torch.randn(f.kvl, rows[s], f.d, generator=gen).to(f.dtype)
        kc1, vc1 = kc0.clone(), vc0.clone()
        for c, s in zip(cases, slots):
            if c is not None:
                kc0[s], vc0[s] = c.kc0[0], c.vc0[0]
                kc1[s], vc1[s] = (x[0] for x in expected_caches(c))
        rc.kc0, rc.vc0, rc.kc1, rc.vc1 = kc0, vc0, kc1, vc1
    rc.rows = rows

    def to(device):
        moved = SimpleNamespace(**vars(rc))
        for name, val in vars(rc).items():
            if torch.is_tensor(val):
                setattr(moved, name, val.to(device))
        moved.seqs = [None if c is None else c.to(device) for c in rc.seqs]
        return moved

    rc.to = to
    return rc


def page_layout(cache_bs, S, page_size, seed, spare=2, shared=()):
    """(table int32 [cache_bs, S / page_size], num_pages): physical ids are a seeded permutation of range(num_pages), `spare` of them
    referenced by nobody; each (a, b, n) of `shared` gives the first n entries of row b the pages of row a (the caller guarantees that
    both slots hold the same rows there)."""
    assert S % page_size == 0
    entries = S // page_size
    assert all(n <= entries and a != b for a, b, n in shared)
    num_pages = cache_bs * entries - sum(n for _, _, n in shared) + spare
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(4241 + seed)).tolist()
    table = torch.full((cache_bs, entries), -1, dtype=torch.int32)
    take = {b: (a, n) for a, b, n in shared}
    for b in sorted(range(cache_bs), key=lambda r: r in take):  # (sharing rows after the rows they share with)
        first = 0
        if b in take:
            a, first = take[b]
            table[b, :first] = table[a, :first]
        for e in range(first, entries):
            table[b, e] = perm.pop()
    assert len(perm) == spare
    return table, num_pages


def trim(table, mapped_rows, page_size):
    """A copy of `table` with the entries above each slot's last needed page (mapped_rows[slot] rows are needed) at -1: the normal
    state of a live table."""
    t = table.clone()
    for s, r in enumerate(mapped_rows):
        t[s, -(-int(r) // page_size):] = -1
    return t


def cache_pages(cache, page_size):
    """[cache_bs, kvl, S, d] -> its pages [cache_bs * S / page_size, kvl, page_size, d], in the order of a flattened table."""
    cb, kvl, S, d = cache.shape
    return cache.view(cb, kvl, S // page_size, page_size, d).permute(0, 2, 1, 3, 4).reshape(-1, kvl, page_size, d)


def to_pools(cache, table, page_size, num_pages, fill):
    """[cache_bs, kvl, S, d] -> the pool [num_pages, kvl, page_size, d] behind `table`; pages nobody references hold `fill`."""
    kvl, d = cache.shape[1], cache.shape[3]
    pool = torch.full((num_pages, kvl, page_size, d), fill, dtype=cache.dtype, device=cache.device)
    pages = cache_pages(cache, page_size)
    idx = table.to(cache.device).long().flatten()
    pool[idx[idx >= 0]] = pages[idx >= 0]
    return pool


def from_pools(pool, table, page_size):
    """The contiguous view [cache_bs, kvl, S, d] of a pool behind `table`; unmapped pages read as NaN."""
    _, kvl, ps, d = pool.shape
    assert ps == page_size
    cb, entries = table.shape
    idx = table.to(pool.device).long().flatten()
    pages = torch.full((cb * entries, kvl, ps, d), float("nan"), dtype=pool.dtype, device=pool.device)
    pages[idx >= 0] = pool[idx[idx >= 0]]
    return pages.view(cb, entries, kvl, ps, d).permute(0, 2, 1, 3, 4).reshape(cb, kvl, entries * ps, d)


def high_page_table(cache_bs, entries, num_pages, seed):
    """A table whose rows are a seeded permutation of the HIGHEST cache_bs * entries page ids of a pool (pools above 4 GiB)."""
    n = cache_bs * entries
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(977 + seed)) + (num_pages - n)
    return perm.to(torch.int32).view(cache_bs, entries)


# the shapes of tests/test_gpu_ragged_f64.py: several positions per launch.  (positions of one launch, max_seq); None: inactive
RAGGED_GEOMS = [(4, 2, 64), (6, 2, 64), (3, 1, 128), (32, 8, 128), (8, 8, 128)]   # + GENERIC_PROBE_GEOM on the non-paged general / split kernels
RAGGED_DECODE = [([0, 31, 32, 700], 1024), ([255, 256, 257, 1023], 1024), ([5, None, 64, 33], 1024), ([8191, 4096, 0, 8190], 8192)]
RAGGED_SPLIT_LONG = ([32767, 257], 32768)   # split kernels only (nsplit 8), on RAGGED_SPLIT_LONG_GEOMS
RAGGED_SPLIT_LONG_GEOMS = [(4, 2, 128), (6, 2, 64)]   # (4, 2, 128) is not in RAGGED_GEOMS: it runs this launch alone (ragged_decode_geoms)
RAGGED_SPLITS = SPLITS
# prefill: ((T, p0) per sequence, slots, cache_bs, max_seq); the second set has every p0 on a page edge
RAGGED_PREFILL = [([(129, 257), (17, 1007), (64, 0), (1, 63), None, (33, 64)], [4, 0, 5, 2, -1, 1], 6, 1024),
                  ([(65, 128), (128, 256), (15, 0)], [3, 5, 0], 6, 1024)]
RAGGED_PREFILL_LONG = ([(300, 7892), (64, 4090)], [1, 0], 2, 8192)   # on PREFILL_LONG_GEOMS
PAGE_SIZES = (64, 128, 256, None)   # None: max_seq itself, one page per sequence
# addresses above 4 GiB: pools of 32 KiB pages that end just above the line, caches of 16 MiB slots whose slot 256 starts on it
BIG_POOL_PAGES, BIG_POOL_GEOM, BIG_POOL_PAGE, BIG_POOL_S = 131072 + 32, (4, 2, 128), 64, 1024
BIG_CACHE_BS, BIG_CACHE_GEOM, BIG_CACHE_S = 260, (8, 8, 128), 8192
BIG_DECODE_POSITIONS = [8191, 4096]
# ragged seeds whose lookup / decoy case misses the margin at beta <= 16 (found by tests/test_glue_ref_cpu.py): (T, p0, i) -> seed
RAGGED_RESEED = {}


def page_sizes(S):
    """256 and max_seq itself (one page per sequence) run for the 1024 cases only."""
    return [S if ps is None else ps for ps in PAGE_SIZES] if S == 1024 else [64, 128]


def ragged_seed(T, p0, i):
    return RAGGED_RESEED.get((T, p0, i), case_seed(T, p0) + 1009 * (i + 1))


def ragged_decode_geoms(paged):
    """The geometries of the ragged decode tests: RAGGED_GEOMS (+ GENERIC_PROBE_GEOM on the non-paged general / split kernels), and the
    geometries of RAGGED_SPLIT_LONG_GEOMS that are not among them, which run the 32768-position launch alone."""
    geoms = RAGGED_GEOMS + ([] if paged else [GENERIC_PROBE_GEOM])
    return geoms + [g for g in RAGGED_SPLIT_LONG_GEOMS if g not in geoms]


def ragged_decode_sets(geom):
    """(positions, max_seq, split_only) of the decode launches of a geometry: RAGGED_DECODE on RAGGED_GEOMS and GENERIC_PROBE_GEOM, and
    RAGGED_SPLIT_LONG on every geometry of RAGGED_SPLIT_LONG_GEOMS."""
    sets = [(p, S, False) for p, S in RAGGED_DECODE] if geom in RAGGED_GEOMS + [GENERIC_PROBE_GEOM] else []
    return sets + ([RAGGED_SPLIT_LONG + (True,)] if geom in RAGGED_SPLIT_LONG_GEOMS else [])


def ragged_prefill_sets(geom):
    return RAGGED_PREFILL + ([RAGGED_PREFILL_LONG] if geom in PREFILL_LONG_GEOMS else [])


def ragged_decode_case(kind, dtype, geom, positions, S, caches=True):
    hl, kvl, d = geom
    return ragged_case([None if p is None else attn_case(kind, dtype, 1, hl, kvl, d, S, 1, p, ragged_seed(1, p, i))
                        for i, p in enumerate(positions)], caches=caches)


def ragged_prefill_case(kind, dtype, geom, seqs, slots, cache_bs, S, caches=True):
    hl, kvl, d = geom
    return ragged_case([None if tp is None else attn_case(kind, dtype, 1, hl, kvl, d, S, tp[0], tp[1], ragged_seed(tp[0], tp[1], i))
                        for i, tp in enumerate(seqs)], slots=slots, cache_bs=cache_bs, caches=caches)


def shared_pair_case(kind, dtype, geom, S, T, p0, positions=None):
    """Three sequences in slots 0, 1, 2 of which 0 and 2 share the cache rows [0, p0) and differ in everything they append: a decode step
    (T = 1) or a prefill chunk at p0 (a multiple of the page size)."""
    hl, kvl, d = geom
    a = attn_case(kind, dtype, 1, hl, kvl, d, S, T, p0, ragged_seed(T, p0, 0))
    b = attn_case(kind, dtype, 1, hl, kvl, d, S, max(1, T // 2), p0 + 70, ragged_seed(T, p0 + 70, 1))
    c = attn_case(kind, dtype, 1, hl, kvl, d, S, max(1, T - 3), p0, ragged_seed(T, p0, 2), prefix_from=a)
    return ragged_case([a, b, c], slots=None if T == 1 else [0, 1, 2], cache_bs=3)
