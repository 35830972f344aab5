"""GPU suite: the non-GEMM kernels of the decode stack (decode_glue.cuh, attn_prefill.cuh through any4_amd/decode_ops.py) against
float64 references and lookup probes (tests/glue_ref.py; its builders and references are checked on the CPU by
tests/test_glue_ref_cpu.py).

1. rope bits at scale: q_out and the cache rows every roping kernel writes are `decode._rope`'s bits over >= 2^22 elements per kernel
   and type (a product contracted into an FMA shows in about 1.5e-5 of bf16 and 1e-4 of fp16 elements).
2. lookup / decoy probes on every attention entry point: a row's output is BIT-equal to the V row its query points at, at the tile,
   chunk and prefix edges; a key the row must not see does not leak in.
3. float64 accuracy with a per-(row, head) bound: e = max_d |got - ref64| / max_d |ref64| <= 2 max(e of the 16-bit torch formulation
   over the case, 2u).  The factor 2 covers the kernels' different rounding points (unnormalised probabilities rounded to 16 bit,
   online rescaling); a lost or misplaced key moves a peaked row by O(1).
4. RMSNorm / SwiGLU against float64 under the bound of two 16-bit roundings.
5. shapes the ABI rejects return TG_E_SHAPE without touching an output.

Lines starting with GLUE_F64 / GLUE_ROPE are the error table: dev/glue_f64_table.py condenses a run's `-s` output into
profiles/glue_f64_errors.txt."""
import ctypes
import math

import pytest
import torch

from tests import glue_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_numerics")]
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
TG_E_SHAPE = -7


def _name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp16"


def _nan_like(shape, dtype):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


# ---------------------------------------------------------------- 1. rope bits at scale

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", R.ROPE_KERNELS)
def test_rope_bits_at_scale(kernel, dtype):
    """Every roped element a kernel hands back (rope_kv: q_out and the k row; the fused kernels and prefill: the k rows) equals
    `decode._rope` (two rounded products, a rounded sum, one rounding to 16 bit), the v rows are the raw v, and everything outside
    the written rows is untouched (NaN stays NaN) -- at positions 0, 1, around the tile edges, above 4096 and at max_seq - 1."""
    from any4_amd import decode_ops as G
    from any4_amd.decode import _rope

    assert R.rope_elements(kernel) >= R.ROPE_MIN_ELEMENTS
    gen = torch.Generator(device=DEV).manual_seed(len(kernel) + (0 if dtype == torch.bfloat16 else 100))
    compared = wrong = 0
    for plan in R.rope_plan(kernel):
        d, bs, hl, kvl, S = plan["d"], plan["bs"], plan["hl"], plan["kvl"], plan["S"]
        scale = 1.0 / math.sqrt(d)
        cos, sin = R.rope_tables(d, S, DEV)
        kc, vc = _nan_like((bs, kvl, S, d), dtype), _nan_like((bs, kvl, S, d), dtype)
        scratch = G.rope_attn_split_scratch(bs, hl, d, 4, DEV) if kernel == "rope_attn_split" else None
        written = torch.zeros(S, dtype=torch.bool, device=DEV)
        plan_wrong = 0
        for T, p0 in plan["calls"]:
            qkv = torch.randn(bs * T, (hl + 2 * kvl) * d, device=DEV, generator=gen).to(dtype)
            pos = torch.tensor([p0], device=DEV)
            c, s_ = cos[p0:p0 + T].view(1, T, 1, d), sin[p0:p0 + T].view(1, T, 1, d)
            want_k = _rope(qkv[:, hl * d:(hl + kvl) * d].reshape(bs, T, kvl, d), c, s_).transpose(1, 2)
            want_v = qkv[:, (hl + kvl) * d:].reshape(bs, T, kvl, d).transpose(1, 2)
            if kernel == "rope_kv":
                q = G.rope_kv(qkv, cos, sin, pos, kc, vc, hl, kvl, d)
                want_q = _rope(qkv[:, :hl * d].reshape(bs, T, hl, d), c, s_).reshape(bs, hl, d)
                plan_wrong += int((q.view(torch.int16) != want_q.view(torch.int16)).sum())
                compared += want_q.numel()
            elif kernel == "rope_attn":
                G.rope_attn(qkv, cos, sin, pos, kc, vc, hl, kvl, d, scale)
            elif kernel == "rope_attn_online":
                G.rope_attn_online(qkv, cos, sin, pos, kc, vc, hl, kvl, d, scale)
            elif kernel == "rope_attn_split":
                G.rope_attn_split(qkv, cos, sin, pos, kc, vc, hl, kvl, d, scale, scratch, 4)
            else:
                G.prefill_attn(qkv, cos, sin, pos, kc, vc, hl, kvl, d, scale, T)
            got_k, got_v = kc[:, :, p0:p0 + T], vc[:, :, p0:p0 + T]
            plan_wrong += int((got_k.view(torch.int16) != want_k.view(torch.int16)).sum())
            compared += want_k.numel()
            assert R.same_bits(got_v.contiguous(), want_v.contiguous()), (kernel, d, p0)
            written[p0:p0 + T] = True
        # nothing but the written rows was touched
        assert torch.isnan(kc[:, :, ~written]).all() and torch.isnan(vc[:, :, ~written]).all(), (kernel, d)
        assert not torch.isnan(kc[:, :, written]).any() and not torch.isnan(vc[:, :, written]).any(), (kernel, d)
        print(f"GLUE_ROPE {kernel} {_name(dtype)} d={d} bs={bs} heads={hl}/{kvl}: {plan_wrong} roped elements differ from _rope")
        wrong += plan_wrong
        del kc, vc
    print(f"GLUE_ROPE {kernel} {_name(dtype)} total: {wrong} of {compared} roped elements differ from _rope")
    assert compared >= R.ROPE_MIN_ELEMENTS
    assert wrong == 0, f"{kernel} {_name(dtype)}: {wrong} of {compared} roped elements differ from decode._rope"


# ---------------------------------------------------------------- attention entry points on a glue_ref case

def _run(entry, c, nsplit=None, scratch=None):
    """One call of `entry` on case `c` (device tensors).  Returns (out [bs * T, hl * d], k cache, v cache after the call)."""
    from any4_amd import decode_ops as G

    pos = torch.tensor([c.p0], device=DEV)
    if entry == "decode_attn":  # no rope, no cache write: the caches already hold the new token's rows
        kc, vc = R.expected_caches(c)
        return G.decode_attn(c.q16[:, 0].contiguous(), kc, vc, pos, c.scale), kc, vc
    kc, vc = c.kc0.clone(), c.vc0.clone()
    a = (c.qkv, c.cos, c.sin, pos, kc, vc, c.hl, c.kvl, c.d, c.scale)
    if entry == "rope_attn":
        out = G.rope_attn(*a)
    elif entry == "rope_attn_online":
        out = G.rope_attn_online(*a)
    elif entry == "rope_attn_split":
        out = G.rope_attn_split(*a, scratch, nsplit)
    elif entry == "prefill_attn":
        out = G.prefill_attn(*a, c.T)
    else:
        raise ValueError(entry)
    return out, kc, vc


def _decode_runs(c, split_only):
    """(label, entry, nsplit) for a decode-shaped case: what the ABI accepts at its head dimension and cache length."""
    runs = []
    if not split_only:
        runs += [("decode_attn", "decode_attn", None), ("rope_attn", "rope_attn", None)]
        if c.d in (64, 128):
            runs.append(("rope_attn_online", "rope_attn_online", None))
    nss = (8,) if split_only else R.SPLITS
    runs += [(f"rope_attn_split/{ns}", "rope_attn_split", ns) for ns in nss]
    return runs


def _calls(c, runs):
    """Yield (label, out, kc, vc) for every run; the split kernel goes twice through one scratch buffer (its counters reset themselves)."""
    from any4_amd import decode_ops as G

    for label, entry, ns in runs:
        if entry == "rope_attn_split":
            scratch = G.rope_attn_split_scratch(c.bs, c.hl, c.d, ns, DEV)
            for rnd in (1, 2):
                yield (f"{label} pass {rnd}",) + _run(entry, c, ns, scratch)
        else:
            yield (label,) + _run(entry, c)


def _check_caches(c, kc, vc, what):
    ek, ev = R.expected_caches(c)
    assert R.same_bits(kc, ek) and R.same_bits(vc, ev), f"{what}: caches differ from the expected bits (rows outside the chunk must be untouched)"


def _check_lookup(c, out, what):
    assert R.same_bits(out, c.want), f"{what} lookup (beta {c.beta}, margin {c.margin:.1f}): {R.returned_rows(c, out)}"


def _allowance(c, ref):
    """(allowance, e of the 16-bit torch formulation): 2 max(e_torch16 over the case, 2u)."""
    e16 = R.row_err(R.case_torch16(c), ref).max().item()
    return 2 * max(e16, 2 * R.unit_roundoff(c.dtype)), e16


def _check_f64(c, out, ref, allow, e16, what):
    assert torch.isfinite(out.float()).all(), what
    e = R.row_err(out.view(c.bs, c.T, c.hl, c.d), ref)
    worst = e.max().item()
    u = R.unit_roundoff(c.dtype)
    print(f"GLUE_F64 {what}: e {worst / u:.2f} u, allowed {allow / u:.2f} u (torch16 {e16 / u:.2f} u)")
    if not worst <= allow:
        b, t, h = (e == e.max()).nonzero()[0].tolist()
        pytest.fail(f"{what}: e = {worst / u:.2f} u > {allow / u:.2f} u allowed at (b {b}, position {c.p0 + t}, head {h}); "
                    f"{int((e > allow).sum())} of {e.numel()} rows over")


def _tag(c, bs, geom):
    return f"{_name(c.dtype)} heads={geom[0]}/{geom[1]}x{geom[2]} bs={bs} T={c.T} p0={c.p0} S={c.S} {c.kind}"


# ---------------------------------------------------------------- 2. lookup and decoy probes

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs,geom", R.probe_geometries())
def test_prefill_attn_lookup_and_decoy(dtype, bs, geom):
    hl, kvl, d = geom
    for T, p0, S in R.prefill_chunks(geom, bs):
        for kind in ("lookup", "decoy"):
            c = R.attn_case(kind, dtype, bs, hl, kvl, d, S, T, p0, R.case_seed(T, p0)).to(DEV)
            what = f"prefill_attn {_tag(c, bs, geom)}"
            out, kc, vc = _run("prefill_attn", c)
            _check_caches(c, kc, vc, what)
            if kind == "lookup":
                _check_lookup(c, out, what)
            else:
                ref = R.case_ref64(c)
                _check_f64(c, out, ref, *_allowance(c, ref), what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs,geom", R.probe_geometries(decode=True))
def test_decode_attention_lookup_and_decoy(dtype, bs, geom):
    """decode_attn, rope_attn, rope_attn_online and rope_attn_split (nsplit 2, 3, 5, 8) at the positions of glue_ref.DECODE_POSITIONS;
    rows above the position hold NaN (decoy: the stale row pos + 1 is finite and must not be seen)."""
    hl, kvl, d = geom
    for pos, S, split_only in R.decode_positions(geom, bs):
        for kind in ("lookup", "decoy"):
            c = R.attn_case(kind, dtype, bs, hl, kvl, d, S, 1, pos, R.case_seed(1, pos)).to(DEV)
            ref = allow = None
            if kind == "decoy":
                ref = R.case_ref64(c)
                allow = _allowance(c, ref)
            for label, out, kc, vc in _calls(c, _decode_runs(c, split_only)):
                what = f"{label} {_tag(c, bs, geom)}"
                _check_caches(c, kc, vc, what)
                if kind == "lookup":
                    _check_lookup(c, out, what)
                else:
                    _check_f64(c, out, ref, *allow, what)


# ---------------------------------------------------------------- 3. float64 accuracy, per-row bound

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs,geom", R.probe_geometries())
def test_prefill_attn_vs_float64(dtype, bs, geom):
    hl, kvl, d = geom
    for T, p0, S in R.prefill_chunks(geom, bs):
        for kind in ("peaked", "normal"):
            c = R.attn_case(kind, dtype, bs, hl, kvl, d, S, T, p0, R.case_seed(T, p0)).to(DEV)
            what = f"prefill_attn {_tag(c, bs, geom)}"
            out, kc, vc = _run("prefill_attn", c)
            _check_caches(c, kc, vc, what)
            ref = R.case_ref64(c)
            _check_f64(c, out, ref, *_allowance(c, ref), what)


# the generic kernels also take d = 8, 16, 32 and 256 (peaked / standard-normal cases only: +-1 key codes collide at small d)
F64_DECODE_GEOMS = R.probe_geometries(decode=True) + [(bs, g) for g in ((4, 2, 8), (4, 2, 16), (8, 2, 32)) for bs in (1, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs,geom", F64_DECODE_GEOMS)
def test_decode_attention_vs_float64(dtype, bs, geom):
    hl, kvl, d = geom
    positions = R.decode_positions(geom, bs) + ([(32767, 32768, True)] if bs == 1 and d < 64 else [])
    for pos, S, split_only in positions:
        for kind in ("peaked", "normal"):
            c = R.attn_case(kind, dtype, bs, hl, kvl, d, S, 1, pos, R.case_seed(1, pos)).to(DEV)
            ref = R.case_ref64(c)
            allow = _allowance(c, ref)
            for label, out, kc, vc in _calls(c, _decode_runs(c, split_only)):
                what = f"{label} {_tag(c, bs, geom)}"
                _check_caches(c, kc, vc, what)
                _check_f64(c, out, ref, *allow, what)


# ---------------------------------------------------------------- 4. RMSNorm and SwiGLU against float64

def _rms_raw(h, delta, w, h_out, y, eps):
    """dg_add_rmsnorm with an h_out of the caller's choice (decode_ops.add_rmsnorm always passes h_out = h)."""
    from any4_amd import _lib
    from any4_amd.decode_ops import _dt, _stream

    rows, dim = h.shape
    ptr = lambda t: None if t is None else t.data_ptr()
    return _lib.load().dg_add_rmsnorm(ptr(h), ptr(delta), ptr(w), ptr(h_out), ptr(y), rows, dim, float(eps), _dt(h), h.device.index, _stream(h))


def _rms_inputs(kind, dtype, rows, dim, gen):
    h = torch.randn(rows, dim, device=DEV, generator=gen)
    dl = torch.randn(rows, dim, device=DEV, generator=gen)
    w = torch.rand(dim, device=DEV, generator=gen) + 0.5
    if kind == "tiny":       # eps dominates the mean square
        h, dl = h * 1e-4, dl * 1e-4
    elif kind == "large":    # |x| ~ 200: squares near the top of fp16's range, sums far above it
        h, dl = h * 200, dl * 20
    elif kind == "zero_row":
        h[rows // 2], dl[rows // 2] = 0, 0
    elif kind == "negative_w":
        w = torch.randn(dim, device=DEV, generator=gen)
    return h.to(dtype), dl.to(dtype), w.to(dtype)


def _check_rms(got_y, y64, dtype, what):
    err, bound = (got_y.double() - y64).abs(), R.two_roundings_bound(y64, dtype)
    rel = (err / bound).max().item()
    print(f"GLUE_F64 {what}: largest error / bound {rel:.3f}")
    assert torch.isfinite(got_y.float()).all() and (err <= bound).all(), (what, rel)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [8, 64, 2040, 2048, 2056, 4096, 8192, 16384])
def test_add_rmsnorm_vs_float64(dtype, dim):
    """|y - ref64| <= (2u + u^2 + 1e-5) |ref64| + smallest normal (glue_ref.two_roundings_bound: the kernel rounds x * r and the
    product with w to 16 bit); the residual is bit-equal to torch's h + delta."""
    from any4_amd import decode_ops as G

    eps = 1e-5
    gen = torch.Generator(device=DEV).manual_seed(dim)
    for rows in (1, 3, 257, 4096):
        kinds = ("unit", "tiny", "large", "zero_row", "negative_w") if rows in (3, 257) else ("unit",)
        for kind in kinds:
            h, dl, w = _rms_inputs(kind, dtype, rows, dim, gen)
            what = f"add_rmsnorm {_name(dtype)} rows={rows} dim={dim} {kind}"
            hs, y64 = R.rmsnorm_ref64(h, dl, w, eps)
            # h_out aliasing h (the wrapper's way): h is updated in place
            h1 = h.clone()
            got_h, got_y = G.add_rmsnorm(h1, dl, w, eps)
            assert got_h is h1 and R.same_bits(h1, hs), what
            _check_rms(got_y, y64, dtype, what + " delta, in place")
            if rows == 4096:
                continue
            # h_out not aliasing h: h stays, h_out gets the sum, y the same bits as before
            h2, ho, y2 = h.clone(), _nan_like((rows, dim), dtype), _nan_like((rows, dim), dtype)
            assert _rms_raw(h2, dl, w, ho, y2, eps) == 0
            assert R.same_bits(h2, h) and R.same_bits(ho, hs) and R.same_bits(y2, got_y), what
            # delta = None: no residual write when h_out is h, a copy when it is not
            _, y64n = R.rmsnorm_ref64(h, None, w, eps)
            h3 = h.clone()
            _, y3 = G.add_rmsnorm(h3, None, w, eps)
            assert R.same_bits(h3, h), what
            _check_rms(y3, y64n, dtype, what + " no delta")
            ho, y4 = _nan_like((rows, dim), dtype), _nan_like((rows, dim), dtype)
            assert _rms_raw(h3, None, w, ho, y4, eps) == 0
            assert R.same_bits(ho, h) and R.same_bits(y4, y3), what
            # want_norm = False: residual add only
            h5 = h.clone()
            got_h, none = G.add_rmsnorm(h5, dl, w, eps, want_norm=False)
            assert none is None and R.same_bits(h5, hs), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("il", [8, 504, 512, 14336, 28672])
def test_swiglu_vs_float64(dtype, il):
    """Gates 0, +-30, +-100 and +-65504 among 3 * standard-normal ones; where the float64 result exceeds the largest finite value of
    the type the output is the infinity of that sign, elsewhere it is inside the two-roundings bound."""
    from any4_amd import decode_ops as G

    for bs in (1, 3, 2048):
        gu = R.swiglu_input(dtype, bs, il, DEV, seed=bs)
        got = G.swiglu(gu)
        ref = R.swiglu_ref64(gu)
        big = ref.abs() > torch.finfo(dtype).max
        err, bound = (got.double() - ref).abs(), R.two_roundings_bound(ref, dtype)
        rel = (err[~big] / bound[~big]).max().item()
        print(f"GLUE_F64 swiglu {_name(dtype)} bs={bs} il={il}: largest error / bound {rel:.3f}, {int(big.sum())} overflowing elements")
        assert (err[~big] <= bound[~big]).all() and torch.isfinite(got[~big].float()).all(), (bs, il, rel)
        assert (got[big].double() == torch.sign(ref[big]) * float("inf")).all(), (bs, il)
        if dtype == torch.bfloat16:
            assert not big.any()
        elif bs >= 3 or il >= 16:  # (one row of eight columns pairs +-65504 with +-0.5 / 1 only)
            assert big.any()


# ---------------------------------------------------------------- 5. shapes the ABI rejects (return codes; nothing is launched)

@pytest.mark.parametrize("dtype", DTYPES)
def test_rejected_shapes_return_tg_e_shape_and_touch_nothing(dtype):
    from any4_amd import _lib
    from any4_amd import decode_ops as G
    from any4_amd.decode_ops import _dt, _stream

    lib = _lib.load()
    dt = _dt(torch.empty(0, dtype=dtype))

    def attempt(entry, bs, hl, kvl, d, S):
        """Call `entry` through the C ABI with buffers sized for the shape; returns (rc, every output buffer untouched)."""
        kc = torch.full((bs, kvl, S, d), 1.5, device=DEV, dtype=dtype)
        vc = torch.full((bs, kvl, S, d), -2.5, device=DEV, dtype=dtype)
        out = torch.full((bs, hl * d), 7.0, device=DEV, dtype=dtype)
        q = torch.full((bs, hl, d), 3.0, device=DEV, dtype=dtype)
        qkv = torch.ones(bs, (hl + 2 * kvl) * d, device=DEV, dtype=dtype)
        cos, sin = torch.ones(S, d, device=DEV), torch.zeros(S, d, device=DEV)
        pos = torch.zeros(1, dtype=torch.long, device=DEV)
        st, dev, scale = _stream(qkv), qkv.device.index, 1.0
        p = lambda t: t.data_ptr()
        if entry == "rope_kv":
            rc = lib.dg_rope_kv(p(qkv), p(cos), p(sin), p(pos), p(q), p(kc), p(vc), bs, hl, kvl, d, S, dt, dev, st)
        elif entry == "decode_attn":
            rc = lib.dg_decode_attn(p(q), p(kc), p(vc), p(pos), p(out), bs, hl, kvl, d, S, scale, dt, dev, st)
        else:  # the fused kernels: one dg_attn_launch each
            scr = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
            kernel = {"rope_attn": _lib.DG_ATTN_GENERAL, "rope_attn_online": _lib.DG_ATTN_ONLINE, "rope_attn_split": _lib.DG_ATTN_SPLIT,
                      "prefill_attn": _lib.DG_ATTN_PREFILL}[entry]
            call = _lib.Attn(kernel=kernel, qkv=p(qkv), cos=p(cos), sin=p(sin), pos=p(pos), k_cache=p(kc), v_cache=p(vc), out=p(out),
                             scratch=p(scr), scratch_bytes=scr.numel() * 4, bs=bs, T=1, hl=hl, kvl=kvl, d=d, max_seq=S, scale=scale, nsplit=2,
                             dtype=dt)
            rc = lib.dg_attn_launch(ctypes.byref(call), dev, st)
        torch.cuda.synchronize()
        clean = bool((kc == 1.5).all() and (vc == -2.5).all() and (out == 7.0).all() and (q == 3.0).all())
        return rc, clean

    attention = ("decode_attn", "rope_attn", "rope_attn_online", "rope_attn_split", "prefill_attn")
    cases = [(e, 2, 4, 2, 24, 64) for e in attention]                                  # d = 24: not a head dimension of any attention kernel
    cases += [(e, 2, 4, 2, 264, 64) for e in attention + ("rope_kv",)]                 # d = 264 > 256
    cases += [(e, 1, 2, 1, 64, 8193) for e in ("decode_attn", "rope_attn", "prefill_attn")]  # max_seq = 8193 (the split kernel goes to 65536)
    cases += [(e, 2, 5, 2, 64, 64) for e in attention + ("rope_kv",)]                  # hl % kvl != 0
    for case in cases:
        rc, clean = attempt(*case)
        assert rc == TG_E_SHAPE and clean, (case, rc, clean)
    # the wrappers raise it as an error
    kc = torch.full((2, 2, 64, 24), 1.5, device=DEV, dtype=dtype)
    with pytest.raises(RuntimeError, match="code -7"):
        G.decode_attn(torch.ones(2, 4, 24, device=DEV, dtype=dtype), kc, kc.clone(), torch.zeros(1, dtype=torch.long, device=DEV), 1.0)
    assert (kc == 1.5).all()
    # dg_add_rmsnorm: dim = 16392 (a multiple of 8 above 16384)
    h = torch.full((2, 16392), 1.5, device=DEV, dtype=dtype)
    w, y = torch.ones(16392, device=DEV, dtype=dtype), torch.full((2, 16392), 7.0, device=DEV, dtype=dtype)
    assert _rms_raw(h, h.clone(), w, h, y, 1e-5) == TG_E_SHAPE
    torch.cuda.synchronize()
    assert (h == 1.5).all() and (y == 7.0).all()
    with pytest.raises(RuntimeError, match="code -7"):
        G.add_rmsnorm(h, None, w, 1e-5)
    assert (h == 1.5).all()
