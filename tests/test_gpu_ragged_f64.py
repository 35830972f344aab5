"""GPU suite: the per-sequence and the paged attention kernels -- dg_rope_attn_seq, dg_rope_attn_online_seq, dg_rope_attn_split_seq,
dg_prefill_attn_seq, dg_rope_attn_online_paged, dg_rope_attn_split_paged, dg_prefill_attn_paged -- against the float64 references and
lookup probes of tests/glue_ref.py, with DIFFERENT positions (prefill: positions, lengths and slots) per sequence in one launch and
scrambled block tables.  Every test is the ragged counterpart of one in tests/test_gpu_glue_f64.py and keeps its checks and its bound:

  lookup   each existing output row is BIT-equal to the V row its query points at (a wrong sequence's position, table row or page returns
           another row or NaN)
  decoy / peaked / normal   e = max_d |got - ref64| / max_d |ref64| <= 2 max(e of the 16-bit torch formulation on that sequence, 2u)
  caches   bit-equal to the expected ones; for pools the WHOLE buffer (written rows, every other row, spare pages, guard elements)
  rows that do not exist (an inactive sequence, t >= len_i) keep the caller's sentinel

glue_ref.ragged_case makes a launch of scalar cases; the shape lists live in glue_ref (RAGGED_*), the builders and these very check
functions are exercised on the CPU by tests/test_glue_ref_cpu.py, against deliberately wrong models of a paged launch.  GLUE_F64 lines
are in the format of tests/test_gpu_glue_f64.py (dev/glue_f64_table.py condenses them)."""
import pytest
import torch

from tests import glue_ref as R
from tests.test_gpu_glue_f64 import DTYPES, _allowance, _check_f64, _name, _tag

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_numerics")]
DEV = "cuda:0"
SENTINEL, SPARE, GUARD = 7.0, 3.0, -5.0
GUARD_ELEMS = 4096  # (a multiple of 8: the pools stay 16-byte aligned)
GIB = 1 << 30


# ---------------------------------------------------------------- checks (device-agnostic: tests/test_glue_ref_cpu.py runs them on models)

def allowances(rc):
    """Per sequence (allowance, e of the 16-bit torch formulation), None for lookup launches and inactive sequences."""
    return [None if c is None or rc.kind == "lookup" else _allowance(c, c.ref64) for c in rc.seqs]


def check_outputs(rc, out, label, allow):
    """out [n * T, hl * d] of a launch that started from SENTINEL everywhere."""
    o = out.view(rc.n, rc.T, rc.hl * rc.d)
    for i, c in enumerate(rc.seqs):
        if c is None:
            assert (o[i] == SENTINEL).all(), f"{label}: the inactive sequence {i} lost its sentinel"
            continue
        what = f"{label} {_tag(c, rc.n, (rc.hl, rc.kvl, rc.d))}"
        assert (o[i, c.T:] == SENTINEL).all(), f"{what}: sequence {i} wrote output rows behind its length {c.T}"
        got = o[i, :c.T].contiguous()
        if rc.kind == "lookup":
            assert R.same_bits(got, c.want), f"{what} sequence {i} lookup (beta {c.beta}, margin {c.margin:.1f}): {R.returned_rows(c, got)}"
        else:
            _check_f64(c, got, c.ref64, *allow[i], what)


def check_caches(rc, kc, vc, label):
    assert R.same_bits(kc, rc.kc1) and R.same_bits(vc, rc.vc1), \
        f"{label}: caches differ from the expected bits (only rows [pos_i, pos_i + len_i) of slot_i may change)"


def pool_buffer(cache, table, page_size, num_pages):
    """(buffer, pool view): the pool of `cache` behind `table` (unreferenced pages SPARE) between GUARD_ELEMS guard elements."""
    pool = R.to_pools(cache, table, page_size, num_pages, SPARE)
    buf = torch.full((pool.numel() + 2 * GUARD_ELEMS,), GUARD, dtype=cache.dtype, device=cache.device)
    view = buf[GUARD_ELEMS: GUARD_ELEMS + pool.numel()].view(pool.shape)
    view.copy_(pool)
    return buf, view


def expected_pools(rc, table, page_size, num_pages):
    """What check_pools compares with, made once per table: the expected buffers and the expected caches as the table shows them."""
    return (pool_buffer(rc.kc1, table, page_size, num_pages)[0], pool_buffer(rc.vc1, table, page_size, num_pages)[0],
            R.from_pools(R.to_pools(rc.kc1, table, page_size, num_pages, SPARE), table, page_size),
            R.from_pools(R.to_pools(rc.vc1, table, page_size, num_pages, SPARE), table, page_size))


def check_pools(expected, kbuf, vbuf, kp, vp, table, page_size, label):
    """Read back through the table the pools are the expected caches, and the whole buffers (spare pages, guard elements, rows of pages
    behind a length) are what the expected caches give."""
    ekbuf, evbuf, ek, ev = expected
    assert R.same_bits(R.from_pools(kp, table, page_size), ek) and R.same_bits(R.from_pools(vp, table, page_size), ev), \
        f"{label}: pools read back through the table differ from the expected caches"
    assert R.same_bits(kbuf, ekbuf) and R.same_bits(vbuf, evbuf), f"{label}: a spare page, a guard element or a row of somebody else's page changed"


def nan_count(t):
    """NaN elements of a large tensor, in slices (no full-size temporary)."""
    flat, total = t.view(-1), 0
    for i in range(0, flat.numel(), 1 << 28):
        total += int(torch.isnan(flat[i: i + (1 << 28)]).sum())
    return total


def check_nan_pools(rc, kp, vp, table, page_size, label):
    """Pools that held NaN outside the rows copied in: the mapped pages are the expected caches and the NaN count says that nothing else
    was written (rc.rows finite rows per slot, no host copy of the pools)."""
    assert R.same_bits(R.from_pools(kp, table, page_size), rc.kc1) and R.same_bits(R.from_pools(vp, table, page_size), rc.vc1), \
        f"{label}: mapped pages differ from the expected caches"
    finite = sum(rc.rows) * rc.kvl * rc.d
    assert nan_count(kp) == kp.numel() - finite and nan_count(vp) == vp.numel() - finite, f"{label}: the NaN count of a pool changed"


# ---------------------------------------------------------------- launches

def _sentinel(rc):
    return torch.full((rc.n * rc.T, rc.hl * rc.d), SENTINEL, device=DEV, dtype=rc.dtype)


def _args(rc):
    return rc.qkv, rc.cos, rc.sin, rc.pos


def _geo(rc):
    return rc.hl, rc.kvl, rc.d, rc.scale


def _splits(split_only):
    return (8,) if split_only else R.RAGGED_SPLITS


def _decode_seq_launches(rc, split_only):
    """(label, out, kc, vc) of every per-sequence decode kernel the ABI has for the shape; the split kernel twice through one scratch."""
    from any4_amd import decode_ops as G

    def run(fn, *more):
        kc, vc, out = rc.kc0.clone(), rc.vc0.clone(), _sentinel(rc)
        fn(*_args(rc), kc, vc, *_geo(rc), *more, per_sequence=True, out=out)
        return out, kc, vc

    if not split_only:
        yield ("rope_attn_seq",) + run(G.rope_attn)
        if rc.d in (64, 128):
            yield ("rope_attn_online_seq",) + run(G.rope_attn_online)
    for ns in _splits(split_only):
        scratch = G.rope_attn_split_scratch(rc.n, rc.hl, rc.d, ns, DEV)
        for rnd in (1, 2):
            yield (f"rope_attn_split_seq/{ns} pass {rnd}",) + run(G.rope_attn_split, scratch, ns)


def _tables(rc, page_size, seed, shared=()):
    """(name, table on the device, num_pages): a scrambled table trimmed to the rows each slot holds, and the same one untrimmed."""
    table, num_pages = R.page_layout(rc.cache_bs, rc.S, page_size, seed, shared=shared)
    return [("trimmed", R.trim(table, rc.rows, page_size).to(DEV), num_pages), ("untrimmed", table.to(DEV), num_pages)]


def _decode_paged_launches(rc, split_only, table, page_size, num_pages, passes):
    """(label, out, kbuf, vbuf, k pool, v pool)"""
    from any4_amd import decode_ops as G

    def run(fn, *more):
        (kbuf, kp), (vbuf, vp) = pool_buffer(rc.kc0, table, page_size, num_pages), pool_buffer(rc.vc0, table, page_size, num_pages)
        out = _sentinel(rc)
        fn(*_args(rc), table, kp, vp, *_geo(rc), *more, out=out)
        return out, kbuf, vbuf, kp, vp

    if not split_only:
        yield ("rope_attn_online_paged",) + run(G.rope_attn_online_paged)
    for ns in _splits(split_only):
        scratch = G.rope_attn_split_scratch(rc.n, rc.hl, rc.d, ns, DEV)
        for rnd in passes:
            yield (f"rope_attn_split_paged/{ns} pass {rnd}",) + run(G.rope_attn_split_paged, scratch, ns)


def _prefill_seq(rc):
    from any4_amd import decode_ops as G

    kc, vc, out = rc.kc0.clone(), rc.vc0.clone(), _sentinel(rc)
    G.prefill_attn(*_args(rc), kc, vc, *_geo(rc), rc.T, out=out, lengths=rc.lengths, slots=rc.slots)
    return out, kc, vc


def _prefill_paged(rc, table, page_size, num_pages):
    from any4_amd import decode_ops as G

    (kbuf, kp), (vbuf, vp) = pool_buffer(rc.kc0, table, page_size, num_pages), pool_buffer(rc.vc0, table, page_size, num_pages)
    out = _sentinel(rc)
    G.prefill_attn_paged(*_args(rc), table, kp, vp, *_geo(rc), rc.T, out=out, lengths=rc.lengths, slots=rc.slots)
    return out, kbuf, vbuf, kp, vp


def _context(rc, label, extra=""):
    print(f"RAGGED {label} {_name(rc.dtype)} heads={rc.hl}/{rc.kvl}x{rc.d} S={rc.S} {rc.kind} pos={rc.pos.tolist()} len={rc.lengths.tolist()} "
          f"slots={rc.slots.tolist()}{extra}")


def _decode_body(dtype, geom, kinds, paged):
    for positions, S, split_only in R.ragged_decode_sets(geom):
        for kind in kinds:
            rc = R.ragged_decode_case(kind, dtype, geom, positions, S).to(DEV)
            allow = allowances(rc)
            if not paged:
                for label, out, kc, vc in _decode_seq_launches(rc, split_only):
                    _context(rc, label)
                    check_caches(rc, kc, vc, label)
                    check_outputs(rc, out, label, allow)
                continue
            for page_size in R.page_sizes(S):
                for name, table, num_pages in _tables(rc, page_size, seed=S + page_size):
                    passes = (1, 2) if name == "trimmed" else (1,)
                    expected = expected_pools(rc, table, page_size, num_pages)
                    for label, out, kbuf, vbuf, kp, vp in _decode_paged_launches(rc, split_only, table, page_size, num_pages, passes):
                        _context(rc, label, f" page_size={page_size} table={name}")
                        check_pools(expected, kbuf, vbuf, kp, vp, table, page_size, label)
                        check_outputs(rc, out, label, allow)


def _prefill_body(dtype, geom, kinds):
    for seqs, slots, cache_bs, S in R.ragged_prefill_sets(geom):
        for kind in kinds:
            rc = R.ragged_prefill_case(kind, dtype, geom, seqs, slots, cache_bs, S).to(DEV)
            allow = allowances(rc)
            _context(rc, "prefill_attn_seq")
            out, kc, vc = _prefill_seq(rc)
            check_caches(rc, kc, vc, "prefill_attn_seq")
            check_outputs(rc, out, "prefill_attn_seq", allow)
            for page_size in R.page_sizes(S):
                for name, table, num_pages in _tables(rc, page_size, seed=S + page_size + 1):
                    expected = expected_pools(rc, table, page_size, num_pages)
                    _context(rc, "prefill_attn_paged", f" page_size={page_size} table={name}")
                    out, kbuf, vbuf, kp, vp = _prefill_paged(rc, table, page_size, num_pages)
                    check_pools(expected, kbuf, vbuf, kp, vp, table, page_size, "prefill_attn_paged")
                    check_outputs(rc, out, "prefill_attn_paged", allow)


# ---------------------------------------------------------------- a, b: lookup and decoy (test_*_lookup_and_decoy of test_gpu_glue_f64.py)

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", R.ragged_decode_geoms(paged=False))
def test_ragged_decode_seq_lookup_and_decoy(dtype, geom):
    """test_decode_attention_lookup_and_decoy, ragged: rope_attn / rope_attn_online / rope_attn_split (nsplit 2, 3, 5, 8; twice through
    one scratch) with per_sequence=True at the position
    sets of glue_ref.RAGGED_DECODE in one launch each; RAGGED_SPLIT_LONG ([32767, 257] of 32768 positions, the split kernel at nsplit 8)
    on (4, 2, 128) -- which runs that launch alone -- and (6, 2, 64)."""
    _decode_body(dtype, geom, ("lookup", "decoy"), paged=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", R.ragged_decode_geoms(paged=True))
def test_ragged_decode_paged_lookup_and_decoy(dtype, geom):
    """rope_attn_online_paged / rope_attn_split_paged on the same launches, with pages of 64, 128, 256 and max_seq positions behind a
    scrambled table -- trimmed to each sequence's rows (unmapped entries read page 0, which belongs to somebody else) and untrimmed."""
    _decode_body(dtype, geom, ("lookup", "decoy"), paged=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", R.RAGGED_GEOMS)
def test_ragged_prefill_lookup_and_decoy(dtype, geom):
    """test_prefill_attn_lookup_and_decoy, ragged: prefill_attn(lengths=, slots=) and prefill_attn_paged at glue_ref.RAGGED_PREFILL
    (+ RAGGED_PREFILL_LONG): a position, a length, a slot and a page phase per sequence in one launch, one sequence absent, filler rows
    behind every length."""
    _prefill_body(dtype, geom, ("lookup", "decoy"))


# ---------------------------------------------------------------- c: float64 accuracy on the same launches

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", R.ragged_decode_geoms(paged=False))
def test_ragged_decode_seq_vs_float64(dtype, geom):
    """test_decode_attention_vs_float64 on the launches of test_ragged_decode_seq_lookup_and_decoy: the project's rope tables, peaked and
    standard-normal inputs, the bound per sequence."""
    _decode_body(dtype, geom, ("peaked", "normal"), paged=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", R.ragged_decode_geoms(paged=True))
def test_ragged_decode_paged_vs_float64(dtype, geom):
    """... and on those of test_ragged_decode_paged_lookup_and_decoy."""
    _decode_body(dtype, geom, ("peaked", "normal"), paged=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", R.RAGGED_GEOMS)
def test_ragged_prefill_vs_float64(dtype, geom):
    """test_prefill_attn_vs_float64 on the launches of test_ragged_prefill_lookup_and_decoy."""
    _prefill_body(dtype, geom, ("peaked", "normal"))


# ---------------------------------------------------------------- d: two table rows that name the same physical pages

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("page_size", [64, 128])
def test_shared_prefix_pages(dtype, page_size):
    """Slots 0 and 2 share their first p0 / page_size pages (p0 = 256: whole pages) and append different rows -- a decode step, then a
    prefill chunk -- to pages of their own: both outputs are their own lookups, the shared pages keep their bits (once, in the one
    physical copy), and each private page holds exactly its own sequence's new rows (the whole-buffer comparison of check_pools)."""
    geom, S, p0 = (6, 2, 64), 1024, 256
    shared = ((0, 2, p0 // page_size),)
    for T in (1, 70):
        for kind in ("lookup", "peaked"):
            rc = R.shared_pair_case(kind, dtype, geom, S, T, p0).to(DEV)
            allow = allowances(rc)
            for name, table, num_pages in _tables(rc, page_size, seed=T, shared=shared):
                assert torch.equal(table[0, :p0 // page_size], table[2, :p0 // page_size]) and table[0, p0 // page_size] != table[2, p0 // page_size]
                expected = expected_pools(rc, table, page_size, num_pages)
                if T == 1:
                    launches = _decode_paged_launches(rc, False, table, page_size, num_pages, (1,))
                else:
                    launches = [("prefill_attn_paged",) + _prefill_paged(rc, table, page_size, num_pages)]
                for label, out, kbuf, vbuf, kp, vp in launches:
                    _context(rc, label, f" page_size={page_size} table={name} shared={shared}")
                    check_pools(expected, kbuf, vbuf, kp, vp, table, page_size, label)
                    check_outputs(rc, out, label, allow)


# ---------------------------------------------------------------- e: addresses above 4 GiB

def _need_12_gib():
    free = torch.cuda.mem_get_info()[0]
    if free < 12 * GIB:
        pytest.skip(f"torch.cuda.mem_get_info() reports {free / GIB:.1f} GiB free, less than the 12 GiB this test needs")


def _finite_rows(rc):
    """Elements per cache that are finite after the launch: P_i rows per active sequence."""
    return sum(c.k_all.shape[2] for c in rc.seqs if c is not None) * rc.kvl * rc.d


def test_paged_pools_above_4_gib():
    """Pools [131072 + 32, 2, 64, 128] bf16 (32 KiB pages, page 131072 starts at byte 2^32), NaN everywhere; the table maps the slots onto
    the highest page ids, so every row straddles the line.  rope_attn_online_paged, rope_attn_split_paged (nsplit 4) and
    prefill_attn_paged return their lookups, the mapped pages hold the expected bits and the NaN count of each pool says that nothing
    else was written.  What these sizes can see: a page base kept as a 32-bit BYTE offset (it wraps to the NaN pages at the front of the
    pool, reads them and writes into them) or as a SIGNED 32-bit element index (element 2^31 sits on the same line).  A base kept as an
    unsigned 32-bit element index would still pass -- the pool ends below element 2^32; that needs pools of 8 GiB each."""
    from any4_amd import decode_ops as G

    _need_12_gib()
    dtype, geom, ps, S, num_pages = torch.bfloat16, R.BIG_POOL_GEOM, R.BIG_POOL_PAGE, R.BIG_POOL_S, R.BIG_POOL_PAGES
    kp = torch.full((num_pages, geom[1], ps, geom[2]), float("nan"), dtype=dtype, device=DEV)
    vp = torch.full_like(kp, float("nan"))
    assert kp.numel() * 2 > 4 * GIB
    decode = R.ragged_decode_case("lookup", dtype, geom, R.RAGGED_DECODE[1][0], S)
    prefill = R.ragged_prefill_case("lookup", dtype, geom, *R.RAGGED_PREFILL[1])
    for rc, entries in ((decode, ("rope_attn_online_paged", "rope_attn_split_paged")), (prefill, ("prefill_attn_paged",))):
        rc = rc.to(DEV)
        table = R.high_page_table(rc.cache_bs, S // ps, num_pages, seed=rc.n).to(DEV)
        line = (4 * GIB) // (geom[1] * ps * geom[2] * 2)
        assert ((table < line).any(1) & (table >= line).any(1)).all()
        rows = table.long().flatten()
        for entry in entries:
            kp[rows], vp[rows] = R.cache_pages(rc.kc0, ps), R.cache_pages(rc.vc0, ps)
            out = _sentinel(rc)
            _context(rc, entry, " pools above 4 GiB")
            if entry == "rope_attn_online_paged":
                G.rope_attn_online_paged(*_args(rc), table, kp, vp, *_geo(rc), out=out)
            elif entry == "rope_attn_split_paged":
                G.rope_attn_split_paged(*_args(rc), table, kp, vp, *_geo(rc), G.rope_attn_split_scratch(rc.n, rc.hl, rc.d, 4, DEV), 4, out=out)
            else:
                G.prefill_attn_paged(*_args(rc), table, kp, vp, *_geo(rc), rc.T, out=out, lengths=rc.lengths, slots=rc.slots)
            check_outputs(rc, out, entry, None)
            check_nan_pools(rc, kp, vp, table, ps, entry)
            kp[rows], vp[rows] = float("nan"), float("nan")
    del kp, vp
    torch.cuda.empty_cache()


def _big_caches(rc, slots):
    """NaN caches [BIG_CACHE_BS, kvl, S, d] on the device with the given slots' rows copied in from the scalar cases."""
    kc = torch.full((R.BIG_CACHE_BS, rc.kvl, rc.S, rc.d), float("nan"), dtype=rc.dtype, device=DEV)
    vc = torch.full_like(kc, float("nan"))
    assert kc[slots[0]].data_ptr() - kc.data_ptr() >= 4 * GIB
    return kc, vc


def _check_big(rc, slots, kc, vc, entry):
    for c, s in zip([c for c in rc.seqs if c is not None], slots):
        ek, ev = R.expected_caches(c)
        assert R.same_bits(kc[s], ek[0]) and R.same_bits(vc[s], ev[0]), (entry, s)
    finite = _finite_rows(rc)
    assert nan_count(kc) == kc.numel() - finite and nan_count(vc) == vc.numel() - finite, entry


def test_contiguous_caches_above_4_gib():
    """Caches [260, 8, 8192, 128] bf16 (16 MiB per slot: slot 256 starts at byte 2^32), NaN everywhere but the rows of the last two slots.
    The per-sequence decode kernels at bs = 260 with every sequence inactive except the last two, and prefill_attn with slots
    [258, 259]: lookups, the two slots' bits, the sentinel of the 258 inactive rows and the NaN count of both caches.  As in the paged
    test, a 32-bit byte offset or a signed 32-bit element index of ((b * kvl + kv) * max_seq + pos) * d shows; an unsigned 32-bit
    element index does not (the caches end below element 2^32)."""
    from any4_amd import decode_ops as G

    _need_12_gib()
    dtype, geom, S, bs = torch.bfloat16, R.BIG_CACHE_GEOM, R.BIG_CACHE_S, R.BIG_CACHE_BS
    slots = [bs - 2, bs - 1]
    rc = R.ragged_decode_case("lookup", dtype, geom, [None] * (bs - 2) + R.BIG_DECODE_POSITIONS, S, caches=False).to(DEV)
    kc, vc = _big_caches(rc, slots)
    for entry in ("rope_attn_seq", "rope_attn_online_seq", "rope_attn_split_seq"):
        for s in slots:
            kc[s], vc[s] = rc.seqs[s].kc0[0], rc.seqs[s].vc0[0]
        out = _sentinel(rc)
        print(f"RAGGED {entry} caches above 4 GiB, positions {R.BIG_DECODE_POSITIONS} in slots {slots}")
        if entry == "rope_attn_seq":
            G.rope_attn(*_args(rc), kc, vc, *_geo(rc), per_sequence=True, out=out)
        elif entry == "rope_attn_online_seq":
            G.rope_attn_online(*_args(rc), kc, vc, *_geo(rc), per_sequence=True, out=out)
        else:
            G.rope_attn_split(*_args(rc), kc, vc, *_geo(rc), G.rope_attn_split_scratch(bs, rc.hl, rc.d, 4, DEV), 4, per_sequence=True, out=out)
        check_outputs(rc, out, entry, None)
        _check_big(rc, slots, kc, vc, entry)
    seqs, _, _, _ = R.RAGGED_PREFILL_LONG
    rc = R.ragged_prefill_case("lookup", dtype, geom, seqs, slots, bs, S, caches=False).to(DEV)
    for c, s in zip(rc.seqs, slots):
        kc[s], vc[s] = c.kc0[0], c.vc0[0]
    out = _sentinel(rc)
    print(f"RAGGED prefill_attn_seq caches above 4 GiB, (T, p0) {seqs} in slots {slots}")
    G.prefill_attn(*_args(rc), kc, vc, *_geo(rc), rc.T, out=out, lengths=rc.lengths, slots=rc.slots)
    check_outputs(rc, out, "prefill_attn_seq", None)
    _check_big(rc, slots, kc, vc, "prefill_attn_seq")
    del kc, vc
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- f: the shape of the lists that the paged ABI refuses

@pytest.mark.parametrize("dtype", DTYPES)
def test_paged_entry_points_refuse_head_dimension_256(dtype):
    """glue_ref.GENERIC_PROBE_GEOM (d = 256) runs on the general and the split kernel only: the three paged entry points return
    TG_E_SHAPE and touch neither the output nor a pool.  The same three calls with the same heads, positions, table and page size go
    through at d = 128 first, so it is the head dimension that is refused and no other argument of the calls."""
    from any4_amd import decode_ops as G

    hl, kvl, refused = R.GENERIC_PROBE_GEOM
    S, ps = 1024, 64
    assert refused == 256
    for d in (128, refused):
        rc = R.ragged_decode_case("normal", dtype, (hl, kvl, d), R.RAGGED_DECODE[0][0], S).to(DEV)
        table, num_pages = R.page_layout(rc.cache_bs, S, ps, seed=0)
        table = table.to(DEV)
        scratch = G.rope_attn_split_scratch(rc.n, rc.hl, rc.d, 4, DEV)
        for call in (lambda out, kp, vp: G.rope_attn_online_paged(*_args(rc), table, kp, vp, *_geo(rc), out=out),
                     lambda out, kp, vp: G.rope_attn_split_paged(*_args(rc), table, kp, vp, *_geo(rc), scratch, 4, out=out),
                     lambda out, kp, vp: G.prefill_attn_paged(*_args(rc), table, kp, vp, *_geo(rc), 1, out=out)):
            (kbuf, kp), (vbuf, vp) = pool_buffer(rc.kc0, table, ps, num_pages), pool_buffer(rc.vc0, table, ps, num_pages)
            before = kbuf.clone(), vbuf.clone()
            out = _sentinel(rc)
            if d != refused:
                call(out, kp, vp)
                assert torch.isfinite(out.float()).all() and not (out == SENTINEL).all(1).any() and not R.same_bits(kbuf, before[0])
                continue
            with pytest.raises(RuntimeError, match=r"code -7"):
                call(out, kp, vp)
            torch.cuda.synchronize()
            assert (out == SENTINEL).all() and R.same_bits(kbuf, before[0]) and R.same_bits(vbuf, before[1])
