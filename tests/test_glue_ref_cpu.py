"""Checks of the checker (no GPU): the builders and float64 references of tests/glue_ref.py that tests/test_gpu_glue_f64.py relies on.

* the lookup / decoy builders meet their margin condition at every shape the GPU file uses;
* on lookup cases the float64 reference and the 16-bit torch formulations return the target V rows bit for bit;
* the float64 references agree with the existing torch formulations (any4_amd/decode.py) within derived bounds;
* the rope sample of the GPU file is large enough: at its element count, `decode._rope` and either single-FMA contraction of the
  same expression differ in at least 20 elements per type;
* the ragged launches of tests/test_gpu_ragged_f64.py (glue_ref.ragged_case, the page layouts and pools) build at every shape and hold
  what they promise, and that file's own check functions pass a plain CPU model of a paged launch and fail four deliberately wrong
  ones: the wrong sequence's position for the mask, table row b + 1 for b, a page base cut to 32 bits, a split block reading the next
  iteration's page."""
import math

import pytest
import torch

from tests import glue_ref as R

DTYPES = [torch.bfloat16, torch.float16]


def _probe_shapes():
    """Every (bs, hl, kvl, d, S, T, p0, seed) the GPU file builds a lookup / decoy case at."""
    shapes = []
    for bs, (hl, kvl, d) in R.probe_geometries():
        for T, p0, S in R.prefill_chunks((hl, kvl, d), bs):
            shapes.append((bs, hl, kvl, d, S, T, p0, R.case_seed(T, p0)))
    for bs, (hl, kvl, d) in R.probe_geometries(decode=True):
        for pos, S, _ in R.decode_positions((hl, kvl, d), bs):
            shapes.append((bs, hl, kvl, d, S, 1, pos, R.case_seed(1, pos)))
    return shapes


def test_lookup_and_decoy_margins_at_every_gpu_shape():
    """attn_case asserts the margin itself; bf16 and fp16 hold the same +-1 / 2^-4 values, so one type covers the condition."""
    worst = {}
    shapes = _probe_shapes()
    assert len(shapes) > 100
    for bs, hl, kvl, d, S, T, p0, seed in shapes:
        for kind in ("lookup", "decoy"):
            c = R.attn_case(kind, torch.bfloat16, bs, hl, kvl, d, S, T, p0, seed)
            assert c.margin >= R.MARGIN and c.beta <= 16, (kind, bs, hl, kvl, d, S, T, p0)
            # off-target weight: at most (positions) e^-margin, times |V| <= 4, below half a bf16 spacing at the smallest |V| = 2^-4
            assert (p0 + T) * math.exp(-c.margin) * 4 <= 0.5 * 2.0 ** -4 * 2.0 ** -7 * (1 + 1e-9)
            key = (kind, d)
            worst[key] = min(worst.get(key, float("inf")), c.margin)
    print("smallest margins", worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,beta", [(64, 6), (128, 4)])
def test_lookup_rows_are_reproduced_bit_for_bit_by_both_references(dtype, d, beta):
    """bs = 2, 8 / 2 heads, S = 1024, T = 300, p0 = 257: attn_ref64 (rounded once), the 16-bit formulation of glue_ref and
    prefill_attention_torch all return V[target]; so does a decode-shaped case."""
    from any4_amd.decode import prefill_attention_torch

    c = R.attn_case("lookup", dtype, 2, 8, 2, d, 1024, 300, 257, seed=1, beta_min=beta)
    assert c.margin >= R.MARGIN
    want = c.want.view(c.bs, c.T, c.hl, c.d)
    assert R.same_bits(R.case_ref64(c).to(dtype), want)
    assert R.same_bits(R.case_torch16(c), want)
    kc, vc = c.kc0.clone(), c.vc0.clone()
    got = prefill_attention_torch(c.qkv, c.cos, c.sin, c.p0, kc, vc, c.hl, c.kvl, c.d, c.T)
    assert R.same_bits(got, c.want)
    ek, ev = R.expected_caches(c)
    assert R.same_bits(kc, ek) and R.same_bits(vc, ev)
    # targets really cycle through the edges: own, own - 1, 0, tile edges, chunk start, prefix end
    pos = torch.arange(c.p0, c.p0 + c.T).view(1, -1, 1)
    for edge in (pos, pos - 1, torch.zeros_like(pos), pos // 64 * 64, pos // 64 * 64 - 1, torch.full_like(pos, c.p0), torch.full_like(pos, c.p0 - 1),
                 pos // 32 * 32, pos // 256 * 256 - 1):
        assert (c.target == edge).any()
    assert (c.target <= pos).all() and (c.target >= 0).all()
    one = R.attn_case("lookup", dtype, 3, 6, 2, d, 1024, 1, 257, seed=2)
    assert R.same_bits(R.case_ref64(one).to(dtype), one.want.view(3, 1, 6, d)) and R.same_bits(R.case_torch16(one), one.want.view(3, 1, 6, d))


@pytest.mark.parametrize("dtype", DTYPES)
def test_decoy_rows_differ_grossly_from_the_hidden_row(dtype):
    """What a kernel that sees the decoy would return (V[p + 1]) misses the float64 expectation by O(1) of the row's size: far
    outside any allowance of the GPU file (which is a few 16-bit roundings)."""
    for T, p0 in ((40, 70), (1, 256)):
        c = R.attn_case("decoy", dtype, 2, 6, 2, 64, 512, T, p0, seed=3)
        ref = R.case_ref64(c)
        assert torch.isfinite(ref).all() and (c.target[:, :-1] == torch.arange(p0 + 1, p0 + T).view(1, -1, 1)).all()
        assert (c.target[:, -1] == p0 + T).all() and torch.isfinite(c.kc0[:, :, p0 + T].float()).all()
        assert torch.isnan(c.kc0[:, :, p0 + T + 1:].float()).all() and torch.isnan(c.kc0[:, :, p0:p0 + T].float()).all()
        kvh = torch.arange(c.hl) // c.rep
        seen = c.v_all[:, kvh][:, :, p0 + 1:p0 + T + 1].transpose(1, 2)          # [bs, T, hl, d]: the hidden rows
        assert R.row_err(seen, ref).min() > 0.25
    # a chunk that ends at max_seq has no row behind it: its last token looks itself up
    c = R.attn_case("decoy", dtype, 1, 2, 1, 64, 128, 8, 120, seed=4)
    assert (c.target[:, -1] == -1).all() and c.k_all.shape[2] == 128


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["peaked", "normal"])
def test_attention_references_agree(dtype, kind):
    """attn_torch16 is prefill_attention_torch's formulation (the same roundings; matmul shapes differ, so not the same bits), and
    both are within a few 16-bit roundings of attn_ref64.  Derived bound per row and element: the 16-bit score carries |score| u,
    which the exponential turns into a relative error of every weight and of their sum (2 max|score| u); the probability and the
    P . V accumulation add u each -- all of it times sum_s p_s |v_s| (there is cancellation in sum_s p_s v_s) -- and the output
    rounding adds u |ref|."""
    from any4_amd.decode import prefill_attention_torch

    u = R.unit_roundoff(dtype)
    c = R.attn_case(kind, dtype, 2, 4, 2, 64, 512, 130, 70, seed=5)
    ref, t16 = R.case_ref64(c), R.case_torch16(c)
    mass = R.attn_ref64(c.q16, c.k_all, c.v_all.abs(), c.visible, c.rep, c.scale)
    kc, vc = c.kc0.clone(), c.vc0.clone()
    pt = prefill_attention_torch(c.qkv, c.cos, c.sin, c.p0, kc, vc, c.hl, c.kvl, c.d, c.T).view(c.bs, c.T, c.hl, c.d)
    ek, ev = R.expected_caches(c)
    assert R.same_bits(kc, ek) and R.same_bits(vc, ev)
    kvh = torch.arange(c.hl) // c.rep
    smax = (torch.einsum("bthd,bhsd->bths", c.q16.double(), c.k_all[:, kvh].double()).abs().max() * c.scale).item()
    bound = u * ((2 + 2 * smax) * mass + ref.abs())
    for name, got in (("attn_torch16", t16), ("prefill_attention_torch", pt)):
        err = (got.double() - ref).abs()
        print(f"{kind} {dtype} {name}: max|score| {smax:.1f}, largest error / bound {(err / bound).max().item():.3f}, "
              f"largest row error {R.row_err(got, ref).max().item() / u:.2f} u")
        assert (err <= bound).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_and_swiglu_references_agree_with_the_torch_formulations(dtype):
    """The 16-bit torch formulations (decode.RMSNorm, silu * up) round twice, so they sit inside two_roundings_bound of the float64
    references -- the bound the kernels are held to."""
    from any4_amd.decode import RMSNorm

    gen = torch.Generator().manual_seed(0)
    for dim in (8, 64, 2040, 4096):
        h, dl = torch.randn(5, dim, generator=gen).to(dtype), torch.randn(5, dim, generator=gen).to(dtype)
        norm = RMSNorm(dim, 1e-5, "cpu", dtype)
        norm.weight.data = (torch.rand(dim, generator=gen) - 0.5).to(dtype)
        for delta in (dl, None):
            hs, y64 = R.rmsnorm_ref64(h, delta, norm.weight, 1e-5)
            assert R.same_bits(hs, h if delta is None else h + dl)
            assert ((norm(hs).double() - y64).abs() <= R.two_roundings_bound(y64, dtype)).all()
    gu = R.swiglu_input(dtype, 3, 512, "cpu")
    ref = R.swiglu_ref64(gu)
    want = torch.nn.functional.silu(gu[:, :512]) * gu[:, 512:]
    big = ref.abs() > torch.finfo(dtype).max
    assert (((want.double() - ref).abs() <= R.two_roundings_bound(ref, dtype)) | big).all()
    assert (want[big].double() == torch.sign(ref[big]) * float("inf")).all()
    if dtype == torch.float16:
        assert big.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_sample_is_large_enough_to_see_one_contracted_product(dtype):
    """At the element count of test_rope_bits_at_scale (per kernel and type; here the smallest of them), _rope and either single-FMA
    variant of the same expression differ in at least 20 elements after the rounding to 16 bit: a kernel compiled with one product
    contracted cannot pass that test by sample size."""
    n = min(R.rope_elements(kernel) for kernel in R.ROPE_KERNELS)
    assert n >= 1 << 22
    d, S = 128, 8192
    cos, sin = R.rope_tables(d, S)
    rows = n // d
    gen = torch.Generator().manual_seed(1)
    pos = torch.randint(0, S, (rows,), generator=gen)
    x = torch.randn(rows, d, generator=gen).to(dtype)
    want = R._rope(x, cos[pos], sin[pos])
    first, second = R.rope_fma_variants(x, cos[pos], sin[pos])
    n1 = int((first.view(torch.int16) != want.view(torch.int16)).sum())
    n2 = int((second.view(torch.int16) != want.view(torch.int16)).sum())
    print(f"{dtype}: {rows * d} elements, mismatches fma-first {n1}, fma-second {n2}")
    assert n1 >= 20 and n2 >= 20


# ---------------------------------------------------------------- ragged launches (tests/test_gpu_ragged_f64.py)

def _ragged_builds(dtype, kinds):
    """Every ragged case the GPU file builds for `dtype` and `kinds`, as ((geometry, sequences, max_seq, kind), thunk)."""
    assert set(R.RAGGED_SPLIT_LONG_GEOMS) <= set(R.ragged_decode_geoms(False)) and set(R.RAGGED_SPLIT_LONG_GEOMS) <= set(R.ragged_decode_geoms(True))
    for geom in R.ragged_decode_geoms(paged=False):
        for positions, S, _ in R.ragged_decode_sets(geom):
            for kind in kinds:
                yield (geom, positions, S, kind), lambda g=geom, p=positions, s=S, k=kind: R.ragged_decode_case(k, dtype, g, p, s)
    for geom in R.RAGGED_GEOMS:
        for seqs, slots, cache_bs, S in R.ragged_prefill_sets(geom):
            for kind in kinds:
                yield (geom, seqs, S, kind), lambda g=geom, q=seqs, sl=slots, cb=cache_bs, s=S, k=kind: R.ragged_prefill_case(k, dtype, g, q, sl, cb, s)


def _check_ragged_structure(rc, composite_ref):
    """What ragged_case promises, whatever the kind.  composite_ref: per sequence, attn_ref64 on the COMPOSITE (its slot of the expected
    caches) equals attn_ref64 on the scalar case it was made of, and on a lookup launch that plain float64 attention, rounded to the
    type, is the expected row bit for bit (the self-check of the scalar builder, applied to the composite)."""
    assert rc.qkv.shape == (rc.n * rc.T, (rc.hl + 2 * rc.kvl) * rc.d) and torch.isfinite(rc.qkv.float()).all()
    q3 = rc.qkv.view(rc.n, rc.T, -1)
    used = set()
    for i, c in enumerate(rc.seqs):
        s = int(rc.slots[i])
        if c is None:
            assert int(rc.lengths[i]) == 0 and (int(rc.pos[i]) == -1 if rc.decode else s == -1)
            continue
        used.add(s)
        assert int(rc.pos[i]) == c.p0 and int(rc.lengths[i]) == c.T and R.same_bits(q3[i, :c.T].contiguous(), c.qkv)
        assert R.same_bits(rc.kc0[s], c.kc0[0]) and R.same_bits(rc.vc0[s], c.vc0[0])
        ek, ev = R.expected_caches(c)
        assert R.same_bits(rc.kc1[s], ek[0]) and R.same_bits(rc.vc1[s], ev[0]) and rc.rows[s] == c.k_all.shape[2]
        if rc.kind in ("lookup", "decoy"):
            assert c.margin >= R.MARGIN and c.beta <= 16
        if composite_ref:
            got = R.attn_ref64(c.q16, rc.kc1[s:s + 1], rc.vc1[s:s + 1], c.visible, rc.rep, rc.scale)
            assert torch.equal(c.ref64, got)
            if rc.kind == "lookup":
                assert R.same_bits(got.to(rc.dtype).reshape(c.T, -1), c.want), i
    for s in range(rc.cache_bs):
        if s not in used:  # nobody's slot: a finite prefix of its own under NaN, unchanged by the call
            assert 0 < rc.rows[s] and torch.isfinite(rc.kc0[s, :, :rc.rows[s]].float()).all() and torch.isnan(rc.kc0[s, :, rc.rows[s]:].float()).all()
            assert R.same_bits(rc.kc1[s], rc.kc0[s]) and R.same_bits(rc.vc1[s], rc.vc0[s])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kinds", [("lookup", "decoy"), ("peaked", "normal")])
def test_ragged_cases_build_at_every_gpu_shape(dtype, kinds):
    """Every launch of tests/test_gpu_ragged_f64.py, with its seeds: attn_case asserts beta <= 16 and the margin for every sequence of a
    lookup / decoy launch (a seed that fails goes into glue_ref.RAGGED_RESEED); the composite holds what ragged_case promises.  The
    references on the composite are recomputed at max_seq 1024 everywhere and at the longer contexts on one geometry."""
    count, long_geoms = 0, set()
    for (geom, _, S, _), build in _ragged_builds(dtype, kinds):
        _check_ragged_structure(build(), composite_ref=S <= 1024 or geom == (6, 2, 64) or S == 32768)
        count += 1
        long_geoms.update([geom] if S == 32768 else [])
    assert count >= 50 and long_geoms == set(R.RAGGED_SPLIT_LONG_GEOMS)
    for kind in kinds[::2]:   # test_shared_prefix_pages: a decode step and a prefill chunk
        for T in (1, 70):
            rc = R.shared_pair_case(kind, dtype, (6, 2, 64), 1024, T, 256)
            _check_ragged_structure(rc, True)
            a, c = rc.seqs[0], rc.seqs[2]
            assert R.same_bits(rc.kc0[0, :, :256], rc.kc0[2, :, :256]) and R.same_bits(rc.vc0[0, :, :256], rc.vc0[2, :, :256])
            assert not R.same_bits(a.k_all[:, :, 256:256 + c.T], c.k_all[:, :, 256:256 + c.T])


def test_big_cases_build_and_their_tables_straddle_the_line():
    """The cases of the two tests above 4 GiB (built without host caches where those would be 4 GiB each), and the paged one's table:
    every row has pages on both sides of byte 2^32 of the pool."""
    geom, ps = R.BIG_POOL_GEOM, R.BIG_POOL_PAGE
    line = (1 << 32) // (geom[1] * ps * geom[2] * 2)
    assert line * geom[1] * ps * geom[2] * 2 == 1 << 32 and R.BIG_POOL_PAGES > line
    for rc in (R.ragged_decode_case("lookup", torch.bfloat16, geom, R.RAGGED_DECODE[1][0], R.BIG_POOL_S),
               R.ragged_prefill_case("lookup", torch.bfloat16, geom, *R.RAGGED_PREFILL[1])):
        table = R.high_page_table(rc.cache_bs, R.BIG_POOL_S // ps, R.BIG_POOL_PAGES, seed=rc.n)
        assert table.max() == R.BIG_POOL_PAGES - 1 and table.unique().numel() == table.numel()
        for i, c in enumerate(rc.seqs):   # among the pages a sequence NEEDS
            need = table[int(rc.slots[i]), :-(-c.k_all.shape[2] // ps)]
            assert need.numel() == 1 or ((need < line).any() and (need >= line).any()) or c.k_all.shape[2] <= 2 * ps, (i, need)
        assert any((table[int(rc.slots[i]), :-(-c.k_all.shape[2] // ps)] < line).any() and (table[int(rc.slots[i]), :-(-c.k_all.shape[2] // ps)] >= line).any()
                   for i, c in enumerate(rc.seqs))
    bs = R.BIG_CACHE_BS
    rc = R.ragged_decode_case("lookup", torch.bfloat16, R.BIG_CACHE_GEOM, [None] * (bs - 2) + R.BIG_DECODE_POSITIONS, R.BIG_CACHE_S, caches=False)
    assert rc.n == bs and not hasattr(rc, "kc0") and rc.pos.tolist() == [-1] * (bs - 2) + R.BIG_DECODE_POSITIONS
    assert (bs - 2) * R.BIG_CACHE_GEOM[1] * R.BIG_CACHE_S * R.BIG_CACHE_GEOM[2] * 2 >= 1 << 32
    rc = R.ragged_prefill_case("lookup", torch.bfloat16, R.BIG_CACHE_GEOM, R.RAGGED_PREFILL_LONG[0], [bs - 2, bs - 1], bs, R.BIG_CACHE_S, caches=False)
    assert rc.slots.tolist() == [bs - 2, bs - 1] and rc.cache_bs == bs


@pytest.mark.parametrize("page_size", [64, 256, 1024])
def test_pools_round_trip(page_size):
    rc = R.ragged_prefill_case("normal", torch.float16, (4, 2, 64), *R.RAGGED_PREFILL[0])
    table, num_pages = R.page_layout(rc.cache_bs, rc.S, page_size, seed=3)
    assert table.shape == (6, 1024 // page_size) and table.unique().numel() == table.numel() and num_pages == table.numel() + 2
    pool = R.to_pools(rc.kc0, table, page_size, num_pages, 3.0)
    assert R.same_bits(R.from_pools(pool, table, page_size), rc.kc0)
    spare = sorted(set(range(num_pages)) - set(table.flatten().tolist()))
    assert len(spare) == 2 and (pool[spare] == 3.0).all()
    # a trimmed table maps what each slot holds: the round trip is still the cache (unmapped rows were NaN and read as NaN)
    trimmed = R.trim(table, rc.rows, page_size)
    assert (trimmed[2] == -1).sum() == (1024 - rc.rows[2]) // page_size and (trimmed >= 0).any(1).all()
    assert R.same_bits(R.from_pools(R.to_pools(rc.kc0, trimmed, page_size, num_pages, 3.0), trimmed, page_size), rc.kc0)
    # shared rows: the same physical pages, one copy
    if page_size == 64:
        sh = R.shared_pair_case("lookup", torch.float16, (6, 2, 64), 1024, 1, 256)
        table, num_pages = R.page_layout(3, 1024, 64, seed=1, shared=((0, 2, 4),))
        assert torch.equal(table[0, :4], table[2, :4]) and table.unique().numel() == table.numel() - 4 and num_pages == table.numel() - 4 + 2
        assert R.same_bits(sh.kc0[0, :, :256], sh.kc0[2, :, :256])
        assert R.same_bits(R.from_pools(R.to_pools(sh.kc0, table, 64, num_pages, 3.0), table, 64), sh.kc0)


def _model_paged_launch(rc, table, page_size, kp, vp, bug=None, line=None):
    """A plain model of a paged launch on the CPU: every sequence's new rows go through the table into the pools, then every row reads its
    context back through the table, in 32-row units, and is solved in float64 and rounded to the type.  `bug` makes it one of the wrong
    kernels the GPU file has to catch:
      wrong_pos    the NEXT active sequence's position decides what a row may see
      row_plus_1   table row b + 1 is used for b
      base32       a page base cut to 32 bits: (page, kv head) aliases modulo `line` pages.  In the pools of the 4 GiB test the line is
                   page 131072; the callers here put it at num_pages // 2 of a small pool -- the same aliasing at a size the CPU holds
      split_next   a 32-row unit takes the page of the unit behind it (a split block reading iteration c + 1's table entry)"""
    from tests.test_gpu_ragged_f64 import SENTINEL

    kvl, num_pages = rc.kvl, kp.shape[0]
    cb, entries = table.shape

    def phys(page, kv):
        if bug == "base32":
            idx = (page * kvl + kv) % (line * kvl)
            return idx // kvl, idx % kvl
        return page, kv

    def page_of(row, r, write):
        if bug == "row_plus_1":
            row = (row + 1) % cb
        e = r // page_size
        if bug == "split_next" and not write:
            e = min(entries - 1, (r // 32 + 1) * 32 // page_size)
        pg = int(table[row, e])
        return pg if 0 <= pg < num_pages else (-1 if write else 0)

    out = torch.full((rc.n, rc.T, rc.hl * rc.d), SENTINEL, dtype=rc.dtype)
    active = [(i, c, int(rc.slots[i])) for i, c in enumerate(rc.seqs) if c is not None]
    for i, c, s in active:
        for r in range(c.p0, c.p0 + c.T):
            pg = page_of(s, r, True)
            for kv in range(kvl if pg >= 0 else 0):
                p, k2 = phys(pg, kv)
                kp[p, k2, r % page_size], vp[p, k2, r % page_size] = c.k_all[0, kv, r], c.v_all[0, kv, r]
    for j, (i, c, s) in enumerate(active):
        visible = c.visible
        if bug == "wrong_pos":
            other = active[(j + 1) % len(active)][1]
            visible = (other.p0 + torch.arange(c.T) + 1).clamp(max=rc.S)
        P = int(visible.max())
        K, V = torch.empty(1, kvl, P, rc.d, dtype=rc.dtype), torch.empty(1, kvl, P, rc.d, dtype=rc.dtype)
        for r0 in range(0, P, 32):
            r1, pg = min(P, r0 + 32), page_of(s, r0, False)
            for kv in range(kvl):
                p, k2 = phys(pg, kv)
                K[0, kv, r0:r1], V[0, kv, r0:r1] = kp[p, k2, r0 % page_size: r0 % page_size + r1 - r0], vp[p, k2, r0 % page_size: r0 % page_size + r1 - r0]
        out[i, :c.T] = R.attn_ref64(c.q16, K, V, visible, rc.rep, rc.scale).to(rc.dtype).reshape(c.T, -1)
    return out.view(rc.n * rc.T, -1)


BUGS = ("wrong_pos", "row_plus_1", "base32", "split_next")
FAILS = (AssertionError, pytest.fail.Exception)


def _model_run(rc, page_size, bug, trimmed=True):
    """The checks of the GPU file's paged launches, on the model.  Returns what raised: (outputs, pools)."""
    from tests import test_gpu_ragged_f64 as G

    table, num_pages = R.page_layout(rc.cache_bs, rc.S, page_size, seed=7)
    if trimmed:
        table = R.trim(table, rc.rows, page_size)
    (kbuf, kp), (vbuf, vp) = G.pool_buffer(rc.kc0, table, page_size, num_pages), G.pool_buffer(rc.vc0, table, page_size, num_pages)
    out = _model_paged_launch(rc, table, page_size, kp, vp, bug, line=num_pages // 2)
    raised = []
    for check in (lambda: G.check_outputs(rc, out, "model", G.allowances(rc)),
                  lambda: G.check_pools(G.expected_pools(rc, table, page_size, num_pages), kbuf, vbuf, kp, vp, table, page_size, "model")):
        try:
            check()
            raised.append(False)
        except FAILS:
            raised.append(True)
    return tuple(raised)


@pytest.mark.parametrize("kind", ["lookup", "decoy", "peaked", "normal"])
def test_the_gpu_checks_pass_a_right_model_and_fail_the_wrong_ones(kind):
    """tests/test_gpu_ragged_f64.py's own check functions on the CPU model of a paged launch (decode and prefill, 64-position pages): the
    right model passes every check; each wrong one fails the output check (lookup: bit equality; the other kinds: the float64 bound),
    and the two that write through a wrong address fail the pool check as well."""
    geom = (4, 2, 64)
    decode = R.ragged_decode_case(kind, torch.bfloat16, geom, *R.RAGGED_DECODE[1])
    prefill = R.ragged_prefill_case(kind, torch.bfloat16, geom, *R.RAGGED_PREFILL[0])
    for rc in (decode, prefill):
        for trimmed in (True, False):
            assert _model_run(rc, 64, None, trimmed) == (False, False), (rc.decode, trimmed)
        for bug in BUGS:
            outputs, pools = _model_run(rc, 64, bug)
            assert outputs, (rc.decode, bug)
            assert pools == (bug in ("row_plus_1", "base32")), (rc.decode, bug)


def test_the_remaining_gpu_checks_fail_when_they_should():
    """The sentinel checks (an inactive sequence, rows behind a length), the guard / spare-page comparison, the contiguous cache check and
    the NaN-count check of the tests above 4 GiB, each against one wrong element."""
    from tests import test_gpu_ragged_f64 as G

    rc = R.ragged_prefill_case("lookup", torch.float16, (4, 2, 64), *R.RAGGED_PREFILL[0])
    table, num_pages = R.page_layout(rc.cache_bs, rc.S, 64, seed=7)
    (kbuf, kp), (vbuf, vp) = G.pool_buffer(rc.kc0, table, 64, num_pages), G.pool_buffer(rc.vc0, table, 64, num_pages)
    out = _model_paged_launch(rc, table, 64, kp, vp)
    expected = G.expected_pools(rc, table, 64, num_pages)
    G.check_outputs(rc, out, "model", None)
    G.check_pools(expected, kbuf, vbuf, kp, vp, table, 64, "model")
    G.check_caches(rc, R.from_pools(kp, table, 64), R.from_pools(vp, table, 64), "model")
    o3 = out.view(rc.n, rc.T, -1)
    for i, t in ((4, 0), (1, 17), (3, 1)):   # the absent sequence; the first filler row of two present ones
        bad = o3.clone()
        bad[i, t, 5] = 1.0
        with pytest.raises(AssertionError, match="sentinel|behind its length"):
            G.check_outputs(rc, bad.view(rc.n * rc.T, -1), "model", None)
    spare = sorted(set(range(num_pages)) - set(table.flatten().tolist()))
    for buf, at in ((kbuf, 3), (vbuf, kbuf.numel() - 1), (kbuf, G.GUARD_ELEMS + spare[0] * kp[0].numel() + 9)):
        keep = buf[at].clone()
        buf[at] = 1.0
        with pytest.raises(AssertionError, match="spare page, a guard"):
            G.check_pools(expected, kbuf, vbuf, kp, vp, table, 64, "model")
        buf[at] = keep
    kc = R.from_pools(kp, table, 64)
    kc[3, 1, 900, 0] = 0.5   # a NaN row of a slot nobody uses
    with pytest.raises(AssertionError, match="caches differ"):
        G.check_caches(rc, kc, R.from_pools(vp, table, 64), "model")
    # NaN pools: one element written into a page nobody maps changes the count and nothing else
    kn, vn = R.to_pools(rc.kc1, table, 64, num_pages, float("nan")), R.to_pools(rc.vc1, table, 64, num_pages, float("nan"))
    G.check_nan_pools(rc, kn, vn, table, 64, "model")
    vn[spare[1], 0, 0, 0] = 0.0
    with pytest.raises(AssertionError, match="NaN count"):
        G.check_nan_pools(rc, kn, vn, table, 64, "model")
    # ... and the aliasing model against the checks of the 4 GiB test
    kn, vn = R.to_pools(rc.kc0, table, 64, num_pages, float("nan")), R.to_pools(rc.vc0, table, 64, num_pages, float("nan"))
    out = _model_paged_launch(rc, table, 64, kn, vn, "base32", line=num_pages // 2)
    with pytest.raises(AssertionError):
        G.check_outputs(rc, out, "model", None)
    with pytest.raises(AssertionError):
        G.check_nan_pools(rc, kn, vn, table, 64, "model")
