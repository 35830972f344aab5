"""CPU suite: tests/tile_ref.py proven without a GPU.  tile_plan -- tgx::tile, tgx::tile_w8 and tile_splits restated -- agrees with the
library's workspace answer and plan over a sweep of shapes (without a device the library plans for 256 CUs); the case tables reach the
regimes they name; a plain-torch twin of the tile GEMM's schedule passes every check at the shapes the GPU file runs; each mutant -- one
way in which w4_gemm_tile_kernel, its launch path or its sum kernel could be subtly wrong -- fails the check named for it and, where its regime is
not its own definition, passes the same check outside it.  $TILE_F64_REPORT_CPU names a file for the twin's figures, the mutant table and the table of the earlier
shapes that let each mutant through (profiles/tile_f64_checks.txt)."""
import ctypes
import itertools
import os

import pytest

from tests import tile_ref as R

CUS = 256
RESULTS = []     # (case id, the twin's worst ratio)
CAUGHT = {}      # mutant -> what caught it
SURVIVORS = {}   # mutant -> [(earlier case, steps per workgroup, steps per group, passed)]
TWIN = R.Twin(CUS)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TILE_F64_REPORT_CPU")
    if path:
        with open(path, "w") as f:
            for cid, ratio in RESULTS:
                f.write(f"twin {cid:100s} {ratio:.3f}\n")
            for mutant, what in CAUGHT.items():
                f.write(f"mutant {mutant}: {what}\n")
            for mutant, rows in SURVIVORS.items():
                f.write(f"earlier cases, mutant {mutant}: let through by {sum(r[3] for r in rows)} of {len(rows)}; caught at: "
                        + ("all" if not any(r[3] for r in rows) else ", ".join(f"{cid} ({ksteps} steps)" for cid, ksteps, _, ok in rows if not ok) or "none") + "\n")


# ---------------------------------------------------------------------------------------------------------------------------------
# tile_plan against the library
# ---------------------------------------------------------------------------------------------------------------------------------

def _args(**kw):
    from any4_amd import _lib

    buf = ctypes.create_string_buffer(256)
    pz = (ctypes.addressof(buf) + 63) & ~63   # (nothing is launched: nothing reads the operands)
    a = _lib.W4Gemm(x=pz, w=pz, qinfo=pz, lut=pz, y=pz, batch=1, stride_x=16, stride_w=16, stride_qinfo=16, stride_lut=16, stride_y=16, numerics=_lib.TG_NUM_REFERENCE, **kw)
    return a, buf, pz


def test_tile_plan_against_the_4_bit_workspace_answer_and_plan():
    """tg_gemm_w4_workspace_bytes = splits m wrows 4 (0 when unsplit) wherever tile_plan has a plan, and tg_gemm_w4_plan -- with exactly
    those bytes attached, and with none -- answers 'tile' exactly where tile_plan (workspace or not) has one."""
    from any4_amd import _lib

    lib = _lib.load()
    a, _buf, pz = _args(dtype=_lib.TG_BF16, inner_k_tiles=4, w_on_right=1)
    ref = ctypes.byref(a)
    seen, planned = set(), 0
    ms = (16, 17, 33, 64, 65, 128, 129, 300, 512, 1930, 2048)
    ns = (8, 72, 200, 1032, 2040, 4096)
    ks = (64, 192, 256, 512, 576, 768, 1024, 1152, 1280, 1536, 2048, 2304, 4096, 4608, 14336)
    for a.m, a.wrows, a.k, a.group, qtype in itertools.product(ms, ns, ks, (32, 64, 128, 256), R.QT):
        if a.k % a.group or (qtype == "mx4" and a.group != 32):
            continue
        a.qtype = R.QT[qtype]
        a.workspace, a.workspace_bytes = None, 0
        need = lib.tg_gemm_w4_workspace_bytes(ref)
        case = (a.m, a.wrows, a.k, a.group, qtype, need)
        assert need >= 0, case
        bare = R.tile_plan(a.m, a.wrows, a.k, a.group, qtype, CUS, workspace=False)
        assert (lib.tg_gemm_w4_plan(ref, -1) == _lib.TG_PLAN_TILE) == (bare is not None), case
        if need:
            a.workspace, a.workspace_bytes = pz, need
        plan = R.tile_plan(a.m, a.wrows, a.k, a.group, qtype, CUS)
        assert (lib.tg_gemm_w4_plan(ref, -1) == _lib.TG_PLAN_TILE) == (plan is not None), case
        if plan is not None:
            planned += 1
            assert need == (plan[3] * a.m * a.wrows * 4 if plan[3] > 1 else 0), (case, plan)
            seen.add((plan[0], plan[1], plan[2], plan[3]))
    assert planned > 1000
    assert seen >= {(128, 128, 1, 1)} | {(bm, 64, ks_, s) for bm in (64, 128) for ks_ in (1, 2) for s in (2, 4, 8) if (ks_, s) != (1, 8)} | {(128, 64, 1, 1), (128, 64, 2, 1)}, seen


def test_tile_plan_against_the_int8_workspace_answer():
    from any4_amd import _lib

    lib = _lib.load()
    a, _buf, _pz = _args(dtype=_lib.TG_F16, inner_k_tiles=2, qtype=_lib.TG_Q_INT8)
    ref = ctypes.byref(a)
    splits = set()
    for a.m, a.wrows, a.k, a.group, a.w_on_right in itertools.product((16, 17, 33, 130, 512, 2048), (16, 80, 208, 1040, 4096), (64, 192, 320, 1024, 1152, 1536, 2048, 4096, 4608),
                                                                       (32, 64, 128, 256), (1, 0)):
        if a.k % a.group:
            continue
        need = lib.tg_gemm_w8_workspace_bytes(ref)
        plan = R.tile_plan(a.m, a.wrows, a.k, a.group, "int8", CUS, int8=True, on_right=bool(a.w_on_right))
        want = plan[3] * a.m * a.wrows * 4 if plan is not None and plan[3] > 1 else 0
        assert need == want, (a.m, a.wrows, a.k, a.group, a.w_on_right, need, plan)
        if plan:
            splits.add(plan[3])
    assert splits == {1, 2, 4, 8}


def test_tile_plan_known_launches():
    """The launches tg_tile.hip's comments name, and the derived shapes, by hand."""
    assert R.tile_plan(128, 4096, 4096, 128, "any4_rowwise", 256)[:5] == (128, 64, 2, 4, 8)      # 64 tiles x 4 splits
    assert R.tile_plan(512, 4096, 4096, 128, "any4_rowwise", 256)[:5] == (128, 64, 2, 1, 32)     # 256 tiles: unsplit
    assert R.tile_plan(1024, 4096, 4096, 128, "int4", 256)[:5] == (128, 128, 1, 1, 64)           # a real prefill: the 128 x 128 tile
    assert R.tile_plan(1024, 4096, 4096, 32, "mx4", 256)[:2] == (128, 64)
    assert R.tile_plan(64, 4096, 4096, 128, "int4", 256, workspace=False) is None and R.tile_plan(16, 4096, 4096, 128, "int4", 256) is None
    mw, nw = R.wide_shape(256)
    assert (mw, nw) == (1930, 2040) and R.capped_rows(256) == 1032
    # steps per table buffer and groups per step on the 128 x 128 tile at k = 768: 1 / 1 / 2 / 4 and 2 / 1 / 1 / 1
    assert [R.tile_plan(mw, nw, 768, g, "int4", 256)[5:7] for g in (32, 64, 128, 256)] == [(1, 2), (1, 1), (2, 1), (4, 1)]
    assert [R.tile_plan(130, 72, 256, g, "int4", 256)[5:7] for g in (32, 64, 128, 256)] == [(1, 4), (1, 2), (1, 1), (2, 1)]   # KS = 2
    assert R.tile_plan(1930, 2040, 768, 32, "int4", 255)[:2] == (128, 128) and R.tile_plan(1930, 2040, 768, 32, "int4", 257)[:2] == (128, 64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables reach what they name
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cus", [64, 256, 304])
def test_every_case_is_in_the_regime_it_names(cus):
    for c in R.cases(cus) + R.probe_cases(cus) + R.group_cases(cus) + R.placement_cases(cus):
        R.assert_regime(c, cus)


def test_the_table_covers_every_listed_shape_and_type():
    cs = R.cases(CUS)
    plans = {R.case_id(c): R.plan_of(c, CUS) for c in cs}
    w4 = [c for c in cs if c.kind == "w4" and c.qtype != "mx4"]
    by = lambda sel: {(c.k, c.g) for c in cs if sel(c)}
    steps = lambda bm, bn, ks_, split: {plans[R.case_id(c)][4] for c in w4 if plans[R.case_id(c)][:3] == (bm, bn, ks_) and (plans[R.case_id(c)][3] > 1) == split}
    assert steps(128, 64, 1, False) == {1, 3, 5, 9} and steps(128, 64, 2, False) >= {1, 2, 3, 5, 10, 18}
    assert steps(128, 64, 2, True) >= {4, 5, 6, 8, 9} and steps(128, 64, 1, True) == {9} and steps(128, 128, 1, False) == {1, 5, 12}
    assert {plans[R.case_id(c)][3] for c in w4} == {1, 2, 4, 8}
    assert {c.m for c in w4 if c.want[0] == 64} == {17, 33, 64} and {c.m for c in w4} >= {65, 129, 130, 255}
    assert {c.wrows % 64 for c in w4 if c.side == "B"} >= {8, 40} and {c.wrows % 128 for c in w4 if c.want[1] == 128} == {120}
    assert {plans[R.case_id(c)][7] % 8 for c in cs} >= {0, 1, 2, 4, 6}
    assert {plans[R.case_id(c)][5:7] for c in w4 if c.want[1] == 128 and c.k == 768} == {(1, 2), (1, 1), (2, 1), (4, 1)}
    for dt in (R.BF16, R.F16):
        assert {c.qtype for c in w4 if c.dtype == dt} == {"int4", "any4_global", "any4_rowwise"}
        assert {c.want[:3] for c in w4 if c.dtype == dt} == {(128, 64, 1), (128, 64, 2), (64, 64, 1), (64, 64, 2), (128, 128, 1)}
    assert any(c.side == "A" for c in w4) and {c.want[:2] for c in cs if c.qtype == "mx4"} == {(128, 64), (64, 64)}
    assert by(lambda c: c.kind == "w8") == {(192, 64), (320, 64), (1152, 64), (256, 128), (256, 256), (1024, 128), (1024, 256), (2048, 128), (2048, 256)}
    assert {(c.m, c.side) for c in cs if c.kind == "w8"} == {(17, "B"), (17, "A"), (130, "B"), (130, "A")}


def test_the_regimes_reached_are_the_regimes_wanted():
    """Reached: the restated plan of every case.  Wanted: what the table writes next to it (with the case's own group size)."""
    R.assert_regimes_reached(R.cases(CUS), CUS)


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin passes every check
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.cases(CUS), ids=R.case_id)
def test_twin_float64(oracle, c):
    R.check_f64(TWIN, oracle, c, CUS, RESULTS)


@pytest.mark.parametrize("c", R.probe_cases(CUS), ids=R.case_id)
def test_twin_probes(oracle, c):
    R.check_select(TWIN, c, CUS)
    R.check_onehot(TWIN, oracle, c, CUS)
    R.check_decoy(TWIN, c, CUS)
    R.check_nonfinite(TWIN, oracle, c, CUS)


@pytest.mark.parametrize("c", R.group_cases(CUS), ids=R.case_id)
def test_twin_group_probes(oracle, c):
    R.check_onehot(TWIN, oracle, c, CUS)


@pytest.mark.parametrize("c", R.placement_cases(CUS), ids=R.case_id)
def test_twin_placement(c):
    R.check_placement(TWIN, c, CUS)


# ---------------------------------------------------------------------------------------------------------------------------------
# every mutant fails the check named for it (and only in its regime)
# ---------------------------------------------------------------------------------------------------------------------------------

def _fails(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e).split(";")[0].split(" at (row, column)")[0]
    return None


def _probe(want, kind="w4", qtype=None):
    return next(c for c in R.probe_cases(CUS) if c.want == want and c.kind == kind and (qtype is None or c.qtype == qtype))


KS1_9_STEPS = _probe((128, 64, 1, 1, 9), qtype="int4")          # g = 32 (nsub 2), wrows 264 (wrows % 16 = 8)
KS1_SPLIT_W16 = _probe((128, 64, 1, 2, 9))                      # wrows 528 (wrows % 16 = 0), on the left
KS2_SPLIT = _probe((128, 64, 2, 2, 6))                          # g = 64, split 2
FOUR_STEPS = R._case("w4", "int4", R.BF16, "B", 32, 65, 520, 512, (128, 64, 2, 1, 4))
G64_KS1 = R._case("w4", "int4", R.BF16, "B", 64, 130, 264, 576, (128, 64, 1, 1, 9))
SPLIT8 = next(c for c in R.cases(CUS) if c.want == (128, 64, 2, 8, 4))
W8 = _probe((128, 64, 1, 1, 5), kind="w8")
WIDE_CUS = 4    # (a 2 x 3 launch of the 128 x 128 tile for a twin that plans for 4 CUs)
WIDE_G256 = R._case("w4", "any4_global", R.BF16, "B", 256, 130, 264, 768, (128, 128, 1, 1, 12))


def _select(c, cus=CUS):
    return lambda twin, oracle: R.check_select(twin, c, cus)


def _onehot(c, cus=CUS):
    return lambda twin, oracle: R.check_onehot(twin, oracle, c, cus)


def _f64(c):
    return lambda twin, oracle: R.check_f64(twin, oracle, c, CUS)


def _bias(c):
    def run(twin, oracle):
        P = R.problem(c)
        R.check_bias(twin, P, R.Twin(CUS)(P), R.case_id(c))
    return run


# mutant -> (the check that must fail, a check of the same kind outside the mutant's regime that must pass, or None)
PROOFS = {
    "stale_ring_slot": (_select(KS1_9_STEPS), _select(FOUR_STEPS)),
    "last_step_dropped": (_select(KS1_9_STEPS), None),
    "tables_overwritten_early": (_onehot(WIDE_G256, WIDE_CUS), None),
    "sub_groups_swapped": (_onehot(KS1_9_STEPS), _onehot(G64_KS1)),
    "split_scales_from_group_0": (_onehot(KS2_SPLIT), _onehot(KS1_9_STEPS)),
    "swizzle_without_row_term": (_select(KS1_9_STEPS), None),
    "last_row_duplicated": (lambda twin, oracle: R.check_placement(twin, R.placement_cases(CUS)[0], CUS), None),
    "ragged_tile_previous_words": (_select(KS1_9_STEPS), _select(KS1_SPLIT_W16)),
    "partials_in_16_bit": (_f64(SPLIT8), _f64(G64_KS1)),
    "bias_once_per_split": (_bias(SPLIT8), _bias(G64_KS1)),
    "truncation": (_f64(G64_KS1), None),
    "int8_bytes_in_k_order": (_select(W8), _select(KS1_9_STEPS)),
}


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutant_fails_the_check_named_for_it(oracle, mutant):
    what, check, where = R.MUTANTS[mutant]
    must_fail, must_pass = PROOFS[mutant]
    cus = WIDE_CUS if mutant == "tables_overwritten_early" else CUS
    assert _fails(lambda: must_fail(R.Twin(cus), oracle)) is None, "the clean twin fails the proof's own case"
    why = _fails(lambda: must_fail(R.Twin(cus, mutant), oracle))
    assert why is not None, f"{mutant} ({what}) passes the {check} check"
    if must_pass is not None:
        assert _fails(lambda: must_pass(R.Twin(cus, mutant), oracle)) is None, f"{mutant} shows outside its regime ({where})"
    CAUGHT[mutant] = f"{what}: fails {check} ({why})" + (f"; passes outside '{where}'" if must_pass is not None else "")


def test_what_the_earlier_shapes_let_through(oracle):
    """What the tile GEMM's tests could see before this suite: random data under the contract (and the fused bias's bits) at every earlier
    case -- the 11 4-bit shapes at four flavours, the mx4 and int8 shapes, the 128-row call with and without a workspace.  No earlier case
    has four steps per group, so none can notice tables written early.  A stale ring slot is let through by exactly the cases of at most
    four steps per workgroup; the earlier cases of 8 steps ((256, 2056, 2048), mx4 (100, 4096, 4096), int8 at g = 64) and the 32-step
    launch without a workspace catch it -- but none of them has a remainder of the ring (steps mod 4 != 0), and none runs 128 x 128.
    (Without $TILE_F64_REPORT_CPU only these two mutants run; with it the whole table goes to the report.)"""
    full = bool(os.environ.get("TILE_F64_REPORT_CPU"))
    rows = R.old_shape_survivors(oracle, None if full else ["stale_ring_slot", "tables_overwritten_early"])
    SURVIVORS.update(rows)
    assert all(spg < 4 and ok for _, _, spg, ok in rows["tables_overwritten_early"]), rows["tables_overwritten_early"]
    assert all(ok == (ksteps <= 4) for _, ksteps, _, ok in rows["stale_ring_slot"]), rows["stale_ring_slot"]
    assert {ksteps for _, ksteps, _, _ in rows["stale_ring_slot"]} == {1, 3, 4, 8, 32}
