"""CPU suite: tests/pair_ref.py -- the restated plan of the persistent pair-table family against the library's own answers (host-only
planner calls, as tests/test_host_cpu.py makes them), its references against the oracle, the regimes of tests/test_gpu_pair_f64.py's cases,
the plain-torch twin of the schedule on every one of those cases, every mutant of the twin against the check named for it, and the same
mutants under what tests/test_gpu_fast.py checks (the gap table of DESIGN.md section 4).  No GPU."""
import numpy as np
import pytest
import torch

from tests import pair_ref as R
from tests.conftest import bits16, from_bits16

BF16, F16 = torch.bfloat16, torch.float16


def test_constants_come_from_the_sources():
    C = R.constants()
    assert (C.TG_PAIR_WGS, C.TG_PAIR_MIN_ITEMS, C.TG_XG_CHUNK, C.TG_B16_CHUNK, C.TG_PAIR_R, C.LDS_LINE) == (512, 192, 4, 4, 2, 80 * 1024)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------

def _agrees(pp, fam, det, ws):
    from any4_amd import _lib

    if pp.family == "pair":
        return fam == _lib.TG_PLAN_PAIR and (det == _lib.TG_PLAN_PAIR_M1_LEAN) == (pp.kernel == "lean") and ws == pp.ws
    if pp.family == "xr":
        return fam == det == _lib.TG_PLAN_PAIR_XR and ws == pp.ws
    # this family declined.  The planner names families, and w4_gemm_pair16_kernel answers TG_PLAN_PAIR too: what can be compared is that
    # the call is not the lean kernel's, not w4_gemm_xr_kernel's, and asks for no workspace (test_declined_* has the sharper case)
    return det != _lib.TG_PLAN_PAIR_M1_LEAN and fam != _lib.TG_PLAN_PAIR_XR and ws == 0


@pytest.mark.parametrize("on_right", [True, False])
def test_plan_is_the_librarys(on_right):
    """m 1 ... 16; k of 1 ... 30 units and 64 / 128 / 224; the four groups, three innerKTiles, four quantisation types; batches on both sides of
    192 and 384 items; a bias, both numerics settings of one row, with and without a workspace."""
    checked = pair = 0
    for inner in ((2, 4, 8) if on_right else (1, 2, 4)):
        for g in (32, 64, 128, 256):
            nsg = max(g // (16 * inner), 1)
            for units in (1, 2, 3, 5, 8, 9, 16, 17, 30, 64, 128, 224):
                k = units * nsg * 16 * inner
                if k % 32 or k % g or k > 16384:
                    continue
                for qtype in ("int4", "any4_global", "any4_rowwise", "mx4"):
                    for m in (1, 2, 4, 5, 8, 9, 16):
                        for wrows, batch in ((64, 191), (64, 192), (64, 383), (64, 384), (48, 400), (192, 173)):
                            for kw in (dict(), dict(bias=True), dict(numerics="fast_mfma"), dict(workspace=False)):
                                if (kw.get("numerics") or kw.get("bias")) and m != 1:
                                    continue
                                pp = R.pair_plan(m, wrows, k, g, qtype, inner, on_right, batch, BF16, **kw)
                                fam, det, ws = R.lib_plan(m, wrows, k, g, qtype, inner, on_right, batch, BF16, **kw)
                                if kw.get("workspace") is False:  # (the query's answer is what the fastest kernel WOULD take)
                                    assert ws == R.pair_plan(m, wrows, k, g, qtype, inner, on_right, batch, BF16).ws
                                    ws = pp.ws
                                assert _agrees(pp, fam, det, ws), (m, wrows, k, g, qtype, inner, batch, kw, pp)
                                checked += 1
                                pair += pp.family == "pair"
    assert checked > 10000 and pair > checked // 4, (checked, pair)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_plan_of_every_case_is_the_librarys(dtype):
    for name in R.CASE_NAMES:
        c = R.case(name)
        if c.qtype == "mx4" and dtype == F16:
            continue
        pp = R.pair_plan(c.m, c.n, c.k, c.g, c.qtype, c.inner, c.on_right, c.batch, dtype, c.numerics, True, bias=c.bias)
        assert pp.family == "pair" and _agrees(pp, *R.lib_plan(c.m, c.n, c.k, c.g, c.qtype, c.inner, c.on_right, c.batch, dtype, c.numerics, True, bias=c.bias)), name


def test_declined_instantiations_are_declined():
    """What launch_pair_m does not instantiate: pair_plan says so, and with more problems than w4_gemm_pair16_kernel's grid takes (65535)
    the library's answer is no pair-table kernel at all."""
    from any4_amd import _lib

    for m, g, qtype, inner in R.DECLINED:
        k = 16 * max(g, 128)
        assert R.pair_plan(m, 64, k, g, qtype, inner, True, 400).family == "other", (m, g, qtype, inner)
        fam, det, ws = R.lib_plan(m, 64, k, g, qtype, inner, True, 65536)
        assert fam not in (_lib.TG_PLAN_PAIR, _lib.TG_PLAN_PAIR_XR) and det == fam and ws == 0, (m, g, qtype, inner, fam)
    # ... while their instantiated neighbours are taken at that batch
    for m, g, qtype, inner in [(1, 256, "any4_rowwise", 8), (1, 128, "int4", 8), (2, 256, "any4_rowwise", 4)]:
        assert R.lib_plan(m, 64, 8 * g, g, qtype, inner, True, 65536)[0] == _lib.TG_PLAN_PAIR


def test_native_rows_words_take_the_b_side_plan():
    """A weights-on-the-left call with tg_w4_gemm.w_format = TG_WFMT_ROWS is a weights-on-the-right call from make_params on (innerKTiles 4 where
    k % 64 == 0, else 2): the planner's three answers equal the B-side call's, the lean kernel included; the reference's Aint4 words take LA = 1."""
    from any4_amd import _lib

    for m, wrows, k, g, qtype, batch in [(1, 192, 1152, 128, "any4_rowwise", 173), (1, 64, 576, 64, "int4", 300), (3, 48, 576, 64, "any4_global", 400),
                                          (8, 64, 1024, 128, "any4_rowwise", 200), (13, 48, 1152, 128, "int4", 300), (2, 48, 288, 32, "mx4", 400)]:
        inner = 4 if k % 64 == 0 else 2
        rows = R.lib_plan(m, wrows, k, g, qtype, 2, False, batch, w_format=_lib.TG_WFMT_ROWS)
        assert rows == R.lib_plan(m, wrows, k, g, qtype, inner, True, batch), (m, wrows, k, g, qtype)
    assert R.lib_plan(1, 192, 1152, 128, "any4_rowwise", 2, False, 173, w_format=_lib.TG_WFMT_ROWS)[1] == _lib.TG_PLAN_PAIR_M1_LEAN
    assert R.pair_plan(1, 192, 1152, 128, "any4_rowwise", 4, False, 173).kernel == "la1"


def test_smallest_xg_k_is_the_first_k_with_a_workspace():
    for m in (1, 8):
        k = R.smallest_xg_k(m)
        assert R.lib_plan(m, 64, k, 128, "any4_rowwise", 4, True, 200)[2] > 0 and R.lib_plan(m, 64, k - 128, 128, "any4_rowwise", 4, True, 200)[2] == 0


def test_cases_reach_every_regime():
    seen = R.assert_regimes_reached([R.case_plan(name) for name in R.CASE_NAMES])
    assert not ({r for r in seen if r.startswith("kernel:")} - R.REQUIRED)
    # a case list without its partial slices: the assertion notices
    with pytest.raises(AssertionError, match="partial"):
        R.assert_regimes_reached([pp for pp in map(R.case_plan, R.CASE_NAMES) if "slice:partial+empty" not in R.regimes(pp)])


def test_item_walks_cover_every_item_once():
    for name in R.CASE_NAMES:
        pp = R.case_plan(name)
        assert (R.walk_writes(pp) == 1).all(), name
        got = sorted(it for wg in range(pp.workgroups) for it in pp.wg_items(wg))
        assert got == list(range(pp.items)), name


# ---- the references ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("qtype,g,dtype", [("int4", 64, BF16), ("any4_global", 128, F16), ("any4_rowwise", 32, BF16), ("any4_rowwise", 256, F16), ("mx4", 32, BF16)])
def test_references_are_the_oracles(oracle, qtype, g, dtype):
    """y64 is oracle.linear_group_scaled's sum before its conversion to f32; the weights behind S are oracle.dequant's bits."""
    bt = R.make_batch(3, 24, 512, g, qtype, 3, dtype, seed=4)
    y64, S = R.ref64(bt)
    q = {"int4": oracle.Q_INT4, "any4_global": oracle.Q_ANY4_GLOBAL, "any4_rowwise": oracle.Q_ANY4_ROWWISE, "mx4": oracle.Q_MX4}[qtype]
    dt = oracle.BF16 if dtype == BF16 else oracle.F16
    for b in range(bt.B):
        qi = bt.exps[b].numpy() if qtype == "mx4" else bits16(torch.stack([bt.scale[b], bt.zero[b]], dim=2))
        lb = None if bt.lut is None else bits16(bt.lut[b])
        _, y32 = oracle.linear_group_scaled(bits16(bt.x[b]), bt.codes[b].int().numpy(), g, q, qi, lb, dt)
        assert np.abs(y64[b] - y32.astype(np.float64)).max() <= 2.0 ** -24 * np.abs(y64[b]).max() + 1e-12 * S[b].max()
        w16 = oracle.dequant(bt.codes[b].int().numpy(), g, q, qi, lb, dt)
        # (as numbers: mx4's code 8 is -0, which the float64 form's "+ zero" turns into +0)
        assert torch.equal(R.weights16(R.weights64(bt, b, b + 1)[0], dtype).float(), from_bits16(w16, dtype).float())
        w = R.weights16(R.weights64(bt, b, b + 1)[0], dtype).double()
        assert np.allclose(S[b], (bt.x[b].double().abs() @ w.abs().t()).numpy(), rtol=1e-12)


# ---- the twin ----------------------------------------------------------------------------------------------------------------------

TWIN_RATIOS = {}


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_twin_is_within_the_bound_on_every_case(name):
    bt, pp = R.case_batch(name), R.case_plan(name)
    y64, S = R.ref64(bt)
    TWIN_RATIOS[name] = R.check_f64(R.twin(pp, bt), y64, S, bt.dtype, name)
    print(f"TWIN {name}: worst error / bound {TWIN_RATIOS[name]:.4f}")


@pytest.mark.parametrize("name", R.PROBE_CASES)
def test_twin_passes_the_exact_probes(name):
    bt, pp = R.case_batch(name), R.case_plan(name)
    probes = [R.probe_one_weight, R.probe_one_hot] + ([] if bt.qtype == "mx4" else [R.probe_zero_point])
    for probe in probes:
        pb, want = probe(pp, bt)
        R.assert_same_bits(R.twin(pp, pb), want, f"{name}: {probe.__name__}")


def test_probe_columns_cover_every_class():
    """wave, ring slot, both ends of every slice and group, every position of a super-tile (nibble, byte lane)."""
    name = "lean rowwise 9 units rblocks 3"
    bt, pp = R.case_batch(name), R.case_plan(name)
    pi = set(R.probe_columns(pp, bt).flatten().tolist())
    st = 16 * bt.inner
    for w in range(R.WAVES):
        if pp.nl[w]:
            assert {w * pp.spw * st, (w * pp.spw + pp.nl[w]) * st - 1} <= pi, w
    assert {0, bt.k - 1} <= pi and set(range(st, 2 * st)) <= pi and {gi * bt.g for gi in range(bt.k // bt.g)} <= pi


# which case shows each mutant (the check is pair_ref.MUTANTS'): the smallest case of the GPU file whose regime the bug needs
MUTANT_CASE = {
    "ring refill takes the current problem": "lean global fp16 ranges of 5-6",
    "global LUT kept across a problem boundary": "lean global fp16 ranges of 5-6",
    "row-wise LUT rows one row block late": "lean rowwise 9 units rblocks 3",
    "activations not restaged": "lean global fp16 ranges of 5-6",
    "partial slice runs its full spw": "lean rowwise 9 units rblocks 3",
    "empty wave adds its clamped load": "lean rowwise 9 units rblocks 3",
    "scale|zero word per super-tile": "lean rowwise 9 units rblocks 3",
    "activation sums indexed from slice 0": "lean rowwise 9 units rblocks 3",
    "zero point by both lane halves": "lean rowwise 9 units rblocks 3",
    "wave 7 dropped": "lean rowwise 6 rounds 192 items",
    "partials summed in 16 bits": "lean rowwise 6 rounds 192 items",
    "last item skipped, first written twice": "lean global fp16 ranges of 5-6",
    "chunked dealing steps by workgroups": "xg m8 chunked",
    "row block of the wrong operand": "lean rowwise 9 units rblocks 3",
    "truncation instead of RNE": "m1 g64",
    "LA activation sums of the item before": "walk la1 inner 4 m5",
}

# the message of each named check: a mutant counts as caught only by the check named for it, not by an assertion inside a probe's builder
CHECK_MESSAGE = {"f64": "outside the bound|differs from the float64 product", "all written": "all written: outputs still hold", "one weight": "one weight: \\d+ outputs differ",
                 "zero point": "zero point: \\d+ outputs differ", "written once": "stored more than once, or never"}


def run_check(check, pp, bt, run):
    """The checks of tests/test_gpu_pair_f64.py by name, on any `run(batch) -> y` -- but for "written once", which exists on the CPU only: it
    counts the stores of the twin's own walk.  A walk that stores an item twice stores the same bits twice, so no output shows it and a NaN
    prefill cannot count stores; on the GPU only the launch's time would.  A known limit of the GPU file."""
    if check in ("f64", "all written"):
        y64, S = R.ref64(bt)
        y = run(bt)
        assert not torch.isnan(y.float()).any() or bt.qtype == "mx4", "all written: outputs still hold the NaN prefill"
        if check == "f64":
            R.check_f64(y, y64, S, bt.dtype)
        return
    if check == "written once":
        assert (R.walk_writes(pp, bt.qtype, getattr(run, "mutant", None)) == 1).all(), "an item is stored more than once, or never"
        return
    probe = {"one weight": R.probe_one_weight, "zero point": R.probe_zero_point}[check]
    pb, want = probe(pp, bt)
    R.assert_same_bits(run(pb), want, check)


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_every_mutant_fails_the_check_named_for_it(mutant):
    name = MUTANT_CASE[mutant]
    bt, pp = R.case_batch(name), R.case_plan(name)
    run = lambda b: R.twin(pp, b, mutant)
    run.mutant = mutant
    with pytest.raises(AssertionError, match=CHECK_MESSAGE[R.MUTANTS[mutant]]):
        run_check(R.MUTANTS[mutant], pp, bt, run)


# ---- the same mutants under what tests/test_gpu_fast.py checks ------------------------------------------------------------------------

def _copies(m, n, k, g, qtype, inner, copies, seed):
    """run_fast's launch: one problem repeated."""
    one = R.make_batch(m, n, k, g, qtype, 1, BF16, seed=seed, inner=inner)
    bt = R.make_batch(m, n, k, g, qtype, 2, BF16, seed=seed, inner=inner)
    for f in ("codes", "x", "scale", "zero", "lut", "exps"):
        t = getattr(one, f)
        setattr(bt, f, None if t is None else t.expand(copies, *t.shape[1:]).contiguous())
    bt.B = copies
    return bt


def passes_run_fast(mutant):
    """run_fast + assert_fast_close on shapes of test_pair_kernel_vs_oracle (innerKTiles 4 and 2, g = 128 / 64 / 32): copy 0 against the
    reference, the middle and the last copy against copy 0 bit for bit, no NaN anywhere."""
    for (n, k, m), (qtype, g, inner) in [((64, 1024, 1), ("any4_rowwise", 128, 4)), ((40, 512, 3), ("any4_global", 64, 4)), ((136, 2048, 1), ("any4_global", 128, 4)),
                                          ((64, 1024, 1), ("any4_rowwise", 32, 2)), ((40, 512, 3), ("int4", 256, 4))]:
        copies = -(-384 // -(-n // 64))
        bt = _copies(m, n, k, g, qtype, inner, copies, seed=n + k + inner)
        pp = R.plan_of(bt)
        assert pp.family == "pair"
        y = R.twin(pp, bt, mutant)
        if torch.isnan(y.float()).any() or not (torch.equal(R.bits(y[0]), R.bits(y[-1])) and torch.equal(R.bits(y[0]), R.bits(y[copies // 2]))):
            return False
        one = _copies(m, n, k, g, qtype, inner, 1, seed=n + k + inner)
        y64, S = R.ref64(one)
        try:
            R.check_f64(y[:1], y64, S, BF16)
        except AssertionError:
            return False
    return True


def passes_stacked_samples(mutant):
    """test_persistent_workgroups_cross_problem_boundaries (700 problems of n = 192, k = 1024, a global LUT each, m = 1 and m = 3: problems
    0, 1, 2, 349, 350, 698, 699 compared, no NaN anywhere) and, for the dealing, test_workspace_variant_chunked_item_dealing (4200 problems,
    8 compared)."""
    shapes = [(1, 192, 1024, 128, "any4_global", 700, (0, 1, 2, 349, 350, 698, 699)), (3, 192, 1024, 128, "any4_global", 700, (0, 1, 2, 349, 350, 698, 699))]
    if mutant and "chunked" in mutant:
        shapes = [(8, 128, 1024, 128, "any4_rowwise", 4200, (0, 1, 2, 3, 2099, 2100, 4198, 4199))]
    on_right = True
    if mutant and mutant.startswith("LA "):  # (its weights-on-the-left case: int4, g = 64, m = 2 -- 4200 items of 32 rows, eight or nine per workgroup)
        shapes, on_right = [(2, 192, 1024, 64, "int4", 700, (0, 1, 2, 349, 350, 698, 699))], False
    for m, n, k, g, qtype, layers, sample in shapes:
        bt = R.make_batch(m, n, k, g, qtype, layers, BF16, seed=11, on_right=on_right)
        pp = R.plan_of(bt)
        y = R.twin(pp, bt, mutant)
        if torch.isnan(y.float()).any():
            return False
        for b in sample:
            y64, S = R.ref64(R.sub_batch(bt, b, b + 1))
            try:
                R.check_f64(y[b:b + 1], y64, S, BF16)
            except AssertionError:
                return False
    return True


def test_gap_table_of_todays_protocol():
    """Every mutant under run_fast's protocol -- the only tests that sweep the instantiation matrix -- and under the sampled problems of the
    stacked launches (lean / general kernel at innerKTiles 4, g = 128 only).  The table goes into DESIGN.md section 4."""
    table = {mutant: (passes_run_fast(mutant), passes_stacked_samples(mutant)) for mutant in R.MUTANTS}
    assert passes_run_fast(None) and passes_stacked_samples(None)
    for mutant, (a, b) in table.items():
        print(f"GAP {mutant:45s} run_fast: {'passes' if a else 'fails':6s}  stacked samples: {'passes' if b else 'fails'}")
    # identical copies hide the walk: what takes another problem's or another row block's data reads equal bytes
    for mutant in ("ring refill takes the current problem", "global LUT kept across a problem boundary", "row-wise LUT rows one row block late",
                   "activations not restaged", "partial slice runs its full spw"):
        assert table[mutant][0], mutant
    # ... and the arithmetic mutants are caught by both, so the protocol itself is sound
    for mutant in ("wave 7 dropped", "truncation instead of RNE", "zero point by both lane halves"):
        assert not table[mutant][0], mutant
