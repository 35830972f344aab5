"""CPU suite: the checks of tests/w16_ref.py proven without a GPU.  A plain-torch twin of each kernel (f32 accumulation, one RNE
rounding) passes every check at the shapes the GPU file runs; each mutant -- one way in which f16_gemm_kernel / w8_gemm_kernel could be
subtly wrong -- fails at least the check named for it.  The case tables are checked against the loop and launch arithmetic they claim
to reach.  $W16_F64_REPORT_CPU names a file for the twins' figures and the mutant table (profiles/w16_f64_checks.txt)."""
import os

import pytest

from tests import w16_ref as R

CPU = "cpu"
RESULTS = []   # (case id, the twin's worst ratio)
CAUGHT = {}    # mutant -> [(check, detail)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("W16_F64_REPORT_CPU")
    if path:
        with open(path, "w") as f:
            for cid, ratio in RESULTS:
                f.write(f"twin {cid:50s} {ratio:.3f}\n")
            for mutant, rows in CAUGHT.items():
                f.write(f"mutant {mutant}: " + "; ".join(f"{name} ({detail})" if detail else name for name, detail in rows) + "\n")


def _pad(side):
    return 8 if side == "B" else 16


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables reach what they claim
# ---------------------------------------------------------------------------------------------------------------------------------

def test_f16_table_reaches_every_loop_regime():
    ks = [s[0] for s in R.F16_SHAPES]
    nws = {k: [R.nw_f16(k, v) for v in range(8)] for k in ks}
    assert nws[32] == [1, 0, 0, 0, 0, 0, 0, 0]
    assert any(len(set(nw)) > 1 and max(nw) < 4 for nw in nws.values())                   # ragged below one ring
    assert nws[1056] == [5, 4, 4, 4, 4, 4, 4, 4]                                             # refills inside the remainder
    assert nws[2048] == [8] * 8                                                              # exactly one steady round
    assert any(min(nw) >= 8 and len(set(nw)) > 1 for nw in nws.values())                     # steady loop, ragged waves
    assert nws[4096] == [16] * 8 and nws[14336] == [56] * 8
    # steps left to the remainder rounds (nw < 8: nw; else 4 + nw % 4): every count the unrolled remainder can see
    rem = {nw if nw < 8 else 4 + nw % 4 for v in nws.values() for nw in v}
    assert rem == set(range(8))
    steady = [c for c in R.F16_CASES if c.k >= R.STEADY_K]
    for dt in (R.BF16, R.F16):
        mine = [c for c in steady if c.dtype == dt]
        assert {c.m for c in mine} >= {1, 5, 16, 17, 33}
        assert {c.n for c in mine if c.side == "B"} >= {8, 24, 48, 136} and {c.n for c in mine if c.side == "A"} >= {16, 48}
        for side, inner in R.F16_LAYOUTS:
            assert {c.k for c in R.F16_CASES if c.dtype == dt and (c.side, c.inner) == (side, inner)} >= set(ks)


def test_w8_table_against_launch_w8():
    for c in R.W8_CASES:
        wrows = -(-c.n // _pad(c.side)) * _pad(c.side)
        sk, tiles, tpb, wgs = R.w8_split(c.m, wrows, c.k)
        assert sk == c.split, (R.w8_id(c), sk)
        assert c.m <= 16 and c.k % 32 == 0 and (c.k // 16) % c.inner == 0
        if c.n >= R.LARGE_N:
            assert tiles % tpb == 1 and wgs == 513, R.w8_id(c)                               # a ragged last workgroup with one row tile
            rows = R.sample_rows(c.n, c.split)
            assert set(range(c.n - 24, c.n)) <= set(rows.tolist()) and rows[0] == 0 and len(rows) <= 600
    assert {c.split for c in R.W8_CASES} == {1, 2, 4, 8}
    assert any((c.k // 16) % 4 for c in R.W8_CASES if c.split == 8)                          # the clamped half step
    nsteps = 4160 // 64
    assert [(nsteps - s + 7) // 8 for s in range(8)] == [9, 8, 8, 8, 8, 8, 8, 8]
    for dt in (R.BF16, R.F16):
        assert {c.g for c in R.W8_CASES if c.dtype == dt} == {32, 128}


def test_selection_columns_hit_every_class():
    for n, k in ((1032, 2272), (1040, 2272), (136, 96), (65544, 256), (1032, 4160)):
        pi = R.selection_columns(n, k)
        assert len(pi) == n and len(set((pi % 1024).tolist())) == min(k, 1024)
        assert (pi < 32).any() and (pi >= k - 32).any()
    assert (R.selection_columns(1032, 2272) >= 1024).sum() > 200                            # the steady loop's later rounds too


@pytest.mark.parametrize("dtype", [R.BF16, R.F16])
def test_twin_dequant_is_the_oracles(oracle, dtype):
    for side in ("B", "A"):
        t = R.TwinW8(side)
        codes, _, sz = R.w8_inputs(1, 72, 256, 32, dtype, CPU, t.pad)
        assert R.bits_equal(t.dequant(codes, sz, 32), R.oracle_int8(oracle, codes, sz, 32, dtype))


# ---------------------------------------------------------------------------------------------------------------------------------
# the twins pass
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.F16_CASES, ids=R.f16_id)
def test_twin_f16_float64(c):
    R.check_f64_f16(R.TwinF16(_pad(c.side)), c, CPU, RESULTS)


@pytest.mark.parametrize("c", R.W8_CASES, ids=R.w8_id)
def test_twin_w8_float64(oracle, c):
    R.check_f64_w8(R.TwinW8(c.side), oracle, c, CPU, RESULTS)


def _battery_f16(gemm, dtype, f64=True):
    """(name, detail, thunk) of every CPU-runnable check of the 16-bit kernel at the GPU file's shapes, for one weight side."""
    side = "B" if gemm.pad == 8 else "A"
    n_sel = 1032 if side == "B" else 1040
    n_half = 136 if side == "B" else 48
    out = []
    if f64:
        for c in R.F16_CASES:
            if c.dtype == dtype and c.side == side and c.inner == 1:
                out.append(("float64 bound", R.f16_id(c), lambda c=c: R.check_f64_f16(gemm, c, CPU)))
    out += [("selection probe", f"m17-n{n_sel}-k2272", lambda: R.check_select_f16(gemm, 17, n_sel, 2272, dtype, CPU)),
            ("selection probe", f"m17-n{n_sel}-k4320", lambda: R.check_select_f16(gemm, 17, n_sel, 4320, dtype, CPU, seed=2)),
            ("selection probe", f"m5-n{136 if side == 'B' else 144}-k96", lambda: R.check_select_f16(gemm, 5, 136 if side == "B" else 144, 96, dtype, CPU)),
            ("one-hot probe", f"m33-n{n_half}-k2272", lambda: R.check_onehot_f16(gemm, 33, n_half, 2272, dtype, CPU)),
            ("decoy", f"m17-n{n_half}-k2080", lambda: R.check_decoy_f16(gemm, 17, n_half, 2080, dtype, CPU)),
            ("non-finite placement", f"m17-n{n_half}-k2080", lambda: R.check_nonfinite_f16(gemm, 17, n_half, 2080, dtype, CPU)),
            ("output guard", f"m17-n{n_half}-k2080", lambda: R.check_guard_f16(gemm, 17, n_half, 2080, dtype, CPU))]
    return out


def _battery_w8(gemm, oracle, dtype, side, f64=True):
    out = []
    if f64:
        for c in R.W8_CASES:
            if c.dtype == dtype and c.side == side and c.n < R.LARGE_N:
                out.append(("float64 bound", R.w8_id(c), lambda c=c: R.check_f64_w8(gemm, oracle, c, CPU)))
    out += [("selection probe", "m16-n1032-k4160-g32", lambda: R.check_select_w8(gemm, 16, 1032, 4160, 32, dtype, CPU)),
            ("selection probe", "m5-n2056-k256-g32", lambda: R.check_select_w8(gemm, 5, 2056, 256, 32, dtype, CPU)),
            ("one-hot probe", "m16-n72-k4160-g32", lambda: R.check_onehot_w8(gemm, oracle, 16, 72, 4160, 32, dtype, CPU)),
            ("decoy", "m5-n68-k4224-g128", lambda: R.check_decoy_w8(gemm, 5, 68, 4224, 128, dtype, CPU)),
            ("non-finite placement", "m16-n72-k4160-g32", lambda: R.check_nonfinite_w8(gemm, oracle, 16, 72, 4160, 32, dtype, CPU))]
    return out


@pytest.mark.parametrize("dtype", [R.BF16, R.F16], ids=R.dt_name)
@pytest.mark.parametrize("side", ["B", "A"])
def test_twin_f16_probes(side, dtype):
    for name, detail, thunk in _battery_f16(R.TwinF16(_pad(side)), dtype, f64=False):
        thunk()


@pytest.mark.parametrize("dtype", [R.BF16, R.F16], ids=R.dt_name)
@pytest.mark.parametrize("side", ["B", "A"])
def test_twin_w8_probes(oracle, side, dtype):
    for name, detail, thunk in _battery_w8(R.TwinW8(side), oracle, dtype, side, f64=False):
        thunk()


# ---------------------------------------------------------------------------------------------------------------------------------
# the mutants fail
# ---------------------------------------------------------------------------------------------------------------------------------

def _failing(battery):
    out = {}
    for name, detail, thunk in battery:
        try:
            thunk()
        except AssertionError:
            out.setdefault(name, []).append(detail)
    return out


# the check that must catch each mutant (others may as well: the table of the report lists all that did)
F16_MUST = {
    "last_step_dropped": ["float64 bound", "selection probe", "one-hot probe"],
    "last_step_twice": ["float64 bound", "selection probe", "one-hot probe"],
    "wrong_ring_slot": ["float64 bound", "selection probe"],
    "x_cols_swapped": ["float64 bound", "selection probe"],
    "half_tile_previous_rows": ["float64 bound", "selection probe"],
    "idle_wave_adds": ["float64 bound", "selection probe"],
    "row_m_unmasked": ["output guard"],
    "partials_in_16_bit": ["float64 bound"],
    "truncation": ["float64 bound"],
}
W8_MUST = {
    "zero_once_per_row": ["float64 bound", "one-hot probe"],
    "byte_order_as_k_order": ["float64 bound", "selection probe", "one-hot probe"],
    "last_step_dropped": ["float64 bound", "selection probe"],
    "truncation": ["float64 bound"],
}


@pytest.mark.parametrize("mutant", list(R.F16_MUTANTS))
def test_f16_mutant_is_caught(mutant):
    for dtype in (R.BF16, R.F16):
        failed = _failing(_battery_f16(R.TwinF16(8, mutant), dtype))      # wrows % 16 = 8 exists on the right only
        assert set(F16_MUST[mutant]) <= set(failed), (mutant, R.dt_name(dtype), sorted(failed))
        if mutant != "half_tile_previous_rows":
            left = _failing(_battery_f16(R.TwinF16(16, mutant), dtype))
            assert set(F16_MUST[mutant]) <= set(left), (mutant, "left", R.dt_name(dtype), sorted(left))
        if dtype == R.BF16:
            CAUGHT[R.F16_MUTANTS[mutant]] = [(name, f"{len(d)} of {sum(1 for b in _battery_f16(R.TwinF16(8), dtype) if b[0] == name)} shapes")
                                             for name, d in failed.items()]
    if mutant == "wrong_ring_slot":   # only a steady-loop k can see it
        assert all(int(d.split("-k")[1].split("-")[0]) >= R.STEADY_K for d in failed["float64 bound"])
    if mutant == "idle_wave_adds":    # only k < 256 has idle waves
        assert all(int(d.split("-k")[1].split("-")[0]) < 256 for d in failed["float64 bound"])


@pytest.mark.parametrize("mutant", list(R.W8_MUTANTS))
def test_w8_mutant_is_caught(oracle, mutant):
    for side in ("B", "A"):
        for dtype in (R.BF16, R.F16):
            failed = _failing(_battery_w8(R.TwinW8(side, mutant), oracle, dtype, side))
            assert set(W8_MUST[mutant]) <= set(failed), (mutant, side, R.dt_name(dtype), sorted(failed))
            if side == "B" and dtype == R.BF16:
                CAUGHT[R.W8_MUTANTS[mutant]] = [(name, f"{len(d)} of {sum(1 for b in _battery_w8(R.TwinW8(side), oracle, dtype, side) if b[0] == name)} shapes")
                                                for name, d in failed.items()]
