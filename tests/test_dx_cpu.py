"""Input gradient of the 4-bit GEMMs, host side (no GPU): the C ABI of tg_gemm_w4_dx and the Autograd registrations."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DX_OPS = {
    "tinygemm_y_f16RM_x_f16RM_w_int4TC": "tinygemm_dx_f16RM_dy_f16RM_w_int4TC",
    "tinygemm_y_f16RM_x_f16RM_w_any4TC": "tinygemm_dx_f16RM_dy_f16RM_w_any4TC",
    "tinygemm_y_f16RM_x_f16RM_w_mx4TC": "tinygemm_dx_f16RM_dy_f16RM_w_mx4TC",
}


def test_dx_symbols_exported_declared_and_abi_unchanged():
    from any4_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "tinygemm_hip.h")).read()
    for sym in ("tg_gemm_w4_dx", "tg_gemm_w4_dx_workspace_bytes"):
        assert re.search(r"TG_API\s+[\w\s\*]+?\b" + sym + r"\s*\(", hdr), f"{sym} not declared with TG_API"
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym), f"{sym} not exported"
        assert sym in _lib.SYMBOLS
    assert _lib.load().tg_gemm_w4_dx_workspace_bytes.restype is ctypes.c_int64
    assert _lib.load().tg_abi_version() == _lib.TG_ABI_VERSION == 10


def _args(**kw):
    """A valid right-side problem with aligned dummy pointers (never dereferenced: the size query needs no GPU)."""
    from any4_amd import _lib

    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 63) & ~63
    a = dict(x=p, w=p, qinfo=p, lut=None, y=p, m=16, wrows=4096, k=4096, group=128, qtype=_lib.TG_Q_INT4, dtype=_lib.TG_BF16,
             w_on_right=1, inner_k_tiles=4, batch=1)
    a.update(kw)
    return _lib.W4Gemm(**a), buf, p


def _ws(**kw):
    from any4_amd import _lib

    args, _buf, _p = _args(**kw)
    return _lib.load().tg_gemm_w4_dx_workspace_bytes(ctypes.byref(args))


def test_dx_workspace_bytes_of_valid_problems():
    from any4_amd import _lib

    # few (m x k) tiles: a split over the weight rows, f32 partials [splits][m][k]
    need = _ws()
    assert need > 0 and need % (16 * 4096 * 4) == 0
    # enough tiles to fill the chip: no split
    assert _ws(m=4096) == 0
    # the native weights-on-the-left format and mx4 are valid too
    assert _ws(w_on_right=0, w_format=_lib.TG_WFMT_ROWS, inner_k_tiles=4) >= 0
    assert _ws(qtype=_lib.TG_Q_MX4, group=32) >= 0
    # a pointer one needs: the any4 LUT
    assert _ws(qtype=_lib.TG_Q_ANY4_ROWWISE) == -1   # TG_E_NULL


@pytest.mark.parametrize("case", ["batch", "bias", "norm", "epilogue", "tc_x", "tc_y", "aint4", "mx4_f16", "null_x", "null_y", "null_w",
                                  "align_x", "align_y", "align_ws", "group", "inner", "k_div", "wrows"])
def test_dx_rejections_without_gpu(case):
    from any4_amd import _lib

    args, _buf, p = _args()
    # the TG_E_* codes of include/tinygemm_hip.h
    E_NULL, E_INNER_K, E_K_DIV, E_GROUP, E_DTYPE, E_SHAPE, E_ALIGN = -1, -2, -3, -4, -5, -7, -8
    expect = {
        "batch": E_SHAPE, "bias": _lib.TG_E_FUSION, "norm": _lib.TG_E_FUSION, "epilogue": _lib.TG_E_FUSION, "tc_x": _lib.TG_E_LAYOUT,
        "tc_y": _lib.TG_E_LAYOUT, "aint4": _lib.TG_E_LAYOUT, "mx4_f16": E_DTYPE, "null_x": E_NULL, "null_y": E_NULL, "null_w": E_NULL,
        "align_x": E_ALIGN, "align_y": E_ALIGN, "align_ws": E_ALIGN, "group": E_GROUP, "inner": E_INNER_K, "k_div": E_K_DIV, "wrows": E_SHAPE,
    }[case]
    if case == "batch":
        args.batch = 2
    elif case == "bias":
        args.bias = p
    elif case == "norm":
        args.norm_weight = p
    elif case == "epilogue":
        args.epilogue = _lib.TG_EPI_SWIGLU
    elif case == "tc_x":
        args.x_layout = _lib.TG_LAYOUT_TC_A
    elif case == "tc_y":
        args.y_layout = _lib.TG_LAYOUT_TC_A
    elif case == "aint4":
        args.w_on_right, args.w_format = 0, _lib.TG_WFMT_M16N8K16
    elif case == "mx4_f16":
        args.qtype, args.dtype, args.group = _lib.TG_Q_MX4, _lib.TG_F16, 32
    elif case == "null_x":
        args.x = None
    elif case == "null_y":
        args.y = None
    elif case == "null_w":
        args.w = None
    elif case == "align_x":
        args.x = p + 2
    elif case == "align_y":
        args.y = p + 8
    elif case == "align_ws":
        args.workspace, args.workspace_bytes = p + 4, 1 << 20
    elif case == "group":
        args.group = 96
    elif case == "inner":
        args.inner_k_tiles = 3
    elif case == "k_div":
        args.k = 4096 + 16
    elif case == "wrows":
        args.wrows = 4100
    L = _lib.load()
    assert L.tg_gemm_w4_dx_workspace_bytes(ctypes.byref(args)) == expect
    # the launching entry point validates identically before any HIP call (device -1: none is selected)
    assert L.tg_gemm_w4_dx(ctypes.byref(args), -1, None) == expect


def test_autograd_kernels_exactly_on_row_major_4bit_gemms():
    import tinygemm  # noqa: F401
    from any4_amd import ops

    has = {name for name in ops.SCHEMAS if torch._C._dispatch_has_kernel_for_dispatch_key(f"tinygemm::{name}", "Autograd")}
    assert has == set(DX_OPS)
    assert ops.AUTOGRAD_OPS == DX_OPS
    for dx in DX_OPS.values():
        assert hasattr(torch.ops.tinygemm, dx)


def test_autograd_registration_keeps_cpu_tensors_failing():
    import tinygemm  # noqa: F401

    x = torch.zeros(1, 64).bfloat16().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        torch.ops.tinygemm.tinygemm_y_f16RM_x_f16RM_w_int4TC(x, torch.zeros(1, 1, 32, 2, dtype=torch.int32), 32,
                                                            torch.zeros(2, 8, 2).bfloat16(), True)
    with pytest.raises(NotImplementedError):
        torch.ops.tinygemm.tinygemm_dx_f16RM_dy_f16RM_w_int4TC(torch.zeros(1, 8).bfloat16(), torch.zeros(1, 1, 32, 2, dtype=torch.int32), 32,
                                                               torch.zeros(2, 8, 2).bfloat16(), True)


def test_modules_route_row_major_4bit_kernels_only():
    import modules

    assert set(modules.Int4Linear._DX_KERNELS) == {"linear_y_f16RM_x_f16RM_W_int4TC", "linear_y_f16RM_W_int4TC_x_f16RM"}
    assert set(modules.Any4Linear._DX_KERNELS) == {"linear_y_f16RM_x_f16RM_W_any4TC", "linear_y_f16RM_W_any4TC_x_f16RM"}
    assert modules.NF4Linear._DX_KERNELS is modules.Any4Linear._DX_KERNELS
    assert set(modules.MX4Linear._DX_KERNELS) == {"linear_y_f16RM_x_f16RM_W_mx4TC", "linear_y_f16RM_W_mx4TC_x_f16RM"}
    assert modules.Int8Linear._DX_KERNELS == {}


# ------------------------------------------------------------------------------------------------
# the split regimes tests/grad_ref.DX_SPLIT_CASES claims, against the library's own answer
# ------------------------------------------------------------------------------------------------

def _dx_case_id(c):
    return f"m{c.m}-r{c.wrows}-k{c.k}"


def _dx_cases():
    from tests import grad_ref

    return grad_ref.DX_SPLIT_CASES


@pytest.mark.parametrize("case", _dx_cases(), ids=_dx_case_id)
def test_dx_split_cases_reach_the_regime_they_claim(case):
    from tests import grad_ref as G

    c = case
    # the library: every launch of the case splits as claimed (the split does not depend on weight kind, group, dtype, side or word order)
    assert c.runs
    for r in c.runs:
        wrows = c.wrows if r.on_right else c.wrows_left
        assert G.dx_splits(c.m, wrows, c.k, r.g, r.qtype, r.dtype, r.on_right, r.inner) == c.splits, r
    # plain arithmetic on the shape: tiles, steps, steps of every split, the ragged edges
    assert c.bm == (32 if c.m <= 32 else 64 if c.m <= 64 else 128)
    assert c.tiles == (G.cdiv(c.m, c.bm), G.cdiv(c.k, G.DX_BK))
    assert c.steps == G.cdiv(c.wrows, G.DX_BR)
    assert c.sps == G.cdiv(c.steps, c.splits)
    assert len(c.split_steps) == c.splits and sum(c.split_steps) == c.steps
    assert c.split_steps == G.split_steps(c.steps, c.splits)
    assert c.last_step_rows == c.wrows - (c.steps - 1) * G.DX_BR
    assert c.last_k_cols == c.k - (c.tiles[1] - 1) * G.DX_BK
    # weights on the left: rows padded to 16 -- the nearest such count with the same steps
    assert c.wrows_left % 16 == 0 and abs(c.wrows_left - c.wrows) <= 8 and G.cdiv(c.wrows_left, G.DX_BR) == c.steps
    assert c.wrows % 8 == 0 and c.k % 32 == 0


def test_dx_split_cases_cover_what_they_are_for():
    from tests import grad_ref as G

    by = {c.m: c for c in G.DX_SPLIT_CASES}
    assert [c.splits for c in G.DX_SPLIT_CASES] == [2, 4, 4, 8, 16]
    assert by[40].bm == 64 and by[40].last_step_rows == 8
    assert by[33].split_steps == (5, 5, 5, 2) and by[33].last_step_rows == 8
    assert by[130].tiles == (2, 17) and by[130].m - 128 == 2 and by[130].last_k_cols == 32 and by[130].split_steps[-1] == 6
    assert by[16].split_steps[6:] == (3, 0)
    assert by[7].split_steps[13:] == (0, 0, 0) and 0 not in by[7].split_steps[:13]
    # the tile limit, not the step limit, stops the m = 130 case: its steps alone would allow 8 splits
    assert G.dx_splits(16, by[130].wrows, 128) == 8
    runs = [r for c in G.DX_SPLIT_CASES for r in c.runs]
    assert {r.qtype for r in runs} == {"int4", "any4_global", "any4_rowwise", "mx4"}
    for q in ("int4", "any4_global", "any4_rowwise"):
        assert {r.dtype for r in runs if r.qtype == q} == {G.BF16, G.F16}, q
    assert all(r.dtype == G.BF16 and r.g == 32 for r in runs if r.qtype == "mx4")
    for c in G.DX_SPLIT_CASES:
        allowed = {i for i in (2, 4, 8) if c.k % (16 * i) == 0}
        assert {r.inner for r in c.runs if r.on_right} == allowed, c.k
        assert any(not r.on_right for r in c.runs)
        assert all(c.k % r.g == 0 for r in c.runs)


def test_dx_probe_shapes_run_the_regime_they_name():
    from tests import grad_ref as G

    for wrows, k, splits in (G.DX_IDENTITY_SMALL, G.DX_IDENTITY_LARGE):
        assert G.dx_splits(wrows, wrows, k) == splits
    wrows, k, _ = G.DX_IDENTITY_LARGE
    assert (G.cdiv(wrows, 128), G.cdiv(k, G.DX_BK), G.cdiv(wrows, G.DX_BR)) == (17, 2, 33)
    n = G.DX_NONFINITE
    assert G.dx_splits(n["m"], n["wrows"], n["k"]) == n["splits"] == 4
    assert n["row"] == n["m"] - 1 and 32 < n["m"] <= 64                    # BM = 64: tile rows 33 ... 63 are clamped copies of row 32
    assert (G.cdiv(n["wrows"], G.DX_BR) - 1) * G.DX_BR <= n["r0"] < n["wrows"]   # r0 in the ragged last step


@pytest.mark.parametrize("inner", [2, 4, 8])
def test_dx_inner_and_split_shapes_really_split(inner):
    """what test_gpu_dx.test_dx_inner_and_split says in its comment: with the workspace these launches split"""
    from tests import grad_ref as G

    for n, k, g, m, qtype, dtype, on_right, inn in G.dx_inner_and_split_shapes(inner):
        assert G.dx_splits(m, n, k, g, qtype, dtype, on_right, inn) == 8, (n, k)
