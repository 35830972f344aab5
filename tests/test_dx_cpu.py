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
    assert _lib.load().tg_abi_version() == _lib.TG_ABI_VERSION == 9


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
