"""Gradients of scales, zeros and LUT of the 4-bit GEMMs, host side (no GPU): the C ABI of tg_gemm_w4_dq, the op registrations and the
opt-in switch."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DQ_OPS = {
    "tinygemm_y_f16RM_x_f16RM_w_int4TC": "tinygemm_dq_f16RM_x_f16RM_w_int4TC",
    "tinygemm_y_f16RM_x_f16RM_w_any4TC": "tinygemm_dq_f16RM_x_f16RM_w_any4TC",
}
E_NULL, E_QTYPE, E_SHAPE = -1, -6, -7   # the TG_E_* codes of include/tinygemm_hip.h


def test_dq_symbols_exported_declared_and_abi_unchanged():
    from any4_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "tinygemm_hip.h")).read()
    for sym in ("tg_gemm_w4_dq", "tg_gemm_w4_dq_workspace_bytes"):
        assert re.search(r"TG_API\s+[\w\s\*]+?\b" + sym + r"\s*\(", hdr), f"{sym} not declared with TG_API"
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym), f"{sym} not exported"
        assert sym in _lib.SYMBOLS
    assert _lib.load().tg_gemm_w4_dq_workspace_bytes.restype is ctypes.c_int64
    assert _lib.load().tg_abi_version() == _lib.TG_ABI_VERSION == 10


def _args(**kw):
    """A valid right-side forward call with aligned dummy pointers (never dereferenced: nothing here reaches a launch)."""
    from any4_amd import _lib

    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 63) & ~63
    a = dict(x=p, w=p, qinfo=p, lut=None, y=None, m=16, wrows=4096, k=4096, group=128, qtype=_lib.TG_Q_INT4, dtype=_lib.TG_BF16,
             w_on_right=1, inner_k_tiles=4, batch=1)
    a.update(kw)
    return _lib.W4Gemm(**a), buf, p


def _ws(**kw):
    from any4_amd import _lib

    args, _buf, _p = _args(**kw)
    return _lib.load().tg_gemm_w4_dq_workspace_bytes(ctypes.byref(args))


def test_dq_workspace_bytes_of_valid_problems():
    from any4_amd import _lib

    # H [k / g][wrows][16] f32; `y` is not read
    assert _ws() == (4096 // 128) * 4096 * 16 * 4
    assert _ws(m=8192) == _ws()                  # no split over m: the bytes do not depend on it
    assert _ws(group=32) == (4096 // 32) * 4096 * 16 * 4
    assert _ws(group=256) == _ws(group=128)      # a group wider than the kernel's 128-column tile: its two halves
    p = _args()[2]
    assert _ws(qtype=_lib.TG_Q_ANY4_ROWWISE, lut=p) == _ws()
    assert _ws(qtype=_lib.TG_Q_ANY4_GLOBAL, lut=p) == _ws() + 4096 * 16 * 4   # ... and the per-row table gradients the row sum reads
    assert _ws(w_on_right=0, w_format=_lib.TG_WFMT_ROWS) > 0
    assert _ws(qtype=_lib.TG_Q_ANY4_ROWWISE) == E_NULL   # a pointer one needs: the any4 LUT


@pytest.mark.parametrize("case", ["mx4", "aint4", "batch", "bias", "norm", "epilogue", "tc_x", "tc_y"])
def test_dq_refusals_without_gpu(case):
    from any4_amd import _lib

    args, _buf, p = _args()
    expect = {"mx4": E_QTYPE, "aint4": _lib.TG_E_LAYOUT, "batch": E_SHAPE, "bias": _lib.TG_E_FUSION, "norm": _lib.TG_E_FUSION,
              "epilogue": _lib.TG_E_FUSION, "tc_x": _lib.TG_E_LAYOUT, "tc_y": _lib.TG_E_LAYOUT}[case]
    if case == "mx4":
        args.qtype, args.group = _lib.TG_Q_MX4, 32
    elif case == "aint4":
        args.w_on_right, args.w_format = 0, _lib.TG_WFMT_M16N8K16
    elif case == "batch":
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
    L = _lib.load()
    assert L.tg_gemm_w4_dq_workspace_bytes(ctypes.byref(args)) == expect
    # the launching entry point validates identically before any HIP call (device -1: none is selected)
    assert L.tg_gemm_w4_dq(ctypes.byref(args), p, p, p, -1, None) == expect


def test_dq_outputs_and_workspace_checked_before_any_launch():
    from any4_amd import _lib

    L = _lib.load()
    args, _buf, p = _args()
    need = L.tg_gemm_w4_dq_workspace_bytes(ctypes.byref(args))
    args.workspace, args.workspace_bytes = p, need
    assert L.tg_gemm_w4_dq(ctypes.byref(args), p, None, None, -1, None) == E_NULL    # both outputs NULL
    assert L.tg_gemm_w4_dq(ctypes.byref(args), p, None, p, -1, None) == E_NULL       # int4 has no LUT: d_lut is ignored
    assert L.tg_gemm_w4_dq(ctypes.byref(args), None, p, None, -1, None) == E_NULL    # no dY
    assert L.tg_gemm_w4_dq(ctypes.byref(args), p + 2, p, None, -1, None) == -8       # TG_E_ALIGN
    args.workspace_bytes = need - 1
    assert L.tg_gemm_w4_dq(ctypes.byref(args), p, p, None, -1, None) == E_SHAPE      # too small a workspace
    args.workspace, args.workspace_bytes = None, 0
    assert L.tg_gemm_w4_dq(ctypes.byref(args), p, p, None, -1, None) == E_NULL       # none at all: it is required


def test_dq_ops_registered_without_autograd_keys():
    import tinygemm  # noqa: F401
    from any4_amd import ops

    assert ops.QGRAD_OPS == DQ_OPS
    assert set(ops.AUTOGRAD_OPS) == set(DQ_OPS) | {"tinygemm_y_f16RM_x_f16RM_w_mx4TC"}
    assert not set(DQ_OPS.values()) & (set(ops.AUTOGRAD_OPS) | set(ops.AUTOGRAD_OPS.values()))
    for name in DQ_OPS.values():
        assert name in ops.SCHEMAS and hasattr(torch.ops.tinygemm, name)
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"tinygemm::{name}", "Autograd")
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"tinygemm::{name}", "CUDA")
    assert str(torch.ops.tinygemm.tinygemm_dq_f16RM_x_f16RM_w_any4TC.default._schema).endswith("-> (Tensor, Tensor)")


def test_dq_ops_keep_cpu_tensors_failing():
    import tinygemm  # noqa: F401

    x, dy = torch.zeros(1, 64).bfloat16(), torch.zeros(1, 8).bfloat16()
    w, q = torch.zeros(1, 1, 32, 2, dtype=torch.int32), torch.zeros(2, 8, 2).bfloat16()
    with pytest.raises(NotImplementedError):
        torch.ops.tinygemm.tinygemm_dq_f16RM_x_f16RM_w_int4TC(x, dy, w, 32, q, True)
    with pytest.raises(NotImplementedError):
        torch.ops.tinygemm.tinygemm_dq_f16RM_x_f16RM_w_any4TC(x, dy, w, 32, q, torch.zeros(8, 16).bfloat16(), True)


def test_quant_param_grad_switch_defaults_off_and_restores():
    import any4_amd

    assert any4_amd.get_quant_param_grad() is False
    with any4_amd.quant_param_grad():
        assert any4_amd.get_quant_param_grad() is True
        with any4_amd.quant_param_grad(False):
            assert any4_amd.get_quant_param_grad() is False
        assert any4_amd.get_quant_param_grad() is True
    assert any4_amd.get_quant_param_grad() is False
    with pytest.raises(ZeroDivisionError):
        with any4_amd.quant_param_grad():
            1 / 0
    assert any4_amd.get_quant_param_grad() is False
    any4_amd.set_quant_param_grad(True)
    try:
        assert any4_amd.get_quant_param_grad() is True
        with any4_amd.quant_param_grad(False):
            assert any4_amd.get_quant_param_grad() is False
    finally:
        any4_amd.set_quant_param_grad(False)
    assert any4_amd.get_quant_param_grad() is False


def test_modules_name_their_dq_ops():
    import modules

    assert modules.Int4Linear._DQ_OP == DQ_OPS["tinygemm_y_f16RM_x_f16RM_w_int4TC"]
    assert modules.Any4Linear._DQ_OP == modules.NF4Linear._DQ_OP == DQ_OPS["tinygemm_y_f16RM_x_f16RM_w_any4TC"]
    assert modules.MX4Linear._DQ_OP is None and modules.Int8Linear._DQ_OP is None


def test_tune_quant_params_refuses_what_it_cannot_tune():
    import modules
    from any4_amd.quantize import tune_quant_params

    x = torch.zeros(2, 64)
    with pytest.raises(ValueError, match="packed int4 / any4"):
        tune_quant_params(modules.MX4Linear(64, 16, bias=False), x, torch.zeros(2, 16))
    with pytest.raises(ValueError, match="packed int4 / any4"):
        tune_quant_params(modules.Int4Linear(64, 16, bias=False, group_size=32), x, torch.zeros(2, 16))   # not packed yet


# ------------------------------------------------------------------------------------------------
# the tile and step counts tests/grad_ref.DQ_CASES claims
# ------------------------------------------------------------------------------------------------

def _dq_cases():
    from tests import grad_ref

    return grad_ref.DQ_CASES, grad_ref.dq_case_id


@pytest.mark.parametrize("case", _dq_cases()[0], ids=_dq_cases()[1])
def test_dq_cases_reach_the_tiles_and_steps_they_claim(case):
    from tests import grad_ref as G

    c = case
    assert c.tiles == (G.cdiv(c.wrows, G.DQ_BR), G.cdiv(c.k, G.DQ_BK))
    assert c.steps == G.cdiv(c.m, G.DQ_BA)
    assert c.k % c.g == 0 and c.k % 32 == 0 and c.wrows % (8 if c.on_right else 16) == 0
    # the library accepts the problem and sizes H for it: [k / min(g, 128)][wrows][16] f32 (+ the per-row tables of a global LUT)
    need = (c.k // min(c.g, 128)) * c.wrows * 16 * 4 + (c.wrows * 16 * 4 if c.qtype == "any4_global" else 0)
    assert G.dq_workspace_bytes(c.m, c.wrows, c.k, c.g, c.qtype, c.dtype, c.on_right, c.inner) == need


def test_dq_cases_cover_what_they_are_for():
    from tests import grad_ref as G

    C = G.DQ_CASES
    assert {c.m for c in C} >= {63, 64, 65, 129}
    assert {c.dtype for c in C} == {G.BF16, G.F16} and {c.on_right for c in C} == {True, False}
    for k, g, tiles_k in ((160, 32, 2), (416, 32, 4), (768, 256, 6)):
        hit = [c for c in C if (c.k, c.g) == (k, g)]
        assert hit and all(c.tiles[1] == tiles_k for c in hit) and {c.on_right for c in hit} == {True, False}, k
    assert 160 % 128 == 32 and 416 % 128 == 32                      # the ragged last k tile is 32 columns wide
    assert any(c.wrows == 264 and c.tiles[0] == 3 for c in C) and 264 - 2 * G.DQ_BR == 8
    rs = [c for c in C if c.qtype == "any4_global" and c.wrows == 2056]
    assert rs and all(c.tiles[0] == 17 for c in rs) and 2056 % 16 != 0   # dq_rowsum_kernel: 16 chains of unequal length
    n = G.DQ_NONFINITE
    assert n["r0"] == n["wrows"] - 1 and n["wrows"] % G.DQ_BR != 0 and n["a0"] == n["m"] - 1 == G.DQ_BA
    assert n["j0"] == n["k"] - 1 and n["k"] % G.DQ_BK == 32
