"""tg_gemm_mx4a8_rows without a GPU: the symbols are declared, exported and bound (ABI 10), every refusal of the entry point comes before any
HIP call (tg_gemm_mx4a8's, then m > 64 and the workspace), the workspace and grid rules, and the Python refusals."""
import ctypes
import os

import pytest
import torch

from any4_amd import _lib, modules, ops
from tests.test_mx4a8_cpu import _P, _args

W = 4096


def test_symbols_abi_workspace_and_grid_rules():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tinygemm_hip.h")) as f:
        header = f.read()
    L, out = _lib.load(), (ctypes.c_int64 * 4)()
    assert L.tg_abi_version() == _lib.TG_ABI_VERSION == 10 and L.tg_gemm_mx4a8_rows_workspace_bytes.restype is ctypes.c_int64
    for n in ("tg_gemm_mx4a8_rows", "tg_gemm_mx4a8_rows_workspace_bytes", "tg_gemm_mx4a8_rows_plan"):
        assert f" {n}(" in header and n in _lib.SYMBOLS and getattr(L, n).argtypes == _lib.SYMBOLS[n]
    assert L.tg_gemm_mx4a8_rows_workspace_bytes(64, 14336, W) == 0 and L.tg_gemm_mx4a8_rows_workspace_bytes(1, 16, 128) == 0
    assert L.tg_gemm_mx4a8_rows_workspace_bytes(17, 4096, 14336) == 2 * 256 * 4 + 2 * 256 * 4 * 1024   # counters + 1 KiB per (block, tile, window)
    assert [L.tg_gemm_mx4a8_rows_workspace_bytes(*a) for a in ((65, 16, 128), (1, 16, 64), (0, 16, 128), (1, 12, 128), (1, 8, 1 << 28))] == [-7, -3, -7, -7, -10]
    assert L.tg_gemm_mx4a8_rows_plan(17, 4096, 14336, out) == 0 and list(out) == [256, 2, 4, W]
    assert L.tg_gemm_mx4a8_rows_plan(3, 14336, 128, out) == 0 and list(out) == [448, 1, 1, W]   # 896 tiles: two per workgroup
    assert L.tg_gemm_mx4a8_rows_plan(65, 16, 128, out) == -7 and L.tg_gemm_mx4a8_rows_plan(1, 16, 128, None) == -1


@pytest.mark.parametrize("kw,ws,ws_bytes,code", [
    (dict(x_codes=None), None, 0, -1), (dict(w=_P + 8), None, 0, -8), (dict(k=576), None, 0, -3), (dict(inner_k_tiles=2), None, 0, -2),
    (dict(w_on_right=0, w_format=_lib.TG_WFMT_M16N8K16), None, 0, _lib.TG_E_LAYOUT), (dict(reserved=1), None, 0, _lib.TG_E_STRUCT),
    (dict(wrows=1 << 22, k=1024), None, 0, -10), (dict(wrows=260), None, 0, -7), (dict(m=0), None, 0, -7),
    (dict(m=65), None, 0, -7), (dict(m=65, k=2 * W), _P, 1 << 30, -7),
    (dict(k=W + 128), None, 1 << 30, -1), (dict(k=W + 128), _P + 8, 1 << 30, -8), (dict(k=W + 128), _P, -1, -8), (dict(k=W + 128), _P, None, -7),
])
def test_refusals(kw, ws, ws_bytes, code):
    L = _lib.load()
    if ws_bytes is None:   # one byte short of what the call asks for
        ws_bytes = L.tg_gemm_mx4a8_rows_workspace_bytes(64, 256, kw["k"]) - 1
    assert L.tg_gemm_mx4a8_rows(ctypes.byref(_args(**kw)), ws, ws_bytes, 0, None) == code


def test_python_refusals():
    x = torch.zeros(65, 128, dtype=torch.bfloat16)
    w, e = torch.zeros(2, 2, 32, 2, dtype=torch.int32), torch.zeros(16, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at most 64"):
        ops.gemm_mx4_a8(x, w, e, True, kernel="rows")
    with pytest.raises(ValueError, match="kernel must be"):
        ops.gemm_mx4_a8(x, w, e, True, kernel="split")
    with pytest.raises(ValueError, match="small_batch"):
        modules.MX4Linear(256, 32, bias=False, dtype=torch.bfloat16, small_batch=True)
    assert modules.MX4Linear(256, 32, bias=False, dtype=torch.bfloat16, activations="mx8").small_batch is False
