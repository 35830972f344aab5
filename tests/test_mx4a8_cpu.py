"""MX4 x MXFP8 without a GPU: the plain-torch layout and definition (utils.mx8_rows_ref, utils.mx4a8_ref), every refusal of
tg_gemm_mx4a8 / tg_quant_mx8_rows (validated before any HIP call) and the construction rules of MX4Linear(activations="mx8")."""
import ctypes

import pytest
import torch

from any4_amd import _lib, modules, utils
from any4_amd.kvcache import mx8_encode


def test_rows_ref_is_mx8_encode_permuted():
    x = (torch.randn(5, 256, generator=torch.Generator().manual_seed(1)) * torch.exp2(torch.arange(5.0) * 3 - 6)[:, None]).bfloat16()
    x[3, 70] = float("inf")
    codes, exps = utils.mx8_rows_ref(x)
    c0, e0 = mx8_encode(x)
    pi = torch.tensor(utils.MX8_ROWS_PI)
    assert sorted(utils.MX8_ROWS_PI) == list(range(32))
    assert torch.equal(exps, e0)
    back = torch.empty_like(codes).reshape(5, 8, 32)
    back[:, :, pi] = codes.reshape(5, 8, 32)
    assert torch.equal(back.reshape(5, 256), c0.view(torch.uint8))


def test_mx4a8_ref_by_hand():   # x = 1.5 2^b in block b; row r: code 3 (1.5) at k = 32 b + r, exponent 127 + r - b: y[r] = sum_b 1.5 2^b 1.5 2^(r - b) = 9 2^r
    k = torch.arange(128)
    x = (1.5 * torch.exp2((k // 32).float()))[None, :].bfloat16()
    codes = torch.zeros(16, 128, dtype=torch.int32)
    for b in range(4):
        codes[torch.arange(16), 32 * b + torch.arange(16)] = 3
    exps = (127 + torch.arange(16)[:, None] - torch.arange(4)[None, :]).to(torch.uint8)
    assert torch.equal(utils.mx4a8_ref(x, codes, exps), (9 * torch.exp2(torch.arange(16.0)))[None, :].double())


_BUF = ctypes.create_string_buffer(512)
_P = (ctypes.addressof(_BUF) + 63) & ~63   # a non-NULL, aligned dummy: refused calls never dereference it


def _args(**kw):
    base = dict(x_codes=_P, x_exps=_P, w=_P, w_exps=_P, y=_P, m=64, wrows=256, k=512, w_on_right=1, w_format=0, inner_k_tiles=4)
    base.update(kw)
    return _lib.MxGemm(**base)


@pytest.mark.parametrize("kw,code", [
    (dict(x_codes=None), -1), (dict(w_exps=None), -1), (dict(y=None), -1),
    (dict(w=_P + 8), -8), (dict(x_exps=_P + 2), -8), (dict(y=_P + 4), -8), (dict(bias=_P + 2), -8),
    (dict(k=576), -3), (dict(inner_k_tiles=2), -2), (dict(w_on_right=0, w_format=_lib.TG_WFMT_M16N8K16), _lib.TG_E_LAYOUT),
    (dict(struct_bytes=ctypes.sizeof(_lib.MxGemm) - 8), _lib.TG_E_STRUCT), (dict(reserved=1), _lib.TG_E_STRUCT),
    (dict(m=1 << 22, k=1024), -10), (dict(wrows=1 << 22, k=1024), -10),
    (dict(wrows=260), -7), (dict(w_on_right=0, w_format=_lib.TG_WFMT_ROWS, wrows=264), -7), (dict(m=0), -7),
])
def test_gemm_refusals(kw, code):
    assert _lib.load().tg_gemm_mx4a8(ctypes.byref(_args(**kw)), 0, None) == code


@pytest.mark.parametrize("a,code", [
    ((None, 4, 128, _P, _P), -1), ((_P, 4, 128, None, _P), -1), ((_P, 4, 128, _P, None), -1),
    ((_P + 2, 4, 128, _P, _P), -8), ((_P, 4, 128, _P + 8, _P), -8),
    ((_P, 4, 144, _P, _P), -3), ((_P, 0, 128, _P, _P), -7), ((_P, 1 << 20, 1024, _P, _P), -10),
])
def test_quantiser_refusals(a, code):
    assert _lib.load().tg_quant_mx8_rows(*a, 0, None) == code


@pytest.mark.parametrize("kw", [dict(group_size=64), dict(in_features=192), dict(w_inner_k=2), dict(dtype=torch.float16), dict(activations="fp8")])
def test_module_refuses_at_construction(kw):
    args = dict(in_features=256, out_features=32, bias=False, dtype=torch.bfloat16, activations="mx8")
    args.update(kw)
    with pytest.raises(ValueError):
        modules.MX4Linear(**args)


def test_module_default_is_unchanged():
    a = modules.MX4Linear(256, 32, bias=True, dtype=torch.bfloat16)
    b = modules.MX4Linear(256, 32, bias=True, dtype=torch.bfloat16, activations="mx8")
    assert a.activations is None and list(a.state_dict()) == list(b.state_dict()) == ["weight", "bias", "exponents"]
    x = torch.zeros(2, 256, dtype=torch.bfloat16, requires_grad=True)
    with pytest.raises(RuntimeError, match="no input gradient"):
        b(x)
