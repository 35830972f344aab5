"""MX4 x MXFP8 on the block-scaled MFMA (tg_quant_mx8_rows / tg_gemm_mx4a8, w4a8_gemm_mx.cuh) against utils.mx8_rows_ref and the float64
definition utils.mx4a8_ref.  Shapes (m, wrows, k) for the tile 64 x 256 and k step 512: one MFMA; ragged in m, n and the k step; more k steps
than the LDS ring (3) and the register ring (2) have stages.  Every GEMM call has NaN decoys behind x and sentinels around y."""
import ctypes

import numpy as np
import pytest
import torch

from any4_amd import _lib, modules, ops, utils
from any4_amd.kvcache import mx8_decode, mx8_encode
from tests.fused_ref import SENTINEL, contract, guard_intact, guarded
from tests.test_gpu_parity import ulp16

pytestmark = pytest.mark.gpu

BM, BN, KS = 64, 256, 512
SHAPES = [(1, 16, 128), (17, BN + 16, KS + 128), (BM + 1, 2 * BN + 16, 4 * KS + 128)]
SIDES = [True, False]   # Bint4 words (weights on the right) / the same words as TG_WFMT_ROWS (on the left)


def _gemm(x, codes, exps, on_right, bias=None):   # CPU operands -> y (CPU) through the C ABI: the quantiser, then the GEMM with decoys behind x and sentinels around y
    m, k = x.shape
    wrows = codes.shape[0]
    dev = torch.device("cuda")
    xc, xe = ops.quantize_mx8_rows(x.to(dev))
    xcb = torch.full((m + 64, k), 0x7F, dtype=torch.uint8, device=dev)
    xeb = torch.full((m + 64, k // 32), 255, dtype=torch.uint8, device=dev)
    xcb[:m], xeb[:m] = xc, xe
    w = ops.convert_matrix_to_m16n8k16_Bint4_layout(codes.to(dev), 4)
    we = exps.to(dev).contiguous()
    yv, whole = guarded(torch.zeros(m, wrows, dtype=torch.bfloat16), dev, fill=SENTINEL)
    b = bias.to(dev) if bias is not None else None
    args = _lib.MxGemm(x_codes=xcb.data_ptr(), x_exps=xeb.data_ptr(), w=w.data_ptr(), w_exps=we.data_ptr(), bias=b.data_ptr() if b is not None else None,
                       y=yv.data_ptr(), m=m, wrows=wrows, k=k, w_on_right=int(on_right), w_format=0 if on_right else _lib.TG_WFMT_ROWS, inner_k_tiles=4)
    _lib.check(_lib.load().tg_gemm_mx4a8(ctypes.byref(args), 0, ops._stream(xcb)), "tg_gemm_mx4a8")
    torch.cuda.synchronize()
    assert guard_intact(yv, whole)
    return yv.cpu()


def _exact(x, codes, exps, on_right):   # A probe whose every product and sum is exact in bf16: the kernel's output equals the float64 definition bit for bit.
    ref = utils.mx4a8_ref(x, codes, exps)
    assert torch.equal(ref.bfloat16().double(), ref), "the probe itself is not exact"
    y = _gemm(x, codes, exps, on_right)
    bad = (y.double() != ref).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} outputs differ, first at (a, r) = {bad[0].tolist()}: {y[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


def _probe_x(m, k):   # distinct E4M3-exact values in the 32 places of a block, another power of two per (row, block)
    kk, a = torch.arange(k)[None, :], torch.arange(m)[:, None]
    return ((8 + kk % 8) * torch.exp2((kk // 8 % 4 + (a * 5 + kk // 32 * 3) % 21 - 10).float())).bfloat16()


@pytest.mark.parametrize("m,k", [(3, 128), (5, 4096 + 32)])
def test_quantiser_bytes(m, k):
    gen = torch.Generator().manual_seed(m * 1000 + k)
    x = torch.randn(m, k, generator=gen) * torch.exp2(torch.randint(-20, 21, (m, k // 32), generator=gen).float()).repeat_interleave(32, 1)
    x[0, :32] = 0
    x[1, 32:64] = 448 * 2.0 ** 5 * torch.where(torch.arange(32) % 2 == 0, 1.0, -1.0)
    x[2, 64:96][7] = float("inf")
    x = x.bfloat16()
    codes, exps = ops.quantize_mx8_rows(x.cuda())
    rc, re = utils.mx8_rows_ref(x)
    assert re[2, 2] == 255 and re[0, 0] == 0
    assert torch.equal(exps.cpu(), re) and torch.equal(codes.cpu(), rc)


@pytest.mark.parametrize("on_right", SIDES)
@pytest.mark.parametrize("m,wrows,k", SHAPES)
def test_exact_one_hot_weights(m, wrows, k, on_right):   # code 1.0 at (r, j), j over all 32 places of the first and last block and every block boundary: PI, the word split, the exponent bytes, lane ownership
    nb = k // 32
    js = list(range(32)) + list(range(k - 32, k)) + [32 * b + d for b in range(1, nb) for d in (-1, 0)]
    codes = torch.zeros(wrows, k, dtype=torch.int32)
    codes[torch.arange(wrows), torch.tensor([js[r % len(js)] for r in range(wrows)])] = 2
    _exact(_probe_x(m, k), codes, torch.full((wrows, nb), 127, dtype=torch.uint8), on_right)


@pytest.mark.parametrize("on_right", SIDES)
@pytest.mark.parametrize("m,wrows,k", SHAPES)
def test_exact_one_hot_activations(m, wrows, k, on_right):   # one activation per row; the launches sweep both ends of EVERY block (tail step too); weight exponents distinct per (row, block)
    nb = k // 32
    codes = torch.randint(0, 16, (wrows, k), generator=torch.Generator().manual_seed(k + m), dtype=torch.int32)
    exps = (118 + (torch.arange(wrows)[:, None] * 7 + torch.arange(nb)[None, :] * 3) % 19).to(torch.uint8)
    a = torch.arange(m)
    for first in range(0, 2 * nb, m):   # row a takes place t = first + a of the 2 nb (block, end) places
        t = (first + a) % (2 * nb)
        x = torch.zeros(m, k)
        x[a, (t // 2) * 32 + 31 * (t % 2)] = torch.exp2((a % 9 - 4).float()) * 1.5
        _exact(x.bfloat16(), codes, exps, on_right)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("on_right", SIDES)
@pytest.mark.parametrize("m,wrows,k", SHAPES)
def test_f64_bound(m, wrows, k, on_right, with_bias):   # |y - mx4a8_ref| <= the project's GEMM allowance, 0.5 ulp16 (1 + 2^-7) + 4e-6 sum |x^ w| (tests.fused_ref.contract).
    gen = torch.Generator().manual_seed(m + wrows + k)
    codes, exps = utils.quantize_mx4(torch.randn(wrows, k, generator=gen), 32)
    x = torch.randn(m, k, generator=gen).bfloat16()
    bias = torch.randn(wrows, generator=gen).bfloat16() if with_bias else None
    ref = utils.mx4a8_ref(x, codes, exps)
    S = mx8_decode(*mx8_encode(x), torch.float64).abs() @ utils.dequantize_mx4(codes, exps).double().abs().t()
    y = _gemm(x, codes, exps, on_right, bias)
    allow = contract(ref.numpy(), S.numpy(), torch.bfloat16)
    if with_bias:   # RNE16(RNE16(acc) + bias): the first rounding within the allowance, the second half an ulp of the sum
        ref = ref + bias.double()
        allow = allow + 0.5 * ulp16(ref.numpy(), torch.bfloat16) * (1 + 2.0 ** -7)
    ratio = float((np.abs(y.double().numpy() - ref.numpy()) / allow).max())
    print(f"mx4a8_f64 m={m} wrows={wrows} k={k} {'Bint4' if on_right else 'rows'} bias={int(with_bias)}: worst |y - ref| / allowance = {ratio:.4f}")
    assert ratio <= 1.0   # (the lines of one run on an MI355X: profiles/mx4a8_f64_checks.txt)


@pytest.mark.parametrize("on_right", SIDES)
def test_nan_placement(on_right):   # a weight exponent of 255: exactly that column; a non-finite activation block: exactly that row
    m, wrows, k = SHAPES[1]
    gen = torch.Generator().manual_seed(5)
    codes, exps = utils.quantize_mx4(torch.randn(wrows, k, generator=gen), 32)
    exps[BN + 3, k // 32 - 1] = 255
    x = torch.randn(m, k, generator=gen).bfloat16()
    x[11, 40] = float("inf")
    y = _gemm(x, codes, exps, on_right)
    want = (torch.arange(m)[:, None] == 11) | (torch.arange(wrows)[None, :] == BN + 3)
    assert torch.equal(torch.isnan(y), want)


@pytest.mark.parametrize("on_right", SIDES)
def test_module_repeatable_and_graph(on_right):   # MX4Linear(activations='mx8'), either kernel: the C ABI's bits; two calls and a captured-graph replay of quantise + GEMM give the same bits
    m, wrows, k = SHAPES[2]
    gen = torch.Generator().manual_seed(9)
    codes, exps = utils.quantize_mx4(torch.randn(wrows, k, generator=gen), 32)
    x = torch.randn(m, k, generator=gen).bfloat16()
    kernel = "linear_y_f16RM_x_f16RM_W_mx4TC" if on_right else "linear_y_f16RM_W_mx4TC_x_f16RM"
    lin = modules.MX4Linear(k, wrows, bias=False, device="cuda", dtype=torch.bfloat16, kernel=kernel, activations="mx8")
    lin.weight.data, lin.exponents.data = codes.cuda(), exps.cuda()
    xd = x.cuda()
    with torch.no_grad():
        y1, y2 = lin(xd), lin(xd)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            yg = lin(xd)
        for _ in range(3):
            yg.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(yg, y1)
    assert torch.equal(y1, y2) and torch.equal(y1.cpu(), _gemm(x, codes, exps, on_right))
