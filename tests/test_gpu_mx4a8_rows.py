"""MX4 x MXFP8 at 1 ... 64 rows (tg_gemm_mx4a8_rows, w4a8_rows_mx.cuh) against the float64 definition utils.mx4a8_ref.  Shapes (m, wrows, k) in
the kernel's constants (k step 512, four waves, window W and the full grid from tg_gemm_mx4a8_rows_plan): one MFMA; ragged m, a tail step, an odd
number of row tiles; every wave a step and wave 0 two; a second k window through the workspace; a second activation block of one row, and four
full ones; workgroups that walk three row tiles (the ring's steady loop, then its one-tile tail) and one that walks two (the two-tile tail).
Every call has NaN decoys behind x and sentinels around y, and runs TWICE on one workspace zeroed once: the same bits, i.e. the counters are
left at zero.  The float64 bound is first checked on the CPU for the same inputs, with float32 sums in the tile kernel's order; an input on
which the matrix instruction itself misses it is on record in profiles/mx4a8_f64_checks.txt (Numerics)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from any4_amd import _lib, modules, ops, utils
from any4_amd.kvcache import mx8_decode, mx8_encode
from tests.fused_ref import SENTINEL, contract, guard_intact, guarded
from tests.test_gpu_mx4a8 import _probe_x
from tests.test_gpu_parity import ulp16

pytestmark = pytest.mark.gpu
KS = 512   # W (k of a window) and FULL (workgroups of a full grid) come from the library when a test runs: _dims
SHAPES = [(1, 16, 128), (5, 48, KS + 128), (16, 32, 4 * KS + 128), (16, 32, "W + 128"), (17, 16, 2 * KS), (64, 16, KS + 128), (3, "16 * (2 * FULL + 1)", 128)]
SIDES = [True, False]   # Bint4 words (weights on the right) / the same words as TG_WFMT_ROWS (on the left)


@functools.lru_cache(None)
def _consts():   # tg_gemm_mx4a8_rows_plan: (workgroups sharing the row tiles, activation blocks, k windows, k of a window)
    out = (ctypes.c_int64 * 4)()
    assert _lib.load().tg_gemm_mx4a8_rows_plan(1, 1 << 24, 128, out) == 0
    return {"W": out[3], "FULL": out[0]}


def _dims(*shape):
    return [eval(v, dict(_consts())) if isinstance(v, str) else v for v in shape]


def _gemm(x, codes, exps, on_right, bias=None):   # CPU operands -> y (CPU) through the C ABI, twice on one workspace
    (m, k), wrows, dev, L = x.shape, codes.shape[0], torch.device("cuda"), _lib.load()
    xc, xe = ops.quantize_mx8_rows(x.to(dev))
    xcb, xeb = torch.full((m + 64, k), 0x7F, dtype=torch.uint8, device=dev), torch.full((m + 64, k // 32), 255, dtype=torch.uint8, device=dev)
    xcb[:m], xeb[:m] = xc, xe
    w, we, b = ops.convert_matrix_to_m16n8k16_Bint4_layout(codes.to(dev), 4), exps.to(dev).contiguous(), bias.to(dev) if bias is not None else None
    need = L.tg_gemm_mx4a8_rows_workspace_bytes(m, wrows, k)
    ws, ys = torch.zeros(need, dtype=torch.uint8, device=dev), []
    for _ in range(2):
        yv, whole = guarded(torch.zeros(m, wrows, dtype=torch.bfloat16), dev, fill=SENTINEL)
        args = _lib.MxGemm(x_codes=xcb.data_ptr(), x_exps=xeb.data_ptr(), w=w.data_ptr(), w_exps=we.data_ptr(), bias=b.data_ptr() if b is not None else None,
                           y=yv.data_ptr(), m=m, wrows=wrows, k=k, w_on_right=int(on_right), w_format=0 if on_right else _lib.TG_WFMT_ROWS, inner_k_tiles=4)
        _lib.check(L.tg_gemm_mx4a8_rows(ctypes.byref(args), ws.data_ptr() if need else None, need, 0, ops._stream(xcb)), "tg_gemm_mx4a8_rows")
        torch.cuda.synchronize()
        assert guard_intact(yv, whole)
        ys.append(yv.cpu())
    assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16)), "the second call on the same workspace gave other bits"
    return ys[0]


def _exact(x, codes, exps, on_right):   # A probe whose every product and sum is exact in bf16: the kernel's output equals the float64 definition bit for bit.
    ref = utils.mx4a8_ref(x, codes, exps)
    assert torch.equal(ref.bfloat16().double(), ref), "the probe itself is not exact"
    y = _gemm(x, codes, exps, on_right)
    bad = (y.double() != ref).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} outputs differ, first at (a, r) = {bad[0].tolist()}: {y[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


@pytest.mark.parametrize("on_right", SIDES)
@pytest.mark.parametrize("m,wrows,k", SHAPES)
def test_exact_one_hot_weights(m, wrows, k, on_right):   # code 1.0 at (r, j); the launches sweep j over all 32 places of the first and last block and every block boundary
    m, wrows, k = _dims(m, wrows, k)
    nb = k // 32
    js = list(range(32)) + list(range(k - 32, k)) + [32 * b + d for b in range(1, nb) for d in (-1, 0)]
    for first in range(0, len(js), wrows):
        codes = torch.zeros(wrows, k, dtype=torch.int32)
        codes[torch.arange(wrows), torch.tensor([js[(first + r) % len(js)] for r in range(wrows)])] = 2
        _exact(_probe_x(m, k), codes, torch.full((wrows, nb), 127, dtype=torch.uint8), on_right)


@pytest.mark.parametrize("on_right", SIDES)
@pytest.mark.parametrize("m,wrows,k", SHAPES)
def test_exact_one_hot_activations(m, wrows, k, on_right):   # one activation per row; the launches sweep both ends of EVERY block; weight exponents distinct per (row, block)
    m, wrows, k = _dims(m, wrows, k)
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
def test_f64_bound(m, wrows, k, on_right, with_bias):   # |y - mx4a8_ref| <= the project's GEMM allowance, 0.5 ulp16 (1 + 2^-7) + 4e-6 sum |x^ w| (tests.fused_ref.contract)
    m, wrows, k = _dims(m, wrows, k)
    gen = torch.Generator().manual_seed(m + wrows + k)
    codes, exps = utils.quantize_mx4(torch.randn(wrows, k, generator=gen), 32)
    x = torch.randn(m, k, generator=gen).bfloat16()
    bias = torch.randn(wrows, generator=gen).bfloat16() if with_bias else None
    ref = utils.mx4a8_ref(x, codes, exps)
    xh, wd = mx8_decode(*mx8_encode(x), torch.float64), utils.dequantize_mx4(codes, exps).double()
    allow = contract(ref.numpy(), (xh.abs() @ wd.abs().t()).numpy(), torch.bfloat16)
    acc = torch.zeros(m, wrows)   # the tile kernel's order in float32: per 512-k step, MFMA c adds the blocks 4 g + c of the step, g = 0 ... 3
    for b0, c in ((b0, c) for b0 in range(0, k // 32, 16) for c in range(4)):
        cols = torch.cat([torch.arange(32 * b, 32 * b + 32) for b in range(b0 + c, min(b0 + 16, k // 32), 4)] or [torch.arange(0)])
        acc = (acc.double() + xh[:, cols] @ wd[:, cols].t()).float()
    y_cpu = acc.bfloat16()
    if with_bias:   # RNE16(RNE16(acc) + bias): the first rounding within the allowance, the second half an ulp of the sum
        ref, y_cpu = ref + bias.double(), (y_cpu.float() + bias.float()).bfloat16()
        allow = allow + 0.5 * ulp16(ref.numpy(), torch.bfloat16) * (1 + 2.0 ** -7)
    worst = lambda y: float((np.abs(y.double().numpy() - ref.numpy()) / allow).max())
    assert worst(y_cpu) <= 1.0, f"float32 sums on the CPU miss the bound on these inputs: {worst(y_cpu):.4f}"
    ratio = worst(_gemm(x, codes, exps, on_right, bias))
    print(f"mx4a8_rows_f64 m={m} wrows={wrows} k={k} {'Bint4' if on_right else 'rows'} bias={int(with_bias)}: worst |y - ref| / allowance = {ratio:.4f} (float32 on the CPU {worst(y_cpu):.4f})")
    assert ratio <= 1.0


@pytest.mark.parametrize("on_right", SIDES)
def test_nan_and_batch_independence(on_right):   # a weight exponent of 255: exactly that column; a non-finite activation block: exactly that row; row 0's bits at m = 1, 16, 17
    m, wrows, k = _dims(17, 32, "W + 128")
    gen = torch.Generator().manual_seed(5)
    codes, exps = utils.quantize_mx4(torch.randn(wrows, k, generator=gen), 32)
    x = torch.randn(m, k, generator=gen).bfloat16()
    y1, y16, y17 = (_gemm(x[:n], codes, exps, on_right) for n in (1, 16, 17))
    assert torch.equal(y1[0], y16[0]) and torch.equal(y1[0], y17[0]) and torch.equal(y16, y17[:16])
    exps[19, k // 32 - 1] = 255
    x[11, 40] = float("inf")
    want = (torch.arange(m)[:, None] == 11) | (torch.arange(wrows)[None, :] == 19)
    assert torch.equal(torch.isnan(_gemm(x, codes, exps, on_right)), want)


@pytest.mark.parametrize("on_right", SIDES)
def test_module_small_batch_and_graph(on_right):   # MX4Linear(small_batch=True): the C ABI's bits, and a captured graph of quantise + GEMM replays to them; 65 rows: the tile kernel
    m, wrows, k = _dims(16, 32, "W + 128")
    gen = torch.Generator().manual_seed(9)
    codes, exps = utils.quantize_mx4(torch.randn(wrows, k, generator=gen), 32)
    x = torch.randn(65, k, generator=gen).bfloat16()
    kernel = "linear_y_f16RM_x_f16RM_W_mx4TC" if on_right else "linear_y_f16RM_W_mx4TC_x_f16RM"
    lins = [modules.MX4Linear(k, wrows, bias=False, device="cuda", dtype=torch.bfloat16, kernel=kernel, activations="mx8", small_batch=sb) for sb in (True, False)]
    for lin in lins:
        lin.weight.data, lin.exponents.data = codes.cuda(), exps.cuda()
    xd, g = x.cuda(), torch.cuda.CUDAGraph()
    with torch.no_grad():
        y1 = lins[0](xd[:m])
        with torch.cuda.graph(g):
            yg = lins[0](xd[:m])
        for _ in range(3):
            yg.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(yg, y1)
        assert torch.equal(lins[0](xd), lins[1](xd))
    assert torch.equal(y1.cpu(), _gemm(x[:m], codes, exps, on_right))
