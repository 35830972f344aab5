"""Quantizer on the box: produces the inputs of the tinygemm path -- codes, per-row
16-entry LUT, per-group scale/zero -- from 16/32-bit weights, and swaps `nn.Linear` modules for the quantized
modules, with the reference's function names, arguments and return conventions:

  group_q / degroup_q / pack_scales_and_zeros / extract_scales_and_zeros     quantize.py:87-181
  intq_quantize_tensor / intq_dequantize_tensor / intq_reconstruct_tensor    quantize.py:183-221
  anyq_quantize_tensor / anyq_dequantize_tensor / anyq_reconstruct_tensor    quantize.py:523-637, 810-825
  intq_layer / anyq_layer                                                    quantize.py:333-391, 827-905
  quantize_model                                                             quantize.py:32-85

What is different by design: the reference clusters every weight row with scikit-learn's KMeans on the host
(one Python task per row under joblib, quantize.py:406-418, 506-521 -- minutes per 4096x4096 layer).  Here all
rows are clustered at once by a batched weighted 1-D Lloyd iteration in torch on the device that holds the
weights (`kmeans_rows`): a 1-D assignment is a `searchsorted` against the 15 midpoints of the sorted
centroids, the update two `scatter_add`s, so a layer takes milliseconds on the GPU.  Parity with scikit-learn
is statistical, not bit-exact (different seeding): tests pin it by reconstruction error against the reference's
own output on the fixture of BASELINE config 1 and by exact recovery when a row has <= 16 distinct values.
This module is the step BEFORE the hot path; none of it runs per token.
"""
from __future__ import annotations

import gc
import warnings
from typing import Callable, Optional

import torch


# --------------------------------------------------------------------------------------------------
# grouping (quantize.py:87-181)
# --------------------------------------------------------------------------------------------------

def pack_scales_and_zeros(scales: torch.Tensor, zeros: torch.Tensor, w_shape) -> torch.Tensor:
    """[n * k/g] scales and zeros -> [k/g][n][2] (scale, zero of one q-group adjacent: one 32-bit load)."""
    n = w_shape[0]
    return torch.stack([scales.reshape(n, -1), zeros.reshape(n, -1)], dim=2).transpose(0, 1).contiguous()


def expand_q_groups(x: torch.Tensor, orig_size, q_group_size: int) -> torch.Tensor:
    n, k = orig_size
    return x.reshape(n, k // q_group_size, 1).expand(n, k // q_group_size, q_group_size).reshape(n, k)


def extract_scales_and_zeros(scales_and_zeros: torch.Tensor, w_shape, q_group_size: int):
    s = scales_and_zeros.transpose(0, 1)
    return expand_q_groups(s[:, :, 0], w_shape, q_group_size), expand_q_groups(s[:, :, 1], w_shape, q_group_size)


_DIVISORS: dict = {}


def _divisor(value: float, device) -> torch.Tensor:
    key = (value, str(device))
    t = _DIVISORS.get(key)
    if t is None:
        t = _DIVISORS[key] = torch.tensor(value, device=device)
    return t


def group_q(w_orig: torch.Tensor, n_bit: int, q_group_size: int = 128, assymetric: bool = True, unsigned: bool = True,
            zero_point: bool = True):
    """Scale every q-group onto the integer grid WITHOUT rounding: returns (w in grid units, the image of 0,
    scales_and_zeros).  Asymmetric: scale = max(max - min, 1e-6) / (2^n - 1), zero = min (+ 2^(n-1) scale)."""
    w = w_orig.float()
    if q_group_size <= 1 or w.dim() != 2 or w.shape[-1] % q_group_size != 0:
        raise ValueError("group_q needs a 2-D tensor whose last dimension is a multiple of q_group_size > 1")
    tq = w.reshape(-1, q_group_size)
    if torch.isnan(tq).any():
        raise ValueError("NaN in the tensor to quantize")
    if assymetric:
        mx, mn = tq.amax(dim=1, keepdim=True), tq.amin(dim=1, keepdim=True)
        lo, hi = (0, 2 ** n_bit - 1) if unsigned else (-(2 ** (n_bit - 1)), 2 ** (n_bit - 1) - 1)
        # (divisor as a tensor on w's device: torch turns `tensor / python_scalar` on the GPU into a multiplication by the rounded
        # reciprocal, one ulp off the IEEE quotient the reference's CPU path computes -- enough to flip a bf16 scale.  PARITY TARGET: the
        # reference run on the CPU, which is what tests/golden/group_quant.npz captured and tests/test_quantize_cpu.py /
        # test_gpu_decode.py check bit for bit on both devices; a checkpoint quantised by the reference ON A GPU can differ from this
        # by one ulp of a scale.  The divisor tensor is made once per (device, value): no host-to-device copy per call.)
        scales = (mx - mn).clamp(min=1e-6) / _divisor(float(hi - lo), w.device)
        zeros = mn + scales * (2 ** (n_bit - 1)) if zero_point else mn
        w_new = tq.sub(mn).div(scales).reshape(w.shape)
        w_zero = torch.zeros_like(tq).sub(mn).div(scales).reshape(w.shape)
    else:
        scales = tq.abs().amax(dim=1, keepdim=True).clamp(min=1e-6) / _divisor(float(2 ** (n_bit - 1) - 1), w.device)
        zeros = torch.zeros_like(scales)
        w_new = tq.div(scales).reshape(w.shape)
        w_zero = torch.zeros_like(w_new)
    return w_new, w_zero, pack_scales_and_zeros(scales, zeros, w.shape)


def degroup_q(w_c: torch.Tensor, scales_and_zeros=None, scales=None, zeros=None, n_bit: int = 4, q_group_size: int = 128,
              centering: bool = True) -> torch.Tensor:
    if scales_and_zeros is not None:
        s1, z1 = extract_scales_and_zeros(scales_and_zeros, w_c.shape, q_group_size)
        scales = s1 if scales is None else scales
        zeros = z1 if zeros is None else zeros
    if not q_group_size:
        return w_c
    if centering:
        w_c = w_c - (2 ** (n_bit - 1))
    return w_c * scales + zeros


# --------------------------------------------------------------------------------------------------
# uniform integer quantization (quantize.py:183-215)
# --------------------------------------------------------------------------------------------------

def intq_quantize_tensor(x: torch.Tensor, n_bit: int = 4, q_group_size: int = 128, scale_only: bool = False,
                         new_grouping=False, unsigned: bool = False, zero_point: bool = False, **_):
    """-> (int32 codes, the image of zero, scales_and_zeros [k/g][n][2] in x's dtype).
    new_grouping="tinygemm": the packing-ready grid of tinygemm_lib.utils.group_quantize_tensor (codes 0..15,
    zero = min + 8 scale) -- what the Int4Linear kernels consume; otherwise group_q + round."""
    if new_grouping == "tinygemm":
        from .utils import group_quantize_tensor

        intq, sz = group_quantize_tensor(x, n_bit=n_bit, q_group_size=q_group_size)
        _, zg = extract_scales_and_zeros(sz, x.shape, q_group_size)
    elif new_grouping:
        raise NotImplementedError("group_q1 (new_grouping=True) is not part of the tinygemm path")
    else:
        intq, zg, sz = group_q(x, n_bit, q_group_size=q_group_size, assymetric=not scale_only, unsigned=unsigned,
                               zero_point=zero_point)
        intq = intq.round()
    return intq.to(torch.int32), zg, sz.to(x.dtype)


def intq_dequantize_tensor(intq: torch.Tensor, scales_and_zeros=None, scales=None, zeros=None, n_bit: int = 4,
                           q_group_size: int = 128, dtype=torch.float16, **_):
    return degroup_q(intq, scales_and_zeros=scales_and_zeros, scales=scales, zeros=zeros, n_bit=n_bit,
                     q_group_size=q_group_size, centering=False).to(dtype)


def intq_reconstruct_tensor(x, n_bit: int = 4, q_group_size: int = 128, unsigned: bool = False, zero_point: bool = False,
                            scale_only: bool = False, dtype=torch.float16, **_):
    intq, _, sz = intq_quantize_tensor(x, n_bit=n_bit, q_group_size=q_group_size, scale_only=scale_only, unsigned=unsigned,
                                       zero_point=zero_point)
    return intq_dequantize_tensor(intq, scales_and_zeros=sz, n_bit=n_bit, q_group_size=q_group_size, dtype=dtype)


# --------------------------------------------------------------------------------------------------
# batched weighted 1-D k-means (replaces quantize.py:406-418 + kmeans.py:139-287)
# --------------------------------------------------------------------------------------------------

def _init_centers(kind: str, x, xs, lo, span, C: int):
    rows, k = x.shape
    steps = (torch.arange(C, device=x.device, dtype=torch.float32) + 0.5) / C
    if kind == "uniform":      # equally spaced over the row's range
        return lo + span * steps
    if kind == "quantile":     # equal-population cells
        return xs[:, (steps * k).long().clamp(0, k - 1)]
    if kind == "density":      # Panter-Dite: the optimal 1-D quantizer's point density goes with pdf^(1/3)
        B = 512
        b = ((x - lo) / span * B).long().clamp(0, B - 1)
        dens = torch.zeros(rows, B, device=x.device).scatter_add_(1, b, torch.ones_like(x)).pow(1.0 / 3.0)
        cdf = dens.cumsum(1)
        cdf = (cdf / cdf[:, -1:]).contiguous()
        bi = torch.searchsorted(cdf, steps.expand(rows, C).contiguous()).clamp(0, B - 1)
        return lo + (bi.float() + 0.5) / B * span
    raise ValueError(f"unknown init {kind!r}")


def _lloyd(x, wts, xw, c, span, max_iter: int, tol: float):
    """Weighted Lloyd iterations from centres c; returns (assign, centres sorted, weighted SSE per row)."""
    rows, k = x.shape
    C = c.shape[1]
    for _ in range(max_iter):
        c = torch.sort(c, dim=1).values
        mid = ((c[:, 1:] + c[:, :-1]) * 0.5).contiguous()
        assign = torch.searchsorted(mid, x)                                   # [rows][k] in 0..C-1
        cnt = torch.zeros(rows, C, device=x.device).scatter_add_(1, assign, wts)
        tot = torch.zeros(rows, C, device=x.device).scatter_add_(1, assign, xw)
        new = torch.where(cnt > 0, tot / cnt.clamp_min(1e-30), c)
        empty = cnt <= 0
        if bool(empty.any()):
            # re-seed the j-th empty cluster of a row at its j-th worst-represented point
            err = (x - new.gather(1, assign)).abs() * wts
            top_e, top_i = torch.topk(err, min(C, k), dim=1)
            rank = (torch.cumsum(empty.int(), dim=1) - 1).clamp(0, top_i.shape[1] - 1)
            cand, cand_e = x.gather(1, top_i).gather(1, rank), top_e.gather(1, rank)
            new = torch.where(empty & (cand_e > 0), cand, new)
        moved = bool(((new - c).abs() > tol * span).any())
        c = new
        if not moved:
            break
    c = torch.sort(c, dim=1).values
    mid = ((c[:, 1:] + c[:, :-1]) * 0.5).contiguous()
    assign = torch.searchsorted(mid, x)
    sse = ((x - c.gather(1, assign)) ** 2 * wts).sum(1)
    return assign, c, sse


def _prefix_f64(v: torch.Tensor, order: str) -> torch.Tensor:
    """[rows][k] f64 -> [rows][k + 1] exclusive-then-total prefix sums, in one of two summation orders."""
    rows, k = v.shape
    zero = torch.zeros(rows, 1, dtype=torch.float64, device=v.device)
    if order == "sequential":
        return torch.cat([zero, v.cumsum(1)], dim=1)
    if order != "blocked":
        raise ValueError(f"unknown prefix order {order!r}")
    nb = (k + 31) // 32  # block totals by a pairwise tree, the blocks' prefix and the inside of a block sequential
    blk = torch.cat([v, torch.zeros(rows, nb * 32 - k, dtype=torch.float64, device=v.device)], dim=1).reshape(rows, nb, 32)
    tot = blk
    while tot.shape[2] > 1:
        tot = tot[:, :, 0::2] + tot[:, :, 1::2]
    base = torch.cat([zero, tot[:, :, 0].cumsum(1)[:, :-1]], dim=1)
    return torch.cat([zero, (base[:, :, None] + blk.cumsum(2)).reshape(rows, nb * 32)[:, :k]], dim=1)


@torch.no_grad()
def lloyd_rows_ref(x: torch.Tensor, wts: Optional[torch.Tensor], c0: torch.Tensor, max_iter: int = 300, tol: float = 1e-6, *,
                   prefix: str = "sequential"):
    """The definition of the fused k-means kernel (csrc/kmeans.cuh, tg_kmeans_rows), in float64: weighted 1-D Lloyd iterations on every
    row of x f32 [rows][k] from the seed centres c0 f32 [rows][C] of ONE seeding; wts f32 [rows][k], already abs().clamp_min(1e-12), or None.

    Per row: sort the row ascending, carrying the weights; f64 prefix sums of w and of x w (the product formed in f64);
    span = max(x_max - x_min, 1e-12).  An iteration sorts the centres, takes the midpoints (c[j+1] + c[j]) * 0.5, gives cluster j the
    points with mid[j-1] < x <= mid[j] (`searchsorted(mid, x)`) and moves its centre to tot / cnt, both differences of prefix sums.  A
    cluster with no points keeps its centre; then the j-th empty cluster of the row (j < k) is re-seeded at the point with the j-th
    largest |x - c[assign]| * w (ties: the lower position in the sorted row), where that error is > 0.  The row stops when no centre
    moved by more than tol * span, or after max_iter iterations.  Then the centres are sorted and the points assigned, in their
    original order, against the final f64 midpoints.

    Two decisions differ from `_lloyd` on purpose:
      * a row stops on its OWN criterion, not when the slowest row of the batch has converged;
      * sums are in f64 and in a fixed order (prefix sums over the sorted row), not f32 scatter_adds.
    `prefix` picks the order of the prefix summation ("sequential" | "blocked"): on inputs whose sums are exact in f64 the result does
    not depend on it, which is what lets the kernel keep block prefixes.

    Returns (assign int32 [rows][k], centres f32 [rows][C] ascending -- one rounding from f64, weighted SSE f64 [rows] against the f64
    centres, iterations run int32 [rows]).
    """
    rows, k = x.shape
    C = c0.shape[1]
    dev = x.device
    xd = x.double()
    xs, order = torch.sort(xd, dim=1, stable=True)
    wd = torch.ones_like(xd) if wts is None else wts.double()
    ws = wd.gather(1, order)
    PW, PX = _prefix_f64(ws, prefix), _prefix_f64(xs * ws, prefix)
    thr = (xs[:, -1] - xs[:, 0]).clamp_min(1e-12) * tol
    c = c0.double().clone()
    active = torch.ones(rows, dtype=torch.bool, device=dev)
    iters = torch.zeros(rows, dtype=torch.int32, device=dev)
    pos = torch.arange(k, device=dev).expand(rows, k).contiguous()
    zero_col = torch.zeros(rows, 1, dtype=torch.long, device=dev)
    k_col = torch.full((rows, 1), k, dtype=torch.long, device=dev)
    m = min(C, k)
    for _ in range(max_iter):
        if not bool(active.any()):
            break
        cs = torch.sort(c, dim=1).values
        mid = ((cs[:, 1:] + cs[:, :-1]) * 0.5).contiguous()
        b = torch.searchsorted(xs, mid, right=True)                 # points <= mid[j]
        B = torch.cat([zero_col, b, k_col], dim=1)
        n = B[:, 1:] - B[:, :-1]
        cnt = PW.gather(1, B[:, 1:]) - PW.gather(1, B[:, :-1])
        tot = PX.gather(1, B[:, 1:]) - PX.gather(1, B[:, :-1])
        ok = (n > 0) & (cnt > 0)
        new = torch.where(ok, tot / torch.where(ok, cnt, torch.ones_like(cnt)), cs)
        empty = n <= 0
        if bool((empty & active[:, None]).any()):
            a_s = torch.searchsorted(b.contiguous(), pos, right=True)  # the cluster of sorted position i: boundaries <= i
            err = (xs - new.gather(1, a_s)).abs() * ws
            se, si = torch.sort(err, dim=1, descending=True, stable=True)
            rank = torch.cumsum(empty.long(), dim=1) - 1
            r = rank.clamp(0, m - 1)
            cand_e = se[:, :m].gather(1, r)
            cand = xs.gather(1, si[:, :m]).gather(1, r)
            new = torch.where(empty & (rank < m) & (cand_e > 0), cand, new)
        moved = ((new - cs).abs() > thr[:, None]).any(1)
        c = torch.where(active[:, None], new, c)
        iters += active.to(torch.int32)
        active = active & moved
    cs = torch.sort(c, dim=1).values
    mid = ((cs[:, 1:] + cs[:, :-1]) * 0.5).contiguous()
    assign = torch.searchsorted(mid, xd.contiguous())
    sse = ((xd - cs.gather(1, assign)) ** 2 * wd).sum(1)
    return assign.to(torch.int32), cs.float(), sse, iters


KMEANS_FUSED_MAX_K = 16384  # the row (and its weights) stay in the LDS of one workgroup: csrc/kmeans.cuh KM_MAX_K
KMEANS_FUSED_MAX_C = 16
KMEANS_FUSED_MAX_S = 4


def kmeans_rows_launch(x: torch.Tensor, wts: Optional[torch.Tensor], c0: torch.Tensor, max_iter: int = 300, tol: float = 1e-6):
    """One tg_kmeans_rows launch: x f32 [rows][k] on the GPU, wts None / f32 [k] (shared) / f32 [rows][k] -- already abs().clamp_min(1e-12)
    --, c0 f32 [S][rows][C] (or [rows][C]: one seeding).  -> (assign int32, centres f32, sse f64, iters int32) as lloyd_rows_ref,
    the seeding with the strictly smallest SSE kept; iters is summed over the seedings."""
    from . import _lib

    if c0.dim() == 2:
        c0 = c0[None]
    rows, k = x.shape
    S, _, C = c0.shape
    if not x.is_cuda:
        raise ValueError("the fused k-means runs on the GPU only (there is no CPU fallback): move the tensor to the device, or pass fused=False")
    if x.dtype != torch.float32 or c0.dtype != torch.float32 or tuple(c0.shape[1:]) != (rows, C) or c0.device != x.device:
        raise ValueError("kmeans_rows_launch: x f32 [rows][k] and c0 f32 [S][rows][C] on one device")
    x, c0 = x.contiguous(), c0.contiguous()
    stride = 0
    if wts is not None:
        if wts.dtype != torch.float32 or wts.device != x.device or tuple(wts.shape) not in ((k,), (rows, k)):
            raise ValueError("kmeans_rows_launch: weights f32 [k] or [rows][k] on x's device")
        wts = wts.contiguous()
        stride = k if wts.dim() == 2 else 0
    assign = torch.empty(rows, k, dtype=torch.int32, device=x.device)
    centers = torch.empty(rows, C, dtype=torch.float32, device=x.device)
    sse = torch.empty(rows, dtype=torch.float64, device=x.device)
    iters = torch.empty(rows, dtype=torch.int32, device=x.device)
    rc = _lib.load().tg_kmeans_rows(x.data_ptr(), 0 if wts is None else wts.data_ptr(), stride, c0.data_ptr(), assign.data_ptr(),
                                    centers.data_ptr(), sse.data_ptr(), iters.data_ptr(), rows, k, C, S, int(max_iter), float(tol),
                                    x.device.index if x.device.index is not None else torch.cuda.current_device(),
                                    torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(rc, "tg_kmeans_rows")
    return assign, centers, sse, iters


@torch.no_grad()
def kmeans_rows(x: torch.Tensor, n_clusters: int = 16, sample_weight: Optional[torch.Tensor] = None,
                max_iter: int = 300, tol: float = 1e-6, init=("uniform", "density", "quantile"), fused: bool = False,
                return_stats: bool = False):
    """Independent 1-D k-means on every row of x [rows][k] (float32, any device).

    sample_weight: None, [k] (shared by all rows -- activation-aware any4, quantize.py:483-489) or [rows][k].
    init: one seeding or a tuple of seedings ("uniform" | "density" | "quantile"); with several, every row keeps
    the clustering with the smallest weighted squared error (scikit-learn's `n_init`, deterministic here).
    Empty clusters are re-seeded at the points with the largest weighted error, so a row with at most C distinct
    values is reproduced exactly.  Stops when no centroid moves by more than tol * row range (max_iter as sklearn).
    Returns (assign int32 [rows][k], centers float32 [rows][C] sorted ascending).

    fused=True: the iterations of all seedings run in ONE launch of the HIP kernel (csrc/kmeans.cuh; its definition is lloyd_rows_ref):
    no host sync, every row stops on its own criterion, f64 sums in a fixed order -- the same bits from run to run.  Weights and seeds
    are prepared exactly as below, in torch.  GPU only, finite values, n_clusters <= 16, rows of at most 16384 points, at most 4
    seedings: anything else raises ValueError before a launch.  return_stats=True (fused only) additionally returns
    (weighted SSE f64 [rows], iterations summed over the seedings int32 [rows]).
    """
    if return_stats and not fused:
        raise ValueError("kmeans_rows: return_stats needs fused=True")
    if fused:  # (the reasons that do not depend on the device first: each can be told apart without a GPU)
        if n_clusters > KMEANS_FUSED_MAX_C or n_clusters < 1:
            raise ValueError(f"kmeans_rows(fused=True): n_clusters must be 1 ... {KMEANS_FUSED_MAX_C}, got {n_clusters}")
        if x.dim() != 2 or x.shape[1] < 1 or x.shape[1] > KMEANS_FUSED_MAX_K:
            raise ValueError(f"kmeans_rows(fused=True): a row holds 1 ... {KMEANS_FUSED_MAX_K} points (it stays in one workgroup's LDS), "
                             f"got shape {tuple(x.shape)}; longer rows (per_row=False) stay on fused=False")
        if not bool(torch.isfinite(x).all()):
            raise ValueError("kmeans_rows(fused=True): non-finite values in the tensor")
        if not x.is_cuda:
            raise ValueError("kmeans_rows(fused=True) runs on the GPU only (there is no CPU fallback): move the tensor to the device, or pass fused=False")
    x = x.float().contiguous()
    rows, k = x.shape
    shared_w = None
    if sample_weight is None:
        wts = None if fused else torch.ones_like(x)
    else:
        wts = sample_weight.to(x.device, torch.float32).abs()
        if fused and wts.dim() == 1:
            shared_w = wts.reshape(k).clamp_min(1e-12).contiguous()  # one [k] vector for all rows: never expanded
            wts = None
        else:
            wts = (wts.reshape(1, k).expand(rows, k) if wts.dim() == 1 else wts.reshape(rows, k)).contiguous()
            wts = wts.clamp_min(1e-12)  # a zero weight must not orphan a point (kmeans.py run_kmeans: sample_weight_eps)
    if fused:
        w_any = shared_w if shared_w is not None else wts
        if w_any is not None and not bool(torch.isfinite(w_any).all()):
            raise ValueError("kmeans_rows(fused=True): non-finite values in the sample weights")
    xw = None if fused else x * wts
    xs = torch.sort(x, dim=1).values
    lo = xs[:, :1]
    span = (xs[:, -1:] - lo).clamp_min(1e-12)
    best = None
    # the reference forwards `init` to scikit-learn (None / "k-means++" / "random", quantize.py:413): those have no meaning
    # for this batched Lloyd -> its default deterministic seedings
    if init is None or (isinstance(init, str) and init in ("k-means++", "random")):
        if init is not None and init not in _WARNED_INIT:
            _WARNED_INIT.add(init)
            warnings.warn(f"kmeans_rows: init={init!r} is scikit-learn's seeding; this batched Lloyd has no random state and "
                          f"uses its deterministic seedings {_SEEDINGS} instead (results do not depend on a seed)", stacklevel=2)
        init = _SEEDINGS
    if fused:
        kinds = (init,) if isinstance(init, str) else tuple(init)
        if not 1 <= len(kinds) <= KMEANS_FUSED_MAX_S:
            raise ValueError(f"kmeans_rows(fused=True): 1 ... {KMEANS_FUSED_MAX_S} seedings, got {len(kinds)}")
        c0 = torch.stack([_init_centers(kind, x, xs, lo, span, n_clusters).expand(rows, n_clusters) for kind in kinds])
        del xs
        a, c, sse, iters = kmeans_rows_launch(x, shared_w if shared_w is not None else wts, c0, max_iter, tol)
        return (a, c, sse, iters) if return_stats else (a, c)
    for kind in ((init,) if isinstance(init, str) else tuple(init)):
        a, c, sse = _lloyd(x, wts, xw, _init_centers(kind, x, xs, lo, span, n_clusters), span, max_iter, tol)
        if best is None:
            best = [a, c, sse]
        else:
            better = sse < best[2]
            best[0] = torch.where(better[:, None], a, best[0])
            best[1] = torch.where(better[:, None], c, best[1])
            best[2] = torch.where(better, sse, best[2])
    return best[0].to(torch.int32), best[1]


# --------------------------------------------------------------------------------------------------
# any4 (quantize.py:523-637, 810-825)
# --------------------------------------------------------------------------------------------------

_SEEDINGS = ("uniform", "density", "quantile")
_WARNED_INIT: set = set()  # scikit-learn seeding names already warned about (kmeans_rows)


@torch.no_grad()
def anyq_quantize_tensor(W: torch.Tensor, n_bit: int = 4, q_group_size: int = 128, per_row: bool = True,
                         zero_point: bool = True, scale_only: bool = False, sample_weight=None,
                         scale_sample_weight: bool = False, abs_weight_sample_weight: bool = False,
                         init=("uniform", "density", "quantile"), max_iter: int = 300, device=None, fused: bool = False, **_):
    """-> (assign int32 [n][k], any4 LUT [n][2^n_bit] (or [2^n_bit] when per_row=False) in the group-scaled
    [0, 2^n_bit - 1] domain, scales_and_zeros [k/g][n][2]); LUT and scales in W's dtype, on W's device.
    `device` = where to do the work (default: W's device; pass "cuda" to cluster a CPU checkpoint on the GPU).
    `fused` = cluster with the HIP k-means kernel (kmeans_rows(fused=True): GPU only, rows of at most 16384 weights, so not
    per_row=False; ValueError otherwise); grouping, sample weights and seeding are the same torch code either way."""
    orig_device, dtype = W.device, W.dtype
    if device is not None:
        W = W.to(device)
    orig_shape = W.shape
    if not per_row:
        if q_group_size:
            Wg, _, sz = group_q(W, n_bit, q_group_size=q_group_size, assymetric=not scale_only, zero_point=zero_point)
            scales, _ = extract_scales_and_zeros(sz, Wg.shape, q_group_size)
        else:
            Wg, sz, scales = W.float(), None, None
        Wg = Wg.reshape(1, -1)
    elif q_group_size:
        Wg, _, sz = group_q(W, n_bit, q_group_size=q_group_size, assymetric=not scale_only, zero_point=zero_point)
        scales, _ = extract_scales_and_zeros(sz, Wg.shape, q_group_size)
    else:
        Wg = W.float()
        sz = pack_scales_and_zeros(torch.ones(W.shape[0], device=W.device), torch.zeros(W.shape[0], device=W.device), W.shape)
        scales = None
    sw = sample_weight
    if isinstance(sw, torch.Tensor):
        sw = sw.to(W.device, torch.float32)
    if scale_sample_weight and scales is not None:
        sw = (torch.ones_like(W[0], dtype=torch.float32) if sw is None else sw) * scales
    if abs_weight_sample_weight:
        sw = (torch.ones_like(W[0], dtype=torch.float32) if sw is None else sw) * W.abs().float()
    if sw is not None and not per_row:
        sw = sw.expand(orig_shape).reshape(1, -1) if sw.dim() == 1 else sw.reshape(1, -1)
    assign, any4 = kmeans_rows(Wg, n_clusters=2 ** n_bit, sample_weight=sw, max_iter=max_iter, init=init, fused=fused)
    if not per_row:
        assign = assign.reshape(orig_shape)
        any4 = any4.squeeze(0)
    return assign.to(orig_device), any4.to(orig_device, dtype), sz.to(orig_device, dtype)


def anyq_dequantize_tensor(assign, any4, scales_and_zeros, n_bit: int = 4, q_group_size: int = 128, per_row: bool = True,
                           scale_only: bool = False, **_):
    """(lut[code] - 2^(n_bit-1)) * scale + zero, evaluated op by op in the LUT's dtype (quantize.py:612-637)."""
    Wc = torch.gather(any4, 1, assign.long()) if per_row else any4[assign.long()]
    if not q_group_size:
        return Wc
    scales, zeros = extract_scales_and_zeros(scales_and_zeros, assign.shape, q_group_size)
    return degroup_q(Wc, scales=scales, zeros=zeros, n_bit=n_bit, q_group_size=q_group_size, centering=not scale_only)


def anyq_reconstruct_tensor(W, n_bit: int = 4, q_group_size: int = 128, per_row: bool = True, scale_only: bool = False, **kw):
    assign, any4, sz = anyq_quantize_tensor(W, n_bit=n_bit, q_group_size=q_group_size, per_row=per_row,
                                            scale_only=scale_only, **kw)
    return anyq_dequantize_tensor(assign, any4, sz, n_bit=n_bit, q_group_size=q_group_size, per_row=per_row,
                                  scale_only=scale_only)


# --------------------------------------------------------------------------------------------------
# module level (quantize.py:32-85, 333-391, 827-905)
# --------------------------------------------------------------------------------------------------

def anyq_layer(module: torch.nn.Module, name: str = "", n_bit: int = 4, group_size: int = 128, per_row: bool = True,
               scale_only: bool = False, sample_weight=None, pseudo: Optional[bool] = None,
               kernel: str = "linear_y_f16RM_x_f16RM_W_any4TC", w_inner_k: int = 4, **kwargs) -> torch.nn.Module:
    """nn.Linear -> Any4Linear on the HIP kernels (pseudo=False, default) or the same nn.Linear with
    reconstructed weights (pseudo=True: fake quantization for accuracy studies)."""
    if pseudo is None:
        pseudo = n_bit != 4
    w = module.weight
    if isinstance(sample_weight, dict):
        sample_weight = sample_weight[name]
    if pseudo:
        w_deq = anyq_reconstruct_tensor(w, n_bit=n_bit, q_group_size=group_size, per_row=per_row, scale_only=scale_only,
                                        sample_weight=sample_weight, **kwargs)
        module.weight.data = w_deq.to(device=w.device, dtype=w.dtype)
        return module
    if n_bit != 4:
        raise ValueError(f"No quantized module for n_bit={n_bit}; use pseudo=True")
    from .modules import Any4Linear  # needs the HIP library: loud ImportError otherwise

    codes, lut, sz = anyq_quantize_tensor(w, n_bit=n_bit, q_group_size=group_size, per_row=per_row, scale_only=scale_only,
                                          sample_weight=sample_weight, **kwargs)
    q = Any4Linear(module.in_features, module.out_features, bias=module.bias is not None, device=w.device, dtype=w.dtype,
                   group_size=group_size if group_size else w.shape[1], per_row=per_row, kernel=kernel, w_inner_k=w_inner_k)
    q.weight.data = codes.to(w.device)
    q.scales_and_zeros.data = sz.to(w.device)
    q.lut.data = lut.to(w.device) - (2 ** (n_bit - 1))  # the kernel's LUT is centred (quantize.py:893)
    q.bias = module.bias
    q.reshape_weight(w_inner_k)
    return q


def tune_quant_params(module: torch.nn.Module, X: torch.Tensor, Y: torch.Tensor, steps: int = 100, lr: float = 1e-3,
                      params=("lut", "scales_and_zeros")):
    """The reference's learn_anyq (quantize.py:648-806) with objective `Y_mse`, run on the real kernels: Adam on the parameters named in
    `params` of a packed Int4Linear / Any4Linear / NF4Linear against loss = mean((module(X) - Y)^2), the codes frozen.  The optimiser
    works on f32 masters; each step rounds them into the module's 16-bit parameters, runs the module's forward and takes the f32
    gradients of the dq op (torch.ops.tinygemm.tinygemm_dq_*) for dLoss/dY.  Returns (loss_before, loss_after) of the module as it was
    handed in / as it is left."""
    from . import ops as _ops

    if getattr(module, "_DQ_OP", None) is None or module.kernel not in module._DX_KERNELS or not module.weight_reshaped:
        raise ValueError("tune_quant_params needs a packed int4 / any4 module on a row-major kernel")
    if module.weight_format == "reference":
        raise RuntimeError(_ops._RELAYOUT_HINT)
    names = tuple(params)
    if not names or any(n not in ("lut", "scales_and_zeros") or getattr(module, n, None) is None for n in names):
        raise ValueError(f"params must name parameters of the module out of ('lut', 'scales_and_zeros'), got {params!r}")
    dq_op = getattr(torch.ops.tinygemm, module._DQ_OP).default
    on_right = module._DX_KERNELS[module.kernel]
    x2d, y2d = X.reshape(-1, X.shape[-1]), Y.reshape(-1, Y.shape[-1])
    masters = {n: getattr(module, n).detach().float().clone().requires_grad_(True) for n in names}
    opt = torch.optim.Adam(list(masters.values()), lr=lr)

    def loss_and_dy():
        with torch.no_grad():
            diff = module(x2d).float() - y2d.float()
            return float(diff.pow(2).mean()), (diff * (2.0 / diff.numel())).to(x2d.dtype)

    loss_before, dy = loss_and_dy()
    loss_after = loss_before
    for _ in range(steps):
        lut = module.lut if hasattr(module, "lut") else None
        extra = () if lut is None else (lut,)
        out = dq_op(x2d, dy, module.weight, module.group_size, module.scales_and_zeros, *extra, on_right)
        grads = {"scales_and_zeros": out if lut is None else out[0], "lut": None if lut is None else out[1]}
        for n in names:
            masters[n].grad = grads[n]
        opt.step()
        with torch.no_grad():
            for n in names:
                getattr(module, n).copy_(masters[n])   # (one rounding to the parameter's 16-bit type; in place: a recorded plan stays valid)
        loss_after, dy = loss_and_dy()
    return loss_before, loss_after


def intq_layer(module: torch.nn.Module, name: str = "", n_bit: int = 4, group_size: int = 128, pseudo: Optional[bool] = None,
               **kwargs) -> torch.nn.Module:
    """nn.Linear -> Int4Linear (uniform int4 on tinygemm's grid) or, pseudo=True, reconstructed weights in place."""
    if pseudo is None:
        pseudo = n_bit not in (4, 8)
    w = module.weight
    if pseudo:
        module.weight.data = intq_reconstruct_tensor(w, n_bit=n_bit, q_group_size=group_size, **kwargs).to(device=w.device, dtype=w.dtype)
        return module
    if n_bit == 8:  # quantize.py:337-360 builds Int8Linear from group_quantize_tensor(n_bit=8)
        from .modules import Int8Linear
        from .utils import group_quantize_tensor

        codes, sz = group_quantize_tensor(w, n_bit=8, q_group_size=group_size)
        q = Int8Linear(module.in_features, module.out_features, bias=module.bias is not None, device=w.device, dtype=w.dtype,
                       group_size=group_size)
        q.weight.data = codes.to(w.device)
        q.scales_and_zeros.data = sz.to(w.device)
        q.bias = module.bias
        q.reshape_weight()
        return q
    if n_bit != 4:
        raise ValueError(f"No int quantized module built for n_bit={n_bit}; use pseudo=True")
    from .modules import Int4Linear

    codes, _, sz = intq_quantize_tensor(w, n_bit=n_bit, q_group_size=group_size, new_grouping="tinygemm")
    q = Int4Linear(module.in_features, module.out_features, bias=module.bias is not None, device=w.device, dtype=w.dtype,
                   group_size=group_size)
    q.weight.data = codes.to(w.device)
    q.scales_and_zeros.data = sz.to(w.device)
    q.bias = module.bias
    q.reshape_weight()
    return q


@torch.no_grad()
def nf4_quantize_tensor(W: torch.Tensor, q_group_size: int = 128):
    """NormalFloat4 with absmax group scaling (what bitsandbytes' quantize_nf4 does, quantize.py:923-937 uses it for the
    pseudo path): -> (int32 codes [n][k], lut [16] = NF4 code book, scales_and_zeros [k/g][n][(absmax, 0)])."""
    from .modules import NF4_VALUES

    n, k = W.shape
    grp = W.float().reshape(-1, q_group_size)
    absmax = grp.abs().amax(dim=1, keepdim=True).clamp_min(1e-12)
    book = torch.tensor(NF4_VALUES, device=W.device, dtype=torch.float32)
    mid = ((book[1:] + book[:-1]) * 0.5).contiguous()
    codes = torch.searchsorted(mid, (grp / absmax).contiguous()).to(torch.int32).reshape(n, k)
    sz = pack_scales_and_zeros(absmax, torch.zeros_like(absmax), W.shape)
    return codes, book.to(W.dtype), sz.to(W.dtype)


def nf4_layer(module: torch.nn.Module, name: str = "", n_bit: int = 4, group_size: int = 128, pseudo: Optional[bool] = None,
              kernel: str = "linear_y_f16RM_x_f16RM_W_any4TC", w_inner_k: int = 4, **_) -> torch.nn.Module:
    """nn.Linear -> NF4Linear (real kernels) or fake-quantized weights in place (pseudo=True)."""
    assert n_bit == 4, "nf4 only supports 4-bit"
    w = module.weight
    codes, lut, sz = nf4_quantize_tensor(w, q_group_size=group_size)
    if pseudo:
        s, _ = extract_scales_and_zeros(sz.float(), w.shape, group_size)
        module.weight.data = (lut.float()[codes.long()] * s).to(w.dtype)
        return module
    from .modules import NF4Linear

    q = NF4Linear(module.in_features, module.out_features, bias=module.bias is not None, device=w.device, dtype=w.dtype,
                  group_size=group_size, kernel=kernel, w_inner_k=w_inner_k)
    q.weight.data, q.scales_and_zeros.data, q.bias = codes.to(w.device), sz.to(w.device), module.bias
    q.reshape_weight(w_inner_k)
    return q


def mx4_layer(module: torch.nn.Module, name: str = "", group_size: int = 32, pseudo: Optional[bool] = None,
              kernel: str = "linear_y_f16RM_x_f16RM_W_mx4TC", w_inner_k: int = 4, **_) -> torch.nn.Module:
    """nn.Linear (bf16) -> MX4Linear, or fake-quantized weights in place (pseudo=True)."""
    from .utils import dequantize_mx4, quantize_mx4

    w = module.weight
    codes, exps = quantize_mx4(w.float(), group_size)
    if pseudo:
        module.weight.data = dequantize_mx4(codes, exps).to(w.dtype)
        return module
    from .modules import MX4Linear

    q = MX4Linear(module.in_features, module.out_features, bias=module.bias is not None, device=w.device, dtype=w.dtype,
                  group_size=group_size, kernel=kernel, w_inner_k=w_inner_k)
    q.weight.data, q.exponents.data, q.bias = codes.to(w.device), exps.to(w.device), module.bias
    q.reshape_weight(w_inner_k)
    return q


def quantize_model(model: torch.nn.Module, layer_from=torch.nn.Linear, layer_to: Callable = anyq_layer, skip_modules=None,
                   **kwargs) -> torch.nn.Module:
    """Replace every `layer_from` submodule by `layer_to(module, name=..., **kwargs)`, in place.
    skip_modules: names or modules to leave alone; default = the LM head when the model has one
    (`lm_head` attribute or `get_output_embeddings()`), as quantization papers do (quantize.py:34-36)."""
    if skip_modules is None:
        head = getattr(model, "lm_head", None)
        if head is None and hasattr(model, "get_output_embeddings"):
            head = model.get_output_embeddings()
        skip_modules = [] if head is None else [head]
    if isinstance(skip_modules, str):
        skip_modules = [s.strip() for s in skip_modules.split(",") if s.strip()]
    if isinstance(skip_modules, torch.nn.Module):
        skip_modules = [skip_modules]
    todo = [(n, m) for n, m in model.named_modules()
            if isinstance(m, layer_from) and n not in skip_modules and not any(m is s for s in skip_modules)]
    for name, module in todo:
        new = layer_to(module, name=name, **kwargs)
        parent = model.get_submodule(".".join(name.split(".")[:-1])) if "." in name else model
        setattr(parent, name.split(".")[-1], new)
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        gc.collect()
    return model
