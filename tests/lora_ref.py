"""Float64 reference of the two LoRA stages (dg_lora_shrink, dg_lora_expand; any4_amd/lora.py: lora_ref is the torch definition) and its
error bound.  A plain helper module (not a conftest), in the style of tests/fused_ref.py; tests/test_lora_cpu.py checks it on the CPU,
tests/test_gpu_lora.py runs the kernels against it.

Row i takes adapter a = idx[i // rows_per_id]; an id outside [0, n_adapters) means no adapter (t = 0, y keeps its bits).

  t[i][j]  = rs_i sum_c A[a][j][c] x~[i][c]          x~ = x, rs = 1 without a norm weight; with g: x~ = RNE16(x g) (ONE rounding: the product of
                                                     two 16-bit numbers is exact in f32), rs = rsqrt(mean(x^2) + eps) -- the "sum" convention
  ref[i][c] = y_in[i][c] + scale[a] sum_j B[a][c][j] t[i][j]          and the kernel answers RNE16 of its f32 value of that.

Bound (u = 2^-24, the unit roundoff of f32; nothing here is fitted to a kernel's output):

  tol = 1/2 ulp16(ref) + u ((k + r + C) scale D + |y_in|) [+ 2^-18 scale D with a norm weight],
        D[i][c] = sum_j |B[a][c][j]| S[i][j],   S[i][j] = rs_i sum_c |A[a][j][c] x~[i][c]|

  * shrink: a sum of k exact products (fused multiply-adds: the product is not rounded) added in ANY order carries at most (k - 1) u S:
    each of the k - 1 additions rounds a partial sum that is at most S in magnitude.  The kernel's order (a lane's chain, the wave sum,
    eight partials in LDS) is one such order.
  * expand: r more additions on sum_j |B t| <= D, so r u D, and the shrink's error enters through |B|: (k - 1) u D.
  * the store: f32(y) + scale x sum is ONE fused multiply-add, rounded once: u (|y_in| + scale D).  Then RNE16: half an ulp16 -- of ref,
    not of the rounded value: were the f32 value on the other side of a power of two than ref, RNE16 gives that power of two, which is
    nearer to ref than the f32 value was.
  * C = 4: the store's share on the delta (1), the multiplication by rs (1), 1 / k as an f32 number inside rs is covered by the rs
    bracket, and the second-order terms ((k u)(r u) D and the like: below u D while k r < 2^24) (2).
  * rs: fused_ref.RS_REL = 2^-18, re-derived for this kernel's sum of squares: a pair as multiply + fused multiply-add (1 rounding on the
    path), a tree over the four pairs of a lane's 16 bytes (2), one addition per pass of 4096 elements (<= 32 for k <= 2^17, the
    kernel's limit), the wave sum (6), eight partials (8), times the f32 1 / k (2), plus eps (1): <= 52 roundings, within the 57 of that
    derivation (every term is positive: relative errors do not amplify); halved by the square root, plus rsqrtf's 2^-23: below 2^-19.
"""
import numpy as np
import torch

RS_REL = 2.0 ** -18
U32 = 2.0 ** -24
C_EXTRA = 4
EPS = 1e-5
BF16, F16 = torch.bfloat16, torch.float16


def ulp16(v, dtype):
    """One unit in the last place of the 16-bit type at |v| (float64 numpy; subnormals: the smallest spacing)."""
    v = np.abs(np.asarray(v, np.float64))
    mant, emin = (7, -126) if dtype == BF16 else (10, -14)
    e = np.floor(np.log2(np.maximum(v, 2.0 ** emin)))
    return np.exp2(np.maximum(e, emin) - mant)


def row_ids(idx, rows_per_id, m, n_adapters):
    """(adapter per row with -1 for none, int64 numpy [m])"""
    ids = np.repeat(np.asarray(idx, np.int64), rows_per_id)[:m]
    return np.where((ids >= 0) & (ids < n_adapters), ids, -1)


def shrink_ref64(x16, A16, idx, rows_per_id, g16=None, eps=EPS):
    """(t [m][r], S [m][r]) in float64 numpy; rows without an adapter: zeros."""
    m, k = x16.shape
    na, r, _ = A16.shape
    ids = row_ids(idx, rows_per_id, m, na)
    xt = x16 if g16 is None else (x16.float() * g16.float()[None, :]).to(x16.dtype)  # one rounding
    xt = xt.double().numpy()
    rs = np.ones(m)
    if g16 is not None:
        x = x16.double().numpy()
        rs = 1.0 / np.sqrt((x * x).mean(axis=1) + float(np.float32(eps)))
    A = A16.double().numpy()
    t, S = np.zeros((m, r)), np.zeros((m, r))
    for i in range(m):
        if ids[i] >= 0:
            t[i] = rs[i] * (A[ids[i]] @ xt[i])
            S[i] = rs[i] * (np.abs(A[ids[i]]) @ np.abs(xt[i]))
    return t, S


def lora_ref64(x16, A16, B16, scale32, idx, rows_per_id, y16, g16=None, eps=EPS):
    """(ref [m][n], tol [m][n], adapted [m] bool, t [m][r], t_tol [m][r]) in float64 numpy, from CPU tensors (scale32: float32 [n_adapters]).
    Rows without an adapter: ref = y_in, tol = 0 (their bits stay)."""
    m, k = x16.shape
    na, n, r = B16.shape
    ids = row_ids(idx, rows_per_id, m, na)
    t, S = shrink_ref64(x16, A16, idx, rows_per_id, g16, eps)
    y = y16.double().numpy()
    B = B16.double().numpy()
    sc = scale32.double().numpy()
    ref, D = y.copy(), np.zeros((m, n))
    for i in range(m):
        if ids[i] >= 0:
            ref[i] += sc[ids[i]] * (B[ids[i]] @ t[i])
            D[i] = abs(sc[ids[i]]) * (np.abs(B[ids[i]]) @ S[i])
    adapted = ids >= 0
    tol = 0.5 * ulp16(ref, y16.dtype) + U32 * ((k + r + C_EXTRA) * D + np.abs(y)) + (RS_REL * D if g16 is not None else 0.0)
    tol = np.where(adapted[:, None], tol, 0.0)
    t_tol = U32 * (k + C_EXTRA) * S + (RS_REL * S if g16 is not None else 0.0)
    return ref, tol, adapted, t, t_tol


def make_case(m, k, r, n, dtype, n_adapters=3, low_rank_slot=1, low_rank=3, seed=0):
    """Inputs of one float64 case (CPU tensors): x = 3 randn with row i scaled by 2^((i mod 5) - 2), g = 1 + 0.1 randn, A = randn / sqrt(k),
    B = randn / sqrt(r), scale = 2, 0.5, 1.25, ..., y = randn.  Slot `low_rank_slot` holds an adapter of rank `low_rank`, zero-padded."""
    gen = torch.Generator().manual_seed(seed * 7919 + 11)
    x = 3 * torch.randn(m, k, generator=gen) * torch.exp2((torch.arange(m) % 5 - 2).float())[:, None]
    g = 1 + 0.1 * torch.randn(k, generator=gen)
    A = torch.randn(n_adapters, r, k, generator=gen) / k ** 0.5
    B = torch.randn(n_adapters, n, r, generator=gen) / r ** 0.5
    A[low_rank_slot, low_rank:] = 0
    B[low_rank_slot, :, low_rank:] = 0
    scale = torch.tensor([2.0, 0.5, 1.25, 1.0][:n_adapters] + [1.0] * max(0, n_adapters - 4), dtype=torch.float32)
    y = torch.randn(m, n, generator=gen)
    return x.to(dtype), g.to(dtype), A.to(dtype), B.to(dtype), scale, y.to(dtype)
