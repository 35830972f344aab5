"""Sampling for the decode stack, defined in plain torch: the counter-based random numbers (Philox4x32-10), the uniform a sequence
draws at a given place, and temperature / top-k / top-p sampling of a row of logits in float64.

This is what `DecodeStack(fused=False)` runs and what the fused sampler (any4_amd/csrc/sample.cuh, `decode_ops.sample`) is tested
against -- the way `kvcache.mx8_encode` defines mx8.  Nothing here is on a hot path.
"""
from __future__ import annotations

import torch

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF


def _mulhilo(m: int, c: torch.Tensor):
    """(hi, lo) 32-bit halves of the 64-bit product m * c; c int64 in [0, 2^32).  In 16-bit pieces: the product itself would leave int64."""
    a, b = m * (c >> 16), m * (c & 0xFFFF)  # m * c = 2^16 a + b, both below 2^48
    x = a + (b >> 16)
    return x >> 16, ((x & 0xFFFF) << 16) | (b & 0xFFFF)


def philox4x32_10(counter4, key2) -> torch.Tensor:
    """Philox4x32 with 10 rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).  counter4 [..., 4], key2 [..., 2]:
    32-bit words held in int64 (anything `torch.as_tensor` takes); returns the four output words, int64 [..., 4]."""
    c = torch.as_tensor(counter4, dtype=torch.int64) & _MASK32
    k = torch.as_tensor(key2, dtype=torch.int64) & _MASK32
    c0, c1, c2, c3 = c.unbind(-1)
    k0, k1 = k.unbind(-1)
    for _ in range(10):
        hi0, lo0 = _mulhilo(PHILOX_M0, c0)
        hi1, lo1 = _mulhilo(PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + PHILOX_W0) & _MASK32, (k1 + PHILOX_W1) & _MASK32
    return torch.stack((c0, c1, c2, c3), dim=-1)


def uniform(seed, ctr) -> torch.Tensor:
    """The uniform a sequence with seed `seed` draws for the token that gets index `ctr` in it (int64 each, broadcast against each other):
    key = the seed's two 32-bit halves, counter = (ctr's two halves, 0, 0), u = (first output word >> 8) * 2^-24 -- float32, exact, in
    [0, 1).  It depends on nothing else: not on the batch slot, not on the rest of the batch, not on how often a graph was replayed."""
    seed, ctr = torch.broadcast_tensors(torch.as_tensor(seed, dtype=torch.int64), torch.as_tensor(ctr, dtype=torch.int64))
    zero = torch.zeros_like(ctr)
    out = philox4x32_10(torch.stack((ctr & _MASK32, (ctr >> 32) & _MASK32, zero, zero), dim=-1),
                        torch.stack((seed & _MASK32, (seed >> 32) & _MASK32), dim=-1))
    return (out[..., 0] >> 8).to(torch.float32) * 2.0 ** -24


def sample_ref(logits: torch.Tensor, temperature, top_k, top_p, u) -> torch.Tensor:
    """The definition.  logits [bs, V] (any float type; evaluated in float64), temperature / top_k / top_p / u: [bs] each -> int64 [bs].
    Per row, with the tokens ranked by (logit descending, index ascending): temperature == 0 gives rank 0 (argmax, lowest index among
    ties; u unused).  Otherwise w_i = exp((l_i - l_max) / temperature); top-k keeps the first top_k ranks (<= 0 or >= V: all), Z_k their
    mass; top-p keeps of those the shortest rank prefix whose mass is >= top_p * Z_k (>= 1: all; at least one token), Z its mass; the
    answer is the first kept rank whose inclusive cumulative mass exceeds u * Z -- the last kept rank if rounding leaves none.  A -inf
    logit has weight 0 and is never returned.  Out of contract: NaN logits, +inf logits (inf - inf is NaN here as in the kernel), a row that
    is all -inf, temperature < 0."""
    bs, V = logits.shape
    dev = logits.device
    temperature, top_p, u = [torch.as_tensor(x, device=dev).reshape(-1).to(torch.float64) for x in (temperature, top_p, u)]
    top_k = torch.as_tensor(top_k, device=dev).reshape(-1).to(torch.int64)
    out = torch.empty(bs, dtype=torch.int64, device=dev)
    rows = max(1, (1 << 22) // V)  # rows per pass: the float64 copies of a pass stay small
    for b0 in range(0, bs, rows):
        sl = slice(b0, min(b0 + rows, bs))
        vals, order = torch.sort(logits[sl].detach().to(torch.float64), dim=1, descending=True, stable=True)
        T, k = temperature[sl, None], top_k[sl, None]
        k = torch.where((k <= 0) | (k >= V), V, k)
        w = torch.exp((vals - vals[:, :1]) / torch.where(T == 0, 1.0, T))
        cum = torch.cumsum(torch.where(torch.arange(V, device=dev)[None, :] < k, w, 0.0), 1)  # (constant = Z_k from rank k - 1 on)
        nucleus = torch.searchsorted(cum, top_p[sl, None] * cum[:, -1:], right=False) + 1
        kept = torch.where(top_p[sl, None] < 1, torch.minimum(nucleus, k), k)
        r = torch.searchsorted(cum, u[sl, None] * cum.gather(1, kept - 1), right=True)
        r = torch.where(T == 0, 0, torch.minimum(r, kept - 1))
        out[sl] = order.gather(1, r).squeeze(1)
    return out
