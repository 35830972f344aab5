"""KV-cache formats and bookkeeping of the decode stack.  `PagePool` (at the end) is the host side of the paged cache: which pages of a
layer's pools are free and how many block-table entries point at each.

The `mx8` KV-cache format of the decode stack: block-scaled 8-bit rows (OCP MXFP8: E4M3 elements, one E8M0 exponent byte per 32
consecutive elements of a row).  Plain torch, CPU and GPU; `mx8_encode` IS the definition of the format -- the HIP writers
(dg_rope_attn_split_mx8, dg_prefill_attn_mx8 and their _seq forms) reproduce its bytes, the readers compute `mx8_decode`.

Per block of 32 elements (values taken as f32):
    amax = max|x| = m * 2^ex, m in [0.5, 1)                          (torch.frexp)
    e    = ex - 9 if m <= 0.875 else ex - 8                         the smallest power of two with amax / 2^e <= 448: nothing clips
    E    = clamp(e + 127, 0, 254); E = 0 for an all-zero block      the exponent byte
    code = RNE_e4m3(clamp(x * 2^(127 - E), -448, 448))              (torch's own cast turns 465 into NaN: the clamp is part of the format)
    a block with a non-finite element: E = 255, every code 0x7f, and it decodes to NaN in all 32 places
    decode = code * 2^(E - 127)
A decoded value has four significant bits, so it is exact in bf16; in fp16 it is exact while it lies inside fp16's range (a stack in
fp16 whose |k|, |v| go beyond that range is out of contract).  Blocks whose maximum is below 2^-100 are out of contract as well: the
kernels may flush what they decode to zero there.  Encoding decoded values again may pick an exponent one lower -- other bytes, the
same values.
"""
from __future__ import annotations

import torch

BLOCK = 32
F8 = torch.float8_e4m3fn


def _blocks(d: int) -> int:
    if d < BLOCK or d % BLOCK:
        raise ValueError(f"mx8 needs rows of a multiple of {BLOCK} elements, got {d}")
    return d // BLOCK


def mx8_encode(x: torch.Tensor):
    """x [..., d] (d % 32 == 0) -> (codes float8_e4m3fn [..., d], exps uint8 [..., d / 32])."""
    nb = _blocks(x.shape[-1])
    xf = x.float().reshape(*x.shape[:-1], nb, BLOCK)
    finite = torch.isfinite(xf).all(-1)
    amax = torch.where(finite, xf.abs().amax(-1), torch.ones((), device=x.device))
    m, ex = torch.frexp(amax)
    E = (ex.to(torch.int32) - 9 + (m > 0.875).to(torch.int32) + 127).clamp(0, 254)
    E = torch.where(amax == 0, torch.zeros_like(E), E)
    scale = ((254 - E) << 23).view(torch.float32)  # 2^(127 - E), exact
    codes = (xf * scale.unsqueeze(-1)).clamp(-448.0, 448.0).to(F8).view(torch.uint8)
    codes = torch.where(finite.unsqueeze(-1), codes, torch.full_like(codes, 0x7F))
    E = torch.where(finite, E, torch.full_like(E, 255))
    return codes.reshape(x.shape).view(F8), E.to(torch.uint8)


def mx8_scale(exps: torch.Tensor) -> torch.Tensor:
    """2^(E - 127) as float32 (E = 0: 2^-127, a denormal; E = 255: NaN), the shape of `exps`."""
    E = exps.to(torch.int32)
    bits = torch.where(E == 0, torch.full_like(E, 0x00400000), E << 23)
    return torch.where(E == 255, torch.full_like(E, 0x7FC00000), bits).view(torch.float32)


def mx8_decode(codes: torch.Tensor, exps: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """(codes [..., d], exps [..., d / 32]) -> values [..., d] of `dtype`."""
    nb = _blocks(codes.shape[-1])
    if tuple(exps.shape) != tuple(codes.shape[:-1]) + (nb,) or exps.dtype != torch.uint8 or codes.dtype != F8:
        raise ValueError(f"mx8_decode: codes {codes.dtype} {tuple(codes.shape)} / exps {exps.dtype} {tuple(exps.shape)} do not belong together")
    vals = codes.float().reshape(*codes.shape[:-1], nb, BLOCK) * mx8_scale(exps).unsqueeze(-1)
    vals = torch.where((exps == 255).unsqueeze(-1), torch.full_like(vals, float("nan")), vals)
    return vals.reshape(codes.shape).to(dtype)


class PagePool:
    """The pages of a paged KV cache (DecodeStack(kv_pages=...)): a free list and a reference count per page.  Plain Python, no tensors --
    one pool serves every layer and, under tensor parallelism, every rank makes the same decisions.  A page is handed out with count 1;
    `retain` adds a holder (prefix sharing), `release` removes one, and a page nobody holds returns to the free list."""

    def __init__(self, num_pages: int):
        if int(num_pages) < 1:
            raise ValueError(f"a page pool needs at least one page, got {num_pages}")
        self.num_pages = int(num_pages)
        self.refs = [0] * self.num_pages
        self._free = list(range(self.num_pages - 1, -1, -1))  # (handed out from the end: page 0 first)

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def alloc(self, n: int) -> list:
        """`n` free pages, each now held once.  More than the free list has: RuntimeError, and nothing changes."""
        n = int(n)
        if n < 0:
            raise ValueError(f"alloc of {n} pages")
        if n > len(self._free):
            raise RuntimeError(f"KV page pool exhausted: {n} pages wanted, {len(self._free)} of {self.num_pages} free")
        ids = [self._free.pop() for _ in range(n)]
        for i in ids:
            self.refs[i] = 1
        return ids

    def _held(self, ids, what):
        ids = [int(i) for i in ids]
        for i in set(ids):
            if not 0 <= i < self.num_pages or self.refs[i] < max(1, ids.count(i) if what == "release" else 1):
                raise ValueError(f"{what} of page {i}, which is not held{' that often' if 0 <= i < self.num_pages and self.refs[i] else ''}")
        return ids

    def retain(self, ids) -> None:
        """One more holder for each of `ids` (pages that are held already)."""
        for i in self._held(ids, "retain"):
            self.refs[i] += 1

    def release(self, ids) -> None:
        """One holder fewer for each of `ids`; a page whose count drops to zero is free again."""
        for i in self._held(ids, "release"):
            self.refs[i] -= 1
            if self.refs[i] == 0:
                self._free.append(i)
