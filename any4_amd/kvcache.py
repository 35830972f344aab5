"""KV-cache formats and bookkeeping of the decode stack.  `KVCache` is a layer's cache: the one place that knows its storage (16-bit or
mx8 rows, contiguous or page pools) and which attention kernel goes with it; `check_cache_config` is the one copy of its rules.
`PagePool` (at the end) is the host side of the paged cache: which pages of a layer's pools are free and how many block-table entries
point at each.

The `mx8` KV-cache format of the decode stack: block-scaled 8-bit rows (OCP MXFP8: E4M3 elements, one E8M0 exponent byte per 32
consecutive elements of a row).  Plain torch, CPU and GPU; `mx8_encode` IS the definition of the format -- the HIP writers
(the DG_ATTN_MX8 flavours of dg_attn_launch) reproduce its bytes, the readers compute `mx8_decode`.

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

import math
import operator

import torch

from . import _lib, decode_ops as G  # (binds nothing of the library until a kernel is launched)

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


def check_cache_config(cfg, kv_cache=None, kv_pages=None, page_size=64, mx8_attention="split") -> None:
    """The rules of a layer's KV cache (`cfg`: head_dim and max_seq), in the order they are refused.  A paged cache (include/
    decode_glue_hip.h): a page is a power of two of at least 64 positions, max_seq whole pages.  kv_cache: None or "mx8", which needs
    head_dim % 32 == 0.  mx8_attention names the decode attention kernel of an mx8 cache: "split" (the default) or "online", which only
    such a cache takes."""
    if kv_pages is not None:
        if kv_cache == "mx8" and cfg.head_dim not in (64, 128):  # (fused or not: the only head sizes for which a kernel reads such pools)
            raise ValueError(f"kv_pages with kv_cache='mx8': paged mx8 pools are not built yet for head_dim {cfg.head_dim} (64 and 128 are)")
        ps = operator.index(page_size)
        if operator.index(kv_pages) < 1:
            raise ValueError(f"kv_pages must be at least 1, got {kv_pages}")
        if ps < 64 or ps & (ps - 1) or ps > cfg.max_seq or cfg.max_seq % ps:
            raise ValueError(f"page_size must be a power of two with 64 <= page_size <= max_seq = {cfg.max_seq} and max_seq % page_size == 0, got {ps}")
    if kv_cache not in (None, "mx8"):
        raise ValueError(f"kv_cache must be None (the stack's dtype) or 'mx8', got {kv_cache!r}")
    if kv_cache == "mx8" and cfg.head_dim % 32:
        raise ValueError(f"kv_cache='mx8' needs head_dim % 32 == 0, got {cfg.head_dim}")
    if mx8_attention not in ("split", "online"):
        raise ValueError(f"mx8_attention must be 'split' or 'online', got {mx8_attention!r}")
    if mx8_attention == "online" and kv_cache != "mx8":
        raise ValueError("mx8_attention='online' needs kv_cache='mx8' (a 16-bit cache takes the one-barrier kernel by itself)")


class KVCache(torch.nn.Module):
    """The KV cache of one decoder layer.  `k` / `v` hold the rows: [bs, kvl, max_seq, d], or with kv_pages the pools [kv_pages, kvl,
    page_size, d] that `table` (int32 [bs, max_seq / page_size], the stack's, shared by all layers) addresses.  kv_cache="mx8": they hold
    float8_e4m3fn codes and `k_exp` / `v_exp` (else None) one exponent byte per 32 elements, [..., d / 32].  `mx8`, `paged`: what it is.
    `table`, `scratch` and `nsplit` are the stack's to set (the split count of the fused decode attention and its scratch buffer); as
    built they are what a layer outside a stack has."""

    def __init__(self, cfg, kvl: int, bs: int, device, dtype, kv_cache=None, kv_pages=None, page_size: int = 64, mx8_attention: str = "split"):
        super().__init__()
        check_cache_config(cfg, kv_cache, kv_pages, page_size, mx8_attention)
        self.mx8, self.paged, self.mx8_attention = kv_cache == "mx8", kv_pages is not None, mx8_attention
        lead = (kv_pages, kvl, page_size) if self.paged else (bs, kvl, cfg.max_seq)
        for name in ("k", "v"):
            rows = torch.zeros(*lead, cfg.head_dim, device=device, dtype=torch.uint8 if self.mx8 else dtype)
            self.register_buffer(name, rows.view(F8) if self.mx8 else rows, persistent=False)
            exps = torch.zeros(*lead, cfg.head_dim // BLOCK, device=device, dtype=torch.uint8) if self.mx8 else None
            self.register_buffer(name + "_exp", exps, persistent=False)
        self.table, self.scratch, self.nsplit = None, None, 1

    @classmethod
    def over(cls, k, v, k_exp=None, v_exp=None) -> "KVCache":
        """A contiguous cache over tensors that exist: the arguments of decode.prefill_attention_torch, a paged cache's gathered twin."""
        kv = cls.__new__(cls)
        torch.nn.Module.__init__(kv)
        kv.mx8, kv.paged, kv.mx8_attention = k_exp is not None, False, "split"
        kv.k, kv.v, kv.k_exp, kv.v_exp = k, v, k_exp, v_exp
        kv.table, kv.scratch, kv.nsplit = None, None, 1
        return kv

    def tensors(self) -> list:
        """The two or four tensors it holds, float8 codes as their bytes (indexing and copies are not implemented for that dtype everywhere)."""
        return [t.view(torch.uint8) if t.dtype == F8 else t for t in (self.k, self.v, self.k_exp, self.v_exp) if t is not None]

    # ---- plain torch (the formulation the kernels are tested against; also the CPU path) ----
    def write(self, put, k_rows, v_rows) -> None:
        """New rows into a contiguous cache: `put(tensor, rows)` is the caller's addressing.  An mx8 cache: the rows are encoded, and `put`
        places the codes (as bytes) and the exponent bytes."""
        if not self.mx8:
            put(self.k, k_rows)
            put(self.v, v_rows)
            return
        for cache, exps, rows in ((self.k, self.k_exp, k_rows), (self.v, self.v_exp, v_rows)):
            codes, e = mx8_encode(rows)
            put(cache.view(torch.uint8), codes.view(torch.uint8))
            put(exps, e)

    def read(self, dtype, S=None):
        """(K, V) [bs, kvl, S, d] (default: every position) of a contiguous cache in `dtype`: mx8_decode of an mx8 cache."""
        if not self.mx8:
            return self.k[:, :, :S], self.v[:, :, :S]
        return mx8_decode(self.k[:, :, :S], self.k_exp[:, :, :S], dtype), mx8_decode(self.v[:, :, :S], self.v_exp[:, :, :S], dtype)

    def gathered(self):
        """The plain-torch twin of a paged cache (what the paged kernels are tested against, not a product): (cache, put) -- `cache` a
        contiguous KVCache [bs, kvl, max_seq, d] over copies gathered through the table, with entries outside the pool clamped to page 0
        as the kernels clamp them, so that the contiguous formulation runs unchanged (mx8 pools: codes AND exponent bytes);
        `put(slots, positions)` (two int64 tensors of one length) copies those rows of `cache` back into the pools, dropping a row whose
        own table entry is outside the pool.  A contiguous cache: (itself, None)."""
        if not self.paged:
            return self, None
        n, kvl, ps, _ = self.k.shape
        tab = self.table.long()
        valid = (tab >= 0) & (tab < n)
        idx = torch.where(valid, tab, torch.zeros_like(tab))
        held = [t for t in (self.k, self.v, self.k_exp, self.v_exp) if t is not None]
        pools = self.tensors()
        views = [pool[idx].permute(0, 2, 1, 3, 4).reshape(tab.shape[0], kvl, tab.shape[1] * ps, pool.shape[3]) for pool in pools]

        def put(slots, positions):
            ok = valid[slots, positions // ps]
            slots, positions = slots[ok], positions[ok]
            pages = tab[slots, positions // ps]
            for pool, view in zip(pools, views):
                pool[pages, :, positions % ps] = view[slots, :, positions]

        return KVCache.over(*[view.view(t.dtype) for view, t in zip(views, held)]), put

    # ---- fused: the one attention launch that goes with this cache (any4_amd/decode_ops.py) ----
    def decode_attention(self, qkv, pos, cos_tab, sin_tab, hl: int, per_sequence: bool = False):
        """One token per sequence at `pos` [1] (per_sequence: `pos` [bs], the _seq entry points): split over the sequence when the
        stack gave a scratch buffer, else the latency kernel (head_dim 64 / 128), else the general one.  An mx8 cache always takes an
        entry point with a scratch buffer (also at a split count of 1): the 256-thread split kernel's, or with mx8_attention="online"
        the one-barrier kernel's.  Pools behind the block table take the _paged entry points; mx8 pools the one _mx8_paged entry point
        (the one-barrier kernel, whatever mx8_attention names, with the stack's split count and scratch)."""
        k, v = self.k, self.v
        _, kvl, _, d = k.shape
        if self.paged and not per_sequence:
            raise RuntimeError("a paged KV cache has a position per sequence")
        if self.mx8 and self.scratch is None:  # (a layer built outside a stack; a stack sets the buffer when it is built)
            self.scratch = G.rope_attn_split_scratch((self.table if self.paged else k).shape[0], hl, d, self.nsplit, qkv.device)
        split = None if self.scratch is None else (self.scratch, self.nsplit)
        exps = (self.k_exp, self.v_exp) if self.mx8 else ()
        if self.mx8 and not self.paged and self.mx8_attention == "online":
            # (by its public name, the only launch made that way: tests/test_gpu_kv8_online.py counts the steps that go through it)
            return G.rope_attn_online_mx8(qkv, cos_tab, sin_tab, pos, k, v, *exps, hl, kvl, d, 1.0 / math.sqrt(d), *split,
                                          per_sequence=per_sequence)
        if split is None:
            kernel = _lib.DG_ATTN_ONLINE if d in (64, 128) else _lib.DG_ATTN_GENERAL
        else:
            kernel = _lib.DG_ATTN_SPLIT
        # (paged mx8 pools: the one-barrier kernel is the only decode kernel with that flavour)
        return G._rope_attn(kernel, qkv, cos_tab, sin_tab, pos, k, v, hl, kvl, d, 1.0 / math.sqrt(d), per_sequence, split=split, exps=exps,
                            table=self.table, one_barrier=self.mx8 and self.paged)

    def prefill_attention(self, qkv, pos, cos_tab, sin_tab, hl: int, T=None, lengths=None, slots=None, per_sequence: bool = False):
        """A chunk of T tokens per sequence (row b * T + t; default T = rows / the cache's batch), token 0 at `pos` [1]: T cache rows
        appended, causal.  per_sequence: `pos`, `lengths`, `slots` [n] on the device (DG_ATTN_SEQ); the context rows of tokens
        that do not exist are zero."""
        k, v = self.k, self.v
        _, kvl, _, d = k.shape
        if self.paged and (not per_sequence or T is None):
            raise RuntimeError("a paged KV cache has a position per sequence")
        T = qkv.shape[0] // k.shape[0] if T is None else T
        out = qkv.new_zeros(qkv.shape[0], hl * d) if per_sequence else None
        return G.prefill_attn(qkv, cos_tab, sin_tab, pos, k, v, hl, kvl, d, 1.0 / math.sqrt(d), T, out=out, lengths=lengths, slots=slots,
                              per_sequence=per_sequence, k_exp=self.k_exp, v_exp=self.v_exp, table=self.table)


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
