"""Decode harness around the quantized linears (BASELINE config 5): prompt prefill and one-token decode steps.

The reference measures model-level speed with `benchmark.py:113-215`: a HuggingFace causal LM, every
`nn.Linear` except the LM head swapped for the quantized module by `quantize_model` (quantize.py:32-85),
forward on random `input_ids[bs, seqlen]`.  Neither checkpoints nor the hub are reachable here, so this
module builds the same *shape* of work from scratch -- a Llama-architecture decoder (RMSNorm, rotary
embeddings, grouped-query attention over a static KV cache, SwiGLU MLP) with random-initialised weights of
the named configuration -- and runs ONE decode step (one new token per sequence) through it; `DecodeStack.prefill` feeds a whole
prompt (T tokens per sequence at once: the linears at bs * T rows, causal flash attention that appends T cache rows) so that the cache
holds a real context before a step is timed or tested, and `DecodeStack.generate` chains the two.  Everything
except the linears is plain torch (plumbing); the linears are whatever the `linear_factory` returns:
`Any4Factory` (the product: `Any4Linear` on the HIP kernels) or `DenseFactory` (bf16 `nn.Linear`, the
baseline the reference's README quotes speedups against).

Launch structure, chosen for the hardware rather than copied from HF:
  * q/k/v are ONE linear (rows concatenated: weight rows are independent units of the tinygemm path) and
    gate/up likewise -> 4 GEMM launches per layer instead of 7;
  * the whole step is captured in a hipGraph (`DecodeStack.capture`): at batch 1 a layer's GEMMs take a few
    microseconds each, so launch gaps would otherwise dominate;
  * `DecodeLayer` states the layer once per schedule -- plain torch (`forward`, `forward_prefill`), eight launches (`forward_fused`),
    five launches (`forward_fused5`: the element-wise stages ride in the GEMMs) -- and the fused schedules take the attention launch as
    an argument: `decode_attention` (one token per sequence) or `prefill_attention` (a chunk; so far on the eight launches only);
  * a layer's KV cache is one object, `DecodeLayer.kv` (any4_amd/kvcache.py: KVCache): it owns the tensors -- 16-bit or mx8 rows,
    contiguous or page pools --, reads and writes them for the plain-torch formulations, gathers a paged cache's contiguous twin, and
    picks the fused attention entry point from what it holds; the two attention fronts of the layer only hand over to it.  The stack
    owns what the layers share: the block table and the page pool, the split count and its scratch buffer;
  * one position model: a stack whose sequences share a position is the ragged one (`ragged=True`: a position per sequence) with every
    position equal, so `DecodeStack` has one step, one `decode` front, one prefill loop (positions, lengths and cache slots as host
    lists; a call that names none per sequence still launches the scalar attention on `prefill_pos`) and one `generate`.  What differs
    is which buffer the step reads (`pos` [1] or `pos_seq` [bs]) and which flavour of the attention launch it makes.  In plain torch the
    token's arithmetic is written once (`DecodeLayer._token_torch`) behind two addressings that are kept apart on purpose: `forward`
    (one rope row, `index_copy_`, one mask) and `forward_seq` (a row per sequence, gather / where / scatter, a mask per sequence) are
    compared bit for bit by tests/test_ragged_cpu.py, which is a check only while they are written independently;
  * LoRA adapters, one per sequence (`DecodeStack(..., adapters=AdapterSet)`, any4_amd/lora.py): every adapted linear is followed by a
    shrink and an expand launch that add the sequence's delta to the linear's output in place, in every schedule; which adapter a
    sequence takes is `adapter_ids`, a static buffer the kernels read, so a captured step serves another mix at every replay.  A stack
    built without `adapters=` has none of it;
  * tensor parallelism = row-sharding of every linear (any4_amd/shard.py): heads are split across ranks so
    attention and the KV cache stay local; per layer 4 all-gathers of [bs, n/G] partial outputs (attention
    output, o_proj, SwiGLU activation, down_proj) over RCCL.  One process per GPU.
"""
from __future__ import annotations

import math
import operator
import os
from dataclasses import dataclass
from functools import partial
from typing import Callable, Optional

import torch
import torch.distributed as dist

from .kvcache import KVCache, PagePool, check_cache_config


@dataclass
class DecodeConfig:
    hidden: int = 4096
    inter: int = 14336
    layers: int = 32
    heads: int = 32
    kv_heads: int = 8
    head_dim: int = 128
    vocab: int = 128256
    max_seq: int = 2048
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5
    group_size: int = 128
    # row order of the fused gate_up weight: 0 = [gate rows; up rows]; 8 = blocks of 8 gate rows followed by the 8 matching up
    # rows, the order the GEMM's fused SwiGLU epilogue wants (tg_w4_gemm.epilogue): a gate row and its up row then meet in one
    # 16-row tile of one workgroup.  `shard_rows` returns the row indices in this order, so a loader needs nothing else.
    gate_up_interleave: int = 0
    # mixture of experts (any4_amd/moe.py): 0 = a dense MLP (nothing changes anywhere); E > 0 = every layer holds E gate_up / down pairs and
    # a router, and a token runs `experts_per_token` of them.  Needs gate_up_interleave = 8 (the stacked experts' row order).
    experts: int = 0
    experts_per_token: int = 2
    # calls of the sparse MLP block with this many rows or more (a prompt) run the grouped path (any4_amd/moe.py: MoEMLP(grouped_from=...),
    # numerics of moe_grouped_ref); 0 = off: every call runs the GEMV launches in blocks of 8 rows
    moe_grouped_from: int = 0

    @classmethod
    def llama3_8b(cls, **kw) -> "DecodeConfig":
        return cls(**kw)

    @classmethod
    def llama2_7b(cls, **kw) -> "DecodeConfig":
        # the reference's default benchmark model (benchmark.py: --model-name meta-llama/Llama-2-7b-hf)
        return cls(hidden=4096, inter=11008, layers=32, heads=32, kv_heads=32, head_dim=128, vocab=32000,
                   rope_theta=10000.0, **kw)

    @classmethod
    def mixtral_8x7b(cls, **kw) -> "DecodeConfig":
        # the mixture-of-experts model of the reference's results table (README: Mixtral-8x7B-Instruct)
        kw = {**dict(hidden=4096, inter=14336, layers=32, heads=32, kv_heads=8, head_dim=128, vocab=32000, rope_theta=1e6, experts=8,
                     experts_per_token=2, gate_up_interleave=8), **kw}
        return cls(**kw)

    def linear_shapes(self):
        """(name, out_features, in_features) of the four fused linears of one layer."""
        qkv = (self.heads + 2 * self.kv_heads) * self.head_dim
        return [("qkv", qkv, self.hidden), ("o", self.hidden, self.heads * self.head_dim),
                ("gate_up", 2 * self.inter, self.hidden), ("down", self.hidden, self.inter)]

    def weight_bytes_4bit(self) -> int:
        """Algorithmic bytes one decode step streams through the quantized linears (bench.py formula, m=1)."""
        total = 0
        for name, n, k in self.linear_shapes():
            one = n * k // 2 + (k // self.group_size) * n * 4 + 32 * n + k * 2 + n * 2
            # (experts: a token streams the experts the router selected, and the 16-bit router)
            total += one * self.experts_per_token if self.experts and name in ("gate_up", "down") else one
        if self.experts:
            total += self.experts * self.hidden * 2
        return total * self.layers


def shard_rows(cfg: DecodeConfig, name: str, rank: int, world: int) -> torch.Tensor:
    """Row indices of the FULL fused weight `name` ("qkv" = [q; k; v] rows, "gate_up" = [gate; up] rows, "o",
    "down") that rank `rank` of `world` owns, in the order of its local weight.  Heads are split across ranks,
    so the local qkv is [q heads of the rank; k heads of the rank; v heads of the rank] and the local gate_up is
    [gate rows of the rank; up rows of the rank].  A checkpoint loader slices codes / LUT rows /
    scales_and_zeros[:, rows, :] with exactly these indices."""
    d = cfg.head_dim

    def span(base, total):
        per = total // world
        return torch.arange(base + rank * per, base + (rank + 1) * per)

    if name == "qkv":
        return torch.cat([span(0, cfg.heads * d), span(cfg.heads * d, cfg.kv_heads * d),
                          span((cfg.heads + cfg.kv_heads) * d, cfg.kv_heads * d)])
    if name == "gate_up":
        gate, up = span(0, cfg.inter), span(cfg.inter, cfg.inter)
        if cfg.gate_up_interleave:
            b = cfg.gate_up_interleave
            return torch.stack([gate.view(-1, b), up.view(-1, b)], dim=1).reshape(-1)
        return torch.cat([gate, up])
    if name in ("o", "down"):
        return span(0, cfg.hidden)
    raise ValueError(name)


# ---------------------------------------------------------------------------------------------------
# linear factories: (name, layer index, in_features, row ranges of the FULL weight owned by this rank) -> module
# ---------------------------------------------------------------------------------------------------

class Any4Factory:
    """Random any4 weights straight in the packed layout (no k-means, no packing pass): uniformly random
    nibbles are what packing uniformly random codes gives.  Per-row LUT, per-group scale/zero."""

    def __init__(self, cfg: DecodeConfig, device, dtype=torch.bfloat16, seed: int = 0, w_inner_k: int = 4,
                 kernel: str = "linear_y_f16RM_x_f16RM_W_any4TC"):
        from .modules import Any4Linear  # imports the HIP library; fails loudly without it

        self._cls = Any4Linear
        self.cfg, self.device, self.dtype, self.inner, self.kernel = cfg, device, dtype, w_inner_k, kernel
        self.gen = torch.Generator(device=device).manual_seed(seed)

    def __call__(self, name: str, layer: int, in_features: int, rows: int) -> torch.nn.Module:
        g, dev = self.cfg.group_size, self.device
        mod = self._cls(in_features, rows, bias=False, device=dev, dtype=self.dtype, group_size=g,
                        kernel=self.kernel, w_inner_k=self.inner, per_row=True)
        on_right = "x_f16RM_W" in self.kernel or "x_f16TC_W" in self.kernel
        if on_right:
            shape = (rows // 8, in_features // (16 * self.inner), 32, self.inner // 2)
        else:
            shape = (rows // 16, in_features // (16 * self.inner), 32, self.inner)
        w = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int64, device=dev, generator=self.gen)
        mod.weight.data = w.to(torch.int32)
        mod.weight_reshaped = True
        # keep activations O(1) through the stack: w ~ N(0, 1/k) after dequant
        std = 1.0 / math.sqrt(in_features)
        scales = torch.rand(in_features // g, rows, device=dev, generator=self.gen) * 0.4 + 0.8
        zeros = torch.randn(in_features // g, rows, device=dev, generator=self.gen) * 0.05
        mod.scales_and_zeros.data = (torch.stack([scales, zeros], dim=2) * std).to(self.dtype).contiguous()
        mod.lut.data = torch.randn(rows, 16, device=dev, generator=self.gen).to(self.dtype)
        return mod


class DenseFactory:
    """16-bit `nn.Linear` baseline (what benchmark.py times before quantize_model)."""

    def __init__(self, cfg: DecodeConfig, device, dtype=torch.bfloat16, seed: int = 0):
        self.cfg, self.device, self.dtype = cfg, device, dtype
        self.gen = torch.Generator(device=device).manual_seed(seed)

    def __call__(self, name: str, layer: int, in_features: int, rows: int) -> torch.nn.Module:
        lin = torch.nn.Linear(in_features, rows, bias=False, device=self.device, dtype=self.dtype)
        w = torch.randn(rows, in_features, device=self.device, generator=self.gen) / math.sqrt(in_features)
        lin.weight.data = w.to(self.dtype)
        lin.weight.requires_grad_(False)
        return lin


# ---------------------------------------------------------------------------------------------------
# the decoder
# ---------------------------------------------------------------------------------------------------

class RMSNorm(torch.nn.Module):
    def __init__(self, dim, eps, device, dtype):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(dim, device=device, dtype=dtype), requires_grad=False)
        self.eps = eps

    def forward(self, x):
        xf = x.float()
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps)
        return xf.to(x.dtype) * self.weight


def _rope_tables(cfg: DecodeConfig, device):
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, cfg.head_dim, 2, device=device, dtype=torch.float32) / cfg.head_dim))
    ang = torch.arange(cfg.max_seq, device=device, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.cos()], dim=-1), torch.cat([ang.sin(), ang.sin()], dim=-1)  # [S, d]


def _rope(x, cos, sin):
    # x [bs, h, d]; HF Llama convention: rotate_half over the two halves of the head dimension
    d2 = x.shape[-1] // 2
    rot = torch.cat([-x[..., d2:], x[..., :d2]], dim=-1)
    return (x.float() * cos + rot.float() * sin).to(x.dtype)


def prefill_attention_torch(qkv, cos_tab, sin_tab, p0: int, k_cache, v_cache, hl: int, kvl: int, d: int, T: int, k_exp=None, v_exp=None):
    """Plain-torch formulation of a prefill chunk's attention (what the prefill kernel, DG_ATTN_PREFILL of dg_attn_launch, is tested against; also the CPU path).
    qkv [bs * T, (hl + 2 kvl) d], row b * T + t = token t of sequence b at position p0 + t.  Ropes q and k with the table rows
    [p0, p0 + T), writes the T k / v rows into the caches and attends over cache[:, :, :p0 + T] with the mask s > p0 + t; rounding
    points as in DecodeLayer.forward: 16-bit score matmul, f32 scale + softmax, 16-bit probabilities, 16-bit P.V.
    k_exp / v_exp: the caches are mx8 (float8_e4m3fn codes with these exponent bytes) -- the rows are encoded on the way in, and the
    attention reads mx8_decode of the cache, the chunk's own rows included.
    Returns the context [bs * T, hl * d]."""
    bs, rep, S = qkv.shape[0] // T, hl // kvl, p0 + T
    rows = torch.arange(p0, S, device=qkv.device)
    cos, sin = cos_tab[p0:S].view(1, T, 1, d), sin_tab[p0:S].view(1, T, 1, d)
    q = _rope(qkv[:, : hl * d].reshape(bs, T, hl, d), cos, sin)
    k = _rope(qkv[:, hl * d: (hl + kvl) * d].reshape(bs, T, kvl, d), cos, sin)
    v = qkv[:, (hl + kvl) * d:].reshape(bs, T, kvl, d)
    kv = KVCache.over(k_cache, v_cache, k_exp, v_exp)
    kv.write(lambda cache, new: cache.index_copy_(2, rows, new), k.transpose(1, 2), v.transpose(1, 2))
    K, V = kv.read(qkv.dtype, S)
    qg = q.reshape(bs, T, kvl, rep, d).permute(0, 2, 3, 1, 4).reshape(bs, kvl, rep * T, d)
    att = torch.matmul(qg, K.transpose(2, 3)).float() * (1.0 / math.sqrt(d))  # [bs, kvl, rep * T, S]
    mask = torch.arange(S, device=qkv.device).view(1, S) > rows.view(T, 1)                    # [T, S]: s > p0 + t
    att = att.view(bs, kvl, rep, T, S).masked_fill(mask, float("-inf")).softmax(-1).to(qkv.dtype).view(bs, kvl, rep * T, S)
    ctx = torch.matmul(att, V)                                                                  # [bs, kvl, rep * T, d]
    return ctx.view(bs, kvl, rep, T, d).permute(0, 3, 1, 2, 4).reshape(bs * T, hl * d)


def prefill_attention_torch_seq(qkv, cos_tab, sin_tab, positions, lengths, slots, k_cache, v_cache, hl: int, kvl: int, d: int, T: int,
                                k_exp=None, v_exp=None):
    """prefill_attention_torch with a position, a length and a cache slot per sequence, all on the host (what its DG_ATTN_SEQ flavour is
    tested against; also the CPU path).  qkv [n * T, (hl + 2 kvl) d], rows padded to the common T: sequence i has `lengths[i]` tokens
    from position `positions[i]` on and lives in k_cache[slots[i]] / v_cache[slots[i]].  Every sequence gets its own rope rows, its
    own cache rows and its own mask; a padding row writes nothing, is seen by nobody and its context row is zero.  A batch in which
    nothing differs (equal positions, every length T, slot i for sequence i) IS prefill_attention_torch's batch and takes it."""
    n = qkv.shape[0] // T
    if n == k_cache.shape[0] and all(int(p) == int(positions[0]) for p in positions) and all(int(x) == T for x in lengths) and \
            [int(x) for x in slots] == list(range(n)):
        return prefill_attention_torch(qkv, cos_tab, sin_tab, int(positions[0]), k_cache, v_cache, hl, kvl, d, T, k_exp, v_exp)
    ctx = qkv.new_zeros(n, T, hl * d)
    rows = qkv.view(n, T, -1)
    for i in range(n):
        L, sl = int(lengths[i]), int(slots[i])
        if L > 0:
            exps = () if k_exp is None else (k_exp[sl: sl + 1], v_exp[sl: sl + 1])
            ctx[i, :L] = prefill_attention_torch(rows[i, :L], cos_tab, sin_tab, int(positions[i]), k_cache[sl: sl + 1], v_cache[sl: sl + 1],
                                                 hl, kvl, d, L, *exps)
    return ctx.view(n * T, hl * d)


def _scatter_rows(cache, pos, active, new):
    """cache[b, :, pos[b], :] = new[b] for the active sequences b, with `pos` [bs] (clamped into the cache) and `active` [bs] on the
    device: an inactive sequence gets its own row back, so nothing is read on the host and nothing of it changes."""
    idx = pos.view(-1, 1, 1, 1).expand(-1, cache.shape[1], 1, cache.shape[3])
    cache.scatter_(2, idx, torch.where(active.view(-1, 1, 1, 1), new.unsqueeze(2), cache.gather(2, idx)))


class DecodeLayer(torch.nn.Module):
    """One decoder layer: four fused linears, two norms and `kv`, its KV cache (any4_amd/kvcache.py: KVCache, the one place that knows
    what the cache looks like and which attention kernel goes with it).
    `k_cache`, `v_cache`, `k_exp`, `v_exp` (a contiguous cache's tensors) and `k_pool`, `v_pool`, `k_exp_pool`, `v_exp_pool` (a paged
    one's) are read-only views of `kv` for the test suites and the dev tools, each None where the layer has no such tensor; nothing in
    the package reads them.  A later change may move the suites to `layer.kv` and drop them."""

    k_cache, v_cache, k_exp, v_exp = (property(lambda self, n=n: None if self.kv.paged else getattr(self.kv, n)) for n in ("k", "v", "k_exp", "v_exp"))
    k_pool, v_pool, k_exp_pool, v_exp_pool = (property(lambda self, n=n: getattr(self.kv, n) if self.kv.paged else None)
                                              for n in ("k", "v", "k_exp", "v_exp"))

    def __init__(self, cfg: DecodeConfig, idx: int, factory: Callable, rank: int, world: int, device, dtype, bs: int,
                 kv_cache: Optional[str] = None, kv_pages: Optional[int] = None, page_size: int = 64, mx8_attention: str = "split"):
        """kv_cache: None = k / v rows in the layer's dtype; "mx8" = block-scaled 8-bit rows (any4_amd/kvcache.py): float8_e4m3fn codes
        in `kv.k` / `kv.v` and one exponent byte per 32 elements in `kv.k_exp` / `kv.v_exp` (both None for a 16-bit cache).
        mx8_attention: the fused decode attention of an mx8 cache -- "split" (the 256-thread split kernel) or "online" (the one-barrier
        kernel, head_dim 64 / 128); the plain-torch path is the same for both.  A paged mx8 layer (kv_pages) accepts either value and
        always runs the one-barrier kernel.
        kv_pages: a paged cache -- `kv.k` / `kv.v` are pools [kv_pages, kvl, page_size, d], addressed through `kv.table` int32 [bs,
        max_seq / page_size], the stack's (it is shared by all layers and set by the stack).  With kv_cache="mx8" (head_dim 64 / 128) four
        pools behind that table: the float8_e4m3fn codes and, in `kv.k_exp` / `kv.v_exp` uint8 [kv_pages, kvl, page_size, d / 32], the
        exponent bytes."""
        super().__init__()
        if cfg.heads % world or cfg.kv_heads % world or cfg.inter % (16 * world) or cfg.hidden % (16 * world):
            raise ValueError(f"heads={cfg.heads}, kv_heads={cfg.kv_heads}, inter={cfg.inter}, hidden={cfg.hidden} "
                             f"must split over world_size={world} in whole heads / 16-row tiles")
        self.cfg, self.world, self.idx = cfg, world, idx
        self.adapters = None  # the stack's AdapterSet (any4_amd/lora.py), set by the stack; None: no adapted linear, nothing changes
        self.hl, self.kvl = cfg.heads // world, cfg.kv_heads // world
        d = cfg.head_dim
        self.qkv = factory("qkv", idx, cfg.hidden, (self.hl + 2 * self.kvl) * d)
        self.o = factory("o", idx, cfg.heads * d, cfg.hidden // world)
        self.moe = None
        if cfg.experts:
            # E gate_up / down pairs from the factory, stacked (expert e at base + e * stride) and dropped; the router from its generator
            from .moe import MoEMLP, MoEWeights

            if world > 1:
                raise ValueError("experts with world > 1: tensor parallelism for experts is not built yet")
            if cfg.gate_up_interleave != 8:
                raise ValueError("experts need gate_up_interleave = 8 (the row order of the stacked gate / up weights)")
            gus = [factory("gate_up", idx, cfg.hidden, 2 * cfg.inter) for _ in range(cfg.experts)]
            downs = [factory("down", idx, cfg.inter, cfg.hidden) for _ in range(cfg.experts)]
            router = torch.randn(cfg.experts, cfg.hidden, device=device, generator=getattr(factory, "gen", None)) / math.sqrt(cfg.hidden)
            self.moe = MoEMLP(router.to(dtype), MoEWeights.from_linears(gus, downs), cfg.experts_per_token,
                              grouped_from=cfg.moe_grouped_from or None)
            self.gate_up = self.down = None
        else:
            self.gate_up = factory("gate_up", idx, cfg.hidden, 2 * cfg.inter // world)
            self.down = factory("down", idx, cfg.inter, cfg.hidden // world)
        self.norm1 = RMSNorm(cfg.hidden, cfg.rms_eps, device, dtype)
        self.norm2 = RMSNorm(cfg.hidden, cfg.rms_eps, device, dtype)
        self.kv = KVCache(cfg, self.kvl, bs, device, dtype, kv_cache, kv_pages, page_size, mx8_attention)  # (refuses what check_cache_config refuses)
        self.mx8_attention = mx8_attention
        # forward_fused5: which stages the library fused (None: not tried yet; set by the first step)
        self._fuse = {"norm1": None, "norm2": None, "mlp": None}

    def _adapted(self, lora, target, x, y, norm=None):
        """`y` = linear `target`'s output for the input `x`, plus the rows' adapter deltas (in place) when the call has adapters (`lora`: an
        any4_amd.lora.AdapterCall); norm: the RMSNorm the GEMM fused, when x is the un-normalised residual stream."""
        return y if lora is None else lora.apply(self.idx, target, x, y, norm)

    def _token_torch(self, kv, h, cos, sin, write, mask, gather, lora=None):
        """The plain-torch arithmetic of one token per sequence, behind either addressing (`forward`, `forward_seq`): `kv` the cache
        (a paged one's gathered twin), `cos` / `sin` the rope rows [1 | bs, 1, d], `write(cache, rows [bs, kvl, d])` puts the new k / v
        rows into a cache, `mask` [1 | bs, 1, 1, S] hides the cache rows behind each position.  Rounding points: 16-bit score matmul,
        f32 scale + softmax, 16-bit probabilities, 16-bit P.V (the formulation the fused schedules are tested against).  An mx8 cache:
        the rows are encoded on the way in and the attention reads mx8_decode of the cache, the new token's own rows included."""
        d, bs = self.cfg.head_dim, h.shape[0]
        xn = self.norm1(h)
        qkv = self._adapted(lora, "qkv", xn, self.qkv(xn))
        q = _rope(qkv[:, : self.hl * d].reshape(bs, self.hl, d), cos, sin)
        k = _rope(qkv[:, self.hl * d: (self.hl + self.kvl) * d].reshape(bs, self.kvl, d), cos, sin)
        v = qkv[:, (self.hl + self.kvl) * d:].reshape(bs, self.kvl, d)
        kv.write(write, k, v)
        K, V = kv.read(h.dtype)
        rep = self.hl // self.kvl
        qg = q.reshape(bs, self.kvl, rep, d)
        att = torch.matmul(qg, K.transpose(2, 3)).float() * (1.0 / math.sqrt(d))  # [bs, kvl, rep, S]
        att = att.masked_fill(mask, float("-inf")).softmax(-1).to(h.dtype)
        ctx = gather(torch.matmul(att, V).reshape(bs, self.hl * d))
        return self._mlp_torch(h + gather(self._adapted(lora, "o", ctx, self.o(ctx))), gather, lora)

    def forward(self, h, pos, cos_tab, sin_tab, arange, gather, lora=None):
        """Plain torch, one token per sequence, every sequence at `pos` [1] on the device: one rope row, one cache row and one mask
        for the batch."""
        cos, sin = cos_tab.index_select(0, pos).view(1, 1, -1), sin_tab.index_select(0, pos).view(1, 1, -1)
        return self._token_torch(self.kv, h, cos, sin, lambda cache, new: cache.index_copy_(2, pos, new.unsqueeze(2)),
                                 (arange > pos).view(1, 1, 1, -1), gather, lora)

    def forward_seq(self, h, pos, cos_tab, sin_tab, arange, gather, lora=None):
        """`forward` with a position per sequence: `pos` int64 [bs] on the device.  Sequence b takes rope row pos[b], writes cache row
        pos[b] and sees rows <= pos[b]; one whose position is outside [0, max_seq) is inactive: its caches keep their bits (its row of
        the result is unspecified).  No value is read on the host.
        A paged layer runs the same formulation on a contiguous cache gathered through the block table and puts the written rows back
        into the pools (`KVCache.gathered`; that path does read a mask on the host)."""
        d, bs = self.cfg.head_dim, h.shape[0]
        active = (pos >= 0) & (pos < self.cfg.max_seq)
        pc = pos.clamp(0, self.cfg.max_seq - 1)
        cos, sin = cos_tab.index_select(0, pc).view(bs, 1, d), sin_tab.index_select(0, pc).view(bs, 1, d)
        kv, put = self.kv.gathered()
        out = self._token_torch(kv, h, cos, sin, lambda cache, new: _scatter_rows(cache, pc, active, new),
                                arange.view(1, 1, 1, -1) > pc.view(bs, 1, 1, 1), gather, lora)
        if put is not None:
            put(torch.arange(bs, device=pos.device)[active], pc[active])
        return out

    def forward_prefill(self, h, positions, lengths, slots, T: int, cos_tab, sin_tab, gather, lora=None):
        """Plain torch, a chunk of tokens per sequence: `h` [n * T, hidden] (row i * T + t), rows padded to the common T.  Host ints
        per sequence: token 0 of sequence i at `positions[i]`, `lengths[i]` tokens, cache slot `slots[i]`.  Each sequence's k / v rows
        are appended to its caches and every token attends causally over cache + chunk (a batch in which nothing differs: in one
        batched formulation, prefill_attention_torch).  A paged layer: on its gathered twin, as forward_seq."""
        kv, put = self.kv.gathered()
        xn = self.norm1(h)
        ctx = prefill_attention_torch_seq(self._adapted(lora, "qkv", xn, self.qkv(xn)), cos_tab, sin_tab, positions, lengths, slots, kv.k, kv.v,
                                          self.hl, self.kvl, self.cfg.head_dim, T, kv.k_exp, kv.v_exp)
        if put is not None:
            rows = [(sl, p + t) for p, n, sl in zip(positions, lengths, slots) for t in range(n)]
            put(*[torch.tensor([r[i] for r in rows], dtype=torch.long, device=h.device) for i in (0, 1)])
        ctx = gather(ctx)
        return self._mlp_torch(h + gather(self._adapted(lora, "o", ctx, self.o(ctx))), gather, lora)

    def _mlp_torch(self, h, gather, lora=None):
        """The plain-torch MLP block behind either attention: h + down(silu(gate) * up) of norm2(h)."""
        xn = self.norm2(h)
        if self.moe is not None:
            return self.moe(xn, residual=h, fused=False)
        gu = self._split_gate_up(self._adapted(lora, "gate_up", xn, self.gate_up(xn)))
        il = self.cfg.inter // self.world
        act = gather(torch.nn.functional.silu(gu[:, :il]) * gu[:, il:])
        return h + gather(self._adapted(lora, "down", act, self.down(act)))

    # ---- the attention launch handed to forward_fused / forward_fused5: RoPE, KV write, attention over the cache; qkv -> context.
    # Which entry point that is follows from what the cache is: KVCache.decode_attention / prefill_attention
    def decode_attention(self, qkv, pos, cos_tab, sin_tab, per_sequence: bool = False):
        """One token per sequence at `pos` [1] (per_sequence: `pos` [bs], the _seq entry points)."""
        return self.kv.decode_attention(qkv, pos, cos_tab, sin_tab, self.hl, per_sequence)

    def prefill_attention(self, qkv, pos, cos_tab, sin_tab, T: Optional[int] = None, lengths=None, slots=None, per_sequence: bool = False):
        """A chunk of T tokens per sequence (row b * T + t; default T = rows / the cache's batch), token 0 at `pos` [1]: T cache rows
        appended, causal.  per_sequence: `pos`, `lengths`, `slots` [n] on the device."""
        return self.kv.prefill_attention(qkv, pos, cos_tab, sin_tab, self.hl, T, lengths, slots, per_sequence)

    def forward_fused(self, h, delta, attention, pos, cos_tab, sin_tab, gather, lora=None):
        """Same layer on the HIP glue kernels (include/decode_glue_hip.h): 4 launches + 4 GEMMs, for one token or a prefill chunk
        (the linears are called as modules, so the library routes them by row count).  `h` is the residual stream (updated in
        place), `delta` the previous layer's not-yet-added MLP output; returns (h, this layer's delta)."""
        from . import decode_ops as G

        h, y = G.add_rmsnorm(h, delta, self.norm1.weight, self.norm1.eps)
        ctx = gather(attention(self._adapted(lora, "qkv", y, self.qkv(y)), pos, cos_tab, sin_tab))
        h, y = G.add_rmsnorm(h, gather(self._adapted(lora, "o", ctx, self.o(ctx))), self.norm2.weight, self.norm2.eps)
        if self.moe is not None:  # route, gate_up, down: the block's output is the layer's delta
            return h, self.moe(y)
        act = gather(G.swiglu(self._split_gate_up(self._adapted(lora, "gate_up", y, self.gate_up(y))).contiguous()))
        return h, gather(self._adapted(lora, "down", act, self.down(act)))

    # ---- five launches per layer: every element-wise stage rides in a GEMM launch (tg_w4_gemm ABI 5) ----
    def _w4(self, lin, x, **kw):
        """`lin` (an Any4Linear / Int4Linear with Bint4 weights) through ops.w4_linear_fused; None if the library has no kernel
        with the requested stages for this problem."""
        from . import ops

        lut = getattr(lin, "lut", None)
        return ops.w4_linear_fused(x, lin.weight, lin.group_size, lin.scales_and_zeros, lut, **kw)

    def _try_fused(self, stage, lin, x, **kw):
        """_w4 for a stage the library may not be able to fuse: its first answer settles `_fuse[stage]`, and a stage settled False
        is not asked again (None at once; the caller then runs the stage as its own launch)."""
        f = self._fuse
        if f.get(stage) is False:
            return None
        y = self._w4(lin, x, **kw)
        if f.get(stage) is None:
            f[stage] = y is not None
        return y

    def launches(self) -> int:
        """Kernel launches of one decode step of this layer on the fused path (after the first step has settled `_fuse`)."""
        f = self._fuse
        if self.moe is not None:
            # qkv GEMM, attention, o GEMM (+ residual), norm2, route, gate_up, down (+ residual); norm1 as in the dense layer
            return 7 + (0 if f.get("norm1") else 1) + (0 if self.adapters is None else 2 * len(self.adapters.targets))
        n = 5  # qkv GEMM, attention, o GEMM (+ residual), gate_up GEMM, down GEMM (+ residual)
        n += 0 if f.get("norm1") else 1                      # RMSNorm in front of qkv as its own launch
        if not f.get("mlp"):
            n += 0 if f.get("norm2") else 1                  # RMSNorm in front of gate_up
            n += 0 if f.get("swiglu") else 1                 # SwiGLU behind it
        if self.adapters is not None:
            n += 2 * len(self.adapters.targets)              # shrink + expand behind every adapted linear
        return n

    def fusable(self) -> bool:
        """The four linears hold Bint4 weights behind the row-major weights-on-the-right kernel (what w4_linear_fused drives)."""
        ok = ("linear_y_f16RM_x_f16RM_W_any4TC", "linear_y_f16RM_x_f16RM_W_int4TC")
        return all(getattr(m, "kernel", None) in ok and getattr(m, "weight_reshaped", False) and getattr(m, "bias", None) is None
                   for m in ((self.qkv, self.o) if self.moe is not None else (self.qkv, self.o, self.gate_up, self.down))) and \
            (self.moe is None or not self.moe.weights.dense)

    def _split_gate_up(self, gu):
        """[bs, 2 il] in the weight's row order -> contiguous [gate | up] halves (what dg_swiglu reads)."""
        b = self.cfg.gate_up_interleave
        if not b:
            return gu
        return gu.view(gu.shape[0], -1, 2, b).transpose(1, 2).reshape(gu.shape[0], -1)

    def forward_fused5(self, h, attention, pos, cos_tab, sin_tab, lora=None):
        """TP = 1.  qkv GEMM (RMSNorm in its activation staging) -> `attention` -> o GEMM (residual add in its store) -> gate_up
        GEMM (RMSNorm in its staging, SwiGLU in its store) -> down GEMM (residual add in its store): 5 launches instead of 8.
        `h` [bs, hidden] is the residual stream, updated in place.  A stage the library cannot fuse for this problem
        (w4_linear_fused returns None) runs as its own launch, as in forward_fused.
        lora (the call has adapters): shrink + expand behind every adapted linear.  Where the GEMM fused the norm no normalised
        activations exist, so the shrink takes the norm weight and reads `h`; the o / down GEMMs keep their residual store and the
        expand adds into `h`; an adapted gate_up gives up the SwiGLU store (the delta must land in front of the activation): norm fused,
        expand, then dg_swiglu."""
        from . import decode_ops as G

        n1, n2 = self.norm1, self.norm2
        qkv = self._try_fused("norm1", self.qkv, h, norm_weight=n1.weight, norm_eps=n1.eps)
        if qkv is None:
            y = G.add_rmsnorm(h, None, n1.weight, n1.eps)[1]
            qkv = self._adapted(lora, "qkv", y, self.qkv(y))
        else:
            self._adapted(lora, "qkv", h, qkv, n1)
        ctx = attention(qkv, pos, cos_tab, sin_tab)
        if self._w4(self.o, ctx, residual=h, out=h) is None:       # (a residual add is available in every 4-bit kernel)
            G.add_rmsnorm(h, self._adapted(lora, "o", ctx, self.o(ctx)), n2.weight, n2.eps, want_norm=False)
        else:
            self._adapted(lora, "o", ctx, h)
        if self.moe is not None:  # norm2 as its own launch, then route, gate_up, down with the residual add in its store
            return self.moe(G.add_rmsnorm(h, None, n2.weight, n2.eps)[1], residual=h, out=h)
        # MLP block: norm2 + SwiGLU inside the gate_up launch ("mlp"; the store needs the 8 + 8 row order); else whichever of the two
        # the library can fuse (a block too large to stage on chip has no fused norm, "norm2", but still the SwiGLU store, "swiglu")
        il8 = self.cfg.gate_up_interleave == 8 and not (lora is not None and lora.has("gate_up"))
        act = gu = None
        if il8:
            act = self._try_fused("mlp", self.gate_up, h, norm_weight=n2.weight, norm_eps=n2.eps, swiglu=True)
        else:
            self._fuse["mlp"] = False
            gu = self._try_fused("norm2", self.gate_up, h, norm_weight=n2.weight, norm_eps=n2.eps)
            if gu is not None:
                self._adapted(lora, "gate_up", h, gu, n2)
        if act is None and gu is None:
            y = G.add_rmsnorm(h, None, n2.weight, n2.eps)[1]
            if il8:
                act = self._try_fused("swiglu", self.gate_up, y, swiglu=True)
            if act is None:
                gu = self._adapted(lora, "gate_up", y, self.gate_up(y))
        if act is None:
            act = G.swiglu(self._split_gate_up(gu).contiguous())
        if self._w4(self.down, act, residual=h, out=h) is None:
            G.add_rmsnorm(h, self._adapted(lora, "down", act, self.down(act)), n2.weight, n2.eps, want_norm=False)
        else:
            self._adapted(lora, "down", act, h)
        return h


class DecodeStack(torch.nn.Module):
    """Embedding -> `cfg.layers` decoder layers -> final norm -> LM head (16-bit, as in the reference:
    quantize_model skips the LM head by default, quantize.py:34-36)."""

    def __init__(self, cfg: DecodeConfig, linear_factory: Callable, device, dtype=torch.bfloat16, bs: int = 1,
                 rank: int = 0, world: int = 1, group=None, seed: int = 0, lm_head: bool = True,
                 fused: Optional[bool] = None, emulate_gather: bool = False, gather: str = "rccl", fuse_gemm_stages: bool = True,
                 ragged: bool = False, kv_cache: Optional[str] = None, kv_pages: Optional[int] = None, page_size: int = 64,
                 mx8_attention: str = "split", adapters=None):
        """adapters: an `any4_amd.lora.AdapterSet` -- LoRA adapters on the fused linears, one per sequence: `adapter_ids` int32 [bs] (a
        static buffer the step reads, so a captured graph sees ids changed between two replays; -1: none) names every sequence's slot of
        the set, `prefill_adapter_ids` those of a prefill's sequences; `decode`, `prefill` and `generate` take a host list (`adapters=`).
        Every adapted linear becomes linear -> lora_shrink -> lora_expand in all schedules (plain torch: lora.lora_ref); TP = 1 only.
        With None (the default) nothing of this exists and the stack is what it was.
        kv_pages: None = every batch slot owns max_seq cache rows (the default).  A number: a PAGED cache (ragged stacks) --
        every layer holds pools [kv_pages, kvl, page_size, d] and one `block_table` int32 [bs, max_seq / page_size] (a static device
        buffer, -1 = unmapped, mirrored on the host) maps position p of slot b to row p % page_size of page block_table[b, p // page_size];
        a `PagePool` (any4_amd/kvcache.py) hands the pages out.  page_size: a power of two, 64 <= page_size <= max_seq, max_seq % page_size
        == 0.  `decode` / `prefill` with host positions and `generate` map what they are about to write (RuntimeError "KV page pool
        exhausted" before anything is launched or mapped) and refuse a write into a page that two slots share; with a device position
        `reserve` is the caller's.  `reserve` / `release` / `fork` manage slots by hand.  The table is updated by in-place copies, so a
        captured step sees pages mapped between two replays.  Under tensor parallelism table and pool decisions are the same on every
        rank and the pools are per rank.  The fused path needs head_dim 64 / 128.  With kv_cache="mx8" the pools are mx8 (head_dim 64 / 128
        only, fused or not: every layer holds four pools, codes and exponent bytes, behind the one table) and everything above holds unchanged.
        kv_cache: None = a 16-bit KV cache in the stack's dtype (the default); "mx8" = block-scaled 8-bit rows (any4_amd/kvcache.py:
        E4M3 codes and one exponent byte per 32 elements, (1 + 1/32) / 2 of the 16-bit cache's bytes; head_dim % 32 == 0).  The fused
        attention launches then are the mx8 entry points (a decode step always the split one, so the stack always owns a split scratch);
        capture, prefill, ragged decode and generate work unchanged on top, TP too (the caches are per rank).  In fp16, k / v values
        beyond fp16's range are out of contract.
        mx8_attention (kv_cache="mx8"): which kernel a fused decode step launches -- "split" (the default): the 256-thread split kernel,
        a thread per key row; "online": the one-barrier kernel's 8-bit flavour (DG_ATTN_ONE_BARRIER: rows across lanes, the first
        chunk requested before the position is known; a fused stack needs head_dim 64 / 128), with the same split count and scratch.
        A paged mx8 stack (kv_pages) accepts either value and always runs the one-barrier kernel (the same flag on paged pools): it is
        the only decode attention kernel with a paged flavour.
        Prefill and the plain-torch path are the same for both.
        ragged: a position per sequence.  `decode` takes `bs` positions (-1: the sequence is inactive and writes nothing), `prefill`
        a position, a length and a cache slot per sequence, `generate` prompts of different lengths; the step (and its captured
        graph) reads `pos_seq` [bs] in place of `pos`.  A stack built without it is what it was.
        fused: run the non-GEMM parts on the HIP glue kernels (default on a GPU) or as plain torch ops
        (the formulation the glue kernels are tested against; also what runs in the CPU plumbing tests).
        emulate_gather: TIMING ONLY -- build rank `rank` of `world` in a single process and replace every all-gather
        by a local copy of the rank's shard into all `world` slots (the values are meaningless): the per-GPU compute
        of a TP=world decode step, without the interconnect.
        fuse_gemm_stages: (fused, TP = 1, 4-bit linears with Bint4 weights) run a layer as FIVE launches -- RMSNorm inside the
        qkv / gate_up GEMMs' activation staging, the residual adds inside the o / down GEMMs' stores, SwiGLU inside gate_up's store
        when cfg.gate_up_interleave == 8 (DecodeLayer.forward_fused5) -- instead of 4 GEMMs + 4 glue kernels.
        gather: "rccl" = all_gather_into_tensor per exchange; "peer" = the one-shot peer-write gather of
        include/peer_gather_hip.h (any4_amd.shard.PeerWriteGather: one kernel per exchange, stores into the peers' buffers)."""
        super().__init__()
        if gather not in ("rccl", "peer"):
            raise ValueError("gather must be 'rccl' or 'peer'")
        self.paged = kv_pages is not None
        if self.paged and not ragged:
            raise ValueError("kv_pages (a paged KV cache) needs DecodeStack(..., ragged=True)")
        check_cache_config(cfg, kv_cache, kv_pages, page_size, mx8_attention)
        self.kv_cache, self.mx8_attention = kv_cache, mx8_attention
        if adapters is not None:
            if cfg.experts and {"gate_up", "down"} & set(adapters.targets):
                raise ValueError("adapters on gate_up / down with experts: LoRA on expert linears is not built yet")
            if world > 1:
                raise ValueError("adapters need world == 1 (row-sharding an adapter's B across ranks is not implemented)")
            want = {name: (n, k) for name, n, k in cfg.linear_shapes() if name in adapters.targets}
            if adapters.cfg.layers != cfg.layers or adapters.shapes != want or adapters.dtype != dtype or \
                    adapters.cfg.gate_up_interleave != cfg.gate_up_interleave:
                raise ValueError("the AdapterSet was built for another configuration or dtype than this stack")
            sd, ad = torch.device(device), adapters.device
            if sd.type != ad.type or (sd.index is not None and ad.index is not None and sd.index != ad.index):
                raise ValueError(f"the AdapterSet lives on {ad}, this stack on {sd}")
        self.adapters = adapters
        self.gather_mode = gather
        self._peer = {}  # output width per rank -> PeerWriteGather
        self.cfg, self.bs, self.rank, self.world, self.group = cfg, bs, rank, world, group
        self.emulate_gather = emulate_gather
        self.fused = torch.device(device).type == "cuda" if fused is None else fused
        if self.paged and self.fused and cfg.head_dim not in (64, 128):
            raise ValueError(f"a fused stack with kv_pages needs head_dim 64 or 128 (the paged kernels), got {cfg.head_dim}")
        if mx8_attention == "online" and self.fused and cfg.head_dim not in (64, 128):
            raise ValueError(f"a fused stack with mx8_attention='online' needs head_dim 64 or 128 (the one-barrier kernel), got {cfg.head_dim}")
        self.fuse_gemm_stages = fuse_gemm_stages
        gen = torch.Generator(device=device).manual_seed(seed)
        self.embed = torch.nn.Embedding(cfg.vocab, cfg.hidden, device=device, dtype=dtype)
        self.embed.weight.data = torch.randn(cfg.vocab, cfg.hidden, device=device, generator=gen).to(dtype)
        self.embed.weight.requires_grad_(False)
        self.layers = torch.nn.ModuleList(
            [DecodeLayer(cfg, i, linear_factory, rank, world, device, dtype, bs, kv_cache=kv_cache, kv_pages=kv_pages, page_size=page_size,
                         mx8_attention=mx8_attention)
             for i in range(cfg.layers)])
        if self.paged:
            self.page_size, self.page_pool = operator.index(page_size), PagePool(kv_pages)
            self._table = [[-1] * (cfg.max_seq // self.page_size) for _ in range(bs)]  # the host mirror of block_table
            self.register_buffer("block_table", torch.full((bs, cfg.max_seq // self.page_size), -1, dtype=torch.int32, device=device),
                                 persistent=False)
        self.norm = RMSNorm(cfg.hidden, cfg.rms_eps, device, dtype)
        self.lm_head = None
        if lm_head:
            self.lm_head = torch.nn.Linear(cfg.hidden, cfg.vocab, bias=False, device=device, dtype=dtype)
            self.lm_head.weight.data = (torch.randn(cfg.vocab, cfg.hidden, device=device, generator=gen)
                                        / math.sqrt(cfg.hidden)).to(dtype)
            self.lm_head.weight.requires_grad_(False)
        cos, sin = _rope_tables(cfg, device)
        self.register_buffer("cos", cos, persistent=False)
        self.register_buffer("sin", sin, persistent=False)
        self.register_buffer("arange", torch.arange(cfg.max_seq, device=device), persistent=False)
        # static inputs (so a captured graph can be replayed with new values)
        self.register_buffer("tokens", torch.zeros(bs, dtype=torch.long, device=device), persistent=False)
        self.register_buffer("pos", torch.zeros(1, dtype=torch.long, device=device), persistent=False)
        # prefill's own position (a captured decode graph reads `pos`; a prefill between two replays must not move it)
        self.register_buffer("prefill_pos", torch.zeros(1, dtype=torch.long, device=device), persistent=False)
        self.ragged = bool(ragged)
        if self.ragged:  # (a sequence per element; prefill uses the first n of its three)
            for name in ("pos_seq", "prefill_pos_seq", "prefill_len", "prefill_slot"):
                self.register_buffer(name, torch.zeros(bs, dtype=torch.long, device=device), persistent=False)
        if adapters is not None:
            for layer in self.layers:
                layer.adapters = adapters
            self._adapter_ids = [-1] * bs  # the host mirror of adapter_ids
            # False: a fused stack adds the deltas with lora.lora_ref (index_select + bmm) instead of the two kernels -- the torch
            # formulation behind the same step, what tools/llama_decode_bench.py --lora measures the kernels against
            self.lora_kernels = True
            for name in ("adapter_ids", "prefill_adapter_ids"):
                self.register_buffer(name, torch.full((bs,), -1, dtype=torch.int32, device=device), persistent=False)
        self._graph = None
        self._graph_samples = False  # the captured step ends with the sampler (capture(sample=True))
        self._out = None
        self._decodes = 0
        self.peer_poll_every = 16  # decode() calls between two non-blocking reads of the peer-gather status words
        # split-sequence attention: enough blocks per head to fill the 256 CUs (one scratch buffer, launches are stream-ordered)
        self._attn_scratch, self._attn_split = None, 1
        if self.fused:
            from . import decode_ops as G

            hl = cfg.heads // world
            # One block per head walks the cache at one CU's pace (Llama-3-8B, tokens/s at positions 136 / 500 / 900 / 1900: 624 / 583 /
            # 553 / 483); split 4 ways: 579 / 579 / 577 / 554, 8 ways: 537 / 535 / 537 / 539 (the cross-block combine costs ~1 us per
            # block of a head; profiles/r04_ab_attention_split.txt).  The grid is fixed when the step is captured, so the cache's
            # capacity decides: up to 1024 positions one block, up to 4096 four, beyond that eight.
            want = 1 if cfg.max_seq <= 1024 else 4 if cfg.max_seq <= 4096 else 8
            self._attn_split = max(1, min(want, 256 // max(1, bs * hl)))
            if os.environ.get("ANY4_ATTN_SPLIT"):  # developer override (A/B of the threshold above)
                self._attn_split = max(1, int(os.environ["ANY4_ATTN_SPLIT"]))
            if self._attn_split > 1 or kv_cache == "mx8":
                self._attn_scratch = G.rope_attn_split_scratch(bs, hl, cfg.head_dim, self._attn_split, device)
        for layer in self.layers:  # what the stack owns of every layer's cache (as built: no table, no scratch, one block per head)
            layer.kv.table, layer.kv.scratch, layer.kv.nsplit = self.block_table if self.paged else None, self._attn_scratch, self._attn_split

    def kv_cache_bytes(self) -> int:
        """Bytes of this rank's KV cache over all layers (an mx8 cache: codes and exponent bytes; a paged one: the pools, all four of an mx8 one)."""
        return sum(t.numel() * t.element_size() for layer in self.layers for t in layer.kv.tensors())

    # ---- the paged cache: which pages a slot holds (host mirror `_table`, device `block_table`, counts in `page_pool`) ----
    def _need_paged(self, slot=None):
        if not self.paged:
            raise ValueError("this stack has no paged KV cache (DecodeStack(..., kv_pages=N))")
        if slot is not None and not 0 <= operator.index(slot) < self.bs:
            raise ValueError(f"slot {slot} outside [0, bs = {self.bs})")

    def _mapped(self, slot) -> int:
        """Pages slot `slot` holds (they are its first table entries)."""
        row = self._table[slot]
        return row.index(-1) if -1 in row else len(row)

    def _sync_row(self, slot) -> None:
        self.block_table[slot].copy_(torch.tensor(self._table[slot], dtype=torch.int32))  # (in place: a captured step reads this buffer)

    def _reserve_all(self, wants) -> None:
        """`wants`: (slot, tokens) pairs.  Maps pages so that positions < tokens of each slot exist -- all of them or, when the pool
        has too few (RuntimeError), none."""
        ps, short = self.page_size, []
        for slot, tokens in wants:
            if not 0 <= tokens <= self.cfg.max_seq:
                raise ValueError(f"{tokens} tokens in slot {slot}: outside the KV cache [0, {self.cfg.max_seq}]")
            have = self._mapped(slot)
            if -(-tokens // ps) > have:
                short.append((slot, have, -(-tokens // ps) - have))
        new = self.page_pool.alloc(sum(n for _, _, n in short))
        for slot, have, n in short:
            self._table[slot][have: have + n] = [new.pop() for _ in range(n)]
            self._sync_row(slot)

    def _refuse_shared(self, writes) -> None:
        """`writes`: (slot, first position, one past the last) -- a row a call is about to write must not lie in a page that another
        slot holds as well (the cache is append-only; there is no copy-on-write)."""
        for slot, p0, p1 in writes:
            for e in range(p0 // self.page_size, -(-p1 // self.page_size)):
                page = self._table[slot][e]
                if page >= 0 and self.page_pool.refs[page] > 1:
                    raise ValueError(f"slot {slot}: positions [{p0}, {p1}) would be written into page {page}, which {self.page_pool.refs[page]} "
                                     "slots share (fork() shares whole pages of a prefix; they are never written again)")

    def reserve(self, slot: int, tokens: int) -> None:
        """Map pages so that positions < `tokens` of `slot` exist (idempotent; pages are never unmapped here)."""
        self._need_paged(slot)
        self._reserve_all([(operator.index(slot), operator.index(tokens))])

    def release(self, slot: int) -> None:
        """Unmap `slot`: its pages lose a holder, and those nobody else holds return to the pool."""
        self._need_paged(slot)
        n = self._mapped(slot)
        if n:
            self.page_pool.release(self._table[slot][:n])
            self._table[slot][:n] = [-1] * n
            self._sync_row(slot)

    @torch.no_grad()
    def fork(self, src: int, dst: int, tokens: int) -> None:
        """Prefix sharing: `dst` (released first) starts as the first `tokens` positions of `src`.  Its first tokens // page_size table
        entries point at src's pages, which gain a holder -- whole shared pages are never written again, since the cache is append-only
        -- and the tokens % page_size rows of a partial last page are copied into a fresh page, in every layer (mx8 pools: codes and
        exponent bytes)."""
        self._need_paged(src)
        self._need_paged(dst)
        src, dst, tokens, ps = operator.index(src), operator.index(dst), operator.index(tokens), self.page_size
        if src == dst or not 0 <= tokens <= self._mapped(src) * ps:
            raise ValueError(f"fork({src}, {dst}, {tokens}): two slots and a prefix inside what slot {src} has mapped "
                             f"({self._mapped(src) * ps} positions) needed")
        self.release(dst)
        full, part = divmod(tokens, ps)
        fresh = self.page_pool.alloc(1 if part else 0)
        self.page_pool.retain(self._table[src][:full])
        self._table[dst][: full + len(fresh)] = self._table[src][:full] + fresh
        self._sync_row(dst)
        if part:
            for layer in self.layers:
                for pool in layer.kv.tensors():
                    pool[fresh[0], :, :part] = pool[self._table[src][full], :, :part]

    # [bs, n/G] on every rank -> [bs, n], rank-major feature order (== row order of the unsharded weight)
    def _gather(self, y, peer_ok=True):
        if self.world == 1:
            return y
        y = y.contiguous()
        if self.emulate_gather:
            return y.repeat(1, self.world)
        if self.gather_mode == "peer" and peer_ok:
            from .shard import PeerWriteGather

            pg = self._peer.get(y.shape[1])
            if pg is None:
                pg = self._peer[y.shape[1]] = PeerWriteGather(self.bs, y.shape[1], group=self.group, device=y.device, dtype=y.dtype)
            return pg.gather(y)
        parts = torch.empty((self.world,) + tuple(y.shape), dtype=y.dtype, device=y.device)
        if dist.get_backend(self.group) == "nccl":
            dist.all_gather_into_tensor(parts, y, group=self.group)
        else:
            dist.all_gather(list(parts.unbind(0)), y, group=self.group)
        if y.shape[0] == 1:
            return parts.view(1, -1)
        return parts.movedim(0, 1).reshape(y.shape[0], -1)

    # ---- adapters: which slot of the AdapterSet every sequence takes (host mirror `_adapter_ids`, device `adapter_ids`) ----
    def _adapter_list(self, ids, n) -> list:
        """`ids` (a call's `adapters=`: n host ints, negative = none) checked against the set."""
        if self.adapters is None:
            raise ValueError("this stack has no adapters (DecodeStack(..., adapters=AdapterSet))")
        if isinstance(ids, torch.Tensor):
            ids = ids.tolist()
        try:
            vals = [operator.index(v) for v in ids]
        except TypeError as e:
            raise ValueError(f"adapters must be {n} host ints (-1: none): {e}") from e
        if len(vals) != n:
            raise ValueError(f"adapters: {len(vals)} ids for {n} sequences")
        if any(v >= self.adapters.n_adapters for v in vals):
            raise ValueError(f"adapters {vals}: each must be -1 (none) or a slot in [0, n_adapters = {self.adapters.n_adapters})")
        return [max(v, -1) for v in vals]

    def _set_adapters(self, slots, vals) -> None:
        """adapter_ids[slot] = id for the named cache slots, in place (a captured step reads this buffer)."""
        for sl, v in zip(slots, vals):
            self._adapter_ids[sl] = v
        self.adapter_ids.copy_(torch.tensor(self._adapter_ids, dtype=torch.int32))

    def set_adapters(self, ids) -> None:
        """The adapter slot of every sequence from the next step on: `bs` host ints (-1: none; an id >= n_adapters raises).  What
        `decode(..., adapters=ids)` does in front of its step; a captured step sees it at the next replay."""
        self._set_adapters(range(self.bs), self._adapter_list(ids, self.bs))

    def _lora(self, idx, rows_per_id):
        """The adapters of one call as the layers take them (None: a stack without)."""
        if self.adapters is None:
            return None
        from .lora import AdapterCall

        return AdapterCall(self.adapters, idx, rows_per_id, self.fused and self.lora_kernels)

    @torch.no_grad()
    def step(self) -> torch.Tensor:
        """One decode step on the static inputs `self.tokens` [bs], `self.pos` [1] (a ragged stack: `self.pos_seq` [bs]); returns
        logits (or the final hidden state when built without LM head)."""
        if self._peer or (self.gather_mode == "peer" and self.world > 1 and not self.emulate_gather):
            before = {w: pg._calls for w, pg in self._peer.items()}
            out = self._step()
            # a gather object alternates between two buffers per call: an odd number of calls per step would make the last
            # call of one step and the first of the next share a buffer (and a captured graph replays the SAME buffers)
            for w, pg in self._peer.items():
                if (pg._calls - before.get(w, 0)) & 1:
                    pg.gather(torch.zeros(1, w, dtype=pg.dtype, device=pg.device))
            return out
        return self._step()

    def _five_launch(self) -> bool:
        """This stack takes DecodeLayer.forward_fused5 (asked at every step: a linear may be swapped after construction)."""
        return self.fused and self.fuse_gemm_stages and self.world == 1 and all(layer.fusable() for layer in self.layers)

    def _head(self, h, delta=None):
        """Final norm (on the fused path it first adds `delta`, the last layer's not-yet-added MLP output) and the LM head."""
        if not self.fused:
            h = self.norm(h)
            return self.lm_head(h) if self.lm_head is not None else h
        from . import decode_ops as G

        _, y = G.add_rmsnorm(h, delta, self.norm.weight, self.norm.eps)
        if self.lm_head is None:
            return y
        # the un-quantised LM head (quantize.py:34-36 skips it): a streaming GEMV for up to four rows, else torch's GEMM
        logits = G.linear16(y, self.lm_head.weight) if self.lm_head.bias is None else None
        return logits if logits is not None else self.lm_head(y)

    def _step(self) -> torch.Tensor:
        """The three schedules.  A ragged stack reads `pos_seq` [bs] where the other reads `pos` [1]: its plain-torch layer addresses
        per sequence (forward_seq), its attention launches are the _seq entry points."""
        pos = self.pos_seq if self.ragged else self.pos
        h, delta = self.embed(self.tokens), None
        five = self._five_launch()
        lora = self._lora(self.adapter_ids, 1) if self.adapters is not None else None
        for layer in self.layers:
            if not self.fused:
                h = (layer.forward_seq if self.ragged else layer)(h, pos, self.cos, self.sin, self.arange, self._gather, lora=lora)
                continue
            attention = partial(layer.decode_attention, per_sequence=True) if self.ragged else layer.decode_attention
            if five:
                h = layer.forward_fused5(h, attention, pos, self.cos, self.sin, lora=lora)
            else:
                h, delta = layer.forward_fused(h, delta, attention, pos, self.cos, self.sin, self._gather, lora=lora)
        return self._head(h, delta)

    # ---- sampling (any4_amd/sampling.py is the definition; fused: dg_sample, one launch) ----
    def _sampling_buffers(self) -> None:
        """The sampler's static buffers, registered on first use (a stack that never samples has none of them): a temperature, a top-k, a
        top-p and a seed per sequence, read by the kernel -- so a captured step sees values set between two replays -- and `sampled`
        int64 [bs], the tokens of the last `sample`.  The defaults are greedy."""
        if "sampled" in self._buffers:
            return
        dev = self.tokens.device
        for name, dtype, fill in (("sample_temperature", torch.float32, 0), ("sample_top_k", torch.int32, 0), ("sample_top_p", torch.float32, 1),
                                  ("sample_seed", torch.long, 0), ("sampled", torch.long, 0)):
            self.register_buffer(name, torch.full((self.bs,), fill, dtype=dtype, device=dev), persistent=False)

    def set_sampling(self, temperature, top_k=0, top_p=1.0, seed=0) -> None:
        """Sampling parameters of the `bs` sequences, each a scalar or `bs` host values: temperature >= 0 (0: greedy), top_k (<= 0 or >=
        vocab: off), top_p > 0 (>= 1: off), seed (int64).  Checked on the host (ValueError) before anything is written."""
        if self.lm_head is None:
            raise ValueError("sampling needs the LM head")

        def per_sequence(x, what, conv):
            if isinstance(x, torch.Tensor):
                x = x.tolist()
            try:
                vals = [conv(v) for v in x] if isinstance(x, (list, tuple)) else [conv(x)] * self.bs
            except TypeError as e:
                raise ValueError(f"{what} must be a number or {self.bs} host numbers: {e}") from e
            if len(vals) != self.bs:
                raise ValueError(f"{what}: {len(vals)} values for bs = {self.bs} sequences")
            return vals

        temperature = per_sequence(temperature, "temperature", float)
        top_k = per_sequence(top_k, "top_k", operator.index)
        top_p = per_sequence(top_p, "top_p", float)
        seed = per_sequence(seed, "seed", operator.index)
        if any(not t >= 0 or math.isinf(t) for t in temperature):
            raise ValueError(f"temperature {temperature}: each must be a finite number >= 0 (0: greedy)")
        if any(not p > 0 for p in top_p):
            raise ValueError(f"top_p {top_p}: each must be > 0 (>= 1: off)")
        if any(not -2 ** 63 <= s < 2 ** 63 for s in seed):
            raise ValueError(f"seed {seed}: each must fit int64")
        self._sampling_buffers()
        top_k = [min(max(k, 0), 2 ** 31 - 1) for k in top_k]
        for buf, vals in ((self.sample_temperature, temperature), (self.sample_top_k, top_k), (self.sample_top_p, top_p), (self.sample_seed, seed)):
            buf.copy_(torch.tensor(vals, dtype=buf.dtype))  # (in place: a captured step reads these buffers)

    @torch.no_grad()
    def sample(self, logits: torch.Tensor, ctr, ctr_add: int = 1) -> torch.Tensor:
        """Sample a token per sequence from `logits` [bs, vocab] under `set_sampling`'s parameters into `self.sampled` (int64 [bs], returned).
        `ctr` (int64 tensor [bs] or [1], or a host int) + ctr_add is the index the new token will have in its sequence: a decode step passes
        its position buffer and 1, a prefill position + length and 0.  Sequence b draws sampling.uniform(seed[b], ctr + ctr_add) -- nothing
        else enters, not the batch slot and not the number of replays.  A negative `ctr` value marks an inactive sequence: token -1.
        Fused: one dg_sample launch on the buffers (graph-capturable); else sampling.sample_ref."""
        self._sampling_buffers()
        if not isinstance(ctr, torch.Tensor):
            ctr = torch.full((1,), operator.index(ctr), dtype=torch.long, device=logits.device)
        if self.fused:
            from . import decode_ops as G

            return G.sample(logits, ctr, self.sample_temperature, self.sample_top_k, self.sample_top_p, self.sample_seed, ctr_add,
                            token_out=self.sampled)
        from . import sampling

        c = ctr.reshape(-1).expand(logits.shape[0])
        u = sampling.uniform(self.sample_seed, c + ctr_add)
        tok = sampling.sample_ref(logits, self.sample_temperature, self.sample_top_k, self.sample_top_p, u)
        self.sampled.copy_(torch.where(c >= 0, tok, -1))
        return self.sampled

    @torch.no_grad()
    def capture(self, warmup: int = 3, sample: bool = False) -> None:
        """Capture `step()` in a hipGraph (torch.cuda.graph).  All ranks must call it together when world > 1.
        sample: the captured step ends with the sampler (`sample` on the step's logits and position buffer): `decode()` returns the logits
        as before and the tokens are in `self.sampled`, under whatever `set_sampling` set last."""
        if sample:
            if self.lm_head is None:
                raise ValueError("capture(sample=True) needs the LM head")
            self._sampling_buffers()

        def step():
            out = self.step()
            if sample:
                self.sample(out, self.pos_seq if self.ragged else self.pos, 1)
            return out

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                step()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._out = step()
        self._graph = g
        self._graph_samples = bool(sample)
        if self._five_launch():
            self.kernels_per_layer = self.layers[0].launches()
            # + embedding gather, final norm, LM head (+ the sampler)
            self.graph_nodes = sum(layer.launches() for layer in self.layers) + 2 + (1 if self.lm_head is not None else 0) + (1 if sample else 0)

    def _set_position(self, position) -> None:
        """decode()'s `position` into the step's position buffer (`pos_seq` of a ragged stack, else `pos`).  Host values are checked
        here; a ragged stack's device tensor is copied as it is (no sync; the kernels ignore a sequence whose position is outside
        the cache)."""
        S, buf = self.cfg.max_seq, self.pos_seq if self.ragged else self.pos
        if self.ragged and isinstance(position, torch.Tensor) and position.device.type != "cpu":
            if position.dtype != torch.long or position.numel() != self.bs:
                raise ValueError(f"a device position must be int64 [bs = {self.bs}], got {position.dtype} {tuple(position.shape)}")
            buf.copy_(position.view(-1))
            return
        try:
            if self.ragged and isinstance(position, torch.Tensor):
                position = position.tolist()
            if self.ragged and isinstance(position, (list, tuple)):
                vals = [operator.index(p) for p in position]
            else:  # one position for every sequence; all a non-ragged stack takes
                vals = [operator.index(position)] * buf.numel()
        except TypeError as e:
            if self.ragged:
                raise ValueError(f"position must be an int, {self.bs} ints or an int64 device tensor: {e}") from e
            raise ValueError("a position per sequence needs DecodeStack(..., ragged=True)") from e
        if len(vals) != buf.numel():
            raise ValueError(f"{len(vals)} positions for bs = {self.bs} sequences")
        if not self.ragged and not 0 <= vals[0] < S:
            raise ValueError(f"position {vals[0]} outside the KV cache [0, {S})")
        if any(not (p == -1 or 0 <= p < S) for p in vals):
            raise ValueError(f"positions {vals}: each must be -1 (inactive) or inside the KV cache [0, {S})")
        if self.paged:  # the rows this step writes exist and are this slot's alone, or nothing is launched
            self._refuse_shared([(b, p, p + 1) for b, p in enumerate(vals) if p >= 0])
            self._reserve_all([(b, p + 1) for b, p in enumerate(vals) if p >= 0])
        if len(set(vals)) == 1:
            buf.fill_(vals[0])  # (a fill: no copy from host memory in the way of the launches)
        else:
            buf.copy_(torch.tensor(vals, dtype=torch.long))

    @torch.no_grad()
    def decode(self, tokens: torch.Tensor, position, adapters=None) -> torch.Tensor:
        """Feed `tokens` [bs] at sequence position `position`; graph replay if captured, else eager.
        A ragged stack also takes a position per sequence: a list / CPU tensor of `bs` ints, each -1 (the sequence is inactive: it
        writes no cache row and its logits row is unspecified) or inside the cache, or an int64 device tensor [bs], which is copied
        without a sync and without a host check (the kernels ignore positions outside the cache).
        adapters (a stack with an AdapterSet): `bs` host ints, the adapter slot of every sequence from this step on (-1: none; an id >=
        n_adapters raises); None: as they are."""
        ids = None if adapters is None else self._adapter_list(adapters, self.bs)
        self._set_position(position)
        if ids is not None:  # (after every check: a refused call writes nothing)
            self._set_adapters(range(self.bs), ids)
        self.tokens.copy_(tokens)
        out = self._out if self._graph is not None else None
        if self._graph is not None:
            self._graph.replay()
        else:
            out = self.step()
        # peer-write gathers: a slice that did not arrive is NaN in the buffers; here the status words are read back on a
        # cadence without synchronising the device (PeerWriteGather.poll) so that a slow / dead rank raises instead of decoding on
        self._decodes += 1
        if self._peer and self._decodes % self.peer_poll_every == 0:
            for pg in self._peer.values():
                pg.poll()
        return out

    # ---- prompt prefill ----
    def _gather_rows(self, y):
        """_gather for bs * T rows: always the all_gather branch (the peer-write buffers are sized for `bs` rows)."""
        return self._gather(y, peer_ok=False)

    def _prefill_chunk(self, toks, positions, lengths, slots, per_sequence):
        """A chunk `toks` [n, T] through every layer; `positions`, `lengths`, `slots`: n host ints each.  Returns the last layer's
        (h, delta), [n * T, hidden] (delta: its not-yet-added MLP output on the fused path, else None).  The fused attention launch is
        the scalar entry point on `prefill_pos` (set to positions[0] here; positions None: left as the caller set it) or, per_sequence,
        the _seq one on the first n of `prefill_pos_seq` / `prefill_len` / `prefill_slot`."""
        n, T = toks.shape
        if not per_sequence and positions is not None:
            self.prefill_pos.fill_(positions[0])
        h, delta = self.embed(toks.reshape(-1)), None  # [n * T, hidden], row i * T + t
        lora = self._lora(self.prefill_adapter_ids[:n], T) if self.adapters is not None else None  # (row i * T + t: sequence i's adapter)
        pos = self.prefill_pos
        if per_sequence and self.fused:
            pos, dev_len, dev_slot = [buf[:n] for buf in (self.prefill_pos_seq, self.prefill_len, self.prefill_slot)]
            for buf, vals in zip((pos, dev_len, dev_slot), (positions, lengths, slots)):
                buf.copy_(torch.tensor(vals, dtype=torch.long))
        for layer in self.layers:
            if not self.fused:  # plain torch needs the positions on the host (prefill() refuses position=None on this path)
                h = layer.forward_prefill(h, positions, lengths, slots, T, self.cos, self.sin, self._gather_rows, lora=lora)
                continue
            # the eight launches of a decode step at n * T rows, with the chunk's attention
            attention = layer.prefill_attention
            if per_sequence:
                attention = partial(attention, T=T, lengths=dev_len, slots=dev_slot, per_sequence=True)
            h, delta = layer.forward_fused(h, delta, attention, pos, self.cos, self.sin, self._gather_rows, lora=lora)
        return h, delta

    @staticmethod
    def _last_rows(hd, n):
        """The last token's row of every sequence out of a chunk's (h, delta), [n * T, hidden] each."""
        return [None if t is None else t.view(n, -1, t.shape[-1])[:, -1].contiguous() for t in hd]

    @torch.no_grad()
    def prefill(self, tokens: torch.Tensor, position=0, chunk: Optional[int] = None, lengths=None, slots=None, adapters=None) -> torch.Tensor:
        """Feed a prompt: `tokens` [bs, T] at sequence positions position ... position + T - 1.  Every layer's KV cache receives the T
        rows a token-by-token `decode()` would have written (bit for bit on the fused path), and the logits [bs, vocab] of the LAST
        token are returned (the final hidden state when built without LM head) -- `decode()` continues at position + T.
        chunk: tokens per pass (default: the whole prompt up to 2048 tokens, longer prompts in pieces of 2048); later pieces attend
        over the cache rows of the earlier ones, which bounds activation memory at bs * chunk rows.
        Eager.  It is also legal inside `torch.cuda.graph` for a fixed T; the position lives in `self.prefill_pos` (not `self.pos`, so a
        captured decode graph is not disturbed): pass position=None to leave that buffer as the caller set it (single chunk, fused
        path only; the kernel itself ignores tokens whose position is outside the cache).
        world > 1: attention stays local (heads are split across ranks); the four exchanges of a layer are all_gathers at bs * T
        rows, also with gather="peer" (the peer-write buffers are sized for the `bs` rows of a decode step).
        A ragged stack: `tokens` [n, T], rows padded on the right to the common T.  `position`: an int or n host ints; `lengths`: n host
        ints in [0, T] (default T), sequence i has tokens[i, :lengths[i]] at positions position[i] ...; `slots`: n distinct host ints in
        [0, bs), the cache slot (= row of a later `decode`) of each sequence (default: slot i, and n == bs).  Chunks advance every
        sequence by `chunk` tokens.  Returns logits [n, vocab] of each sequence's LAST VALID token (unspecified for a length of 0);
        cache slots not named are not touched.
        adapters (a stack with an AdapterSet): n host ints, the adapter slot of each sequence (-1: none).  They are written to
        `adapter_ids[slot]` too, so the decode steps that follow use the same adapter; None: each sequence takes what `adapter_ids` holds
        for its cache slot.  (position=None: the caller owns `prefill_adapter_ids` as well.)"""
        per_sequence = lengths is not None or slots is not None or isinstance(position, (list, tuple)) or \
            (isinstance(position, torch.Tensor) and position.dim() > 0) or self.paged  # (there is no scalar-position paged kernel)
        if per_sequence and not self.ragged:
            raise ValueError("positions / lengths / slots per sequence need DecodeStack(..., ragged=True)")
        if per_sequence and position is None:
            raise ValueError("position=None (the caller owns prefill_pos) does not go with lengths / slots")
        if tokens.dim() != 2 or tokens.shape[1] < 1 or not (1 <= tokens.shape[0] <= self.bs if per_sequence else tokens.shape[0] == self.bs):
            raise ValueError(f"tokens must be [{'1 <= n <= ' if per_sequence else ''}bs = {self.bs}, T >= 1], got {tuple(tokens.shape)}")
        S, (n, T) = self.cfg.max_seq, tokens.shape
        if position is None:  # nothing is made on the host and copied here: a pageable copy is not legal inside a graph capture
            if adapters is not None:
                raise ValueError("position=None (the caller owns the prefill buffers) does not go with adapters=")
            if not self.fused or (chunk is not None and int(chunk) < T):
                raise ValueError("position=None (the caller owns prefill_pos) needs the fused path and a single chunk")
            return self._head(*self._last_rows(self._prefill_chunk(tokens, None, None, None, False), n))
        # one model on the host: a position, a length and a slot per sequence (a call that names none: the same for everybody)
        if not per_sequence:
            position = int(position)

        def ints(x, what):
            if isinstance(x, torch.Tensor):
                x = x.tolist()
            vals = [operator.index(v) for v in x] if isinstance(x, (list, tuple)) else [operator.index(x)] * n
            if len(vals) != n:
                raise ValueError(f"{what}: {len(vals)} values for {n} sequences")
            return vals

        try:
            position, lengths = ints(position, "position"), ints(T if lengths is None else lengths, "lengths")
            if slots is None and n != self.bs:
                raise ValueError(f"{n} sequences in a stack of bs = {self.bs} need `slots`")
            slots = ints(list(range(self.bs)) if slots is None else slots, "slots")
        except TypeError as e:
            raise ValueError(f"position / lengths / slots must be host ints: {e}") from e
        if any(not 0 <= x <= T for x in lengths):
            raise ValueError(f"lengths {lengths}: each must be in [0, T = {T}]")
        if any(p < 0 or p + x > S for p, x in zip(position, lengths)):
            raise ValueError(f"positions {position} + lengths {lengths} outside the KV cache [0, {S})")
        if any(not 0 <= x < self.bs for x in slots) or len(set(slots)) != n:
            raise ValueError(f"slots {slots}: {n} distinct values in [0, bs = {self.bs}) needed")
        chunk = min(T, 2048) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        if adapters is not None:
            adapters = self._adapter_list(adapters, n)
        if self.paged:
            self._refuse_shared([(sl, p, p + x) for p, x, sl in zip(position, lengths, slots) if x > 0])
            self._reserve_all([(sl, p + x) for p, x, sl in zip(position, lengths, slots) if x > 0])
        # the LM head runs on the last token of every sequence only.  Named per sequence, the last valid token may lie in any chunk: its
        # row of the last layer's output is picked on the device; else it is the last row of the last chunk
        last = torch.tensor([max(x - 1, 0) for x in lengths], dtype=torch.long).to(tokens.device) if per_sequence else None
        if self.adapters is not None:  # (after every check: nothing is written by a call that raises)
            if adapters is not None:
                self._set_adapters(slots, adapters)
            self.prefill_adapter_ids[:n].copy_(torch.tensor([self._adapter_ids[sl] for sl in slots], dtype=torch.int32))
        keep = None
        for c0 in range(0, T, chunk):
            toks = tokens[:, c0: c0 + chunk]
            Tc = toks.shape[1]
            hd = self._prefill_chunk(toks, [p + c0 for p in position], [min(max(x - c0, 0), Tc) for x in lengths], slots, per_sequence)
            if not per_sequence:
                keep = self._last_rows(hd, n) if c0 + Tc >= T else None
                continue
            idx = (last - c0).clamp(0, Tc - 1).view(n, 1, 1)
            here = ((last >= c0) & (last < c0 + Tc)).view(n, 1)
            rows = [None if t is None else t.view(n, Tc, -1).gather(1, idx.expand(n, 1, t.shape[-1])).squeeze(1) for t in hd]
            keep = rows if keep is None else [None if r is None else torch.where(here, r, k) for r, k in zip(rows, keep)]
        return self._head(*[None if t is None else t.contiguous() for t in keep])

    def _picked(self, logits):
        """The sampled tokens of the decode step that returned `logits`: the captured sampler has written them, else one launch does."""
        if self._graph is not None and self._graph_samples:
            return self.sampled
        return self.sample(logits, self.pos_seq if self.ragged else self.pos, 1)

    @torch.no_grad()
    def generate(self, prompt, new_tokens: int, eos: Optional[int] = None, *, temperature=None, top_k=0, top_p=1.0, seed=0,
                 adapters=None) -> torch.Tensor:
        """Greedy continuation: `prefill(prompt)` [bs, T], then `decode` (graph replay if captured) from position T.
        Returns the `new_tokens` generated token ids [bs, new_tokens].
        temperature (None: greedy, the argmax of every step): a SAMPLED continuation -- every token, the first one after the prefill
        included, comes from `sample` under `set_sampling(temperature, top_k, top_p, seed)` (each a scalar or `bs` host values, checked
        before anything is launched).  The token with index i of a sequence is drawn with sampling.uniform(seed, i), so a sequence's
        continuation does not depend on its slot or on the rest of the batch beyond what the logits do.  A step captured with
        `capture(sample=True)` samples inside the graph and the tokens go back in without a host round trip; otherwise the sampler is
        one launch behind each step.
        A ragged stack also takes a list of `bs` 1-D token tensors of different lengths, and `eos`: a sequence that has emitted `eos`,
        or whose next position would be outside the cache, is inactive from the next step on (decided on the device, no sync per
        step) and its remaining outputs are `eos` (-1 when eos is None).
        adapters (a stack with an AdapterSet): `bs` host ints, the adapter slot of every sequence for the prefill and every step (they
        stay in `adapter_ids`); None: as they are."""
        if adapters is not None:
            adapters = self._adapter_list(adapters, self.bs)
        if self.lm_head is None:
            raise ValueError("generate needs the LM head")
        if new_tokens < 1:
            raise ValueError(f"new_tokens must be >= 1, got {new_tokens}")
        per_sequence = isinstance(prompt, (list, tuple)) or eos is not None
        sampled = temperature is not None
        if sampled:
            self.set_sampling(temperature, top_k, top_p, seed)
        if self.paged:  # every slot's whole run, up front (the per-sequence steps below pass device positions); nothing is released here
            lens = [p.numel() for p in prompt] if isinstance(prompt, (list, tuple)) else [prompt.shape[-1]] * self.bs
            if len(lens) == self.bs:
                self._reserve_all([(b, min(n + new_tokens, self.cfg.max_seq)) for b, n in enumerate(lens)])
        if not per_sequence:
            base = prompt.shape[1] if prompt.dim() == 2 else 0  # a host int: decode() fills the position
            logits = self.prefill(prompt, adapters=adapters)
            tok = self.sample(logits, base, 0) if sampled else logits.argmax(-1)
        else:  # right-padded prefill with lengths; who is still active is kept on the device
            if not self.ragged:
                raise ValueError("prompts of different lengths / eos need DecodeStack(..., ragged=True)")
            prompts = list(prompt.unbind(0)) if isinstance(prompt, torch.Tensor) else list(prompt)
            if len(prompts) != self.bs or any(p.dim() != 1 or p.numel() < 1 for p in prompts):
                raise ValueError(f"prompts must be bs = {self.bs} non-empty 1-D token tensors")
            lens = [p.numel() for p in prompts]
            dev = self.tokens.device
            padded = torch.zeros(self.bs, max(lens), dtype=torch.long, device=dev)
            for b, p in enumerate(prompts):
                padded[b, : lens[b]] = p.to(dev)
            logits = self.prefill(padded, position=0, lengths=lens, adapters=adapters)
            base = torch.tensor(lens, dtype=torch.long).to(dev)
            tok = self.sample(logits, base, 0) if sampled else logits.argmax(-1)
            alive = torch.ones(self.bs, dtype=torch.bool, device=dev)
            fill = -1 if eos is None else int(eos)
        out = [tok.clone()]
        for i in range(new_tokens - 1):  # the token emitted at step i is fed at position len_b + i
            if not per_sequence:
                logits = self.decode(tok, base + i)
                tok = self._picked(logits) if sampled else logits.argmax(-1)
            else:
                if eos is not None:
                    alive = alive & (tok != eos)
                alive = alive & (base + i < self.cfg.max_seq)
                logits = self.decode(torch.where(alive, tok, 0), torch.where(alive, base + i, -1))
                tok = torch.where(alive, self._picked(logits) if sampled else logits.argmax(-1), fill)
            out.append(tok.clone())
        return torch.stack(out, dim=1)


def memory_allocated_mb(device=None) -> float:
    """ROCm replacement of the reference's nvidia-smi based MemoryTracker (utils.py:241): peak bytes the
    caching allocator handed out on this device, in MiB."""
    return torch.cuda.max_memory_allocated(device) / 2 ** 20
