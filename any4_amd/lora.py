"""LoRA adapters on the decode stack's fused linears: many adapters resident at once, one picked per sequence on the device.

An adapter of a linear y = W x is a pair (A [r, k], B [n, r]) and a factor alpha: y += (alpha / r) B (A x).  The stack's linears are
fused (q / k / v one linear, gate / up one linear), so an adapter here belongs to one of the four targets "qkv", "o", "gate_up", "down"
of a layer; `fuse_projections` builds such a fused adapter from adapters trained on the separate projections.

  * `AdapterSet` owns the static tensors every adapted linear reads -- A [n_adapters, rank, k], B [n_adapters, n, rank], scale
    [n_adapters] -- and is handed to `DecodeStack(..., adapters=set)`.  `load` / `clear` copy in place, so a captured step sees them.
  * `lora_ref` is the definition, in plain torch: what `fused=False` stacks run and what the two kernels (include/decode_glue_hip.h:
    dg_lora_shrink, dg_lora_expand; decode_ops.lora_shrink / lora_expand) are tested against.
  * `LoRALinear` is the training-side wrapper of one linear; `AdapterSet.load_modules` serves what was trained with it.
"""
from __future__ import annotations

import operator

import torch

TARGETS = ("qkv", "o", "gate_up", "down")


def lora_ref(x, A, B, scale, idx, rows_per_id, y, norm_weight=None, eps: float = 1e-5):
    """The definition of the adapter delta on a linear's output, IN PLACE on y [m, n] (returned).  Row i takes adapter a = idx[i //
    rows_per_id]; an id outside [0, n_adapters) leaves the row's bits alone.
      t[i] = A[a] @ x[i]                         f32 accumulation of 16-bit products
      y[i] = RNE16(f32(y[i]) + scale[a] * (B[a] @ t[i]))
    norm_weight g [k] (the RMSNorm in front of the linear, in the GEMV's "sum" convention, tests/fused_ref.py): t[i] = rs[i] * A[a] @
    RNE16(x[i] * g), rs = rsqrt(mean(x[i]^2) + eps) in f32.  index_select + bmm over rows; nothing is read on the host."""
    m, na = x.shape[0], A.shape[0]
    ids = idx.long().repeat_interleave(int(rows_per_id))[:m]
    valid = (ids >= 0) & (ids < na)
    safe = torch.where(valid, ids, torch.zeros_like(ids))
    xt = x if norm_weight is None else (x.float() * norm_weight.float()).to(x.dtype)
    t = torch.bmm(A.index_select(0, safe).float(), xt.float().unsqueeze(2)).squeeze(2)          # [m, r]
    if norm_weight is not None:
        xf = x.float()
        t = t * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    d = torch.bmm(B.index_select(0, safe).float(), t.unsqueeze(2)).squeeze(2) * scale.index_select(0, safe).unsqueeze(1)  # [m, n]
    y.copy_(torch.where(valid.unsqueeze(1), (y.float() + d).to(y.dtype), y))
    return y


def fuse_projections(parts):
    """The adapter of a fused linear from the adapters of its projections: parts = [(A_q [r_q, k], B_q [n_q, r_q]), (A_k, B_k), ...] in the
    row order of the fused weight (q, k, v / gate, up).  Returns (A [sum r, k], B [sum n, sum r]): the A's stacked, the B's block-diagonal,
    so that B (A x) is the concatenation of the projections' B_i (A_i x).  The projections must share one alpha / rank factor (one `scale`
    per adapter and linear); fold a different one into its B."""
    A = torch.cat([a for a, _ in parts], dim=0)
    B = torch.block_diag(*[b for _, b in parts])
    return A, B


class AdapterCall:
    """One call's view of an AdapterSet, handed down to the layers: which adapter every row takes (`idx` int32 on the device, row i takes
    idx[i // rows_per_id]) and whether the kernels or `lora_ref` run."""

    def __init__(self, aset: "AdapterSet", idx: torch.Tensor, rows_per_id: int, fused: bool):
        self.set, self.idx, self.rows_per_id, self.fused = aset, idx, int(rows_per_id), fused

    def has(self, target: str) -> bool:
        return target in self.set.targets

    def apply(self, layer: int, target: str, x, y, norm=None):
        """y (the output of linear `target` of layer `layer` for the input x, [rows, n]) += the rows' adapter deltas, in place.  norm: the
        RMSNorm module the linear's GEMM fused, when x is the un-normalised residual stream."""
        if target not in self.set.targets:
            return y
        A, B, scale = self.set.tensors(layer, target)
        g, eps = (None, 0.0) if norm is None else (norm.weight, norm.eps)
        if not self.fused:
            return lora_ref(x, A, B, scale, self.idx, self.rows_per_id, y, g, eps)
        from . import decode_ops as G

        t = G.lora_shrink(x, A, self.idx, self.rows_per_id, g, eps, out=self.set.scratch(x.shape[0]))
        return G.lora_expand(t, B, scale, self.idx, y, self.rows_per_id)


class AdapterSet:
    """`n_adapters` adapter slots of rank <= `rank` for the linears `targets` of every layer of a `DecodeConfig`.  Per layer and target:
    A [n_adapters, rank, k], B [n_adapters, n, rank] in `dtype`, scale float32 [n_adapters]; an empty slot is all zeros (its delta is 0).
    B is kept in the row order of the stack's weight (gate_up: `shard_rows(cfg, "gate_up", 0, 1)`, the 8 + 8 interleave included).
    One float32 scratch t [rows, rank] serves every linear (launches are stream-ordered); it only ever grows, and no buffer a captured
    graph may have seen is released (`scratch`)."""

    def __init__(self, cfg, n_adapters: int, rank: int, device, dtype=torch.bfloat16, targets=TARGETS):
        n_adapters, rank = operator.index(n_adapters), operator.index(rank)
        if n_adapters < 1:
            raise ValueError(f"n_adapters must be >= 1, got {n_adapters}")
        if rank % 8 or not 8 <= rank <= 64:
            raise ValueError(f"rank must be a multiple of 8 in [8, 64] (the kernels' range), got {rank}")
        targets = tuple(targets)
        if not targets or any(t not in TARGETS for t in targets):
            raise ValueError(f"targets must be among {TARGETS}, got {targets}")
        if dtype not in (torch.bfloat16, torch.float16, torch.float32):  # (float32: the plain-torch formulation only, the kernels are 16-bit)
            raise ValueError(f"dtype must be bfloat16 or float16 (float32 on the plain-torch path), got {dtype}")
        self.cfg, self.n_adapters, self.rank, self.device, self.dtype, self.targets = cfg, n_adapters, rank, torch.device(device), dtype, targets
        self.shapes = {name: (n, k) for name, n, k in cfg.linear_shapes() if name in targets}
        self._w = {}
        for layer in range(cfg.layers):
            for name, (n, k) in self.shapes.items():
                self._w[layer, name] = (torch.zeros(n_adapters, rank, k, dtype=dtype, device=device),
                                        torch.zeros(n_adapters, n, rank, dtype=dtype, device=device),
                                        torch.zeros(n_adapters, dtype=torch.float32, device=device))
        self._buffers = []  # every scratch buffer ever handed out, smallest first (see `scratch`)

    def tensors(self, layer: int, target: str):
        """(A, B, scale) of one linear."""
        return self._w[layer, target]

    def scratch(self, rows: int) -> torch.Tensor:
        """t [rows, rank] float32: a view of the scratch buffer.  A call with more rows than any before it gets a larger buffer (at least
        twice the last), and every earlier buffer is KEPT: a captured graph holds the address of the one it was captured on and goes on
        writing there at every replay, so that memory must never return to the allocator while the set lives.  Launches that share the
        set are stream-ordered (one stream), so sharing a buffer between them is safe."""
        if not self._buffers or self._buffers[-1].shape[0] < rows:
            grown = max(rows, 2 * self._buffers[-1].shape[0] if self._buffers else 0)
            self._buffers.append(torch.empty(grown, self.rank, dtype=torch.float32, device=self.device))
        return self._buffers[-1][:rows]

    def _slot(self, slot) -> int:
        slot = operator.index(slot)
        if not 0 <= slot < self.n_adapters:
            raise ValueError(f"adapter slot {slot} outside [0, n_adapters = {self.n_adapters})")
        return slot

    @torch.no_grad()
    def load(self, slot: int, weights, alpha) -> None:
        """Put an adapter into `slot`: weights = {(layer, target): (A [r', k], B [n, r'])} with r' <= rank, B in the canonical row order of
        the FULL fused weight ([q; k; v], [gate; up]).  alpha: a number, or {(layer, target): number}; the factor is alpha / r', the
        adapter's own rank.  Zero-padded to the set's rank and copied in place (a captured step reads these tensors); linears the dict does
        not name keep a zero delta.  Checked as a whole before anything is written."""
        from .decode import shard_rows

        slot = self._slot(slot)
        staged = []
        for key, (A, B) in weights.items():
            if key not in self._w:
                raise ValueError(f"no adapted linear {key}: layers [0, {self.cfg.layers}), targets {self.targets}")
            n, k = self.shapes[key[1]]
            r = A.shape[0] if A.dim() == 2 else -1
            if not 1 <= r <= self.rank or tuple(A.shape) != (r, k) or tuple(B.shape) != (n, r):
                raise ValueError(f"{key}: A [r' <= {self.rank}, {k}] and B [{n}, r'] needed, got {tuple(A.shape)} and {tuple(B.shape)}")
            a = float(alpha[key] if isinstance(alpha, dict) else alpha)
            if key[1] == "gate_up":
                B = B[shard_rows(self.cfg, "gate_up", 0, 1).to(B.device)]
            staged.append((key, r, A, B, a / r))
        self.clear(slot)
        for key, r, A, B, s in staged:
            dA, dB, ds = self._w[key]
            dA[slot, :r].copy_(A)
            dB[slot, :, :r].copy_(B)
            ds[slot] = s

    @torch.no_grad()
    def load_modules(self, slot: int, modules) -> None:
        """`load` from {(layer, target): LoRALinear}: serve what was trained."""
        self.load(slot, {key: (m.A.detach(), m.B.detach()) for key, m in modules.items()}, {key: m.alpha for key, m in modules.items()})

    @torch.no_grad()
    def clear(self, slot: int) -> None:
        """Zero a slot's scale, A and B in every linear."""
        slot = self._slot(slot)
        for A, B, s in self._w.values():
            A[slot].zero_()
            B[slot].zero_()
            s[slot] = 0


class LoRALinear(torch.nn.Module):
    """`base` (a frozen linear: an Any4Linear, an nn.Linear) with one trainable adapter: y = base(x) + (alpha / rank) B (A x), A [rank, k]
    random, B [n, rank] zero at the start.  While anything requires grad the delta is two torch matmuls under autograd (the input gradient
    flows on through `base`, a 4-bit one's through its dx kernel); under no_grad on a GPU it is the serving pair of kernels, bit for bit what
    a DecodeStack with this adapter loaded (`AdapterSet.load_modules`) adds to the linear's output."""

    def __init__(self, base: torch.nn.Module, rank: int, alpha: float, seed: int = 0):
        super().__init__()
        k, n, dev = base.in_features, base.out_features, base.weight.device
        # (a packed linear's weight is int32 words; its 16-bit type is that of its scales)
        dtype = base.weight.dtype if base.weight.is_floating_point() else base.scales_and_zeros.dtype
        self.base, self.rank, self.alpha = base, operator.index(rank), float(alpha)
        gen = torch.Generator().manual_seed(seed)
        self.A = torch.nn.Parameter((torch.randn(self.rank, k, generator=gen) / k ** 0.5).to(device=dev, dtype=dtype))
        self.B = torch.nn.Parameter(torch.zeros(n, self.rank, device=dev, dtype=dtype))
        self._idx = None

    def forward(self, x):
        y = self.base(x)
        s = self.alpha / self.rank
        if torch.is_grad_enabled() and (x.requires_grad or self.A.requires_grad or self.B.requires_grad):
            return y + torch.matmul(torch.matmul(x, self.A.t()), self.B.t()) * s
        if not y.is_contiguous():  # (the delta lands in place through a 2-D view of y: a reshape that copies would lose it)
            raise RuntimeError("LoRALinear: the base linear's output must be contiguous")
        x2, y2 = x.reshape(-1, x.shape[-1]), y.view(-1, y.shape[-1])
        m = x2.shape[0]
        if self._idx is None or self._idx.device != x.device:
            self._idx = torch.zeros(1, dtype=torch.int32, device=x.device)  # every row takes adapter 0 of a set of one
        A, B = self.A.detach().unsqueeze(0), self.B.detach().unsqueeze(0)
        scale = torch.full((1,), s, dtype=torch.float32, device=x.device)
        if not x.is_cuda:
            lora_ref(x2, A, B, scale, self._idx, m, y2)
            return y
        from . import decode_ops as G

        G.lora_expand(G.lora_shrink(x2.contiguous(), A, self._idx, m), B, scale, self._idx, y2, m)
        return y
