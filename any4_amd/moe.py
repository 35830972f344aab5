"""Mixture of experts (MoE) for the decode stack: a top-k router and expert MLPs whose 4-bit weights are picked on the device.

A sparse MLP block replaces a layer's one gate_up / down pair by E of them and a router [E, hidden]; every token runs `top_k` of the E
(Mixtral-8x7B: 8 experts, 2 per token).  Three launches serve it (include/decode_glue_hip.h): dg_moe_route, then dg_moe_w4_launch twice
(DG_MOE_GATE_UP, DG_MOE_DOWN); all three read their indices on the device, so a captured step follows the router from replay to replay.

  * `moe_ref` is the definition, plain torch in float64: what the kernels and the plain-torch formulation are tested against.
  * `ExpertStack` is one linear of every expert, stacked so that expert e sits at base + e * stride; `MoEWeights` is a layer's pair of them
    (gate_up in the 8 + 8 interleaved row order of `DecodeConfig.gate_up_interleave = 8`, and down).
  * `MoEMLP(router_w, weights, top_k)` is the block: `forward(x, residual)` runs the three launches, `forward(..., fused=False)` a
    plain-torch formulation that runs ALL experts and combines them with a mask (no value is read on the host either way).

For activation row i (16-bit, already RMS-normed):
  logits   l[i][e] = sum_c router_w[e][c] x[i][c]             f32 sums, NOT rounded to 16 bit
  softmax  p = softmax(l[i]) over all E
  select   the top_k largest p, ordered by (p descending, expert index ascending): a tie goes to the lower index
  gates    g[i][s] = p_s / sum_{s' < top_k} p_{s'}
  expert   e = ids[i][s]:  a = RNE16(RNE16(silu(RNE16(gate))) RNE16(up)) of x[i] . W13[e]^T (dg_swiglu's rounding points),
           d_s = a . W2[e]^T, the group-scaled contraction (scale and zero applied to f32 partial sums), NOT rounded
  combine  y[i] = RNE16(sum_s g[i][s] d_s (+ residual[i]))
"""
from __future__ import annotations

import torch

QT_INT4, QT_ANY4_GLOBAL, QT_ANY4_ROWWISE = 0, 1, 2


def unpack_bint4(words: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """codes int64 [n][k] of Bint4 words at innerKTiles 4, int32 [n / 8][k / 64][32][2] (plain torch, any device): lane t = 4 (row & 7) + q
    of a (tile, 64-k super-tile) holds two words, one per 32-k chunk c; byte j of a word holds k = 64 s + 32 c + 2 q + 16 (j & 1) + (j >> 1) in
    its low nibble and that k + 8 in its high nibble."""
    w = words.reshape(n // 8, k // 64, 8, 4, 2).to(torch.int64) & 0xFFFFFFFF     # [tile][s][r][q][c]
    j = torch.arange(4, device=words.device)
    byte = (w.unsqueeze(-1) >> (8 * j)) & 0xFF                                    # [tile][s][r][q][c][j]
    nib = torch.stack([byte & 15, byte >> 4], dim=-1)                             # [...][j][hi]
    q = torch.arange(4, device=words.device).view(4, 1, 1, 1)
    c = torch.arange(2, device=words.device).view(1, 2, 1, 1)
    jj = j.view(1, 1, 4, 1)
    hi = torch.arange(2, device=words.device).view(1, 1, 1, 2)
    kk = (32 * c + 2 * q + 16 * (jj & 1) + (jj >> 1) + 8 * hi).reshape(-1)        # k within the super-tile, in [q][c][j][hi] order
    codes = torch.empty(n // 8, k // 64, 8, 64, dtype=torch.int64, device=words.device)
    codes[..., kk] = nib.reshape(n // 8, k // 64, 8, 64)
    return codes.permute(0, 2, 1, 3).reshape(n, k)


class ExpertStack:
    """One linear [n, k] of each of E experts, stacked.  4-bit: `words` int32 [E][n / 8][k / 64][32][2] (Bint4, innerKTiles 4), `qinfo`
    [E][k / group][n][2] 16-bit, `lut` [E][n][16] / [E][16] / None (int4).  Dense (the 16-bit baseline, plain-torch path only): `dense`
    [E][n][k]."""

    def __init__(self, n, k, group=None, words=None, qinfo=None, lut=None, dense=None):
        self.n, self.k, self.group, self.words, self.qinfo, self.lut, self.dense = n, k, group, words, qinfo, lut, dense
        self.E = (dense if dense is not None else words).shape[0]

    @property
    def qtype(self) -> int:
        return QT_INT4 if self.lut is None else QT_ANY4_GLOBAL if self.lut.dim() == 2 else QT_ANY4_ROWWISE

    @property
    def dtype(self):
        return self.dense.dtype if self.dense is not None else self.qinfo.dtype

    def weights64(self, e: int) -> torch.Tensor:
        """[n][k] float64: the group-scaled weights scale * lut[code] + zero, NOT rounded to 16 bit (the contraction the kernels compute
        applies scale and zero to f32 partial sums, so no 16-bit weight ever exists)."""
        if self.dense is not None:
            return self.dense[e].double()
        codes = unpack_bint4(self.words[e], self.n, self.k)
        if self.lut is None:
            v = (codes - 8).double()
        else:
            lut = self.lut[e].double()
            lut = lut.expand(self.n, 16) if lut.dim() == 1 else lut
            v = torch.gather(lut, 1, codes)
        q = self.qinfo[e].double()                                                # [k / g][n][2]
        scale = q[:, :, 0].t().repeat_interleave(self.group, dim=1)               # [n][k]
        zero = q[:, :, 1].t().repeat_interleave(self.group, dim=1)
        return v * scale + zero

    def weights16(self, e: int) -> torch.Tensor:
        """[n][k] in the stack's 16-bit type: what the plain-torch formulation multiplies by (on a GPU: tg_dequant_w4)."""
        if self.dense is not None:
            return self.dense[e]
        if self.words.is_cuda and self.k % 512 == 0:  # (tg_dequant_w4 walks 512 k per wave; other k: the torch formulation below)
            from . import ops

            return ops.dequant_w4(self.words[e], self.qinfo[e], None if self.lut is None else self.lut[e], self.group, self.qtype, self.k, 4, self.n)
        return self.weights64(e).to(self.dtype)

    @classmethod
    def from_linears(cls, modules) -> "ExpertStack":
        """Stack modules made by the existing factories: Any4Linear / Int4Linear holding Bint4 words at innerKTiles 4, or nn.Linear."""
        m0 = modules[0]
        if isinstance(m0, torch.nn.Linear):
            return cls(m0.out_features, m0.in_features, dense=torch.stack([m.weight.detach() for m in modules]).contiguous())
        for m in modules:
            if not getattr(m, "weight_reshaped", False) or m.weight.dim() != 4 or m.weight.shape[2:] != (32, 2) or getattr(m, "bias", None) is not None \
                    or "x_f16RM_W" not in getattr(m, "kernel", ""):
                raise ValueError("MoE experts need Any4Linear / Int4Linear modules with Bint4 weights at innerKTiles 4 and no bias (or nn.Linear)")
        lut = None if not hasattr(m0, "lut") else torch.stack([m.lut.detach() for m in modules]).contiguous()
        return cls(m0.out_features, m0.in_features, m0.group_size, torch.stack([m.weight.detach() for m in modules]).contiguous(),
                   torch.stack([m.scales_and_zeros.detach() for m in modules]).contiguous(), lut)


class MoEWeights:
    """One layer's experts: `gate_up` [2 il, hidden] with rows in blocks of 8 gate + 8 up, and `down` [hidden, il]."""

    def __init__(self, gate_up: ExpertStack, down: ExpertStack):
        if gate_up.E != down.E or gate_up.n != 2 * down.k or gate_up.k != down.n:
            raise ValueError("gate_up [2 il, hidden] and down [hidden, il] of the same number of experts needed")
        self.gate_up, self.down, self.E = gate_up, down, gate_up.E

    @classmethod
    def from_linears(cls, gate_up_modules, down_modules) -> "MoEWeights":
        return cls(ExpertStack.from_linears(list(gate_up_modules)), ExpertStack.from_linears(list(down_modules)))

    @property
    def dense(self) -> bool:
        return self.gate_up.dense is not None


def _split8(gu):
    """[rows, 2 il] in blocks of 8 gate + 8 up -> (gate [rows, il], up [rows, il])"""
    v = gu.reshape(gu.shape[0], -1, 2, 8)
    return v[:, :, 0].reshape(gu.shape[0], -1), v[:, :, 1].reshape(gu.shape[0], -1)


def route_ref(logits: torch.Tensor, top_k: int):
    """(ids int64 [m][top_k], gates [m][top_k]) from logits [m][E], in the logits' float type: softmax, the top_k by (p descending, index
    ascending), renormalised."""
    p = torch.softmax(logits, dim=-1)
    ps, ids = torch.sort(p, dim=-1, descending=True, stable=True)
    ps, ids = ps[:, :top_k], ids[:, :top_k]
    return ids, ps / ps.sum(dim=-1, keepdim=True)


def moe_ref(x, router_w, experts: MoEWeights, top_k: int, residual=None, parts: bool = False):
    """The definition (module docstring), float64: y [m][hidden] in x's dtype; parts: (y, ids, gates, logits) with the float64 values."""
    dt = x.dtype
    x64 = x.double()
    logits = x64 @ router_w.double().t()
    ids, gates = route_ref(logits, top_k)
    m = x.shape[0]
    acc = torch.zeros(m, experts.down.n, dtype=torch.float64, device=x.device)
    for e in range(experts.E):
        hit = ids == e                                                             # [m][top_k]
        rows = hit.any(dim=1).nonzero().flatten()
        if rows.numel() == 0:
            continue
        g, u = _split8(x64[rows] @ experts.gate_up.weights64(e).t())
        g16, u16 = g.to(dt).double(), u.to(dt).double()
        a = ((g16 / (1.0 + torch.exp(-g16))).to(dt).double() * u16).to(dt).double()
        d = a @ experts.down.weights64(e).t()
        acc[rows] += (gates[rows] * hit[rows]).sum(dim=1, keepdim=True) * d
    if residual is not None:
        acc = acc + residual.double()
    y = acc.to(dt)
    return (y, ids, gates, logits) if parts else y


class MoEMLP(torch.nn.Module):
    """The sparse MLP block: router [E, hidden] (16-bit), the stacked experts, `top_k` experts per token.
    forward(x [rows, hidden] (normed), residual=None) -> RNE16(sum_s g_s down_s(swiglu(gate_up_s(x))) (+ residual)).
    record: an optional list; the plain-torch path appends (its f32 logits [rows][E], the activations x) to it at every call (tests
    assert the router's margins on them)."""

    def __init__(self, router_w: torch.Tensor, weights: MoEWeights, top_k: int):
        super().__init__()
        E = weights.E
        if router_w.dim() != 2 or router_w.shape[0] != E or router_w.shape[1] != weights.gate_up.k:
            raise ValueError(f"router_w must be [E = {E}, hidden = {weights.gate_up.k}], got {tuple(router_w.shape)}")
        if not 1 <= E <= 64 or not 1 <= top_k <= min(E, 8):
            raise ValueError(f"1 <= E <= 64 and 1 <= top_k <= min(E, 8) needed, got E = {E}, top_k = {top_k}")
        self.router = torch.nn.Parameter(router_w, requires_grad=False)
        self.weights, self.top_k, self.record = weights, int(top_k), None

    def forward(self, x, residual=None, fused: bool = True, out=None):
        """out (the kernels only): where the result goes; it may be `residual` itself -- the residual stream, updated in place."""
        if not fused:
            return self._torch(x, residual)
        if self.weights.dense:
            raise RuntimeError("MoEMLP: the kernels need 4-bit experts; 16-bit experts run with fused=False only")
        from . import decode_ops as G

        ids, gates = G.moe_route(x, self.router, self.top_k)
        act = G.moe_gate_up(x, self.weights.gate_up, ids)
        return G.moe_down(act, self.weights.down, ids, gates, residual, out)

    def _torch(self, x, residual=None):
        """All E experts on every row, combined with a device-side mask: E times the work, nothing read on the host."""
        W = self.weights
        logits = x.float() @ self.router.float().t()
        if self.record is not None:
            self.record.append((logits.detach().clone(), x.detach().clone()))
        ids, gates = route_ref(logits, self.top_k)
        acc = torch.zeros(x.shape[0], W.down.n, dtype=torch.float32, device=x.device)
        for e in range(W.E):
            g, u = _split8(x @ W.gate_up.weights16(e).t())
            d = (torch.nn.functional.silu(g) * u) @ W.down.weights16(e).t()
            acc += (gates * (ids == e)).sum(dim=1, keepdim=True) * d.float()
        if residual is not None:
            acc = acc + residual.float()
        return acc.to(x.dtype)
