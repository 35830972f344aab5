"""Mixture of experts (MoE) for the decode stack: a top-k router and expert MLPs whose 4-bit weights are picked on the device.

A sparse MLP block replaces a layer's one gate_up / down pair by E of them and a router [E, hidden]; every token runs `top_k` of the E
(Mixtral-8x7B: 8 experts, 2 per token).  Three launches serve it (include/decode_glue_hip.h): dg_moe_route, then dg_moe_launch (DG_MOE_GEMV) twice
(DG_MOE_GATE_UP, DG_MOE_DOWN); all three read their indices on the device, so a captured step follows the router from replay to replay.

  * `moe_ref` is the definition, plain torch in float64: what the kernels and the plain-torch formulation are tested against.
  * `ExpertStack` is one linear of every expert, stacked so that expert e sits at base + e * stride; `MoEWeights` is a layer's pair of them
    (gate_up in the 8 + 8 interleaved row order of `DecodeConfig.gate_up_interleave = 8`, and down).
  * `MoEMLP(router_w, weights, top_k)` is the block: `forward(x, residual)` runs the three launches, `forward(..., fused=False)` a
    plain-torch formulation that runs ALL experts and combines them with a mask (no value is read on the host either way).
  * Many rows (a prompt): `MoEMLP(..., grouped_from=R)` runs calls of R rows or more as route, dg_moe_group, dg_moe_launch (DG_MOE_GROUPED) twice: the
    pairs sorted by expert (`group_ref` is the definition of that workspace) and a tile GEMM that reads a selected expert once per 128 of
    its rows.  A tile GEMM dequantises into LDS, so its weights are the 16-bit ones, w = RNE16(fma(lut[code], scale, zero)), as in the dense
    stack's prefill: `moe_grouped_ref` (= moe_ref(..., weights="rounded")) is the definition of that path, everything else as below.

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

    def weights_rounded64(self, e: int) -> torch.Tensor:
        """[n][k] float64: the 16-bit weights RNE16(fma(f32(lut[code]), f32(scale), f32(zero))) a tile GEMM multiplies by.  (The float64
        scale * lut + zero of 16-bit factors is exact up to the last of 53 bits; rounding it to f32 is the fma.)"""
        if self.dense is not None:
            return self.dense[e].double()
        return self.weights64(e).float().to(self.dtype).double()

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


def moe_ref(x, router_w, experts: MoEWeights, top_k: int, residual=None, parts: bool = False, weights: str = "exact"):
    """The definition (module docstring), float64: y [m][hidden] in x's dtype; parts: (y, ids, gates, logits) with the float64 values.
    weights: "exact" -- scale * lut[code] + zero, not rounded: the GEMV path -- or "rounded" -- the 16-bit weights of the grouped path."""
    if weights not in ("exact", "rounded"):
        raise ValueError(f'weights must be "exact" or "rounded", got {weights!r}')
    w64 = (lambda st, e: st.weights64(e)) if weights == "exact" else (lambda st, e: st.weights_rounded64(e))
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
        g, u = _split8(x64[rows] @ w64(experts.gate_up, e).t())
        g16, u16 = g.to(dt).double(), u.to(dt).double()
        a = ((g16 / (1.0 + torch.exp(-g16))).to(dt).double() * u16).to(dt).double()
        d = a @ w64(experts.down, e).t()
        acc[rows] += (gates[rows] * hit[rows]).sum(dim=1, keepdim=True) * d
    if residual is not None:
        acc = acc + residual.double()
    y = acc.to(dt)
    return (y, ids, gates, logits) if parts else y


def moe_grouped_ref(x, router_w, experts: MoEWeights, top_k: int, residual=None, parts: bool = False):
    """The definition of the GROUPED path (MoEMLP(grouped_from=...), dg_moe_launch's DG_MOE_GROUPED), float64: moe_ref over the 16-bit weights
    w = RNE16(fma(lut[code], scale, zero)) -- what a tile GEMM holds in LDS --, with moe_ref's rounding points for SwiGLU and the combine."""
    return moe_ref(x, router_w, experts, top_k, residual, parts, weights="rounded")


GROUP_PERM = 136  # int32 units in front of perm in the group workspace: n_tiles, n_invalid, n_valid, bm; count[64]; offset[68]


def group_bound(P: int, E: int, BM: int) -> int:
    """The m-extent of the grouped GEMM's grid: no list of tiles of P pairs over E experts is longer."""
    return -(-P // BM) + min(E, P)


def group_ws_ints(P: int, E: int, BM: int) -> int:
    """int32 units of dg_moe_group's workspace: the header, perm [P], invalid [P], tiles [bound][3]."""
    return GROUP_PERM + 2 * P + 3 * group_bound(P, E, BM)


def group_ref(ids, E: int, BM: int):
    """The definition of dg_moe_group's workspace, plain numpy: ids [m][top_k] -> a namespace of int32 arrays
      perm [P]       the pairs p = i top_k + s with an id in [0, E), sorted by (expert ascending, pair ascending) (stable); -1 from n_valid on
      invalid [P]    the other pairs, ascending; -1 from n_invalid on
      count [E], offset [E + 1] (its prefix)
      tiles [bound][3]  (expert, first position in perm, rows <= BM), ceil(count[e] / BM) per expert, experts ascending; zeros from n_tiles on
      n_tiles, n_invalid, n_valid, bound = ceil(P / BM) + min(E, P)
      workspace      the whole int32 image as the kernel writes it (include/decode_glue_hip.h)"""
    import numpy as np
    from types import SimpleNamespace

    a = (ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)).astype(np.int64).reshape(-1)
    P = a.size
    ok = (a >= 0) & (a < E)
    pairs = np.arange(P, dtype=np.int64)
    valid = pairs[ok]
    order = valid[np.argsort(a[valid], kind="stable")]
    bad = pairs[~ok]
    count = np.bincount(a[valid], minlength=E)[:E].astype(np.int32) if valid.size else np.zeros(E, np.int32)
    offset = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    bound = group_bound(P, E, BM)
    tiles = np.zeros((bound, 3), np.int32)
    n = 0
    for e in range(E):
        for t in range(0, int(count[e]), BM):
            tiles[n] = (e, offset[e] + t, min(BM, int(count[e]) - t))
            n += 1
    perm = np.full(P, -1, np.int32)
    perm[:order.size] = order
    invalid = np.full(P, -1, np.int32)
    invalid[:bad.size] = bad
    ws = np.zeros(group_ws_ints(P, E, BM), np.int32)
    ws[:4] = (n, bad.size, order.size, BM)
    ws[4:4 + E] = count
    ws[68:68 + E + 1] = offset
    ws[GROUP_PERM:GROUP_PERM + P] = perm
    ws[GROUP_PERM + P:GROUP_PERM + 2 * P] = invalid
    ws[GROUP_PERM + 2 * P:] = tiles.reshape(-1)
    return SimpleNamespace(perm=perm, invalid=invalid, count=count, offset=offset, tiles=tiles, n_tiles=n, n_invalid=int(bad.size),
                           n_valid=int(order.size), bound=bound, workspace=ws)


class MoEMLP(torch.nn.Module):
    """The sparse MLP block: router [E, hidden] (16-bit), the stacked experts, `top_k` experts per token.
    forward(x [rows, hidden] (normed), residual=None) -> RNE16(sum_s g_s down_s(swiglu(gate_up_s(x))) (+ residual)).
    record: an optional list; the plain-torch path appends (its f32 logits [rows][E], the activations x) to it at every call (tests
    assert the router's margins on them)."""

    def __init__(self, router_w: torch.Tensor, weights: MoEWeights, top_k: int, grouped_from: int = None):
        """grouped_from = R: forward(fused=True) on R rows or more runs the grouped path (module docstring; its numerics are
        moe_grouped_ref's); None: every call runs the GEMV launches."""
        super().__init__()
        E = weights.E
        if router_w.dim() != 2 or router_w.shape[0] != E or router_w.shape[1] != weights.gate_up.k:
            raise ValueError(f"router_w must be [E = {E}, hidden = {weights.gate_up.k}], got {tuple(router_w.shape)}")
        if not 1 <= E <= 64 or not 1 <= top_k <= min(E, 8):
            raise ValueError(f"1 <= E <= 64 and 1 <= top_k <= min(E, 8) needed, got E = {E}, top_k = {top_k}")
        self.router = torch.nn.Parameter(router_w, requires_grad=False)
        if grouped_from is not None and grouped_from < 1:
            raise ValueError(f"grouped_from must be None or >= 1, got {grouped_from}")
        self.weights, self.top_k, self.record = weights, int(top_k), None
        self.grouped_from = grouped_from
        self._grouped = {}  # rows -> (bm, ids, gates, group workspace, act, f32 workspace): allocated at the first call with that row count

    def forward(self, x, residual=None, fused: bool = True, out=None):
        """out (the kernels only): where the result goes; it may be `residual` itself -- the residual stream, updated in place."""
        if not fused:
            return self._torch(x, residual)
        if self.weights.dense:
            raise RuntimeError("MoEMLP: the kernels need 4-bit experts; 16-bit experts run with fused=False only")
        from . import decode_ops as G

        if self.grouped_from is not None and x.shape[0] >= self.grouped_from:
            return self._forward_grouped(x, residual, out)
        ids, gates = G.moe_route(x, self.router, self.top_k)
        act = G.moe_gate_up(x, self.weights.gate_up, ids)
        return G.moe_down(act, self.weights.down, ids, gates, residual, out)

    def _forward_grouped(self, x, residual, out):
        """route, group, grouped gate_up, grouped down (+ combine).  The buffers between the launches are kept per row count: no allocation
        at steady state, and a captured graph replays on the buffers it was captured with."""
        from . import decode_ops as G

        W, rows, k = self.weights, x.shape[0], self.top_k
        buf = self._grouped.get(rows)
        if buf is None:
            plan = G.moe_grouped_plan(1, W.down, rows, k)
            dev = x.device
            buf = self._grouped[rows] = (
                int(plan[0]), torch.empty((rows, k), dtype=torch.int32, device=dev), torch.empty((rows, k), dtype=torch.float32, device=dev),
                torch.empty(int(plan[5]) // 4, dtype=torch.int32, device=dev), torch.empty((rows * k, W.down.k), dtype=x.dtype, device=dev),
                torch.empty((rows * k, W.down.n), dtype=torch.float32, device=dev))
        bm, ids, gates, gws, act, fws = buf
        G.moe_route(x, self.router, k, ids, gates)
        G.moe_group(ids, W.E, bm, gws)
        G.moe_gate_up_grouped(x, W.gate_up, ids, gws, act)
        return G.moe_down_grouped(act, W.down, ids, gates, gws, residual, out, fws)

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
