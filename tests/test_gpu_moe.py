"""Mixture-of-experts kernels on the GPU (dg_moe_route, dg_moe_launch with DG_MOE_GEMV) against the float64 references and bounds of tests/moe_ref.py,
exact lookup probes, graph replay, and the decode stack with experts against its plain-torch path.  Run: pytest -m gpu."""
import numpy as np
import pytest
import torch

from tests import moe_ref as R
from tests.moe_ref import BF16, F16

pytestmark = pytest.mark.gpu
DEV = "cuda"
GU, DN = 0, 1

# (stage, weight rows, k, m, top_k) of the float64 cases below: hidden sizes 512 / 1664 (26 super-tiles: a ragged split over 8 waves), il 64 /
# 192 (3 super-tiles: five waves own no k) / 1664, and 4144 rows = 259 units (two passes per workgroup, the last workgroup with one)
GEMV_CASES = [
    # stage, n, k, m, E, top_k, g, qtype, dtype, residual
    (GU, 128, 512, 1, 1, 1, 64, "int4", BF16, False),
    (GU, 384, 1664, 3, 5, 2, 128, "any4_global", F16, False),
    (GU, 3328, 512, 8, 8, 3, 256, "any4_rowwise", BF16, False),
    (GU, 4144, 512, 8, 8, 2, 128, "any4_rowwise", F16, False),
    (GU, 3328, 1664, 3, 5, 3, 64, "any4_rowwise", BF16, False),
    (DN, 512, 64, 1, 1, 1, 64, "int4", F16, True),
    (DN, 1664, 192, 3, 5, 2, 64, "any4_global", BF16, False),
    (DN, 512, 1664, 8, 8, 3, 128, "any4_rowwise", BF16, True),
    (DN, 1664, 1664, 8, 5, 2, 128, "int4", F16, True),
    (DN, 4144, 192, 8, 8, 2, 64, "any4_rowwise", BF16, True),
]
GEMV_SHAPES = [(c[0], c[1], c[2], c[3], c[5]) for c in GEMV_CASES]


def _cid(c):
    return f"{'gate_up' if c[0] == GU else 'down'}-n{c[1]}-k{c[2]}-m{c[3]}-E{c[4]}-top{c[5]}-g{c[6]}-{c[7]}-{'bf16' if c[8] == BF16 else 'fp16'}"


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _run(stage, stack, x, ids, gates=None, res=None):
    """One launch into a guarded output; asserts the guard bands; returns y on the CPU."""
    from any4_amd import decode_ops as G

    m, top_k = ids.shape
    shape = (m * top_k, stack.n // 2) if stage == GU else (m, stack.n)
    view, whole = R.guarded(torch.zeros(shape, dtype=x.dtype), DEV, fill=R.SENTINEL)
    view.view(torch.int16).fill_(R.SENTINEL)
    if stage == GU:
        G.moe_gate_up(x.to(DEV), stack, _i32(ids), out=view)
    else:
        G.moe_down(x.to(DEV), stack, _i32(ids), gates.to(DEV), None if res is None else res.to(DEV), out=view)
    torch.cuda.synchronize()
    assert R.guard_intact(view, whole), "wrote outside the output"
    return view.cpu()


def _within(y, ref, tol, what):
    err = np.abs(y.double().numpy() - ref)
    bad = err > tol
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} outside the bound; worst ratio {np.nanmax(err / tol):.2f} at {np.argwhere(bad)[:4].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------------------
# router
# ---------------------------------------------------------------------------------------------------------------------------------
ROUTER_CASES = [(m, k, E, t, BF16) for m in (1, 8) for k in (512, 1664, 4096) for E, t in ((8, 2), (5, 3), (2, 1))] + \
               [(m, k, 64, 4, BF16) for m in (1, 8) for k in (512, 4096)] + [(8, 1664, 8, 2, F16), (8, 4096, 64, 4, F16)]


def _route(x, rw, top_k):
    from any4_amd import decode_ops as G

    m = x.shape[0]
    iv, iw = R.guarded(torch.zeros(m * top_k * 2, dtype=torch.int16), DEV, fill=R.SENTINEL)
    gv, gw = R.guarded(torch.zeros(m * top_k * 2, dtype=torch.int16), DEV, fill=R.SENTINEL)
    ids, gates = iv.view(torch.int32).view(m, top_k), gv.view(torch.float32).view(m, top_k)
    G.moe_route(x.to(DEV), rw.to(DEV), top_k, ids, gates)
    torch.cuda.synchronize()
    assert R.guard_intact(iv, iw) and R.guard_intact(gv, gw), "the router wrote outside ids / gates"
    return ids.cpu().clone(), gates.cpu().clone()


@pytest.mark.parametrize("m,k,E,top_k,dtype", ROUTER_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_router(m, k, E, top_k, dtype):
    x, rw = R.router_inputs(m, k, E, dtype, seed=0)
    ids64, gates64, logits, A, gtol = R.route_ref64(x, rw, top_k)
    ok, worst = R.margin_ok(logits, A, top_k)
    print(f"margin: smallest gap / (2 allowance) = {worst:.2f}")
    assert ok.all(), f"rows {np.nonzero(~ok)[0].tolist()} are too close to a tie for an id comparison (ratio {worst:.2f}): no row may be left out"
    ids, gates = _route(x, rw, top_k)
    assert np.array_equal(ids.numpy(), ids64), (ids.tolist(), ids64.tolist())
    err = np.abs(gates.double().numpy() - gates64)
    print(f"gates: worst error / bound = {(err / gtol).max():.3f}")
    assert (err <= gtol).all(), (err / gtol).max()
    ids2, gates2 = _route(x, rw, top_k)
    assert torch.equal(ids, ids2) and torch.equal(gates.view(torch.int32), gates2.view(torch.int32))


def test_router_ties_go_to_the_lower_index():
    x, rw = R.router_inputs(8, 1664, 8, BF16, seed=2)
    rw[6], rw[3] = rw[2].clone(), rw[0].clone()          # 2 == 6 and 0 == 3 on every row
    ids, gates = _route(x, rw, 3)
    ids64 = R.route_ref64(x, rw, 3)[0]
    seen = 0
    for row in ids.tolist():
        for lo, hi in ((2, 6), (0, 3)):
            if hi in row:
                seen += 1
                assert lo in row and row.index(lo) + 1 == row.index(hi), row
            elif lo in row:
                assert row.index(lo) == 2, row      # the pair was cut by top_k: the lower index got the last slot
    assert seen, "no row selected a duplicated expert"
    assert np.array_equal(ids.numpy(), ids64)
    assert all(len(set(r)) == 3 for r in ids.tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# the two stages against float64
# ---------------------------------------------------------------------------------------------------------------------------------

def test_regimes_reached():
    """On this device's own plan: fewer units than workgroups, a remainder, several passes, waves without k."""
    R.assert_regimes_reached(GEMV_SHAPES, device=torch.cuda.current_device())


@pytest.mark.parametrize("case", GEMV_CASES, ids=_cid)
def test_stage_f64(oracle, case):
    stage, n, k, m, E, top_k, g, qtype, dtype, with_res = case
    stack, raw = R.make_stack(oracle, E, n, k, g, qtype, dtype)
    sd = R.to_dev(stack, DEV)
    ids = R.spread_ids(m, top_k, E, seed=n + k)
    if stage == GU:
        x = R.pair_inputs(m, k, dtype, 1)
        ref, tol = R.gate_up_ref64(raw, g, x, ids, E)
        y = _run(GU, sd, x, ids)
        y2 = _run(GU, sd, x, ids)
    else:
        x = R.pair_inputs(m * top_k, k, dtype, 2)
        gates = torch.softmax(torch.randn(m, top_k, generator=torch.Generator().manual_seed(5)), dim=1)
        res = R.make_inputs(m, n, k, dtype, 3)[2] if with_res else None
        ref, tol = R.down_ref64(raw, g, x, ids, gates, E, res)
        y = _run(DN, sd, x, ids, gates, res)
        y2 = _run(DN, sd, x, ids, gates, res)
    _within(y, ref, tol, _cid(case))
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), "two launches differ"


# ---------------------------------------------------------------------------------------------------------------------------------
# lookup probes: exact
# ---------------------------------------------------------------------------------------------------------------------------------
PROBE = dict(E=5, n=384, k=192, g=64)    # DOWN: 24 units, 3 super-tiles (one group each)
PROBE_GU = dict(E=5, n=288, k=256, g=128)


@pytest.mark.parametrize("qtype,dtype", [("any4_rowwise", BF16), ("any4_global", F16), ("int4", BF16)])
def test_onehot_down_returns_the_named_experts_weights(oracle, qtype, dtype):
    """top_k = 1 (the gate is exactly 1), activation row i is 1.0 at column j(i): y[i][r] is RNE16(fma(lut[code], scale, zero)) of expert
    ids[i], row r, column j(i), bit for bit -- a wrong expert stride, row, column, nibble or group shows."""
    E, n, k, g = (PROBE[f] for f in ("E", "n", "k", "g"))
    stack, raw = R.make_stack(oracle, E, n, k, g, qtype, dtype)
    m = 8
    ids = np.array([[4], [0], [2], [2], [1], [3], [0], [4]], np.int32)
    cols = np.array([0, 191, 63, 64, 9, 130, 77, 25])      # both nibbles, every byte position, every group, first and last column
    x = torch.zeros(m, k, dtype=dtype)
    x[torch.arange(m), torch.from_numpy(cols)] = 1.0
    y = _run(DN, R.to_dev(stack, DEV), x, ids, torch.ones(m, 1))
    want = torch.stack([R.weights16(oracle, raw[int(ids[i, 0])], g, qtype, dtype)[:, cols[i]] for i in range(m)])
    want = (want.float() + 0.0).to(dtype)                   # (-0 among +0 products sums to +0)
    bad = y.view(torch.int16) != want.contiguous().view(torch.int16)
    assert not bad.any(), f"{int(bad.sum())} / {bad.numel()} differ; (row, weight row) {torch.nonzero(bad)[:4].tolist()}"


@pytest.mark.parametrize("qtype,dtype", [("any4_rowwise", BF16), ("int4", F16)])
def test_onehot_gate_up_returns_the_named_experts_weights(oracle, qtype, dtype):
    """The same through the SwiGLU store: expected = dg_swiglu of the named expert's gate and up weights of that column."""
    from any4_amd import decode_ops as G

    E, n, k, g = (PROBE_GU[f] for f in ("E", "n", "k", "g"))
    stack, raw = R.make_stack(oracle, E, n, k, g, qtype, dtype)
    m, top_k = 4, 2
    ids = np.array([[4, 0], [2, 3], [1, 2], [0, 4]], np.int32)
    cols = np.array([255, 0, 127, 138])
    x = torch.zeros(m, k, dtype=dtype)
    x[torch.arange(m), torch.from_numpy(cols)] = 1.0
    y = _run(GU, R.to_dev(stack, DEV), x, ids)
    rows = []
    for i in range(m):
        for s in range(top_k):
            w = (R.weights16(oracle, raw[int(ids[i, s])], g, qtype, dtype)[:, cols[i]].float() + 0.0).to(dtype).view(-1, 2, 8)
            rows.append(torch.cat([w[:, 0].reshape(-1), w[:, 1].reshape(-1)]))
    want = G.swiglu(torch.stack(rows).to(DEV).contiguous()).cpu()
    bad = y.view(torch.int16) != want.view(torch.int16)
    assert not bad.any(), f"{int(bad.sum())} / {bad.numel()} differ; (pair, column) {torch.nonzero(bad)[:4].tolist()}"


@pytest.mark.parametrize("stage", [GU, DN], ids=["gate_up", "down"])
def test_unselected_experts_are_never_read(oracle, stage):
    """Words, scales / zeros and LUT of every unselected expert become garbage / NaN: the output keeps its bits."""
    P = PROBE_GU if stage == GU else PROBE
    E, n, k, g = (P[f] for f in ("E", "n", "k", "g"))
    stack, raw = R.make_stack(oracle, E, n, k, g, "any4_rowwise", BF16)
    m, top_k = 3, 2
    ids = np.array([[1, 3], [3, 1], [1, 3]], np.int32)
    x = R.pair_inputs(m if stage == GU else m * top_k, k, BF16, 7)
    gates = torch.tensor([[0.75, 0.25], [0.5, 0.5], [0.125, 0.875]])
    clean = _run(stage, R.to_dev(stack, DEV), x, ids, gates)
    words, qinfo, lut = stack.words.clone(), stack.qinfo.clone(), stack.lut.clone()
    for e in (0, 2, 4):
        words[e] = torch.randint(-2 ** 31, 2 ** 31 - 1, words[e].shape, generator=torch.Generator().manual_seed(e)).to(torch.int32)
        qinfo[e], lut[e] = float("nan"), float("nan")
    dirty = _run(stage, R.to_dev(stack, DEV, words=words, qinfo=qinfo, lut=lut), x, ids, gates)
    assert torch.equal(clean.view(torch.int16), dirty.view(torch.int16))
    ref, tol = (R.gate_up_ref64(raw, g, x, ids, E) if stage == GU else R.down_ref64(raw, g, x, ids, gates, E))
    _within(clean, ref, tol, "clean")


ID_PATTERNS = {
    "all rows one expert": lambda m, t, E: np.full((m, t), 3),                       # (top_k = 1 below: 8 pairs on one expert)
    "every row another": lambda m, t, E: (np.arange(m)[:, None] + np.arange(t)[None, :] * 0) % E,
    "duplicates in a row": lambda m, t, E: np.stack([[i % E] * t for i in range(m)]),
    "one expert, 24 pairs": lambda m, t, E: np.full((m, t), 1),                      # three sweeps of eight
}


@pytest.mark.parametrize("pattern", list(ID_PATTERNS))
@pytest.mark.parametrize("stage", [GU, DN], ids=["gate_up", "down"])
def test_id_patterns(oracle, stage, pattern):
    P = PROBE_GU if stage == GU else PROBE
    E, n, k, g = (P[f] for f in ("E", "n", "k", "g"))
    stack, raw = R.make_stack(oracle, E, n, k, g, "any4_rowwise", BF16)
    m, top_k = 8, {"all rows one expert": 1, "every row another": 1, "duplicates in a row": 3, "one expert, 24 pairs": 3}[pattern]
    ids = ID_PATTERNS[pattern](m, top_k, E).astype(np.int32)
    x = R.pair_inputs(m if stage == GU else m * top_k, k, BF16, 11)
    gates = torch.softmax(torch.randn(m, top_k, generator=torch.Generator().manual_seed(6)), dim=1)
    res = R.make_inputs(m, n, k, BF16, 12)[2]
    y = _run(stage, R.to_dev(stack, DEV), x, ids, gates, res)
    ref, tol = (R.gate_up_ref64(raw, g, x, ids, E) if stage == GU else R.down_ref64(raw, g, x, ids, gates, E, res))
    _within(y, ref, tol, pattern)
    if stage == GU and top_k > 1:      # the slots of a row hold the same expert: the same bits
        v = y.view(m, top_k, -1).view(torch.int16)
        assert all(torch.equal(v[:, 0], v[:, s]) for s in range(1, top_k))


def test_invalid_ids(oracle):
    """-1 and E: GATE_UP writes a zero row, DOWN adds nothing; a row without a valid id gets the residual's bits, or zeros."""
    E, n, k, g = (PROBE[f] for f in ("E", "n", "k", "g"))
    stack, raw = R.make_stack(oracle, E, n, k, g, "any4_rowwise", BF16)
    sd = R.to_dev(stack, DEV)
    ids = np.array([[2, -1], [E, 4], [-1, E], [0, 1], [7, -2 ** 31]], np.int32)
    m, top_k = ids.shape
    x = R.pair_inputs(m * top_k, k, BF16, 13)
    gates = torch.full((m, top_k), 0.5)
    res = R.make_inputs(m, n, k, BF16, 14)[2]
    y = _run(DN, sd, x, ids, gates, res)
    _within(y, *R.down_ref64(raw, g, x, ids, gates, E, res), "down with invalid ids")
    assert torch.equal(y[2].view(torch.int16), res[2].view(torch.int16)) and torch.equal(y[4].view(torch.int16), res[4].view(torch.int16))
    y0 = _run(DN, sd, x, ids, gates, None)
    assert not y0[2].view(torch.int16).any() and not y0[4].view(torch.int16).any()
    Eg, ng, kg, gg = (PROBE_GU[f] for f in ("E", "n", "k", "g"))
    gstack, graw = R.make_stack(oracle, Eg, ng, kg, gg, "any4_rowwise", BF16)
    xg = R.pair_inputs(m, kg, BF16, 15)
    a = _run(GU, R.to_dev(gstack, DEV), xg, ids)
    _within(a, *R.gate_up_ref64(graw, gg, xg, ids, Eg), "gate_up with invalid ids")
    invalid = torch.from_numpy(((ids < 0) | (ids >= Eg)).reshape(-1))
    assert not a[invalid].view(torch.int16).any() and a[~invalid].view(torch.int16).any(dim=1).all()


@pytest.mark.parametrize("stage", [GU, DN], ids=["gate_up", "down"])
def test_row_blocks_m19(oracle, stage):
    """m = 19 through the entry point: three launches of 8, 8 and 3 rows; the same bits as those launches made by hand."""
    P = PROBE_GU if stage == GU else PROBE
    E, n, k, g = (P[f] for f in ("E", "n", "k", "g"))
    stack, raw = R.make_stack(oracle, E, n, k, g, "any4_global", F16)
    sd = R.to_dev(stack, DEV)
    m, top_k = 19, 2
    ids = R.spread_ids(m, top_k, E, seed=19)
    x = R.pair_inputs(m if stage == GU else m * top_k, k, F16, 16)
    gates = torch.softmax(torch.randn(m, top_k, generator=torch.Generator().manual_seed(7)), dim=1)
    res = R.make_inputs(m, n, k, F16, 17)[2]
    y = _run(stage, sd, x, ids, gates, res)
    ref, tol = (R.gate_up_ref64(raw, g, x, ids, E) if stage == GU else R.down_ref64(raw, g, x, ids, gates, E, res))
    _within(y, ref, tol, "m = 19")
    per = 1 if stage == GU else top_k
    parts = [_run(stage, sd, x[r0 * per:(r0 + 8) * per], ids[r0:r0 + 8], gates[r0:r0 + 8], res[r0:r0 + 8]) for r0 in (0, 8, 16)]
    assert torch.equal(y.view(torch.int16), torch.cat(parts).view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------------------
# graph replay
# ---------------------------------------------------------------------------------------------------------------------------------

def _block_tensors(oracle, E, hidden, il, g, dtype, top_k):
    from any4_amd.moe import MoEMLP, MoEWeights

    gu, _ = R.make_stack(oracle, E, 2 * il, hidden, g, "any4_rowwise", dtype, 3)
    dn, _ = R.make_stack(oracle, E, hidden, il, g, "any4_rowwise", dtype, 4)
    rw = R.router_inputs(1, hidden, E, dtype, 5)[1]
    return MoEMLP(rw.to(DEV), MoEWeights(R.to_dev(gu, DEV), R.to_dev(dn, DEV)), top_k)


def test_graph_replay_follows_the_router(oracle):
    """route -> gate_up -> down captured once; replays with other activations select other experts and give the uncaptured launches' bits."""
    block = _block_tensors(oracle, 8, 512, 192, 64, BF16, 2)
    m = 4
    xs = [R.router_inputs(m, 512, 8, BF16, seed)[0].to(DEV) for seed in (1, 2, 3)]
    rs = [R.make_inputs(m, 512, 512, BF16, seed)[2].to(DEV) for seed in (1, 2, 3)]
    eager = [block(x, residual=r) for x, r in zip(xs, rs)]
    from any4_amd import decode_ops as G

    picks = [G.moe_route(x, block.router, 2)[0].cpu() for x in xs]
    assert not torch.equal(picks[0], picks[1]) and not torch.equal(picks[1], picks[2]), "the activations do not move the selection"
    x, r = xs[0].clone(), rs[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        block(x, residual=r)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = block(x, residual=r)
    for xi, ri, want in list(zip(xs, rs, eager))[::-1]:
        x.copy_(xi)
        r.copy_(ri)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------------------
# the block and the stack against the plain-torch path
# ---------------------------------------------------------------------------------------------------------------------------------

def test_block_against_the_definition(oracle):
    """The three launches chained, against moe_ref in float64 on the same stacks (margins asserted first)."""
    from any4_amd.moe import MoEWeights, moe_ref

    E, hidden, il, g, top_k, m = 8, 512, 192, 64, 2, 8
    block = _block_tensors(oracle, E, hidden, il, g, BF16, top_k)
    gu, gu_raw = R.make_stack(oracle, E, 2 * il, hidden, g, "any4_rowwise", BF16, 3)
    dn, dn_raw = R.make_stack(oracle, E, hidden, il, g, "any4_rowwise", BF16, 4)
    x = R.router_inputs(m, hidden, E, BF16, 21)[0]
    res = R.make_inputs(m, hidden, hidden, BF16, 22)[2]
    rw = block.router.detach().cpu()
    ids64, _, logits, A, _ = R.route_ref64(x, rw, top_k)
    assert R.margin_ok(logits, A, top_k)[0].all()
    y = block(x.to(DEV), residual=res.to(DEV)).cpu()
    ref, ids, gates, _ = moe_ref(x, rw, MoEWeights(gu, dn), top_k, res, parts=True)
    assert np.array_equal(ids.numpy(), ids64)
    # the activation rows of the kernel and of the definition may differ by a rounding each (bounded in test_stage_f64); here the block's
    # output is held to the DOWN bound on the definition's own activations plus one ulp16 of every activation pushed through |W2|
    act = []
    for i in range(m):
        for s in range(top_k):
            gv = (x[i].double().numpy() @ R.weights64(gu_raw[int(ids[i, s])], g).T).reshape(-1, 2, 8)
            g16, u16 = (torch.from_numpy(np.ascontiguousarray(gv[:, j].reshape(-1))).to(BF16).double() for j in (0, 1))
            act.append(((g16 / (1 + torch.exp(-g16))).to(BF16).double() * u16).to(BF16))
    act = torch.stack(act)
    ref64, tol = R.down_ref64(dn_raw, g, act, ids.numpy(), gates.float(), E, res)
    extra = np.zeros_like(ref64)
    for i in range(m):
        for s in range(top_k):
            a = act[i * top_k + s].double().numpy()
            extra[i] += float(gates[i, s]) * (2.0 ** -7 * np.abs(a)) @ np.abs(R.weights64(dn_raw[int(ids[i, s])], g)).T
    _within(y, ref64, tol + extra, "block")
    assert (np.abs(ref.double().numpy() - ref64) <= tol).all()


STACK = dict(hidden=512, inter=192, layers=2, heads=4, kv_heads=2, head_dim=64, vocab=256, max_seq=64, group_size=64, gate_up_interleave=8,
             experts=4, experts_per_token=2)
T0, STEPS = 5, 6


def _pair(bs, ragged, five, seed=3, **kw):
    """(the fused stack, its plain-torch twin on the same weights with the router's logits recorded)"""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**STACK)
    mk = lambda **k2: DecodeStack(cfg, Any4Factory(cfg, DEV, seed=seed), DEV, bs=bs, seed=9, ragged=ragged, **kw, **k2)
    fused, plain = mk(fused=True, fuse_gemm_stages=five), mk(fused=False)
    assert fused._five_launch() == five and all(layer.launches() >= 7 for layer in fused.layers)
    for layer in plain.layers:
        layer.moe.record = []
    return cfg, fused, plain


def _margins(plain, top_k=2):
    """The router-margin condition on everything the plain-torch path recorded since the last call: no row may be left out."""
    for layer in plain.layers:
        for logits, x in layer.moe.record:
            A = R.SLACK * (x.double().abs() @ layer.moe.router.double().abs().t()).cpu().numpy()
            ok, worst = R.margin_ok(logits.double().cpu().numpy(), A, top_k)
            assert ok.all(), f"layer {layer.idx}: a row within {worst:.2f} of a tie; choose another seed"
        layer.moe.record.clear()


def _contract(a, b, what):
    a, b = a.float(), b.float()
    assert torch.isfinite(a).all(), what
    assert (a - b).abs().max() <= 0.03 * b.abs().max() + 1e-3, (what, float((a - b).abs().max()), float(b.abs().max()))   # tests/test_gpu_decode.py


def _drive(cfg, stacks, bs, ragged, check):
    """A prefill of T0 tokens and STEPS decode steps on every stack; check(outputs, what) after each."""
    toks = torch.randint(0, cfg.vocab, (bs, T0 + STEPS), generator=torch.Generator().manual_seed(1)).to(DEV)
    lengths = [5, 3, 4][:bs]
    if ragged:
        check([s.prefill(toks[:, :T0], position=0, lengths=lengths) for s in stacks], "prefill")
    else:
        check([s.prefill(toks[:, :T0], position=0) for s in stacks], "prefill")
    for i in range(STEPS):
        position = [n + i for n in lengths] if ragged else T0 + i
        check([s.decode(toks[:, T0 + i], position).clone() for s in stacks], f"step {i}")


@pytest.mark.parametrize("five", [False, True], ids=["8-launch", "5-launch"])
@pytest.mark.parametrize("ragged", [False, True], ids=["", "ragged"])
@pytest.mark.parametrize("bs", [1, 3])
def test_stack_against_plain_torch(bs, ragged, five):
    cfg, fused, plain = _pair(bs, ragged, five)

    def check(outs, what):
        _margins(plain)
        _contract(outs[0], outs[1], what)

    _drive(cfg, (fused, plain), bs, ragged, check)


@pytest.mark.parametrize("five", [False, True], ids=["8-launch", "5-launch"])
def test_stack_captured(five):
    """The captured step gives the eager step's bits while the tokens move the selection, and stays within the plain path's contract."""
    cfg, eager, plain = _pair(3, True, five)
    graph = _pair(3, True, five)[1]
    graph.capture()
    assert graph._graph is not None

    def check(outs, what):
        _margins(plain)
        assert torch.equal(outs[0], outs[1]), what
        _contract(outs[0], outs[2], what)

    _drive(cfg, (graph, eager, plain), 3, True, check)


def test_stack_paged_mx8_and_sampling():
    """The MoE block under a paged mx8 cache, and a sampled generate: the block sees [rows][hidden] only."""
    cfg, fused, plain = _pair(3, True, True, kv_cache="mx8", kv_pages=6, page_size=64)

    def check(outs, what):
        _margins(plain)
        _contract(outs[0], outs[1], what)

    _drive(cfg, (fused, plain), 3, True, check)
    cfg, a, _ = _pair(2, False, True)
    b = _pair(2, False, False)[1]
    prompt = torch.randint(0, cfg.vocab, (2, 4), generator=torch.Generator().manual_seed(3)).to(DEV)
    ta, ta2 = (a.generate(prompt, 5, temperature=0.8, top_k=20, top_p=0.9, seed=11) for _ in range(2))
    assert ta.shape == (2, 5) and torch.equal(ta, ta2) and int(ta.min()) >= 0 and int(ta.max()) < cfg.vocab
    assert b.generate(prompt, 5, temperature=0.8, top_k=20, top_p=0.9, seed=11).shape == (2, 5)
