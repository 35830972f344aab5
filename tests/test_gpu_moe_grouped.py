"""The grouped mixture-of-experts path on the GPU (dg_moe_group, dg_moe_launch with DG_MOE_GROUPED) against group_ref in every int and the float64
references and bounds of tests/moe_grouped_ref.py; exact probes, row independence, determinism, the block and the decode stack with
moe_grouped_from.  Tile sizes come from the plan, never from a literal.  Run: pytest -m gpu."""
import functools

import numpy as np
import pytest
import torch

from tests import moe_grouped_ref as GR
from tests import moe_ref as R
from tests.moe_ref import BF16, F16

pytestmark = pytest.mark.gpu
DEV = "cuda"
GU, DN = GR.GU, GR.DN
E, TOP_K, HIDDEN, IL, G64 = 8, 2, 512, 192, 64      # gate_up [384][512], down [512][192] (three super-tiles: one per step)
INT_MAX = 2 ** 31 - 1


def _bm():
    return GR.plan(GU, 2 * IL, HIDDEN, 9, TOP_K)[0]


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _rand_ids(m, top_k=TOP_K, n_experts=E, seed=0):
    return np.random.default_rng(seed + m).integers(0, n_experts, (m, top_k)).astype(np.int32)


def _dt(dtype):
    return "bf16" if dtype == BF16 else "fp16"


# the stage cases: (name, ids, stage, n, k, g, qtype, dtype, residual)
def _stage_cases():
    bm = _bm()
    crafted = GR.crafted_ids(bm)
    out = []
    for stage, n, k in ((GU, 2 * IL, HIDDEN), (DN, HIDDEN, IL)):
        out += [("m9", _rand_ids(9), stage, n, k, G64, "any4_rowwise", BF16, True), ("m70", _rand_ids(70), stage, n, k, G64, "int4", F16, False)]
        out += [("crafted", crafted, stage, n, k, G64, q, d, True) for q, d in (("int4", BF16), ("any4_global", F16), ("any4_rowwise", BF16),
                                                                                 ("any4_rowwise", F16))]
    out.append(("m70", _rand_ids(70), DN, HIDDEN, 256, 128, "any4_rowwise", BF16, True))    # four super-tiles, g = 128: two per step
    return out


def regime_cases():
    """(ids, E, stage, n, k, top_k) of every stage case (tests/test_moe_grouped_cpu.py asserts the regimes without a GPU, too)."""
    return [(c[1], E, c[2], c[3], c[4], c[1].shape[1]) for c in _stage_cases()]


def _cid(c):
    return f"{'gate_up' if c[2] == GU else 'down'}-{c[0]}-k{c[4]}-g{c[5]}-{c[6]}-{_dt(c[7])}"


@functools.lru_cache(maxsize=None)
def _dev_stack(oracle, n, k, g, qtype, dtype, seed=0):
    stack, raw = R.make_stack(oracle, E, n, k, g, qtype, dtype, seed)
    return R.to_dev(stack, DEV), raw, stack


def _group(ids):
    """dg_moe_group into a guarded workspace: the int32 image on the CPU and the device tensor."""
    from any4_amd import decode_ops as G

    m, top_k = ids.shape
    bm, _, _, _, _, gbytes, _ = GR.plan(GU, 2 * IL, HIDDEN, m, top_k)
    view, whole = R.guarded(torch.zeros(gbytes // 2, dtype=torch.int16), DEV, fill=R.SENTINEL)
    view.fill_(R.SENTINEL)
    ws = view.view(torch.int32)
    G.moe_group(_i32(ids), E, bm, ws)
    torch.cuda.synchronize()
    assert R.guard_intact(view, whole), "dg_moe_group wrote outside its workspace"
    return ws.cpu().numpy().copy(), ws


def _run(stage, stack, x, ids, gates=None, res=None, alias=False):
    """group + one grouped launch into a guarded output, the f32 workspace pre-filled with NaN; returns y on the CPU."""
    from any4_amd import decode_ops as G

    m, top_k = ids.shape
    _, ws = _group(ids)
    dids = _i32(ids)
    shape = (m * top_k, stack.n // 2) if stage == GU else (m, stack.n)
    view, whole = R.guarded(torch.zeros(shape, dtype=x.dtype), DEV, fill=R.SENTINEL)
    view.view(torch.int16).fill_(R.SENTINEL)
    if stage == GU:
        G.moe_gate_up_grouped(x.to(DEV), stack, dids, ws, out=view)
    else:
        fws = torch.full((m * top_k, stack.n), float("nan"), dtype=torch.float32, device=DEV)
        r = None if res is None else res.to(DEV)
        if alias:
            view.copy_(r)
            r = view
        G.moe_down_grouped(x.to(DEV), stack, dids, gates.to(DEV), ws, r, out=view, f32_ws=fws)
    torch.cuda.synchronize()
    assert R.guard_intact(view, whole), "wrote outside the output"
    return view.cpu()


def _within(y, ref, tol, what):
    err = np.abs(y.double().numpy() - ref)
    bad = err > tol
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(tol > 0, err / tol, 0))
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert np.isfinite(y.float().numpy()).all(), f"{what}: not finite"
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} outside the bound; worst ratio {worst:.2f} at {np.argwhere(bad)[:4].tolist()}"


def _gates(m, top_k, seed=5):
    return torch.softmax(torch.randn(m, top_k, generator=torch.Generator().manual_seed(seed)), dim=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the group kernel: every int
# ---------------------------------------------------------------------------------------------------------------------------------

def _group_id_cases():
    bm = _bm()
    out = [(f"random m={m}", _rand_ids(m)) for m in (1, 9, 70, 300)]
    out.append(("crafted counts", GR.crafted_ids(bm)))
    out.append(("one expert, top_k = 1", np.full((2 * bm + 5, 1), 3, np.int32)))
    bad = _rand_ids(70, seed=3)
    bad[::7, 0], bad[3::11, 1], bad[5::13, 0] = -1, E, INT_MAX
    out.append(("invalid ids", bad))
    return out


@pytest.mark.parametrize("name,ids", _group_id_cases(), ids=[c[0] for c in _group_id_cases()])
def test_group_kernel_equals_group_ref(name, ids):
    from any4_amd.moe import group_ref

    want = group_ref(ids, E, _bm()).workspace
    got, _ = _group(ids)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} ints differ, first at {bad[:8].tolist()}: {got[bad[:8]].tolist()} != {want[bad[:8]].tolist()}"
    again, _ = _group(ids)
    assert np.array_equal(got, again), "two launches differ"


# ---------------------------------------------------------------------------------------------------------------------------------
# the two stages against float64
# ---------------------------------------------------------------------------------------------------------------------------------

def test_regimes_reached():
    GR.assert_regimes_reached(regime_cases(), device=torch.cuda.current_device())


@pytest.mark.parametrize("case", _stage_cases(), ids=_cid)
def test_stage_f64(oracle, case):
    _, ids, stage, n, k, g, qtype, dtype, with_res = case
    sd, raw, _ = _dev_stack(oracle, n, k, g, qtype, dtype)
    m, top_k = ids.shape
    if stage == GU:
        x = R.pair_inputs(m, k, dtype, 1)
        ref, tol = GR.gate_up_ref64(oracle, raw, g, qtype, x, ids, E)
        y = _run(GU, sd, x, ids)
    else:
        x = R.pair_inputs(m * top_k, k, dtype, 2)
        gates = _gates(m, top_k)
        res = R.make_inputs(m, n, k, dtype, 3)[2] if with_res else None
        ref, tol = GR.down_ref64(oracle, raw, g, qtype, x, ids, gates, E, res)
        y = _run(DN, sd, x, ids, gates, res)
    _within(y, ref, tol, _cid(case))


# ---------------------------------------------------------------------------------------------------------------------------------
# exact probes
# ---------------------------------------------------------------------------------------------------------------------------------

def _onehot_batch(k, dtype):
    """top_k = 1, the crafted counts as ids [P][1]; row i is 1.0 at column (37 i + 5) mod k: every tile shape, many columns."""
    ids = GR.crafted_ids(_bm(), top_k=1)
    m = ids.shape[0]
    cols = (37 * np.arange(m) + 5) % k
    cols[:4] = (0, k - 1, 63, 64)
    x = torch.zeros(m, k, dtype=dtype)
    x[torch.arange(m), torch.from_numpy(cols)] = 1.0
    return ids, cols, x


@pytest.mark.parametrize("qtype,dtype", [("any4_rowwise", BF16), ("any4_global", F16), ("int4", BF16)])
def test_onehot_down_returns_the_named_experts_weights(oracle, qtype, dtype):
    """top_k = 1, gate 1.0, no residual, activation row i is 1.0 at column j(i): y[i][r] is the oracle's 16-bit weight of expert ids[i], row r,
    column j(i), bit for bit, for every row of the crafted batch -- a wrong expert stride, gathered row, tile row, nibble or group shows."""
    sd, raw, _ = _dev_stack(oracle, HIDDEN, IL, G64, qtype, dtype)
    ids, cols, x = _onehot_batch(IL, dtype)
    y = _run(DN, sd, x, ids, torch.ones(ids.shape[0], 1))
    w16 = [R.weights16(oracle, raw[e], G64, qtype, dtype) for e in range(E)]
    want = torch.stack([w16[int(ids[i, 0])][:, cols[i]] for i in range(ids.shape[0])])
    want = (want.float() + 0.0).to(dtype)                   # (-0 among +0 products sums to +0)
    bad = y.view(torch.int16) != want.contiguous().view(torch.int16)
    assert not bad.any(), f"{int(bad.sum())} / {bad.numel()} differ; (row, weight row) {torch.nonzero(bad)[:4].tolist()}"


@pytest.mark.parametrize("qtype,dtype", [("any4_rowwise", BF16), ("int4", F16)])
def test_onehot_gate_up_returns_the_swiglu_of_single_weights(oracle, qtype, dtype):
    """The same through the SwiGLU store (the lane exchange of gate row r and up row r + 8): expected = dg_swiglu of the named expert's
    gate and up weights of that column, bit for bit."""
    from any4_amd import decode_ops as G

    sd, raw, _ = _dev_stack(oracle, 2 * IL, HIDDEN, G64, qtype, dtype)
    ids, cols, x = _onehot_batch(HIDDEN, dtype)
    y = _run(GU, sd, x, ids)
    w16 = [R.weights16(oracle, raw[e], G64, qtype, dtype) for e in range(E)]
    rows = []
    for i in range(ids.shape[0]):
        w = (w16[int(ids[i, 0])][:, cols[i]].float() + 0.0).to(dtype).view(-1, 2, 8)
        rows.append(torch.cat([w[:, 0].reshape(-1), w[:, 1].reshape(-1)]))
    want = G.swiglu(torch.stack(rows).to(DEV).contiguous()).cpu()
    bad = y.view(torch.int16) != want.view(torch.int16)
    assert not bad.any(), f"{int(bad.sum())} / {bad.numel()} differ; (pair, column) {torch.nonzero(bad)[:4].tolist()}"


@pytest.mark.parametrize("stage", [GU, DN], ids=["gate_up", "down"])
def test_unselected_experts_are_never_read(oracle, stage):
    """Words, scales / zeros and LUT of every unselected expert become garbage / NaN: the output keeps its bits."""
    n, k = (2 * IL, HIDDEN) if stage == GU else (HIDDEN, IL)
    sd, raw, stack = _dev_stack(oracle, n, k, G64, "any4_rowwise", BF16)
    m = 40
    ids = np.array([[1, 3], [3, 6], [6, 1]] * 14, np.int32)[:m]
    x = R.pair_inputs(m if stage == GU else m * TOP_K, k, BF16, 7)
    gates = _gates(m, TOP_K, 8)
    clean = _run(stage, sd, x, ids, gates)
    words, qinfo, lut = stack.words.clone(), stack.qinfo.clone(), stack.lut.clone()
    for e in (0, 2, 4, 5, 7):
        words[e] = torch.randint(-2 ** 31, 2 ** 31 - 1, words[e].shape, generator=torch.Generator().manual_seed(e)).to(torch.int32)
        qinfo[e], lut[e] = float("nan"), float("nan")
    dirty = _run(stage, R.to_dev(stack, DEV, words=words, qinfo=qinfo, lut=lut), x, ids, gates)
    assert torch.equal(clean.view(torch.int16), dirty.view(torch.int16))
    ref, tol = (GR.gate_up_ref64(oracle, raw, G64, "any4_rowwise", x, ids, E) if stage == GU else
                GR.down_ref64(oracle, raw, G64, "any4_rowwise", x, ids, gates, E))
    _within(clean, ref, tol, "clean")


def test_invalid_ids_and_aliasing(oracle):
    """-1, E and 2^31 - 1: GATE_UP writes +0 rows, DOWN adds nothing (the NaN its f32 workspace holds there is never read); a row without a
    valid id gets the residual's bits, or zeros.  y aliasing residual gives the non-aliased bits."""
    qtype = "any4_rowwise"
    ids = _rand_ids(70, seed=4)
    ids[::7, 0], ids[3::11, 1], ids[5::13, 0], ids[14] = -1, E, INT_MAX, (-1, E)
    m, top_k = ids.shape
    sd, raw, _ = _dev_stack(oracle, HIDDEN, IL, G64, qtype, BF16)
    x = R.pair_inputs(m * top_k, IL, BF16, 13)
    gates = _gates(m, top_k, 9)
    res = R.make_inputs(m, HIDDEN, IL, BF16, 14)[2]
    y = _run(DN, sd, x, ids, gates, res)
    _within(y, *GR.down_ref64(oracle, raw, G64, qtype, x, ids, gates, E, res), "down with invalid ids")
    assert torch.equal(y[14].view(torch.int16), res[14].view(torch.int16))
    assert not _run(DN, sd, x, ids, gates, None)[14].view(torch.int16).any()
    assert torch.equal(_run(DN, sd, x, ids, gates, res, alias=True).view(torch.int16), y.view(torch.int16)), "y aliasing residual differs"
    gsd, graw, _ = _dev_stack(oracle, 2 * IL, HIDDEN, G64, qtype, BF16)
    xg = R.pair_inputs(m, HIDDEN, BF16, 15)
    a = _run(GU, gsd, xg, ids)
    _within(a, *GR.gate_up_ref64(oracle, graw, G64, qtype, xg, ids, E), "gate_up with invalid ids")
    invalid = torch.from_numpy(((ids < 0) | (ids >= E)).reshape(-1))
    assert invalid.sum() > 10 and not a[invalid].view(torch.int16).any() and a[~invalid].view(torch.int16).any(dim=1).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# row independence and determinism
# ---------------------------------------------------------------------------------------------------------------------------------

def _block(oracle, dtype=BF16, grouped_from=None, top_k=TOP_K):
    from any4_amd.moe import MoEMLP, MoEWeights

    gu = _dev_stack(oracle, 2 * IL, HIDDEN, G64, "any4_rowwise", dtype, 3)[0]
    dn = _dev_stack(oracle, HIDDEN, IL, G64, "any4_rowwise", dtype, 4)[0]
    rw = R.router_inputs(1, HIDDEN, E, dtype, 5)[1]
    return MoEMLP(rw.to(DEV), MoEWeights(gu, dn), top_k, grouped_from=grouped_from)


def _two_stages(oracle, x, ids, gates, res):
    """grouped gate_up chained into grouped down on given ids and gates: y on the CPU."""
    gu = _dev_stack(oracle, 2 * IL, HIDDEN, G64, "any4_rowwise", BF16, 3)[0]
    dn = _dev_stack(oracle, HIDDEN, IL, G64, "any4_rowwise", BF16, 4)[0]
    return _run(DN, dn, _run(GU, gu, x, ids), ids, gates, res)


def test_row_independence(oracle):
    """The output bits of token i in the m = 300 launch equal those of an m = 1 launch of that token with its ids and gates."""
    m = 300
    ids = _rand_ids(m, n_experts=3, seed=6)               # 600 pairs on three experts: each spans two tiles
    x = R.pair_inputs(m, HIDDEN, BF16, 21)
    gates = _gates(m, TOP_K, 22)
    res = R.make_inputs(m, HIDDEN, HIDDEN, BF16, 23)[2]
    y = _two_stages(oracle, x, ids, gates, res)
    from any4_amd.moe import group_ref

    G = group_ref(ids, E, _bm())
    assert G.n_tiles > 3 and (G.tiles[:G.n_tiles, 2] < _bm()).any()   # first (full) and second (partial) tiles: the rows below sit in both kinds
    for i in (0, 1, 77, 150, 223, 298, 299):
        one = _two_stages(oracle, x[i:i + 1], ids[i:i + 1], gates[i:i + 1], res[i:i + 1])
        assert torch.equal(one.view(torch.int16), y[i:i + 1].view(torch.int16)), f"token {i} depends on its batch"


def test_launch_to_launch_determinism(oracle):
    ids = GR.crafted_ids(_bm())
    m = ids.shape[0]
    x = R.pair_inputs(m, HIDDEN, BF16, 24)
    gates = _gates(m, TOP_K, 25)
    res = R.make_inputs(m, HIDDEN, HIDDEN, BF16, 26)[2]
    a, b = (_two_stages(oracle, x, ids, gates, res) for _ in range(2))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------------------
# the block and the stack
# ---------------------------------------------------------------------------------------------------------------------------------

def test_block_against_the_definition(oracle):
    """MoEMLP(grouped_from=16) on 70 rows: route, group, grouped gate_up, grouped down against moe_grouped_ref (margins asserted first)."""
    from any4_amd.moe import MoEWeights, moe_grouped_ref

    m = 70
    block = _block(oracle, grouped_from=16)
    _, gu_raw, gu = _dev_stack(oracle, 2 * IL, HIDDEN, G64, "any4_rowwise", BF16, 3)
    _, dn_raw, dn = _dev_stack(oracle, HIDDEN, IL, G64, "any4_rowwise", BF16, 4)
    x = R.router_inputs(m, HIDDEN, E, BF16, 21)[0]
    res = R.make_inputs(m, HIDDEN, HIDDEN, BF16, 22)[2]
    rw = block.router.detach().cpu()
    ids64, _, logits, A, _ = R.route_ref64(x, rw, TOP_K)
    ok, worst = R.margin_ok(logits, A, TOP_K)
    assert ok.all(), f"rows {np.nonzero(~ok)[0].tolist()} are too close to a tie (ratio {worst:.2f}): no row may be left out"
    y = block(x.to(DEV), residual=res.to(DEV)).cpu()
    assert list(block._grouped) == [m]
    ref, ids, gates, _ = moe_grouped_ref(x, rw, MoEWeights(gu, dn), TOP_K, res, parts=True)
    assert np.array_equal(ids.numpy(), ids64)
    # as tests/test_gpu_moe.py: the DOWN bound on the definition's own activations plus one ulp16 of every activation pushed through |W2|
    act = GR.act16_ref(oracle, gu_raw, G64, "any4_rowwise", x, ids.numpy(), E)
    ref64, tol = GR.down_ref64(oracle, dn_raw, G64, "any4_rowwise", act, ids.numpy(), gates.float(), E, res)
    extra = np.zeros_like(ref64)
    for i in range(m):
        for s in range(TOP_K):
            a = act[i * TOP_K + s].double().numpy()
            extra[i] += float(gates[i, s]) * (2.0 ** -7 * np.abs(a)) @ np.abs(GR.w16_64(oracle, dn_raw, int(ids[i, s]), G64, "any4_rowwise", BF16)).T
    _within(y, ref64, tol + extra, "block")
    assert (np.abs(ref.double().numpy() - ref64) <= tol).all()
    # below grouped_from the same module runs the GEMV launches and allocates no grouped buffer
    block(x[:8].to(DEV), residual=res[:8].to(DEV))
    assert list(block._grouped) == [m]


STACK = dict(hidden=512, inter=192, layers=2, heads=4, kv_heads=2, head_dim=64, vocab=256, max_seq=64, group_size=64, gate_up_interleave=8,
             experts=4, experts_per_token=2)
T, BS, STEPS = 24, 3, 3
LENGTHS = [24, 17, 20]


def _stacks(grouped_from, seed=3, ragged=True):
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**STACK, moe_grouped_from=grouped_from)
    mk = lambda **k2: DecodeStack(cfg, Any4Factory(cfg, DEV, seed=seed), DEV, bs=BS, seed=9, ragged=ragged, **k2)
    fused, plain = mk(fused=True), mk(fused=False)
    for layer in plain.layers:
        layer.moe.record = []
    return cfg, fused, plain


def _margins(plain, top_k=2):
    for layer in plain.layers:
        for logits, x in layer.moe.record:
            A = R.SLACK * (x.double().abs() @ layer.moe.router.double().abs().t()).cpu().numpy()
            ok, worst = R.margin_ok(logits.double().cpu().numpy(), A, top_k)
            assert ok.all(), f"layer {layer.idx}: a row within {worst:.2f} of a tie; choose another seed"
        layer.moe.record.clear()


def _contract(a, b, what):
    a, b = a.float(), b.float()
    assert torch.isfinite(a).all(), what
    assert (a - b).abs().max() <= 0.03 * b.abs().max() + 1e-3, (what, float((a - b).abs().max()), float(b.abs().max()))   # tests/test_gpu_moe.py


def _tokens(cfg, seed=3):
    """(seed 3: the router margins the stack test asserts are 65 times the allowance; with seed 1 one row of layer 0 sits at 0.12)"""
    return torch.randint(0, cfg.vocab, (BS, T + STEPS), generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_stack_prefill_and_decode_against_plain_torch():
    """Two MoE layers with moe_grouped_from = 16: a ragged prefill of T = 24 at bs 3 (72 rows: grouped), then decode steps (3 rows: the
    GEMV launches), against the plain-torch stack within the existing stack tests' tolerance."""
    cfg, fused, plain = _stacks(16)
    toks = _tokens(cfg)
    a, b = (s.prefill(toks[:, :T], position=0, lengths=LENGTHS) for s in (fused, plain))
    _margins(plain)
    _contract(a, b, "prefill")
    assert all(list(layer.moe._grouped) == [BS * T] for layer in fused.layers), "the prefill did not take the grouped path"
    for i in range(STEPS):
        position = [n + i for n in LENGTHS]
        a, b = (s.decode(toks[:, T + i], position).clone() for s in (fused, plain))
        _margins(plain)
        _contract(a, b, f"step {i}")
    assert all(list(layer.moe._grouped) == [BS * T] for layer in fused.layers)


def test_stack_with_the_option_off_issues_no_grouped_launch():
    cfg, fused, plain = _stacks(0)
    toks = _tokens(cfg)
    a, b = (s.prefill(toks[:, :T], position=0, lengths=LENGTHS) for s in (fused, plain))
    _contract(a, b, "prefill")
    assert all(layer.moe.grouped_from is None and not layer.moe._grouped for layer in fused.layers)


def test_captured_block_follows_the_router(oracle):
    """The grouped block on 72 rows captured once and replayed with other activations: other experts, the eager launches' bits."""
    from any4_amd import decode_ops as G

    block = _block(oracle, grouped_from=16)
    m = BS * T
    xs = [R.router_inputs(m, HIDDEN, E, BF16, seed)[0].to(DEV) for seed in (1, 2, 3)]
    rs = [R.make_inputs(m, HIDDEN, HIDDEN, BF16, seed)[2].to(DEV) for seed in (1, 2, 3)]
    eager = [block(x, residual=r).clone() for x, r in zip(xs, rs)]
    picks = [G.moe_route(x, block.router, TOP_K)[0].cpu() for x in xs]
    assert not torch.equal(picks[0], picks[1]) and not torch.equal(picks[1], picks[2]), "the activations do not move the selection"
    x, r = xs[0].clone(), rs[0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = block(x, residual=r)
    for xi, ri, want in list(zip(xs, rs, eager))[::-1]:
        x.copy_(xi)
        r.copy_(ri)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), want.view(torch.int16))


def test_captured_prefill_follows_the_router():
    """The same prefill (T = 24 at bs 3, position=None: the stack's prefill_pos buffer) captured and replayed twice with different tokens;
    both replays equal the eager prefill of those tokens."""
    cfg, eager, _ = _stacks(16, ragged=False)
    graphed = _stacks(16, ragged=False)[1]
    toks = [_tokens(cfg, seed)[:, :T].contiguous() for seed in (1, 2)]
    want = [eager.prefill(t, position=0).clone() for t in toks]
    assert not torch.equal(want[0], want[1])
    assert torch.equal(graphed.prefill(toks[0], position=0), want[0])   # warm-up: every buffer exists before the capture; prefill_pos = 0
    buf = toks[0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = graphed.prefill(buf, position=None)
    for t, w in list(zip(toks, want))[::-1]:
        buf.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, w)
    assert all(list(layer.moe._grouped) == [BS * T] for layer in graphed.layers)
