"""The grouped mixture-of-experts path without a GPU: group_ref's properties, moe_grouped_ref against an independent per-token loop, the
helper's references (tests/moe_grouped_ref.py) against it, the plan, the C ABI (symbols, every refusal of the grouped kernel before a launch) and the
defaults that keep the module on its GEMV launches.  Run: pytest -m "not gpu"."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import moe_grouped_ref as GR
from tests import moe_ref as R

BF16, F16 = torch.bfloat16, torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1


def _bm():
    return GR.plan(GR.GU, 384, 512, 9, 2)[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# group_ref
# ---------------------------------------------------------------------------------------------------------------------------------

def _ids_cases():
    bm = _bm()
    rng = np.random.default_rng(0)
    yield "random m=1", rng.integers(0, 8, (1, 2)), 8, bm
    yield "random m=70", rng.integers(0, 8, (70, 2)), 8, bm
    yield "random m=300 top 3", rng.integers(0, 5, (300, 3)), 5, bm
    yield "small tiles", rng.integers(0, 8, (40, 2)), 8, 4
    yield "crafted", GR.crafted_ids(bm), 8, bm
    yield "one expert", np.full((2 * bm + 5, 1), 3), 8, bm
    bad = rng.integers(0, 8, (50, 2))
    bad[::7, 0], bad[3::11, 1], bad[5::13, 0], bad[1, 1] = -1, 8, INT_MAX, -2 ** 31
    yield "invalid ids", bad, 8, bm
    yield "all invalid", np.full((3, 2), -1), 8, bm


@pytest.mark.parametrize("name,ids,E,bm", list(_ids_cases()), ids=[c[0] for c in _ids_cases()])
def test_group_ref_properties(name, ids, E, bm):
    from any4_amd.moe import GROUP_PERM, group_ref

    G = group_ref(ids, E, bm)
    flat = np.asarray(ids, np.int64).reshape(-1)
    P = flat.size
    ok = (flat >= 0) & (flat < E)
    perm = G.perm[:G.n_valid]
    # a permutation of the valid pairs, sorted by (expert, pair): the stable order
    assert sorted(perm.tolist()) == np.nonzero(ok)[0].tolist() and (G.perm[G.n_valid:] == -1).all()
    keys = [(int(flat[p]), int(p)) for p in perm]
    assert keys == sorted(keys)
    # invalid ids land in invalid[] only
    assert G.invalid[:G.n_invalid].tolist() == np.nonzero(~ok)[0].tolist() and (G.invalid[G.n_invalid:] == -1).all()
    assert G.n_valid + G.n_invalid == P
    # count and its prefix
    assert G.count.tolist() == [int((flat == e).sum()) for e in range(E)]
    assert G.offset.tolist() == [0] + np.cumsum(G.count).tolist() and G.offset[E] == G.n_valid
    # the tiles cover perm exactly once, never cross an expert, hold at most bm rows; their number is within the bound
    covered = []
    for e, first, rows in G.tiles[:G.n_tiles].tolist():
        assert 1 <= rows <= bm and G.offset[e] <= first and first + rows <= G.offset[e + 1]
        covered += range(first, first + rows)
    assert covered == list(range(G.n_valid))
    assert G.tiles[:G.n_tiles, 0].tolist() == sorted(G.tiles[:G.n_tiles, 0].tolist())
    assert G.n_tiles == sum(-(-int(c) // bm) for c in G.count) <= G.bound == -(-P // bm) + min(E, P)
    assert not G.tiles[G.n_tiles:].any()
    # the workspace image
    ws = G.workspace
    assert ws.dtype == np.int32 and ws.size == GROUP_PERM + 2 * P + 3 * G.bound
    assert ws[:4].tolist() == [G.n_tiles, G.n_invalid, G.n_valid, bm] and ws[4:4 + E].tolist() == G.count.tolist()
    assert ws[68:69 + E].tolist() == G.offset.tolist() and np.array_equal(ws[GROUP_PERM:GROUP_PERM + P], G.perm)
    assert np.array_equal(ws[GROUP_PERM + P:GROUP_PERM + 2 * P], G.invalid) and np.array_equal(ws[GROUP_PERM + 2 * P:], G.tiles.reshape(-1))


def test_crafted_counts_and_regimes():
    from any4_amd.moe import group_ref

    bm = _bm()
    ids = GR.crafted_ids(bm)
    G = group_ref(ids, 8, bm)
    assert set(G.count.tolist()) == {0, 1, bm - 1, bm, bm + 1, 2 * bm + 3}
    from tests.test_gpu_moe_grouped import regime_cases

    GR.assert_regimes_reached(regime_cases())


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------------------

def _weights(oracle, E, il, hidden, g, qtype, dtype, seed=0):
    from any4_amd.moe import MoEWeights

    gu, gu_raw = R.make_stack(oracle, E, 2 * il, hidden, g, qtype, dtype, seed)
    dn, dn_raw = R.make_stack(oracle, E, hidden, il, g, qtype, dtype, seed + 1)
    return MoEWeights(gu, dn), gu_raw, dn_raw


def _loop_ref(oracle, x16, rw16, gu_raw, dn_raw, g, qtype, top_k, res16):
    """Token by token, expert by expert, float64 numpy over the ORACLE's 16-bit weights: (y64 [m][hidden], ids, gates)."""
    dt = x16.dtype
    r16 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt).double().numpy()
    m, E = x16.shape[0], rw16.shape[0]
    x, rw = x16.double().numpy(), rw16.double().numpy()
    out, ids_all, gates_all = [], [], []
    for i in range(m):
        l = np.array([float(np.dot(rw[e], x[i])) for e in range(E)])
        p = np.exp(l - l.max())
        p /= p.sum()
        ids = sorted(range(E), key=lambda e: (-p[e], e))[:top_k]
        gates = np.array([p[e] for e in ids]) / sum(p[e] for e in ids)
        y = np.zeros(dn_raw[0][0].shape[0])
        for e, gt in zip(ids, gates):
            gu = (GR.w16_64(oracle, gu_raw, e, g, qtype, dt) @ x[i]).reshape(-1, 2, 8)
            gate, up = r16(gu[:, 0].reshape(-1)), r16(gu[:, 1].reshape(-1))
            a = r16(r16(gate / (1 + np.exp(-gate))) * up)
            y += gt * (GR.w16_64(oracle, dn_raw, e, g, qtype, dt) @ a)
        out.append(y + (0 if res16 is None else res16[i].double().numpy()))
        ids_all.append(ids)
        gates_all.append(gates)
    return np.stack(out), np.array(ids_all), np.stack(gates_all)


@pytest.mark.parametrize("E,top_k,qtype,dtype,res", [(4, 2, "any4_rowwise", BF16, True), (1, 1, "int4", BF16, False), (5, 1, "any4_global", F16, True),
                                                      (3, 3, "any4_rowwise", F16, False)])
def test_moe_grouped_ref_against_a_per_token_loop(oracle, E, top_k, qtype, dtype, res):
    from any4_amd.moe import moe_grouped_ref, moe_ref

    hidden, il, g, m = 128, 64, 64, 5
    W, gu_raw, dn_raw = _weights(oracle, E, il, hidden, g, qtype, dtype)
    # the package's rounded weights are the oracle's, bit for bit
    for st, raw in ((W.gate_up, gu_raw), (W.down, dn_raw)):
        for e in range(E):
            assert np.array_equal(st.weights_rounded64(e).numpy(), GR.w16_64(oracle, raw, e, g, qtype, dtype))
    x, rw = R.router_inputs(m, hidden, E, dtype, seed=3)
    r = R.make_inputs(m, hidden, hidden, dtype, 4)[2] if res else None
    y, ids, gates, _ = moe_grouped_ref(x, rw, W, top_k, r, parts=True)
    y64, ids2, gates2 = _loop_ref(oracle, x, rw, gu_raw, dn_raw, g, qtype, top_k, r)
    assert np.array_equal(ids.numpy(), ids2)
    assert np.abs(gates.numpy() - gates2).max() < 1e-12
    err = np.abs(y.double().numpy() - y64)
    assert (err <= R.contract(y64, 0 * y64, dtype)).all(), err.max()
    # "rounded" is moe_ref's option, and it is not the default
    assert torch.equal(y, moe_ref(x, rw, W, top_k, r, weights="rounded"))
    with pytest.raises(ValueError):
        moe_ref(x, rw, W, top_k, r, weights="other")


def test_helper_references_against_the_definition(oracle):
    """gate_up_ref64 chained into down_ref64 (the helper's, on the oracle's weights) against moe_ref(weights="rounded")."""
    from any4_amd.moe import moe_ref

    E, hidden, il, g, top_k, m, qtype = 4, 128, 64, 64, 2, 6, "any4_rowwise"
    W, gu_raw, dn_raw = _weights(oracle, E, il, hidden, g, qtype, BF16, 5)
    x, rw = R.router_inputs(m, hidden, E, BF16, seed=6)
    res = R.make_inputs(m, hidden, hidden, BF16, 7)[2]
    y, ids, gates, _ = moe_ref(x, rw, W, top_k, res, parts=True, weights="rounded")
    act64, atol = GR.gate_up_ref64(oracle, gu_raw, g, qtype, x, ids.numpy(), E)
    act16 = GR.act16_ref(oracle, gu_raw, g, qtype, x, ids.numpy(), E)
    assert (np.abs(act16.double().numpy() - act64) <= atol).all()   # the definition's 16-bit activations lie within the GATE_UP bound
    ref, tol = GR.down_ref64(oracle, dn_raw, g, qtype, act16, ids.numpy(), gates.float(), E, res)
    # (the f32 gates differ from the float64 ones by 2^-24 relative: inside the slack)
    assert (np.abs(y.double().numpy() - ref) <= tol).all()
    # invalid ids: zero rows, nothing added
    bad = ids.numpy().copy()
    bad[0, 0], bad[2, 1] = -1, E
    a2, t2 = GR.gate_up_ref64(oracle, gu_raw, g, qtype, x, bad, E)
    assert not a2[0].any() and not t2[0].any() and not a2[2 * top_k + 1].any() and np.array_equal(a2[1], act64[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# plan and C ABI
# ---------------------------------------------------------------------------------------------------------------------------------

def test_plan_for_the_mixtral_shape():
    """The header's byte formulas: group workspace 4 (136 + 2 P + 3 bound), bound = ceil(P / bm) + min(E, P); f32 workspace 4 P wrows."""
    for T in (64, 512):
        P = 2 * T
        bm, bn, bound, tiles_n, ks, gbytes, fbytes = GR.plan(GR.GU, 28672, 4096, T, 2, g=128)
        assert bound == -(-P // bm) + 8 and tiles_n == -(-28672 // bn) and ks == 2
        assert gbytes == 4 * (136 + 2 * P + 3 * bound) and fbytes == 0
        bm2, bn2, bound2, tiles_n2, ks2, gbytes2, fbytes2 = GR.plan(GR.DN, 4096, 14336, T, 2, g=128)
        assert (bm2, bn2, bound2, gbytes2) == (bm, bn, bound, gbytes) and tiles_n2 == -(-4096 // bn) and ks2 == 2
        assert fbytes2 == 4 * P * 4096
    assert GR.plan(GR.DN, 512, 192, 9, 2)[4] == 1 and GR.plan(GR.DN, 512, 256, 9, 2, g=128)[4] == 2
    assert GR.plan(GR.GU, 384, 512, 1, 1, E=8)[2] == 1 + 1            # min(E, P) = 1


def test_symbols_are_declared_exported_and_bound():
    """(the struct's mirror: tests/test_moe_cpu.py -- both kernels share struct dg_moe)"""
    from any4_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "decode_glue_hip.h")).read()
    lib = _lib.load()
    for name in ("dg_moe_group", "dg_moe_launch", "dg_moe_plan"):
        assert re.search(r"TG_API\s+int\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes == _lib.SYMBOLS[name]
    assert lib.tg_abi_version() == _lib.TG_ABI_VERSION == 10


def _gws(P, E):
    """bytes of the group workspace (the header's formula, bm from the plan)"""
    return 4 * (136 + 2 * P + 3 * (-(-P // _bm()) + min(E, P)))


def _call(**over):
    from any4_amd import _lib

    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 63) & ~63
    kw = dict(kernel=_lib.DG_MOE_GROUPED, stage=_lib.DG_MOE_DOWN, x=p, w=p, qinfo=p, lut=p, y=p, ids=p, gates=p, residual=p, group_ws=p, f32_ws=p, stride_w=16,
              stride_qinfo=16, stride_lut=16, m=2, wrows=64, k=128, group_ws_bytes=_gws(4, 4), f32_ws_bytes=4 * 4 * 64, E=4, top_k=2,
              group=64, qtype=2, dtype=_lib.TG_BF16, inner_k_tiles=4)
    kw.update({k: (p + v[1] if isinstance(v, tuple) else v) for k, v in over.items()})
    c = _lib.Moe(**kw)
    c._keep = buf
    return c


def test_every_refusal_comes_before_a_launch():
    """Dummy pointers: a call that got as far as a launch would fault or fail on a machine without a GPU; each answers its own code, in
    the GEMV kernel's order (the one check_moe), the workspaces among them."""
    from any4_amd import _lib

    L = _lib.load()
    E = dict(null=-1, inner=-2, kdiv=-3, group=-4, dtype=-5, qtype=-6, shape=-7, align=-8, size=-10, layout=-12, struct=-14)
    launch = lambda c: L.dg_moe_launch(ctypes.byref(c), 0, None)
    assert L.dg_moe_launch(None, 0, None) == E["null"]
    assert launch(_call(struct_bytes=144)) == E["struct"]                   # ABI 9's dg_moe_w4
    assert launch(_call(struct_bytes=176)) == E["struct"]                   # ... and dg_moe_grouped
    assert launch(_call(struct_bytes=ctypes.sizeof(_lib.Moe) + 8, x=None)) == E["struct"]   # struct before the pointers
    assert launch(_call(stage=2)) == E["layout"]
    for f in ("x", "w", "qinfo", "lut", "y", "ids", "gates", "group_ws", "f32_ws"):
        assert launch(_call(**{f: None})) == E["null"], f
    assert launch(_call(stage=0, gates=None, f32_ws=None, f32_ws_bytes=0, residual=None, dtype=7)) == E["dtype"]   # GATE_UP needs neither
    assert launch(_call(lut=None, qtype=0, dtype=7)) == E["dtype"]          # int4 needs no LUT; null before dtype
    assert launch(_call(group_ws=None, dtype=7)) == E["null"]
    assert launch(_call(dtype=2)) == E["dtype"]
    for q in (3, 4, -1):
        assert launch(_call(qtype=q)) == E["qtype"], q
    assert launch(_call(dtype=2, qtype=3)) == E["dtype"]
    for bad in (dict(m=0), dict(E=0), dict(E=65), dict(top_k=0), dict(top_k=9, E=16), dict(top_k=3, E=2), dict(k=96), dict(k=0), dict(wrows=24),
                dict(wrows=0)):
        assert launch(_call(**bad)) == E["shape"], bad
        assert launch(_call(**bad, inner_k_tiles=2, group=32, group_ws_bytes=0)) == E["shape"], bad   # shape before size, innerKTiles, group
    assert launch(_call(m=32769, group_ws_bytes=1 << 30, f32_ws_bytes=1 << 40)) == E["size"]         # P = 65538 pairs
    assert launch(_call(m=32768, group_ws_bytes=_gws(65536, 4), f32_ws_bytes=4 * 65536 * 64, inner_k_tiles=2)) == E["inner"]
    assert launch(_call(m=1 << 40)) == E["size"]
    assert launch(_call(group_ws_bytes=_gws(4, 4) - 4)) == E["size"]
    assert launch(_call(f32_ws_bytes=4 * 4 * 64 - 4)) == E["size"]
    assert launch(_call(stage=0, f32_ws_bytes=0, inner_k_tiles=2)) == E["inner"]                      # GATE_UP: no f32 workspace needed
    assert launch(_call(group_ws_bytes=0, inner_k_tiles=2, group=32)) == E["size"]                   # size before innerKTiles and group
    assert launch(_call(inner_k_tiles=2)) == E["inner"]
    assert launch(_call(inner_k_tiles=8, group=32)) == E["inner"]
    for g in (32, 16, 512, 96):
        assert launch(_call(group=g)) == E["group"], g
    assert launch(_call(group=256, k=128)) == E["group"]
    assert launch(_call(group=32, x=("off", 8))) == E["group"]              # group before alignment
    for f in ("x", "w", "qinfo", "lut", "y", "residual", "f32_ws"):
        assert launch(_call(**{f: ("off", 8)})) == E["align"], f
    for f in ("ids", "gates", "group_ws"):
        assert launch(_call(**{f: ("off", 2)})) == E["align"], f
    for f in ("stride_w", "stride_qinfo", "stride_lut"):
        assert launch(_call(**{f: 24})) == E["align"], f
    # the plan: no workspace is looked at
    out = (ctypes.c_int64 * 8)()
    assert L.dg_moe_plan(ctypes.byref(_call(group=32)), -1, out) == E["group"]
    assert L.dg_moe_plan(ctypes.byref(_call()), -1, None) == E["null"]
    assert L.dg_moe_plan(ctypes.byref(_call(group_ws=None, f32_ws=None, group_ws_bytes=0, f32_ws_bytes=0)), -1, out) == 0
    assert tuple(out)[5:] == (_gws(4, 4), 4 * 4 * 64, 0)
    # dg_moe_group
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 63) & ~63
    bm = out[0]
    group = lambda ids=p, ws=p, nbytes=_gws(4, 4), m=2, t=2, E_=4, b=bm: L.dg_moe_group(ids, ws, nbytes, m, t, E_, b, 0, None)
    assert group(ids=None) == E["null"] and group(ws=None) == E["null"]
    for kw in (dict(m=0), dict(E_=0), dict(E_=65), dict(t=0), dict(t=9, E_=16), dict(t=3, E_=2), dict(b=bm + 1), dict(b=0)):
        assert group(**kw) == E["shape"], kw
        assert group(**kw, ids=None) == E["null"], kw
    assert group(m=32769, nbytes=1 << 30) == E["size"] and group(nbytes=_gws(4, 4) - 1) == E["size"]
    assert group(nbytes=0, ids=p + 2) == E["size"]                          # size before alignment
    assert group(ids=p + 2) == E["align"] and group(ws=p + 2) == E["align"]


# ---------------------------------------------------------------------------------------------------------------------------------
# defaults: nothing changes
# ---------------------------------------------------------------------------------------------------------------------------------

def test_defaults_leave_the_launch_sequence(oracle, monkeypatch):
    from any4_amd import decode_ops as G
    from any4_amd.decode import DecodeConfig
    from any4_amd.moe import MoEMLP

    assert DecodeConfig().moe_grouped_from == 0 and DecodeConfig.mixtral_8x7b().moe_grouped_from == 0
    W = _weights(oracle, 4, 64, 128, 64, "any4_rowwise", BF16)[0]
    rw = R.router_inputs(1, 128, 4, BF16, 1)[1]
    calls = []
    for name in ("moe_route", "moe_gate_up", "moe_down", "moe_group", "moe_gate_up_grouped", "moe_down_grouped", "moe_grouped_plan"):
        def fake(*a, _n=name, **k):
            calls.append(_n)
            return (torch.zeros(1), torch.zeros(1)) if _n == "moe_route" else (128, 64, 1, 1, 1, 4096, 4096) if _n == "moe_grouped_plan" else torch.zeros(1)
        monkeypatch.setattr(G, name, fake)
    x = torch.zeros(40, 128, dtype=BF16)
    block = MoEMLP(rw, W, 2)
    assert block.grouped_from is None
    block(x)
    assert calls == ["moe_route", "moe_gate_up", "moe_down"] and not block._grouped
    calls.clear()
    block = MoEMLP(rw, W, 2, grouped_from=16)
    block(x[:15])
    assert calls == ["moe_route", "moe_gate_up", "moe_down"] and not block._grouped
    with pytest.raises(ValueError):
        MoEMLP(rw, W, 2, grouped_from=0)
