"""Mixture of experts without a GPU: the definition (any4_amd/moe.py: moe_ref) against an independent per-token loop, ties, gates, the C
ABI (symbols, the one struct's mirror, every refusal of the GEMV kernel before a launch, the fields a call does not read), the configuration and the plain-torch layer.  Run: pytest -m "not gpu"."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import moe_ref as R

BF16, F16 = torch.bfloat16, torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weights(oracle, E, il, hidden, g, qtype, dtype, seed=0):
    from any4_amd.moe import MoEWeights

    gu, gu_raw = R.make_stack(oracle, E, 2 * il, hidden, g, qtype, dtype, seed)
    dn, dn_raw = R.make_stack(oracle, E, hidden, il, g, qtype, dtype, seed + 1)
    return MoEWeights(gu, dn), gu_raw, dn_raw


def _loop_ref(x16, rw16, gu_raw, dn_raw, g, top_k, res16):
    """Token by token, expert by expert, float64 numpy from codes / scales / zeros / LUT: (y64 [m][hidden], ids, gates)."""
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
            gu = (R.weights64(gu_raw[e], g) @ x[i]).reshape(-1, 2, 8)
            gate, up = r16(gu[:, 0].reshape(-1)), r16(gu[:, 1].reshape(-1))
            a = r16(r16(gate / (1 + np.exp(-gate))) * up)
            y += gt * (R.weights64(dn_raw[e], g) @ a)
        out.append(y + (0 if res16 is None else res16[i].double().numpy()))
        ids_all.append(ids)
        gates_all.append(gates)
    return np.stack(out), np.array(ids_all), np.stack(gates_all)


@pytest.mark.parametrize("E,top_k,qtype,dtype,res", [(4, 2, "any4_rowwise", BF16, True), (1, 1, "int4", BF16, False), (5, 1, "any4_global", F16, True),
                                                      (3, 3, "any4_rowwise", F16, False)])
def test_moe_ref_against_a_per_token_loop(oracle, E, top_k, qtype, dtype, res):
    from any4_amd.moe import moe_ref

    hidden, il, g, m = 128, 64, 64, 5
    W, gu_raw, dn_raw = _weights(oracle, E, il, hidden, g, qtype, dtype)
    x, rw = R.router_inputs(m, hidden, E, dtype, seed=3)
    r = R.make_inputs(m, hidden, hidden, dtype, 4)[2] if res else None
    y, ids, gates, _ = moe_ref(x, rw, W, top_k, r, parts=True)
    y64, ids2, gates2 = _loop_ref(x, rw, gu_raw, dn_raw, g, top_k, r)
    assert np.array_equal(ids.numpy(), ids2)
    assert np.abs(gates.numpy() - gates2).max() < 1e-12
    # the two float64 sums differ in order only: the 16-bit result is the rounding of either, up to a hair at a rounding boundary
    err = np.abs(y.double().numpy() - y64)
    assert (err <= R.contract(y64, 0 * y64, dtype)).all(), err.max()


def test_ties_go_to_the_lower_index_and_gates_sum_to_one():
    from any4_amd.moe import route_ref

    x, rw = R.router_inputs(8, 256, 6, BF16, seed=1)
    rw[4] = rw[1]                                   # experts 1 and 4 tie on every row
    for logits in ((x.double() @ rw.double().t()), (x.float() @ rw.float().t())):
        ids, gates = route_ref(logits, 3)
        for row in ids.tolist():
            if 4 in row:
                assert 1 in row and row.index(1) < row.index(4), row
        assert any(4 in row or 1 in row for row in ids.tolist())
        assert (gates.double().sum(dim=1) - 1).abs().max() <= 2.0 ** -22
    ids64, gates64, *_ = R.route_ref64(x, rw, 3)
    assert np.array_equal(ids64, route_ref(x.double() @ rw.double().t(), 3)[0].numpy())
    assert np.abs(gates64.sum(axis=1) - 1).max() <= 2.0 ** -22


def test_symbols_are_declared_exported_and_bound():
    from any4_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "decode_glue_hip.h")).read()
    lib = _lib.load()
    for name in ("dg_moe_route", "dg_moe_launch", "dg_moe_plan"):
        assert re.search(r"TG_API\s+int\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes == _lib.SYMBOLS[name]
    for name in ("dg_moe_w4_launch", "dg_moe_w4_plan", "dg_moe_grouped_launch", "dg_moe_grouped_plan"):   # ABI 9's four: removed, not kept as shims
        assert name not in hdr and name not in _lib.SYMBOLS and not hasattr(lib, name), name
    assert lib.tg_abi_version() == _lib.TG_ABI_VERSION == 10
    names = ("DG_MOE_GATE_UP", "DG_MOE_DOWN", "DG_MOE_GEMV", "DG_MOE_GROUPED")
    assert tuple(getattr(_lib, n) for n in names) == tuple(int(re.search(rf"#define {n} (\d+)", hdr).group(1)) for n in names) == (0, 1, 0, 1)


def test_struct_mirror_is_the_headers():
    """The one struct of both kernels, field for field."""
    from any4_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "decode_glue_hip.h")).read()
    assert len(re.findall(r"typedef struct dg_moe\w*", hdr)) == 1 and not hasattr(_lib, "MoeW4") and not hasattr(_lib, "MoeGrouped")
    body = re.search(r"typedef struct dg_moe \{(.*?)\} dg_moe;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, name = re.match(r"(.*?)(\w+)$", decl).groups()
        ctype = ctype.replace("const", "").strip()
        fields.append((name, ctypes.c_void_p if ctype.endswith("*") else {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}[ctype]))
    assert [(n, t) for n, t in _lib.Moe._fields_] == fields
    assert ctypes.sizeof(_lib.Moe) == sum(ctypes.sizeof(t) for _, t in fields) == 184      # no hidden padding
    assert [f[0] for f in fields[:2]] == ["struct_bytes", "kernel"] and _lib.Moe().struct_bytes == 184
    sizes = [ctypes.sizeof(t) for _, t in fields[2:]]
    assert sizes == sorted(sizes, reverse=True)                      # pointers and 64-bit fields in front of the 32-bit ones


def _call(**over):
    from any4_amd import _lib

    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 63) & ~63
    kw = dict(kernel=_lib.DG_MOE_GEMV, stage=_lib.DG_MOE_DOWN, x=p, w=p, qinfo=p, lut=p, y=p, ids=p, gates=p, residual=p, stride_w=16, stride_qinfo=16, stride_lut=16, m=2,
              wrows=64, k=128, E=4, top_k=2, group=64, qtype=2, dtype=_lib.TG_BF16, inner_k_tiles=4)
    kw.update({k: (p + v[1] if isinstance(v, tuple) else v) for k, v in over.items()})
    c = _lib.Moe(**kw)
    c._keep = buf
    return c


def test_every_refusal_comes_before_a_launch():
    """Dummy pointers: a call that got as far as a launch would fault or fail on a machine without a GPU; each answers its own code."""
    from any4_amd import _lib

    L = _lib.load()
    E = dict(null=-1, inner=-2, kdiv=-3, group=-4, dtype=-5, qtype=-6, shape=-7, align=-8, size=-10, layout=-12, struct=-14)
    launch = lambda c: L.dg_moe_launch(ctypes.byref(c), 0, None)
    assert L.dg_moe_launch(None, 0, None) == E["null"]
    for n in (136, 144, 176):                                               # ABI 9's two structs among them
        assert launch(_call(struct_bytes=n)) == E["struct"], n
    assert launch(_call(struct_bytes=152, x=None)) == E["struct"]          # struct before the pointers
    assert launch(_call(struct_bytes=152, kernel=2)) == E["struct"]        # ... and before the kernel
    assert launch(_call(stage=2)) == E["layout"]
    for kern in (2, -1):
        assert launch(_call(kernel=kern)) == E["layout"], kern
        assert launch(_call(kernel=kern, x=None)) == E["layout"], kern      # the kernel before the pointers
    assert launch(_call(stage=2, x=None)) == E["layout"]
    for f in ("x", "w", "qinfo", "lut", "y", "ids", "gates"):
        assert launch(_call(**{f: None})) == E["null"], f
    assert launch(_call(lut=None, qtype=0, dtype=7)) == E["dtype"]          # int4 needs no LUT; null before dtype
    assert launch(_call(x=None, dtype=7)) == E["null"]
    assert launch(_call(dtype=2)) == E["dtype"]
    for q in (3, 4, -1):                                                    # mx4, int8
        assert launch(_call(qtype=q)) == E["qtype"], q
    assert launch(_call(dtype=2, qtype=3)) == E["dtype"]                    # dtype before qtype
    for bad in (dict(m=0), dict(E=0), dict(E=65), dict(top_k=0), dict(top_k=9, E=16), dict(top_k=3, E=2), dict(k=96), dict(k=0), dict(wrows=24),
                dict(wrows=0)):
        assert launch(_call(**bad)) == E["shape"], bad
        assert launch(_call(**bad, inner_k_tiles=2, group=32)) == E["shape"], bad   # shape before innerKTiles and group
    assert launch(_call(inner_k_tiles=2)) == E["inner"]
    assert launch(_call(inner_k_tiles=8, group=32)) == E["inner"]
    for g in (32, 16, 512, 96):
        assert launch(_call(group=g)) == E["group"], g
    assert launch(_call(group=256, k=128)) == E["group"]                    # does not divide k
    assert launch(_call(group=32, x=("off", 8))) == E["group"]              # group before alignment
    for f in ("x", "w", "qinfo", "lut", "y", "residual"):
        assert launch(_call(**{f: ("off", 8)})) == E["align"], f
    for f in ("ids", "gates"):
        assert launch(_call(**{f: ("off", 2)})) == E["align"], f
    for f in ("stride_w", "stride_qinfo", "stride_lut"):
        assert launch(_call(**{f: 24})) == E["align"], f
    assert launch(_call(k=65536, wrows=16)) == E["size"]                    # one activation row no longer fits the staging
    out = (ctypes.c_int64 * 8)()
    assert L.dg_moe_plan(ctypes.byref(_call(group=32)), -1, out) == E["group"]
    assert L.dg_moe_plan(ctypes.byref(_call()), -1, None) == E["null"]
    assert L.dg_moe_plan(ctypes.byref(_call(kernel=2)), -1, out) == E["layout"]
    assert L.dg_moe_plan(ctypes.byref(_call(k=65536, wrows=16)), -1, out) == E["size"]
    # the router
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63
    route = lambda x=p, w=p, i=p, g=p, m=1, k=64, E_=8, t=2, dt=0: L.dg_moe_route(x, w, i, g, m, k, E_, t, dt, 0, None)
    for kw in (dict(x=None), dict(w=None), dict(i=None), dict(g=None)):
        assert route(**kw) == E["null"], kw
    assert route(dt=3) == E["dtype"] and route(x=None, dt=3) == E["null"]
    for kw in (dict(m=0), dict(E_=0), dict(E_=65), dict(t=0), dict(t=9, E_=16), dict(t=3, E_=2), dict(k=0)):
        assert route(**kw) == E["shape"], kw
    assert route(k=68) == E["kdiv"]
    assert route(x=p + 8) == E["align"] and route(w=p + 8) == E["align"] and route(i=p + 2) == E["align"] and route(g=p + 2) == E["align"]


def test_fields_the_call_does_not_use_are_not_read():
    """A GEMV call answers what it answers without workspaces whatever group_ws / f32_ws and their sizes hold, and a grouped GATE_UP call
    whatever f32_ws holds.  Every call ends in an error code: the group that no kernel has, or a device index that no machine has."""
    from any4_amd import _lib

    L = _lib.load()
    no_device = 1 << 20
    garbage = [dict(group_ws=None, f32_ws=None), dict(group_ws=("off", 2), f32_ws=("off", 2)), dict(group_ws=("off", 8), f32_ws=("off", 8)),
               dict(group_ws_bytes=-1, f32_ws_bytes=-1), dict(group_ws=("off", 2), f32_ws=None, group_ws_bytes=-1, f32_ws_bytes=-1)]
    for stage in (_lib.DG_MOE_GATE_UP, _lib.DG_MOE_DOWN):
        for ws in [{}] + garbage:
            assert L.dg_moe_launch(ctypes.byref(_call(stage=stage, group=32, **ws)), 0, None) == -4, (stage, ws)       # TG_E_GROUP
            assert L.dg_moe_launch(ctypes.byref(_call(stage=stage, **ws)), no_device, None) == -9, (stage, ws)         # TG_E_DEVICE
    grouped = dict(kernel=_lib.DG_MOE_GROUPED, stage=_lib.DG_MOE_GATE_UP, group_ws=("off", 0), group_ws_bytes=1 << 20)
    for ws in (dict(f32_ws=None), dict(f32_ws=("off", 2)), dict(f32_ws=("off", 8)), dict(f32_ws_bytes=-1), dict(f32_ws=("off", 2), f32_ws_bytes=-1)):
        assert L.dg_moe_launch(ctypes.byref(_call(**grouped, group=32, **ws)), 0, None) == -4, ws
        assert L.dg_moe_launch(ctypes.byref(_call(**grouped, **ws)), no_device, None) == -9, ws
    assert L.dg_moe_launch(ctypes.byref(_call(**{**grouped, "group_ws": ("off", 2)})), no_device, None) == -8          # (its own workspace is read)
    # GATE_UP has neither gates nor a residual
    for kern in ({}, grouped):
        for f in ("gates", "residual"):
            assert L.dg_moe_launch(ctypes.byref(_call(**{"stage": _lib.DG_MOE_GATE_UP, **kern, f: ("off", 2)})), no_device, None) == -9, (kern, f)
    # the planner fills eight int64: four for the GEMV, seven for the grouped kernel, zeros behind them
    out = (ctypes.c_int64 * 8)(*[-1] * 8)
    assert L.dg_moe_plan(ctypes.byref(_call()), -1, out) == 0 and all(v > 0 for v in out[:4]) and list(out[4:]) == [0] * 4
    out = (ctypes.c_int64 * 8)(*[-1] * 8)
    assert L.dg_moe_plan(ctypes.byref(_call(kernel=_lib.DG_MOE_GROUPED, group_ws=None, f32_ws=None)), -1, out) == 0
    assert all(v > 0 for v in out[:7]) and out[7] == 0


def test_planner_regimes():
    """The shapes tests/test_gpu_moe.py uses reach every regime of the decomposition (planned for 256 compute units)."""
    from tests.test_gpu_moe import GEMV_SHAPES

    R.assert_regimes_reached(GEMV_SHAPES)
    assert R.plan(0, 28672, 4096, 1, 2) == (256, 7, 8, 8)                  # Mixtral gate_up: 1792 units over 256 workgroups
    assert R.plan(1, 4096, 14336, 8, 2)[:3] == (256, 1, 3)                 # Mixtral down: the staged rows of k = 14336 leave three pairs per sweep
    assert R.plan(1, 16 * 5000, 64, 8, 2)[1] == 16                         # never more than 16 units per workgroup


def test_config():
    from any4_amd.decode import DecodeConfig

    c = DecodeConfig()
    assert (c.experts, c.experts_per_token) == (0, 2)
    assert c.linear_shapes() == [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
    assert c.weight_bytes_4bit() == 3756261376                               # the dense Llama-3-8B figure, as before
    assert DecodeConfig.llama2_7b().weight_bytes_4bit() == 3488104448
    mx = DecodeConfig.mixtral_8x7b()
    assert (mx.hidden, mx.inter, mx.layers, mx.heads, mx.kv_heads, mx.head_dim, mx.vocab, mx.rope_theta, mx.experts, mx.experts_per_token,
            mx.gate_up_interleave) == (4096, 14336, 32, 32, 8, 128, 32000, 1e6, 8, 2, 8)
    one = lambda n, k: n * k // 2 + (k // 128) * n * 4 + 32 * n + k * 2 + n * 2
    want = 32 * (one(6144, 4096) + one(4096, 4096) + 2 * (one(28672, 4096) + one(4096, 14336)) + 8 * 4096 * 2)
    assert mx.weight_bytes_4bit() == want


def _tiny(**kw):
    from any4_amd.decode import DecodeConfig

    return DecodeConfig(**{**dict(hidden=128, inter=64, layers=2, heads=4, kv_heads=2, head_dim=32, vocab=64, max_seq=32, group_size=64,
                                  gate_up_interleave=8, experts=4, experts_per_token=2), **kw})


def test_construction_refusals():
    from any4_amd.decode import DecodeLayer, DecodeStack, DenseFactory
    from any4_amd.lora import AdapterSet

    cfg = _tiny()
    fac = DenseFactory(cfg, "cpu", BF16)
    with pytest.raises(ValueError, match="not built yet"):
        DecodeLayer(cfg, 0, fac, 0, 2, "cpu", BF16, 1)
    for targets in (("gate_up",), ("qkv", "down")):
        with pytest.raises(ValueError, match="not built yet"):
            DecodeStack(cfg, fac, "cpu", BF16, fused=False, adapters=AdapterSet(cfg, 2, 8, "cpu", BF16, targets=targets))
    DecodeStack(cfg, fac, "cpu", BF16, fused=False, adapters=AdapterSet(cfg, 2, 8, "cpu", BF16, targets=("qkv", "o")))   # keeps working
    with pytest.raises(ValueError, match="gate_up_interleave"):
        DecodeStack(_tiny(gate_up_interleave=0), fac, "cpu", BF16, fused=False)


def test_plain_torch_layer_against_the_definition():
    """DenseFactory experts on the CPU: the all-experts-and-mask formulation against moe_ref, and a decode step runs."""
    from any4_amd.decode import DecodeStack, DenseFactory
    from any4_amd.moe import moe_ref

    cfg = _tiny()
    stack = DecodeStack(cfg, DenseFactory(cfg, "cpu", BF16, seed=2), "cpu", BF16, bs=2, fused=False)
    layer = stack.layers[1]
    assert layer.gate_up is None and layer.down is None and layer.moe.router.shape == (4, 128) and layer.launches() == 8
    x, r = R.make_inputs(6, 128, 128, BF16, 9)[::2]
    layer.moe.record = []
    y = layer.moe(x, residual=r, fused=False)
    ref, ids, gates, logits = moe_ref(x, layer.moe.router, layer.moe.weights, 2, r, parts=True)
    A = R.SLACK * (x.double().abs() @ layer.moe.router.double().abs().t()).numpy()
    assert R.margin_ok(logits.numpy(), A, 2)[0].all()                        # (seeded: no row is near a tie)
    assert len(layer.moe.record) == 1 and np.abs(layer.moe.record[0][0].double().numpy() - logits.numpy()).max() <= A.max()
    # The torch path rounds gate, up, their product and every expert's down output to 16 bit (2^-8 relative each, the gate's through
    # silu' <= 1.1): at most 2^-8 (1.1 + 1 + 1 + 1) < 2^-5 of S = sum_s g_s |a_s| . |W2|, plus the final rounding.
    W = layer.moe.weights
    S = np.zeros(ref.shape)
    for i in range(x.shape[0]):
        for s in range(2):
            e = int(ids[i, s])
            gu = (W.gate_up.weights64(e) @ x[i].double()).view(-1, 2, 8)
            a = torch.nn.functional.silu(gu[:, 0].reshape(-1)) * gu[:, 1].reshape(-1)
            S[i] += float(gates[i, s]) * (W.down.weights64(e).abs() @ a.abs()).numpy()
    err = (y.double() - ref.double()).abs().numpy()
    assert (err <= 2.0 ** -5 * S + 2 * R.contract(ref.double().numpy(), 0, BF16)).all(), (err / (2.0 ** -5 * S)).max()
    with pytest.raises(RuntimeError, match="4-bit experts"):
        layer.moe(x)
    assert stack.decode(torch.tensor([1, 2]), 0).shape == (2, 64)
