"""What the C ABI answers over a grid of calls, as a digest (developer tool; needs no GPU: the planner and all validation run before any HIP call):
    python dev/plan_sweep.py [--lib PATH/libtinygemm_hip.so] [--quick]     the planner: workspace bytes and kernel family of every case
    python dev/plan_sweep.py --errors [N] [--seed S] [--lib ...] [--abi8 | --abi9]
                                                                           return codes of N broken structs per GEMM entry point, then of
                                                                           N // 25 broken calls of dg_decode_attn, of each of the
                                                                           nineteen accepted calls of dg_attn_launch, of each (kernel,
                                                                           stage) of dg_moe_launch, of dg_moe_plan, dg_moe_route and
                                                                           dg_moe_group
Prints the number of cases, a histogram of the answers and a sha256 over their sequence.  Two builds route / validate alike when they
print the same digest for the same script; run it before and after a change of the host launch path (or with --lib on an older build).
No digest is recorded anywhere: a performance change may move the routing on purpose.
"""
import argparse
import collections
import ctypes
import hashlib
import itertools
import os
import random
import sys
from array import array

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from any4_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=L.LIB_PATH)
ap.add_argument("--quick", action="store_true", help="a 1/96 sub-grid of the planner sweep")
ap.add_argument("--errors", nargs="?", type=int, const=100000, default=0, metavar="N")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--abi8", action="store_true", help="--errors: --lib is a build up to ABI 8; make the attention calls through its positional entry points")
ap.add_argument("--abi9", action="store_true", help="--errors: --lib is a build of ABI 9; make the mixture-of-experts calls through its dg_moe_w4_* / dg_moe_grouped_* entry points")
opt = ap.parse_args()
lib = ctypes.CDLL(opt.lib)
P = ctypes.POINTER(L.W4Gemm)
for name in ("tg_gemm_w4", "tg_gemm_w4_dx", "tg_gemm_w8"):
    getattr(lib, name).argtypes = [P, ctypes.c_int, ctypes.c_void_p]
    getattr(lib, name + "_workspace_bytes").argtypes = [P]
    getattr(lib, name + "_workspace_bytes").restype = ctypes.c_int64
lib.tg_gemm_w4_plan.argtypes = [P, ctypes.c_int]

BASE = 1 << 20          # dummy pointers, 64-byte aligned: nothing is launched, so nothing reads them
NO_DEVICE = 1 << 20     # a device index no machine has: a launch entry point with a valid struct answers TG_E_DEVICE instead of launching


def report(title, answers):
    """answers: array('q') of everything recorded, in order"""
    hist = collections.Counter(answers[1::2]) if title.startswith("planner") else collections.Counter(answers)
    print(f"{title}: {len(answers) // 2 if title.startswith('planner') else len(answers)} cases")
    shown = sorted(hist.items())[:24]
    print("  answers: " + ", ".join(f"{k}: {v}" for k, v in shown) + (f", ... ({len(hist)} different)" if len(hist) > len(shown) else ""))
    print("  sha256 " + hashlib.sha256(answers.tobytes()).hexdigest())


def valid(**kw):
    a = L.W4Gemm(x=BASE, w=2 * BASE, qinfo=3 * BASE, lut=4 * BASE, y=5 * BASE, m=1, wrows=4096, k=4096, group=128, qtype=0, dtype=0,
                 w_on_right=1, inner_k_tiles=4, batch=1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def planner():
    """(workspace bytes, plan) of tg_gemm_w4 over the main grid, then the smaller legs: fused stages, dx, w8"""
    a = valid(stride_x=16, stride_w=16, stride_qinfo=16, stride_lut=16, stride_y=16)
    ref = ctypes.byref(a)
    wsb, plan = lib.tg_gemm_w4_workspace_bytes, lib.tg_gemm_w4_plan
    out = array("q")
    ms = (1, 2, 4, 5, 8, 9, 16, 17, 33, 64, 65, 512)
    rows = (16, 4096, 4104, 14336, 28672, 32832)
    ks = (64, 512, 4096, 8192, 14336)
    if opt.quick:
        ms, rows, ks = ms[::4], rows[::4], ks[::2] + (14336,)

    def pair():
        a.workspace, a.workspace_bytes = None, 0
        need = wsb(ref)
        out.append(need)
        out.append(plan(ref, -1))
        if need > 0:  # ... and with the workspace it asked for
            a.workspace, a.workspace_bytes = 6 * BASE, need
        out.append(need)
        out.append(plan(ref, -1))

    inner = list(itertools.product((1, 16, 64), range(4), (0, 1), (0, 1)))
    for a.m, a.wrows, a.k, a.group, a.qtype, a.dtype, a.w_on_right, a.inner_k_tiles in itertools.product(
            ms, rows, ks, (32, 64, 128, 256), range(4), (0, 1), (1, 0), (1, 2, 4, 8)):
        for a.batch, a.numerics, a.w_format, frag in inner:
            a.x_layout = a.y_layout = frag
            pair()
    report("planner, tg_gemm_w4", out)

    # fused stages on the same entry point: norm_weight / SwiGLU / a bias with a row stride
    out = array("q")
    a = valid()
    ref = ctypes.byref(a)
    for a.m, a.wrows, a.k, a.group, a.qtype, a.w_on_right, a.inner_k_tiles, a.batch, a.numerics in itertools.product(
            (1, 4, 8, 16, 17, 64), (4096, 4104, 14336, 28672), (512, 4096, 8192), (32, 64, 128), range(4), (1, 0), (2, 4), (1, 16), range(4)):
        for norm, a.epilogue, bias in itertools.product((0, 1), (0, 1), (0, 1, 2)):
            a.norm_weight = 7 * BASE if norm else None
            a.bias, a.bias_row_stride = (8 * BASE if bias else None), (a.wrows if bias == 2 else 0)
            pair()
    report("planner, tg_gemm_w4 with fused stages", out)

    # the other two entry points report workspace bytes only
    out = array("q")
    a = valid()
    ref = ctypes.byref(a)
    for a.m, a.wrows, a.k, a.group, a.dtype, a.w_on_right, a.inner_k_tiles in itertools.product(
            (1, 16, 17, 33, 64, 65, 512, 4096), rows, ks, (32, 64, 128, 256), (0, 1), (1, 0), (1, 2, 4, 8)):
        for a.qtype, a.w_format in itertools.product(range(4), (0, 1)):
            out.append(lib.tg_gemm_w4_dx_workspace_bytes(ref))
        a.qtype, a.w_format = L.TG_Q_INT8, 0
        for a.batch in (1, 16):
            out.append(lib.tg_gemm_w8_workspace_bytes(ref))
        a.batch = 1
    report("workspace bytes, tg_gemm_w4_dx / tg_gemm_w8", out)


# ---- error codes: start from a valid struct, break one, two or three fields ----
_PTR = (None, BASE + 4, BASE + 8, BASE)
_SIZE = (0, -1, 1 << 31, (1 << 31) - 1, 1 << 20, 17, 4104, 96, 4096)
_STRIDE = (0, 16, 8, 4, 2)
_FULL, _PREFIX = ctypes.sizeof(L.W4Gemm), L.W4Gemm.stride_y.offset + 8
BREAKS = {
    "x": _PTR, "w": _PTR, "qinfo": _PTR + (BASE + 2,), "lut": _PTR, "y": _PTR + (BASE + 2,), "bias": _PTR, "norm_weight": _PTR, "workspace": _PTR,
    "m": _SIZE, "wrows": _SIZE, "k": _SIZE,
    "group": (0, 16, 32, 64, 128, 256, 512, 48, -32), "qtype": (-1, 0, 1, 2, 3, 4, 5), "dtype": (-1, 0, 1, 2), "w_on_right": (0, 1, 2),
    "inner_k_tiles": (-1, 0, 1, 2, 3, 4, 8, 16), "batch": (-1, 0, 1, 2, 16),
    "stride_x": _STRIDE, "stride_w": _STRIDE, "stride_qinfo": _STRIDE, "stride_lut": _STRIDE, "stride_y": _STRIDE, "stride_bias": _STRIDE,
    "numerics": (-1, 0, 1, 2, 3, 4), "reserved": (0, 1), "reserved6": (0, 1), "workspace_bytes": (-1, 0, 1 << 20),
    "x_layout": (0, 1, 2), "y_layout": (0, 1, 2), "bias_row_stride": (-4, 0, 2, 4, 4096), "epilogue": (0, 1, 2), "w_format": (0, 1, 2),
    "struct_bytes": (0, _PREFIX - 8, _PREFIX, _FULL - 8, _FULL, _FULL + 8), "struct_reserved": (0, 1),
}


def errors(n):
    names = sorted(BREAKS)
    entries = [("tg_gemm_w4", lambda r: lib.tg_gemm_w4(r, NO_DEVICE, None), 0),
               ("tg_gemm_w4_plan", lambda r: lib.tg_gemm_w4_plan(r, -1), 0),
               ("tg_gemm_w4_workspace_bytes", lib.tg_gemm_w4_workspace_bytes, 0),
               ("tg_gemm_w4_dx", lambda r: lib.tg_gemm_w4_dx(r, NO_DEVICE, None), 0),
               ("tg_gemm_w4_dx_workspace_bytes", lib.tg_gemm_w4_dx_workspace_bytes, 0),
               ("tg_gemm_w8", lambda r: lib.tg_gemm_w8(r, NO_DEVICE, None), L.TG_Q_INT8),
               ("tg_gemm_w8_workspace_bytes", lib.tg_gemm_w8_workspace_bytes, L.TG_Q_INT8)]
    for e, (name, fn, qtype) in enumerate(entries):
        rng = random.Random(1000 * opt.seed + e)
        out = array("q")
        for _ in range(n):
            a = valid(qtype=qtype, m=rng.choice((1, 8, 16, 64)), inner_k_tiles=rng.choice((2, 4)))
            for f in rng.sample(names, rng.choice((1, 2, 3))):
                setattr(a, f, rng.choice(BREAKS[f]))
            out.append(fn(ctypes.byref(a)))
        report(name, out)


# ---- the attention calls of include/decode_glue_hip.h: start from a valid call, break none, one or two fields ----
# Every call names NO_DEVICE, so one that passes validation answers TG_E_DEVICE from DeviceScope (tg_common.cuh: hipGetDevice fails, or
# hipSetDevice of an index no machine has) in front of everything that touches the GPU.  Any other non-negative answer ends the sweep.
_I31 = (1 << 31) - 1
ATTN_BREAKS = {
    "dtype": (-1, 0, 1, 2),
    "bs": (0, -1, 1, 2, 3, 65535, 65536, _I31 // 8, _I31 // 8 + 1),           # prefill: grid.y; the others: bs * hl (hl = 8) an int32
    "T": (0, -1, 1, 16, _I31 // 4, _I31 // 4 + 1),                            # bs * T <= INT32_MAX / 2 at bs = 2
    "cache_bs": (0, -1, 2, 3, _I31, _I31 + 1),
    "hl": (0, -1, 1, 6, 7, 8), "kvl": (0, -1, 1, 2, 3, 8),
    "d": (0, 4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 136, 256, 264),
    "max_seq": (0, -1, 1, 4096, 8192, 8193, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 25) - 1, 1 << 25),  # ... * d * 2 < 2^32 at d = 128 / 64
    "nsplit": (0, -1, 1, 4, 64, 65),
    "scratch_bytes": (0, -1, -4, 16),                                          # relative to what the (broken) sizes need
    "page_size": (0, -64, 32, 48, 64, 96, 128, 4096, 8192), "num_pages": (0, -1, 1, 5, _I31, _I31 + 1),
}


def attn_valid(names):
    v = dict(bs=2, T=16, cache_bs=2, hl=8, kvl=2, d=128, max_seq=4096, scale=0.125, nsplit=4, dtype=0, device=NO_DEVICE, stream=None, scratch_bytes=0,
             page_size=64, num_pages=5)
    v.update((name, (i + 1) * BASE) for i, name in enumerate(n for n in names if n not in v))  # the pointers
    return v


DECODE_ATTN = ("qkv", "k_cache", "v_cache", "pos", "out", "bs", "hl", "kvl", "d", "max_seq", "scale", "dtype", "device", "stream")
INT64 = ("scratch_bytes", "bs", "T", "cache_bs", "max_seq", "page_size", "num_pages")


def draw_order(kernel, flags):
    """The argument order this call had as a positional entry point up to ABI 8.  The sweep hands out pointers and draws what to break in
    this order, so its digests are those recorded for that ABI (profiles/attn_call_refactor_checks.txt), and --abi8 can still make the call."""
    prefill, split, seq, mx8, paged = kernel == L.DG_ATTN_PREFILL, kernel == L.DG_ATTN_SPLIT, flags & L.DG_ATTN_SEQ, flags & L.DG_ATTN_MX8, flags & L.DG_ATTN_PAGED
    return (["qkv", "cos", "sin", "pos"] + (["len", "slot"] if prefill and seq else []) + (["table"] if paged else []) + ["k_cache", "v_cache"]
            + (["k_exp", "v_exp"] if mx8 else []) + ["out"] + (["scratch", "scratch_bytes"] if split else []) + ["bs"] + (["T"] if prefill else [])
            + (["cache_bs"] if prefill and seq else []) + ["hl", "kvl", "d", "max_seq"] + (["page_size", "num_pages"] if paged else []) + ["scale"]
            + (["nsplit"] if split else []) + ["dtype", "device", "stream"])


def attn_errors(n):
    """dg_decode_attn, then the nineteen accepted calls of dg_attn_launch: first the twelve that were swept as positional entry points (base
    by base, scalar / per sequence, 16-bit / mx8), then the paged, the one-barrier mx8 and the paged mx8 ones.  --abi8: the same argument
    lists through the positional symbols of a build up to ABI 8 (--lib), which is how two such builds are compared."""
    twelve = [(k, (L.DG_ATTN_SEQ if seq else 0) | (L.DG_ATTN_MX8 if mx8 else 0))
              for k, has_mx8 in ((L.DG_ATTN_GENERAL, False), (L.DG_ATTN_ONLINE, False), (L.DG_ATTN_SPLIT, True), (L.DG_ATTN_PREFILL, True))
              for seq in (False, True) for mx8 in ((False, True) if has_mx8 else (False,))]
    pairs = twelve + [p for p in L.ATTN_FLAVOURS if p[1] & L.DG_ATTN_PAGED and not p[1] & L.DG_ATTN_MX8] + \
        [p for p in L.ATTN_FLAVOURS if p[1] & L.DG_ATTN_ONE_BARRIER and not p[1] & L.DG_ATTN_PAGED] + \
        [p for p in L.ATTN_FLAVOURS if p[1] & L.DG_ATTN_PAGED and p[1] & L.DG_ATTN_MX8]
    assert len(pairs) == len(set(pairs)) == 19
    if not opt.abi8:
        lib.dg_attn_launch.argtypes = [ctypes.POINTER(L.Attn), ctypes.c_int, ctypes.c_void_p]
    for e, pair in enumerate([None] + pairs):
        entry = "dg_decode_attn" if pair is None else L.ATTN_FLAVOURS[pair]
        names = list(DECODE_ATTN) if pair is None else draw_order(*pair)
        if pair is None or opt.abi8:
            fn = getattr(lib, entry)
            fn.argtypes = [ctypes.c_int64 if a in INT64 else ctypes.c_float if a == "scale" else ctypes.c_int if a in ATTN_BREAKS or a == "device"
                           else ctypes.c_void_p for a in names]
        pointers = [name for name in attn_valid(names) if name not in ATTN_BREAKS and name not in ("scale", "device", "stream")]
        fields = sorted(set(names) & set(ATTN_BREAKS)) + pointers
        rng = random.Random(1000 * opt.seed + 100 + e)
        out = array("q")
        for _ in range(n):
            v = attn_valid(names)
            slack = 0
            for f in rng.sample(fields, rng.choice((0, 1, 2))):
                if f == "scratch_bytes":
                    slack = rng.choice(ATTN_BREAKS[f])
                else:
                    v[f] = rng.choice(ATTN_BREAKS[f]) if f in ATTN_BREAKS else rng.choice((None, v[f] + 4, v[f] + 8, v[f]))
            heads = v["bs"] * v["hl"]
            v["scratch_bytes"] = max(-(1 << 62), min(1 << 62, (heads * 4 + 15) // 16 * 16 + heads * v["nsplit"] * (v["d"] + 2) * 4 + slack))
            if pair is None or opt.abi8:
                rc = fn(*[v[name] for name in names])
            else:
                call = L.Attn(kernel=pair[0], flags=pair[1], **{name: v[name] for name in names if name not in ("device", "stream")})
                rc = lib.dg_attn_launch(ctypes.byref(call), v["device"], v["stream"])
            if rc >= 0:
                sys.exit(f"{entry}: answer {rc} to {v}: a call of this sweep got past DeviceScope")
            out.append(rc)
        report(entry, out)


# ---- the mixture-of-experts calls: start from a valid call, break none, one or two fields ----
# The fields in the order of ABI 9's two structs (dg_moe_w4; dg_moe_grouped = that plus the workspaces), which is the order the sweep
# draws in, so that --abi9 makes the same cases through that build's two structs.
_MOE_PTRS = ("x", "w", "qinfo", "lut", "y", "ids", "gates", "residual")
_MOE_I64 = ("stride_w", "stride_qinfo", "stride_lut", "m", "wrows", "k")
_MOE_I32 = ("E", "top_k", "group", "qtype", "dtype", "inner_k_tiles")


def _abi9_struct(grouped):
    ptrs, i64 = (_MOE_PTRS + ("group_ws", "f32_ws"), _MOE_I64 + ("group_ws_bytes", "f32_ws_bytes")) if grouped else (_MOE_PTRS, _MOE_I64)

    class Abi9Moe(ctypes.Structure):
        _fields_ = ([("struct_bytes", ctypes.c_uint32), ("stage", ctypes.c_int32)] + [(f, ctypes.c_void_p) for f in ptrs] +
                    [(f, ctypes.c_int64) for f in i64] + [(f, ctypes.c_int32) for f in _MOE_I32])
    return Abi9Moe


_STRIDE16 = (0, 16, 8, 24, 32)
MOE_BREAKS = {
    "m": (0, -1, 1, 8, 9, 19, 32768, 32769, 65536, 65537, 1 << 30, 1 << 31), "wrows": (0, 16, 24, 64, 4096, 1 << 24, (1 << 24) + 16),
    "k": (0, 64, 96, 128, 192, 4096, 65536, 1 << 20), "E": (0, 1, 2, 4, 64, 65), "top_k": (0, 1, 2, 3, 8, 9),
    "group": (0, 32, 64, 128, 256, 512, 96), "qtype": (-1, 0, 1, 2, 3, 4, 5), "dtype": (-1, 0, 1, 2), "inner_k_tiles": (0, 2, 4, 8),
    "stride_w": _STRIDE16, "stride_qinfo": _STRIDE16, "stride_lut": _STRIDE16,
    "struct_bytes": (None, -8, 0, 8),            # nothing, or relative to the size of the struct the build has
    "group_ws_bytes": (0, -1, -4, 4096), "f32_ws_bytes": (0, -1, -4, 4096),   # relative to what the (broken) sizes need
}


def moe_fields(grouped, stage):
    """The fields of a (kernel, stage) call in ABI 9's order, and those of them the call has: GATE_UP has neither gates nor a residual,
    and its grouped flavour no f32 workspace (ABI 9 checked the alignment of such a pointer all the same; ABI 10 does not read it)."""
    ptrs, i64 = (_MOE_PTRS + ("group_ws", "f32_ws"), _MOE_I64 + ("group_ws_bytes", "f32_ws_bytes")) if grouped else (_MOE_PTRS, _MOE_I64)
    order = ("struct_bytes",) + ptrs + i64 + _MOE_I32
    absent = () if stage == L.DG_MOE_DOWN else ("gates", "residual", "f32_ws", "f32_ws_bytes")
    return order, [f for f in order if f not in absent]


def moe_draw(rng, grouped, stage, plan):
    """One call's fields by name; a broken pointer is NULL or 2, 4 or 8 bytes off"""
    order, has = moe_fields(grouped, stage)
    v = dict(m=2, wrows=64, k=128, E=4, top_k=2, group=64, qtype=2, dtype=0, inner_k_tiles=4, stride_w=16, stride_qinfo=16, stride_lut=16)
    v.update((name, (i + 1) * BASE) for i, name in enumerate(f for f in order if f not in v and not f.endswith("_bytes")))
    slack = dict(group_ws_bytes=0, f32_ws_bytes=0)
    struct_bytes = 0
    for f in rng.sample(has, rng.choice((0, 1, 2))):
        if f == "struct_bytes":
            struct_bytes = rng.choice(MOE_BREAKS[f])
        elif f in slack:
            slack[f] = rng.choice(MOE_BREAKS[f])
        else:
            v[f] = rng.choice(MOE_BREAKS[f]) if f in MOE_BREAKS else rng.choice((None, v[f] + 2, v[f] + 4, v[f] + 8, v[f]))
    if grouped:
        clamp = lambda b: max(-(1 << 62), min(1 << 62, b))
        pairs = v["m"] * v["top_k"]
        v["group_ws_bytes"] = clamp(4 * (136 + 2 * pairs + 3 * (-(-pairs // 128) + min(v["E"], pairs))) + slack["group_ws_bytes"])
        v["f32_ws_bytes"] = clamp(4 * pairs * v["wrows"] + slack["f32_ws_bytes"])
    if stage != L.DG_MOE_DOWN:
        v["gates"] = v["residual"] = None
        if grouped:
            v["f32_ws"], v["f32_ws_bytes"] = None, 0
    if plan and grouped:
        v["group_ws"] = v["f32_ws"] = None   # (the planner looks at neither)
    return v, struct_bytes


def moe_struct(grouped, stage, v, struct_bytes):
    cls = _abi9_struct(grouped) if opt.abi9 else L.Moe
    kw = dict(v, stage=stage) if opt.abi9 else dict(v, stage=stage, kernel=L.DG_MOE_GROUPED if grouped else L.DG_MOE_GEMV)
    return cls(struct_bytes=0 if struct_bytes is None else ctypes.sizeof(cls) + struct_bytes, **kw)


def moe_errors(n):
    """dg_moe_launch per (kernel, stage), dg_moe_plan over all four, dg_moe_route, dg_moe_group.  --abi9: the same cases through
    dg_moe_w4_launch / dg_moe_grouped_launch and their planners of a build of ABI 9 (--lib)."""
    def entry(grouped, what):
        name = (("dg_moe_grouped_" if grouped else "dg_moe_w4_") if opt.abi9 else "dg_moe_") + what
        fn = getattr(lib, name)
        fn.argtypes = None   # (the struct's class differs from case to case under --abi9: passed by reference)
        return fn

    e = 0
    for grouped in (False, True):
        for stage in (L.DG_MOE_GATE_UP, L.DG_MOE_DOWN):
            rng = random.Random(1000 * opt.seed + 200 + e)
            e += 1
            out = array("q")
            fn = entry(grouped, "launch")
            for _ in range(n):
                call = moe_struct(grouped, stage, *moe_draw(rng, grouped, stage, False))
                rc = fn(ctypes.byref(call), ctypes.c_int(NO_DEVICE), ctypes.c_void_p(None))
                if rc >= 0:
                    sys.exit(f"dg_moe_launch: answer {rc}: a call of this sweep got past DeviceScope")
                out.append(rc)
            report(f"dg_moe_launch {'DG_MOE_GROUPED' if grouped else 'DG_MOE_GEMV'} {'DG_MOE_DOWN' if stage else 'DG_MOE_GATE_UP'}", out)
    # the planner: the code, and behind a 0 the plan (four values of the GEMV, seven of the grouped kernel)
    rng = random.Random(1000 * opt.seed + 210)
    out = array("q")
    for _ in range(n):
        grouped, stage = rng.choice((False, True)), rng.choice((L.DG_MOE_GATE_UP, L.DG_MOE_DOWN))
        call = moe_struct(grouped, stage, *moe_draw(rng, grouped, stage, True))
        plan = ((ctypes.c_int64 * 7) if grouped else (ctypes.c_int32 * 4))() if opt.abi9 else (ctypes.c_int64 * 8)()
        rc = entry(grouped, "plan")(ctypes.byref(call), ctypes.c_int(-1), plan)
        out.append(rc)
        if rc == 0:
            out.extend(plan[:7 if grouped else 4])
            if any(plan[7 if grouped else 4:]):
                sys.exit(f"dg_moe_plan: {list(plan)}: not zero behind the plan")
    report("dg_moe_plan", out)
    # the two positional entry points, alike in both ABIs
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    lib.dg_moe_route.argtypes = [vp] * 4 + [i64] * 4 + [ctypes.c_int, ctypes.c_int, vp]
    lib.dg_moe_group.argtypes = [vp, vp] + [i64] * 5 + [ctypes.c_int, vp]
    ptr = lambda rng, p: rng.choice((None, p + 2, p + 4, p + 8, p))
    route = dict(m=(0, -1, 1, 19, 1 << 31, (1 << 31) - 1), k=(0, 4, 8, 64, 68, 4096, 1 << 20, (1 << 20) + 8), E=MOE_BREAKS["E"], top_k=MOE_BREAKS["top_k"],
                 dtype=MOE_BREAKS["dtype"])
    rng = random.Random(1000 * opt.seed + 211)
    out = array("q")
    for _ in range(n):
        v = dict(x=BASE, router_w=2 * BASE, ids=3 * BASE, gates=4 * BASE, m=2, k=128, E=4, top_k=2, dtype=0)
        for f in rng.sample(list(v), rng.choice((0, 1, 2))):
            v[f] = rng.choice(route[f]) if f in route else ptr(rng, v[f])
        out.append(lib.dg_moe_route(*v.values(), NO_DEVICE, None))
    report("dg_moe_route", out)
    rng = random.Random(1000 * opt.seed + 212)
    out = array("q")
    for _ in range(n):
        v = dict(ids=BASE, group_ws=2 * BASE, group_ws_bytes=0, m=2, top_k=2, E=4, bm=128)
        slack = 0
        for f in rng.sample(list(v), rng.choice((0, 1, 2))):
            if f == "group_ws_bytes":
                slack = rng.choice(MOE_BREAKS[f])
            else:
                v[f] = rng.choice(MOE_BREAKS[f]) if f in MOE_BREAKS else rng.choice((0, 64, 127, 128, 256)) if f == "bm" else ptr(rng, v[f])
        pairs, bm = v["m"] * v["top_k"], max(1, v["bm"])
        v["group_ws_bytes"] = 4 * (136 + 2 * pairs + 3 * (-(-pairs // bm) + min(v["E"], pairs))) + slack
        out.append(lib.dg_moe_group(*v.values(), NO_DEVICE, None))
    report("dg_moe_group", out)
    if min(out) >= 0:
        sys.exit("dg_moe_group: a call of this sweep got past DeviceScope")


if opt.errors:
    errors(opt.errors)
    attn_errors(max(1, opt.errors // 25))
    moe_errors(max(1, opt.errors // 25))
else:
    planner()
