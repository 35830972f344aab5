"""The persistent pair-table family (w4_gemm_pair_kernel, w4_pair_m1_lean_kernel, the two 16x16x32 layouts; any4_amd/csrc/w4_gemm_pair.cuh,
tg_pair.hip) for its tests: the host plan restated, batches of DIFFERENT problems, float64 references, the bound, exact probes and a
plain-torch twin of the schedule with mutants.  A helper module (not a conftest), in the style of tests/tile_ref.py and tests/moe_ref.py;
tests/test_pair_ref_cpu.py checks it on the CPU, tests/test_gpu_pair_f64.py runs the kernels against it.

pair_plan       launch_pair, pair_groups, pair_lds_plan, pair_lean_call, launch_pair_m and launch_pair_la as plain Python, for STACKED calls
                (batch >= 2: w4_gemv_kernel and w4_gemm_pair16_loop_kernel, which sit in front of this family, take one problem per call
                only) of up to 16 activation rows.  The one family in front that takes stacked calls, w4_gemm_xr_kernel, is restated as far
                as "takes the call" (xr_takes).  Constants come from the sources' defaults (constants()).
references      per problem of a batch: y64 = x . (lut[code] scale + zero) in float64, the weights not rounded, and S = sum |x w| on the
                oracle's 16-bit weights RNE16(fma(lut[code], scale, zero)).  tests/test_pair_ref_cpu.py pins both to the oracle.
bound           the project's GEMM contract (assert_fast_close): |y - y64| <= 0.5 ulp16(y64) (1 + 2^-7) + 4e-6 S.  Nothing
                here is fitted to a kernel's output.
probes          inputs for which every f32 intermediate is exact, with the expected output: one weight per row, the zero point of one
                group per row, one-hot activation rows.
twin            the schedule in plain torch: the item walk of every workgroup with the register ring, the table and the staged activations as
                explicit state (which problem and row block each operand of an item comes from), then per wave its k-slice, per group an
                f32 sum taken as a running difference, y += scale d + zero sum(x) with the zero term once per row, the lane halves added,
                the eight wave partials added in wave order, one RNE rounding.  MUTANTS are the bugs it can be given.
"""
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import torch

BF16, F16 = torch.bfloat16, torch.float16
QT = {"int4": 0, "any4_global": 1, "any4_rowwise": 2, "mx4": 3}
NUMERICS = {"fast": 0, "reference": 1, "fast_mfma": 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "any4_amd", "csrc")
WAVES = 8
MX4_VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


@functools.lru_cache(maxsize=1)
def constants():
    """The tuning constants the plan depends on, read from the defaults in the sources (#ifndef NAME / #define NAME value), and the LDS
    line of two workgroups per CU (`lds > 80u * 1024u` in tg_pair.hip)."""
    c = {}
    for name in ("tg_common.cuh", "tg_xr.hip"):
        text = open(os.path.join(CSRC, name)).read()
        for key, val in re.findall(r"#ifndef (TG_\w+)\s*\n\s*#define \1 (\d+)\b", text):
            c[key] = int(val)
    lines = set(re.findall(r"lds > (\d+)u \* 1024u", open(os.path.join(CSRC, "tg_pair.hip")).read()))
    assert len(lines) == 1, lines
    c["LDS_LINE"] = int(lines.pop()) * 1024
    for key in ("TG_PAIR_WGS", "TG_PAIR_MIN_ITEMS", "TG_XG_CHUNK", "TG_B16_CHUNK", "TG_PAIR_R", "TG_PAIR_RA", "TG_PAIR_RA1", "TG_PAIR_RB16", "TG_PAIR_MR1",
                "TG_PAIR_NSG2", "TG_PAIR_NSG2_M1", "TG_PAIR_MR1_GPS", "TG_PAIR_M1_LEAN", "TG_M1_DEFAULT_MFMA", "TG_XR_MIN_M", "TG_XR_MIN_ITEMS_PER_WG"):
        assert key in c, f"{key}: no default found in the sources"
    return SimpleNamespace(**c)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------------------

def xr_takes(C, m, wrows, k, g, qtype, inner, dtype, batch, numerics, workspace, norm, epilogue):
    """launch_pair_xr (tg_xr.hip) for a stacked row-major call: (taken, workspace bytes)."""
    qmx = qtype == "mx4"
    if inner != 4 or norm or epilogue or wrows % 64:
        return False, 0

    def one(nch, pk, window=False):
        if qmx and (nch != 16 or dtype != BF16):
            return False
        if m > (8 if pk else 16) or m < (1 if numerics == "fast_mfma" else C.TG_XR_MIN_M):
            return False
        cpg = min(g // 32, nch)
        if (cpg != 1) if qmx else (cpg not in (1, 2, 4, 8)):
            return False
        if qmx and (k // g) % 16:
            return False
        if nch > 24 and cpg == 2 and not pk:
            return False
        if cpg == 8 and nch % 8:
            return False
        items = wrows // 64 * batch
        if items < C.TG_XR_MIN_ITEMS_PER_WG * 256:
            return False
        ngroups = 256 * nch // g if window else k // g
        return (32768 if qmx else 2 * 65536 + ngroups * 64) <= 160 * 1024

    def windows(nchs):
        if qmx or any((256 * n) % g for n in nchs) or not 9 <= m <= 16 or not workspace:
            return False, 0
        if not all(one(n, False, True) for n in nchs):
            return False, 0
        return True, len(nchs) * batch * m * wrows * 4

    if k == 4096:
        return one(16, False), 0
    if k == 8192 and m <= 8 and not qmx:
        return one(32, True), 0
    if k == 8192 and m >= 9:
        if not qmx:
            ok, ws = windows((16, 16))
            if ok:
                return ok, ws
        return one(32, False), 0
    if k == 14336 and not qmx:
        if m == 8:
            return one(56, True), 0
        if m >= 9:
            return windows((16, 16, 24))
    return False, 0


def _slices(ksuper, spw, ring):
    nl = [max(min(spw, ksuper - w * spw), 0) for w in range(WAVES)]
    return nl, [max(-(-n // ring), 1) for n in nl], [n % ring != 0 for n in nl]


def _lds_plan(C, pp, inner, qmx, ngroups, x_bytes, alias, alias_if_large):
    pp.lds_x = 0 if qmx else 65536
    pp.lds_xs = (pp.lds_x + x_bytes + 32 * inner + 15) & ~15
    pp.lds_red = (pp.lds_xs + (0 if qmx else ngroups * pp.xs_rows * 4) + 15) & ~15
    lds = pp.lds_red + 8 * 2 * pp.rused * pp.red_lanes * 4
    pp.red_alias = bool(alias or (alias_if_large and lds > C.LDS_LINE))
    if pp.red_alias:
        lds, pp.lds_red = pp.lds_red, 0
    return lds


def _groups(k, g, inner):
    gps, nsg = (1, g // (16 * inner)) if g >= 16 * inner else ((16 * inner) // g, 1)
    ksuper = k // (16 * inner)
    return gps, nsg, ksuper, -(-(ksuper // nsg) // 8) * nsg


def _mx4_blocks_fit(ngroups, spw, gps):
    return not (ngroups < 16 or ngroups % 4 or ((spw * gps) % 4 and spw * gps > 12))


def _workspace(batch, xrows, k, ngroups, xs_rows):
    return batch * (xrows * k * 2 + ((ngroups * xs_rows * 4 + 15) & ~15))


def _pair_b(C, m, wrows, k, g, qtype, inner, batch, numerics, workspace, bias, norm, epilogue):
    """launch_pair<DT, I, QMX>: the plan, or None where the path answers TG_PAIR_NA."""
    qmx = qtype == "mx4"
    R = C.TG_PAIR_R
    gps, nsg, ksuper, spw = _groups(k, g, inner)
    ngroups = k // g
    mregs = 4 if m <= 8 else 16
    ma = 2 * mregs
    mrows = min(m, ma)
    pp = SimpleNamespace(spw=spw, gps=gps, nsg=nsg, ksuper=ksuper, rused=mrows if mrows < 4 else mregs, xs_rows=4 if mrows <= 4 else ma,
                         red_lanes=32 if mrows <= 4 else 64, la=0, inner=inner, qmx=qmx)
    lds = _lds_plan(C, pp, inner, qmx, ngroups, mrows * (k * 2 + 16), not qmx and mrows > 4, False)
    if qmx and not _mx4_blocks_fit(ngroups, spw, gps):
        return None
    if norm and (qmx or lds > C.LDS_LINE or m > ma):
        return None
    need = 0
    if lds > C.LDS_LINE:
        if mregs != 4 or m > ma:
            return None
        xw_bytes = (16 if inner == 2 else 8) * (32 * inner + 16)
        lds = _lds_plan(C, pp, inner, qmx, ngroups, 8 * xw_bytes, pp.red_alias, True)
        if (qmx and pp.red_alias) or lds > C.LDS_LINE:
            return None
        need = _workspace(batch, m, k, ngroups, pp.xs_rows)
        if not workspace:
            return None
    xg = need != 0
    pp.lds, pp.xg, pp.ws = lds, xg, need
    pp.rblocks, pp.rw = -(-wrows // 64), 64
    pp.items = pp.rblocks * -(-m // ma) * batch
    if pp.items > 2 ** 31 - 1 or pp.items < C.TG_PAIR_MIN_ITEMS:
        return None
    pp.chunk = C.TG_XG_CHUNK if xg and pp.items >= C.TG_PAIR_WGS * C.TG_XG_CHUNK * 4 else 1
    lean_ok = (C.TG_PAIR_M1_LEAN and C.TG_PAIR_MR1 == 1 and R == 2 and m == 1 and not xg and not norm and not bias and not epilogue and
               wrows % 64 == 0 and not pp.red_alias and spw % 2 == 0 and ksuper % 2 == 0 and numerics != "fast_mfma")

    def pair_m(GPS, NSG):
        m1 = m == 1 and C.TG_PAIR_MR1 == 1 and (qmx or GPS <= C.TG_PAIR_MR1_GPS)
        if mregs != 4:
            return None
        if inner == 8 and (qmx or not m1 or norm):
            return None
        if norm and (qmx or GPS > 1):
            return None
        return ("m1" if m1 else "general"), GPS, NSG

    def pick():
        if gps == 1:
            fixed = bool(C.TG_PAIR_NSG2 and (C.TG_PAIR_NSG2_M1 or not (m == 1 and C.TG_PAIR_MR1 == 1)))
            if inner == 4 and not qmx:
                if numerics == "fast_mfma" and m == 1 and not xg and not norm and fixed and nsg == R:
                    return "m1_mfma", 1, R
                if fixed and nsg == R and lean_ok:
                    return "lean", 1, R
            if fixed and nsg == R:
                return pair_m(1, R)
            if not qmx and fixed and m == 1 and C.TG_PAIR_MR1 == 1 and not norm and nsg in (1, 4):
                if nsg == 1:
                    return "m1", 1, 1
                if inner <= 4:
                    return "m1", 1, 4
            return pair_m(1, 0)
        if inner >= 4 and gps == 2:
            return pair_m(2, 0)
        if inner >= 8 and gps == 4:
            return pair_m(4, 0)
        return None

    got = pick()
    if got is None:
        return None
    pp.kernel, pp.GPS, pp.NSG = got
    mr1 = pp.kernel in ("m1", "m1_mfma", "lean")
    pp.ring = R if qmx else 4 if (mr1 and pp.NSG == 4) else 1 if pp.GPS > 1 else R
    # DOT (w4_gemm_pair.cuh): the m = 1 kernels that contract per lane, both lane halves of a row accumulating
    pp.dot = pp.kernel == "lean" or (pp.kernel == "m1" and (qmx or pp.NSG > 0))
    return pp


def _pair_la(C, la, m, wrows, k, g, qtype, inner, batch, workspace, norm, epilogue):
    """launch_pair_la<DT, I, QMX, LA>: LA = 1 Aint4 weights, LA = 2 Bint4 weights with 9 ... 16 activation rows."""
    qmx = qtype == "mx4"
    if inner not in ((1, 2, 4) if la == 1 else (2, 4)) or (la == 1 and inner < 2):
        return None
    if m > 16 or norm or epilogue:
        return None
    ring0 = C.TG_PAIR_RB16 if la == 2 else C.TG_PAIR_R
    gps, nsg, ksuper, spw = _groups(k, g, inner)
    ngroups = k // g
    if qmx and not _mx4_blocks_fit(ngroups, spw, gps):
        return None
    pp = SimpleNamespace(spw=spw, gps=gps, nsg=nsg, ksuper=ksuper, rused=m if m < 4 else 4, xs_rows=4 if m <= 4 else 8 if m <= 8 else 16,
                         red_lanes=32 if m <= 8 else 64, la=la, inner=inner, qmx=qmx, xg=True, dot=False)
    pp.lds = _lds_plan(C, pp, inner, qmx, ngroups, 0, False, True)
    if pp.lds > C.LDS_LINE:
        return None
    pp.rblocks, pp.rw = -(-wrows // 32), 32
    pp.items = pp.rblocks * batch
    if pp.items > 2 ** 31 - 1 or pp.items < (2 if la == 2 else 1) * C.TG_PAIR_MIN_ITEMS:
        return None
    pp.ws = _workspace(batch, m + 1, k, ngroups, pp.xs_rows)
    if not workspace:
        return None
    pp.chunk = C.TG_B16_CHUNK if la == 2 and pp.items >= C.TG_PAIR_WGS * C.TG_B16_CHUNK * 4 else 1
    if gps == 1:
        pp.GPS, pp.NSG = 1, (1 if C.TG_PAIR_NSG2 and nsg == 1 else ring0 if C.TG_PAIR_NSG2 and nsg == ring0 else 0)
    elif inner >= 4 and gps == 2:
        pp.GPS, pp.NSG = 2, 0
    else:
        return None
    pp.kernel = f"la{la}"
    pp.ring = C.TG_PAIR_R if qmx and la == 0 else (C.TG_PAIR_RA1 if pp.GPS > 1 else C.TG_PAIR_RA if la == 1 else C.TG_PAIR_RB16)
    return pp


def pair_plan(m, wrows, k, g, qtype, inner=4, on_right=True, batch=2, dtype=BF16, numerics="fast", workspace=True, bias=False, norm=False,
              epilogue=False):
    """What a stacked tg_gemm_w4 call (row-major operands, batch >= 2, m <= 16) runs.  .family: 'pair' (this family), 'xr' (w4_gemm_xr_kernel)
    or 'other' (this family declined: w4_gemm_pair16_kernel or a reference-numerics kernel).  For 'pair': .kernel in lean / m1 / m1_mfma /
    general / la1 / la2 with the template's GPS, NSG, ring and xg; spw, nl / rounds / partial per wave; red_alias; rblocks, items,
    workgroups, chunk; wg_items(wg) = the items of a workgroup in the order it takes them; .ws = the workspace bytes."""
    C = constants()
    assert batch >= 2 and 1 <= m <= 16, "pair_plan restates stacked calls of up to 16 activation rows"
    qmx = qtype == "mx4"
    other = SimpleNamespace(family="other", kernel=None, ws=0)
    if (numerics == "reference" and not qmx) or (qmx and dtype != BF16):
        return other
    if on_right:
        num = "fast_mfma" if (C.TG_M1_DEFAULT_MFMA and numerics == "fast" and m == 1 and not qmx) else numerics
        took, ws = xr_takes(C, m, wrows, k, g, qtype, inner, dtype, batch, num, workspace, norm, epilogue)
        if took:
            return SimpleNamespace(family="xr", kernel=None, ws=ws)
        pp = _pair_b(C, m, wrows, k, g, qtype, inner, batch, num, workspace, bias, norm, epilogue) if inner in (2, 4, 8) else None
        if pp is None and m > 8:
            pp = _pair_la(C, 2, m, wrows, k, g, qtype, inner, batch, workspace, norm, epilogue)
    else:
        pp = _pair_la(C, 1, m, wrows, k, g, qtype, inner, batch, workspace, norm, epilogue)
    if pp is None:
        return other
    pp.family = "pair"
    pp.m, pp.wrows, pp.k, pp.g, pp.batch = m, wrows, k, g, batch
    pp.nl, pp.rounds, pp.partial = _slices(pp.ksuper, pp.spw, pp.ring)
    pp.workgroups = min(pp.items, C.TG_PAIR_WGS)
    pp.wg_items = functools.partial(wg_items, pp)
    return pp


def wg_items(pp, wg):
    """The items workgroup `wg` takes, in its order: a contiguous range (pair_walk_range) where the workgroup stages the activations, the
    chunked round-robin dealing of the workspace variants (XG, LA) otherwise."""
    if not pp.xg:
        return list(range(wg * pp.items // pp.workgroups, (wg + 1) * pp.items // pp.workgroups))
    out, it, cpos, stride = [], wg * pp.chunk, 0, pp.workgroups * pp.chunk - (pp.chunk - 1)
    while it < pp.items:
        out.append(it)
        big = cpos + 1 >= pp.chunk
        it, cpos = it + (stride if big else 1), (0 if big else cpos + 1)
    return out


def kernel_class(pp):
    """The instantiation class of a planned call: kernel, NSG, GPS, workspace activations, mx4, innerKTiles (4 unless named)."""
    return (f"{pp.kernel}:NSG{pp.NSG}:GPS{pp.GPS}" + (":xg" if pp.xg and not pp.la else "") + (":mx4" if pp.qmx else "") +
            (f":I{pp.inner}" if pp.inner != 4 else ""))


def regimes(pp):
    """The names of the regimes a planned call reaches (assert_regimes_reached)."""
    cls = kernel_class(pp)
    r = {f"kernel:{pp.kernel}", cls}
    live = [n for n in pp.nl if n]
    r.add("slice:full" if all(n == pp.spw for n in pp.nl) else "")
    r.add("slice:partial+empty" if live[-1] < pp.spw and len(live) < WAVES else "")
    r.add("slice:one wave" if len(live) == 1 else "")
    r.add("slice:empty waves" if len(live) < WAVES else "")
    r.add(f"round:partial:{'ring4' if pp.ring == 4 else pp.kernel}" if any(p and n for p, n in zip(pp.partial, pp.nl)) else "")
    r.add("round:one" if max(pp.rounds) == 1 else "round:many" if max(pp.rounds) >= 6 else "")
    r.add(f"round:many:{pp.kernel}{':xg' if pp.xg and not pp.la else ''}{':mx4' if pp.qmx else ''}" if max(pp.rounds) >= 6 else "")
    r.add("red_alias" if pp.red_alias else "")
    r.add("items<workgroups" if pp.items < constants().TG_PAIR_WGS else "")
    per = sorted({len(wg_items(pp, w)) for w in (0, 1, pp.workgroups // 2, pp.workgroups - 1)})
    r.add("range:1-2" if per[0] >= 1 and per[-1] <= 2 and pp.items >= constants().TG_PAIR_WGS else "")
    r.add("range:5-6" if per[0] >= 5 and per[-1] <= 6 else "")
    r.add("range:16+" if per[0] >= 16 else "")
    r.add(f"rblocks:{pp.rblocks}")
    r.add("wrows%64" if pp.wrows % 64 and pp.kernel != "lean" else "")
    r.add("chunked" if pp.chunk > 1 else "")
    r.add("chunked:partial visit" if pp.chunk > 1 and pp.items % pp.chunk else "")
    r.add("empty waves+several items" if len(live) < WAVES and per[0] >= 2 else "")
    # per kernel class: a steady state of three or more items in every workgroup over problems of several row blocks (ranges start and end
    # inside a problem), and a partial slice with empty waves behind it
    r.add(f"walk:{cls}" if per[0] >= 3 and pp.rblocks > 1 else "")
    r.add(f"slice:partial+empty:{cls}" if live[-1] < pp.spw and len(live) < WAVES else "")
    return r - {""}


# What the GPU file's cases, taken together, must reach.  Not in the list because no call reaches them: four groups per super-tile
# (innerKTiles 8 at g = 32: launch_pair_m declines everything but the m = 1 kernel at one group per super-tile, see DECLINED), and a partial
# last round on the ring of four or on the general template with NSG = R -- a wave's slice is a whole number of groups, so with a group of
# R super-tiles nl is a multiple of R.  A partial round exists where a group is one super-tile (NSG 1 on the m = 1 kernel and on the Aint4
# layout, NSG 0 on the general template) and for mx4, whose slices are cut in super-tiles.
WALK_CLASSES = ["lean:NSG2:GPS1", "m1:NSG1:GPS1", "m1:NSG2:GPS1", "m1:NSG4:GPS1", "m1:NSG2:GPS1:I2", "m1:NSG1:GPS1:I8", "m1_mfma:NSG2:GPS1",
                "general:NSG0:GPS1", "general:NSG2:GPS1", "general:NSG0:GPS2", "general:NSG2:GPS1:I2", "m1:NSG0:GPS2:mx4", "general:NSG0:GPS2:mx4",
                "m1:NSG2:GPS1:xg", "general:NSG2:GPS1:xg", "la1:NSG2:GPS1", "la1:NSG1:GPS1:I2", "la1:NSG0:GPS2:mx4", "la2:NSG2:GPS1", "la2:NSG2:GPS1:I2"]
# (the workspace variant of the m = 1 kernel starts at 53 units: from 49 units on a launch has no empty wave, so its partial slice has none behind it)
PARTIAL_CLASSES = [c for c in WALK_CLASSES if c != "m1:NSG2:GPS1:xg"]
REQUIRED = ({"kernel:lean", "kernel:m1", "kernel:general", "kernel:m1_mfma", "kernel:la1", "kernel:la2", "m1:NSG2:GPS1:I8", "m1:NSG1:GPS1:I2",
             "red_alias", "slice:full", "slice:partial+empty", "slice:one wave", "round:partial:general", "round:partial:m1", "round:partial:la1",
             "round:one", "round:many", "items<workgroups", "range:1-2", "range:5-6", "range:16+", "rblocks:1", "rblocks:3", "rblocks:5",
             "wrows%64", "chunked", "chunked:partial visit", "empty waves+several items",
             # many rounds per wave (k = 14336 where the class takes it; the staged kernels end where the workspace variant begins: lean at 6144)
             "round:many:lean", "round:many:m1", "round:many:m1:xg", "round:many:general:xg", "round:many:m1:mx4", "round:many:la1", "round:many:la2"}
            | set(WALK_CLASSES) | {f"walk:{c}" for c in WALK_CLASSES} | {f"slice:partial+empty:{c}" for c in PARTIAL_CLASSES})


def assert_regimes_reached(plans):
    seen = set()
    for pp in plans:
        assert pp.family == "pair", pp
        seen |= regimes(pp)
    missing = REQUIRED - seen
    assert not missing, f"regimes not reached: {sorted(missing)}"
    return seen


# ---------------------------------------------------------------------------------------------------------------------------------
# batches of different problems
# ---------------------------------------------------------------------------------------------------------------------------------

def make_batch(m, n, k, g, qtype, batch, dtype=BF16, seed=0, inner=4, on_right=True):
    """`batch` different problems (CPU): codes uint8 [B][n][k], x [B][m][k], scale / zero [B][k / g][n] and the LUT ([B][16], [B][n][16] or
    None), or for mx4 exps uint8 [B][n][k / g].  n is the call's wrows (a multiple of the packed tile's rows)."""
    assert n % (8 if on_right else 16) == 0
    gen = torch.Generator().manual_seed(1000003 * seed + 7 * n + k + 31 * batch + QT[qtype] + 13 * m)
    bt = SimpleNamespace(m=m, n=n, k=k, g=g, qtype=qtype, B=batch, dtype=dtype, inner=inner, on_right=on_right, bias=None, x_pad=0)
    # (eight codes per random 64-bit word: the draw of half a billion codes is a third of a large case's host time otherwise)
    bt.codes = (torch.randint(-2 ** 63, 2 ** 63 - 1, (batch * n * k // 8,), dtype=torch.int64, generator=gen).view(torch.uint8) & 15).view(batch, n, k)
    bt.x = torch.randn(batch, m, k, generator=gen).to(dtype)
    bt.lut = bt.exps = bt.scale = bt.zero = None
    if qtype == "mx4":
        bt.exps = torch.randint(120, 131, (batch, n, k // g), dtype=torch.uint8, generator=gen)
    else:
        bt.scale = (torch.rand(batch, k // g, n, generator=gen) * 0.02 + 0.005).to(dtype)
        bt.zero = (torch.randn(batch, k // g, n, generator=gen) * 0.01).to(dtype)
        if qtype == "any4_global":
            bt.lut = torch.randn(batch, 16, generator=gen).to(dtype)
        elif qtype == "any4_rowwise":
            bt.lut = torch.randn(batch, n, 16, generator=gen).to(dtype)
    return bt


def sub_batch(bt, lo, hi):
    """The problems [lo, hi) of a batch as a batch."""
    sb = SimpleNamespace(**vars(bt))
    sb.B = hi - lo
    for f in ("codes", "x", "scale", "zero", "lut", "exps", "bias"):
        if getattr(bt, f) is not None:
            setattr(sb, f, getattr(bt, f)[lo:hi])
    return sb


def plan_of(bt, numerics="fast", workspace=True, **kw):
    return pair_plan(bt.m, bt.n, bt.k, bt.g, bt.qtype, bt.inner, bt.on_right, bt.B, bt.dtype, numerics, workspace, bias=bt.bias is not None, **kw)


def table64(bt, lo, hi):
    """[hi - lo][n][16] float64: the 16 values a code selects, per row."""
    nb = hi - lo
    if bt.qtype == "int4":
        t = torch.arange(-8, 8, dtype=torch.float64)
    elif bt.qtype == "mx4":
        t = torch.tensor(MX4_VALUES + [-v for v in MX4_VALUES], dtype=torch.float64)
    elif bt.qtype == "any4_global":
        return bt.lut[lo:hi].double()[:, None, :].expand(nb, bt.n, 16)
    else:
        return bt.lut[lo:hi].double()
    return t.expand(nb, bt.n, 16)


def scale_zero64(bt, lo, hi):
    """([nb][n][k / g] scale, zero) float64; mx4: 2^(e - 127), e = 0 -> 2^-127, e = 255 -> NaN; zero 0."""
    if bt.qtype == "mx4":
        e = bt.exps[lo:hi].double()
        s = torch.exp2(e - 127)
        s = torch.where(e == 255, torch.full_like(s, float("nan")), s)
        return s, torch.zeros_like(s)
    return bt.scale[lo:hi].double().transpose(1, 2), bt.zero[lo:hi].double().transpose(1, 2)


def weights64(bt, lo, hi):
    """[nb][n][k] float64: lut[code] scale + zero, not rounded."""
    v = torch.gather(table64(bt, lo, hi), 2, bt.codes[lo:hi].long())
    s, z = scale_zero64(bt, lo, hi)
    nb = hi - lo
    return (v.view(nb, bt.n, -1, bt.g) * s[..., None] + z[..., None]).view(nb, bt.n, bt.k)


def weights16(w64, dtype):
    """The oracle's dequantised weights RNE16(fmaf(lut, scale, zero)): the float64 value is the exact fma argument (16-bit factors), its
    conversion to f32 the fma's one rounding."""
    return w64.float().to(dtype)


def ref64(bt, step=256):
    """(y64 [B][m][n], S [B][m][n]) float64 numpy, for every problem of the batch."""
    y, S = np.empty((bt.B, bt.m, bt.n)), np.empty((bt.B, bt.m, bt.n))
    step = max(1, min(step, (1 << 25) // (bt.n * bt.k)))
    for lo in range(0, bt.B, step):
        hi = min(lo + step, bt.B)
        w = weights64(bt, lo, hi)
        x = bt.x[lo:hi].double()
        y[lo:hi] = torch.bmm(x, w.transpose(1, 2)).numpy()
        w16 = weights16(w, bt.dtype).double().abs_()
        S[lo:hi] = torch.bmm(x.abs(), w16.transpose(1, 2)).numpy()
    S = np.nan_to_num(S, nan=0.0)   # (where the product is NaN the output must be NaN: no bound is taken there)
    return y, S


def ulp16(y64, dtype):
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(y64, np.float64)), 1e-300)))
    return np.exp2(e - 7) if dtype == BF16 else np.exp2(np.maximum(e, -14) - 10)


def bound(y64, S, dtype):
    """The GEMM contract of DESIGN section 4 (assert_fast_close)."""
    return 0.5 * ulp16(y64, dtype) * (1 + 2.0 ** -7) + 4e-6 * S + 1e-37


def check_f64(y16, y64, S, dtype, what=""):
    """Every output of every problem within the bound (NaN exactly where the float64 product has it); returns the worst error / bound."""
    got = y16.detach().double().cpu().numpy()
    nan = np.isnan(y64)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at {np.argwhere(np.isnan(got) != nan)[:6].tolist()} (problem, row, column) differs from the float64 product"
    ratio = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, y64)) / bound(np.where(nan, 1.0, y64), S, dtype))
    bad = ratio > 1
    assert not bad.any(), (f"{what}: {bad.sum()} / {bad.size} outputs outside the bound, in problems {np.unique(np.nonzero(bad)[0])[:8].tolist()}; "
                           f"first (problem, activation row, weight row) {np.argwhere(bad)[0].tolist()}; worst error / bound {ratio.max():.3f}")
    return float(ratio.max())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def assert_same_bits(a, b, what):
    da = bits(a) != bits(b)
    assert not da.any(), f"{what}: {int(da.sum())} outputs differ, first (problem, activation row, weight row) {da.nonzero()[0].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------------------
# exact probes: every f32 intermediate is exact, the expected output is known to the bit
# ---------------------------------------------------------------------------------------------------------------------------------

def _probe_base(pp, bt):
    """A copy of the batch's shape with a LUT whose entry 0 is 0 and entry 1 is 1.0 (int4: codes 8 and 9; mx4: codes 0 and 2), power-of-two
    scales that differ by (problem, group, row), zeros 0, small-integer activations.  Returns (batch, code of 0, code of 1)."""
    gen = torch.Generator().manual_seed(99 + bt.n + bt.k)
    pb = SimpleNamespace(**vars(bt))
    c0, c1 = {"int4": (8, 9), "mx4": (0, 2)}.get(bt.qtype, (0, 1))
    ng = bt.k // bt.g
    e = (torch.arange(bt.B)[:, None, None] * 5 + torch.arange(ng)[None, :, None] * 3 + torch.arange(bt.n)[None, None, :]) % 7 - 3   # [B][ng][n]
    if bt.qtype == "mx4":
        pb.exps = (127 + e).transpose(1, 2).contiguous().to(torch.uint8)
    else:
        pb.scale = torch.exp2(e.float()).to(bt.dtype)
        pb.zero = torch.zeros_like(pb.scale)
        if bt.lut is not None:
            lut = torch.randint(2, 9, bt.lut.shape, generator=gen).to(bt.dtype)   # (every other entry: an integer that is neither 0 nor 1)
            lut[..., 0], lut[..., 1] = 0.0, 1.0
            pb.lut = lut
    pb.x = torch.randint(-4, 5, bt.x.shape, generator=gen).to(bt.dtype)
    pb.codes = torch.full_like(bt.codes, c0)
    return pb, c0, c1


def probe_columns(pp, bt):
    """pi [B][n]: the column of (problem, row)'s one weight.  The candidates are the first and last column of every wave's slice, of every
    ring slot's super-tile inside it, of every group, every position of one super-tile (so both nibbles and all four byte lanes of a packed
    word), and the two ends of k; (problem, row) walks the list with a stride coprime to its length."""
    st = 16 * bt.inner
    cols = {0, bt.k - 1}
    for w in range(WAVES):
        for l in range(pp.nl[w]):
            s = w * pp.spw + l
            if l < 2 * pp.ring or l >= pp.nl[w] - pp.ring:
                cols |= {s * st, s * st + st - 1}
    cols |= {gi * bt.g for gi in range(bt.k // bt.g)} | {gi * bt.g + bt.g - 1 for gi in range(bt.k // bt.g)}
    cols |= set(range(st, min(2 * st, bt.k)))
    cols = torch.tensor(sorted(cols))
    idx = (torch.arange(bt.B)[:, None] * 37 + torch.arange(bt.n)[None, :] * 11) % len(cols)
    return cols[idx]


def probe_one_weight(pp, bt):
    """One weight per row: (batch, expected y [B][m][n] as the output type).  y = x[b][a][pi(b, r)] scale[b][group][r], exact."""
    pb, c0, c1 = _probe_base(pp, bt)
    pi = probe_columns(pp, bt)
    pb.codes.scatter_(2, pi[:, :, None], torch.full((bt.B, bt.n, 1), c1, dtype=torch.uint8))
    s, _ = scale_zero64(pb, 0, bt.B)
    sc = torch.gather(s, 2, (pi // bt.g)[:, :, None])[:, :, 0]                                      # [B][n]
    xv = torch.gather(pb.x.double(), 2, pi[:, None, :].expand(bt.B, bt.m, bt.n))                    # [B][m][n]
    want = xv * sc[:, None, :]
    assert torch.equal(want.to(bt.dtype).double(), want), "the probe's expected values are 16-bit numbers"
    return pb, want.to(bt.dtype)


def probe_zero_point(pp, bt):
    """All codes select 0; the zero word is 1.0 in one group per (problem, row): y = that group's sum of x, exact (|sum| <= 4 g <= 1024:
    an integer below 2^8 only for bf16 after the draw is thinned, so the activations are 0 outside every fourth column)."""
    assert bt.qtype != "mx4"
    pb, c0, c1 = _probe_base(pp, bt)
    keep = (torch.arange(bt.k) % 8 == (torch.arange(bt.k) // bt.g) % 8)
    pb.x = torch.where(keep[None, None, :], pb.x, torch.zeros_like(pb.x)).clamp(-3, 3)              # |group sum| <= 3 g / 8 <= 96: exact in 16 bits
    ng = bt.k // bt.g
    gsel = (torch.arange(bt.B)[:, None] * 3 + torch.arange(bt.n)[None, :] * 5) % ng                 # [B][n]
    z = torch.zeros(bt.B, ng, bt.n)
    z.scatter_(1, gsel[:, None, :], 1.0)
    pb.zero = z.to(bt.dtype)
    gs = pb.x.double().reshape(bt.B, bt.m, ng, bt.g).sum(dim=3)                                     # [B][m][ng]
    want = torch.gather(gs, 2, gsel[:, None, :].expand(bt.B, bt.m, bt.n))
    assert torch.equal(want.to(bt.dtype).double(), want)
    return pb, want.to(bt.dtype)


def probe_one_hot(pp, bt):
    """One-hot activation rows (the column at the ends of groups and slices, by problem and activation row), power-of-two scales, zeros 0,
    integer LUT entries, random codes: y = lut[b][r][code[b][r][c]] scale[b][group(c)][r], exact."""
    pb, c0, c1 = _probe_base(pp, bt)
    pb.codes = bt.codes.clone()
    pi = probe_columns(pp, bt)
    col = pi[:, :bt.m] if bt.n >= bt.m else pi[:, :1].expand(bt.B, bt.m)                             # [B][m]
    pb.x = torch.zeros_like(bt.x)
    pb.x.scatter_(2, col[:, :, None], torch.full((bt.B, bt.m, 1), 2.0, dtype=bt.dtype))
    tab = table64(pb, 0, bt.B)
    s, _ = scale_zero64(pb, 0, bt.B)
    want = torch.empty(bt.B, bt.m, bt.n, dtype=torch.float64)
    for a in range(bt.m):
        code = torch.gather(pb.codes.long(), 2, col[:, a, None, None].expand(bt.B, bt.n, 1))        # [B][n][1]
        want[:, a, :] = 2.0 * torch.gather(tab, 2, code)[:, :, 0] * torch.gather(s, 2, (col[:, a, None, None] // bt.g).expand(bt.B, bt.n, 1))[:, :, 0]
    want = want + 0.0   # (a sum that starts from +0 never ends as -0)
    assert torch.equal(want.to(bt.dtype).double(), want)
    return pb, want.to(bt.dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------------------

MUTANTS = {
    "ring refill takes the current problem": "f64",
    "global LUT kept across a problem boundary": "f64",
    "row-wise LUT rows one row block late": "f64",
    "activations not restaged": "f64",
    "partial slice runs its full spw": "f64",
    "empty wave adds its clamped load": "f64",
    "scale|zero word per super-tile": "one weight",
    "activation sums indexed from slice 0": "zero point",
    "zero point by both lane halves": "zero point",
    "wave 7 dropped": "f64",
    "partials summed in 16 bits": "f64",
    "last item skipped, first written twice": "all written",
    # (every item is still reached, more than once: the same values are stored again, so only the walk itself shows it -- on the GPU, the time)
    "chunked dealing steps by workgroups": "written once",
    "row block of the wrong operand": "one weight",
    "truncation instead of RNE": "f64",
    # the 16x16x32 layouts request an item's activation sums one item ahead (xs_request): the request that is not renewed
    "LA activation sums of the item before": "zero point",
}


def _walk(pp, mutant):
    """The item walk of every workgroup with its carried state.  Per executed item: where it is written (b, rb) and the (problem, row
    block) each operand is taken from: `ring` (the first `ring` super-tiles of every wave's slice, requested at the end of the previous
    item), `cur` (the later super-tiles), `lut`, `q` (scale | zero words), and the problem `xb` of the activations in LDS."""
    rb_n = pp.rblocks
    rows = []
    glob = pp.qtype == "any4_global"
    for wg in range(pp.workgroups):
        its = wg_items(pp, wg)
        if mutant == "chunked dealing steps by workgroups" and pp.xg:
            its, it, cpos = [], wg * pp.chunk, 0
            while it < pp.items:
                its.append(it)
                big = cpos + 1 >= pp.chunk
                it, cpos = it + (pp.workgroups - (pp.chunk - 1) if big else 1), (0 if big else cpos + 1)
        if not its:
            continue
        if mutant == "last item skipped, first written twice":
            its = [its[0]] + its[:-1]
        dec = lambda it: (it // rb_n, it % rb_n)
        ring_src = lp_src = dec(its[0])
        xs_src = dec(its[0])[0]
        table_src, staged_b, prev = None, dec(its[0])[0], dec(its[0])
        for i, it in enumerate(its):
            b, rb = dec(it)
            nxt = dec(its[i + 1]) if i + 1 < len(its) else (b, rb)
            if mutant == "row-wise LUT rows one row block late" and pp.qtype == "any4_rowwise":
                lp_src, prev = prev, (b, rb)
            rebuild = i == 0 or pp.qtype == "any4_rowwise" or pp.red_alias or (glob and b != table_src[0])
            if mutant == "global LUT kept across a problem boundary" and glob and not pp.red_alias:
                rebuild = i == 0
            if rebuild:
                table_src = lp_src
            if not pp.xg and b != staged_b and mutant != "activations not restaged":
                staged_b = b
            xb = b if pp.xg else staged_b
            xs_b = xs_src if pp.la else xb            # (the 16x16x32 layouts: sums requested into registers during the item before)
            q = (b, rb)
            if mutant == "row block of the wrong operand":
                wrong = rb_n + 1
                q = (min(it // wrong, pp.batch - 1), min(it % wrong, rb_n - 1))
            rows.append((b, rb, ring_src, (b, rb), table_src, q, xb, xs_b))
            lp_src = nxt
            xs_src = xs_src if mutant == "LA activation sums of the item before" else nxt[0]
            ring_src = (b, nxt[1]) if mutant == "ring refill takes the current problem" else nxt
    return rows


def walk_writes(pp, qtype="int4", mutant=None):
    """[batch][rblocks] how often the walk stores each item's outputs."""
    n = torch.zeros(pp.batch, pp.rblocks, dtype=torch.long)
    for row in _walk(SimpleNamespace(**vars(pp), qtype=qtype), mutant):
        n[row[0], row[1]] += 1
    return n


def twin(pp, bt, mutant=None, step=128):
    """y [B][m][n] of the output type, NaN where no item wrote; the schedule of the module docstring on the plan `pp`."""
    assert mutant is None or mutant in MUTANTS, mutant
    pp = SimpleNamespace(**vars(pp), qtype=bt.qtype)
    f32 = torch.float32
    st = 16 * bt.inner
    seg = min(st, bt.g)                       # k elements between two possible group boundaries
    sps = st // seg                           # segments per super-tile (= GPS)
    gseg = bt.g // seg                        # segments per group
    nseg_w = pp.spw * sps
    n, k, m, B = bt.n, bt.k, bt.m, bt.B
    y = torch.full((B, m, n), float("nan"), dtype=bt.dtype)
    walk = _walk(pp, mutant)
    halves = 2 if pp.dot else 1
    # the k positions of lane half h inside a 32-k chunk: quads 2 h, 2 h + 1 hold k = 2 q + {0, 8, 16, 24, 1, 9, 17, 25}
    half_of = torch.tensor([(kk % 8) // 4 for kk in range(32)]).repeat(k // 32) if halves == 2 else torch.zeros(k, dtype=torch.long)
    rw = pp.rw
    running = pp.kernel in ("m1", "m1_mfma", "lean")
    s64, z64 = scale_zero64(bt, 0, B)
    for lo in range(0, len(walk), step):
        part = walk[lo:lo + step]
        ni = len(part)
        rows_of = lambda src: (torch.tensor([s[1] for s in src])[:, None] * rw + torch.arange(rw)[None, :]).clamp(max=n - 1)    # [ni][rw]
        prob = lambda src: torch.tensor([s[0] for s in src])
        def take(t3, src):                       # t3 [B][n][...] -> [ni][rw][...]
            return t3[prob(src)[:, None], rows_of(src)]
        codes_cur = take(bt.codes, [p[3] for p in part]).long()
        codes_ring = take(bt.codes, [p[2] for p in part]).long()
        # which super-tiles of a row come through the ring from the previous item's requests
        s_idx = torch.arange(pp.ksuper)
        from_ring = ((s_idx % pp.spw) < pp.ring) if pp.spw else torch.zeros_like(s_idx, dtype=torch.bool)
        codes = torch.where(from_ring.repeat_interleave(st)[None, None, :], codes_ring, codes_cur)
        tab = torch.stack([table64(bt, s[0], s[0] + 1)[0] for s in [p[4] for p in part]])                 # [ni][n][16]
        tab = tab[torch.arange(ni)[:, None], rows_of([p[4] for p in part])].to(f32)                       # [ni][rw][16]
        v = torch.gather(tab, 2, codes)                                                                   # [ni][rw][k] f32 (16-bit values)
        qsrc, rsrc = [p[5] for p in part], [p[2] for p in part]
        sc_cur, zp_cur = take(s64, qsrc).to(f32), take(z64, qsrc).to(f32)                                 # [ni][rw][ng]
        qring = [(r[0], r[1]) if mutant != "row block of the wrong operand" else q for r, q in zip(rsrc, qsrc)]
        sc_ring, zp_ring = take(s64, qring).to(f32), take(z64, qring).to(f32)
        x = bt.x[torch.tensor([p[6] for p in part])].to(f32)                                              # [ni][m][k]
        xs = bt.x[torch.tensor([p[7] for p in part])].to(f32).reshape(ni, m, k // bt.g, bt.g).sum(dim=3)   # the per-group activation sums
        # products per (segment, lane half): exact 16 x 16-bit products, f32 sums
        P = torch.zeros(ni, m, rw, k // seg, halves, dtype=f32)
        for h in range(halves):
            mask = (half_of == h).to(f32)
            P[..., h] = torch.einsum("iagk,irgk->iarg", (x * mask).reshape(ni, m, k // seg, seg), v.reshape(ni, rw, k // seg, seg))
        total = torch.zeros(ni, m, rw, dtype=f32)
        for w in range(WAVES):
            nl = pp.nl[w]
            if mutant == "wave 7 dropped" and w == 7:
                continue
            run = nl
            if mutant == "partial slice runs its full spw" and 0 < nl < pp.spw:
                run = pp.spw
            if mutant == "empty wave adds its clamped load" and nl == 0:
                run = 1
            yacc = torch.zeros(ni, m, rw, halves, dtype=f32)
            acc = torch.zeros(ni, m, rw, halves, dtype=f32)
            prev = torch.zeros_like(acc)
            for j in range(run * sps):
                l = j // sps
                s = w * pp.spw + l if l < nl else 0                                      # (a request past the slice reads super-tile 0)
                sg = s * sps + j % sps                                                  # the segment
                acc = acc + P[:, :, :, sg, :]
                gi = sg // gseg
                last = (sg + 1) % gseg == 0 or j + 1 == run * sps
                if not last:
                    continue
                gq = min(s, k // bt.g - 1) if (mutant == "scale|zero word per super-tile" and pp.nsg > 1) else gi
                gx = (gi - (w * pp.spw * sps) // gseg) % (k // bt.g) if mutant == "activation sums indexed from slice 0" else gi
                l_first = max((gi * gseg) // sps - w * pp.spw, 0)                        # the group's first super-tile carries its word
                ring_q = l_first < pp.ring and l < nl
                sc = (sc_ring if ring_q else sc_cur)[:, None, :, gq, None]
                zp = (zp_ring if ring_q else zp_cur)[:, None, :, gq, None].expand(ni, 1, rw, halves).clone()
                if halves == 2 and mutant != "zero point by both lane halves":
                    zp[..., 1] = 0.0
                d = acc - prev if running else acc
                if running:
                    prev = acc
                else:
                    acc = torch.zeros_like(acc)
                yacc = (yacc.double() + sc.double() * d.double()).to(f32)               # fma: one rounding
                yacc = (yacc.double() + zp.double() * xs[:, :, None, gx, None].double()).to(f32)
            pw = yacc.sum(dim=3) if halves == 2 else yacc[..., 0]                       # the lane halves
            total = (total + pw).to(bt.dtype).to(f32) if mutant == "partials summed in 16 bits" else total + pw
        out = total.to(bt.dtype)
        if mutant == "truncation instead of RNE":  # one step back towards zero where RNE rounded away from it
            away = out.float().abs() > total.abs()
            out = torch.where(away, (out.view(torch.int16) - 1).view(bt.dtype), out)
        if bt.bias is not None:
            bias = bt.bias[torch.tensor([p[0] for p in part])[:, None], rows_of([(0, p[1]) for p in part])]          # [ni][rw]
            out = (out.float() + bias[:, None, :].float()).to(bt.dtype)
        for i, p in enumerate(part):
            r0 = p[1] * rw
            r1 = min(r0 + rw, n)
            y[p[0], :, r0:r1] = out[i, :, :r1 - r0]
    return y


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's own answers (host-only: nothing is launched, no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------------------

def lib_plan(m, wrows, k, g, qtype, inner=4, on_right=True, batch=2, dtype=BF16, numerics="fast", workspace=True, bias=False, norm=False,
             epilogue=False, w_format=0):
    """(tg_gemm_w4_plan, tg_gemm_w4_plan_detail, tg_gemm_w4_workspace_bytes) of the call, on dummy pointers that the planner never
    dereferences; with `workspace` the call brings exactly the bytes the query asks for."""
    import ctypes

    from any4_amd import _lib

    L = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63
    args = _lib.W4Gemm(x=p, w=p, qinfo=p, lut=p, y=p, m=m, wrows=wrows, k=k, group=g, qtype=QT[qtype], dtype=_lib.TG_BF16 if dtype == BF16 else _lib.TG_F16,
                       w_on_right=1 if on_right else 0, inner_k_tiles=inner, batch=batch, stride_x=16, stride_w=16, stride_qinfo=16, stride_lut=16,
                       stride_y=16, numerics=NUMERICS[numerics], bias=p if bias else None, stride_bias=16 if bias else 0,
                       norm_weight=p if norm else None, norm_eps=1e-5, epilogue=_lib.TG_EPI_SWIGLU if epilogue else 0,
                       w_format=w_format)
    need = L.tg_gemm_w4_workspace_bytes(ctypes.byref(args))
    if workspace and need > 0:
        args.workspace, args.workspace_bytes = p, need
    return L.tg_gemm_w4_plan(ctypes.byref(args), 0), L.tg_gemm_w4_plan_detail(ctypes.byref(args), 0), need


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_pair_f64.py (the CPU file asserts their regimes and runs the twin on them)
# ---------------------------------------------------------------------------------------------------------------------------------

def smallest_xg_k(m, g=128, qtype="any4_rowwise", inner=4, wrows=64, batch=200, dtype=BF16):
    """The smallest k (a multiple of the group and of 128) at which the plan says that a call of m rows takes the workspace variant."""
    for k in range(max(g, 128), 16385, max(g, 128)):
        pp = pair_plan(m, wrows, k, g, qtype, inner, True, batch, dtype)
        if pp.family == "pair" and pp.xg:
            return k
    raise AssertionError("no XG k")


def case(name):
    """name -> SimpleNamespace(m, n, k, g, qtype, inner, on_right, batch, dtype, numerics, bias)."""
    c = dict(inner=4, on_right=True, dtype=BF16, numerics="fast", bias=False)
    c.update(_CASES[name])
    if c["k"] in ("xg1", "xg8"):
        c["k"] = smallest_xg_k(int(c["k"][2:]), c["g"], c["qtype"], c["inner"])
    return SimpleNamespace(name=name, **c)


_CASES = {
    # the lean m = 1 kernel: bf16 / fp16, row-wise / global / int4; 9 units (a partial slice, empty waves), 5 units, 1 unit, 48 units
    "lean rowwise 9 units rblocks 3": dict(m=1, n=192, k=1152, g=128, qtype="any4_rowwise", batch=173),
    "lean global fp16 ranges of 5-6": dict(m=1, n=64, k=640, g=128, qtype="any4_global", batch=5 * 512 + 7, dtype=F16),
    "lean int4 one unit rblocks 5 ranges of 16": dict(m=1, n=320, k=128, g=128, qtype="int4", batch=1700),
    "lean rowwise 6 rounds 192 items": dict(m=1, n=64, k=6144, g=128, qtype="any4_rowwise", batch=192),
    "lean global 17 units": dict(m=1, n=64, k=2176, g=128, qtype="any4_global", batch=600),
    # the m = 1 specialisation: a group of 1 / 2 (bias: lean declines) / 4 super-tiles; innerKTiles 2 and 8
    "m1 g64": dict(m=1, n=40, k=576, g=64, qtype="any4_rowwise", batch=200),
    "m1 g128 bias 17 units": dict(m=1, n=192, k=2176, g=128, qtype="any4_global", batch=173, bias=True),
    "m1 g256 ring of four": dict(m=1, n=64, k=1280, g=256, qtype="int4", batch=600),
    "m1 g256 ring of four 9 units fp16": dict(m=1, n=64, k=2304, g=256, qtype="any4_rowwise", batch=300, dtype=F16),
    "m1 inner 2 g64": dict(m=1, n=8, k=576, g=64, qtype="any4_rowwise", inner=2, batch=300),
    "m1 inner 2 g32": dict(m=1, n=72, k=288, g=32, qtype="int4", inner=2, batch=150),
    "m1 inner 8 g256": dict(m=1, n=64, k=1280, g=256, qtype="any4_global", inner=8, batch=200),
    "m1 inner 8 g128": dict(m=1, n=40, k=1152, g=128, qtype="any4_rowwise", inner=8, batch=200),
    # the general template
    "general m2 NSG R": dict(m=2, n=192, k=1152, g=128, qtype="any4_rowwise", batch=173),
    "general m3 NSG 0 partial round": dict(m=3, n=40, k=576, g=64, qtype="any4_rowwise", batch=400),
    "general m4 GPS 2": dict(m=4, n=64, k=320, g=32, qtype="any4_global", batch=1000),
    "general m5 red_alias": dict(m=5, n=192, k=1152, g=128, qtype="int4", batch=173),
    "general m8 inner 2 g256 fp16": dict(m=8, n=64, k=768, g=256, qtype="any4_rowwise", inner=2, batch=200, dtype=F16),
    "general m2 inner 2 global ranges of 2-3": dict(m=2, n=8, k=576, g=64, qtype="any4_global", inner=2, batch=1200),
    "general m8 full slices": dict(m=8, n=8, k=512, g=64, qtype="any4_global", batch=250),
    # mx4
    "mx4 m1": dict(m=1, n=64, k=1280, g=32, qtype="mx4", batch=300),
    "mx4 m8": dict(m=8, n=64, k=1280, g=32, qtype="mx4", batch=200),
    # the workspace variant at the smallest k at which the plan says XG; k = 14336; chunked dealing with a partial last visit
    "xg m1": dict(m=1, n=64, k="xg1", g=128, qtype="any4_rowwise", batch=192),
    "xg m8": dict(m=8, n=64, k="xg8", g=128, qtype="any4_global", batch=200),
    "xg m4 k14336": dict(m=4, n=64, k=14336, g=128, qtype="int4", batch=192),
    "xg m8 chunked": dict(m=8, n=64, k="xg8", g=128, qtype="any4_rowwise", batch=8195),
    "xg m1 k14336": dict(m=1, n=64, k=14336, g=128, qtype="any4_global", batch=192),
    # per kernel class: three or more items in every workgroup over problems of three row blocks, 9 units (a partial slice, empty waves)
    "walk m1 g64": dict(m=1, n=192, k=576, g=64, qtype="any4_rowwise", batch=520),
    "walk m1 g128 bias": dict(m=1, n=192, k=1152, g=128, qtype="any4_global", batch=520, bias=True),
    "walk m1 g128 bias k6144": dict(m=1, n=64, k=6144, g=128, qtype="int4", batch=192, bias=True),
    "walk m1 g256 ring of four": dict(m=1, n=192, k=2304, g=256, qtype="any4_rowwise", batch=520),
    "walk m1 inner 2 g64": dict(m=1, n=192, k=576, g=64, qtype="any4_global", inner=2, batch=520),
    "walk m1 inner 8 g128": dict(m=1, n=192, k=1152, g=128, qtype="any4_rowwise", inner=8, batch=520),
    "walk mfma m1": dict(m=1, n=192, k=1152, g=128, qtype="any4_global", batch=520, numerics="fast_mfma"),
    "walk general m3 NSG 0": dict(m=3, n=192, k=576, g=64, qtype="any4_rowwise", batch=520),
    "walk general m2 NSG R": dict(m=2, n=192, k=1152, g=128, qtype="any4_global", batch=520),
    "walk general m5 red_alias": dict(m=5, n=192, k=1152, g=128, qtype="any4_global", batch=520),
    "walk general m4 GPS 2": dict(m=4, n=192, k=576, g=32, qtype="any4_global", batch=520),
    "walk general m2 inner 2": dict(m=2, n=192, k=576, g=64, qtype="any4_rowwise", inner=2, batch=520),
    "walk mx4 m1": dict(m=1, n=192, k=1280, g=32, qtype="mx4", batch=520),
    "walk mx4 m8": dict(m=8, n=192, k=1280, g=32, qtype="mx4", batch=520),
    "mx4 m1 k14336": dict(m=1, n=64, k=14336, g=32, qtype="mx4", batch=192),
    "walk xg m1": dict(m=1, n=192, k="xg1", g=128, qtype="any4_rowwise", batch=512),
    "walk xg m8": dict(m=8, n=192, k=1152, g=128, qtype="any4_global", batch=520),
    "walk la1 inner 4 m5": dict(m=5, n=96, k=1152, g=128, qtype="any4_rowwise", on_right=False, batch=520),
    "walk la1 inner 2 m2 g32": dict(m=2, n=96, k=288, g=32, qtype="any4_global", inner=2, on_right=False, batch=520),
    "walk la1 m16 mx4": dict(m=16, n=96, k=1280, g=32, qtype="mx4", on_right=False, batch=520),
    "la1 m5 k14336": dict(m=5, n=64, k=14336, g=128, qtype="any4_global", on_right=False, batch=96),
    "walk la2 m9": dict(m=9, n=96, k=1152, g=128, qtype="any4_rowwise", batch=520),
    "walk la2 m13 inner 2": dict(m=13, n=96, k=576, g=64, qtype="any4_global", inner=2, batch=520),
    "la2 m9 k14336": dict(m=9, n=40, k=14336, g=128, qtype="int4", batch=200),
    # the MFMA m = 1 flavour
    "mfma m1": dict(m=1, n=192, k=1152, g=128, qtype="any4_rowwise", batch=173, numerics="fast_mfma"),
    # the 16x16x32 layouts
    "la1 inner 4 m5": dict(m=5, n=48, k=1152, g=128, qtype="any4_rowwise", on_right=False, batch=200),
    "la1 inner 2 m2 g32": dict(m=2, n=48, k=576, g=32, qtype="int4", inner=2, on_right=False, batch=200),
    "la1 inner 4 m16 mx4": dict(m=16, n=64, k=1280, g=32, qtype="mx4", on_right=False, batch=100),
    "la2 m9": dict(m=9, n=64, k=1152, g=128, qtype="any4_rowwise", batch=192),
    "la2 m13 inner 2": dict(m=13, n=40, k=576, g=64, qtype="any4_global", inner=2, batch=200),
    "la2 m16": dict(m=16, n=64, k=640, g=128, qtype="int4", batch=192),
}
CASE_NAMES = list(_CASES)

# instantiations that launch_pair_m declines (tg_pair.hip): (m, g, qtype, inner) -- asserted as declined, not skipped
DECLINED = [(2, 256, "any4_rowwise", 8), (1, 64, "any4_rowwise", 8), (1, 32, "int4", 8), (1, 256, "mx4", 8), (8, 128, "any4_global", 8)]

# one representative per kernel class for the exact probes
PROBE_CASES = ["lean rowwise 9 units rblocks 3", "m1 g64", "m1 g256 ring of four 9 units fp16", "m1 inner 8 g128", "general m3 NSG 0 partial round",
               "general m4 GPS 2", "general m5 red_alias", "mx4 m8", "xg m8", "mfma m1", "la1 inner 4 m5", "la2 m13 inner 2",
               "walk la1 inner 4 m5", "walk la2 m13 inner 2", "walk mx4 m8", "walk general m2 inner 2"]


@functools.lru_cache(maxsize=2)
def case_batch(name):
    c = case(name)
    bt = make_batch(c.m, c.n, c.k, c.g, c.qtype, c.batch, c.dtype, seed=CASE_NAMES.index(name), inner=c.inner, on_right=c.on_right)
    if c.qtype == "mx4":  # an exponent of 255 in one problem only: NaN in one weight row of that problem
        bt.exps[c.batch // 2, 5, 3] = 255
    if c.bias:  # an all-zero bias: the call leaves the lean kernel for the general template and the sums stay what the references describe
        bt.bias = torch.zeros(c.batch, c.n, dtype=c.dtype)
    return bt


def random_bias(bt):
    return torch.randn(bt.B, bt.n, generator=torch.Generator().manual_seed(5)).to(bt.dtype)


def case_plan(name):
    c = case(name)
    return pair_plan(c.m, c.n, c.k, c.g, c.qtype, c.inner, c.on_right, c.batch, c.dtype, c.numerics, True, bias=c.bias)
