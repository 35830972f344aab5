"""Float64 references, input builders and bounds for the mixture-of-experts kernels (dg_moe_route, dg_moe_launch with DG_MOE_GEMV; any4_amd/moe.py:
moe_ref is the definition).  A plain helper module (not a conftest), in the style of tests/lora_ref.py and tests/fused_ref.py;
tests/test_moe_cpu.py checks it on the CPU, tests/test_gpu_moe.py runs the kernels against it.

Nothing here uses any4_amd.moe's unpacking or weights: codes come from rand_problem, are packed by the oracle, and the float64 weights
are formed from codes, scales, zeros and LUT directly, so a layout mistake in the package cannot cancel against the same mistake here.

Bounds (u = 2^-24; nothing is fitted to a kernel's output):

  router logit   A[i][e] = 4e-6 sum_c |x[i][c] router_w[e][c]|: the project's accumulation slack (tests/w16_ref.py).  It equals 67 u, i.e.
                 covers 67 rounded additions on partial sums that never exceed the sum of absolute values.  The router's longest chain:
                 a lane's 16 fused multiply-adds per pass of 4096 elements (k <= 4096 here: one pass), 6 steps of the wave sum, 8 partials
                 in wave order: 30.
  selection      CONDITION, asserted on the float64 logits before any id is compared: among a row's first top_k + 1 ranks every adjacent
                 gap exceeds twice the larger of the two logits' allowances.  Then no rounding within the allowance can change the set
                 or the order of the selected experts.
  gates          g_s = exp(l_s) / sum_t exp(l_t) over the selected t: d g_s = g_s (d l_s - sum_t g_t d l_t), so |d g_s| <= 2 g_s (1 - g_s)
                 max_t A_t <= max_t A_t / 2 to first order; allowed: 2 max_t A_t (four times that, which swallows the higher orders for
                 A << 1) + 2^-22 for the f32 softmax itself (expf within an ulp, two sums of at most 64 / 8 terms, two divisions:
                 relative 2^-23 + 2^-24 + ... on values <= 1).
  GATE_UP        sums known to contract(ref, S) (tests/fused_ref.py: half an ulp16 (1 + 2^-7) + 4e-6 S, S = sum |x w|), pushed through the
                 SwiGLU store with its two roundings by fused_ref.swiglu_of_sums (glue_ref.two_roundings_bound inside).
  DOWN           contract(ref, S) with S[i] = sum_s g_s sum_c |a_s[c] w[c]| + u |residual|.  The chain behind one output: 16 v_dot2 and two
                 fused multiply-adds per step, k / 1024 steps per wave (2 at k = 1664), the four sub-slots (2), 8 partials, top_k <= 3 gate
                 terms, the residual: below 67 roundings for k <= 2048, the largest k this module's cases use.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from any4_amd.moe import ExpertStack
from tests.conftest import bits16, from_bits16  # noqa: F401
from tests.fused_ref import contract, guard_intact, guarded, make_inputs, swiglu_of_sums  # noqa: F401
from tests.test_gpu_parity import oracle_weights, rand_problem

BF16, F16 = torch.bfloat16, torch.float16
QT = {"int4": 0, "any4_global": 1, "any4_rowwise": 2}
U32 = 2.0 ** -24
SLACK = 4e-6
SENTINEL = 0x5A5A


@functools.lru_cache(maxsize=4)
def make_stack(oracle, E, n, k, g, qtype, dtype, seed=0):
    """E experts of one linear [n][k] (CPU): (ExpertStack with oracle-packed words, per-expert list of (codes, qinfo, lut))."""
    parts = [rand_problem(n, k, g, 1, qtype, dtype=dtype, seed=seed * 131 + e * 17 + n + k + g) for e in range(E)]
    words = torch.stack([torch.from_numpy(oracle.pack_Bint4(c.numpy(), 4).astype(np.int32)) for c, _, _, _ in parts])
    qinfo = torch.stack([q for _, _, q, _ in parts])
    lut = None if qtype == "int4" else torch.stack([l for _, _, _, l in parts])
    raw = [(c, q, l) for c, _, q, l in parts]
    return ExpertStack(n, k, g, words.contiguous(), qinfo.contiguous(), None if lut is None else lut.contiguous()), raw


def to_dev(stack, device, **over):
    """A copy of the stack on `device` (over: tensors to put in place of words / qinfo / lut)."""
    f = lambda name: None if getattr(stack, name) is None else over.get(name, getattr(stack, name)).to(device).contiguous()
    return ExpertStack(stack.n, stack.k, stack.group, f("words"), f("qinfo"), f("lut"))


def weights64(raw_e, g):
    """[n][k] float64 numpy: scale * lut[code] + zero from codes, qinfo [k / g][n][2] and LUT, not rounded."""
    codes, qinfo, lut = raw_e
    c = codes.numpy().astype(np.int64)
    n, k = c.shape
    if lut is None:
        v = (c - 8).astype(np.float64)
    else:
        l = lut.double().numpy()
        l = np.broadcast_to(l, (n, 16)) if l.ndim == 1 else l
        v = np.take_along_axis(l, c, axis=1)
    q = qinfo.double().numpy()
    return v * np.repeat(q[:, :, 0].T, g, axis=1) + np.repeat(q[:, :, 1].T, g, axis=1)


def weights16(oracle, raw_e, g, qtype, dtype):
    """[n][k] 16-bit tensor: the oracle's dequantised weights RNE16(fma(lut[code], scale, zero))."""
    codes, qinfo, lut = raw_e
    return from_bits16(oracle_weights(oracle, codes, g, qtype, qinfo, lut, dtype), dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# router
# ---------------------------------------------------------------------------------------------------------------------------------

def router_inputs(m, k, E, dtype, seed):
    """x by fused_ref.make_inputs' recipe, router_w = randn / sqrt(k), seeded (CPU tensors of `dtype`)."""
    x = make_inputs(m, 16, k, dtype, seed)[0]
    gen = torch.Generator().manual_seed(seed * 7919 + 23)
    return x, (torch.randn(E, k, generator=gen) / k ** 0.5).to(dtype)


def route_ref64(x16, rw16, top_k):
    """(ids [m][top_k], gates [m][top_k], logits [m][E], A [m][E], gate_tol [m][top_k]) float64 numpy."""
    x, w = x16.double().numpy(), rw16.double().numpy()
    logits = x @ w.T
    A = SLACK * (np.abs(x) @ np.abs(w).T)
    order = np.argsort(-logits, axis=1, kind="stable")      # (descending, the lower index first among equals)
    ids = order[:, :top_k]
    ls = np.take_along_axis(logits, ids, axis=1)
    ex = np.exp(ls - ls[:, :1])
    gates = ex / ex.sum(axis=1, keepdims=True)
    gate_tol = 2 * np.take_along_axis(A, ids, axis=1).max(axis=1, keepdims=True) + 2.0 ** -22 + 0 * gates
    return ids, gates, logits, A, gate_tol


def margin_ok(logits, A, top_k):
    """The selection condition per row: every adjacent gap among the first top_k + 1 ranks exceeds twice the larger allowance of the two
    (exact ties -- duplicated router rows -- are the tie tests' business and fail this on purpose).  Returns (ok [m] bool, worst ratio)."""
    order = np.argsort(-logits, axis=1, kind="stable")[:, :top_k + 1]
    ls, As = np.take_along_axis(logits, order, axis=1), np.take_along_axis(A, order, axis=1)
    if ls.shape[1] < 2:
        return np.ones(len(ls), bool), np.inf
    gap = ls[:, :-1] - ls[:, 1:]
    need = 2 * np.maximum(As[:, :-1], As[:, 1:])
    return (gap > need).all(axis=1), float((gap / need).min())


# ---------------------------------------------------------------------------------------------------------------------------------
# the two GEMV stages
# ---------------------------------------------------------------------------------------------------------------------------------

def valid_ids(ids, E):
    ids = np.asarray(ids, np.int64)
    return np.where((ids >= 0) & (ids < E), ids, -1)


def gate_up_ref64(raw, g, x16, ids, E):
    """DG_MOE_GATE_UP: (ref [m top_k][n / 2], tol) float64 numpy; pairs without a valid id: zeros, tol 0 (their bits are +0)."""
    dtype = x16.dtype
    ids = valid_ids(ids, E)
    m, top_k = ids.shape
    x = x16.double().numpy()
    n = raw[0][0].shape[0]
    ref, tol = np.zeros((m * top_k, n // 2)), np.zeros((m * top_k, n // 2))
    for e in np.unique(ids[ids >= 0]):
        w = weights64(raw[e], g)
        rows = np.unique(np.nonzero(ids == e)[0])
        sums, S = x[rows] @ w.T, np.abs(x[rows]) @ np.abs(w).T
        y, t = swiglu_of_sums(sums, contract(sums, S, dtype), dtype)
        for j, i in enumerate(rows):
            for s in np.nonzero(ids[i] == e)[0]:
                ref[i * top_k + s], tol[i * top_k + s] = y[j], t[j]
    return ref, tol


def down_ref64(raw, g, act16, ids, gates32, E, res16=None):
    """DG_MOE_DOWN: (ref [m][n], tol) float64 numpy from the 16-bit pair rows act16 [m top_k][k] and the f32 gates."""
    dtype = act16.dtype
    ids = valid_ids(ids, E)
    m, top_k = ids.shape
    a = act16.double().numpy()
    gt = gates32.double().numpy()
    n = raw[0][0].shape[0]
    ref, S = np.zeros((m, n)), np.zeros((m, n))
    for e in np.unique(ids[ids >= 0]):
        w = weights64(raw[e], g)
        for i, s in zip(*np.nonzero(ids == e)):
            ref[i] += gt[i, s] * (a[i * top_k + s] @ w.T)
            S[i] += abs(gt[i, s]) * (np.abs(a[i * top_k + s]) @ np.abs(w).T)
    if res16 is not None:
        r = res16.double().numpy()
        ref, S = ref + r, S + np.abs(r)
    return ref, contract(ref, S, dtype)


def spread_ids(m, top_k, E, seed):
    """ids [m][top_k]: distinct experts within a row, seeded."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(E)[:top_k] for _ in range(m)]).astype(np.int32)


def pair_inputs(rows, k, dtype, seed):
    """[rows][k] activations: make_inputs' recipe (row scales 2^((a mod 5) - 2))."""
    return make_inputs(rows, 16, k, dtype, seed)[0]


def plan(stage, n, k, m, top_k, E=8, g=64, qtype="any4_rowwise", dtype=BF16, device=-1):
    """decode_ops.moe_plan for a shape: (workgroups, units per workgroup, pairs per sweep, waves with some k)."""
    from any4_amd import decode_ops as G

    return G.moe_plan(stage, SimpleNamespace(n=n, k=k, E=E, group=g, qtype=QT[qtype], dtype=dtype), m, top_k, device)


def assert_regimes_reached(cases, device=-1):
    """Over the (stage, n, k, m, top_k) cases: one with fewer 16-row units than compute units, one whose last workgroup owns fewer units
    than the others, one with several passes per workgroup, one in which some waves own no k."""
    seen = set()
    for stage, n, k, m, top_k in cases:
        wgs, upw, _, waves = plan(stage, n, k, m, top_k, device=device)
        units = n // 16
        seen |= {"few" if units < 256 else "", "remainder" if units % upw else "", "passes" if upw > 1 else "", "idle waves" if waves < 8 else ""}
    missing = {"few", "remainder", "passes", "idle waves"} - seen
    assert not missing, f"regimes not reached: {missing}"
