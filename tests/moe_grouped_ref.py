"""Float64 references, crafted inputs and bounds for the GROUPED mixture-of-experts path (dg_moe_group, dg_moe_launch with DG_MOE_GROUPED; any4_amd/moe.py:
moe_grouped_ref and group_ref are the definitions).  A plain helper module (not a conftest), in the style of tests/moe_ref.py, from which it
takes stacks, inputs and the router's references; tests/test_moe_grouped_cpu.py checks it on the CPU, tests/test_gpu_moe_grouped.py runs the
kernels against it.

Weights.  A tile GEMM dequantises into LDS: its weights are w16 = RNE16(fma(f32(lut[row][code]), f32(scale), f32(zero))).  Here they are the
ORACLE's (moe_ref.weights16: formed from codes, qinfo and LUT by the reference C code), not the package's unpacking; sums are float64 over them.

Bounds (nothing is fitted to a kernel's output):
  GATE_UP   contract(ref, S) (tests/fused_ref.py: half an ulp16 (1 + 2^-7) + 4e-6 S) with S = sum |x w16|, pushed through the SwiGLU store
            with its two roundings by fused_ref.swiglu_of_sums.
  DOWN      contract(ref, S) with S[i] = sum_s g_s sum |a_s w16| + |residual|, as moe_ref.down_ref64.
  The slack 4e-6 S is 67 u (u = 2^-24): 67 rounded additions on partial sums that never exceed S.  The kernel's longest chain behind one
  output: one v_mfma_f32_16x16x32 per 32 k into ONE f32 accumulator, k ascending, never split over workgroups or waves -- 16 of them at
  k = 512, the largest k here.  Counting an MFMA as four rounded additions (its 32 products in four blocks of 8 k, each block's sum added
  with one rounding: an ASSUMPTION about the matrix core; tests/tile_ref.py holds the same MFMA chain to the same contract) gives 64;
  the combine adds top_k = 2 fused multiply-adds and the residual: 67.  The GATE_UP chain is the 64 alone.
"""
import numpy as np

from any4_amd.moe import group_ref
from tests import moe_ref as R
from tests.moe_ref import BF16, F16, QT  # noqa: F401
from tests.fused_ref import contract, swiglu_of_sums

GU, DN = 0, 1
_W16 = {}


def w16_64(oracle, raw, e, g, qtype, dtype):
    """[n][k] float64 numpy: the oracle's 16-bit weights of expert e (cached per stack)."""
    key = (id(raw), e)
    if key not in _W16:
        _W16[key] = (raw, R.weights16(oracle, raw[e], g, qtype, dtype).double().numpy())   # (raw kept alive: its id is the key)
    return _W16[key][1]


def gate_up_ref64(oracle, raw, g, qtype, x16, ids, E):
    """DG_MOE_GATE_UP of the grouped path: (ref [m top_k][n / 2], tol) float64 numpy; pairs without a valid id: zeros, tol 0."""
    dtype = x16.dtype
    ids = R.valid_ids(ids, E)
    m, top_k = ids.shape
    x = x16.double().numpy()
    n = raw[0][0].shape[0]
    ref, tol = np.zeros((m * top_k, n // 2)), np.zeros((m * top_k, n // 2))
    for e in np.unique(ids[ids >= 0]):
        w = w16_64(oracle, raw, int(e), g, qtype, dtype)
        rows = np.unique(np.nonzero(ids == e)[0])
        sums, S = x[rows] @ w.T, np.abs(x[rows]) @ np.abs(w).T
        y, t = swiglu_of_sums(sums, contract(sums, S, dtype), dtype)
        for j, i in enumerate(rows):
            for s in np.nonzero(ids[i] == e)[0]:
                ref[i * top_k + s], tol[i * top_k + s] = y[j], t[j]
    return ref, tol


def act16_ref(oracle, raw, g, qtype, x16, ids, E):
    """[m top_k][n / 2] 16-bit tensor: the definition's activation rows RNE16(RNE16(silu(RNE16(gate))) RNE16(up)) from float64 sums over the
    oracle's 16-bit weights (rows of pairs without a valid id: zeros) -- what the DOWN reference of a chained block starts from."""
    import torch

    dtype = x16.dtype
    ids = R.valid_ids(ids, E)
    m, top_k = ids.shape
    x = x16.double().numpy()
    out = torch.zeros(m * top_k, raw[0][0].shape[0] // 2, dtype=dtype)
    r16 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).double()
    for i in range(m):
        for s in range(top_k):
            if ids[i, s] >= 0:
                gv = (w16_64(oracle, raw, int(ids[i, s]), g, qtype, dtype) @ x[i]).reshape(-1, 2, 8)
                g16, u16 = r16(gv[:, 0].reshape(-1)), r16(gv[:, 1].reshape(-1))
                out[i * top_k + s] = ((g16 / (1 + torch.exp(-g16))).to(dtype).double() * u16).to(dtype)
    return out


def down_ref64(oracle, raw, g, qtype, act16, ids, gates32, E, res16=None):
    """DG_MOE_DOWN of the grouped path (GEMM and combine): (ref [m][n], tol) float64 numpy from the 16-bit pair rows and the f32 gates."""
    dtype = act16.dtype
    ids = R.valid_ids(ids, E)
    m, top_k = ids.shape
    a = act16.double().numpy()
    gt = gates32.double().numpy()
    n = raw[0][0].shape[0]
    ref, S = np.zeros((m, n)), np.zeros((m, n))
    for e in np.unique(ids[ids >= 0]):
        w = w16_64(oracle, raw, int(e), g, qtype, dtype)
        ii, ss = np.nonzero(ids == e)
        pr = ii * top_k + ss
        d, Sd = a[pr] @ w.T, np.abs(a[pr]) @ np.abs(w).T
        np.add.at(ref, ii, gt[ii, ss][:, None] * d)
        np.add.at(S, ii, np.abs(gt[ii, ss])[:, None] * Sd)
    if res16 is not None:
        r = res16.double().numpy()
        ref, S = ref + r, S + np.abs(r)
    return ref, contract(ref, S, dtype)


def plan(stage, n, k, m, top_k, E=8, g=64, qtype="any4_rowwise", dtype=BF16, device=-1):
    """decode_ops.moe_grouped_plan for a shape: (bm, bn, m-extent bound, n tiles, super-tiles per step, group ws bytes, f32 ws bytes)."""
    from types import SimpleNamespace

    from any4_amd import decode_ops as G

    return G.moe_grouped_plan(stage, SimpleNamespace(n=n, k=k, E=E, group=g, qtype=QT[qtype], dtype=dtype), m, top_k, device)


def crafted_counts(bm, E=8):
    """Pairs per expert: exactly the values {0, 1, bm - 1, bm, bm + 1, 2 bm + 3} (an even total for top_k = 2)."""
    c = [0, 1, bm - 1, bm, bm + 1, 2 * bm + 3, 1, 1]
    assert E == 8 and sum(c) % 2 == 0
    return c


def crafted_ids(bm, top_k=2, E=8, seed=0):
    """ids [m][top_k] whose per-expert pair counts are crafted_counts(bm), shuffled (two slots of a row may name the same expert)."""
    counts = crafted_counts(bm, E)
    flat = np.repeat(np.arange(E), counts)
    np.random.default_rng(seed).shuffle(flat)
    return flat.reshape(-1, top_k).astype(np.int32)


def regimes(ids, E, stage, n, k, top_k, device=-1):
    """The regimes one case reaches, from the plan and group_ref."""
    bm, _, bound, tiles_n, ks, _, _ = plan(stage, n, k, ids.shape[0], top_k, E=E, device=device)
    G = group_ref(ids, E, bm)
    rows = G.tiles[:G.n_tiles, 2]
    per_expert = np.bincount(G.tiles[:G.n_tiles, 0], minlength=E)
    assert bound == G.bound
    return {"single-row tile" if (rows == 1).any() else "", "full tile" if (rows == bm).any() else "",
            "three tiles of one expert" if (per_expert >= 3).any() else "", "expert without a pair" if (G.count == 0).any() else "",
            "idle workgroups" if G.bound > G.n_tiles else "", "several n tiles" if tiles_n > 1 else "",
            "one super-tile per step" if ks == 1 else "two super-tiles per step"}


WANTED = {"single-row tile", "full tile", "three tiles of one expert", "expert without a pair", "idle workgroups", "several n tiles",
          "one super-tile per step", "two super-tiles per step"}


def assert_regimes_reached(cases, device=-1):
    """cases: (ids, E, stage, n, k, top_k)."""
    seen = set()
    for c in cases:
        seen |= regimes(*c, device=device)
    assert not WANTED - seen, f"regimes not reached: {WANTED - seen}"
