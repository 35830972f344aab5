"""CPU suite: the float64 definition of the fused k-means kernel (any4_amd/quantize.py: lloyd_rows_ref) against today's quantizer
(kmeans_rows), its fixed-point properties, exact probes on a dyadic grid under two orders of the prefix summation, and the host side
of tg_kmeans_rows / tg_kmeans_rows_plan (include/tinygemm_hip.h): symbols, refusals, the Python flag's refusals."""
import ctypes
import os
import re

import pytest
import torch

from any4_amd import _lib
from any4_amd import quantize as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDINGS = ("uniform", "density", "quantile")
E_NULL, E_SHAPE, E_ALIGN, E_SIZE = -1, -7, -8, -10


def prep_weights(x, sample_weight):
    """kmeans_rows' own preparation: abs, broadcast, clamp_min(1e-12)."""
    if sample_weight is None:
        return None
    rows, k = x.shape
    w = sample_weight.float().abs()
    w = (w.reshape(1, k).expand(rows, k) if w.dim() == 1 else w.reshape(rows, k)).contiguous()
    return w.clamp_min(1e-12)


def seeds(x, C, kinds=SEEDINGS):
    """[S][rows][C]: the unchanged _init_centers, as kmeans_rows calls it."""
    xs = torch.sort(x, dim=1).values
    lo = xs[:, :1]
    span = (xs[:, -1:] - lo).clamp_min(1e-12)
    return torch.stack([Q._init_centers(kind, x, xs, lo, span, C).expand(x.shape[0], C) for kind in kinds]).contiguous()


def best_of(results):
    """kmeans_rows' rule: keep the seeding with the strictly smallest SSE, in order."""
    a, c, sse, _ = results[0]
    a, c, sse = a.clone(), c.clone(), sse.clone()
    for a2, c2, s2, _ in results[1:]:
        better = s2 < sse
        a, c, sse = torch.where(better[:, None], a2, a), torch.where(better[:, None], c2, c), torch.where(better, s2, sse)
    return a, c, sse


def weighted_sse(x, w, a, c):
    wd = torch.ones_like(x, dtype=torch.float64) if w is None else w.double()
    return ((x.double() - c.double().gather(1, a.long())) ** 2 * wd).sum(1)


def check_fixed_point(x, w, a, c, mean_tol=1e-6):
    """The three properties kmeans_rows is tested for: ascending centres, every point (within 1e-6 span) at its nearest centre,
    every centre of a non-empty cluster the weighted mean of its points."""
    rows, k = x.shape
    C = c.shape[1]
    xd, cd = x.double(), c.double()
    wd = torch.ones_like(xd) if w is None else w.double()
    assert bool((cd[:, 1:] >= cd[:, :-1]).all())
    span = (xd.amax(1) - xd.amin(1)).clamp_min(1e-12)
    d_own = (xd - cd.gather(1, a.long())).abs()
    d_min = (xd[:, :, None] - cd[:, None, :]).abs().amin(2)
    assert bool((d_own <= d_min + 1e-6 * span[:, None]).all())
    cnt = torch.zeros(rows, C, dtype=torch.float64).scatter_add_(1, a.long(), wd)
    tot = torch.zeros(rows, C, dtype=torch.float64).scatter_add_(1, a.long(), xd * wd)
    has = cnt > 0
    dev = ((tot / cnt.clamp_min(1e-300) - cd).abs() / span[:, None])[has]
    assert float(dev.max()) <= mean_tol, float(dev.max())
    return float(dev.max())


@pytest.fixture(scope="module")
def random_case():
    torch.manual_seed(6)
    x = Q.group_q(torch.randn(64, 2048), 4, 128)[0]
    sw = torch.rand(2048) ** 4 + 1e-3
    return x, sw


def grid_case(rows, k, weights, seed):
    """Inputs on a dyadic grid: x = integers in [0, 15 * 1024] / 1024, w = integers in [1, 256] / 16.  At k <= 16384 every f64 sum of
    w and of x w stays below 2^53 units of its grid (2^-4, 2^-14) and is exact, whatever the order."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 15 * 1024 + 1, (rows, k), generator=g).float() / 1024
    if weights == "none":
        return x, None
    shape = (k,) if weights == "shared" else (rows, k)
    return x, torch.randint(1, 257, shape, generator=g).float() / 16


# ---------------------------------------------------------------- the reference against today's quantizer

@pytest.mark.parametrize("weighted", [False, True])
def test_reference_matches_kmeans_rows(random_case, weighted):
    x, sw = random_case
    sw = sw if weighted else None
    w = prep_weights(x, sw)
    c0 = seeds(x, 16)
    results = []
    for s, kind in enumerate(SEEDINGS):
        res = Q.lloyd_rows_ref(x, w, c0[s], 300, 1e-6)
        results.append(res)
        a_t, c_t = Q.kmeans_rows(x, 16, sample_weight=sw, init=kind)
        sse_t = weighted_sse(x, w, a_t, c_t)
        rel = ((res[2] - sse_t).abs() / sse_t).max().item()
        print(f"{kind} weighted={weighted}: per-row SSE vs kmeans_rows, max relative {rel:.3e}; iters mean {res[3].float().mean():.1f} max {int(res[3].max())}")
        assert rel <= 2e-3
        assert res[0].dtype == torch.int32 and res[1].dtype == torch.float32 and res[2].dtype == torch.float64 and res[3].dtype == torch.int32
        assert int(res[3].min()) >= 1 and int(res[3].max()) <= 300
    a_t, c_t = Q.kmeans_rows(x, 16, sample_weight=sw)
    sse_t = weighted_sse(x, w, a_t, c_t)
    _, _, sse_b = best_of(results)
    assert ((sse_b - sse_t).abs() / sse_t).max().item() <= 2e-3


@pytest.mark.parametrize("weighted", [False, True])
def test_reference_fixed_point_properties(random_case, weighted):
    x, sw = random_case
    w = prep_weights(x, sw if weighted else None)
    for c0 in seeds(x, 16):
        a, c, sse, _ = Q.lloyd_rows_ref(x, w, c0, 300, 1e-6)
        check_fixed_point(x, w, a, c)
        assert torch.allclose(sse, weighted_sse(x, w, a, c), rtol=1e-5)


def test_reference_recovers_few_distinct_values():
    torch.manual_seed(0)
    vals = torch.randn(7, 5)
    x = vals.repeat(1, 40)[:, torch.randperm(200)]
    for c0 in seeds(x, 16):
        a, c, sse, _ = Q.lloyd_rows_ref(x, None, c0, 300, 1e-6)
        assert torch.equal(c.gather(1, a.long()), x)
        assert float(sse.max()) == 0.0


def test_reference_one_cluster_is_the_weighted_mean():
    x = torch.tensor([[0.0, 1.0]])
    a, c, _, it = Q.lloyd_rows_ref(x, torch.tensor([[9.0, 1.0]]), torch.tensor([[0.5]]), 300, 1e-6)
    assert abs(float(c[0, 0]) - 0.1) < 1e-7 and a.tolist() == [[0, 0]] and int(it[0]) >= 1


def test_reference_rows_stop_on_their_own():
    """A row that has converged is left alone while another goes on (and the count of its iterations says so)."""
    x, _ = grid_case(2, 512, "none", 3)
    x[0] = torch.arange(16).repeat(32).float()   # converges at once from a uniform seeding
    c0 = seeds(x, 16, ("uniform",))[0]
    _, _, _, it = Q.lloyd_rows_ref(x, None, c0, 300, 1e-6)
    assert int(it[0]) < int(it[1])


# ---------------------------------------------------------------- exact probes: the order of the prefix summation cannot matter

@pytest.mark.parametrize("rows,k,weights,C", [(8, 1024, "rows", 16), (5, 300, "shared", 16), (3, 8, "none", 16), (2, 16384, "shared", 16),
                                              (40, 128, "none", 2), (6, 777, "rows", 1)])
def test_reference_exact_under_two_prefix_orders(rows, k, weights, C):
    x, sw = grid_case(rows, k, weights, 100 + k)
    w = prep_weights(x, sw)
    for s, c0 in enumerate(seeds(x, C)):
        a1, c1, s1, i1 = Q.lloyd_rows_ref(x, w, c0, 300, 1e-6, prefix="sequential")
        a2, c2, s2, i2 = Q.lloyd_rows_ref(x, w, c0, 300, 1e-6, prefix="blocked")
        assert torch.equal(a1, a2) and torch.equal(c1, c2) and torch.equal(i1, i2), SEEDINGS[s]
        assert torch.allclose(s1, s2, rtol=1e-12, atol=0)


# ---------------------------------------------------------------- host side

def test_symbols_declared_exported_bound():
    hdr = open(os.path.join(ROOT, "include", "tinygemm_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("tg_kmeans_rows", "tg_kmeans_rows_plan"):
        assert re.search(r"TG_API\s+int\s+" + s + r"\s*\(", hdr) and hasattr(lib, s) and s in _lib.SYMBOLS
    assert _lib.load().tg_abi_version() == _lib.TG_ABI_VERSION == 10
    assert re.search(r"#define\s+TG_ABI_VERSION\s+10\b", hdr)


def plan(rows, k, C, S, max_iter=300, tol=1e-6, weighted=1):
    out = (ctypes.c_int64 * 2)(-1, -1)
    rc = _lib.load().tg_kmeans_rows_plan(rows, k, C, S, max_iter, tol, weighted, out)
    return rc, out[0], out[1]


def test_plan_answers_without_a_gpu():
    rc, grid, lds = plan(1100, 128, 16, 3)
    assert rc == 0 and grid == 1100 and 0 < lds < 8 * 1024
    rc, grid, lds = plan(2, 16384, 16, 3, weighted=1)       # the cap, with weights: the row, its weights and the block prefixes
    assert rc == 0 and grid == 2 and 2 * 16384 * 4 + 8 * 1024 <= lds <= 160 * 1024
    rc, _, lds_u = plan(2, 16384, 16, 3, weighted=0)
    assert rc == 0 and lds_u < lds
    rc, _, lds_p = plan(2, 14336, 16, 3, weighted=1)        # padded to the next power of two for the sorting network
    assert rc == 0 and lds_p == lds
    assert plan(0, 128, 16, 3)[:2] == (0, 0)
    assert _lib.load().tg_kmeans_rows_plan(4, 128, 16, 3, 300, 1e-6, 1, None) == E_NULL


REFUSALS = [
    (dict(k=0), E_SHAPE), (dict(k=16385), E_SIZE), (dict(C=0), E_SHAPE), (dict(C=17), E_SHAPE), (dict(S=0), E_SHAPE), (dict(S=5), E_SHAPE),
    (dict(rows=-1), E_SHAPE), (dict(max_iter=0), E_SHAPE), (dict(max_iter=10001), E_SHAPE), (dict(tol=-1.0), E_SHAPE),
    (dict(tol=float("nan")), E_SHAPE),
]


@pytest.mark.parametrize("change,code", REFUSALS)
def test_refusals_through_plan_and_launch(change, code):
    base = dict(rows=4, k=128, C=16, S=3, max_iter=300, tol=1e-6)
    a = {**base, **change}
    assert plan(a["rows"], a["k"], a["C"], a["S"], a["max_iter"], a["tol"])[0] == code
    fake = 0x10000  # aligned, never dereferenced: the call is refused before any HIP call
    lib = _lib.load()
    rc = lib.tg_kmeans_rows(fake, fake, a["k"], fake, fake, fake, fake, fake, a["rows"], a["k"], a["C"], a["S"], a["max_iter"], a["tol"], -1, None)
    assert rc == code
    assert lib.tg_error_string(rc).decode() not in ("ok", "unknown tinygemm error")


def test_launch_refuses_pointers_and_strides():
    lib, fake = _lib.load(), 0x10000

    def call(x=fake, w=fake, ws=128, c0=fake, assign=fake, centers=fake, sse=fake, iters=fake, rows=4):
        return lib.tg_kmeans_rows(x, w, ws, c0, assign, centers, sse, iters, rows, 128, 16, 3, 300, 1e-6, -1, None)

    for name in ("x", "c0", "assign", "centers"):
        assert call(**{name: 0}) == E_NULL, name
    for name in ("x", "w", "c0", "assign", "centers", "iters"):
        assert call(**{name: fake + 2}) == E_ALIGN, name
    assert call(sse=fake + 4) == E_ALIGN
    assert call(ws=64) == E_SHAPE                      # a row stride that is neither k nor 0
    assert call(rows=0, x=0, c0=0, assign=0, centers=0, sse=0, iters=0) == 0   # no rows: success, nothing launched
    assert plan(4, 16384, 16, 3)[0] == 0 and plan(4, 16385, 16, 3)[0] == E_SIZE


def test_fused_flag_refuses_before_a_launch():
    x = torch.randn(4, 128)
    with pytest.raises(ValueError, match="GPU only"):
        Q.kmeans_rows(x, fused=True)
    with pytest.raises(ValueError, match="GPU only"):
        Q.anyq_quantize_tensor(x.to(torch.bfloat16), fused=True)
    bad = x.clone()
    bad[1, 3] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        Q.kmeans_rows(bad, fused=True)
    with pytest.raises(ValueError, match="n_clusters"):
        Q.kmeans_rows(x, n_clusters=17, fused=True)
    with pytest.raises(ValueError, match="16384"):
        Q.kmeans_rows(torch.zeros(1, 16385), fused=True)
    with pytest.raises(ValueError, match="16384"):
        Q.anyq_quantize_tensor(torch.randn(256, 128).to(torch.bfloat16), per_row=False, fused=True)   # one row of 32768 weights
    with pytest.raises(ValueError, match="return_stats"):
        Q.kmeans_rows(x, return_stats=True)
    a, c = Q.kmeans_rows(x)   # the default is the torch path, as before
    assert a.shape == (4, 128) and c.shape == (4, 16)
