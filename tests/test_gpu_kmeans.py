"""GPU suite: the fused k-means kernel (any4_amd/csrc/kmeans.cuh, tg_kmeans_rows) against its float64 definition
(any4_amd/quantize.py: lloyd_rows_ref).

Exact probes: on inputs on a dyadic grid (tests/test_kmeans_cpu.py: grid_case) every f64 sum is exact, so kernel and reference must
agree in every bit of the assignment, the centres and the iteration count, whatever the order of the kernel's prefix summation; the
SSE is a sum of k rounded terms in another order: 1e-10 relative (the bound for reordering k <= 16384 non-negative f64 terms is about
k * 2^-53 = 2e-12).  Random data: per-row SSE within the project's rtol = 2e-3 and the fixed-point properties on the kernel's own output.
Figures of one run on an MI355X: profiles/kmeans_f64_checks.txt (written to $KMEANS_F64_REPORT when the module is done).
"""
import copy
import os

import numpy as np
import pytest
import torch

from any4_amd import quantize as Q
from tests.conftest import bits16, from_bits16, load_golden
from tests.test_kmeans_cpu import SEEDINGS, best_of, check_fixed_point, grid_case, prep_weights, seeds, weighted_sse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESULTS = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("KMEANS_F64_REPORT")
    if path:
        with open(path, "w") as f:
            for cid, what, val in RESULTS:
                f.write(f"gpu  {cid:60s} {what:46s} {val:.3e}\n")


def launch(x, sw, c0, max_iter=300, tol=1e-6):
    """x, sw ([k] shared / [rows][k] / None, prepared), c0 on the CPU -> the kernel's four outputs on the CPU."""
    out = Q.kmeans_rows_launch(x.to(DEV), None if sw is None else sw.to(DEV), c0.to(DEV), max_iter, tol)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def prepared(sw):
    return None if sw is None else sw.float().abs().clamp_min(1e-12)


def assert_exact(got, ref, cid):
    a, c, sse, it = got
    ar, cr, sser, itr = ref
    assert torch.equal(a, ar), cid
    assert torch.equal(c.view(torch.int32), cr.view(torch.int32)), cid
    assert torch.equal(it, itr), cid
    dev = ((sse - sser).abs() / sser.clamp_min(1e-300)).max().item() if float(sser.max()) > 0 else float((sse - sser).abs().max())
    RESULTS.append((cid, "SSE vs f64 reference, max relative", dev))
    assert bool(((sse - sser).abs() <= 1e-10 * sser).all()), (cid, dev)


SHAPES = [(8, 1024, "rows"), (5, 300, "shared"), (3, 8, "none"), (2, 14336, "shared"), (2, 16384, "shared"), (1100, 128, "none")]


@pytest.mark.parametrize("C", [1, 2, 16])
@pytest.mark.parametrize("rows,k,weights", SHAPES)
def test_exact_probes(rows, k, weights, C):
    x, sw = grid_case(rows, k, weights, 7 * k + C)
    w = prep_weights(x, sw)
    for s, c0 in enumerate(seeds(x, C)):
        ref = Q.lloyd_rows_ref(x, w, c0, 300, 1e-6)
        assert_exact(launch(x, prepared(sw), c0), ref, f"exact {rows}x{k} {weights} C={C} {SEEDINGS[s]}")


def test_best_of_three_seedings():
    x, sw = grid_case(16, 1024, "rows", 11)
    c0 = seeds(x, 16)
    singles = [launch(x, prepared(sw), c0[s]) for s in range(3)]
    a, c, sse, it = launch(x, prepared(sw), c0)
    ab, cb, sb = best_of(singles)
    assert torch.equal(a, ab) and torch.equal(c, cb)          # the strictly smallest SSE, in order: kmeans_rows' rule
    for r in range(x.shape[0]):
        assert any(torch.equal(a[r], s_[0][r]) and torch.equal(c[r], s_[1][r]) for s_ in singles)
    smallest = torch.stack([s_[2] for s_ in singles]).amin(0)
    assert bool(((sse - smallest).abs() <= 1e-10 * smallest).all())
    assert torch.equal(it, singles[0][3] + singles[1][3] + singles[2][3])


@pytest.fixture(scope="module")
def random_case():
    torch.manual_seed(6)
    x = Q.group_q(torch.randn(64, 2048), 4, 128)[0]
    return x, torch.rand(2048) ** 4 + 1e-3


@pytest.mark.parametrize("weighted", [False, True])
def test_random_data(random_case, weighted):
    x, sw = random_case
    sw = sw if weighted else None
    w = prep_weights(x, sw)
    a, c, sse, it = (t.cpu() for t in Q.kmeans_rows(x.to(DEV), 16, sample_weight=sw, fused=True, return_stats=True))
    c0 = seeds(x, 16)
    _, _, sse_ref = best_of([Q.lloyd_rows_ref(x, w, c0[s], 300, 1e-6) for s in range(3)])
    rel = ((sse - sse_ref).abs() / sse_ref).max().item()
    cid = f"random 64x2048 {'weighted' if weighted else 'unweighted'}"
    RESULTS.append((cid, "per-row SSE vs f64 reference, max relative", rel))
    assert rel <= 2e-3
    assert torch.allclose(sse, weighted_sse(x, w, a, c), rtol=1e-5)
    RESULTS.append((cid, "centre vs weighted mean of its cluster / span", check_fixed_point(x, w, a, c)))
    RESULTS.append((cid, "iterations, mean over rows (3 seedings)", it.float().mean().item()))
    RESULTS.append((cid, "iterations, max over rows (3 seedings)", float(it.max())))
    # ... and the same quantizer as today's torch path
    a_t, c_t = Q.kmeans_rows(x.to(DEV), 16, sample_weight=sw)
    sse_t = weighted_sse(x, w, a_t.cpu(), c_t.cpu())
    assert ((sse - sse_t).abs() / sse_t).max().item() <= 2e-3


def test_few_distinct_values_are_reproduced():
    torch.manual_seed(0)
    x5 = torch.randn(7, 5).repeat(1, 40)[:, torch.randperm(200)]
    g = torch.Generator().manual_seed(1)
    x16 = torch.stack([torch.linspace(-8, 7, 16).repeat(8)[torch.randperm(128, generator=g)] for _ in range(9)])
    for x in (x5, x16):
        a, c = Q.kmeans_rows(x.to(DEV), 16, fused=True)
        assert torch.equal(c.cpu().gather(1, a.cpu().long()), x)
        for c0 in seeds(x, 16):
            got = launch(x, None, c0)
            assert torch.equal(got[1].gather(1, got[0].long()), x) and float(got[2].max()) == 0.0


@pytest.mark.parametrize("weights", ["none", "rows"])
def test_empty_clusters_are_reseeded_as_in_the_reference(weights):
    """Two far outliers stretch the row's range, so the uniform seeding leaves most clusters without a point."""
    x, sw = grid_case(6, 512, weights, 21)
    x = x / 16                     # the bulk in [0, 15/16] ...
    x[:, 5], x[:, 300] = 15.0, -12.0   # ... and the outliers (still on the 2^-14 grid)
    w = prep_weights(x, sw)
    c0 = seeds(x, 16, ("uniform",))[0]
    mid = (c0[:, 1:] + c0[:, :-1]) * 0.5
    assert int((torch.bincount(torch.searchsorted(mid[0].contiguous(), x[0].contiguous()), minlength=16) == 0).sum()) >= 8
    ref = Q.lloyd_rows_ref(x, w, c0, 300, 1e-6)
    assert_exact(launch(x, prepared(sw), c0), ref, f"empty clusters 6x512 {weights}")
    # fewer iterations than it takes to converge: the re-seeded centres themselves are compared
    for n_it in (1, 2, 3):
        assert_exact(launch(x, prepared(sw), c0, max_iter=n_it), Q.lloyd_rows_ref(x, w, c0, n_it, 1e-6), f"empty clusters, {n_it} iterations {weights}")


def test_two_launches_give_the_same_bits(random_case):
    x, sw = random_case
    xd, swd = x.to(DEV), sw.to(DEV)
    r1 = Q.kmeans_rows(xd, 16, sample_weight=swd, fused=True, return_stats=True)
    r2 = Q.kmeans_rows(xd, 16, sample_weight=swd, fused=True, return_stats=True)
    for t1, t2 in zip(r1, r2):
        assert torch.equal(t1.view(torch.int32) if t1.dtype != torch.float64 else t1.view(torch.int64),
                           t2.view(torch.int32) if t2.dtype != torch.float64 else t2.view(torch.int64))


def test_fused_flag_refuses_on_the_gpu():
    x = torch.randn(4, 128, device=DEV)
    with pytest.raises(ValueError, match="n_clusters"):
        Q.kmeans_rows(x, n_clusters=17, fused=True)
    with pytest.raises(ValueError, match="16384"):
        Q.anyq_quantize_tensor(torch.randn(256, 128, device=DEV).to(torch.bfloat16), per_row=False, fused=True)
    bad = x.clone()
    bad[0, 0] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        Q.kmeans_rows(bad, fused=True)


def test_end_to_end_against_the_reference_fixture():
    d = load_golden("any4_n1024_k1024_g128_seed1234.npz")
    torch.manual_seed(1234)
    W = (torch.randn(1024, 1024) * 0.02).to(torch.bfloat16)
    c8 = d["codes_nib"]
    codes_ref = np.empty((1024, 1024), np.int32)
    codes_ref[:, 0::2], codes_ref[:, 1::2] = c8 & 15, c8 >> 4
    ref = Q.anyq_dequantize_tensor(torch.from_numpy(codes_ref), from_bits16(d["lut_bits"], torch.bfloat16), from_bits16(d["sz_bits"], torch.bfloat16))
    codes, lut, sz = Q.anyq_quantize_tensor(W.to(DEV), n_bit=4, q_group_size=128, per_row=True, fused=True)
    assert codes.is_cuda and codes.dtype == torch.int32 and int(codes.min()) >= 0 and int(codes.max()) <= 15 and lut.shape == (1024, 16)
    assert np.array_equal(bits16(sz.cpu()), d["sz_bits"])
    mine = Q.anyq_dequantize_tensor(codes, lut, sz).cpu()
    mse = lambda t: ((t.float() - W.float()) ** 2).mean().item()
    RESULTS.append(("end to end 1024x1024 g128", "reconstruction MSE / the reference's", mse(mine) / mse(ref)))
    assert mse(mine) <= 1.02 * mse(ref), (mse(mine), mse(ref))


def test_anyq_layer_fused_real_kernels_vs_pseudo():
    torch.manual_seed(4)
    lin = torch.nn.Linear(512, 256, bias=True, device=DEV, dtype=torch.bfloat16)
    x = torch.randn(5, 512, device=DEV).to(torch.bfloat16)
    q = Q.anyq_layer(copy.deepcopy(lin), name="lin", group_size=128, fused=True)
    assert type(q).__name__ == "Any4Linear" and q.weight_reshaped
    twin = Q.anyq_layer(copy.deepcopy(lin), name="lin", group_size=128, pseudo=True, fused=True)
    y_q, y_t = q(x).float(), twin(x).float()
    assert (y_q - y_t).abs().max() <= 0.02 * y_t.abs().max() + 1e-2
    assert (y_q - lin(x).float()).abs().max() <= 0.25 * lin(x).float().abs().max()
