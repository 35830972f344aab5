"""GPU suite (-m gpu): w4_gemm_tile_kernel (w4_gemm_tile.cuh, launched from tg_tile.hip) and tile_split_sum_kernel -- the GEMM of every
4-bit call with more than 64 activation rows (from 17 with a workspace) and of tg_gemm_w8 from 17 -- under the project's GEMM contract at the
smallest shapes that reach every regime of its tiles, step widths, splits, rings and table buffers (tests/tile_ref.py states the contract,
restates the launch plan and holds the case tables; tests/test_tile_ref_cpu.py proves on the CPU that the checks pass a correct twin and
fail every mutant).  Every case asserts the restated plan -- for this device's CU count -- as its precondition.

  1  the float64 bound on random data, the padded rows' zeros, the fused bias's bits on the direct and on the split-sum store, every split
     case again without a workspace (unsplit)
  2  exact probes on one representative per (words, tile shape, KS, split or not) class and on the 128 x 128 tile: one-hot weights over every
     column class, one-hot activations over both ends of every group, placement of every output of a ragged launch, decoys in the padded
     rows and behind x, inf / NaN placement
  3  two calls and a captured-graph replay of a split launch (two kernels) give the same bits

The C ABI is driven directly: a workspace of exactly the queried size (= splits m wrows 4, asserted) filled with 0xff, a patterned guard
behind it, y at the front of a larger patterned buffer; after every call both guards are intact.

Figures of one run on an MI355X (worst |y - y64| / allowance per case): profiles/tile_f64_checks.txt.
"""
import ctypes
import os

import pytest
import torch

from tests import tile_ref as R
from tests.test_gpu_parity import DEV, T  # noqa: F401  (T is a fixture)

pytestmark = pytest.mark.gpu

RESULTS = []  # (case id and regime, worst |y - y64| / allowance): written to $TILE_F64_REPORT when the module is done
Y_SENTINEL, WS_GUARD, GUARD_BYTES = 0x5A5A, 0xA5, 4096


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TILE_F64_REPORT")
    if path:
        with open(path, "w") as f:
            for cid, ratio in RESULTS:
                f.write(f"gpu  {cid:100s} {ratio:.3f}\n")


@pytest.fixture(scope="module")
def cus(T):
    return torch.cuda.get_device_properties(0).multi_processor_count


class Call:
    """One tg_gemm_w4 / tg_gemm_w8 call on the problem P, set up once: launch() may run many times (and inside a graph capture),
    finish() synchronises, checks the guards and returns y [m][wrows] on the CPU."""

    def __init__(self, T, P, cus, bias=None, workspace=True):
        from any4_amd import _lib

        self.L, self.P = _lib.load(), P
        d = lambda t: None if t is None else t.to(DEV)
        int8 = P.kind == "w8"
        if P.packed is None:
            codes = P.codes.to(DEV)
            if int8:
                P.packed = T.convert_matrix_to_m16n8k16_Bint8_layout(codes, 2) if P.side == "B" else T.convert_matrix_to_m16n8k16_Aint8_layout(codes, 2)
                rows = P.packed.shape[0] * (8 if P.side == "B" else 16)
            else:
                if P.side == "A":   # native weights-on-the-left words: the Bint4 tensor of the rows padded to 16 (tg_w4_gemm.w_format = TG_WFMT_ROWS)
                    codes = torch.cat([codes, torch.zeros(P.wrows - codes.shape[0], P.k, dtype=torch.int32, device=DEV)])
                P.packed = T.convert_matrix_to_m16n8k16_Bint4_layout(codes, 4)
                rows = P.packed.shape[0] * 8
            assert rows == P.wrows, (rows, P.wrows)
        behind = getattr(P, "x_behind", None)
        self.x = d(P.x if behind is None else torch.cat([P.x, behind]))
        self.q, self.lut, self.bias = d(P.qinfo.contiguous()), d(P.lut), d(bias)
        self.ybuf = torch.full((P.m * P.wrows + GUARD_BYTES // 2,), Y_SENTINEL, dtype=torch.int16, device=DEV)
        a = _lib.W4Gemm(x=self.x.data_ptr(), w=P.packed.data_ptr(), qinfo=self.q.data_ptr(), lut=(self.lut.data_ptr() if self.lut is not None else None),
                        y=self.ybuf.data_ptr(), m=P.m, wrows=P.wrows, k=P.k, group=P.g, qtype=_lib.TG_Q_INT8 if int8 else R.QT[P.qtype],
                        dtype=_lib.TG_BF16 if P.dtype == R.BF16 else _lib.TG_F16, w_on_right=1 if P.side == "B" else 0, inner_k_tiles=2 if int8 else 4, batch=1,
                        numerics=_lib.TG_NUM_REFERENCE, bias=(self.bias.data_ptr() if bias is not None else None),
                        w_format=_lib.TG_WFMT_ROWS if not int8 and P.side == "A" else _lib.TG_WFMT_M16N8K16)
        self.args, self.entry = a, (self.L.tg_gemm_w8 if int8 else self.L.tg_gemm_w4)
        plan = R.tile_plan(P.m, P.wrows, P.k, P.g, P.qtype, cus, workspace, int8, P.side == "B", P.dtype)
        assert plan is not None, "the tile GEMM declines this call"
        self.need, self.ws = 0, None
        if workspace:
            self.need = (self.L.tg_gemm_w8_workspace_bytes if int8 else self.L.tg_gemm_w4_workspace_bytes)(ctypes.byref(a))
            assert self.need == (plan[3] * P.m * P.wrows * 4 if plan[3] > 1 else 0), (self.need, plan)   # the restated split is the library's
            if self.need:
                self.ws = torch.empty(self.need + GUARD_BYTES, dtype=torch.uint8, device=DEV)
                self.ws[:self.need] = 0xff      # NaN bit patterns: nothing may be read that the call did not write first
                self.ws[self.need:] = WS_GUARD
                a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.need
        if not int8:
            assert self.L.tg_gemm_w4_plan(ctypes.byref(a), 0) == _lib.TG_PLAN_TILE

    def launch(self):
        from any4_amd import _lib

        _lib.check(self.entry(ctypes.byref(self.args), 0, torch.cuda.current_stream().cuda_stream), "tile GEMM")

    def finish(self):
        torch.cuda.synchronize()
        P, n = self.P, self.P.m * self.P.wrows
        assert bool((self.ybuf[n:] == Y_SENTINEL).all()), "the call wrote behind y"
        if self.ws is not None:
            assert bool((self.ws[self.need:] == WS_GUARD).all()), "the call wrote behind its workspace"
        return self.ybuf[:n].cpu().view(P.dtype).view(P.m, P.wrows)


class Op:
    """The C ABI behind tile_ref's gemm(P, bias=None, workspace=True)."""

    def __init__(self, T, cus):
        self.T, self.cus = T, cus

    def __call__(self, P, bias=None, workspace=True):
        call = Call(self.T, P, self.cus, bias, workspace)
        call.launch()
        return call.finish()


@pytest.fixture(scope="module")
def op(T, cus):
    return Op(T, cus)


def _cases(fn):
    """The tables are made for 256 CUs at collection (the ids); the test takes the same row made for the device's CU count."""
    return pytest.mark.parametrize("i", range(len(fn(256))), ids=[R.case_id(c) for c in fn(256)])


@_cases(R.cases)
def test_tile_float64(op, oracle, cus, i):
    R.check_f64(op, oracle, R.cases(cus)[i], cus, RESULTS)


@_cases(R.probe_cases)
def test_tile_selection_probe(op, cus, i):
    R.check_select(op, R.probe_cases(cus)[i], cus)


@_cases(R.probe_cases)
def test_tile_onehot_probe(op, oracle, cus, i):
    R.check_onehot(op, oracle, R.probe_cases(cus)[i], cus)


@_cases(R.group_cases)
def test_tile_onehot_probe_where_the_table_buffer_turns(op, oracle, cus, i):
    R.check_onehot(op, oracle, R.group_cases(cus)[i], cus)


@_cases(R.placement_cases)
def test_tile_placement_probe(op, cus, i):
    R.check_placement(op, R.placement_cases(cus)[i], cus)


@_cases(R.probe_cases)
def test_tile_decoys_and_nonfinite(op, oracle, cus, i):
    c = R.probe_cases(cus)[i]
    R.check_decoy(op, c, cus)
    R.check_nonfinite(op, oracle, c, cus)


def test_tile_split_launch_replays_the_same_bits(T, cus):
    """A split launch is two kernels on one stream (the tile kernel's f32 partial tiles, then tile_split_sum_kernel): two eager calls and
    a captured-graph replay give the same bits, with and without a fused bias."""
    c = next(c for c in R.cases(cus) if c.want == (128, 64, 2, 4, 9))
    assert R.assert_regime(c, cus)[3] == 4
    P = R.problem(c, seed=8)
    for bias in (None, torch.randn(c.wrows, generator=torch.Generator().manual_seed(5)).to(c.dtype)):
        first = Call(T, P, cus, bias)
        first.launch()
        eager = first.finish().clone()
        first.launch()
        assert R.bits_equal(first.finish(), eager), "two calls differ"
        call = Call(T, P, cus, bias)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call.launch()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        call.ybuf[:c.m * c.wrows] = Y_SENTINEL
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call.launch()
        graph.replay()
        assert R.bits_equal(call.finish(), eager), "the replayed graph differs from the eager call"


def test_tile_regimes_reached_are_the_regimes_wanted(cus):
    """On this device's CU count: the restated plan of every case lands in the regime the table writes next to it, and no regime is missing."""
    print("\n".join(str(r) for r in sorted(R.assert_regimes_reached(R.cases(cus), cus))))
