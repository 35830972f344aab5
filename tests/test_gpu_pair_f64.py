"""GPU suite (-m gpu): the persistent pair-table family -- w4_gemm_pair_kernel in its instantiations, the lean m = 1 kernel, the two 16x16x32
layouts (any4_amd/csrc/w4_gemm_pair.cuh, tg_pair.hip) -- on batches of DIFFERENT problems: every case is one tg_gemm_w4 call through the C
ABI, every problem has its own weights, scale | zero words, LUT and activations, and every output of every problem is compared.

  * float64: |y - y64| <= 0.5 ulp16(y64) (1 + 2^-7) + 4e-6 S against the unrounded group-scaled sum (tests/pair_ref.py: ref64, bound), per
    regime of the plan (pair_ref.REQUIRED); pair_plan is asserted against tg_gemm_w4_plan_detail and tg_gemm_w4_workspace_bytes of that very call
  * exact probes on one case per kernel class: one weight per row, the zero point of one group per row, one-hot activation rows -- bit for bit
  * isolation: a NaN in one problem's activations, LUT or scale stays in that problem's outputs; 2^15 in padded rows changes no bit
  * y and the workspace sit between guard bands, y is prefilled with NaN and the workspace (exactly the queried bytes) with 0xff; two launches
    and a captured replay give the same bits; a fused bias is `y + bias` bit for bit; the lean kernel equals the general template
The benchmark's own shape stays in tests/test_gpu_fast.py.
"""
import ctypes
import functools

import pytest
import torch

from tests import pair_ref as R
from tests.test_gpu_parity import DEV, T  # noqa: F401  (T is a fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_weight_format")]  # (the Aint4 cases bring the reference's words)

GUARD = 4096      # bytes on each side of y and of the workspace
SENTINEL = 0x5A5A


def pack(T, bt):
    """[B][...] packed words of every problem: the rows of all problems as one matrix (n is a whole number of packed tiles)."""
    conv = T.convert_matrix_to_m16n8k16_Bint4_layout if bt.on_right else T.convert_matrix_to_m16n8k16_Aint4_layout
    step = max(1, (1 << 26) // (bt.n * bt.k))
    parts = [conv(bt.codes[lo:lo + step].reshape(-1, bt.k).to(DEV).int(), bt.inner) for lo in range(0, bt.B, step)]
    w = torch.cat(parts)
    return w.reshape(bt.B, w.shape[0] // bt.B, *w.shape[1:]).contiguous()


class Launch:
    """One tg_gemm_w4 call over the batch `bt`: the operands on the device, y (NaN inside, SENTINEL around) and the workspace (0xff, exactly
    the queried bytes, 0xff around).  w: the packed words of an earlier Launch of the same codes.  x_pad: rows of 2^15 behind row m - 1 of
    every problem's activations.  row_pad: as many rows of 2^15 behind row wrows - 1 of every problem's LUT and behind its last group's
    scale | zero words (the buffers of a 64-row block that the call's wrows does not fill)."""

    def __init__(self, T, bt, numerics="fast", w=None, x_pad=0, row_pad=0):
        from any4_amd import _lib

        self.L, self.bt = _lib.load(), bt
        self.w = pack(T, bt) if w is None else w
        x = bt.x if not x_pad else torch.cat([bt.x, torch.full((bt.B, x_pad, bt.k), 2.0 ** 15, dtype=bt.dtype)], dim=1)
        self.x = x.to(DEV).contiguous()
        self.q = (bt.exps if bt.qtype == "mx4" else torch.stack([bt.scale, bt.zero], dim=3)).to(DEV).contiguous()
        self.lut = None if bt.lut is None else bt.lut.to(DEV).contiguous()
        if row_pad:
            big = lambda t, tail: torch.cat([t.reshape(bt.B, -1), torch.full((bt.B, tail), 2.0 ** 15, dtype=bt.dtype)], dim=1).to(DEV).contiguous()
            self.q = big(torch.stack([bt.scale, bt.zero], dim=3), 2 * row_pad)
            self.lut = None if bt.lut is None else big(bt.lut, 16 * row_pad)
        self.bias = None if bt.bias is None else bt.bias.to(DEV).contiguous()
        g = GUARD // 2
        self.ybuf = torch.empty(2 * g + bt.B * bt.m * bt.n, dtype=torch.int16, device=DEV)
        self.y = self.ybuf[g:-g].view(bt.dtype).view(bt.B, bt.m, bt.n)
        a = _lib.W4Gemm(x=self.x.data_ptr(), w=self.w.data_ptr(), qinfo=self.q.data_ptr(), lut=None if self.lut is None else self.lut.data_ptr(),
                        y=self.y.data_ptr(), m=bt.m, wrows=bt.n, k=bt.k, group=bt.g, qtype=R.QT[bt.qtype],
                        dtype=_lib.TG_BF16 if bt.dtype == torch.bfloat16 else _lib.TG_F16, w_on_right=1 if bt.on_right else 0, inner_k_tiles=bt.inner,
                        batch=bt.B, stride_x=self.x.stride(0) * 2, stride_w=self.w.stride(0) * 4, stride_qinfo=self.q.stride(0) * self.q.element_size(),
                        stride_lut=0 if self.lut is None else self.lut.stride(0) * 2, stride_y=bt.m * bt.n * 2, numerics=R.NUMERICS[numerics],
                        bias=None if self.bias is None else self.bias.data_ptr(), stride_bias=0 if self.bias is None else self.bias.stride(0) * 2)
        self.need = self.L.tg_gemm_w4_workspace_bytes(ctypes.byref(a))
        assert self.need >= 0
        self.wsbuf = torch.empty(2 * GUARD + self.need, dtype=torch.uint8, device=DEV)
        if self.need:
            a.workspace, a.workspace_bytes = self.wsbuf.data_ptr() + GUARD, self.need
        self.args = a
        self.plan = (self.L.tg_gemm_w4_plan(ctypes.byref(a), 0), self.L.tg_gemm_w4_plan_detail(ctypes.byref(a), 0))

    def prefill(self):
        self.ybuf.fill_(SENTINEL)
        self.y.fill_(float("nan"))
        self.wsbuf.fill_(0xff)

    def call(self):
        from any4_amd import _lib

        _lib.check(self.L.tg_gemm_w4(ctypes.byref(self.args), 0, torch.cuda.current_stream().cuda_stream), "tg_gemm_w4")

    def run(self):
        """prefill, launch, check the guard bands; returns y [B][m][n] on the host."""
        self.prefill()
        self.call()
        torch.cuda.synchronize()
        g = GUARD // 2
        assert bool((self.ybuf[:g] == SENTINEL).all()) and bool((self.ybuf[-g:] == SENTINEL).all()), "written outside y"
        assert bool((self.wsbuf[:GUARD] == 0xff).all()) and bool((self.wsbuf[GUARD + self.need:] == 0xff).all()), "written outside the workspace"
        return self.y.cpu()


def assert_plan(launch, pp):
    """pair_plan as the precondition, against the library's answers for that very call."""
    from any4_amd import _lib

    assert pp.family == "pair", pp
    assert launch.plan == (_lib.TG_PLAN_PAIR, _lib.TG_PLAN_PAIR_M1_LEAN if pp.kernel == "lean" else _lib.TG_PLAN_PAIR), (launch.plan, pp.kernel)
    assert launch.need == pp.ws, (launch.need, pp.ws)


@functools.lru_cache(maxsize=1)
def reference(name):
    return R.ref64(R.case_batch(name))


def same_where_finite(a, b, what):
    """Equal bits; NaN where the other has NaN (payloads are not compared)."""
    na, nb = torch.isnan(a.float()), torch.isnan(b.float())
    assert torch.equal(na, nb), f"{what}: NaN in different places"
    R.assert_same_bits(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b), what)


# ---- float64, every problem, per regime -----------------------------------------------------------------------------------------------

def test_cases_reach_every_regime_on_this_device():
    R.assert_regimes_reached([R.case_plan(name) for name in R.CASE_NAMES])


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_every_problem_against_float64(T, name):
    c, bt, pp = R.case(name), R.case_batch(name), R.case_plan(name)
    launch = Launch(T, bt, c.numerics)
    assert_plan(launch, pp)
    y = launch.run()
    y64, S = reference(name)
    ratio = R.check_f64(y, y64, S, bt.dtype, name)
    print(f"PAIR_F64 {name}: {pp.kernel} NSG {pp.NSG} GPS {pp.GPS} ring {pp.ring} xg {int(pp.xg)} k {bt.k} items {pp.items}: worst error / bound {ratio:.4f}")
    same_where_finite(launch.run(), y, f"{name}: second launch")


def test_declined_instantiations_are_declined(T):
    """What launch_pair_m does not instantiate goes elsewhere: no workspace asked, not the lean kernel, and pair_plan says 'other'."""
    from any4_amd import _lib

    for m, g, qtype, inner in R.DECLINED:
        k = 16 * max(g, 128)
        assert R.pair_plan(m, 64, k, g, qtype, inner, True, 400).family == "other"
        fam, det, ws = R.lib_plan(m, 64, k, g, qtype, inner, True, 65536)
        assert fam not in (_lib.TG_PLAN_PAIR, _lib.TG_PLAN_PAIR_XR) and det == fam and ws == 0, (m, g, qtype, inner, fam)


def test_smallest_xg_k_is_read_off_the_plan(T):
    for m in (1, 8):
        k = R.smallest_xg_k(m)
        print(f"PAIR_F64 smallest XG k for m = {m}: {k}")
        assert R.lib_plan(m, 64, k, 128, "any4_rowwise", 4, True, 200)[2] > 0 and R.lib_plan(m, 64, k - 128, 128, "any4_rowwise", 4, True, 200)[2] == 0


# ---- exact probes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.PROBE_CASES)
def test_exact_probes(T, name):
    c, bt, pp = R.case(name), R.case_batch(name), R.case_plan(name)
    probes = [R.probe_one_weight, R.probe_one_hot] + ([] if bt.qtype == "mx4" else [R.probe_zero_point])
    for probe in probes:
        pb, want = probe(pp, bt)
        launch = Launch(T, pb, c.numerics)
        assert_plan(launch, pp)
        R.assert_same_bits(launch.run(), want, f"{name}: {probe.__name__}")


# ---- isolation ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lean rowwise 9 units rblocks 3", "lean global fp16 ranges of 5-6", "general m3 NSG 0 partial round", "xg m8", "la1 inner 4 m5",
                                  "la2 m13 inner 2"])
def test_a_nan_stays_in_its_problem_and_padding_is_not_read(T, name):
    from types import SimpleNamespace

    c, bt, pp = R.case(name), R.case_batch(name), R.case_plan(name)
    base = Launch(T, bt, c.numerics)
    assert_plan(base, pp)
    y0 = base.run()
    b, row = bt.B // 2, 3

    def poisoned(**kw):
        pb = SimpleNamespace(**vars(bt))
        for key, fn in kw.items():
            t = getattr(bt, key).clone()
            fn(t)
            setattr(pb, key, t)
        return pb

    def check(pb, what, x_pad=0):
        y = Launch(T, pb, c.numerics, w=base.w, x_pad=x_pad).run()
        nan = torch.isnan(torch.from_numpy(R.ref64(R.sub_batch(pb, b, b + 1))[0]))[0]
        assert torch.equal(torch.isnan(y[b].float()), nan), f"{name}: {what}: NaN of problem {b} not where the float64 product has it"
        keep = torch.ones(bt.B, dtype=torch.bool)
        keep[b] = False
        R.assert_same_bits(y[keep], y0[keep], f"{name}: {what}: another problem changed")
        R.assert_same_bits(torch.where(nan, torch.zeros_like(y[b]), y[b]), torch.where(nan, torch.zeros_like(y0[b]), y0[b]), f"{name}: {what}: problem {b} outside the NaN")

    def set_x(t):
        t[b, 0, 7] = float("nan")

    def set_scale(t):
        t[b, 1, row] = float("nan")

    def set_lut(t):  # one entry of a global LUT, the whole LUT row of one weight row
        if t.dim() == 2:
            t[b, 5] = float("nan")
        else:
            t[b, row, :] = float("nan")

    check(poisoned(x=set_x), "NaN activation")
    check(poisoned(scale=set_scale), "NaN scale")
    if bt.lut is not None:
        check(poisoned(lut=set_lut), "NaN LUT")
    # 2^15 behind row m - 1 of every problem's activations: not read
    y = Launch(T, bt, c.numerics, w=base.w, x_pad=1).run()
    R.assert_same_bits(y, y0, f"{name}: a row of 2^15 behind the activations")


def test_padded_rows_change_no_bit(T):
    """Rows of the tile padding INSIDE wrows (n = 40 with rows 36 ... 39 treated as the padding of 36 rows, the project's convention): 2^15 in
    their scales, zeros and LUT rows changes no bit of rows 0 ... 35.  And rows BEYOND wrows: the LUT and the scale | zero words of every
    problem are followed by 24 rows of 2^15 (rows 40 ... 63 of the last 64-row block), which a kernel that did not clamp its rows to
    wrows - 1 would read: no bit of any output changes."""
    from types import SimpleNamespace

    for name in ("m1 g64", "general m3 NSG 0 partial round", "la2 m13 inner 2"):
        c, bt, pp = R.case(name), R.case_batch(name), R.case_plan(name)
        assert bt.n == 40
        base = Launch(T, bt, c.numerics)
        y0 = base.run()
        pb = SimpleNamespace(**vars(bt))
        pb.scale, pb.zero, pb.lut = bt.scale.clone(), bt.zero.clone(), bt.lut.clone()
        pb.scale[:, :, 36:], pb.zero[:, :, 36:] = 2.0 ** 15, 2.0 ** 15
        if pb.lut.dim() == 3:
            pb.lut[:, 36:, :] = 2.0 ** 15
        y = Launch(T, pb, c.numerics, w=base.w).run()
        R.assert_same_bits(y[:, :, :36], y0[:, :, :36], f"{name}: padded rows inside wrows")
        beyond = Launch(T, bt, c.numerics, w=base.w, row_pad=24)
        assert_plan(beyond, pp)
        R.assert_same_bits(beyond.run(), y0, f"{name}: rows of 2^15 beyond wrows")


# ---- bias, lean against general, captured replay --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lean rowwise 9 units rblocks 3", "m1 g256 ring of four", "general m5 red_alias", "mx4 m8", "xg m8", "mfma m1", "la1 inner 4 m5",
                                  "la2 m13 inner 2"])
def test_fused_bias_is_y_plus_bias_bit_for_bit(T, name):
    from types import SimpleNamespace

    c, bt = R.case(name), R.case_batch(name)
    zero = SimpleNamespace(**{**vars(bt), "bias": torch.zeros(bt.B, bt.n, dtype=bt.dtype)})
    l0 = Launch(T, zero, c.numerics)
    pp = R.plan_of(zero, c.numerics)
    assert_plan(l0, pp)
    assert pp.kernel != "lean"
    y0 = l0.run()
    bias = R.random_bias(bt)
    y = Launch(T, SimpleNamespace(**{**vars(bt), "bias": bias}), c.numerics, w=l0.w).run()
    same_where_finite(y, (y0.float() + bias[:, None, :].float()).to(bt.dtype), f"{name}: fused bias")


@pytest.mark.parametrize("name", [n for n in R.CASE_NAMES if n.startswith("lean")])
def test_lean_kernel_equals_the_general_template(T, name):
    from types import SimpleNamespace

    bt, pp = R.case_batch(name), R.case_plan(name)
    lean = Launch(T, bt)
    assert_plan(lean, pp)
    assert pp.kernel == "lean"
    zero = SimpleNamespace(**{**vars(bt), "bias": torch.zeros(bt.B, bt.n, dtype=bt.dtype)})
    general = Launch(T, zero, w=lean.w)
    gp = R.plan_of(zero)
    assert_plan(general, gp)
    assert gp.kernel == "m1" and (gp.spw, gp.nl, gp.items) == (pp.spw, pp.nl, pp.items)
    assert torch.equal(lean.run().float(), general.run().float()), f"{name}: the lean kernel and the general template differ"


@pytest.mark.parametrize("name", ["lean rowwise 9 units rblocks 3", "xg m8", "la2 m13 inner 2"])
def test_captured_replay_gives_the_eager_bits(T, name):
    c, bt = R.case(name), R.case_batch(name)
    launch = Launch(T, bt, c.numerics)
    eager = launch.run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch.call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch.call()
    launch.prefill()
    graph.replay()
    torch.cuda.synchronize()
    R.assert_same_bits(launch.y.cpu(), eager, f"{name}: captured replay")
