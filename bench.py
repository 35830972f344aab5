#!/usr/bin/env python3
"""bench.py -- any4 W4A16 small-batch GEMM on MI355X: achieved GB/s against the HBM roofline.

Contract (one JSON line on rank 0):
    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Workload (BASELINE.json configs[1]): any4 (per-row 16-entry bf16 LUT, g = 128) W4A16 GEMV, m = 1,
n = k = 4096, weights packed on the B side with innerKTiles = 4 -- exactly what Any4Linear's default
kernel `linear_y_f16RM_x_f16RM_W_any4TC` runs, in the library's default numerics.  One STEP is one pass over a
batch of L = 512 independent such layers (distinct weights, activations and outputs: 4.6 GB, far beyond L2 +
Infinity Cache, so every step streams its weights from HBM; about the 4-bit weight volume of a Llama-3-8B
decode step) issued as ONE stacked launch of the C-ABI entry point tg_gemm_w4 (batch = L).  Inputs are
resident in HBM before the timed region.  Before the timed steps the GPU is kept under the same load for
~2 s of untimed steps (`settle_steps`): the power controller needs tens of ms to reach its steady clock
(DESIGN.md 5), and the run leaves a GPU footprint an external sampler can see.

`value` = algorithmic bytes of all ranks per step / max-over-ranks step time.
Algorithmic bytes per layer: n*k/2 + (k/g)*n*4 + 32*n + m*k*2 + m*n*2 = 9 060 352 B.

A plain run stops there: set-up, warm-up, the timed steps, the outputs (--dump-outputs DIR: the last timed step's
output as DIR/y.npy in float32, same inputs on every run with the same arguments) and the result line.
With --full, rank 0 then (a) checks three layers of the timed launch's output against the CPU oracle,
(b) times the other BASELINE configs as extra keys (m = 8; config 3 = m = 8, 8192^2, weights on the A side;
config 4 = int4 / nf4-style global LUT / mx4 at m = 1), (c) times single-layer launches (what one
Any4Linear.forward issues), (d) times the reference's CPU path on the host cores, (e) the decode leg, the
rocprofv3 PMC passes and (N > 1) the other exchanges and the weak-scaling protocol.

N > 1 (north_star / SURVEY.md 8e): ONE stack of L layers of n rows, row-sharded -- rank r owns rows
[r*n/N, (r+1)*n/N) of every layer (packed codes, LUT rows, scale/zero columns); the activations are
replicated; every step ends with ONE gather of the partial outputs of the whole layer batch, inside the
timed region (RCCL all_gather_into_tensor over xGMI; the one-shot peer-write gather of
include/peer_gather_hip.h timed beside it).  Total work is fixed as N grows -> "scaling": "strong";
`value` = algorithmic bytes of the WHOLE problem per step / max-over-ranks step time, `roofline` = the
per-rank kernel on its shard.  The weak-scaling protocol of rounds 1-5 (every rank its own n rows) stays
as the extra key `weak_scaling`.
--same-device / --dist-backend gloo: a dry run of the N > 1 path with every rank on GPU 0 (one-GPU boxes;
RCCL refuses two ranks on one device, so the exchange is then the peer-write gather over IPC).
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# the cpu_baseline legs use OpenMP / torch threads: without thread binding libgomp's workers pile onto a few cores
_SCHEDULABLE_CPUS = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)  # before binding
os.environ.setdefault("OMP_PROC_BIND", "true")

import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 measured float4 copy
QT = {"int4": 0, "any4_global": 1, "any4_rowwise": 2, "mx4": 3}


def alg_bytes(m, n, k, g, qtype="any4_rowwise"):
    """packed weights + quantisation info + LUT + activations + outputs."""
    lut = {"any4_rowwise": 32 * n, "any4_global": 32, "int4": 0, "mx4": 0}[qtype]
    q = n * k // g if qtype == "mx4" else (k // g) * n * 4
    return n * k // 2 + q + lut + m * k * 2 + m * n * 2


def physical_cores():
    """(physical cores, logical CPUs) of the host from /proc/cpuinfo; (None, n) if it cannot be read."""
    try:
        seen, phys, core = set(), None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    seen.add((phys, core))
                phys = core = None
        return (len(seen) or None), (os.cpu_count() or 1)
    except OSError:
        return None, (os.cpu_count() or 1)


def make_batch(L, m, n, k, g, inner, device, seed, qtype="any4_rowwise", on_right=True):
    """Synthetic tensors of the SURVEY 8d recipe, generated on the device (packed words are uniformly
    random nibbles, which is what packing uniformly random codes gives)."""
    gen = torch.Generator(device=device).manual_seed(seed)
    shape = (L, n // 8, k // (16 * inner), 32, inner // 2) if on_right else (L, n // 16, k // (16 * inner), 32, inner)
    w = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int64, device=device, generator=gen).to(torch.int32)
    x = torch.randn(L, m, k, device=device, generator=gen).to(torch.bfloat16)
    if qtype == "mx4":
        q = torch.randint(120, 131, (L, n, k // g), dtype=torch.uint8, device=device, generator=gen)
    else:
        scales = torch.rand(L, k // g, n, device=device, generator=gen) * 0.02 + 0.005
        zeros = torch.randn(L, k // g, n, device=device, generator=gen) * 0.01
        q = torch.stack([scales, zeros], dim=3).to(torch.bfloat16).contiguous()
    lut = {"any4_rowwise": lambda: torch.randn(L, n, 16, device=device, generator=gen).to(torch.bfloat16),
           "any4_global": lambda: torch.randn(L, 16, device=device, generator=gen).to(torch.bfloat16)}.get(qtype, lambda: None)()
    y = torch.empty(L, m, n, device=device, dtype=torch.bfloat16)
    return w, x, q, lut, y


def make_args(_lib, w, x, q, lut, y, m, n, k, g, qtype, on_right, inner, batch, numerics="fast", native=False):
    """native (weights on the left only): the A-shaped tensor holds the row-per-lane word order (tg_w4_gemm.w_format = TG_WFMT_ROWS,
    what convert_matrix_to_m16n8k16_Aint4_layout returns by default) instead of the reference's Aint4 words."""
    return _lib.W4Gemm(
        w_format=_lib.TG_WFMT_ROWS if (native and not on_right) else _lib.TG_WFMT_M16N8K16,
        x=x.data_ptr(), w=w.data_ptr(), qinfo=q.data_ptr(), lut=(lut.data_ptr() if lut is not None else None), y=y.data_ptr(),
        m=m, wrows=n, k=k, group=g, qtype=QT[qtype], dtype=_lib.TG_BF16, w_on_right=1 if on_right else 0,
        inner_k_tiles=inner, batch=batch, stride_x=x.stride(0) * 2, stride_w=w.stride(0) * 4,
        stride_qinfo=q.stride(0) * q.element_size(), stride_lut=(lut.stride(0) * 2 if lut is not None else 0),
        stride_y=y.stride(0) * 2, numerics={"fast": _lib.TG_NUM_FAST, "reference": _lib.TG_NUM_REFERENCE, "fast_mfma": _lib.TG_NUM_FAST_MFMA, "fast_dot2": _lib.TG_NUM_FAST_DOT2}[numerics])


def calibrate_x(run, x, y):
    """Scale the activations IN PLACE by a power of two (exact in bf16: every product, sum and rounding of the GEMM scales with it) so
    that the largest output lies in (0.95, 1.9]: where north_star's 1e-2 is quoted (the captured fixture: max|y| = 2.2) and one bf16
    output step is 7.8e-3.  `run` launches the GEMM once; returns the scale."""
    run()
    torch.cuda.synchronize()
    ymax = max(float(torch.nan_to_num(y.float(), nan=0.0, posinf=0.0, neginf=0.0).abs().max().item()), 1e-30)
    import math

    sc = 2.0 ** math.floor(math.log2(1.9 / ymax))
    x.mul_(sc)
    return sc


def attach_workspace(lib, aa, device):
    """The scratch tg_gemm_w4_workspace_bytes asks for (m > 1 at k = 4096: the activations are re-arranged once per launch
    for the pair-table kernel).  Allocated once, outside every timed region; the returned tensor keeps it alive."""
    need = lib.tg_gemm_w4_workspace_bytes(ctypes.byref(aa))
    if need < 0:
        raise SystemExit(f"bench.py: tg_gemm_w4_workspace_bytes failed with {need}")
    if need == 0:
        return None
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    aa.workspace, aa.workspace_bytes = ws.data_ptr(), need
    return ws


DUMP_CAP_BYTES = 48 << 20  # --dump-outputs stays under 64 MB


def dump_outputs(directory, y):
    """--dump-outputs: `y` (what a caller of the timed path receives) as float32 DIR/y.npy; larger than DUMP_CAP_BYTES, a fixed
    sample of its elements (seed 0, flat indices in increasing order) as DIR/y_sample.npy.  Returns {file name: shape}."""
    import numpy as np

    os.makedirs(directory, exist_ok=True)
    if y.numel() * 4 <= DUMP_CAP_BYTES:
        name, arr = "y", y.float().cpu().numpy()
    else:
        idx = np.sort(np.random.default_rng(0).choice(y.numel(), DUMP_CAP_BYTES // 4, replace=False))
        name, arr = "y_sample", y.reshape(-1)[torch.from_numpy(idx).to(y.device)].float().cpu().numpy()
    np.save(os.path.join(directory, name + ".npy"), arr)
    return {name + ".npy": list(arr.shape)}


def check_layers(w, x, q, lut, y, g, qtype, on_right, inner, plan, layers=(0, 1, -1), rows=256, native=False):
    """Untimed: `rows` weight rows of a few layers of the launch's output against BOTH CPU oracles.

    * pass / fail: the restatement of the arithmetic the kernel that ran implements -- oracle.linear_group_scaled (the derived
      group-scaled formula, in double) when the pair-table kernel ran, oracle.linear (the reference's arithmetic: every weight
      rounded to 16 bits, MatrixLayoutB.cuh:1042-1046) otherwise -- at half an output ulp + f32 accumulation slack;
    * reported for every leg, in north_star's terms: the distance from the REFERENCE-FAITHFUL result (oracle.linear) --
      max-abs against its bf16 outputs and its f32 sums, max|y|, the same error at the captured fixture's scale
      (max|y| = 2.2, SURVEY.md 8c: north_star's 1e-2 is quoted there), the fraction of outputs whose bf16 bits differ from the
      reference-faithful bf16 result, and `formula_distance_f32`: the two CPU restatements against each other BEFORE the output
      rounding (what the regrouped arithmetic itself changes; 0 for the reference-numerics kernels).
    Contract (raises SystemExit otherwise): formula_distance_f32 <= 1e-2 at the fixture's scale, and the bf16 output within
    max(1e-2 at the fixture's scale, ONE bf16 step of the largest output) of the reference-faithful bf16 output.  (For
    |y| >= 2 one bf16 step is 1.6e-2: no kernel with bf16 outputs -- the reference's own included, whose summation order
    differs from its CPU path -- can promise 1e-2 there; a flipped final rounding is exactly one step.)"""
    import numpy as np

    from oracle import oracle as orc

    def bits(t):
        return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)

    n, k = y.shape[2], x.shape[2]
    oq = {"int4": orc.Q_INT4, "any4_global": orc.Q_ANY4_GLOBAL, "any4_rowwise": orc.Q_ANY4_ROWWISE, "mx4": orc.Q_MX4}[qtype]
    own = err_ref32 = err_ref16 = ymax = formula = 0.0
    differ = total = 0
    steps = 0
    for b in layers:
        if native and not on_right:  # the A-shaped tensor holds Bint4 words (innerKTiles 4 at k % 64 == 0, else 2)
            ib = 4 if k % 64 == 0 else 2
            codes = orc.unpack_Bint4(w[b].cpu().numpy().reshape(n // 8, k // (16 * ib), 32, ib // 2), n, k)[:rows]
        else:
            codes = (orc.unpack_Bint4 if on_right else orc.unpack_Aint4)(w[b].cpu().numpy(), n, k)[:rows]
        qi = q[b].cpu().numpy()[:rows] if qtype == "mx4" else bits(q[b][:, :rows].contiguous())
        lb = None if lut is None else (bits(lut[b][:rows]) if qtype == "any4_rowwise" else bits(lut[b]))
        xb = bits(x[b])
        r16, r32 = orc.linear(xb, codes, g, oq, qi, lb)                      # the reference's arithmetic
        y32 = orc.linear_group_scaled(xb, codes, g, oq, qi, lb)[1] if plan in ("pair", "gemv") else r32
        fin = np.isfinite(r32) & np.isfinite(y32)
        formula = max(formula, float(np.abs(y32.astype(np.float64) - r32.astype(np.float64))[fin].max()))
        wq = orc.bf16_to_f32(orc.dequant(codes, g, oq, qi, lb)).astype(np.float64)
        S = np.abs(x[b].double().cpu().numpy()) @ np.abs(wq).T
        got = y[b][:, :rows].double().cpu().numpy()
        ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(y32), 1e-30))) - 7)
        err = np.abs(got - y32)
        finite = np.isfinite(r32)  # (mx4 with exponent 255 gives NaN rows: not in the bench recipe, but keep the sums clean)
        if not (err[finite] <= (0.5 * ulp * (1 + 2.0 ** -7) + 4e-6 * S)[finite]).all():
            raise SystemExit(f"bench.py: output of layer {b} ({qtype}) does not match the oracle: max err {err[finite].max()}")
        own = max(own, float(err[finite].max()))
        err_ref32 = max(err_ref32, float(np.abs(got - r32.astype(np.float64))[finite].max()))
        ref16 = orc.bf16_to_f32(r16).astype(np.float64)
        err_ref16 = max(err_ref16, float(np.abs(got - ref16)[finite].max()))
        ymax = max(ymax, float(np.abs(ref16[finite]).max()))
        gb = bits(y[b][:, :rows].contiguous()).astype(np.int32)
        # bf16 bit patterns are monotone in the value within a sign: distance in representable steps
        key = lambda u: np.where(u & 0x8000, -(u & 0x7fff), u & 0x7fff)  # noqa: E731
        d = np.abs(key(gb) - key(r16.astype(np.int32)))
        differ += int((d[finite] != 0).sum())
        total += int(finite.sum())
        # (outputs near zero sit many bf16 steps from anything: the step count is only meaningful where |y| is large)
        top = finite & (np.abs(ref16) >= 2.0 ** np.floor(np.log2(max(float(np.abs(ref16[finite]).max()), 1e-30))))
        steps = max(steps, int(d[top].max()) if top.any() else 0)
    scale = 2.2 / max(ymax, 2.2)
    step = float(np.exp2(np.floor(np.log2(max(ymax, 1e-30))) - 7))  # one bf16 step of the largest output
    # north_star's contract, RAW: the activations of every leg are scaled (calibrate_x: by a power of two, exact in bf16) so that
    # max|y| lies in (0.95, 1.9] -- the order of the captured fixture's 2.2, below the binade where ONE bf16 step is
    # already 1.6e-2 -- and there the output must be within 1e-2 max-abs of the reference-faithful bf16 result, no other clause
    if not (ymax < 2.0 and formula <= 1e-2 and err_ref16 <= 1e-2):
        raise SystemExit(f"bench.py: {qtype}: max-abs {err_ref16:.3e} from the reference-faithful bf16 result (arithmetic before the output "
                         f"rounding: {formula:.3e}) at max|y| = {ymax:.3f}: outside north_star's 1e-2 at max|y| < 2")
    return {"max_abs_err_vs_kernel_formula": own, "kernel_formula": "group_scaled" if plan in ("pair", "gemv") else "reference",
            "max_abs_err_vs_reference": err_ref16, "max_abs_err_vs_reference_f32": err_ref32, "max_abs_y": ymax,
            "one_bf16_step_at_max_abs_y": step, "contract": "max_abs_err_vs_reference <= 1e-2 at max|y| < 2 (raw)",
            "max_abs_err_vs_reference_at_fixture_scale": err_ref16 * scale,
            "formula_distance_f32": formula, "formula_distance_f32_at_fixture_scale": formula * scale,
            "frac_outputs_differing_from_reference_bf16": round(differ / max(total, 1), 5), "max_bf16_steps_from_reference_in_top_binade": steps,
            "outputs_checked": total}


def cpu_baseline_torch(m, n, k, g, budget_s=10.0):
    """The reference's CPU path (quantize.py:612-637 anyq_dequantize_tensor -> degroup_q 160-174, then x @ W^T), restated
    with torch ops on bf16 CPU tensors: gather the per-row LUT, (w - 8) * scale + zero op by op in bf16, matmul.
    (the reference's LUT lives in the [0, 15] domain and the module stores lut - 8.)"""
    gen = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 16, (n, k), dtype=torch.int64, generator=gen)
    lut = (torch.rand(n, 16, generator=gen) * 15).to(torch.bfloat16)
    scales = (torch.rand(k // g, n, generator=gen) * 0.02 + 0.005).to(torch.bfloat16)
    zeros = (torch.randn(k // g, n, generator=gen) * 0.01).to(torch.bfloat16)
    x = torch.randn(m, k, generator=gen).to(torch.bfloat16)

    def layer():
        w = torch.gather(lut, 1, codes)                                   # [n][k] bf16, values in [0, 15]
        w = w.view(n, k // g, g)
        w = (w - 8) * scales.t().unsqueeze(2) + zeros.t().unsqueeze(2)    # degroup_q: op by op in bf16
        return x @ w.view(n, k).t()

    # thread count: SURVEY 8d asks for os.cpu_count(), but torch's bf16 CPU element-wise ops collapse when oversubscribed
    # (measured: 1.7 s per layer with 256 threads on a 128-core host), so probe and keep the fastest; all counts are reported
    phys, logical = physical_cores()
    cands = sorted({c for c in (8, 16, 32, 64, phys or 0, _SCHEDULABLE_CPUS) if 0 < c <= _SCHEDULABLE_CPUS})
    probe = {}
    for c in cands:
        torch.set_num_threads(c)
        layer()
        t0 = time.perf_counter()
        layer()
        probe[c] = time.perf_counter() - t0
        if probe[c] > 2.0 and len(probe) > 1:
            break
    threads = min(probe, key=probe.get)
    torch.set_num_threads(threads)
    layer()
    layers, t0 = 0, time.perf_counter()
    while True:
        layer()
        layers += 1
        dt = time.perf_counter() - t0
        if (dt >= budget_s and layers >= 3) or layers >= 2000:
            break
    return {"value": round(layers * alg_bytes(m, n, k, g) / dt / 1e9, 4), "unit": "GB/s", "cores": threads, "kind": "port",
            "sample": f"{layers} layers of the bench workload (m={m}, n=k={n}, g={g}) in {dt:.1f} s = {dt / layers * 1e3:.1f} ms per layer; "
                      f"torch {torch.__version__} CPU bf16: gather LUT -> (w-8)*scale+zero -> matmul (the reference's quantize.py:612-637, 160-174), "
                      f"torch.set_num_threads({threads}) = fastest of {sorted(probe)} (os.cpu_count() = {logical}); host has {phys} physical cores / {logical} logical CPUs, {_SCHEDULABLE_CPUS} schedulable"}


def cpu_baseline_oracle(m, n, k, g, budget_s=8.0):
    """The C oracle (oracle/tinygemm_oracle.c: the reference KERNEL's arithmetic, OpenMP over weight rows) on the same workload."""
    import numpy as np

    from oracle import oracle as orc

    orc.build()
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 16, (n, k), dtype=np.int32)
    lut = orc.bf16_bits(rng.standard_normal((n, 16)).astype(np.float32))
    sz = orc.bf16_bits((rng.random((k // g, n, 2)) * 0.02).astype(np.float32))
    x = orc.bf16_bits(rng.standard_normal((m, k)).astype(np.float32))
    avail = _SCHEDULABLE_CPUS
    cands = sorted({min(avail, 1 << i) for i in range(0, 10)} | {avail})
    best, best_t = 1, float("inf")
    for t in cands:
        orc.set_num_threads(t)
        orc.linear(x, codes, g, orc.Q_ANY4_ROWWISE, sz, lut)
        t0 = time.perf_counter()
        orc.linear(x, codes, g, orc.Q_ANY4_ROWWISE, sz, lut)
        dt = time.perf_counter() - t0
        if dt < best_t:
            best, best_t = t, dt
    orc.set_num_threads(best)
    orc.linear(x, codes, g, orc.Q_ANY4_ROWWISE, sz, lut)
    layers, t0 = 0, time.perf_counter()
    while True:
        orc.linear(x, codes, g, orc.Q_ANY4_ROWWISE, sz, lut)
        layers += 1
        dt = time.perf_counter() - t0
        if dt >= budget_s or layers >= 2000:
            break
    return {"value": round(layers * alg_bytes(m, n, k, g) / dt / 1e9, 4), "unit": "GB/s", "cores": orc.num_threads(), "kind": "port",
            "sample": f"{layers} layers in {dt:.1f} s, OpenMP over weight rows, {dt / layers * 1e3:.1f} ms per layer; fastest of thread counts {cands}"}


def decode_leg(device, steps=48, warmup=8, start_pos=128, layers=None):
    """BASELINE config 5 at TP = 1: one decode step (one new token, batch 1) of a Llama-3-8B-shaped stack -- 32 layers, hidden
    4096, 32 / 8 heads, inter 14336, random any4 weights of that architecture (no checkpoints here), 16-bit LM head as in the
    reference (quantize.py:34-36), static KV cache, the whole step replayed from one hipGraph (any4_amd/decode.py; protocol
    of the reference's benchmark.py:113-215 minus HuggingFace's Python).  HBM bytes per token = the algorithmic bytes of the
    4-bit linears + the 16-bit LM head + the KV cache read at the timed positions."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig.llama3_8b(max_seq=1024, gate_up_interleave=8)  # (gate / up rows in blocks of 8 + 8: SwiGLU rides in the GEMM's store)
    if layers is not None:
        cfg.layers = layers
    stack = DecodeStack(cfg, Any4Factory(cfg, device, torch.bfloat16, seed=1), device, torch.bfloat16, bs=1)
    stack.capture()
    tok = torch.randint(0, cfg.vocab, (1,), device=device)
    for i in range(warmup):
        stack.decode(tok, start_pos + i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(steps):
        stack.decode(tok, start_pos + warmup + i)
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    dev_ms = e0.elapsed_time(e1) / steps
    nodes = getattr(stack, "graph_nodes", None)
    pos_mid = start_pos + warmup + steps // 2
    b4 = cfg.weight_bytes_4bit()
    lm = cfg.vocab * cfg.hidden * 2
    kv = 2 * cfg.layers * cfg.kv_heads * cfg.head_dim * 2 * pos_mid
    total = b4 + lm + kv
    out = {"ms_per_token": round(dev_ms, 4), "ms_per_token_wall": round(wall * 1e3, 4), "tokens_per_s": round(1e3 / dev_ms, 1),
           "hbm_bytes_per_token": total, "bytes_4bit_linears": b4, "bytes_lm_head_16bit": lm, "bytes_kv_cache": kv,
           "hbm_roofline_ms": round(total / (HBM_PEAK_GBPS * 1e9) * 1e3, 4),
           "frac_of_hbm_roofline": round(total / (HBM_PEAK_GBPS * 1e9) * 1e3 / dev_ms, 4),
           "layers": cfg.layers, "tp": 1, "bs": 1, "hipgraph": True, "kernels_per_layer": getattr(stack, "kernels_per_layer", None),
           "note": f"Llama-3-8B shape, random any4 weights (per-row LUT, g=128), KV cache of {cfg.max_seq}, tokens at positions "
                   f"{start_pos + warmup}..{start_pos + warmup + steps - 1}, default numerics; {steps} graph replays between one HIP-event pair"}
    if nodes is not None:
        out["graph_nodes"] = nodes
    del stack
    torch.cuda.empty_cache()
    return out


def decode_shaped_exchange(lib, _lib, w, x, sz, lut, y, m, n, k, g, inner, device, local_rank, stream, world, rccl=True, iters=256):
    """N > 1 only: the exchange as a decode step issues it -- ONE layer per launch (this rank's [n, k] shard of an
    [N n, k] projection), then the gather of the [m, n] partial outputs (m n 2 bytes per rank: latency-bound), back to back on
    one stream, for (a) no exchange, (b) RCCL all_gather_into_tensor, (c) the one-shot peer-write gather of
    include/peer_gather_hip.h.  Every rank runs the same sequence; times are the max over ranks, in us per layer."""
    import torch.distributed as dist

    nl = min(int(w.shape[0]), 64)
    singles = [make_args(_lib, w[i:i + 1], x[i:i + 1], sz[i:i + 1], lut[i:i + 1], y[i:i + 1], m, n, k, g, "any4_rowwise", True, inner, 1)
               for i in range(nl)]
    parts = torch.empty(world, m, n, device=device, dtype=torch.bfloat16)

    def launch(i):
        _lib.check(lib.tg_gemm_w4(ctypes.byref(singles[i % nl]), local_rank, stream.cuda_stream), "tg_gemm_w4")

    def timed(after):
        for i in range(8):
            launch(i)
            after(i)
        dist.barrier()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(iters):
            launch(i)
            after(i)
        e1.record(stream)
        torch.cuda.synchronize()
        t = torch.tensor([e0.elapsed_time(e1) * 1e3 / iters], device=device if rccl else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return round(float(t[0]), 3)

    out = {"layers_in_rotation": nl, "iters": iters, "bytes_per_rank_per_gather": m * n * 2,
           "us_per_layer_gemv_only": timed(lambda i: None)}
    if rccl:
        out["us_per_layer_gemv_plus_rccl_all_gather"] = timed(lambda i: dist.all_gather_into_tensor(parts, y[i % nl]))
    pg, err = None, None
    try:  # (the constructor either succeeds on every rank or raises on every rank)
        from any4_amd.shard import PeerWriteGather

        pg = PeerWriteGather(max(m, 1), n, device=device, dtype=torch.bfloat16, timeout_us=500_000)
    except Exception as e:  # noqa: BLE001
        err = f"{type(e).__name__}: {e}"
    if pg is not None:
        ok = 1
        try:
            for i in range(4):
                pg.gather(y[i % nl].view(m, n))
            pg.check()
        except Exception as e:  # noqa: BLE001
            ok, err = 0, f"{type(e).__name__}: {e}"
        t = torch.tensor([ok], device=device if rccl else "cpu", dtype=torch.int32)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        if int(t[0]) == 1:
            out["us_per_layer_gemv_plus_peer_write_gather"] = timed(lambda i: pg.gather(y[i % nl].view(m, n)))
            try:
                pg.check()
            except RuntimeError as e:
                err = str(e)
        elif err is None:
            err = "a peer rank reported a failed peer-write gather"
        pg.close()
    if err is not None:
        out["peer_write_gather_error"] = err
    out["note"] = ("one single-layer tg_gemm_w4 launch per layer + the gather of its [m, n] outputs, back to back on one stream, max over ranks; "
                   "the stacked 4 MiB-per-rank all-gather inside `value` is the bandwidth-shaped exchange, this is the latency-shaped one a decode step issues")
    return out


def m1_contraction_ab(_lib, lib, ops, timed, args_default, tensors, shape, device, bytes_per_launch, rounds=6, reps=60):
    """The headline launch with its m = 1 contraction (a) per lane on v_dot2_f32_bf16 (TG_NUM_FAST_DOT2) and (b) on the matrix core
    (TG_NUM_FAST_MFMA: v_mfma_f32_32x32x16_bf16, north_star's "fed to bf16 MFMA"), ALTERNATING on this box in the sustained state of
    the timed region: `rounds` alternations of `reps` back-to-back launches each between one HIP-event pair.  Which of the two the
    library's default (TG_NUM_FAST) takes is reported next to it (`default_contraction`, tg_m1_default_contraction())."""
    w, x, sz, lut, y = tensors
    m, n, k, g, inner, L = shape
    arms = {}
    for name in ("fast_dot2", "fast_mfma"):
        aa = make_args(_lib, w, x, sz, lut, y, m, n, k, g, "any4_rowwise", True, inner, L, name, native=True)
        arms[name] = (aa, attach_workspace(lib, aa, device))
    us = {name: [] for name in arms}
    for _ in range(rounds):
        for name, (aa, _ws) in arms.items():
            us[name].append(timed(aa, reps))
    out = {}
    for name, v in us.items():
        fr = [bytes_per_launch / (t * 1e-6) / 1e9 / HBM_PEAK_GBPS for t in v]
        out[name] = {"launch_us": [round(t, 2) for t in v], "frac_mean": round(sum(fr) / len(fr), 4), "frac_min": round(min(fr), 4),
                     "frac_max": round(max(fr), 4)}
    d = out["fast_mfma"]["frac_mean"] / out["fast_dot2"]["frac_mean"] - 1.0
    out["mfma_over_dot2_percent"] = round(100.0 * d, 2)
    out["default_contraction"] = {0: "v_dot2", 1: "mfma"}.get(int(lib.tg_m1_default_contraction()), "?")
    out["protocol"] = f"{rounds} alternations x {reps} stacked launches of {L} layers per arm, one HIP-event pair per arm and round, same process, after the timed region"
    return out


def pmc_mean(counters, extra, timeout_s=240):
    """Mean over the GEMM kernel's dispatches of each PMC counter in `counters` -- one rocprofv3 pass per counter (never together
    with a trace) over `bench.py --roofline-only <extra>` in a child process.  Returns ({counter: mean}, None) or (None, why)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found on this box"
    vals = {}
    tmp = tempfile.mkdtemp(prefix="bench_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        for ctr in counters:
            d = os.path.join(tmp, ctr)
            cmd = [prof, "--pmc", ctr, "--output-format", "csv", "-d", d, "-o", "pmc", "--", sys.executable,
                   os.path.abspath(__file__), "--roofline-only", "--steps", "3", "--warmup", "2", "--settle-s", "0.02", *extra]
            try:
                subprocess.run(cmd, cwd="/tmp", env=env, timeout=timeout_s, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
            except (subprocess.SubprocessError, OSError) as e:
                return None, f"rocprofv3 --pmc {ctr} pass failed ({type(e).__name__})"
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if "w4_gemm" in r["Kernel_Name"] and "xprep" not in r["Kernel_Name"] and r["Counter_Name"] == ctr:
                        rows.append(float(r["Counter_Value"]))
            if not rows:
                return None, f"no {ctr} rows for the GEMM kernel in the rocprofv3 output"
            vals[ctr] = sum(rows) / len(rows)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return vals, None


def pmc_traffic(L, bytes_per_launch, timeout_s=240):
    """HBM bytes per launch of the dominant kernel from the PMC counters, measured live: two rocprofv3 passes (FETCH_SIZE and
    WRITE_SIZE do not fit one pass on gfx950) over `bench.py --roofline-only` in a child process, corrected as
    MI355X_MICROARCH.md (HBM section) prescribes: FETCH_SIZE counts the 128-byte requests of 16-byte-per-lane streaming reads
    at 64 bytes -> read bytes = 2 x FETCH_SIZE[KB] x 1024; WRITE_SIZE[KB] x 1024 as reported.  Returns (bytes or None, note)."""
    vals, why = pmc_mean(("FETCH_SIZE", "WRITE_SIZE"), ["--layers", str(L)], timeout_s)
    if vals is None:
        return None, why
    rd, wr = 2.0 * vals["FETCH_SIZE"] * 1024.0, vals["WRITE_SIZE"] * 1024.0
    return int(rd + wr), (f"live: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes) over `bench.py --roofline-only --layers {L}`; "
                          f"mean over the kernel's dispatches: FETCH_SIZE {vals['FETCH_SIZE']:.0f} KB x 2 (gfx950 correction for 16-B/lane streaming reads) "
                          f"+ WRITE_SIZE {vals['WRITE_SIZE']:.0f} KB = {(rd + wr) / bytes_per_launch:.4f} x the algorithmic bytes")


def pmc_mfma_util():
    """MfmaUtil (percent of cycles the matrix pipe is busy, rocprofv3's derived counter) of the legs the metric / BASELINE config 3
    name it for -- north_star: 'MFMA utilisation at m=8/16' -- live, one child pass each; None where a pass failed."""
    out = {}
    for name, extra in (("m8", ["--m", "8", "--layers", "256"]), ("m16", ["--m", "16", "--layers", "256"]),
                        ("config3", ["--m", "8", "--n", "8192", "--k", "8192", "--layers", "64", "--left"])):
        vals, why = pmc_mean(("MfmaUtil",), extra)
        out[name] = round(vals["MfmaUtil"], 2) if vals else None
        if vals is None:
            out[name + "_note"] = why
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--layers", type=int, default=512, help="independent layers per step (stacked launch)")
    ap.add_argument("--m", type=int, default=1)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--settle-s", type=float, default=2.0, help="seconds of untimed steps before the timed region")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-decode", action="store_true", help="skip the Llama-3-8B decode leg (config 5)")
    ap.add_argument("--no-pmc", action="store_true", help="skip the live rocprofv3 PMC passes that fill roofline.traffic")
    ap.add_argument("--left", action="store_true", help="weights on the left (weightOnRight=False ops) in the library's default packed format")
    ap.add_argument("--dist-backend", default=os.environ.get("BENCH_DIST_BACKEND", "nccl"), choices=("nccl", "gloo"),
                    help="torch.distributed backend for N > 1 (nccl = RCCL; gloo: control plane only, the data exchange is the peer-write gather)")
    ap.add_argument("--same-device", action="store_true", help="N > 1 dry run on a one-GPU box: every rank on GPU 0")
    ap.add_argument("--roofline-only", action="store_true",
                    help="skip the informational legs (other configs, single-layer, cpu): every launch of the stacked "
                         "kernel is then a timed-shape launch, which is what the rocprofv3 --stats pass wants")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure, also the oracle check, the other configs, single-layer launches, many-rows GEMM, "
                         "decode leg, PMC passes, CPU baselines and (N > 1) the other exchanges; a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's output (the whole problem's [layers, m, n]) to DIR/y.npy in float32; "
                         f"above {DUMP_CAP_BYTES >> 20} MiB a fixed, seeded sample of its elements to DIR/y_sample.npy instead")
    a = ap.parse_args()
    if a.steps < 1:
        raise SystemExit("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus and world > 1:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    if a.same_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)

    import torch.distributed as dist

    if world > 1:
        dist.init_process_group(backend=a.dist_backend)  # "nccl" is RCCL on ROCm
    rccl = world > 1 and a.dist_backend == "nccl"

    def barrier():
        # (gloo: a CPU barrier; the ranks' GPU work is fenced by the synchronize() next to every call)
        dist.barrier()

    def all_max(vals):
        """max over ranks of a list of floats (on the device for RCCL, on the host for gloo)."""
        if world == 1:
            return [float(v) for v in vals]
        t = torch.tensor(vals, dtype=torch.float64, device=device if rccl else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return [float(v) for v in t]

    from any4_amd import _lib, ops

    lib = _lib.load()
    L, m, n_full, k, g, inner = a.layers, a.m, a.n, a.k, a.group, 4
    on_right = not a.left
    if n_full % (world * 16):
        raise SystemExit(f"--n {n_full} must split into whole 16-row tiles per rank (N = {world})")
    n = n_full // world          # this rank's rows of every layer (strong scaling: the whole problem is L layers of n_full rows)
    w, x, sz, lut, y = make_batch(L, m, n, k, g, inner, device, seed=1234 + rank, on_right=on_right)

    def replicate(t):
        """Every rank sees rank 0's activations (as after the previous layer's gather)."""
        if rccl:
            dist.broadcast(t, src=0)
        elif world > 1:
            c = t.cpu()
            dist.broadcast(c, src=0)
            t.copy_(c)

    replicate(x)
    args = make_args(_lib, w, x, sz, lut, y, m, n, k, g, "any4_rowwise", on_right, inner, L, native=True)
    args_ws = attach_workspace(lib, args, device)  # noqa: F841  (kept alive)
    plan = ops.gemm_w4_plan(m, n, k, g, QT["any4_rowwise"], on_right, inner, torch.bfloat16, L, "fast", weight_format="native")
    stream = torch.cuda.current_stream()

    def launch(aa):
        _lib.check(lib.tg_gemm_w4(ctypes.byref(aa), local_rank, stream.cuda_stream), "tg_gemm_w4")

    x_scale = calibrate_x(lambda: launch(args), x, y)
    replicate(x)

    # the exchange of a step: ONE gather of the [L m][n / N] partial outputs of the whole layer batch
    pg, pg_err, y_all = None, None, None
    if world > 1:
        y_all = torch.empty(world, L, m, n, device=device, dtype=torch.bfloat16)   # RCCL's layout: rank-major
        try:  # (the constructor either succeeds on every rank or raises on every rank)
            from any4_amd.shard import PeerWriteGather

            pg = PeerWriteGather(L * m, n, device=device, dtype=torch.bfloat16, timeout_us=5_000_000)   # -> [L m][n_full], feature order
        except Exception as e:  # noqa: BLE001
            pg_err = f"{type(e).__name__}: {e}"
        if not rccl and pg is None:
            raise SystemExit(f"bench.py: --dist-backend gloo needs the peer-write gather for the data exchange ({pg_err})")
    exchange_kind = "none" if world == 1 else ("rccl_all_gather_into_tensor" if rccl else "peer_write_gather")

    def gather_rccl():
        dist.all_gather_into_tensor(y_all, y)
        return y_all

    def gather_peer():
        return pg.gather(y.view(L * m, n))

    gather = (lambda: None) if world == 1 else (gather_rccl if rccl else gather_peer)

    def step():
        launch(args)
        gather()

    def fence():
        # (the device is drained first: a rank arrives at the barrier when ITS work is done; then once more for RCCL's own barrier kernel)
        torch.cuda.synchronize()
        if world > 1:
            barrier()
            torch.cuda.synchronize()

    if a.warmup > 0:  # the first warm-up step also pays for one-off initialisation (code load, RCCL communicator): keep it
        step()        # out of the clock that decides about settling steps
        fence()
    t_w = time.perf_counter()
    for _ in range(a.warmup - 1):
        step()
    fence()
    # untimed settling under the timed load; every rank derives the SAME number of steps
    t_warm = all_max([time.perf_counter() - t_w])[0]
    per_step = t_warm / (a.warmup - 1) if a.warmup > 1 else 1.0e-3
    settle = 0 if t_warm >= a.settle_s else min(5000, int((a.settle_s - t_warm) / max(per_step, 1e-5)) + 1)
    for _ in range(settle):
        step()
    fence()
    # kernel-only duration of the dominant kernel, measured live with HIP events on the launch stream
    # (N = 1: ONE event pair around the K back-to-back launches -- an event pair per launch puts two marker packets between
    #  consecutive kernels, 5-6 us per 820-us step that belong to the measurement, not to the path; N > 1: a pair per launch,
    #  because the all-gather sits between the launches)
    per_launch = world > 1
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps if per_launch else 1)]
    gathered = None
    t0 = time.perf_counter()
    if not per_launch:
        ev[0][0].record(stream)
    for s in range(a.steps):
        if per_launch:
            ev[s][0].record(stream)
        launch(args)
        if per_launch:
            ev[s][1].record(stream)
            gathered = gather()
    if not per_launch:
        ev[0][1].record(stream)
    fence()
    elapsed = time.perf_counter() - t0
    kern_ms = sum(e0.elapsed_time(e1) for e0, e1 in ev) / a.steps

    elapsed, kern_ms = all_max([elapsed, kern_ms])

    # what a caller of the timed path receives from its last step: [L][m][n_full] (N > 1: the gathered outputs of every rank)
    dumped = None
    if a.dump_outputs and rank == 0:
        if world == 1:
            y_out = y
        elif rccl:
            y_out = gathered.permute(1, 2, 0, 3).reshape(L, m, n_full)   # rank-major [N][L][m][n] -> rows of rank r at [r n, (r+1) n)
        else:
            y_out = gathered.view(L, m, n_full)                           # the peer-write gather's [L m][n_full], feature order
        dumped = dump_outputs(a.dump_outputs, y_out)

    bytes_layer = alg_bytes(m, n, k, g)              # this rank's shard of one layer (x is read by every rank)
    bytes_layer_full = alg_bytes(m, n_full, k, g)    # the layer of the whole problem (x counted once)
    bytes_step_rank = L * bytes_layer
    ms_per_step = elapsed / a.steps * 1e3
    value = L * bytes_layer_full / (elapsed / a.steps) / 1e9
    achieved = bytes_step_rank / (kern_ms * 1e-3) / 1e9

    def timed_steps(fn, steps):
        """`steps` calls of fn between two fences, max over ranks, ms per step."""
        fn()
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        fence()
        return all_max([(time.perf_counter() - t0) / steps * 1e3])[0]

    def timed(aa, reps):
        for _ in range(3):
            launch(aa)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            launch(aa)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # us per launch

    slope_us = main_check = m1_ab = None
    if rank == 0 and a.full and not a.roofline_only:
        # marginal rate: slope of launch time over the number of stacked layers -- measured first, while the
        # clock is still in the steady state of the timed region
        half = make_args(_lib, w, x, sz, lut, y, m, n, k, g, "any4_rowwise", on_right, inner, L // 2, native=True)
        t_half, t_full = timed(half, 40), timed(args, 40)
        slope_us = (t_full - t_half) / (L - L // 2)
        if m == 1 and on_right and world == 1:
            m1_ab = m1_contraction_ab(_lib, lib, ops, timed, args, (w, x, sz, lut, y), (m, n, k, g, inner, L), device, bytes_step_rank)
        # (a) the timed launch's own output against the oracle
        main_check = check_layers(w, x, sz, lut, y, g, "any4_rowwise", on_right, inner, plan, native=True)

    exchange = strong_extra = weak = None
    if world > 1 and a.full and not a.roofline_only:
        # the same strong-scaling step with the other exchange, and with none (what the exchange costs)
        side = min(a.steps, 50)
        strong_extra = {"ms_per_step_no_exchange": round(timed_steps(lambda: launch(args), side), 5)}
        both = pg is not None and rccl
        if both:
            ok = 1
            try:
                for _ in range(3):
                    gather_peer()
                pg.check()
            except Exception as e:  # noqa: BLE001
                ok, pg_err = 0, f"{type(e).__name__}: {e}"
            if min(all_max([-float(ok)])) == -1.0 and ok:   # every rank's peer-write gather worked
                ms_peer = timed_steps(lambda: (launch(args), gather_peer()), side)
                strong_extra["peer_write_gather"] = {"ms_per_step": round(ms_peer, 5), "value_GBps": round(L * bytes_layer_full / ms_peer / 1e6, 2)}
        if pg_err is not None:
            strong_extra["peer_write_gather_error"] = pg_err
        strong_extra["note"] = (f"{side} steps each, same protocol as the timed region: the kernel alone, and (RCCL runs) the step with the one-shot "
                                "peer-write gather (include/peer_gather_hip.h: [L m][n] in feature order) instead of RCCL's all_gather_into_tensor")
        exchange = decode_shaped_exchange(lib, _lib, w, x, sz, lut, y, m, n, k, g, inner, device, local_rank, stream, world, rccl)
        if pg is not None:
            pg.close()
            pg = None
        # the weak-scaling protocol of rounds 1-5: every rank ITS OWN n_full rows of every layer, RCCL all-gather of y per step
        torch.cuda.synchronize()
        del w, sz, lut
        torch.cuda.empty_cache()
        ww, _, wq, wl, wy = make_batch(L, m, n_full, k, g, inner, device, seed=4321 + rank, on_right=on_right)
        wargs = make_args(_lib, ww, x, wq, wl, wy, m, n_full, k, g, "any4_rowwise", on_right, inner, L, native=True)
        wargs_ws = attach_workspace(lib, wargs, device)  # noqa: F841
        wy_all = torch.empty(world, L, m, n_full, device=device, dtype=torch.bfloat16) if rccl else None

        def weak_step():
            launch(wargs)
            if rccl:
                dist.all_gather_into_tensor(wy_all, wy)

        ms_weak = timed_steps(weak_step, side)
        weak = {"value": round(world * L * bytes_layer_full / ms_weak / 1e6, 2), "unit": "GB/s", "ms_per_step": round(ms_weak, 5), "steps": side,
                "scaling": "weak", "exchange": "rccl_all_gather_into_tensor" if rccl else "none (gloo dry run)",
                "note": f"every rank its own {n_full} rows of each of the {L} layers (an [N n, k] projection), all-gather of the [L m][n] outputs per step"}
        del ww, wq, wl, wy, wy_all
        w = sz = lut = None

    if rank == 0 and a.roofline_only:
        print(json.dumps({"roofline_only": True, "launch_us": round(kern_ms * 1e3, 3), "GBps": round(achieved, 2),
                          "steps": a.steps, "warmup": a.warmup, "settle_steps": settle, "layers": L, "kernel_plan": plan}), flush=True)
    elif rank == 0:

        def leg(qtype, mm, nn, kk, gg, on_right, layers, note, numerics="fast", native=True):
            """One more BASELINE config as a stacked launch of `layers` layers (same protocol: steady clock, HIP events).
            native: weights on the left in the library's default packed format (row-per-lane order) -- False: the reference's words."""
            ww, xx, qq, ll, yy = make_batch(layers, mm, nn, kk, gg, inner, device, 77, qtype, on_right)
            aa = make_args(_lib, ww, xx, qq, ll, yy, mm, nn, kk, gg, qtype, on_right, inner, layers, numerics, native)
            ws = attach_workspace(lib, aa, device)  # noqa: F841
            xs = calibrate_x(lambda: launch(aa), xx, yy)
            wf = "native" if native else "reference"
            pl = ops.gemm_w4_plan(mm, nn, kk, gg, QT[qtype], on_right, inner, torch.bfloat16, layers, numerics, weight_format=wf)
            pld = ops.gemm_w4_plan(mm, nn, kk, gg, QT[qtype], on_right, inner, torch.bfloat16, layers, numerics, detail=True, weight_format=wf)
            bl = alg_bytes(mm, nn, kk, gg, qtype)
            reps = max(10, int(0.25e6 / (layers * bl / 5e6)))  # ~0.25 s of launches
            us = timed(aa, reps) / layers
            chk = check_layers(ww, xx, qq, ll, yy, gg, qtype, on_right, inner, pl, layers=(0, -1), rows=128, native=native)
            return {"us_per_layer": round(us, 4), "GBps": round(bl / us / 1e3, 2), "frac": round(bl / us / 1e3 / HBM_PEAK_GBPS, 4),
                    "algorithmic_bytes_per_layer": bl, "layers_per_launch": layers, "kernel_plan": pld, "numerics": numerics,
                    "check": chk, "x_scale": xs, "note": note}

        # N > 1: the other configs, the single-launch figures, the decode leg and the CPU baselines are N = 1 facts (the driver's
        # N = 1 run carries them): rank 0 does not keep the other ranks waiting in the final barrier for them
        legs = {} if world > 1 or not a.full else {
            "m8": leg("any4_rowwise", 8, n, k, g, True, L, f"the metric's second point: m=8, n=k={n}, g={g}, Bint4"),
            "m16": leg("any4_rowwise", 16, n, k, g, True, L // 2, f"m=16 (the reference's full 16-row tile, TinyGemmImpl.cuh:53-54), n=k={n}, g={g}, Bint4"),
            "config3": leg("any4_rowwise", 8, 8192, 8192, 128, False, 128, "BASELINE config 3: m=8, n=k=8192, g=128, weights on the A side (weightOnRight=False ops), in the packed format convert_matrix_to_m16n8k16_Aint4_layout returns (row-per-lane order, TG_WFMT_ROWS)"),
            "config3_reference_words": leg("any4_rowwise", 8, 8192, 8192, 128, False, 128, "config 3 on a tensor that holds the reference's own Aint4 words (a checkpoint packed by the CUDA implementation, any4_amd.weight_format('reference'))", native=False),
            "m1_mfma": leg("any4_rowwise", 1, n, k, g, True, L, "the headline workload with the m = 1 contraction on the matrix core (TG_NUM_FAST_MFMA: north_star's 'fed to bf16 MFMA'; w4_gemm_xr_kernel's 16x16x32 MFMAs) instead of the per-lane v_dot2 the default takes", "fast_mfma"),
            "int4": leg("int4", 1, n, k, g, True, L, "BASELINE config 4: uniform int4, m=1"),
            "nf4": leg("any4_global", 1, n, k, g, True, L, "BASELINE config 4: one global 16-entry LUT (the reference's NF4 path), m=1"),
            "mx4": leg("mx4", 1, n, k, 32, True, L, "BASELINE config 4: mx4 (fp4-e2m1 codes, e8m0 exponent per 32), m=1; weights converted by v_cvt_scalef32_pk_bf16_fp4"),
            "mx4_m16": leg("mx4", 16, n, k, 32, True, L // 2, "mx4, m=16 (w4_gemm_xr_kernel, weights converted in registers)"),
            # the same workload with the reference's own dequant arithmetic (every weight rounded to 16 bits with one fma,
            # MatrixLayoutB.cuh:1042-1046): the kernels whose weights are bit-identical to the reference's
            "reference_numerics": {
                "m1": leg("any4_rowwise", 1, n, k, g, True, L, f"TG_NUM_REFERENCE, m=1, n=k={n}, g={g}, Bint4", "reference"),
                "m8": leg("any4_rowwise", 8, n, k, g, True, L, f"TG_NUM_REFERENCE, m=8, n=k={n}, g={g}, Bint4", "reference"),
            },
        }

        def many_rows_leg(mm, nn, kk, gg, layers=8):
            """More than 64 activation rows (a prefill through the modules): one nn x kk layer per launch on the library's own LDS-tiled
            MFMA GEMM (w4_gemm_tile_kernel, plan 'tile').  Matrix-core bound: achieved TFLOP/s against the dense bf16 MFMA peak; checked
            against the oracle's reference-faithful weights on a sample of rows."""
            ww, xx, qq, ll, yy = make_batch(layers, mm, nn, kk, gg, inner, device, 55, "any4_rowwise", True)
            xx.mul_(2.0 ** -5)   # (k = 4096 products of unit-variance activations: keep max|y| near 1 like the other legs)
            singles = [make_args(_lib, ww[i:i + 1], xx[i:i + 1], qq[i:i + 1], ll[i:i + 1], yy[i:i + 1], mm, nn, kk, gg, "any4_rowwise", True, inner, 1)
                       for i in range(layers)]
            # the caller's scratch (as the ops bring it): fewer tiles than CUs -> a split-K launch, f32 partial tiles summed in split order
            ws_keep = attach_workspace(lib, singles[0], device)  # noqa: F841  (kept alive)
            for sa in singles[1:]:
                sa.workspace, sa.workspace_bytes = singles[0].workspace, singles[0].workspace_bytes   # (one stream: the launches are ordered)
            for sa in singles:
                launch(sa)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(5):
                for sa in singles:
                    launch(sa)
            e1.record(stream)
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / (5 * layers)
            # a sample of 8 activation rows x 256 weight rows of the last layer against the oracle (f64 sums of the reference's weights)
            import numpy as np

            from oracle import oracle as orc

            bits = lambda t: t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)  # noqa: E731
            rows = 256
            codes = orc.unpack_Bint4(ww[-1].cpu().numpy(), nn, kk)[:rows]
            wq = orc.bf16_to_f32(orc.dequant(codes, gg, orc.Q_ANY4_ROWWISE, bits(qq[-1][:, :rows].contiguous()), bits(ll[-1][:rows]))).astype(np.float64)
            xs = xx[-1][:: max(1, mm // 8)][:8].double().cpu().numpy()
            want = xs @ wq.T
            got = yy[-1][:: max(1, mm // 8)][:8, :rows].double().cpu().numpy()
            # half an output ulp (exact: 2^(floor(log2 |y|) - 8)) + f32 accumulation slack over k products in the matrix core's order
            ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 7)
            tol = 0.5 * ulp * (1 + 2.0 ** -6) + (np.abs(xs) @ np.abs(wq).T) * 3e-5 + 1e-30   # (sqrt(k) 2^-24 = 3.8e-6 of sum |x w| is one sigma)
            err = float((np.abs(got - want) / tol).max())
            if not err <= 1.0:
                raise SystemExit(f"bench.py: many-rows GEMM (m = {mm}) does not match the oracle: err / tol = {err:.3f}")
            flop = 2.0 * mm * nn * kk
            return {"m": mm, "n": nn, "k": kk, "us_per_layer": round(us, 2), "TFLOPs": round(flop / us * 1e-6, 1),
                    "frac_of_mfma_peak": round(flop / us * 1e-6 / 2500.0, 4), "peak_TFLOPs": 2500.0, "bound": "mfma",
                    "kernel_plan": ops.gemm_w4_plan(mm, nn, kk, gg, QT["any4_rowwise"], True, inner, torch.bfloat16, 1, "fast"),
                    "split_k_workspace_bytes": int(singles[0].workspace_bytes), "check_err_over_tol": round(err, 3),
                    "note": "one layer per launch, distinct weights per launch; the reference walks m in 16-row blocks (TinyGemmImpl.cuh:379-392), "
                            "this kernel dequantises once per 128-row tile; a 16-bit GEMM of the vendor library on the dequantised weights is an opt-in route (ANY4_LARGE_M_GEMM=library)"}

        many_rows = {} if world > 1 or not a.full else {"m64": many_rows_leg(64, n, k, g), "m128": many_rows_leg(128, n, k, g), "m512": many_rows_leg(512, n, k, g),
                                          "m2048": many_rows_leg(2048, n, k, g, layers=4)}

        # (c) single-layer launches: what one module forward issues (the reference's microbenchmark shape) -- Any4Linear's
        # default kernel (per-row LUT any4, weights on the B side) and Int4Linear's (modules.py:21: uniform int4, A side)
        def single_layer(qtype, on_right, tensors=None, m=m, n=n, k=k, layers=None):
            ww, xx, qq, ll, yy = tensors or make_batch(layers or L, m, n, k, g, inner, device, 91 + m, qtype, on_right)
            nl = ww.shape[0]
            sl = lambda t, i: None if t is None else t[i:i + 1]  # noqa: E731
            singles = [make_args(_lib, ww[i:i + 1], xx[i:i + 1], qq[i:i + 1], sl(ll, i), yy[i:i + 1], m, n, k, g, qtype, on_right, inner, 1,
                                 native=True) for i in range(nl)]
            for sa in singles:
                launch(sa)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for sa in singles:
                launch(sa)
            e1.record(stream)
            torch.cuda.synchronize()
            single_us = e0.elapsed_time(e1) * 1e3 / nl
            # cold single launch: one launch between two events, a different (cold) layer every time
            cold = []
            for i in range(0, nl, 8):
                c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                c0.record(stream)
                launch(singles[i])
                c1.record(stream)
                torch.cuda.synchronize()
                cold.append(c0.elapsed_time(c1) * 1e3)
            cold_us = sorted(cold)[len(cold) // 2]
            # the same launches replayed from one hipGraph (no per-launch host work: what the GPU needs per layer)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                cs = torch.cuda.current_stream().cuda_stream  # the capture stream
                for sa in singles:
                    _lib.check(lib.tg_gemm_w4(ctypes.byref(sa), local_rank, cs), "tg_gemm_w4 (graph capture)")
            gr.replay()
            torch.cuda.synchronize()
            e0.record(stream)
            for _ in range(5):
                gr.replay()
            e1.record(stream)
            torch.cuda.synchronize()
            graph_us = e0.elapsed_time(e1) * 1e3 / (5 * nl)
            bl = alg_bytes(m, n, k, g, qtype)
            return {"us_per_launch_back_to_back": round(single_us, 3), "GBps_back_to_back": round(bl / single_us / 1e3, 2),
                    "frac_back_to_back": round(bl / single_us / 1e3 / HBM_PEAK_GBPS, 4),
                    "us_cold_event_pair": round(cold_us, 3), "frac_cold": round(bl / cold_us / 1e3 / HBM_PEAK_GBPS, 4),
                    "us_per_launch_in_hipgraph": round(graph_us, 3), "frac_in_hipgraph": round(bl / graph_us / 1e3 / HBM_PEAK_GBPS, 4),
                    "kernel_plan": ops.gemm_w4_plan(m, n, k, g, QT[qtype], on_right, inner, torch.bfloat16, 1, "fast", weight_format="native")}

        full1 = a.full and world == 1
        single_b = single_layer("any4_rowwise", True, (w, x, sz, lut, y)) if full1 else {}
        single_a = single_layer("int4", False) if full1 else {}
        # ... and at a few rows (a prefill of a few tokens through the module; what the reference's microbenchmark.py:20-59 times)
        single_m8 = single_layer("any4_rowwise", True, m=8) if full1 else {}
        single_m16 = single_layer("any4_rowwise", True, m=16) if full1 else {}
        # ... and a gate+up-shaped layer (28672 x 4096, Llama-3-8B) at 16 rows: one workgroup per 64-row item on w4_gemm_xr_kernel
        single_m16_gate_up = single_layer("any4_rowwise", True, m=16, n=28672, k=4096, layers=16) if full1 and (n, k) == (4096, 4096) else {}
        # the host floor of the entry point: back-to-back launches of a 16 x 512 problem (5.9 KB) through the same C-ABI call
        floor_us = None
        if a.full:
            tw_, tx_, tq_, tl_, ty_ = make_batch(1, 1, 16, 512, g, inner, device, 5)
            tiny = make_args(_lib, tw_, tx_, tq_, tl_, ty_, 1, 16, 512, g, "any4_rowwise", True, inner, 1)
            for _ in range(20):
                launch(tiny)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(L):
                launch(tiny)
            e1.record(stream)
            torch.cuda.synchronize()
            floor_us = e0.elapsed_time(e1) * 1e3 / L

        # (d) BASELINE config 5 (TP = 1) and the live PMC traffic of the timed kernel; the bench tensors are released first
        decode = None
        if full1 and not a.no_decode:
            try:
                decode = decode_leg(device)
            except Exception as e:  # noqa: BLE001  (an informational leg must not take the metric line down with it)
                decode = {"error": f"{type(e).__name__}: {e}"}
        if not a.full:
            traffic, traffic_note = None, "not measured in a plain run (--full)"
        else:
            traffic, traffic_note = (None, "skipped (--no-pmc or N > 1)") if (a.no_pmc or world > 1) else pmc_traffic(L, bytes_step_rank)

        out = {
            "metric": "any4 W4A16 GEMM achieved GB/s (m=1, n=k=4096, g=128)",
            "value": round(value, 2),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "settle_steps": settle,
            "ms_per_step": round(ms_per_step, 5),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "workload": f"any4 W4A16 GEMV m={m} n={n_full} k={k} g={g} per-row LUT, Bint4 innerKTiles=4, default (group-scaled) numerics; "
                            f"one step = {L} independent layers (distinct cold weights) in one stacked launch"
                            + (f"; the {n_full} rows of every layer sharded over {world} ranks ({n} rows each, x replicated) + one gather of the layer batch's "
                               f"outputs per step ({exchange_kind})" if world > 1 else ""),
                "layers_per_step": L, "m": m, "n": n_full, "k": k, "group": g, "rows_per_rank": n, "exchange": exchange_kind,
                "x_scale": x_scale,  # activations = randn * this power of two (calibrate_x): max|y| in (0.95, 1.9]
                "algorithmic_bytes_per_layer": bytes_layer_full,
                "algorithmic_bytes_per_layer_per_rank": bytes_layer,
                "numerics": "TG_NUM_FAST (group-scaled: scale / zero applied per quantisation group to the f32 accumulator; the reference "
                            "rounds every dequantised weight to bf16 first, MatrixLayoutB.cuh:1042-1046 -- see `numerics_check` for the distance "
                            "and `reference_numerics` for the kernels with the reference's own arithmetic)",
            },
            # 3 layers x 256 rows of the TIMED launch's y against both CPU oracles (see check_layers)
            **({"numerics_check": main_check} if a.full else {}),
            "roofline": {
                "bound": "hbm",
                "kernel": {"pair": ("w4_gemm_xr_kernel<BF16> / w4_gemm_pair_kernel<BF16, I=4> (persistent work items, pair-table lookups, m = 1 contraction on the matrix core: "
                                    "v_mfma_f32_16x16x32_bf16 / 32x32x16_bf16, group-scaled accumulators)" if (m == 1 and lib.tg_m1_default_contraction() == 1) else
                                    "w4_gemm_pair_kernel<BF16, I=4> (persistent, 64-row work items, pair-table lookups, v_dot2 contraction at m = 1, group-scaled accumulators; "
                                    "the matrix-core contraction timed beside it, alternating: `m1_contraction_ab`)"),
                           "stream": "w4_gemm_stream_kernel<BF16, Bint4 innerK=4>", "splitk": "w4_gemm_kernel<BF16>"}[plan],
                "m1_default_contraction": {0: "v_dot2", 1: "mfma"}.get(int(lib.tg_m1_default_contraction())),
                "achieved": round(achieved, 2),
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBPS, 4),
                "traffic": traffic,
                "traffic_note": traffic_note,
                "launch_us": round(kern_ms * 1e3, 3),
                "bytes_per_launch": bytes_step_rank,
            },
        }
        if dumped is not None:
            out["dumped_outputs"] = dumped
        if a.full:
            out.update({
                "marginal": {
                    "us_per_layer": round(slope_us, 4),
                    "GBps": round(bytes_layer / slope_us / 1e3, 2),
                    "frac": round(bytes_layer / slope_us / 1e3 / HBM_PEAK_GBPS, 4),
                    "note": f"dT/dL between stacked launches of {L // 2} and {L} layers (launch overhead cancels)",
                },
                **legs,
                "single_layer_launch": {
                    **single_b,
                    "us_launch_floor_back_to_back": round(floor_us, 3),
                    "int4_a_side": single_a,
                    "m8": single_m8,
                    "m16": single_m16,
                    "m16_28672x4096": single_m16_gate_up,
                    "note": "one 4096x4096 GEMV per launch: top level = any4 per-row LUT, weights on the B side (what Any4Linear.forward issues); "
                            "int4_a_side = uniform int4, weights on the A side (Int4Linear's default kernel, modules.py:21); m8 / m16 = the top-level layer at 8 / 16 activation rows.  back_to_back = launches of "
                            "distinct cold layers on one stream (event time / launches); cold = median HIP-event time of an isolated launch (event pair "
                            "floor on this stack: ~4.3 us); in_hipgraph = the same launches replayed from one captured graph; launch_floor = a 16 x 512 "
                            "problem through the same entry point, back to back: the host/runtime cost per launch that back_to_back cannot go below",
                },
                "many_rows_gemm": many_rows,
                "decode_llama3_8b": decode,
            })
        if m1_ab is not None:
            out["m1_contraction_ab"] = m1_ab
        if world > 1:
            out["strong_scaling"] = {"value": round(value, 2), "unit": "GB/s", "ms_per_step": round(ms_per_step, 5), "exchange": exchange_kind,
                                     "rows_per_rank": n, "per_rank_roofline_frac": round(achieved / HBM_PEAK_GBPS, 4),
                                     "per_rank_kernel_us": round(kern_ms * 1e3, 3), **(strong_extra or {})}
            if weak is not None:
                out["weak_scaling"] = weak
        if exchange is not None:
            out["decode_shaped_exchange"] = exchange
        if full1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_torch(m, n, k, g)
            out["cpu_baseline_c_oracle"] = cpu_baseline_oracle(m, n, k, g)
        if full1:
            # the LAST key of the line: what a reader of its tail needs -- the metric's second point (m = 8), the other BASELINE
            # configs as fractions of the 8 TB/s HBM roofline, MFMA utilisation where the metric asks for it, the decode step
            fr = lambda name, sub=None: (legs.get(name, {}) if sub is None else legs.get(name, {}).get(sub, {})).get("frac")  # noqa: E731
            out["legs_summary"] = {
                "frac_of_hbm_roofline": {"m1": round(achieved / HBM_PEAK_GBPS, 4), "m1_mfma_contraction": fr("m1_mfma"), "m8": fr("m8"), "m16": fr("m16"), "config3": fr("config3"),
                                         "config3_reference_words": fr("config3_reference_words"), "int4": fr("int4"), "nf4": fr("nf4"),
                                         "mx4": fr("mx4"), "reference_numerics_m1": fr("reference_numerics", "m1"),
                                         "reference_numerics_m8": fr("reference_numerics", "m8")},
                "mfma_util_percent": None if a.no_pmc else pmc_mfma_util(),
                "single_layer_us": {"any4_b_side_back_to_back": single_b.get("us_per_launch_back_to_back"),
                                    "any4_b_side_per_graph_node": single_b.get("us_per_launch_in_hipgraph"),
                                    "int4_a_side_per_graph_node": single_a.get("us_per_launch_in_hipgraph"),
                                    "any4_m8_per_graph_node": single_m8.get("us_per_launch_in_hipgraph"),
                                    "any4_m16_per_graph_node": single_m16.get("us_per_launch_in_hipgraph"),
                                    "any4_m16_28672x4096_per_graph_node": single_m16_gate_up.get("us_per_launch_in_hipgraph")},
                "many_rows_us_per_4096x4096_layer": {kk_: vv_["us_per_layer"] for kk_, vv_ in many_rows.items()},
                "decode_llama3_8b": None if not decode or "error" in decode else
                {"ms_per_token": decode["ms_per_token"], "frac_of_hbm_roofline": decode["frac_of_hbm_roofline"],
                 "kernels_per_layer": decode["kernels_per_layer"]},
            }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
