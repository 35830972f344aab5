"""Input-gradient GEMM of a 4-bit linear (tg_gemm_w4_dx) against what a user could run instead, one layer per call, Llama-3-8B shapes.

    python tools/dx_bench.py [--iters 50] [--rounds 5] [--m 16,128,512,2048] [--out FILE.jsonl]

For each layer (out x in = 4096 x 4096, 14336 x 4096, 4096 x 14336; any4 row-wise LUT, groups of 128, Bint4 innerKTiles 4, bf16) and each m,
four things are timed ALTERNATING in one process (rounds x iters launches each, CUDA events, the median round reported):
  dx        dX = dY . W by the dx op (tinygemm_dx_f16RM_dy_f16RM_w_any4TC)
  fwd       the forward op of the same layer at m rows (the LDS-tiled tile GEMM, plan 'tile')
  deq_mm    tg_dequant_w4 (ops.dequant_w4) + torch.matmul(dY, W)
  dense     torch.matmul(dY, W) on a dense bf16 copy of the weights
dx is cross-checked against deq_mm on every size timed.  Then the eager forward of one Any4Linear (4096 x 4096, bias) at 16 / 512 rows, in grad
mode (the bias is a Parameter: the autograd path) and under no_grad, host-inclusive (launch + Python), per call.
One JSON object per line on stdout (and --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

# --root DIR: import the library from another checkout (e.g. the parent commit, built) -- the module timing before / after a change
_ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(_ROOT))

import torch  # noqa: E402

LAYERS = [("4096x4096", 4096, 4096), ("14336x4096", 14336, 4096), ("4096x14336", 4096, 14336)]   # (name, out = weight rows, in = k)


def _layer(n, k, g, dev):
    from any4_amd import ops

    gen = torch.Generator(device=dev).manual_seed(n * 7 + k)
    codes = torch.randint(0, 16, (n, k), dtype=torch.int32, device=dev, generator=gen)
    w = torch.ops.tinygemm.convert_matrix_to_m16n8k16_Bint4_layout(codes, 4)
    sz = torch.stack([torch.rand(k // g, n, device=dev, generator=gen) * 0.02 + 0.005,
                      torch.randn(k // g, n, device=dev, generator=gen) * 0.01], 2).bfloat16().contiguous()
    lut = torch.randn(n, 16, device=dev, generator=gen).bfloat16()
    return w, sz, lut, ops


def _time_alternating(fns, iters, rounds):
    """{name: median over rounds of the mean us per call}; the functions take turns round by round"""
    res = {name: [] for name in fns}
    for fn in fns.values():   # warm-up (plans, workspaces, LDS attributes)
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            res[name].append(a.elapsed_time(b) * 1e3 / iters)
    return {name: statistics.median(v) for name, v in res.items()}


def bench_layers(ms, iters, rounds, emit):
    T = torch.ops.tinygemm
    dev = torch.device("cuda", torch.cuda.current_device())
    g = 128
    for name, n, k in LAYERS:
        w, sz, lut, ops = _layer(n, k, g, dev)
        wd = ops.dequant_w4(w, sz, lut, g, ops.TG_Q_ANY4_ROWWISE, k, 4, n)   # [n][k] dense bf16 copy, the reference's weights
        for m in ms:
            dy = torch.randn(m, n, device=dev).bfloat16()
            x = torch.randn(m, k, device=dev).bfloat16()
            fns = {
                "dx": lambda: T.tinygemm_dx_f16RM_dy_f16RM_w_any4TC(dy, w, g, sz, lut, True),
                "fwd": lambda: T.tinygemm_y_f16RM_x_f16RM_w_any4TC(x, w, g, sz, lut, True),
                "deq_mm": lambda: torch.matmul(dy, ops.dequant_w4(w, sz, lut, g, ops.TG_Q_ANY4_ROWWISE, k, 4, n)),
                "dense": lambda: torch.matmul(dy, wd),
            }
            got = fns["dx"]().float()
            want = fns["deq_mm"]().float()
            ref = (dy.double() @ wd.double()).float()
            err_dx = float(((got - ref).abs().max() / ref.abs().max()).item())
            err_mm = float(((want - ref).abs().max() / ref.abs().max()).item())
            assert err_dx < 2e-2, f"dx op disagrees with the dense product: {err_dx}"
            t = _time_alternating(fns, iters, rounds)
            emit({"what": "layer", "layer": name, "wrows": n, "k": k, "m": m, **{f"{a}_us": round(b, 2) for a, b in t.items()},
                  "dx_over_fwd": round(t["dx"] / t["fwd"], 3), "dx_tflops": round(2 * m * n * k / t["dx"] / 1e6, 1),
                  "max_rel_err_dx": err_dx, "max_rel_err_deq_mm": err_mm,
                  "dx_workspace_bytes": ops._WS_BYTES.get(("w4_dx", m, n, k, g, ops.TG_Q_ANY4_ROWWISE, 0, 1, 4, dev.index))})


def bench_module(iters, rounds, emit):
    import modules

    dev = torch.device("cuda", torch.cuda.current_device())
    n = k = 4096
    mod = modules.Any4Linear(k, n, bias=True, device=dev, dtype=torch.bfloat16, group_size=128, kernel="linear_y_f16RM_x_f16RM_W_any4TC")
    mod.weight.data = torch.randint(0, 16, (n, k), dtype=torch.int32, device=dev)
    mod.scales_and_zeros.data = (torch.rand(k // 128, n, 2, device=dev) * 0.01).bfloat16()
    mod.lut.data = torch.randn(n, 16, device=dev).bfloat16()
    mod.bias.data = torch.randn(n, device=dev).bfloat16()
    mod.reshape_weight()
    for m in (16, 512):
        x = torch.randn(m, k, device=dev).bfloat16()
        with torch.no_grad():
            y0 = mod(x)
        y1 = mod(x)
        assert torch.equal(y0, y1.detach())
        for mode in ("no_grad", "grad"):
            per = []
            for _ in range(rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if mode == "no_grad":
                    with torch.no_grad():
                        for _ in range(iters):
                            mod(x)
                else:
                    for _ in range(iters):
                        mod(x)
                torch.cuda.synchronize()
                per.append((time.perf_counter() - t0) * 1e6 / iters)
            emit({"what": "module_forward", "module": "Any4Linear 4096x4096 bias", "m": m, "mode": mode, "us_per_call": round(statistics.median(per), 2)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--m", default="16,128,512,2048")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-module", action="store_true")
    ap.add_argument("--module-only", action="store_true")
    ap.add_argument("--root", default=None, help="checkout to import the library from (default: this one)")
    a = ap.parse_args()
    import tinygemm  # noqa: F401

    out = open(a.out, "w") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit({"what": "device", "name": torch.cuda.get_device_name(), "torch": torch.__version__, "root": os.path.basename(os.path.abspath(_ROOT))})
    if not a.module_only:
        bench_layers([int(v) for v in a.m.split(",")], a.iters, a.rounds, emit)
    if not a.no_module:
        bench_module(a.iters * 4, a.rounds, emit)


if __name__ == "__main__":
    main()
