"""The any4 quantizer's clustering step: the fused k-means kernel (anyq_quantize_tensor(fused=True), tg_kmeans_rows) against the batched
torch Lloyd of the same checkout (fused=False), one linear per call, Llama-3-8B shapes.

    python tools/quantize_bench.py [--rounds 3] [--seed 0] [--layers 6144x4096,4096x4096] [--out profiles/kmeans_bench.jsonl]

For the four linears of a layer (out x in = 6144 x 4096, 4096 x 4096, 28672 x 4096, 4096 x 14336; bf16 weights from a seed, groups of
128), unweighted and with a [k] sample weight (rand^4 + 1e-3), `anyq_quantize_tensor` is timed with fused=False and fused=True
ALTERNATING in one process: each leg warmed once, then `rounds` rounds, a synchronised host clock around the call.  Per leg:
  ms                 the rounds' wall times of the whole call (group_q, weights, seeding, clustering, casts)
  peak_bytes         torch.cuda.max_memory_allocated over the call, above what was allocated before it (W itself excluded)
  kernel_ms          fused only: the tg_kmeans_rows launch alone (device events); torch_fraction = 1 - kernel_ms / ms: what of the
                     fused call is still torch (group_q, the sort and the three seedings)
  iters_mean / _max  fused only: Lloyd iterations per row, summed over the three seedings
  mse, mse_ratio     reconstruction MSE against W; fused / torch
GPU only, reads nothing outside the tree.  One JSON object per line on stdout (and --out); a verdict line per shape:
fused faster than torch by more than the spread of the rounds (slowest fused round < fastest torch round), and lower peak bytes.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

LAYERS = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]   # (out = weight rows, in = k): qkv, o, gate_up, down
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--layers", default=",".join(f"{n}x{k}" for n, k in LAYERS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "quantize_bench.py needs a GPU"
    from any4_amd import quantize as Q

    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    # the launch alone, by device events: a wrapper around the one function that makes it
    launch, seen = Q.kmeans_rows_launch, {}

    def timed_launch(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = launch(*a, **kw)
        e1.record()
        seen["events"], seen["iters"] = (e0, e1), res[3]
        return res

    Q.kmeans_rows_launch = timed_launch
    mse = lambda w_hat, W: float(((w_hat.float() - W.float()) ** 2).mean())
    ok_all = True
    for spec in args.layers.split(","):
        n, k = (int(v) for v in spec.split("x"))
        gen = torch.Generator(device=DEV).manual_seed(args.seed + n + k)
        W = (torch.randn(n, k, device=DEV, generator=gen) * 0.02).to(torch.bfloat16)
        for weighted in (False, True):
            sw = (torch.rand(k, device=DEV, generator=gen) ** 4 + 1e-3) if weighted else None
            legs = {"torch": dict(fused=False), "fused": dict(fused=True)}
            rec = {name: dict(layer=f"{n}x{k}", group=args.group, weighted=weighted, path=name, ms=[], peak_bytes=0) for name in legs}

            def run(name):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                res = Q.anyq_quantize_tensor(W, n_bit=4, q_group_size=args.group, sample_weight=sw, **legs[name])
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                return res, dt, torch.cuda.max_memory_allocated() - base

            for name in legs:   # warm-up: allocator, LDS attribute, the divisor tensors
                res, _, _ = run(name)
                rec[name]["mse"] = mse(Q.anyq_dequantize_tensor(*res, q_group_size=args.group), W)
                del res
            for _ in range(args.rounds):
                for name in legs:
                    res, dt, peak = run(name)
                    del res
                    rec[name]["ms"].append(round(dt, 3))
                    rec[name]["peak_bytes"] = max(rec[name]["peak_bytes"], peak)
                    if name == "fused":
                        e0, e1 = seen["events"]
                        rec[name].setdefault("kernel_ms_rounds", []).append(round(e0.elapsed_time(e1), 3))
                        rec[name]["iters_mean"] = round(float(seen["iters"].float().mean()), 2)
                        rec[name]["iters_max"] = int(seen["iters"].max())
            for name in legs:
                rec[name]["ms_median"] = statistics.median(rec[name]["ms"])
            f = rec["fused"]
            f["kernel_ms"] = statistics.median(f.pop("kernel_ms_rounds"))
            f["torch_fraction"] = round(1.0 - f["kernel_ms"] / f["ms_median"], 3)
            f["mse_ratio"] = round(f["mse"] / rec["torch"]["mse"], 5)
            f["speedup"] = round(rec["torch"]["ms_median"] / f["ms_median"], 2)
            f["peak_ratio"] = round(f["peak_bytes"] / max(rec["torch"]["peak_bytes"], 1), 3)
            ok = max(f["ms"]) < min(rec["torch"]["ms"]) and f["peak_bytes"] < rec["torch"]["peak_bytes"]
            f["accepted"] = ok
            ok_all &= ok
            emit(rec["torch"])
            emit(f)
            print(f"# {n}x{k} weighted={weighted}: torch {rec['torch']['ms_median']:.1f} ms, fused {f['ms_median']:.1f} ms (kernel {f['kernel_ms']:.1f} ms) "
                  f"= {f['speedup']} x; peak bytes x {f['peak_ratio']}; MSE x {f['mse_ratio']}; {'ok' if ok else 'NOT faster beyond the spread / not smaller'}",
                  flush=True)
        del W
        torch.cuda.empty_cache()
    Q.kmeans_rows_launch = launch
    print("# all shapes: " + ("fused faster beyond the spread and smaller" if ok_all else "acceptance NOT met at every shape"))
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
