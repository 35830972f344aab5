"""MX4 x MXFP8 (MX4Linear(activations="mx8"): quantise launch + tg_gemm_mx4a8) against the same MX4Linear on the W4A16 kernels and a bf16
nn.Linear, one layer per call.  At m <= 64 a fourth leg: ops.gemm_mx4_a8(kernel="rows") on the module's operands, i.e. quantise launch +
tg_gemm_mx4a8_rows at every m <= 64, also where small_batch=True would take the tile kernel (`w4a8_rows`; `rows_weight_gbps` = the packed weights' bytes out * in / 2 over that leg's time, quantise launch
included: against the 8 TB/s of the part).

    python tools/mx4a8_bench.py [--iters 200] [--rounds 5] [--runs 3] [--m 1,4,8,16,32,64,128,512,2048] [--out profiles/mx4a8_bench.jsonl]

Layers out x in = 4096 x 4096, 14336 x 4096 and 4096 x 14336, bf16.  The paths are timed ALTERNATING in one process: per run `rounds` rounds of
`iters` back-to-back calls each between two device events (200 calls: a window of 6 - 100 ms; no cache flush: a prefill layer's weights
are re-read from where the last call left them on every path alike), the median round is the run's figure; `runs` runs -- repeats inside
this one process, after one warm-up -- give the median and the spread (max - min) that the comparison is held against.  `rel_err`:
|y_w4a8 - y_w4a16| / |y_w4a16| (Frobenius) on randn activations and the same weights: what the 8-bit activations cost.  One JSON object
per line on stdout and in --out.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

LAYERS = [("4096x4096", 4096, 4096), ("14336x4096", 14336, 4096), ("4096x14336", 4096, 14336)]   # (name, out, in)


def _round_us(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--m", default="1,4,8,16,32,64,128,512,2048")
    ap.add_argument("--out", default=os.path.join("profiles", "mx4a8_bench.jsonl"))
    a = ap.parse_args()
    from any4_amd import modules, ops, utils

    dev = torch.device("cuda")
    lines = []
    for name, n, k in LAYERS:
        gen = torch.Generator().manual_seed(n + k)
        codes, exps = utils.quantize_mx4(torch.randn(n, k, generator=gen), 32)
        lins = {}
        for key, act in (("w4a8", "mx8"), ("w4a16", None)):
            lin = modules.MX4Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16, activations=act)
            lin.weight.data, lin.exponents.data = codes.to(dev), exps.to(dev)
            lin.reshape_weight(4)
            lins[key] = lin
        dense = torch.nn.Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)
        dense.weight.data = utils.dequantize_mx4(codes, exps).bfloat16().to(dev)
        for m in [int(v) for v in a.m.split(",")]:
            x = torch.randn(m, k, generator=gen).bfloat16().to(dev)
            with torch.no_grad():
                paths = {"w4a8": lambda: lins["w4a8"](x), "w4a16": lambda: lins["w4a16"](x), "bf16": lambda: dense(x)}
                if m <= 64:
                    paths["w4a8_rows"] = lambda: ops.gemm_mx4_a8(x, lins["w4a8"].weight, lins["w4a8"].exponents, True, None, kernel="rows")
                y8, y16 = paths["w4a8"]().float(), paths["w4a16"]().float()
                rel = float((y8 - y16).norm() / y16.norm())
                for f in paths.values():   # warm-up: every path, this shape
                    for _ in range(5):
                        f()
                torch.cuda.synchronize()
                runs = {p: [] for p in paths}
                for _ in range(a.runs):
                    rounds = {p: [] for p in paths}
                    for _ in range(a.rounds):
                        for p, f in paths.items():
                            rounds[p].append(_round_us(f, a.iters))
                    for p in paths:
                        runs[p].append(statistics.median(rounds[p]))
            rec = {"layer": name, "m": m, "rel_err_vs_w4a16": round(rel, 5)}
            for p in paths:
                rec[p + "_us"] = round(statistics.median(runs[p]), 2)
                rec[p + "_spread_us"] = round(max(runs[p]) - min(runs[p]), 2)
            if m <= 64:
                rec["rows_weight_gbps"] = round(n * k / 2 / rec["w4a8_rows_us"] / 1e3, 1)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
