"""Gradients of scales, zeros and LUT of a 4-bit linear (tg_gemm_w4_dq) against what a user could run instead, one layer per call,
Llama-3-8B shapes.

    python tools/dq_bench.py [--iters 10] [--rounds 3] [--m 512,2048,8192] [--out profiles/dq_bench.jsonl]

For each layer (out x in = 4096 x 4096, 14336 x 4096, 4096 x 14336; any4 row-wise LUT, groups of 128, Bint4 innerKTiles 4, bf16) and each m,
three things are timed ALTERNATING in one process (rounds x iters launches each, CUDA events, the median round reported):
  dq        (d_qinfo, d_lut) by the dq op (tinygemm_dq_f16RM_x_f16RM_w_any4TC): the binning GEMM and its finishing pass
  wgrad16   dY^T . x as a bf16 torch.matmul ALONE -- the FLOP floor of any route (it bins nothing)
  torch     what a user can write without the op: dY^T . x in f32, scatter_add of the [n][k] f32 matrix into [n][k / g][16] bins by the
            unpacked codes, then ds / dz / dlut from the bins
dq is cross-checked against the torch leg on every size timed.  One JSON object per line on stdout (and --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

LAYERS = [("4096x4096", 4096, 4096), ("14336x4096", 14336, 4096), ("4096x14336", 4096, 14336)]   # (name, out = weight rows, in = k)


def _time_alternating(fns, iters, rounds):
    """{name: median over rounds of the mean us per call}; the functions take turns round by round"""
    res = {name: [] for name in fns}
    for fn in fns.values():   # warm-up (workspaces, LDS attributes, the GEMM library's heuristics)
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
    from any4_amd import ops

    T = torch.ops.tinygemm
    dev = torch.device("cuda", torch.cuda.current_device())
    g = 128
    for name, n, k in LAYERS:
        gen = torch.Generator(device=dev).manual_seed(n * 7 + k)
        codes = torch.randint(0, 16, (n, k), dtype=torch.int32, device=dev, generator=gen)
        w = T.convert_matrix_to_m16n8k16_Bint4_layout(codes, 4)
        sz = torch.stack([torch.rand(k // g, n, device=dev, generator=gen) * 0.02 + 0.005,
                          torch.randn(k // g, n, device=dev, generator=gen) * 0.01], 2).bfloat16().contiguous()
        lut = torch.randn(n, 16, device=dev, generator=gen).bfloat16()
        idx = codes.long().view(n, k // g, g)
        del codes
        s32, l32 = sz[..., 0].float().t().contiguous(), lut.float()   # [n][k / g], [n][16]

        def by_torch(x, dy):
            G = dy.float().t() @ x.float()                                      # [n][k] f32: the matrix the kernel never writes
            H = torch.zeros(n, k // g, 16, device=dev).scatter_add_(2, idx, G.view(n, k // g, g))
            dq = torch.stack([(H * l32[:, None, :]).sum(2).t(), H.sum(2).t()], 2)
            return dq, (H * s32[:, :, None]).sum(1)

        for m in ms:
            dy = torch.randn(m, n, device=dev).bfloat16()
            x = torch.randn(m, k, device=dev).bfloat16()
            fns = {
                "dq": lambda: T.tinygemm_dq_f16RM_x_f16RM_w_any4TC(x, dy, w, g, sz, lut, True),
                "wgrad16": lambda: torch.matmul(dy.t(), x),
                "torch": lambda: by_torch(x, dy),
            }
            got, want = fns["dq"](), fns["torch"]()
            errs = [float(((a - b).abs().max() / b.abs().max()).item()) for a, b in zip(got, want)]
            assert max(errs) < 1e-3, f"dq op disagrees with the torch evaluation: {errs}"
            t = _time_alternating(fns, iters, rounds)
            emit({"what": "layer", "layer": name, "wrows": n, "k": k, "m": m, **{f"{a}_us": round(b, 2) for a, b in t.items()},
                  "dq_over_wgrad16": round(t["dq"] / t["wgrad16"], 3), "dq_over_torch": round(t["dq"] / t["torch"], 3),
                  "dq_tflops": round(2 * m * n * k / t["dq"] / 1e6, 1), "max_rel_diff_d_qinfo": errs[0], "max_rel_diff_d_lut": errs[1],
                  "dq_workspace_bytes": ops._WS_BYTES.get(("w4_dq", n, k, g, ops.TG_Q_ANY4_ROWWISE, 0, 1, 4, 0))})
        del idx, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--m", default="512,2048,8192")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import tinygemm  # noqa: F401

    out = open(a.out, "w") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit({"what": "device", "name": torch.cuda.get_device_name(), "torch": torch.__version__})
    bench_layers([int(v) for v in a.m.split(",")], a.iters, a.rounds, emit)


if __name__ == "__main__":
    main()
