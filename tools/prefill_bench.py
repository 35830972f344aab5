"""Prompt prefill: the prefill kernel (DG_ATTN_PREFILL of dg_attn_launch) at the kernel level and DecodeStack.prefill at the stack level.  Needs a GPU.

    python tools/prefill_bench.py [--kernel] [--stack] [--config llama3_8b] [--baseline] [--profile] [--iters 20] [--rounds 5]

Kernel level (--kernel): Llama-3-8B heads (32 / 8 x 128) and Llama-2 heads (32 / 32 x 128), bs = 1, bf16, max_seq 4096, T = 128 / 512 /
2048 / 4096 at p0 = 0 and the chunked case T = 2048 at p0 = 2048.  Two legs ALTERNATING in one process (rounds x iters launches each, CUDA
events, the median round reported):
  prefill_attn  decode_ops.prefill_attn (rope + cache append + causal flash attention, two launches)
  sdpa          what torch offers for the same step: rope of q and k with the table rows, index_copy_ of the T rows into the caches,
                torch.nn.functional.scaled_dot_product_attention over cache[:, :, :p0 + T] (is_causal=True at p0 = 0, a mask otherwise)
TFLOP/s counts 4 d hl (number of unmasked (t, s) pairs); `peak_frac` is against the 2.5 PFLOP/s bf16 MFMA peak.
Stack level (--stack): time to first token of `DecodeStack.prefill` for T = 128 / 512 / 2048 (Any4Factory, or DenseFactory with
--baseline), and -- the only way to ingest a prompt without prefill -- the same prompt fed token by token through the captured decode
graph, alternating with the prefill leg at T = 512.  --profile re-runs one prefill per T under `rocprofv3 --kernel-trace --stats` in a
child process and splits its device time into GEMM / attention / glue (RMSNorm, SwiGLU) / other (profiles/prefill_kernel_stats.csv).
One JSON object per line on stdout and in profiles/prefill_bench.jsonl.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import math
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_BF16 = 2.5e15
HEADS = [("llama3_8b", 32, 8, 128), ("llama2_7b", 32, 32, 128)]
KERNEL_CASES = [(128, 0), (512, 0), (2048, 0), (4096, 0), (2048, 2048)]


def _time_alternating(fns, iters, rounds):
    """{name: median over rounds of the mean us per call}; the functions take turns round by round"""
    res = {name: [] for name in fns}
    for fn in fns.values():
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


def bench_kernel(iters, rounds, emit):
    from any4_amd import decode_ops as G
    from any4_amd.decode import DecodeConfig, _rope, _rope_tables

    dev, dtype, S = torch.device("cuda", torch.cuda.current_device()), torch.bfloat16, 4096
    F = torch.nn.functional
    for name, hl, kvl, d in HEADS:
        cos, sin = _rope_tables(DecodeConfig(head_dim=d, max_seq=S), dev)
        scale, rep = 1.0 / math.sqrt(d), hl // kvl
        kc = torch.randn(1, kvl, S, d, device=dev).to(dtype)
        vc = torch.randn(1, kvl, S, d, device=dev).to(dtype)
        for T, p0 in KERNEL_CASES:
            qkv = torch.randn(T, (hl + 2 * kvl) * d, device=dev).to(dtype)
            pos = torch.tensor([p0], device=dev)
            rows = torch.arange(p0, p0 + T, device=dev)
            mask = None if p0 == 0 else (torch.arange(p0 + T, device=dev).view(1, -1) <= rows.view(-1, 1))
            out = torch.empty(T, hl * d, device=dev, dtype=dtype)

            def ours():
                return G.prefill_attn(qkv, cos, sin, pos, kc, vc, hl, kvl, d, scale, T, out=out)

            def sdpa():
                c, s_ = cos[p0:p0 + T].view(1, T, 1, d), sin[p0:p0 + T].view(1, T, 1, d)
                q = _rope(qkv[:, : hl * d].reshape(1, T, hl, d), c, s_).transpose(1, 2)
                k = _rope(qkv[:, hl * d:(hl + kvl) * d].reshape(1, T, kvl, d), c, s_)
                kc.index_copy_(2, rows, k.transpose(1, 2))
                vc.index_copy_(2, rows, qkv[:, (hl + kvl) * d:].reshape(1, T, kvl, d).transpose(1, 2))
                kk, vv = kc[:, :, :p0 + T], vc[:, :, :p0 + T]
                if rep > 1:
                    kk, vv = kk.repeat_interleave(rep, dim=1), vv.repeat_interleave(rep, dim=1)
                o = F.scaled_dot_product_attention(q, kk, vv, attn_mask=mask, is_causal=mask is None, scale=scale)
                return o.transpose(1, 2).reshape(T, hl * d)

            a, b = ours().float(), sdpa().float()
            err = float((a - b).abs().max() / b.abs().max())
            assert err < 3e-2, f"prefill_attn disagrees with scaled_dot_product_attention: {err}"
            t = _time_alternating({"prefill_attn": ours, "sdpa": sdpa}, iters, rounds)
            flop = 4.0 * d * hl * (T * p0 + T * (T + 1) / 2)
            emit({"what": "kernel", "heads": name, "hl": hl, "kvl": kvl, "d": d, "bs": 1, "T": T, "p0": p0, "max_seq": S,
                  "prefill_attn_us": round(t["prefill_attn"], 1), "sdpa_rope_cache_us": round(t["sdpa"], 1),
                  "tflops": round(flop / t["prefill_attn"] / 1e6, 1), "peak_frac": round(flop / (t["prefill_attn"] * 1e-6) / PEAK_BF16, 4),
                  "speedup_vs_sdpa": round(t["sdpa"] / t["prefill_attn"], 2), "max_rel_diff_vs_sdpa": err})


def _build_stack(config, baseline, max_seq):
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack, DenseFactory

    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = getattr(DecodeConfig, config)(max_seq=max_seq)
    fac = DenseFactory(cfg, dev) if baseline else Any4Factory(cfg, dev)
    return cfg, DecodeStack(cfg, fac, dev, bs=1)


def bench_stack(config, baseline, rounds, emit, max_seq=2048):
    cfg, stack = _build_stack(config, baseline, max_seq)
    dev = stack.pos.device
    toks = torch.randint(0, cfg.vocab, (1, 2048), device=dev)
    linears = "dense" if baseline else "any4"
    for T in (128, 512, 2048):
        t = _time_alternating({"prefill": lambda: stack.prefill(toks[:, :T])}, 3, rounds)
        emit({"what": "stack_ttft", "config": config, "linears": linears, "bs": 1, "T": T, "prefill_ms": round(t["prefill"] / 1e3, 3)})
    # the parent's only way to ingest a prompt: T replays of the captured one-token graph
    stack.capture()
    T = 512

    def token_by_token():
        for i in range(T):
            stack.decode(toks[:, i], i)

    t = _time_alternating({"prefill": lambda: stack.prefill(toks[:, :T]), "token_by_token": token_by_token}, 1, rounds)
    emit({"what": "stack_vs_token_by_token", "config": config, "linears": linears, "bs": 1, "T": T,
          "prefill_ms": round(t["prefill"] / 1e3, 3), "token_by_token_graph_ms": round(t["token_by_token"] / 1e3, 3),
          "speedup": round(t["token_by_token"] / t["prefill"], 1)})


def profile_child(config, baseline, T):
    """Two identical prefills under the profiler (the parent halves the per-kernel totals)."""
    cfg, stack = _build_stack(config, baseline, 2048)
    toks = torch.randint(0, cfg.vocab, (1, T), device=stack.pos.device)
    for _ in range(2):
        stack.prefill(toks)
    torch.cuda.synchronize()


def _family(kernel):
    k = kernel.lower()
    if "prefill_attn" in k or "prefill_rope" in k:
        return "attention"
    if "gemm" in k or "cijk" in k or "linear16" in k:
        return "gemm"
    if "add_rmsnorm" in k or "swiglu" in k:
        return "glue"
    return "other"  # torch's own kernels: embedding gather, copies, and the traced process's one-off random weight initialisation


def bench_profile(config, baseline, emit):
    prof = shutil.which("rocprofv3")
    if prof is None:
        emit({"what": "stack_split", "skipped": "rocprofv3 not found"})
        return
    rows_out = []
    for T in (128, 512, 2048):
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   "--profile-child", str(T), "--config", config] + (["--baseline"] if baseline else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if r.returncode != 0 or not files:
                emit({"what": "stack_split", "T": T, "skipped": f"rocprofv3 pass failed (rc {r.returncode})", "stderr": r.stderr[-300:]})
                continue
            split = {"gemm": 0.0, "attention": 0.0, "glue": 0.0, "other": 0.0}
            with open(files[0]) as f:
                for row in csv.DictReader(f):
                    ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
                    split[_family(row["Name"])] += ns / 2  # two identical prefills were traced
                    rows_out.append({"T": T, "family": _family(row["Name"]), **row})
            emit({"what": "stack_split", "config": config, "linears": "dense" if baseline else "any4", "T": T,
                  **{f"{k}_ms": round(v / 1e6, 3) for k, v in split.items()},
                  "note": "device time per prefill; `other` = torch's own kernels incl. the one-off weight initialisation of the traced process"})
    if rows_out:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "prefill_kernel_stats.csv"), "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows_out[0].keys()), extrasaction="ignore")
            w.writeheader()
            w.writerows(rows_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--stack", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--config", default="llama3_8b", choices=["llama3_8b", "llama2_7b"])
    ap.add_argument("--baseline", action="store_true", help="DenseFactory (bf16 nn.Linear) instead of Any4Factory")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_bench.jsonl"))
    ap.add_argument("--profile-child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.profile_child is not None:
        profile_child(a.config, a.baseline, a.profile_child)
        return
    if not (a.kernel or a.stack or a.profile):
        a.kernel = a.stack = True
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    emit({"what": "device", "name": torch.cuda.get_device_name(), "torch": torch.__version__})
    if a.kernel:
        bench_kernel(a.iters, a.rounds, emit)
    if a.stack:
        bench_stack(a.config, a.baseline, a.rounds, emit)
    if a.profile:
        bench_profile(a.config, a.baseline, emit)


if __name__ == "__main__":
    main()
