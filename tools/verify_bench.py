"""Timing of the speculative-decoding verify pass on an MI355X:  python tools/verify_bench.py [--skip-stack] [--layers N]

Kernel leg   dg_verify_attn against dg_prefill_attn_seq on the SAME call (Llama-3-8B geometry: 32 query / 8 kv heads of 128, cache of
             8192 positions), T = 2 / 4 / 8, bs = 1 / 8, positions near 512 / 4096 / 8190; nsplit by DecodeStack's rule.
Stack leg    one eager and one captured `DecodeStack.verify` pass at T = 4 / 8 against the captured decode step of the same stack, in ms per
             pass, and the break-even acceptance it implies: a pass that keeps `a` drafts emits a + 1 tokens, so it pays (the drafter's
             own cost aside) from a > t_verify / t_decode - 1.

Protocol: the legs alternate in one process; a window is LAUNCHES back-to-back launches between two device events; every figure is the
median of REPEATS windows with the spread (min ... max).  One JSON line per configuration goes to profiles/verify_bench.jsonl."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAUNCHES, REPEATS = 50, 9
DEV = "cuda:0"


def window(fn, launches=LAUNCHES):
    """microseconds per launch of `launches` launches between two device events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / launches


def alternate(legs, launches=LAUNCHES):
    """{name: (median, min, max)} in microseconds: every leg warmed up, then REPEATS rounds of one window per leg"""
    for fn in legs.values():
        window(fn, 5)
    times = {name: [] for name in legs}
    for _ in range(REPEATS):
        for name, fn in legs.items():
            times[name].append(window(fn, launches))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def kernel_leg(emit):
    from any4_amd import decode_ops as G
    from any4_amd.decode import DecodeConfig, _rope_tables

    hl, kvl, d, S = 32, 8, 128, 8192
    cos, sin = _rope_tables(DecodeConfig(head_dim=d, max_seq=S), DEV)
    gen = torch.Generator(device=DEV).manual_seed(0)
    for bs in (1, 8):
        kc = torch.randn(bs, kvl, S, d, device=DEV, generator=gen).bfloat16()
        vc = torch.randn(bs, kvl, S, d, device=DEV, generator=gen).bfloat16()
        nsplit = max(1, min(8, 256 // (bs * kvl)))
        for T in (2, 4, 8):
            qkv = torch.randn(bs * T, (hl + 2 * kvl) * d, device=DEV, generator=gen).bfloat16()
            scratch = G.verify_attn_scratch(bs, hl, d, T, nsplit, DEV)
            o1, o2 = torch.empty(bs * T, hl * d, device=DEV, dtype=torch.bfloat16), torch.empty(bs * T, hl * d, device=DEV, dtype=torch.bfloat16)
            for near in (512, 4096, 8190):
                pos = torch.full((bs,), min(near, S - T), dtype=torch.long, device=DEV)
                legs = {
                    "verify": lambda: G.verify_attn(qkv, cos, sin, pos, kc, vc, hl, kvl, d, 1 / math.sqrt(d), T, nsplit, scratch, out=o1),
                    "prefill": lambda: G.prefill_attn(qkv, cos, sin, pos, kc, vc, hl, kvl, d, 1 / math.sqrt(d), T, out=o2, per_sequence=True),
                }
                r = alternate(legs)
                torch.cuda.synchronize()
                diff = (o1.float() - o2.float()).abs().max().item()
                emit(dict(leg="kernel", bs=bs, T=T, pos=int(pos[0]), nsplit=nsplit, launches=LAUNCHES, repeats=REPEATS,
                          verify_us=r["verify"], prefill_us=r["prefill"], speedup=r["prefill"][0] / r["verify"][0], max_abs_diff=diff))


def stack_leg(emit, layers):
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig.llama3_8b(max_seq=8192, layers=layers)
    stack = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=0), DEV, bs=1, ragged=True)
    p0 = 4096
    stack.decode(torch.zeros(1, dtype=torch.long, device=DEV), [p0])
    stack.capture()
    graph = stack._graph
    for T in (4, 8):
        toks = torch.zeros(1, T, dtype=torch.long, device=DEV)
        stack.verify(toks, [p0])  # (makes the scratch, fills the position buffers)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            stack.verify(toks, None)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                stack.verify(toks, None)
        torch.cuda.current_stream().wait_stream(side)
        r = alternate({"decode_graph": graph.replay, "verify_eager": lambda: stack.verify(toks, None), "verify_graph": g.replay}, launches=10)
        ms = {k: tuple(x / 1e3 for x in v) for k, v in r.items()}
        emit(dict(leg="stack", layers=layers, bs=1, T=T, pos=p0, nsplit=stack._verify_split, launches=10, repeats=REPEATS,
                  decode_graph_ms=ms["decode_graph"], verify_eager_ms=ms["verify_eager"], verify_graph_ms=ms["verify_graph"],
                  break_even_accepted=ms["verify_graph"][0] / ms["decode_graph"][0] - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-stack", action="store_true")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("verify_bench.py measures on a GPU; there is none")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        kernel_leg(emit)
        if not a.skip_stack:
            stack_leg(emit, a.layers)


if __name__ == "__main__":
    main()
