#!/usr/bin/env python3
"""Model-level decode benchmark (BASELINE config 5; counterpart of the reference's benchmark.py:113-215).

    python tools/llama_decode_bench.py --config llama3_8b --baseline
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29511 \
        tools/llama_decode_bench.py --config llama3_8b                   # TP=8, rows sharded, RCCL all-gathers

Random-initialised weights of the named architecture (no checkpoints here), random token ids, one new token per
sequence per step over a static KV cache.  Prints one JSON line on rank 0: ms per token, tokens/s, and the rate at which
the 4-bit weights stream (algorithmic bytes of the quantized linears / step time).

    python tools/llama_decode_bench.py --config llama3_8b --ragged [--out profiles/ragged_bench.jsonl]

--ragged (one GPU): what a position per sequence costs and buys, one JSON line per leg, appended to --out:
  (a) the captured step of a ragged and a non-ragged stack at equal positions, bs = 1 / 4 / 8, alternating in one process;
  (b) eight prompts of 16 ... 512 tokens through `generate(list)` on one ragged bs = 8 stack against the only route there is without
      it, eight bs = 1 `generate` runs one after the other; tokens/s of the new tokens.

    python tools/llama_decode_bench.py --config llama3_8b --kv-cache mx8 [--ragged] [--out profiles/kv8_bench.jsonl]

--kv-cache mx8 (one GPU): the block-scaled 8-bit KV cache against the 16-bit one, one JSON line per leg, appended
to --out: the caches' bytes, and the captured step of a 16-bit-cache stack and an mx8-cache stack, alternating in one process, at
bs = 1 and 8 with the position near 512, 4096 and the end of an 8192-position cache.  With --ragged: leg (b) above on a 16-bit and on
an mx8 ragged bs = 8 stack.

    python tools/llama_decode_bench.py --config llama3_8b --kv-cache mx8 --mx8-attention online [--out profiles/kv8_online_bench.jsonl]

--mx8-attention online (with --kv-cache mx8; one GPU): the one-barrier kernel's 8-bit flavour ("the one-barrier
kernel on mx8 rows"): THREE captured steps in one process -- 16-bit cache, mx8 cache with mx8_attention="split", mx8 cache with
mx8_attention="online" -- alternating five times (the order rotates), 30 steps after 10 warm-up steps each, at bs = 1 and 8 with the
position near 512, 4096 and the end of an 8192-position cache; one JSON line per (bs, position) cell, appended to --out.

    python tools/llama_decode_bench.py --config llama3_8b --paged [--out profiles/paged_bench.jsonl]

--paged (one GPU): the paged KV cache against the contiguous one, one JSON line per leg, appended to --out:
  (a) the captured step of a paged ragged stack (64-position pages, every page mapped up front, in reverse physical order) and of the
      contiguous ragged stack, alternating in one process, at bs = 1 and 8 with the position near 512, 4096 and the end of an
      8192-position cache;
  (b) `kv_cache_bytes()` of a pool sized for the eight prompts of --ragged leg (b) plus their new tokens against the contiguous bs = 8
      stack's, and the seconds of `generate(list)` on either.

    python tools/llama_decode_bench.py --config llama3_8b --paged --kv-cache mx8 [--out profiles/paged_mx8_bench.jsonl]

--paged --kv-cache mx8 (one GPU): the same two legs with mx8 stacks -- leg (a) alternates the contiguous mx8 stack
with mx8_attention="online" (the dg_rope_attn_online_mx8_seq flavour of dg_attn_launch) against the paged mx8 stack (dg_rope_attn_online_mx8_paged), the same kernel
with and without the page lookup; leg (b) reports the bytes of the four mx8 pools for the eight prompts.

    python tools/llama_decode_bench.py --config llama3_8b --sample [--out profiles/sample_bench.jsonl]

--sample (one GPU): what sampling costs, one JSON line per batch size (1 and 8), appended to --out: the captured step
alone, with the fused sampler (dg_sample) as its last node, followed by the same sampler as an eager launch, and followed by the torch
formulation (sort, softmax, cumsum, masked softmax, multinomial) -- alternating in one process, the order rotating -- and the sampler
launched back to back on its own.  temperature 0.8, top_k 50, top_p 0.95.

    python tools/llama_decode_bench.py --config llama3_8b --interleave --lora 16 [--adapters 8] [--out profiles/lora_bench.jsonl]

--lora RANK (one GPU): per-sequence LoRA adapters on the four fused linears, one JSON line per batch size (1 and 8),
appended to --out: the captured step near position 512 (a) without adapters, (b) with an AdapterSet attached and every id -1 -- the price
of the eight added launches per layer --, (c) every sequence on adapter 0, (d) a different adapter per sequence (bs = 8), (e) the torch
formulation of the deltas (index_select + bmm) behind the same fused step.  The legs alternate in one process, three runs each, the order
rotating; (b), (c) and (d) replay one captured graph and differ only in `adapter_ids`.

    python tools/llama_decode_bench.py --moe [--layers N] [--out profiles/moe_bench.jsonl]

    python tools/llama_decode_bench.py --moe --moe-prefill [--layers N] [--out profiles/moe_grouped_bench.jsonl]

--moe --moe-prefill (one GPU): `prefill` of 64 / 128 / 512 tokens at bs 1 and of 128 at bs 8 at the Mixtral-8x7B shape (8 layers by default),
the grouped path against the row blocks of 8 rows on the same stack, alternating, three runs each, median (min - max).

--moe (one GPU): mixture of experts at the Mixtral-8x7B shape (8 experts, 2 per token), two JSON lines per batch size
(1 and 8), appended to --out: the captured step on dg_moe_route / dg_moe_launch (DG_MOE_GEMV) against the formulation that is possible without them
(every expert through the module GEMVs, a device-side mask: it captures too), alternating, three runs each; and DG_MOE_GEMV GATE_UP /
DOWN against the module GEMV on ONE expert's linears at the same m, one pair per layer and graph, with the effective bandwidth over the
bytes of the experts the seeded router selected (computed from shapes, `moe_bytes`).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def time_steps(stack, steps, warmup, start_pos, after=None):
    """Seconds per decode step; after(logits): what follows every step (--sample: a sampler behind the replay)."""
    tok = torch.randint(0, stack.cfg.vocab, (stack.bs,), device=stack.tokens.device)
    for i in range(warmup):
        out = stack.decode(tok, start_pos + i)
        if after is not None:
            after(out)
    if dist.is_initialized():
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = stack.decode(tok, start_pos + warmup + i)
        if after is not None:
            after(out)
    if dist.is_initialized():
        dist.barrier()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def torch_sample(logits, temperature, top_k, top_p):
    """Temperature / top-k / top-p the way it is written in torch: a full sort of the row, softmax, cumsum, a masked softmax, multinomial."""
    vals, idx = torch.sort(logits.float() / temperature, dim=-1, descending=True)
    vals[:, top_k:] = float("-inf")
    probs = torch.softmax(vals, dim=-1)
    before = torch.cumsum(probs, dim=-1) - probs
    probs = torch.softmax(vals.masked_fill(before >= top_p, float("-inf")), dim=-1)
    return idx.gather(1, torch.multinomial(probs, 1)).squeeze(1)


def sample_bench(a, cfg, device):
    """--sample: the captured step without the sampler, with the sampler as its last node, and followed by the torch formulation;
    and the sampler launch on its own."""
    from any4_amd.decode import Any4Factory, DecodeStack

    T, K, P = 0.8, 50, 0.95
    base = {"config": a.config, "layers": cfg.layers, "max_seq": cfg.max_seq, "vocab": cfg.vocab, "data": "synthetic (random weights, random tokens)",
            "temperature": T, "top_k": K, "top_p": P, "steps": a.steps, "warmup": a.warmup, "start_pos": a.start_pos, "rounds": a.rounds}
    legs = []
    for bs in (1, 8):
        def stack(sample):
            st = DecodeStack(cfg, Any4Factory(cfg, device, torch.bfloat16, seed=1, kernel=a.kernel), device, torch.bfloat16, bs=bs,
                             fuse_gemm_stages=not a.no_fuse)
            st.set_sampling(T, K, P, seed=list(range(bs)))
            st.capture(sample=sample)
            return st

        plain, fused = stack(False), stack(True)
        runs = {"step": (plain, None), "step_with_sampler_node": (fused, None),
                "step_then_torch_sampler": (plain, lambda logits: torch_sample(logits, T, K, P)),
                "step_then_eager_sampler": (plain, lambda logits: plain.sample(logits, plain.pos, 1))}
        series = {k: [] for k in runs}
        order = list(runs)
        for r in range(a.rounds):
            for k in order[r % len(order):] + order[: r % len(order)]:
                st, after = runs[k]
                series[k].append(round(time_steps(st, a.steps, a.warmup, a.start_pos, after) * 1e3, 4))
        ms = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "series": v} for k, v in series.items()}
        # the sampler alone, back to back on the logits of the last step: kernel time (an empty launch is ~8 us of the ~70)
        logits = plain._out
        for _ in range(20):
            plain.sample(logits, plain.pos, 1)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(200):
            plain.sample(logits, plain.pos, 1)
        ev[1].record()
        torch.cuda.synchronize()
        legs.append(dict(base, leg="captured step: plain / sampler as last node / followed by the torch formulation / by the eager sampler",
                         bs=bs, graph_nodes={"step": getattr(plain, "graph_nodes", None), "step_with_sampler_node": getattr(fused, "graph_nodes", None)},
                         ms_per_step=ms, sampler_node_us=round((ms["step_with_sampler_node"]["median"] - ms["step"]["median"]) * 1e3, 2),
                         torch_sampler_us=round((ms["step_then_torch_sampler"]["median"] - ms["step"]["median"]) * 1e3, 2),
                         sampler_back_to_back_us=round(ev[0].elapsed_time(ev[1]) / 200 * 1e3, 2)))
        del plain, fused, runs
        torch.cuda.empty_cache()
    return legs


def lora_bench(a, cfg, device):
    """--lora RANK: the captured step without adapters (a), with adapters attached and every id -1 (b), every sequence on adapter 0 (c), a
    different adapter per sequence (d, bs = 8), and the torch formulation of the deltas (lora_ref: index_select + bmm) behind the same
    fused step with every sequence on adapter 0 (e).  (b), (c) and (d) are ONE captured graph: only `adapter_ids` changes."""
    from any4_amd.decode import Any4Factory, DecodeStack
    from any4_amd.lora import AdapterSet

    base = {"config": a.config, "layers": cfg.layers, "max_seq": cfg.max_seq, "data": "synthetic (random weights, random tokens, random adapters)",
            "rank": a.lora, "n_adapters": a.adapters, "steps": a.steps, "warmup": a.warmup, "start_pos": a.start_pos, "rounds": a.rounds,
            "interleave": cfg.gate_up_interleave}
    legs = []
    for bs in (1, 8):
        def stack(adapters, kernels=True):
            aset = None
            if adapters:
                aset = AdapterSet(cfg, a.adapters, a.lora, device, torch.bfloat16)
                gen = torch.Generator(device=device).manual_seed(5)
                for slot in range(a.adapters):  # random adapters of full rank on all four linears of every layer, scale 2
                    aset.load(slot, {(layer, name): ((torch.randn(a.lora, k, device=device, generator=gen) / k ** 0.5).bfloat16(),
                                                     (torch.randn(n, a.lora, device=device, generator=gen) * 0.05).bfloat16())
                                     for layer in range(cfg.layers) for name, n, k in cfg.linear_shapes()}, alpha=2.0 * a.lora)
            st = DecodeStack(cfg, Any4Factory(cfg, device, torch.bfloat16, seed=1, kernel=a.kernel), device, torch.bfloat16, bs=bs,
                             fuse_gemm_stages=not a.no_fuse, adapters=aset)
            if adapters:
                st.lora_kernels = kernels
                st.decode(torch.zeros(bs, dtype=torch.long, device=device), 0, adapters=[0] * bs)  # (captured with live adapters)
            st.capture()
            return st

        plain, kern, ref = stack(False), stack(True), stack(True, kernels=False)
        runs = {"a_no_adapters": (plain, None), "b_attached_all_off": (kern, [-1] * bs), "c_all_on_adapter_0": (kern, [0] * bs),
                "e_torch_all_on_adapter_0": (ref, [0] * bs)}
        if bs > 1:
            runs["d_adapter_per_sequence"] = (kern, [i % a.adapters for i in range(bs)])
        series = {k: [] for k in runs}
        order = list(runs)
        for r in range(a.rounds):
            for k in order[r % len(order):] + order[: r % len(order)]:
                st, ids = runs[k]
                if ids is not None:
                    st.set_adapters(ids)
                series[k].append(round(time_steps(st, a.steps, a.warmup, a.start_pos) * 1e3, 4))
        ms = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "series": v} for k, v in series.items()}
        med = lambda k: ms[k]["median"]
        legs.append(dict(base, leg="captured step: no adapters / attached, all off / all on adapter 0 / one per sequence / torch formulation",
                         bs=bs, kernels_per_layer={"a": getattr(plain, "kernels_per_layer", None), "b_c_d": getattr(kern, "kernels_per_layer", None)},
                         ms_per_step=ms,
                         added_launches_us_per_layer=round((med("b_attached_all_off") - med("a_no_adapters")) * 1e3 / cfg.layers, 2),
                         adapter_work_us_per_layer=round((med("c_all_on_adapter_0") - med("b_attached_all_off")) * 1e3 / cfg.layers, 2),
                         kernels_vs_torch=round(med("c_all_on_adapter_0") / med("e_torch_all_on_adapter_0"), 4)))
        del plain, kern, ref, runs
        torch.cuda.empty_cache()
    return legs


def moe_bytes(stack, n_experts):
    """Bytes `n_experts` experts of one stacked linear hold: packed words, scale | zero words, LUT rows -- from shapes alone."""
    lut = 0 if stack.lut is None else stack.n * 32 if stack.lut.dim() == 3 else 32
    return n_experts * (stack.n * stack.k // 2 + (stack.k // stack.group) * stack.n * 4 + lut)


def moe_bench(a, cfg, device):
    """--moe: (1) the captured step of a stack with experts on dg_moe_route / dg_moe_launch (DG_MOE_GEMV) against the formulation that is possible
    WITHOUT them -- every expert through the module GEMVs (w4_linear_fused: SwiGLU in gate_up's store), combined with a device-side mask,
    the router in torch; nothing read on the host, so it captures too -- at bs 1 and 8, alternating in one process, three runs each.
    (2) DG_MOE_GEMV GATE_UP + DOWN back to back against the module GEMVs on ONE expert's two linears at the same m, as graphs of one
    pair per layer (every pair reads another layer's weights: nothing is served from a cache), alternating, three runs; the effective
    bandwidth is over the bytes of the experts the seeded router selected (moe_bytes: from shapes)."""
    from any4_amd import decode_ops as G, ops
    from any4_amd.decode import Any4Factory, DecodeStack
    from any4_amd.moe import route_ref

    class AllExperts(torch.nn.Module):
        """The block without the feature: E x (gate_up + SwiGLU, down) on the existing kernels and a mask."""

        def __init__(self, moe):
            super().__init__()
            self.m, self.weights, self.router, self.top_k = moe, moe.weights, moe.router, moe.top_k   # (what DecodeLayer reads of its block)

        def forward(self, x, residual=None, fused=True, out=None):
            W, top_k = self.m.weights, self.m.top_k
            ids, gates = route_ref(x.float() @ self.m.router.float().t(), top_k)
            acc = torch.zeros(x.shape[0], W.down.n, dtype=torch.float32, device=x.device)
            for e in range(W.E):
                act = ops.w4_linear_fused(x, W.gate_up.words[e], W.gate_up.group, W.gate_up.qinfo[e], W.gate_up.lut[e], swiglu=True)
                d = ops.w4_linear_fused(act, W.down.words[e], W.down.group, W.down.qinfo[e], W.down.lut[e])
                acc += (gates * (ids == e)).sum(dim=1, keepdim=True) * d.float()
            y = (acc if residual is None else acc + residual.float()).to(x.dtype)
            return y if out is None else out.copy_(y)

    base = {"config": a.config, "layers": cfg.layers, "experts": cfg.experts, "experts_per_token": cfg.experts_per_token, "hidden": cfg.hidden,
            "inter": cfg.inter, "max_seq": cfg.max_seq, "data": "synthetic (random weights, random tokens)", "steps": a.steps,
            "warmup": a.warmup, "start_pos": a.start_pos, "rounds": a.rounds}
    stat = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "series": v}
    legs = []
    for bs in (1, 8):
        def stack(all_experts):
            st = DecodeStack(cfg, Any4Factory(cfg, device, torch.bfloat16, seed=1, kernel=a.kernel), device, torch.bfloat16, bs=bs,
                             fuse_gemm_stages=not a.no_fuse)
            if all_experts:
                for layer in st.layers:
                    layer.moe = AllExperts(layer.moe)
            st.capture()
            return st

        new, old = stack(False), stack(True)
        runs = {"moe_kernels": new, "all_experts_masked": old}
        series = {k: [] for k in runs}
        order = list(runs)
        for r in range(a.rounds):
            for k in order[r % 2:] + order[: r % 2]:
                series[k].append(round(time_steps(runs[k], a.steps, a.warmup, a.start_pos) * 1e3, 4))
        ms = {k: stat(v) for k, v in series.items()}
        legs.append(dict(base, leg="captured step: dg_moe kernels / all experts through the module GEMVs and a mask", bs=bs,
                         kernels_per_layer=getattr(new, "kernels_per_layer", None), ms_per_step=ms,
                         ratio_new_over_old=round(ms["moe_kernels"]["median"] / ms["all_experts_masked"]["median"], 4)))
        del old, runs

        # (2) the two GEMV stages alone, one (gate_up, down) pair per layer and graph
        layers = [layer.moe for layer in new.layers]
        gen = torch.Generator(device=device).manual_seed(7)
        x = torch.randn(bs, cfg.hidden, device=device, generator=gen).bfloat16()
        picks = [G.moe_route(x, m.router, m.top_k) for m in layers]
        distinct = [int(torch.unique(ids).numel()) for ids, _ in picks]
        act1 = torch.randn(bs, cfg.inter, device=device, generator=gen).bfloat16()

        def moe_pairs():
            for m, (ids, gates) in zip(layers, picks):
                G.moe_down(G.moe_gate_up(x, m.weights.gate_up, ids), m.weights.down, ids, gates)

        def gemv_pairs():
            for m in layers:
                gu, dn = m.weights.gate_up, m.weights.down
                ops.w4_linear_fused(ops.w4_linear_fused(x, gu.words[0], gu.group, gu.qinfo[0], gu.lut[0], swiglu=True), dn.words[0], dn.group,
                                    dn.qinfo[0], dn.lut[0])

        def stage_only(fn):
            return lambda: [fn(m, p) for m, p in zip(layers, picks)]

        fns = {"moe_gate_up+down": moe_pairs, "gemv_gate_up+down_one_expert": gemv_pairs,
               "moe_gate_up": stage_only(lambda m, p: G.moe_gate_up(x, m.weights.gate_up, p[0])),
               "moe_down": stage_only(lambda m, p: G.moe_down(act1.repeat_interleave(m.top_k, dim=0), m.weights.down, p[0], p[1])),
               "gemv_gate_up": stage_only(lambda m, p: ops.w4_linear_fused(x, m.weights.gate_up.words[0], m.weights.gate_up.group,
                                                                            m.weights.gate_up.qinfo[0], m.weights.gate_up.lut[0], swiglu=True)),
               "gemv_down": stage_only(lambda m, p: ops.w4_linear_fused(act1, m.weights.down.words[0], m.weights.down.group,
                                                                         m.weights.down.qinfo[0], m.weights.down.lut[0]))}
        graphs = {}
        for k, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            graphs[k] = g

        def timed(g, reps=20):
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                g.replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps / len(layers) * 1e6   # us per layer

        series = {k: [] for k in graphs}
        order = list(graphs)
        for r in range(a.rounds):
            for k in order[r % len(order):] + order[: r % len(order)]:
                series[k].append(round(timed(graphs[k]), 3))
        us = {k: stat(v) for k, v in series.items()}
        gu0, dn0 = layers[0].weights.gate_up, layers[0].weights.down
        mean_distinct = sum(distinct) / len(distinct)
        sel = {"gate_up": moe_bytes(gu0, mean_distinct), "down": moe_bytes(dn0, mean_distinct)}
        one = {"gate_up": moe_bytes(gu0, 1), "down": moe_bytes(dn0, 1)}
        tbs = lambda nbytes, k: round(nbytes / (us[k]["median"] * 1e-6) / 1e12, 3)
        legs.append(dict(base, leg="kernels: DG_MOE_GEMV GATE_UP / DOWN against the module GEMV on one expert, one pair per layer and graph", bs=bs,
                         distinct_experts_per_layer=distinct, us_per_layer=us,
                         selected_bytes_per_layer={k: int(v) for k, v in sel.items()}, one_expert_bytes=one,
                         effective_TBps={"moe_gate_up": tbs(sel["gate_up"], "moe_gate_up"), "moe_down": tbs(sel["down"], "moe_down"),
                                         "moe_pair": tbs(sel["gate_up"] + sel["down"], "moe_gate_up+down"),
                                         "gemv_gate_up": tbs(one["gate_up"], "gemv_gate_up"), "gemv_down": tbs(one["down"], "gemv_down"),
                                         "gemv_pair": tbs(one["gate_up"] + one["down"], "gemv_gate_up+down_one_expert")}))
        del new, graphs, layers, picks
        torch.cuda.empty_cache()
    return legs


def moe_prefill_bench(a, cfg, device):
    """--moe --moe-prefill: `prefill` of T tokens on a stack with experts, the grouped path (MoEMLP.grouped_from = 1: route, dg_moe_group,
    dg_moe_launch with DG_MOE_GROUPED twice) against the row-block path (grouped_from = None: DG_MOE_GEMV in blocks of 8 rows) on the SAME stack
    and weights, alternating in one process, three runs each.  The row-block path's kernels are the ones this library had before the grouped
    path existed, so in the same build it stands for the earlier library.  One JSON line per (T, bs) leg."""
    from any4_amd.decode import Any4Factory, DecodeStack

    base = {"config": a.config, "layers": cfg.layers, "experts": cfg.experts, "experts_per_token": cfg.experts_per_token, "hidden": cfg.hidden,
            "inter": cfg.inter, "group_size": cfg.group_size, "kernel": a.kernel, "dtype": "bf16",
            "data": "synthetic (random weights, random tokens)", "rounds": a.rounds}
    stat = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "series": v}
    legs = []
    stacks = {}
    for T, bs in ((64, 1), (128, 1), (512, 1), (128, 8)):
        if bs not in stacks:
            stacks.clear()
            stacks[bs] = DecodeStack(cfg, Any4Factory(cfg, device, torch.bfloat16, seed=1, kernel=a.kernel), device, torch.bfloat16, bs=bs)
        st = stacks[bs]
        toks = torch.randint(0, cfg.vocab, (bs, T), generator=torch.Generator().manual_seed(T)).to(device)

        def run(grouped, reps):
            for layer in st.layers:
                layer.moe.grouped_from = 1 if grouped else None
            st.prefill(toks, position=0)   # warm-up (and the grouped buffers of this row count)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                st.prefill(toks, position=0)
            t1.record()
            torch.cuda.synchronize()
            return round(t0.elapsed_time(t1) / reps, 4)

        series = {"grouped": [], "row_blocks": []}
        order = list(series)
        for r in range(a.rounds):
            for k in order[r % 2:] + order[: r % 2]:
                series[k].append(run(k == "grouped", 5 if k == "grouped" else 2))
        ms = {k: stat(v) for k, v in series.items()}
        spread = max(ms[k]["max"] - ms[k]["min"] for k in ms)
        legs.append(dict(base, leg="prefill: grouped tile GEMM / row blocks of 8 (DG_MOE_GEMV)", T=T, bs=bs, rows=T * bs, ms_per_prefill=ms,
                         speedup_grouped=round(ms["row_blocks"]["median"] / ms["grouped"]["median"], 3),
                         grouped_faster_by_more_than_the_larger_spread=bool(ms["row_blocks"]["median"] - ms["grouped"]["median"] > spread)))
    return legs


def ragged_bench(a, cfg, device):
    """The two legs of --ragged; returns the JSON-able results."""
    from any4_amd.decode import Any4Factory, DecodeStack

    def stack(bs, ragged):
        st = DecodeStack(cfg, Any4Factory(cfg, device, torch.bfloat16, seed=1, kernel=a.kernel), device, torch.bfloat16, bs=bs,
                         fuse_gemm_stages=not a.no_fuse, ragged=ragged)
        st.capture()
        return st

    base = {"config": a.config, "layers": cfg.layers, "max_seq": cfg.max_seq, "data": "synthetic (random weights, random tokens)"}
    legs = []
    # (a) the same step, positions [p] * bs through pos_seq vs p through pos; rounds alternate so that drift hits both alike
    leg = dict(base, leg="a: captured step at equal positions, ragged vs non-ragged, alternating", steps=a.steps, warmup=a.warmup,
               start_pos=a.start_pos, rounds=a.rounds, ms_per_step={})
    for bs in (1, 4, 8):
        pair = {"plain": stack(bs, False), "ragged": stack(bs, True)}
        series = {k: [] for k in pair}
        for r in range(a.rounds):
            for k in (("plain", "ragged") if r % 2 == 0 else ("ragged", "plain")):
                series[k].append(round(time_steps(pair[k], a.steps, a.warmup, a.start_pos) * 1e3, 4))
        leg["ms_per_step"][f"bs{bs}"] = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "series": v}
                                         for k, v in series.items()}
        del pair
        torch.cuda.empty_cache()
    legs.append(leg)
    # (b) a ragged batch of eight against eight runs at batch 1
    lengths, new = [16, 32, 64, 96, 128, 256, 384, 512], a.new_tokens
    gen = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab, (n,), generator=gen).to(device) for n in lengths]

    def timed(fn):
        fn()  # (first call: allocator, workspaces)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    one, eight = stack(1, False), stack(8, True)
    t_seq = timed(lambda: [one.generate(p.view(1, -1), new) for p in prompts])
    t_rag = timed(lambda: eight.generate(prompts, new))
    legs.append(dict(base, leg="b: eight prompts, generate(list) on a ragged bs = 8 stack vs eight bs = 1 runs in a row",
                     prompt_lengths=lengths, new_tokens=new,
                     sequential_bs1={"seconds": round(t_seq, 4), "tokens_per_s": round(8 * new / t_seq, 1)},
                     ragged_bs8={"seconds": round(t_rag, 4), "tokens_per_s": round(8 * new / t_rag, 1)},
                     speedup=round(t_seq / t_rag, 3)))
    return legs


def kv8_bench(a, cfg, device):
    """The legs of --kv-cache mx8; yields the JSON-able results."""
    from any4_amd.decode import Any4Factory, DecodeStack

    def stack(bs, kv_cache, ragged=False):
        st = DecodeStack(cfg, Any4Factory(cfg, device, torch.bfloat16, seed=1, kernel=a.kernel), device, torch.bfloat16, bs=bs,
                         fuse_gemm_stages=not a.no_fuse, ragged=ragged, kv_cache=kv_cache)
        st.capture()
        return st

    base = {"config": a.config, "layers": cfg.layers, "max_seq": cfg.max_seq, "data": "synthetic (random weights, random tokens, zero caches)"}
    if a.ragged:  # leg (b) of --ragged on either cache
        lengths, new = [16, 32, 64, 96, 128, 256, 384, 512], a.new_tokens
        gen = torch.Generator().manual_seed(0)
        prompts = [torch.randint(0, cfg.vocab, (n,), generator=gen).to(device) for n in lengths]
        res = {}
        for name, kv in (("cache16", None), ("mx8", "mx8")):
            st = stack(8, kv, ragged=True)
            st.generate(prompts, new)  # (first call: allocator, workspaces)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.generate(prompts, new)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            res[name] = {"seconds": round(t, 4), "tokens_per_s": round(8 * new / t, 1), "kv_cache_bytes": st.kv_cache_bytes(), "attn_split": st._attn_split}
            del st
            torch.cuda.empty_cache()
        yield dict(base, leg="kv8 b: eight prompts, generate(list) on a ragged bs = 8 stack, 16-bit cache vs mx8 cache", prompt_lengths=lengths,
                   new_tokens=new, **res, mx8_over_cache16=round(res["mx8"]["seconds"] / res["cache16"]["seconds"], 4))
        return
    for bs in (1, 8):
        pair = {"cache16": stack(bs, None), "mx8": stack(bs, "mx8")}
        leg = dict(base, leg="kv8 a: captured step, 16-bit cache vs mx8 cache, alternating", bs=bs, steps=a.steps, warmup=a.warmup, rounds=a.rounds,
                   kv_cache_bytes={k: st.kv_cache_bytes() for k, st in pair.items()}, attn_split={k: st._attn_split for k, st in pair.items()},
                   ms_per_step={})
        for want in (512, 4096, cfg.max_seq):
            start = max(0, min(want, cfg.max_seq - a.warmup - a.steps))  # (the timed steps end inside the cache)
            series = {k: [] for k in pair}
            for r in range(a.rounds):
                for k in (("cache16", "mx8") if r % 2 == 0 else ("mx8", "cache16")):
                    series[k].append(round(time_steps(pair[k], a.steps, a.warmup, start) * 1e3, 4))
            med = {k: sorted(v)[len(v) // 2] for k, v in series.items()}
            leg["ms_per_step"][f"pos{start + a.warmup}"] = dict(
                {k: {"median": med[k], "min": min(v), "max": max(v), "series": v} for k, v in series.items()},
                mx8_over_cache16=round(med["mx8"] / med["cache16"], 4))
        yield leg
        del pair
        torch.cuda.empty_cache()


def kv8_online_bench(a, cfg, device):
    """The cells of --kv-cache mx8 --mx8-attention online; yields the JSON-able results, one per (bs, position)."""
    from any4_amd.decode import Any4Factory, DecodeStack

    def stack(bs, **kw):
        st = DecodeStack(cfg, Any4Factory(cfg, device, torch.bfloat16, seed=1, kernel=a.kernel), device, torch.bfloat16, bs=bs,
                         fuse_gemm_stages=not a.no_fuse, **kw)
        st.capture()
        return st

    base = {"config": a.config, "layers": cfg.layers, "max_seq": cfg.max_seq, "data": "synthetic (random weights, random tokens, zero caches)"}
    names = ("cache16", "mx8_split", "mx8_online")
    for bs in (1, 8):
        trio = {"cache16": stack(bs), "mx8_split": stack(bs, kv_cache="mx8", mx8_attention="split"),
                "mx8_online": stack(bs, kv_cache="mx8", mx8_attention="online")}
        for want in (512, 4096, cfg.max_seq):
            start = max(0, min(want, cfg.max_seq - a.warmup - a.steps))  # (the timed steps end inside the cache)
            series = {k: [] for k in names}
            for r in range(a.rounds):
                for k in names[r % 3:] + names[:r % 3]:
                    series[k].append(round(time_steps(trio[k], a.steps, a.warmup, start) * 1e3, 4))
            med = {k: sorted(v)[len(v) // 2] for k, v in series.items()}
            yield dict(base, leg="kv8 online: captured step, 16-bit cache vs mx8 split vs mx8 online, alternating", bs=bs, pos=start + a.warmup,
                       steps=a.steps, warmup=a.warmup, rounds=a.rounds, attn_split={k: st._attn_split for k, st in trio.items()},
                       ms_per_step={k: {"median": med[k], "min": min(v), "max": max(v), "series": v} for k, v in series.items()},
                       online_over_split=round(med["mx8_online"] / med["mx8_split"], 4),
                       online_over_cache16=round(med["mx8_online"] / med["cache16"], 4),
                       split_over_cache16=round(med["mx8_split"] / med["cache16"], 4))
        del trio
        torch.cuda.empty_cache()


def paged_bench(a, cfg, device):
    """The legs of --paged (with --kv-cache mx8: on mx8 stacks, the contiguous one on the one-barrier kernel); yields the JSON-able results."""
    from any4_amd.decode import Any4Factory, DecodeStack

    ps = 64
    mx8 = a.kv_cache == "mx8"

    def stack(bs, kv_pages, capture=True):
        st = DecodeStack(cfg, Any4Factory(cfg, device, torch.bfloat16, seed=1, kernel=a.kernel), device, torch.bfloat16, bs=bs,
                         fuse_gemm_stages=not a.no_fuse, ragged=True, kv_pages=kv_pages, page_size=ps,
                         **(dict(kv_cache="mx8", mx8_attention="online") if mx8 else {}))
        if kv_pages is not None and capture:  # every position exists before the timed steps; physical order is not logical order
            st.page_pool._free.reverse()
            for b in range(bs):
                st.reserve(b, cfg.max_seq)
        if capture:
            st.capture()
        return st

    base = {"config": a.config, "layers": cfg.layers, "max_seq": cfg.max_seq, "page_size": ps, **({"kv_cache": "mx8"} if mx8 else {}),
            "data": "synthetic (random weights, random tokens, zero caches)"}
    for bs in (1, 8):
        pair = {"contiguous": stack(bs, None), "paged": stack(bs, bs * cfg.max_seq // ps)}
        leg = dict(base, leg="paged a: captured ragged step, contiguous cache vs page pool, alternating", bs=bs, steps=a.steps, warmup=a.warmup,
                   rounds=a.rounds, kv_cache_bytes={k: st.kv_cache_bytes() for k, st in pair.items()},
                   attn_split={k: st._attn_split for k, st in pair.items()}, ms_per_step={})
        for want in (512, 4096, cfg.max_seq):
            start = max(0, min(want, cfg.max_seq - a.warmup - a.steps))  # (the timed steps end inside the cache)
            series = {k: [] for k in pair}
            for r in range(a.rounds):
                for k in (("contiguous", "paged") if r % 2 == 0 else ("paged", "contiguous")):
                    series[k].append(round(time_steps(pair[k], a.steps, a.warmup, start) * 1e3, 4))
            med = {k: sorted(v)[len(v) // 2] for k, v in series.items()}
            leg["ms_per_step"][f"pos{start + a.warmup}"] = dict(
                {k: {"median": med[k], "min": min(v), "max": max(v), "series": v} for k, v in series.items()},
                paged_over_contiguous=round(med["paged"] / med["contiguous"], 4))
        yield leg
        del pair
        torch.cuda.empty_cache()
    # (b) the pool the eight prompts need against eight slots of max_seq rows
    lengths, new = [16, 32, 64, 96, 128, 256, 384, 512], a.new_tokens
    gen = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab, (n,), generator=gen).to(device) for n in lengths]
    pages = sum(-(-(n + new) // ps) for n in lengths)
    res = {}
    for name, kv_pages in (("contiguous", None), ("paged", pages)):
        st = stack(8, kv_pages, capture=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.generate(prompts, new)
        torch.cuda.synchronize()
        res[name] = {"kv_cache_bytes": st.kv_cache_bytes(), "generate_seconds_eager_first_call": round(time.perf_counter() - t0, 4)}
        if kv_pages is not None:
            res[name].update(kv_pages=pages, free_pages_after=st.page_pool.free_pages)
        del st
        torch.cuda.empty_cache()
    yield dict(base, leg="paged b: KV bytes of a pool sized for eight prompts + new tokens vs the contiguous bs = 8 stack", prompt_lengths=lengths,
               new_tokens=new, **res, paged_over_contiguous_bytes=round(res["paged"]["kv_cache_bytes"] / res["contiguous"]["kv_cache_bytes"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="llama3_8b", choices=["llama3_8b", "llama2_7b", "mixtral_8x7b", "tiny"])
    ap.add_argument("--layers", type=int, default=None, help="override the number of decoder layers")
    ap.add_argument("--bs", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 100; with --mx8-attention online 30)")
    ap.add_argument("--warmup", type=int, default=None, help="warm-up steps (default 20; with --mx8-attention online 10)")
    ap.add_argument("--max-seq", type=int, default=1024)
    ap.add_argument("--start-pos", type=int, default=None, help="sequence position of the first timed token (default 128; with --lora 512)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--interleave", action="store_true", help="gate_up rows in blocks of 8 gate + 8 up (lets the GEMM fuse SwiGLU)")
    ap.add_argument("--no-fuse", action="store_true", help="separate glue kernels around the GEMMs (8 launches per layer instead of 5)")
    ap.add_argument("--baseline", action="store_true", help="also time the same stack with 16-bit nn.Linear")
    ap.add_argument("--kernel", default="linear_y_f16RM_x_f16RM_W_any4TC")
    ap.add_argument("--emulate-tp", type=int, default=0,
                    help="single process, timing only: build rank 0 of a TP=N model and replace the all-gathers by local "
                         "copies -> per-GPU compute time of a TP=N step without the interconnect")
    ap.add_argument("--gather", default="rccl", choices=["rccl", "peer"],
                    help="TP > 1: RCCL all_gather_into_tensor per exchange, or the one-shot peer-write gather (include/peer_gather_hip.h)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend; gloo needs --gather peer (no CUDA collectives: only the IPC handles travel through it)")
    ap.add_argument("--same-device", action="store_true",
                    help="functional check on a one-GPU box: every rank uses GPU 0 (needs --backend gloo --gather peer); the time "
                         "it prints is two processes sharing one GPU, not a TP measurement")
    ap.add_argument("--ragged", action="store_true", help="the two legs of DESIGN.md section 13 (see the module docstring); one GPU")
    ap.add_argument("--rounds", type=int, default=None, help="--ragged leg (a): alternations per batch size (default 7; with --mx8-attention online 5)")
    ap.add_argument("--new-tokens", type=int, default=64, help="--ragged leg (b): tokens generated per prompt")
    ap.add_argument("--kv-cache", default=None, choices=["mx8"],
                    help="the legs of DESIGN.md section 15: the mx8 KV cache against the 16-bit one at an 8192-position cache (see the module docstring); one GPU")
    ap.add_argument("--mx8-attention", default=None, choices=["online"],
                    help="with --kv-cache mx8: the three-way comparison of DESIGN.md section 15 (16-bit, mx8 split, mx8 online; see the module docstring); one GPU")
    ap.add_argument("--paged", action="store_true",
                    help="the legs of DESIGN.md section 16: the paged KV cache against the contiguous one at an 8192-position cache (see the module docstring); one GPU")
    ap.add_argument("--sample", action="store_true",
                    help="the leg of DESIGN.md section 18: the captured step with and without the sampler node, and followed by the torch formulation (see the module docstring); one GPU")
    ap.add_argument("--lora", type=int, default=0, metavar="RANK",
                    help="per-sequence LoRA adapters of this rank on the four fused linears (DESIGN.md section 20; see the module docstring); one GPU")
    ap.add_argument("--adapters", type=int, default=8, help="--lora: adapters resident in the set")
    ap.add_argument("--moe", action="store_true",
                    help="mixture of experts (DESIGN.md section 22): the Mixtral-8x7B shape (--layers N for fewer layers; --config tiny: a small "
                         "one) on the dg_moe kernels against all experts through the module GEMVs and a mask, and the two GEMV stages alone")
    ap.add_argument("--moe-prefill", action="store_true",
                    help="with --moe: prefill of 64 / 128 / 512 tokens at bs 1 and 128 at bs 8 (8 layers unless --layers), the grouped tile GEMM "
                         "(MoEMLP.grouped_from) against the row blocks of 8, one line per leg appended to profiles/moe_grouped_bench.jsonl")
    ap.add_argument("--out", default=None, help="--ragged / --kv-cache / --paged: the file the JSON lines are appended to (default "
                                                "profiles/ragged_bench.jsonl, with --kv-cache profiles/kv8_bench.jsonl, with --paged profiles/paged_bench.jsonl, with both profiles/paged_mx8_bench.jsonl)")
    a = ap.parse_args()
    if a.mx8_attention and not a.kv_cache:
        raise SystemExit("--mx8-attention goes with --kv-cache mx8")
    three_way = a.mx8_attention == "online"
    a.steps = a.steps if a.steps is not None else 30 if three_way else 100
    a.warmup = a.warmup if a.warmup is not None else 10 if three_way else 20
    a.rounds = a.rounds if a.rounds is not None else 3 if a.lora or a.moe else 5 if three_way else 7  # (--lora: three runs per leg)
    a.start_pos = a.start_pos if a.start_pos is not None else 512 if a.lora else 128
    if a.moe:
        a.out = a.out or os.path.join(ROOT, "profiles", "moe_grouped_bench.jsonl" if a.moe_prefill else "moe_bench.jsonl")
        if a.moe_prefill and a.layers is None:
            a.layers = 8
        a.config = "mixtral_8x7b" if a.config == "llama3_8b" else a.config
    if a.lora:
        a.out = a.out or os.path.join(ROOT, "profiles", "lora_bench.jsonl")
    if a.out is None and a.sample:
        a.out = os.path.join(ROOT, "profiles", "sample_bench.jsonl")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "paged_mx8_bench.jsonl" if a.paged and a.kv_cache else "paged_bench.jsonl" if a.paged else "kv8_online_bench.jsonl" if three_way else
                             "kv8_bench.jsonl" if a.kv_cache else "ragged_bench.jsonl")
    if a.backend == "gloo" and a.gather != "peer":
        raise SystemExit("--backend gloo moves no CUDA tensors: use it with --gather peer")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU (the HIP path has no CPU fallback)")
    if a.same_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group(backend=a.backend)

    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack, DenseFactory, memory_allocated_mb

    if a.config == "tiny":
        cfg = DecodeConfig(hidden=512, inter=1024, layers=2, heads=8, kv_heads=8, head_dim=64, vocab=1024, max_seq=a.max_seq)
        if a.moe:
            cfg.experts, cfg.experts_per_token, cfg.gate_up_interleave = 4, 2, 8
    else:
        cfg = getattr(DecodeConfig, a.config)(max_seq=a.max_seq)
    if a.layers is not None:
        cfg.layers = a.layers
    if a.interleave:
        cfg.gate_up_interleave = 8

    if a.moe:
        if world > 1 or not cfg.experts:
            raise SystemExit("--moe runs on one GPU, with a configuration that has experts (mixtral_8x7b, tiny)")
        with open(a.out, "a") as f:
            for leg in (moe_prefill_bench if a.moe_prefill else moe_bench)(a, cfg, device):
                line = json.dumps(leg)
                print(line, flush=True)
                f.write(line + "\n")
        return

    if a.lora:
        if world > 1:
            raise SystemExit("--lora runs on one GPU")
        with open(a.out, "a") as f:
            for leg in lora_bench(a, cfg, device):
                line = json.dumps(leg)
                print(line, flush=True)
                f.write(line + "\n")
        return

    if a.sample:
        if world > 1:
            raise SystemExit("--sample runs on one GPU")
        with open(a.out, "a") as f:
            for leg in sample_bench(a, cfg, device):
                line = json.dumps(leg)
                print(line, flush=True)
                f.write(line + "\n")
        return

    if a.paged:
        if world > 1:
            raise SystemExit("--paged runs on one GPU")
        cfg.max_seq = 8192
        with open(a.out, "a") as f:
            for leg in paged_bench(a, cfg, device):
                line = json.dumps(leg)
                print(line, flush=True)
                f.write(line + "\n")
        return

    if a.kv_cache:
        if world > 1:
            raise SystemExit("--kv-cache runs on one GPU")
        cfg.max_seq = 8192
        with open(a.out, "a") as f:
            for leg in (kv8_online_bench if three_way else kv8_bench)(a, cfg, device):
                line = json.dumps(leg)
                print(line, flush=True)
                f.write(line + "\n")
        return

    if a.ragged:
        if world > 1:
            raise SystemExit("--ragged runs on one GPU")
        with open(a.out, "a") as f:
            for leg in ragged_bench(a, cfg, device):
                line = json.dumps(leg)
                print(line, flush=True)
                f.write(line + "\n")
        return

    def run(factory_cls, label):
        torch.cuda.reset_peak_memory_stats(device)
        fac = factory_cls(cfg, device, torch.bfloat16, seed=1 + rank) if factory_cls is DenseFactory else \
            factory_cls(cfg, device, torch.bfloat16, seed=1 + rank, kernel=a.kernel)
        if a.emulate_tp > 1:
            stack = DecodeStack(cfg, fac, device, torch.bfloat16, bs=a.bs, rank=0, world=a.emulate_tp, emulate_gather=True)
        else:
            stack = DecodeStack(cfg, fac, device, torch.bfloat16, bs=a.bs, rank=rank, world=world, gather=a.gather, fuse_gemm_stages=not a.no_fuse)
        graph = False
        if not a.no_graph:
            try:
                stack.capture()
                graph = True
            except Exception as e:  # noqa: BLE001  (symmetric across ranks: same code, same shapes)
                if rank == 0:
                    print(f"[{label}] graph capture failed ({type(e).__name__}: {e}); timing eager", file=sys.stderr)
                stack._graph = None
        dt = time_steps(stack, a.steps, a.warmup, a.start_pos)
        out = {"linears": label, "ms_per_token": round(dt * 1e3, 4), "tokens_per_s": round(a.bs / dt, 1),
               "hipgraph": graph, "peak_mem_mib": round(memory_allocated_mb(device), 1)}
        if label == "any4":
            out["weight_stream_GBps_all_ranks"] = round(cfg.weight_bytes_4bit() / dt / 1e9, 1)
        for pg in stack._peer.values():
            pg.check()
            pg.close()
        del stack, fac
        torch.cuda.empty_cache()
        return out

    res = {"config": a.config, "layers": cfg.layers, "bs": a.bs, "tp": world, "gather": a.gather if world > 1 else None,
           "ranks_share_one_gpu": bool(a.same_device), "emulated_tp_compute_only": a.emulate_tp or None, "max_seq": cfg.max_seq,
           "steps": a.steps, "warmup": a.warmup, "data": "synthetic (random weights, random tokens)",
           "algorithmic_4bit_bytes_per_token": cfg.weight_bytes_4bit()}
    res["any4"] = run(Any4Factory, "any4")
    if a.baseline:
        res["bf16"] = run(DenseFactory, "bf16")
        res["speedup_vs_bf16"] = round(res["bf16"]["ms_per_token"] / res["any4"]["ms_per_token"], 3)
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
