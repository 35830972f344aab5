#!/usr/bin/env python3
"""Digests of what the plain-torch decode stack computes, without a GPU: run it around every change of any4_amd/decode.py that should
not move a bit.

    python dev/decode_digests.py [--decode PATH]

Tiny seeded `DenseFactory` stacks on the CPU (fused=False; hidden 64, 2 layers, 4 / 2 heads of 16, max_seq 32, bs 3), float32 and
bfloat16, ragged and not.  After each stage -- a chunked prefill, three decode steps, `generate`; on the ragged stack also a step with
an inactive sequence, a prefill of two sequences into named slots at different positions and lengths, and `generate` over prompts of
different lengths with `eos` -- sha256 over the stage's result and the bytes of every cache tensor a layer has (of k_cache, v_cache,
k_exp, v_exp, k_pool, v_pool, k_exp_pool, v_exp_pool).  One line per (dtype, stack), with the stages' digests shortened, and the digest
of all of them.  Behind those four lines, the other kinds of cache on a second geometry (hidden 128, 2 layers, 2 / 1 heads of 64, max_seq
128, bs 3; ragged): kv_cache="mx8", kv_pages=5, and both -- the ragged stages, then a prefill and a step across a page boundary and, on
the paged ones, a fork with a partial page and a step behind it.  --decode PATH runs another copy of decode.py (an older commit's:
`git show REV:any4_amd/decode.py > /tmp/decode_old.py`) in place of the tree's; two copies compute the same when the lines agree (a
copy that does not know a kind of cache prints so in that line).
"""
import argparse
import hashlib
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def load_decode(path):
    if path is None:
        from any4_amd import decode
        return decode
    spec = importlib.util.spec_from_file_location("any4_amd.decode", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["any4_amd.decode"] = mod
    spec.loader.exec_module(mod)
    return mod


CACHE_NAMES = ("k_cache", "v_cache", "k_exp", "v_exp", "k_pool", "v_pool", "k_exp_pool", "v_exp_pool")


def digest(stack, *results):
    h = hashlib.sha256()
    caches = [getattr(layer, name, None) for layer in stack.layers for name in CACHE_NAMES]
    for t in list(results) + [c for c in caches if c is not None]:
        h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_stages(stack, toks, T, ragged):
    stages = [("prefill", digest(stack, stack.prefill(toks[:, :T], position=2, chunk=3)))]
    for i in range(3):
        stages.append((f"step{i}", digest(stack, stack.decode(toks[:, T + i], 2 + T + i))))
    stages.append(("generate", digest(stack, stack.generate(toks[:, :5], 4))))
    if ragged:
        stages.append(("inactive", digest(stack, stack.decode(toks[:, 12], [9, -1, 9])[[0, 2]])))
        stages.append(("slots", digest(stack, stack.prefill(toks[:2, 8:12], position=[3, 0], lengths=[4, 2], slots=[2, 0], chunk=3))))
        prompts = [toks[0, :2], toks[1, :6], toks[2, :4]]
        first = stack.generate(prompts, 5)
        stages.append(("generate-list", digest(stack, first)))
        stages.append(("generate-eos", digest(stack, stack.generate(prompts, 5, eos=int(first[1, 2])))))
    return stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode", default=None, help="another copy of decode.py to run in place of any4_amd/decode.py")
    a = ap.parse_args()
    D = load_decode(a.decode)
    cfg = D.DecodeConfig(hidden=64, inter=128, layers=2, heads=4, kv_heads=2, head_dim=16, vocab=97, max_seq=32, group_size=32)
    bs, T = 3, 7
    toks = torch.randint(0, cfg.vocab, (bs, 16), generator=torch.Generator().manual_seed(5))
    total = hashlib.sha256()
    for dtype in (torch.float32, torch.bfloat16):
        for ragged in (False, True):
            stack = D.DecodeStack(cfg, D.DenseFactory(cfg, "cpu", dtype, seed=3), "cpu", dtype, bs=bs, seed=4, fused=False, ragged=ragged)
            stages = run_stages(stack, toks, T, ragged)
            for _, d in stages:
                total.update(d.encode())
            print(f"{str(dtype).split('.')[-1]:8s} {'ragged' if ragged else 'plain ':6s} " + " ".join(f"{n}={d[:12]}" for n, d in stages))
    print("all of the four lines above", total.hexdigest())
    # the other kinds of cache: 64-wide heads (what a paged mx8 cache needs), pages of 64 positions, two of them per slot
    cfg = D.DecodeConfig(hidden=128, inter=128, layers=2, heads=2, kv_heads=1, head_dim=64, vocab=97, max_seq=128, group_size=32)
    for label, kw in (("mx8", dict(kv_cache="mx8")), ("paged", dict(kv_pages=5)), ("paged-mx8", dict(kv_cache="mx8", kv_pages=5))):
        for dtype in (torch.float32, torch.bfloat16):
            name = f"{str(dtype).split('.')[-1]:8s} {label:9s} "
            try:
                stack = D.DecodeStack(cfg, D.DenseFactory(cfg, "cpu", dtype, seed=3), "cpu", dtype, bs=bs, seed=4, fused=False, ragged=True, **kw)
            except (TypeError, ValueError) as e:
                print(name + f"not in this decode.py ({e})")
                continue
            stages = run_stages(stack, toks, T, True)
            stages.append(("cross", digest(stack, stack.prefill(toks[:1, :10], position=[59], lengths=[10], slots=[1], chunk=4))))
            stages.append(("step-cross", digest(stack, stack.decode(toks[:, 13], [12, 69, -1])[:2])))
            if "kv_pages" in kw:
                stack.fork(1, 2, 70)  # a whole shared page and six rows copied into a fresh one
                stages.append(("fork", digest(stack, stack.block_table)))
                stages.append(("step-fork", digest(stack, stack.decode(toks[:, 14], [13, 70, 70]))))
            for _, d in stages:
                total.update(d.encode())
            print(name + " ".join(f"{n}={d[:12]}" for n, d in stages))
    print("all", total.hexdigest())


if __name__ == "__main__":
    main()
