"""What the mx8 KV cache costs in accuracy on a synthetic stack (developer tool):
    python dev/kv8_accuracy.py [--config llama3_8b] [--layers N] [--prompt 512] [--new 64] [--out profiles/kv8_bench.jsonl]
Two fused stacks on the same random any4 weights and the same tokens, one with the 16-bit cache and one with kv_cache="mx8":
  prefill   max|a - b| / max|b| of the last token's logits after a prompt
  forced    the 16-bit stack's own greedy continuation fed to both: the same figure per step, and how often the two argmax agree
  free      both generate greedily on their own: the length of the common prefix of the two continuations
Random weights make flat logits (many near-ties), so argmax agreement here is a lower bound on what a trained model would show."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="llama3_8b", choices=["llama3_8b", "llama2_7b"])
ap.add_argument("--layers", type=int, default=None)
ap.add_argument("--prompt", type=int, default=512)
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--bs", type=int, default=2)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
cfg = getattr(DecodeConfig, a.config)(max_seq=a.prompt + a.new + 1)
if a.layers is not None:
    cfg.layers = a.layers
mk = lambda kv: DecodeStack(cfg, Any4Factory(cfg, dev, torch.bfloat16, seed=1), dev, torch.bfloat16, bs=a.bs, seed=2, kv_cache=kv)  # noqa: E731
s16, s8 = mk(None), mk("mx8")
toks = torch.randint(0, cfg.vocab, (a.bs, a.prompt), generator=torch.Generator().manual_seed(0)).to(dev)
gap = lambda x, y: ((x.float() - y.float()).abs().max() / y.float().abs().max()).item()  # noqa: E731
l16, l8 = s16.prefill(toks), s8.prefill(toks)
res = {"tool": "dev/kv8_accuracy.py", "config": a.config, "layers": cfg.layers, "bs": a.bs, "prompt": a.prompt, "new_tokens": a.new,
       "data": "synthetic (random weights, random tokens)", "prefill_logits_gap": round(gap(l8, l16), 5)}
gaps, agree, tok = [], 0, l16.argmax(-1)
agree += int((l8.argmax(-1) == tok).sum())
for i in range(a.new - 1):
    l16, l8 = s16.decode(tok, a.prompt + i), s8.decode(tok, a.prompt + i)
    gaps.append(gap(l8, l16))
    agree += int((l8.argmax(-1) == l16.argmax(-1)).sum())
    tok = l16.argmax(-1)
res["forced_logits_gap_max"], res["forced_logits_gap_mean"] = round(max(gaps), 5), round(sum(gaps) / len(gaps), 5)
res["forced_argmax_agreement"] = f"{agree} of {a.bs * a.new}"
g16, g8 = mk(None).generate(toks, a.new), mk("mx8").generate(toks, a.new)
res["free_common_prefix"] = [int(((g16[b] != g8[b]).nonzero()[:1].flatten().tolist() or [a.new])[0]) for b in range(a.bs)]
res["free_argmax_agreement"] = f"{int((g16 == g8).sum())} of {a.bs * a.new}"
line = json.dumps(res)
print(line, flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write(line + "\n")
