"""Back-to-back time of the sampler launch (dg_sample) by vocab, batch, temperature (0: passes 1 and 3 of sample.cuh only) and dtype:
    python dev/sample_probe.py > profiles/sample_probe.txt        """
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from any4_amd import decode_ops as G

dev = "cuda:0"
for dtype in (torch.bfloat16, torch.float16):
    for V in (1003, 32000, 128256):
        for bs in (1, 8):
            logits = (4 * torch.randn(bs, V, generator=torch.Generator().manual_seed(1))).to(dtype).to(dev)
            for T, k, p in ((0.0, 0, 1.0), (0.8, 0, 1.0), (0.8, 50, 0.95)):
                args = (torch.zeros(1, dtype=torch.long, device=dev), torch.full((bs,), T, device=dev), torch.full((bs,), k, dtype=torch.int32, device=dev),
                        torch.full((bs,), p, device=dev), torch.arange(bs, device=dev))
                tok = torch.empty(bs, dtype=torch.long, device=dev)
                for _ in range(20):
                    G.sample(logits, *args, token_out=tok)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                for _ in range(300):
                    G.sample(logits, *args, token_out=tok)
                ev[1].record()
                torch.cuda.synchronize()
                line = f"{str(dtype)[6:]:9s} V={V:6d} bs={bs} T={T} k={k:2d} p={p}: {ev[0].elapsed_time(ev[1]) / 300 * 1e3:7.2f} us"
                print(line, flush=True)
