"""GPU suite: DecodeStack.verify and speculative.generate_speculative on the fused path, against token-by-token `decode` on a twin stack
under the stack contract of tests/test_gpu_decode.py: max|a - b| <= 0.03 max|b| + 1e-3.  max_seq 2048 gives the verify kernel four
blocks over the context (and a scratch), as a stack of that capacity has."""
import pytest
import torch

from any4_amd import speculative
from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_numerics")]
DEV = "cuda:0"
CFG = dict(hidden=256, inter=512, layers=2, heads=4, kv_heads=2, head_dim=64, vocab=128, max_seq=2048, group_size=64)


def _stack(seed=3):
    cfg = DecodeConfig(**CFG)
    return DecodeStack(cfg, Any4Factory(cfg, DEV, seed=seed), DEV, bs=2, seed=seed + 6, ragged=True)


def _close(a, b):
    a, b = a.float(), b.float()
    assert torch.isfinite(a).all() and (a - b).abs().max() <= 0.03 * b.abs().max() + 1e-3, ((a - b).abs().max(), b.abs().max())


def test_verify_logits_are_decode_logits_and_dead_rows_are_harmless():
    gen = torch.Generator().manual_seed(1)
    prompt, toks = torch.randint(0, 128, (2, 70), generator=gen).to(DEV), torch.randint(0, 128, (2, 5), generator=gen).to(DEV)
    a, b = _stack(), _stack()
    lens = [70, 13]   # (a second 64-position tile for one sequence, the chunk straddling nothing for the other)
    for s in (a, b):
        s.prefill(prompt, position=0, lengths=lens)
    assert a._verify_split == 4 and not a._verify_scratch
    got = a.verify(toks, lens)
    assert 2 in a._verify_scratch and got.shape == (2, 5, 128)
    for t in range(5):
        _close(got[:, t], b.decode(toks[:, t], [n + t for n in lens]))
    other = (toks[:, 2] + 1) % 128   # one draft accepted: position + 2 takes another token, over the rows verify left there
    _close(a.decode(other, [n + 2 for n in lens]), b.decode(other, [n + 2 for n in lens]))


@pytest.mark.parametrize("drafter", ["twin", "stranger"])
def test_generate_speculative_emits_the_targets_greedy_tokens(drafter):
    k, new = 3, 12
    prompt = torch.randint(0, 128, (2, 9), generator=torch.Generator().manual_seed(2)).to(DEV)
    out, mean = speculative.generate_speculative(_stack(), _stack(3 if drafter == "twin" else 11), prompt, new, k)
    assert out.shape == (2, new) and (mean > 0 if drafter == "twin" else mean < k), mean
    replay = _stack()
    logits = replay.prefill(prompt, position=0)
    for j in range(new):   # every emitted token is an arg-max of the token-by-token logits, up to the numeric contract
        lg = logits.float()
        picked = lg.gather(1, out[:, j:j + 1]).squeeze(1)
        assert (lg.max(dim=1).values - picked <= 0.03 * lg.abs().max(dim=1).values + 1e-3).all(), (j, out[:, j].tolist())
        logits = replay.decode(out[:, j], 9 + j)
