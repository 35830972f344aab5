"""CPU suite of the speculative-decoding verify pass: the C ABI of dg_verify_attn (struct mirror, symbols, every refusal with fake pointers
before any launch), speculative.accept_greedy on hand-written cases, DecodeStack.verify's refusals and its plain-torch formulation
against token-by-token decode, and generate_speculative's loop against generate.  No HIP compute."""
import ctypes
import re

import pytest
import torch

from any4_amd import _lib, speculative
from any4_amd.decode import DecodeConfig
from tests.attn_abi import CTYPE, header
from tests.test_decode_cpu import CFG
from tests.test_ragged_cpu import ATOL, _stack, _tokens

E_NULL, E_DTYPE, E_SHAPE, E_ALIGN, E_STRUCT = -1, -5, -7, -8, -14
P = 0x10000  # a fake, 16-byte aligned device pointer: every call below is refused before it would be read


def test_struct_mirror_and_symbols():
    body = re.search(r"typedef struct dg_verify \{(.*?)\} dg_verify;", header(), re.S).group(1)
    fields = []
    for line in body.strip().splitlines():
        kind, name = re.match(r"\s*([\w \*]+?)\s*\b(\w+);", line).groups()
        fields.append((name, _lib._vp if kind.endswith("*") else CTYPE[kind]))
    assert _lib.Verify._fields_ == fields and fields[0][0] == "struct_bytes"
    assert ctypes.sizeof(_lib.Verify) == sum(ctypes.sizeof(t) for _, t in fields)   # no hidden padding
    lib = _lib.load()
    assert lib.tg_abi_version() == 10
    for name in ("dg_verify_attn", "dg_verify_attn_scratch_bytes"):
        assert re.search(r"TG_API\s+\w+\s+" + name + r"\s*\(", header()) and getattr(lib, name).argtypes == _lib.SYMBOLS[name]
    assert lib.dg_verify_attn_scratch_bytes(2, 8, 128, 4, 1) == 0
    assert lib.dg_verify_attn_scratch_bytes(2, 8, 128, 4, 3) == 64 + 2 * 4 * 8 * 3 * 130 * 4


GOOD = dict(qkv=P, cos=P, sin=P, pos=P, k_cache=P, v_cache=P, out=P, scratch=P, scratch_bytes=1 << 30, bs=2, cache_bs=2, max_seq=1024, T=4,
            hl=8, kvl=2, d=128, nsplit=2, dtype=_lib.TG_BF16, scale=1.0)
REFUSALS = [
    (dict(struct_bytes=8), E_STRUCT), (dict(qkv=None), E_NULL), (dict(pos=None), E_NULL), (dict(out=None), E_NULL), (dict(scratch=None), E_NULL),
    (dict(dtype=7), E_DTYPE), (dict(d=96), E_SHAPE), (dict(d=256), E_SHAPE), (dict(T=0), E_SHAPE), (dict(T=9), E_SHAPE), (dict(nsplit=0), E_SHAPE),
    (dict(nsplit=65), E_SHAPE), (dict(hl=7), E_SHAPE), (dict(bs=0), E_SHAPE), (dict(cache_bs=3), E_SHAPE), (dict(max_seq=0), E_SHAPE),
    (dict(qkv=P + 8), E_ALIGN), (dict(cos=P + 4), E_ALIGN), (dict(k_cache=P + 2), E_ALIGN), (dict(out=P + 8), E_ALIGN), (dict(scratch=P + 8), E_ALIGN),
    (dict(scratch_bytes=64 + 2 * 4 * 8 * 2 * 130 * 4 - 1), E_SHAPE),
    (dict(d=96, qkv=P + 8), E_SHAPE), (dict(qkv=P + 8, scratch_bytes=0), E_ALIGN),   # the order: shape, alignment, the scratch's size
]


@pytest.mark.parametrize("change,code", REFUSALS)
def test_refusals_come_before_any_launch(change, code):
    lib = _lib.load()
    assert lib.dg_verify_attn(None, 0, None) == E_NULL
    assert lib.dg_verify_attn(ctypes.byref(_lib.Verify(**{**GOOD, **change})), 0, None) == code


@pytest.mark.parametrize("draft,target,accepted,nxt", [
    ([[5, 1, 2, 3]], [[9, 2, 3, 4]], [0], [9]),                                   # none accepted: the target's own token
    ([[5, 1, 2, 3]], [[1, 2, 3, 4]], [3], [4]),                                   # all accepted: the bonus token
    ([[5, 1, 2, 3]], [[1, 7, 3, 4]], [1], [7]),                                   # a mismatch in the middle hides later agreement
    ([[5, 1, 2, 3], [6, 4, 4, 4], [7, 0, 0, 0]], [[1, 2, 0, 0], [4, 4, 4, 8], [1, 0, 0, 0]], [2, 3, 0], [0, 8, 1]),
    ([[5]], [[3]], [0], [3]),                                                     # T = 1: a plain decode step
])
def test_accept_greedy(draft, target, accepted, nxt):
    a, n = speculative.accept_greedy(torch.tensor(draft), torch.tensor(target))
    assert a.tolist() == accepted and n.tolist() == nxt


def test_verify_refuses_what_is_not_built():
    cfg = DecodeConfig(**{**CFG, "hidden": 128, "head_dim": 32, "max_seq": 64})   # (a shape every cache layout accepts)
    toks = _tokens(cfg, 2, 4)
    for kw in (dict(ragged=False), dict(kv_cache="mx8"), dict(kv_pages=8)):
        from any4_amd.decode import DecodeStack
        from tests.test_decode_cpu import SeededDense

        s = DecodeStack(cfg, SeededDense(cfg, 0, 1), "cpu", torch.float32, bs=2, seed=7, **{"ragged": True, **kw})
        with pytest.raises(ValueError, match="not built yet"):
            s.verify(toks, 0)
    with pytest.raises(ValueError, match="not built yet"):
        _stack(cfg, 2).verify(_tokens(cfg, 2, 9), 0)


def test_verify_torch_formulation_and_generate_speculative():
    """Plain torch: verify's row t is decode's logits of token t; a decode after a partly rejected verify is unharmed by the dead rows;
    generate_speculative emits generate's tokens with a twin drafter (everything accepted) and with a drafter that knows nothing."""
    cfg = DecodeConfig(**CFG)
    toks, T = _tokens(cfg, 2, 12), 5
    a, b = _stack(cfg, 2), _stack(cfg, 2)
    a.prefill(toks[:, :4], position=0)
    b.prefill(toks[:, :4], position=0)
    got = a.verify(toks[:, 4:4 + T], [4, 4])
    want = torch.stack([b.decode(toks[:, 4 + t], [4 + t, 4 + t]).clone() for t in range(T)], dim=1)
    assert got.shape == want.shape and torch.allclose(got, want, atol=ATOL)
    other = (toks[:, 6] + 1) % cfg.vocab   # tokens 4, 5 accepted; position 6 takes another token over verify's dead rows
    assert torch.allclose(a.decode(other, [6, 6]), b.decode(other, [6, 6]), atol=ATOL)
    prompt = toks[:, :3]
    want = _stack(cfg, 2).generate(prompt, 6)
    out, mean = speculative.generate_speculative(_stack(cfg, 2), _stack(cfg, 2), prompt, 6, 3)
    assert torch.equal(out, want) and mean == 3
    out, mean = speculative.generate_speculative(_stack(cfg, 2), lambda seqs, k: torch.zeros(2, k, dtype=torch.long), prompt, 6, 2)
    assert torch.equal(out, want) and mean < 2
