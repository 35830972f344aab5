"""CPU suite: which fused attention entry point a DecodeLayer launches for each kind of KV cache, and with which arguments -- pinned
without a GPU.  The library is replaced by a recorder (the device check and the stream lookup of decode_ops by no-ops), a fused stack is
built on the CPU, `layer.decode_attention` and `layer.prefill_attention` are called once each, and the one recorded launch is compared
with a literal: every pointer is named after the tensor it belongs to (`new`: a tensor the call made, the output), every other
argument is its value, in the order of include/decode_glue_hip.h.  Over all rows the nineteen fused attention symbols are launched."""
import math

import pytest
import torch

from any4_amd import _lib, decode_ops
from any4_amd.decode import DecodeConfig, DecodeStack, DenseFactory

BS, HL, KVL, T = 2, 2, 1, 3
TAIL = [0, None, 0]                              # dtype (bf16), device (a CPU tensor has no index), stream
S64, S32, S128 = 0.125, 1 / math.sqrt(32), 1 / math.sqrt(128)
HEAD, HEAD_SEQ = ["qkv", "cos", "sin", "pos"], ["qkv", "cos", "sin", "pos_seq"]
PRE, PRE_SEQ = ["qkv", "cos", "sin", "prefill_pos"], ["qkv", "cos", "sin", "prefill_pos_seq", "prefill_len", "prefill_slot"]
KV, KV8 = ["k_cache", "v_cache"], ["k_cache", "v_cache", "k_exp", "v_exp"]
POOLS, POOLS8 = ["block_table", "k_pool", "v_pool"], ["block_table", "k_pool", "v_pool", "k_exp_pool", "v_exp_pool"]
SCR = "_attn_scratch"

# (id, head_dim, max_seq, DecodeStack keywords, decode launch, prefill launch)
ROWS = [
    ("16bit", 64, 128, dict(),
     ("dg_rope_attn_online", HEAD + KV + ["new", 2, 2, 1, 64, 128, S64] + TAIL),
     ("dg_prefill_attn", PRE + KV + ["new", 2, 3, 2, 1, 64, 128, S64] + TAIL)),
    ("16bit-ragged", 64, 128, dict(ragged=True),
     ("dg_rope_attn_online_seq", HEAD_SEQ + KV + ["new", 2, 2, 1, 64, 128, S64] + TAIL),
     ("dg_prefill_attn_seq", PRE_SEQ + KV + ["new", 2, 3, 2, 2, 1, 64, 128, S64] + TAIL)),
    ("16bit-d32", 32, 128, dict(),
     ("dg_rope_attn", HEAD + KV + ["new", 2, 2, 1, 32, 128, S32] + TAIL),
     ("dg_prefill_attn", PRE + KV + ["new", 2, 3, 2, 1, 32, 128, S32] + TAIL)),
    ("16bit-d32-ragged", 32, 128, dict(ragged=True),
     ("dg_rope_attn_seq", HEAD_SEQ + KV + ["new", 2, 2, 1, 32, 128, S32] + TAIL),
     ("dg_prefill_attn_seq", PRE_SEQ + KV + ["new", 2, 3, 2, 2, 1, 32, 128, S32] + TAIL)),
    ("16bit-2048", 64, 2048, dict(),
     ("dg_rope_attn_split", HEAD + KV + ["new", SCR, 4240, 2, 2, 1, 64, 2048, S64, 4] + TAIL),
     ("dg_prefill_attn", PRE + KV + ["new", 2, 3, 2, 1, 64, 2048, S64] + TAIL)),
    ("16bit-2048-ragged", 64, 2048, dict(ragged=True),
     ("dg_rope_attn_split_seq", HEAD_SEQ + KV + ["new", SCR, 4240, 2, 2, 1, 64, 2048, S64, 4] + TAIL),
     ("dg_prefill_attn_seq", PRE_SEQ + KV + ["new", 2, 3, 2, 2, 1, 64, 2048, S64] + TAIL)),
    ("mx8-split", 64, 128, dict(kv_cache="mx8"),
     ("dg_rope_attn_split_mx8", HEAD + KV8 + ["new", SCR, 1072, 2, 2, 1, 64, 128, S64, 1] + TAIL),
     ("dg_prefill_attn_mx8", PRE + KV8 + ["new", 2, 3, 2, 1, 64, 128, S64] + TAIL)),
    ("mx8-split-ragged", 64, 128, dict(kv_cache="mx8", ragged=True),
     ("dg_rope_attn_split_mx8_seq", HEAD_SEQ + KV8 + ["new", SCR, 1072, 2, 2, 1, 64, 128, S64, 1] + TAIL),
     ("dg_prefill_attn_mx8_seq", PRE_SEQ + KV8 + ["new", 2, 3, 2, 2, 1, 64, 128, S64] + TAIL)),
    ("mx8-online", 64, 128, dict(kv_cache="mx8", mx8_attention="online"),
     ("dg_rope_attn_online_mx8", HEAD + KV8 + ["new", SCR, 1072, 2, 2, 1, 64, 128, S64, 1] + TAIL),
     ("dg_prefill_attn_mx8", PRE + KV8 + ["new", 2, 3, 2, 1, 64, 128, S64] + TAIL)),
    ("mx8-online-ragged", 64, 128, dict(kv_cache="mx8", mx8_attention="online", ragged=True),
     ("dg_rope_attn_online_mx8_seq", HEAD_SEQ + KV8 + ["new", SCR, 1072, 2, 2, 1, 64, 128, S64, 1] + TAIL),
     ("dg_prefill_attn_mx8_seq", PRE_SEQ + KV8 + ["new", 2, 3, 2, 2, 1, 64, 128, S64] + TAIL)),
    ("paged", 64, 128, dict(ragged=True, kv_pages=3),
     ("dg_rope_attn_online_paged", HEAD_SEQ + POOLS + ["new", 2, 2, 1, 64, 128, 64, 3, S64] + TAIL),
     ("dg_prefill_attn_paged", PRE_SEQ + POOLS + ["new", 2, 3, 2, 2, 1, 64, 128, 64, 3, S64] + TAIL)),
    ("paged-2048", 64, 2048, dict(ragged=True, kv_pages=3),
     ("dg_rope_attn_split_paged", HEAD_SEQ + POOLS + ["new", SCR, 4240, 2, 2, 1, 64, 2048, 64, 3, S64, 4] + TAIL),
     ("dg_prefill_attn_paged", PRE_SEQ + POOLS + ["new", 2, 3, 2, 2, 1, 64, 2048, 64, 3, S64] + TAIL)),
    ("paged-mx8", 64, 128, dict(ragged=True, kv_pages=3, kv_cache="mx8"),
     ("dg_rope_attn_online_mx8_paged", HEAD_SEQ + POOLS8 + ["new", SCR, 1072, 2, 2, 1, 64, 128, 64, 3, S64, 1] + TAIL),
     ("dg_prefill_attn_mx8_paged", PRE_SEQ + POOLS8 + ["new", 2, 3, 2, 2, 1, 64, 128, 64, 3, S64] + TAIL)),
    ("paged-mx8-online-d128", 128, 2048, dict(ragged=True, kv_pages=3, kv_cache="mx8", mx8_attention="online", page_size=128),
     ("dg_rope_attn_online_mx8_paged", HEAD_SEQ + POOLS8 + ["new", SCR, 8336, 2, 2, 1, 128, 2048, 128, 3, S128, 4] + TAIL),
     ("dg_prefill_attn_mx8_paged", PRE_SEQ + POOLS8 + ["new", 2, 3, 2, 2, 1, 128, 2048, 128, 3, S128] + TAIL)),
]
ARGTYPES = {**_lib.SYMBOLS, **_lib.PAGED_SYMBOLS, **_lib.KV8_ONLINE_SYMBOLS, **_lib.PAGED_MX8_SYMBOLS}
NINETEEN = {name for name in ARGTYPES if name.startswith(("dg_rope_attn", "dg_prefill_attn")) and not name.endswith("_bytes")}


class Recorder:
    """Stands in for the loaded library: sizes and error strings come from the real one, every other call is recorded and succeeds."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith("_bytes") or name == "tg_error_string":
            return getattr(self.real, name)
        return lambda *args: self.calls.append((name, args)) or 0


def _named(call, roles):
    """A recorded launch with every pointer argument replaced by the name of its tensor ("new": none of the named ones)."""
    name, args = call
    types = ARGTYPES[name]
    assert len(args) == len(types), name
    return name, [roles.get(a, "new") if t is _lib._vp and a not in (None, 0) else a for a, t in zip(args, types)]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_one_launch_per_call_with_the_arguments_of_the_cache(row, monkeypatch):
    _, d, S, kw, want_decode, want_prefill = row
    rec = Recorder(_lib.load())
    monkeypatch.delenv("ANY4_ATTN_SPLIT", raising=False)
    monkeypatch.setattr(decode_ops, "_gpu", lambda *ts: None)
    monkeypatch.setattr(decode_ops, "_stream", lambda t: 0)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    cfg = DecodeConfig(hidden=2 * d, inter=64, layers=1, heads=HL, kv_heads=KVL, head_dim=d, vocab=32, max_seq=S, group_size=32)
    stack = DecodeStack(cfg, DenseFactory(cfg, "cpu", torch.bfloat16), "cpu", torch.bfloat16, bs=BS, fused=True, lm_head=False, **kw)
    layer, ragged = stack.layers[0], bool(kw.get("ragged"))
    roles = {}
    for owner, names in ((stack, ("cos", "sin", "pos", "pos_seq", "prefill_pos", "prefill_pos_seq", "prefill_len", "prefill_slot", "block_table",
                                  "_attn_scratch")),
                         (layer, ("k_cache", "v_cache", "k_exp", "v_exp", "k_pool", "v_pool", "k_exp_pool", "v_exp_pool"))):
        for name in names:
            if getattr(owner, name, None) is not None:
                assert roles.setdefault(getattr(owner, name).data_ptr(), name) == name
    for rows, want in ((BS, want_decode), (BS * T, want_prefill)):
        qkv = torch.zeros(rows, (HL + 2 * KVL) * d, dtype=torch.bfloat16)
        roles[qkv.data_ptr()] = "qkv"
        del rec.calls[:]
        if rows == BS:
            layer.decode_attention(qkv, stack.pos_seq if ragged else stack.pos, stack.cos, stack.sin, per_sequence=ragged)
        elif ragged:
            layer.prefill_attention(qkv, stack.prefill_pos_seq, stack.cos, stack.sin, T=T, lengths=stack.prefill_len, slots=stack.prefill_slot,
                                    per_sequence=True)
        else:
            layer.prefill_attention(qkv, stack.prefill_pos, stack.cos, stack.sin)
        assert len(rec.calls) == 1, [c[0] for c in rec.calls]
        got = _named(rec.calls[0], roles)
        assert got == (want[0], want[1]), got
        del roles[qkv.data_ptr()]


def test_the_rows_launch_exactly_the_nineteen_fused_attention_symbols():
    """The twelve, the three `_paged`, the two `_online_mx8` and the two `_mx8_paged` (each row asserts that its two names are launched)."""
    named = {launch[0] for row in ROWS for launch in row[4:]}
    assert len(NINETEEN) == 19 and named == NINETEEN, sorted(named ^ NINETEEN)
