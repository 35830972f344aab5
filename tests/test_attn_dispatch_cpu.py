"""CPU suite: which fused attention call a DecodeLayer launches for each kind of KV cache, and with which fields -- pinned without a GPU.
The library is replaced by a recorder (the device check and the stream lookup of decode_ops by no-ops), a fused stack is built on the
CPU, `layer.decode_attention` and `layer.prefill_attention` are called once each, and the one recorded dg_attn_launch -- the struct copied
at call time -- is compared with a literal, field by field: every pointer is named after the tensor it belongs to (`new`: a tensor the
call made, the output; None: null), every other field is its value.  A field that a row does not name must be null / zero.  Over all rows
the nineteen (kernel, flags) pairs of include/decode_glue_hip.h are launched."""
import ctypes
import math

import pytest
import torch

from any4_amd import _lib, decode_ops
from any4_amd.decode import DecodeConfig, DecodeStack, DenseFactory
from tests import attn_abi
from any4_amd._lib import (DG_ATTN_GENERAL as GENERAL, DG_ATTN_ONLINE as ONLINE, DG_ATTN_SPLIT as SPLIT, DG_ATTN_PREFILL as PREFILL,
                           DG_ATTN_SEQ as SEQ, DG_ATTN_MX8 as MX8, DG_ATTN_PAGED as PAGED, DG_ATTN_ONE_BARRIER as ONE_BARRIER)

BS, HL, KVL, T = 2, 2, 1, 3
S64, S32, S128 = 0.125, 1 / math.sqrt(32), 1 / math.sqrt(128)
HEAD, HEAD_SEQ = dict(qkv="qkv", cos="cos", sin="sin", pos="pos"), dict(qkv="qkv", cos="cos", sin="sin", pos="pos_seq")
PRE = dict(qkv="qkv", cos="cos", sin="sin", pos="prefill_pos", T=3)
PRE_SEQ = dict(qkv="qkv", cos="cos", sin="sin", pos="prefill_pos_seq", len="prefill_len", slot="prefill_slot", T=3, cache_bs=2)
KV = dict(k_cache="k_cache", v_cache="v_cache")
KV8 = dict(KV, k_exp="k_exp", v_exp="v_exp")
SCR = "_attn_scratch"


def pools(page_size, **more):
    return dict(table="block_table", k_cache="k_pool", v_cache="v_pool", page_size=page_size, num_pages=3, **more)


def pools8(page_size):
    return pools(page_size, k_exp="k_exp_pool", v_exp="v_exp_pool")


def split(scratch_bytes, nsplit):
    return dict(scratch=SCR, scratch_bytes=scratch_bytes, nsplit=nsplit)


def launch(kernel, flags, d, max_seq, scale, *pieces):
    """(kernel, flags, fields): the fields of every row (the output is the call's own, the dtype bf16) and the row's pieces"""
    fields = dict(out="new", bs=2, hl=2, kvl=1, d=d, max_seq=max_seq, scale=ctypes.c_float(scale).value, dtype=0)
    for piece in pieces:
        fields.update(piece)
    return kernel, flags, fields


# (id, head_dim, max_seq, DecodeStack keywords, decode launch, prefill launch)
ROWS = [
    ("16bit", 64, 128, dict(),
     launch(ONLINE, 0, 64, 128, S64, HEAD, KV),
     launch(PREFILL, 0, 64, 128, S64, PRE, KV)),
    ("16bit-ragged", 64, 128, dict(ragged=True),
     launch(ONLINE, SEQ, 64, 128, S64, HEAD_SEQ, KV),
     launch(PREFILL, SEQ, 64, 128, S64, PRE_SEQ, KV)),
    ("16bit-d32", 32, 128, dict(),
     launch(GENERAL, 0, 32, 128, S32, HEAD, KV),
     launch(PREFILL, 0, 32, 128, S32, PRE, KV)),
    ("16bit-d32-ragged", 32, 128, dict(ragged=True),
     launch(GENERAL, SEQ, 32, 128, S32, HEAD_SEQ, KV),
     launch(PREFILL, SEQ, 32, 128, S32, PRE_SEQ, KV)),
    ("16bit-2048", 64, 2048, dict(),
     launch(SPLIT, 0, 64, 2048, S64, HEAD, KV, split(4240, 4)),
     launch(PREFILL, 0, 64, 2048, S64, PRE, KV)),
    ("16bit-2048-ragged", 64, 2048, dict(ragged=True),
     launch(SPLIT, SEQ, 64, 2048, S64, HEAD_SEQ, KV, split(4240, 4)),
     launch(PREFILL, SEQ, 64, 2048, S64, PRE_SEQ, KV)),
    ("mx8-split", 64, 128, dict(kv_cache="mx8"),
     launch(SPLIT, MX8, 64, 128, S64, HEAD, KV8, split(1072, 1)),
     launch(PREFILL, MX8, 64, 128, S64, PRE, KV8)),
    ("mx8-split-ragged", 64, 128, dict(kv_cache="mx8", ragged=True),
     launch(SPLIT, MX8 | SEQ, 64, 128, S64, HEAD_SEQ, KV8, split(1072, 1)),
     launch(PREFILL, MX8 | SEQ, 64, 128, S64, PRE_SEQ, KV8)),
    ("mx8-online", 64, 128, dict(kv_cache="mx8", mx8_attention="online"),
     launch(SPLIT, MX8 | ONE_BARRIER, 64, 128, S64, HEAD, KV8, split(1072, 1)),
     launch(PREFILL, MX8, 64, 128, S64, PRE, KV8)),
    ("mx8-online-ragged", 64, 128, dict(kv_cache="mx8", mx8_attention="online", ragged=True),
     launch(SPLIT, MX8 | ONE_BARRIER | SEQ, 64, 128, S64, HEAD_SEQ, KV8, split(1072, 1)),
     launch(PREFILL, MX8 | SEQ, 64, 128, S64, PRE_SEQ, KV8)),
    ("paged", 64, 128, dict(ragged=True, kv_pages=3),
     launch(ONLINE, SEQ | PAGED, 64, 128, S64, HEAD_SEQ, pools(64)),
     launch(PREFILL, SEQ | PAGED, 64, 128, S64, PRE_SEQ, pools(64))),
    ("paged-2048", 64, 2048, dict(ragged=True, kv_pages=3),
     launch(SPLIT, SEQ | PAGED, 64, 2048, S64, HEAD_SEQ, pools(64), split(4240, 4)),
     launch(PREFILL, SEQ | PAGED, 64, 2048, S64, PRE_SEQ, pools(64))),
    ("paged-mx8", 64, 128, dict(ragged=True, kv_pages=3, kv_cache="mx8"),
     launch(SPLIT, SEQ | PAGED | MX8 | ONE_BARRIER, 64, 128, S64, HEAD_SEQ, pools8(64), split(1072, 1)),
     launch(PREFILL, SEQ | PAGED | MX8, 64, 128, S64, PRE_SEQ, pools8(64))),
    ("paged-mx8-online-d128", 128, 2048, dict(ragged=True, kv_pages=3, kv_cache="mx8", mx8_attention="online", page_size=128),
     launch(SPLIT, SEQ | PAGED | MX8 | ONE_BARRIER, 128, 2048, S128, HEAD_SEQ, pools8(128), split(8336, 4)),
     launch(PREFILL, SEQ | PAGED | MX8, 128, 2048, S128, PRE_SEQ, pools8(128))),
]
POINTERS = {name for name, t in _lib.Attn._fields_ if t is _lib._vp}


class Recorder:
    """Stands in for the loaded library: sizes and error strings come from the real one, every other call is recorded and succeeds."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith("_bytes") or name == "tg_error_string":
            return getattr(self.real, name)
        if name == "dg_attn_launch":  # (byref(struct), device, stream): the struct is the caller's to reuse, so it is copied now
            return lambda call, device, stream: self.calls.append((name, (_lib.Attn.from_buffer_copy(call._obj), device, stream))) or 0
        return lambda *args: self.calls.append((name, args)) or 0


def _named(call, roles):
    """A recorded launch as (kernel, flags, dtype and the fields that are not null / zero), every pointer replaced by the name of its tensor ("new":
    none of the named ones).  The struct says its own length; device (a CPU tensor has no index) and stream go beside it."""
    name, (a, device, stream) = call
    assert name == "dg_attn_launch" and a.struct_bytes == ctypes.sizeof(_lib.Attn) and device is None and stream == 0
    fields = {}
    for field, _ in _lib.Attn._fields_:
        v = getattr(a, field)
        if field in POINTERS:
            v = None if v is None else roles.get(v, "new")
        if field not in ("struct_bytes", "kernel", "flags") and (v not in (None, 0) or field == "dtype"):
            fields[field] = v
    return a.kernel, a.flags, fields


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
        assert got == want, got
        del roles[qkv.data_ptr()]


def test_the_rows_launch_exactly_the_nineteen_pairs_of_the_headers_table():
    """DG_ATTN_FLAVOURS of include/decode_glue_hip.h (each row asserts that its two pairs are launched)"""
    table = set(attn_abi.header_flavours().values())
    launched = {launch[:2] for row in ROWS for launch in row[4:]}
    assert len(table) == 19 and launched == table, sorted(launched ^ table)
