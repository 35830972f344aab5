"""What the CPU suites share about the fused attention ABI (include/decode_glue_hip.h): the header's struct and its table of accepted
calls, parsed; and one call of dg_attn_launch by flavour name, which is how the precondition tests issue their calls -- fake pointers, no
GPU: every call they make returns a TG_E_* code before the first HIP call."""
import ctypes
import os
import re

from any4_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "decode_glue_hip.h")
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
ALIASES = {"k": "k_cache", "v": "v_cache", "k_pool": "k_cache", "v_pool": "v_cache", "n": "bs"}   # names the tests' argument sets use


def header():
    with open(HEADER) as f:
        return f.read()


def header_fields():
    """[(name, ctype)] of `struct dg_attn`, in the header's order; a pointer of any kind is a c_void_p"""
    body = re.search(r"typedef struct dg_attn \{(.*?)\} dg_attn;", header(), re.S).group(1)
    fields = []
    for line in body.strip().splitlines():
        kind, name = re.match(r"\s*([\w \*]+?)\s*\b(\w+);", line).groups()
        fields.append((name, _lib._vp if kind.endswith("*") else CTYPE[kind]))
    return fields


def header_constants():
    """{name: value} of the DG_ATTN_* kernels (the enum) and flag bits (the #defines)"""
    text = header()
    values = {name: int(v) for name, v in re.findall(r"^\s*(DG_ATTN_\w+) = (\d+),?$", text, re.M)}
    values.update({name: int(v) for name, v in re.findall(r"^#define (DG_ATTN_\w+) (\d+)u$", text, re.M)})
    return values


def header_flavours():
    """{name up to ABI 8: (kernel, flags)}: DG_ATTN_FLAVOURS"""
    consts = header_constants()
    return {name: (eval(kernel, consts), eval(flags, consts)) for name, kernel, flags in re.findall(r"^\s*X\((dg_\w+), (\w+), ([^)]+)\)", header(), re.M)}


PAIR = {name: pair for pair, name in _lib.ATTN_FLAVOURS.items()}


def launch(L, what, device=0, stream=None, struct_bytes=None, **fields):
    """dg_attn_launch of the flavour `what` (a name of the header's table, or a (kernel, flags) pair) with these fields"""
    kernel, flags = PAIR[what] if isinstance(what, str) else what
    a = _lib.Attn(kernel=kernel, flags=flags)
    for name, value in fields.items():
        setattr(a, ALIASES.get(name, name), value.value if isinstance(value, ctypes.c_void_p) else value)
    if struct_bytes is not None:
        a.struct_bytes = struct_bytes
    return L.dg_attn_launch(ctypes.byref(a), device, stream)
