"""ctypes binding of include/tinygemm_hip.h.  No fallbacks: if the HIP library is missing the
import fails loudly (build it with `python -m any4_amd.build`)."""
from __future__ import annotations

import ctypes
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtinygemm_hip.so")

TG_BF16, TG_F16 = 0, 1
TG_Q_INT4, TG_Q_ANY4_GLOBAL, TG_Q_ANY4_ROWWISE, TG_Q_MX4, TG_Q_INT8 = 0, 1, 2, 3, 4
TG_NUM_FAST, TG_NUM_REFERENCE, TG_NUM_FAST_MFMA, TG_NUM_FAST_DOT2 = 0, 1, 2, 3
TG_ABI_VERSION = 8
TG_PLAN_SPLITK, TG_PLAN_STREAM, TG_PLAN_PAIR, TG_PLAN_PAIR_XR, TG_PLAN_GEMV, TG_PLAN_TILE = 1, 2, 3, 4, 5, 6
TG_PLAN_PAIR_M1_LEAN = 7  # tg_gemm_w4_plan_detail only
TG_LAYOUT_RM, TG_LAYOUT_TC_A = 0, 1
TG_E_LAYOUT = -12
TG_E_FUSION = -13
TG_E_STRUCT = -14
TG_EPI_NONE, TG_EPI_SWIGLU = 0, 1
TG_WFMT_M16N8K16, TG_WFMT_ROWS = 0, 1

_i32, _i64, _vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


class W4Gemm(ctypes.Structure):
    """struct tg_w4_gemm (include/tinygemm_hip.h)"""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32), ("struct_reserved", ctypes.c_uint32),
        ("x", _vp), ("w", _vp), ("qinfo", _vp), ("lut", _vp), ("y", _vp),
        ("m", _i64), ("wrows", _i64), ("k", _i64),
        ("group", _i32), ("qtype", _i32), ("dtype", _i32), ("w_on_right", _i32), ("inner_k_tiles", _i32),
        ("batch", _i32),
        ("stride_x", _i64), ("stride_w", _i64), ("stride_qinfo", _i64), ("stride_lut", _i64), ("stride_y", _i64),
        ("numerics", _i32), ("reserved", _i32), ("bias", _vp), ("stride_bias", _i64),
        ("workspace", _vp), ("workspace_bytes", _i64),
        ("x_layout", _i32), ("y_layout", _i32),
        ("bias_row_stride", _i64), ("norm_weight", _vp), ("norm_eps", ctypes.c_float), ("epilogue", _i32),
        ("w_format", _i32), ("reserved6", _i32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if "struct_bytes" not in kw:  # ABI 6: the struct says how long it is
            self.struct_bytes = ctypes.sizeof(W4Gemm)


TG_PEER_MAX_WORLD = 16


class PeerHandle(ctypes.Structure):
    """struct tg_peer_handle (include/peer_gather_hip.h): a hipIpcMemHandle_t"""

    _fields_ = [("bytes", ctypes.c_ubyte * 64)]


class PeerGather(ctypes.Structure):
    """struct tg_peer_gather (include/peer_gather_hip.h)"""

    _fields_ = [
        ("src", _vp), ("dst", _vp * TG_PEER_MAX_WORLD), ("flags", _vp * TG_PEER_MAX_WORLD), ("seq", _vp), ("status", _vp),
        ("world", _i32), ("rank", _i32), ("m", _i64), ("cols_local", _i64), ("timeout_us", _i64),
    ]


# The twelve fused attention entry points of include/decode_glue_hip.h: four bases, each with a `_seq` flavour (a position per sequence), two of
# them with `_mx8` ones (an mx8 KV cache) -- and, bound as a group of their own (PAGED_SYMBOLS; the header declares them DG_PAGED_API), the
# `_paged` flavour of three bases (a page pool behind a block table; per sequence, 16-bit rows) -- and, a group of their own too (KV8_ONLINE_SYMBOLS;
# DG_KV8_API), dg_rope_attn_online_mx8(_seq): the one-barrier kernel on an mx8 cache (kv8_online_signature) -- and, again a group of their own
# (PAGED_MX8_SYMBOLS; DG_PAGED_KV8_API), dg_rope_attn_online_mx8_paged / dg_prefill_attn_mx8_paged: mx8 page pools (paged_mx8_signature).  Their argument lists are these pieces, by name: SYMBOLS takes the types, decode_ops.attn_args
# puts a call's values in the same order.
_ci, _cf = ctypes.c_int, ctypes.c_float
ATTN_BASES = {"dg_rope_attn": False, "dg_rope_attn_online": False, "dg_rope_attn_split": True, "dg_prefill_attn": True}  # base: has _mx8 flavours
_ATTN_HEAD = [("qkv", _vp), ("cos", _vp), ("sin", _vp), ("pos", _vp)]
_ATTN_LEN_SLOT = [("len", _vp), ("slot", _vp)]                      # dg_prefill_attn*_seq
_ATTN_CACHES = [("k_cache", _vp), ("v_cache", _vp)]
_ATTN_POOLS = [("table", _vp), ("k_pool", _vp), ("v_pool", _vp)]   # *_paged
_ATTN_PAGES = [("page_size", _i64), ("num_pages", _i64)]            # *_paged, behind max_seq
ATTN_PAGED_BASES = ("dg_rope_attn_online", "dg_rope_attn_split", "dg_prefill_attn")
_ATTN_EXPS = [("k_exp", _vp), ("v_exp", _vp)]                       # *_mx8*
_ATTN_SCRATCH = [("scratch", _vp), ("scratch_bytes", _i64)]         # dg_rope_attn_split*
_ATTN_SHAPE = [("hl", _ci), ("kvl", _ci), ("d", _ci), ("max_seq", _i64), ("scale", _cf)]
_ATTN_TAIL = [("dtype", _ci), ("device", _ci), ("stream", _vp)]


@functools.lru_cache(maxsize=None)
def attn_signature(base, seq=False, mx8=False, paged=False):
    """(entry point, ((argument name, ctype), ...)) of one flavour of an attention base (paged: the `_paged` one, which is per sequence)"""
    if base not in ATTN_BASES or (mx8 and not ATTN_BASES[base]) or (paged and (mx8 or base not in ATTN_PAGED_BASES)):
        raise KeyError(f"no attention entry point {base}{'_mx8' if mx8 else ''}{'_paged' if paged else ''}")
    seq = seq or paged
    prefill, split = base == "dg_prefill_attn", base == "dg_rope_attn_split"
    shape = _ATTN_SHAPE[:4] + _ATTN_PAGES + _ATTN_SHAPE[4:] if paged else _ATTN_SHAPE
    args = (_ATTN_HEAD + (_ATTN_LEN_SLOT if prefill and seq else []) + (_ATTN_POOLS if paged else _ATTN_CACHES) + (_ATTN_EXPS if mx8 else [])
            + [("out", _vp)] + (_ATTN_SCRATCH if split else []) + [("bs", _i64)] + ([("T", _i64)] if prefill else [])
            + ([("cache_bs", _i64)] if prefill and seq else []) + shape + ([("nsplit", _ci)] if split else []) + _ATTN_TAIL)
    return base + ("_paged" if paged else ("_mx8" if mx8 else "") + ("_seq" if seq else "")), tuple(args)


def kv8_online_signature(seq=False):
    """(entry point, ((argument name, ctype), ...)) of dg_rope_attn_online_mx8(_seq): the one-barrier kernel on an mx8 cache, which takes
    the argument list of dg_rope_attn_split_mx8(_seq).  A function of its own: attn_signature("dg_rope_attn_online", mx8=True) stays a
    KeyError, as that base has no `_mx8` flavour among the twelve."""
    args = (_ATTN_HEAD + _ATTN_CACHES + _ATTN_EXPS + [("out", _vp)] + _ATTN_SCRATCH + [("bs", _i64)] + _ATTN_SHAPE + [("nsplit", _ci)]
            + _ATTN_TAIL)
    return "dg_rope_attn_online_mx8" + ("_seq" if seq else ""), tuple(args)


ATTN_PAGED_MX8_BASES = ("dg_rope_attn_online", "dg_prefill_attn")


def paged_mx8_signature(base):
    """(entry point, ((argument name, ctype), ...)) of dg_rope_attn_online_mx8_paged / dg_prefill_attn_mx8_paged: mx8 page pools behind the
    block table -- the `_paged` list of dg_rope_attn_split / dg_prefill_attn with the exponent pools behind the code pools.  A function of
    its own: attn_signature(base, mx8=True, paged=True) stays a KeyError, the twelve and the three paged ones are what they were."""
    if base not in ATTN_PAGED_MX8_BASES:
        raise KeyError(f"no attention entry point {base}_mx8_paged")
    prefill = base == "dg_prefill_attn"
    args = (_ATTN_HEAD + (_ATTN_LEN_SLOT if prefill else []) + _ATTN_POOLS + _ATTN_EXPS + [("out", _vp)] + ([] if prefill else _ATTN_SCRATCH)
            + [("bs", _i64)] + ([("T", _i64), ("cache_bs", _i64)] if prefill else []) + _ATTN_SHAPE[:4] + _ATTN_PAGES + _ATTN_SHAPE[4:]
            + ([] if prefill else [("nsplit", _ci)]) + _ATTN_TAIL)
    return base + "_mx8_paged", tuple(args)


# name -> argtypes, exactly the prototypes of include/tinygemm_hip.h
SYMBOLS = {
    "tg_abi_version": [],
    "tg_m1_default_contraction": [],
    "tg_error_string": [ctypes.c_int],
    "tg_convert_to_Bint4": [_vp, _i64, _i64, ctypes.c_int, _vp, ctypes.c_int, _vp],
    "tg_convert_to_Aint4": [_vp, _i64, _i64, ctypes.c_int, _vp, ctypes.c_int, _vp],
    "tg_convert_to_A16": [_vp, _i64, _i64, _vp, ctypes.c_int, _vp],
    "tg_convert_from_A16": [_vp, _i64, _i64, _vp, ctypes.c_int, _vp],
    "tg_convert_to_B16": [_vp, _i64, _i64, ctypes.c_int, _vp, ctypes.c_int, _vp],
    "tg_convert_from_B16": [_vp, _i64, _i64, ctypes.c_int, _vp, ctypes.c_int, _vp],
    "tg_dequant_int4": [_vp, _i64, _vp, ctypes.c_int, _vp],
    "tg_unpack_int4": [_vp, ctypes.c_int, _i64, _i64, ctypes.c_int, _vp, ctypes.c_int, _vp],
    "tg_dequant_w4": [_vp, _vp, _vp, _i64, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp],
    "tg_dequant_w4_panel": [_vp, _vp, _vp, _i64, _i64, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp],
    "tg_gemm_w4": [ctypes.POINTER(W4Gemm), ctypes.c_int, _vp],
    "tg_gemm_w4_plan": [ctypes.POINTER(W4Gemm), ctypes.c_int],
    "tg_gemm_w4_plan_detail": [ctypes.POINTER(W4Gemm), ctypes.c_int],
    "tg_gemm_w4_workspace_bytes": [ctypes.POINTER(W4Gemm)],
    "tg_gemm_w4_dx": [ctypes.POINTER(W4Gemm), ctypes.c_int, _vp],
    "tg_gemm_w4_dx_workspace_bytes": [ctypes.POINTER(W4Gemm)],
    "tg_gemm_w4_dq": [ctypes.POINTER(W4Gemm), _vp, _vp, _vp, ctypes.c_int, _vp],
    "tg_gemm_w4_dq_workspace_bytes": [ctypes.POINTER(W4Gemm)],
    "tg_gemm_f16": [_vp, _vp, _vp, _i64, _i64, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp],
    "tg_convert_to_Bint8": [_vp, _i64, _i64, ctypes.c_int, _vp, ctypes.c_int, _vp],
    "tg_convert_to_Aint8": [_vp, _i64, _i64, ctypes.c_int, _vp, ctypes.c_int, _vp],
    "tg_gemm_w8": [ctypes.POINTER(W4Gemm), ctypes.c_int, _vp],
    "tg_gemm_w8_workspace_bytes": [ctypes.POINTER(W4Gemm)],
    # include/peer_gather_hip.h (one-shot peer-write gather of row-sharded outputs)
    "tg_peer_alloc": [ctypes.c_int, _i64, ctypes.POINTER(_vp)],
    "tg_peer_free": [ctypes.c_int, _vp],
    "tg_peer_export": [ctypes.c_int, _vp, ctypes.POINTER(PeerHandle)],
    "tg_peer_open": [ctypes.c_int, ctypes.POINTER(PeerHandle), ctypes.POINTER(_vp)],
    "tg_peer_close": [ctypes.c_int, _vp],
    "tg_peer_gather_launch": [ctypes.POINTER(PeerGather), ctypes.c_int, _vp],
    # include/decode_glue_hip.h (non-GEMM kernels of the decode harness)
    "dg_add_rmsnorm": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, ctypes.c_float, ctypes.c_int, ctypes.c_int, _vp],
    "dg_rope_kv": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64,
                   ctypes.c_int, ctypes.c_int, _vp],
    "dg_decode_attn": [_vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64, ctypes.c_float,
                       ctypes.c_int, ctypes.c_int, _vp],
    "dg_rope_attn_split_scratch_bytes": [_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int],
    "dg_swiglu": [_vp, _vp, _i64, _i64, ctypes.c_int, ctypes.c_int, _vp],
    "dg_linear16": [_vp, _vp, _vp, _i64, _i64, _i64, ctypes.c_int, ctypes.c_int, _vp],
    # the sampler: logits, ctr, temperature, top_k, top_p, seed, u_in, token_out, u_out, scratch, scratch_bytes, bs, vocab, ld,
    # per_sequence, ctr_add, dtype, device, stream
    "dg_sample": [_vp] * 10 + [_i64, _i64, _i64, _i64, ctypes.c_int, _i64, ctypes.c_int, ctypes.c_int, _vp],
    "dg_sample_scratch_bytes": [_i64, _i64],
    # per-sequence LoRA adapters: x, norm_weight, A, idx, t, m, k, r, n_adapters, rows_per_id, eps, dtype, device, stream
    "dg_lora_shrink": [_vp] * 5 + [_i64] * 5 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, _vp],
    # t, B, scale, idx, y, m, n, r, ldy, n_adapters, rows_per_id, dtype, device, stream
    "dg_lora_expand": [_vp] * 5 + [_i64] * 6 + [ctypes.c_int, ctypes.c_int, _vp],
}
for _base, _has_mx8 in ATTN_BASES.items():
    for _seq in (False, True):
        for _mx8 in (False, True) if _has_mx8 else (False,):
            _name, _args = attn_signature(_base, _seq, _mx8)
            SYMBOLS[_name] = [t for _, t in _args]
# name -> argtypes of the paged attention entry points (the DG_PAGED_API prototypes of include/decode_glue_hip.h); load() binds them too
PAGED_SYMBOLS = {}
for _base in ATTN_PAGED_BASES:
    _name, _args = attn_signature(_base, paged=True)
    PAGED_SYMBOLS[_name] = [t for _, t in _args]

# name -> argtypes of the one-barrier kernel's mx8 entry points (the DG_KV8_API prototypes of include/decode_glue_hip.h); load() binds them too
KV8_ONLINE_SYMBOLS = {}
for _seq in (False, True):
    _name, _args = kv8_online_signature(_seq)
    KV8_ONLINE_SYMBOLS[_name] = [t for _, t in _args]

# name -> argtypes of the paged mx8 entry points (the DG_PAGED_KV8_API prototypes of include/decode_glue_hip.h); load() binds them too
PAGED_MX8_SYMBOLS = {}
for _base in ATTN_PAGED_MX8_BASES:
    _name, _args = paged_mx8_signature(_base)
    PAGED_MX8_SYMBOLS[_name] = [t for _, t in _args]

_lib = None


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"tinygemm HIP library not built: {LIB_PATH} is missing. "
            "Run `python -m any4_amd.build` (needs hipcc; cross-compiles gfx950 without a GPU). "
            "There is no CPU/PyTorch fallback for the tinygemm ops."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in {**SYMBOLS, **PAGED_SYMBOLS, **KV8_ONLINE_SYMBOLS, **PAGED_MX8_SYMBOLS}.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # a stale build: the header declares a symbol the .so does not export
            raise ImportError(f"{LIB_PATH} does not export {name}; rebuild with `python -m any4_amd.build`") from e
        fn.argtypes = argtypes
        fn.restype = (ctypes.c_char_p if name == "tg_error_string" else
                      ctypes.c_int64 if name in ("dg_rope_attn_split_scratch_bytes", "dg_sample_scratch_bytes", "tg_gemm_w4_workspace_bytes", "tg_gemm_w8_workspace_bytes",
                                                                                          "tg_gemm_w4_dx_workspace_bytes", "tg_gemm_w4_dq_workspace_bytes") else ctypes.c_int)
    if lib.tg_abi_version() != TG_ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {lib.tg_abi_version()} != {TG_ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().tg_error_string(rc).decode()
        raise RuntimeError(f"tinygemm::{what}: {msg} (code {rc})")
