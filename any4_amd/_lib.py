"""ctypes binding of include/tinygemm_hip.h.  No fallbacks: if the HIP library is missing the
import fails loudly (build it with `python -m any4_amd.build`)."""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtinygemm_hip.so")

TG_BF16, TG_F16 = 0, 1
TG_Q_INT4, TG_Q_ANY4_GLOBAL, TG_Q_ANY4_ROWWISE, TG_Q_MX4, TG_Q_INT8 = 0, 1, 2, 3, 4
TG_NUM_FAST, TG_NUM_REFERENCE, TG_NUM_FAST_MFMA, TG_NUM_FAST_DOT2 = 0, 1, 2, 3
TG_ABI_VERSION = 10
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


# The fused attention call of include/decode_glue_hip.h: four kernels, four flag bits, one struct
DG_ATTN_GENERAL, DG_ATTN_ONLINE, DG_ATTN_SPLIT, DG_ATTN_PREFILL = 0, 1, 2, 3
DG_ATTN_SEQ, DG_ATTN_MX8, DG_ATTN_PAGED, DG_ATTN_ONE_BARRIER = 1, 2, 4, 8
_u32, _f32 = ctypes.c_uint32, ctypes.c_float


class Attn(ctypes.Structure):
    """struct dg_attn (include/decode_glue_hip.h)"""

    _fields_ = [
        ("struct_bytes", _u32), ("kernel", _i32),
        ("qkv", _vp), ("cos", _vp), ("sin", _vp), ("pos", _vp), ("k_cache", _vp), ("v_cache", _vp), ("out", _vp),
        ("k_exp", _vp), ("v_exp", _vp), ("len", _vp), ("slot", _vp), ("table", _vp), ("scratch", _vp),
        ("scratch_bytes", _i64), ("bs", _i64), ("T", _i64), ("cache_bs", _i64), ("max_seq", _i64), ("page_size", _i64), ("num_pages", _i64),
        ("flags", _u32), ("hl", _i32), ("kvl", _i32), ("d", _i32), ("nsplit", _i32), ("dtype", _i32), ("scale", _f32), ("reserved", _u32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if "struct_bytes" not in kw:
            self.struct_bytes = ctypes.sizeof(Attn)


# The mixture-of-experts call of include/decode_glue_hip.h: two kernels, two stages, one struct
DG_MOE_GATE_UP, DG_MOE_DOWN = 0, 1
DG_MOE_GEMV, DG_MOE_GROUPED = 0, 1


class Moe(ctypes.Structure):
    """struct dg_moe (include/decode_glue_hip.h)"""

    _fields_ = [
        ("struct_bytes", _u32), ("kernel", _i32),
        ("x", _vp), ("w", _vp), ("qinfo", _vp), ("lut", _vp), ("y", _vp), ("ids", _vp), ("gates", _vp), ("residual", _vp),
        ("group_ws", _vp), ("f32_ws", _vp),
        ("stride_w", _i64), ("stride_qinfo", _i64), ("stride_lut", _i64), ("m", _i64), ("wrows", _i64), ("k", _i64),
        ("group_ws_bytes", _i64), ("f32_ws_bytes", _i64),
        ("stage", _i32), ("E", _i32), ("top_k", _i32), ("group", _i32), ("qtype", _i32), ("dtype", _i32), ("inner_k_tiles", _i32),
        ("reserved", _u32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if "struct_bytes" not in kw:
            self.struct_bytes = ctypes.sizeof(Moe)


# (kernel, flags) -> the name the call had as an entry point of its own up to ABI 8: DG_ATTN_FLAVOURS of the header, which is what
# dg_attn_launch accepts; error messages keep these names.  A copy written by hand (the header is not read at run time): a new flavour
# gets its row here as well as there, and tests/test_host_cpu.py fails until the two agree.
ATTN_FLAVOURS = {
    (DG_ATTN_GENERAL, 0): "dg_rope_attn",
    (DG_ATTN_GENERAL, DG_ATTN_SEQ): "dg_rope_attn_seq",
    (DG_ATTN_ONLINE, 0): "dg_rope_attn_online",
    (DG_ATTN_ONLINE, DG_ATTN_SEQ): "dg_rope_attn_online_seq",
    (DG_ATTN_ONLINE, DG_ATTN_SEQ | DG_ATTN_PAGED): "dg_rope_attn_online_paged",
    (DG_ATTN_SPLIT, 0): "dg_rope_attn_split",
    (DG_ATTN_SPLIT, DG_ATTN_SEQ): "dg_rope_attn_split_seq",
    (DG_ATTN_SPLIT, DG_ATTN_MX8): "dg_rope_attn_split_mx8",
    (DG_ATTN_SPLIT, DG_ATTN_MX8 | DG_ATTN_SEQ): "dg_rope_attn_split_mx8_seq",
    (DG_ATTN_SPLIT, DG_ATTN_MX8 | DG_ATTN_ONE_BARRIER): "dg_rope_attn_online_mx8",
    (DG_ATTN_SPLIT, DG_ATTN_MX8 | DG_ATTN_ONE_BARRIER | DG_ATTN_SEQ): "dg_rope_attn_online_mx8_seq",
    (DG_ATTN_SPLIT, DG_ATTN_SEQ | DG_ATTN_PAGED): "dg_rope_attn_split_paged",
    (DG_ATTN_SPLIT, DG_ATTN_SEQ | DG_ATTN_PAGED | DG_ATTN_MX8 | DG_ATTN_ONE_BARRIER): "dg_rope_attn_online_mx8_paged",
    (DG_ATTN_PREFILL, 0): "dg_prefill_attn",
    (DG_ATTN_PREFILL, DG_ATTN_SEQ): "dg_prefill_attn_seq",
    (DG_ATTN_PREFILL, DG_ATTN_MX8): "dg_prefill_attn_mx8",
    (DG_ATTN_PREFILL, DG_ATTN_MX8 | DG_ATTN_SEQ): "dg_prefill_attn_mx8_seq",
    (DG_ATTN_PREFILL, DG_ATTN_SEQ | DG_ATTN_PAGED): "dg_prefill_attn_paged",
    (DG_ATTN_PREFILL, DG_ATTN_SEQ | DG_ATTN_PAGED | DG_ATTN_MX8): "dg_prefill_attn_mx8_paged",
}


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
    "dg_attn_launch": [ctypes.POINTER(Attn), ctypes.c_int, _vp],
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
    # mixture of experts: x, router_w, ids, gates, m, k, E, top_k, dtype, device, stream
    "dg_moe_route": [_vp] * 4 + [_i64] * 4 + [ctypes.c_int, ctypes.c_int, _vp],
    "dg_moe_launch": [ctypes.POINTER(Moe), ctypes.c_int, _vp],
    "dg_moe_plan": [ctypes.POINTER(Moe), ctypes.c_int, ctypes.POINTER(_i64)],
    # mixture of experts, many rows: ids, group_ws, group_ws_bytes, m, top_k, E, bm, device, stream
    "dg_moe_group": [_vp, _vp] + [_i64] * 5 + [ctypes.c_int, _vp],
    # the quantizer's k-means: x, w, w_row_stride, c0, assign, centers, sse, iters, rows, k, C, S, max_iter, tol, device, stream
    "tg_kmeans_rows": [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                       ctypes.c_int, _vp],
    # rows, k, C, S, max_iter, tol, weighted, out[2]
    "tg_kmeans_rows_plan": [_i64, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.POINTER(_i64)],
}
# Up to ABI 8 three groups of attention entry points were bound from tables of their own.  Nothing is any more, and nothing in this
# tree reads these; the names stay, empty, so that a module written against that binding, which merges the four tables when it is
# imported (`{**SYMBOLS, **PAGED_SYMBOLS, ...}`), still imports and fails where it makes its call, not where it is loaded.
PAGED_SYMBOLS, KV8_ONLINE_SYMBOLS, PAGED_MX8_SYMBOLS = {}, {}, {}

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
    for name, argtypes in SYMBOLS.items():
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
