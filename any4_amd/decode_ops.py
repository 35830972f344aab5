"""ctypes front-end of include/decode_glue_hip.h: the non-GEMM kernels of a decode step (one new token per sequence) and of the
prompt prefill in front of it (`prefill_attn`: a chunk of tokens per sequence).

Every function takes torch tensors on a ROCm device, allocates the output with `torch.empty` (caching
allocator, current stream) and launches on `torch.cuda.current_stream()`; they are legal inside
`torch.cuda.graph` capture.  No CPU fallback: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return _lib.TG_BF16
    if t.dtype == torch.float16:
        return _lib.TG_F16
    raise RuntimeError(f"decode glue kernels need bf16 or fp16 tensors, got {t.dtype}")


def _gpu(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise RuntimeError("decode glue kernels need contiguous tensors on a ROCm device (there is no CPU fallback)")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t):
    if _raw_stream is not None:
        return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


def add_rmsnorm(h: torch.Tensor, delta, weight: torch.Tensor, eps: float, want_norm: bool = True):
    """(h + delta, rmsnorm(h + delta) * weight); delta may be None.  h is updated IN PLACE when delta is given
    (the residual stream is a running sum).  h [rows, dim]."""
    _gpu(h, delta, weight)
    rows, dim = h.shape
    y = torch.empty_like(h) if want_norm else None
    _lib.check(_lib.load().dg_add_rmsnorm(h.data_ptr(), None if delta is None else delta.data_ptr(), weight.data_ptr(),
                                          h.data_ptr(), None if y is None else y.data_ptr(), rows, dim, float(eps),
                                          _dt(h), h.device.index, _stream(h)), "dg_add_rmsnorm")
    return h, y


def _rope_front(qkv, cos, sin, pos, k_cache, v_cache, hl, d, *more, out=None):
    """What the rope / attention wrappers share: the device check (`more`: further tensors of the call), the dtype check of the
    tables and `pos`, and the output [rows of qkv, hl * d] (allocated unless given).  Returns (out, rows of qkv, max_seq)."""
    _gpu(qkv, cos, sin, pos, k_cache, v_cache, *more, out)
    if cos.dtype != torch.float32 or pos.dtype != torch.int64:
        raise RuntimeError("rope tables must be float32 and pos int64")
    if out is None:
        out = torch.empty((qkv.shape[0], hl * d), dtype=qkv.dtype, device=qkv.device)
    return out, qkv.shape[0], k_cache.shape[2]


def rope_kv(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor,
            v_cache: torch.Tensor, hl: int, kvl: int, d: int) -> torch.Tensor:
    """qkv [bs, (hl + 2 kvl) d] -> rotated q [bs, hl, d]; rotated k and v are written into the caches at `pos`."""
    q, bs, max_seq = _rope_front(qkv, cos, sin, pos, k_cache, v_cache, hl, d)
    _lib.check(_lib.load().dg_rope_kv(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), q.data_ptr(),
                                      k_cache.data_ptr(), v_cache.data_ptr(), bs, hl, kvl, d, max_seq, _dt(qkv),
                                      qkv.device.index, _stream(qkv)), "dg_rope_kv")
    return q.view(bs, hl, d)


def decode_attn(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor, scale: float) -> torch.Tensor:
    """q [bs, hl, d], caches [bs, kvl, max_seq, d] -> context [bs, hl * d] over positions 0..pos."""
    _gpu(q, k_cache, v_cache, pos)
    bs, hl, d = q.shape
    kvl, max_seq = k_cache.shape[1], k_cache.shape[2]
    out = torch.empty((bs, hl * d), dtype=q.dtype, device=q.device)
    _lib.check(_lib.load().dg_decode_attn(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), pos.data_ptr(),
                                          out.data_ptr(), bs, hl, kvl, d, max_seq, float(scale), _dt(q), q.device.index,
                                          _stream(q)), "dg_decode_attn")
    return out


def _per_sequence(pos, n, what):
    """`pos` (already checked: int64, contiguous, on the device) holds one position per sequence."""
    if pos.numel() != n:
        raise RuntimeError(f"{what}: per_sequence needs {n} int64 positions (one per sequence), got {pos.numel()}")


F8 = torch.float8_e4m3fn


def _mx8_exps(what, k_cache, v_cache, k_exp, v_exp, d):
    """The exponent tensors of an mx8 cache pair (any4_amd/kvcache.py), checked: () for 16-bit caches, which must bring none."""
    mx8 = k_cache.dtype == F8 or v_cache.dtype == F8
    if not mx8:
        if k_exp is not None or v_exp is not None:
            raise RuntimeError(f"{what}: k_exp / v_exp belong to float8_e4m3fn (mx8) caches, got {k_cache.dtype}")
        return ()
    if k_cache.dtype != F8 or v_cache.dtype != F8 or k_exp is None or v_exp is None:
        raise RuntimeError(f"{what}: an mx8 cache is k_cache, v_cache (float8_e4m3fn) and k_exp, v_exp (uint8)")
    if d % 32:
        raise RuntimeError(f"{what}: an mx8 cache needs head_dim % 32 == 0, got {d}")
    for c, e in ((k_cache, k_exp), (v_cache, v_exp)):
        if e.dtype != torch.uint8 or tuple(e.shape) != tuple(c.shape[:-1]) + (d // 32,) or c.shape[-1] != d:
            raise RuntimeError(f"{what}: exponents must be uint8 {tuple(c.shape[:-1]) + (d // 32,)} for codes {tuple(c.shape)}, got {e.dtype} {tuple(e.shape)}")
    return (k_exp, v_exp)


def _paged(what, table, k_pool, v_pool, kvl, d, exps=()):
    """The paging fields of a DG_ATTN_PAGED launch, checked: `table` int32 [cache_bs, max_seq / page_size] on the pools' device, the pools
    [num_pages, kvl, page_size, d] in a 16-bit type -- or, with exps = (k_exp, v_exp) (checked already: _mx8_pools), float8_e4m3fn codes of
    a paged mx8 launch.  Returns them by field name (the pools are the call's k_cache / v_cache), with max_seq (the exponents go in with every mx8 call: _attn_launch)."""
    if table.dtype != torch.int32 or table.dim() != 2 or k_pool.dim() != 4 or k_pool.shape != v_pool.shape or k_pool.dtype != v_pool.dtype or \
            tuple(k_pool.shape[1::2]) != (kvl, d):
        raise RuntimeError(f"{what}: table must be int32 [cache_bs, max_seq / page_size] and the pools [num_pages, {kvl}, page_size, {d}], got "
                           f"{table.dtype} {tuple(table.shape)}, {tuple(k_pool.shape)}, {tuple(v_pool.shape)}")
    if not exps and k_pool.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError(f"{what}: a paged cache holds 16-bit rows, got {k_pool.dtype}")
    num_pages, _, page_size, _ = k_pool.shape
    return dict(table=table, k_cache=k_pool, v_cache=v_pool, page_size=page_size, num_pages=num_pages, max_seq=table.shape[1] * page_size)


def _mx8_pools(what, k_pool, v_pool, k_exp, v_exp, d):
    """(k_exp, v_exp) of mx8 page pools, checked on the host (in front of the device check): code pools float8_e4m3fn [num_pages, kvl,
    page_size, d], exponent pools uint8 [num_pages, kvl, page_size, d / 32].  16-bit pools do not belong to the entry points that ask."""
    exps = _mx8_exps(what, k_pool, v_pool, k_exp, v_exp, d)
    if not exps:
        raise RuntimeError(f"{what}: the pools must be float8_e4m3fn (mx8), got {k_pool.dtype}; 16-bit pools: the _paged entry points")
    return exps


def _attn_flags(per_sequence, exps, table, one_barrier=False):
    """The flag word of a call: what its caches are and how `pos` is read, said explicitly (the library infers nothing)"""
    return ((_lib.DG_ATTN_SEQ if per_sequence else 0) | (_lib.DG_ATTN_MX8 if exps else 0) | (_lib.DG_ATTN_PAGED if table is not None else 0)
            | (_lib.DG_ATTN_ONE_BARRIER if one_barrier else 0))


def _attn_name(kernel, flags):
    """The call's name in messages: the one it has in the header's table of accepted calls"""
    return _lib.ATTN_FLAVOURS.get((kernel, flags), "dg_attn_launch")


def _attn_launch(kernel, flags, exps, qkv, **values):
    """One dg_attn_launch: `values` are fields of _lib.Attn by name, tensors (or None) for pointers; exps = (k_exp, v_exp) of an mx8 cache,
    or ().  qkv also supplies dtype, device and stream."""
    values.update(zip(("k_exp", "v_exp"), exps), qkv=qkv)
    call = _lib.Attn(kernel=kernel, flags=flags, dtype=_dt(qkv),
                     **{name: v.data_ptr() if isinstance(v, torch.Tensor) else v for name, v in values.items()})
    rc = _lib.load().dg_attn_launch(ctypes.byref(call), qkv.device.index, _stream(qkv))
    if rc != 0:
        _lib.check(rc, _attn_name(kernel, flags))


def _rope_attn(kernel, qkv, cos, sin, pos, k_cache, v_cache, hl, kvl, d, scale, per_sequence=False, out=None, split=None, exps=(), table=None,
               one_barrier=False):
    """rope_attn / rope_attn_online / rope_attn_split: three kernels (_lib.DG_ATTN_GENERAL / ONLINE / SPLIT) behind one argument list
    (per_sequence: DG_ATTN_SEQ, `pos` [bs]).  split = (scratch, nsplit) of rope_attn_split; exps = (k_exp, v_exp) of an mx8 cache:
    DG_ATTN_MX8; table: the caches are page pools behind this block table: DG_ATTN_PAGED (per sequence); one_barrier: DG_ATTN_ONE_BARRIER,
    rope_attn_online_mx8 and rope_attn_online_mx8_paged (split and exps given, kernel DG_ATTN_SPLIT)."""
    scratch, nsplit = split if split is not None else (None, None)
    out, bs, max_seq = _rope_front(qkv, cos, sin, pos, k_cache, v_cache, hl, d, scratch, table, *exps, out=out)
    flags = _attn_flags(per_sequence, exps, table, one_barrier)
    # the prefix of the messages below is the flavour's name without `_seq`, as it always was (a paged flavour has no such suffix: it
    # is per sequence by definition).  Every public function above gives a pair of the table; _attn_name's fallback is for none of them.
    what = _attn_name(kernel, flags & ~_lib.DG_ATTN_SEQ if table is None else flags)
    if out.shape != (bs, hl * d) or out.dtype != qkv.dtype:
        raise RuntimeError(f"{what}: out must be [{bs}, {hl * d}] {qkv.dtype}")
    if per_sequence:
        _per_sequence(pos, bs, what)
    more = {} if split is None else dict(scratch=scratch, scratch_bytes=scratch.numel() * 4, nsplit=nsplit)
    if table is not None:
        if table.shape[0] != bs:
            raise RuntimeError(f"{what}: the table needs a row per sequence ({bs}), got {tuple(table.shape)}")
        more.update(_paged(what, table, k_cache, v_cache, kvl, d, exps))
    else:
        more.update(k_cache=k_cache, v_cache=v_cache, max_seq=max_seq)
    _attn_launch(kernel, flags, exps, qkv, cos=cos, sin=sin, pos=pos, out=out, bs=bs, hl=hl, kvl=kvl, d=d, scale=float(scale), **more)
    return out


def rope_attn(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor,
              v_cache: torch.Tensor, hl: int, kvl: int, d: int, scale: float, per_sequence: bool = False,
              out: torch.Tensor = None) -> torch.Tensor:
    """rope_kv + decode_attn in one launch: qkv [bs, (hl + 2 kvl) d] -> context [bs, hl * d]; caches updated at `pos`.
    per_sequence: `pos` is int64 [bs], sequence b sits at pos[b]; a sequence whose position is outside [0, max_seq) writes nothing
    and leaves its row of `out` (allocated here, uninitialised, unless given) as it was."""
    return _rope_attn(_lib.DG_ATTN_GENERAL, qkv, cos, sin, pos, k_cache, v_cache, hl, kvl, d, scale, per_sequence, out)


def rope_attn_online(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, hl: int, kvl: int, d: int, scale: float, per_sequence: bool = False,
                     out: torch.Tensor = None) -> torch.Tensor:
    """rope_attn built for latency (head_dim 64 / 128): one barrier, every load issued up front, softmax statistics combined
    flash-decoding style -- the same caches bit for bit, the output within 16-bit rounding of rope_attn's.  per_sequence: as rope_attn."""
    return _rope_attn(_lib.DG_ATTN_ONLINE, qkv, cos, sin, pos, k_cache, v_cache, hl, kvl, d, scale, per_sequence, out)


def rope_attn_split_scratch(bs: int, hl: int, d: int, nsplit: int, device) -> torch.Tensor:
    """Zeroed scratch buffer for rope_attn_split (counters + per-chunk partials); reusable by stream-ordered launches."""
    n = _lib.load().dg_rope_attn_split_scratch_bytes(bs, hl, d, nsplit)
    return torch.zeros((n + 3) // 4, dtype=torch.int32, device=device)


def rope_attn_split(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor,
                    v_cache: torch.Tensor, hl: int, kvl: int, d: int, scale: float, scratch: torch.Tensor, nsplit: int,
                    per_sequence: bool = False, out: torch.Tensor = None, k_exp: torch.Tensor = None, v_exp: torch.Tensor = None) -> torch.Tensor:
    """rope_attn with the sequence split over `nsplit` blocks per head (fills the GPU at batch 1 / long contexts).
    per_sequence, out: as rope_attn.  float8_e4m3fn caches with `k_exp`, `v_exp` (uint8 [bs, kvl, max_seq, d / 32]) are an mx8 cache
    (any4_amd/kvcache.py): the mx8 entry points, which also take nsplit = 1."""
    exps = _mx8_exps("rope_attn_split", k_cache, v_cache, k_exp, v_exp, d)
    return _rope_attn(_lib.DG_ATTN_SPLIT, qkv, cos, sin, pos, k_cache, v_cache, hl, kvl, d, scale, per_sequence, out, (scratch, nsplit), exps)


def rope_attn_online_mx8(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                         k_exp: torch.Tensor, v_exp: torch.Tensor, hl: int, kvl: int, d: int, scale: float, scratch: torch.Tensor, nsplit: int,
                         per_sequence: bool = False, out: torch.Tensor = None) -> torch.Tensor:
    """rope_attn_online's one-barrier kernel on an mx8 cache (head_dim 64 / 128), `nsplit` blocks per head (1 ... 64; `scratch` as for
    rope_attn_split): a row's 8-byte pieces lie across lanes as the 16-bit rows do and are converted on use, the new token is encoded
    byte for byte as mx8_encode does and enters the scores and the value sum as its decoded row.  The arithmetic behind the conversion
    is rope_attn_online's (nsplit = 1) / rope_attn_split's (more) on a 16-bit cache holding the decoded values, bit for bit."""
    exps = _mx8_exps("rope_attn_online_mx8", k_cache, v_cache, k_exp, v_exp, d)
    if not exps:
        raise RuntimeError(f"rope_attn_online_mx8: the caches must be float8_e4m3fn (mx8), got {k_cache.dtype}; 16-bit caches: rope_attn_online / rope_attn_split")
    return _rope_attn(_lib.DG_ATTN_SPLIT, qkv, cos, sin, pos, k_cache, v_cache, hl, kvl, d, scale, per_sequence, out, (scratch, nsplit), exps,
                      one_barrier=True)


def rope_attn_online_paged(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, table: torch.Tensor,
                           k_pool: torch.Tensor, v_pool: torch.Tensor, hl: int, kvl: int, d: int, scale: float, out: torch.Tensor = None) -> torch.Tensor:
    """rope_attn_online(per_sequence=True) on a paged cache: pools [num_pages, kvl, page_size, d] behind `table` int32 [bs, max_seq /
    page_size] on the device -- position p of sequence b is row p % page_size of page table[b, p // page_size] (-1: unmapped).  An entry
    outside the pool is read as page 0 and never written through."""
    return _rope_attn(_lib.DG_ATTN_ONLINE, qkv, cos, sin, pos, k_pool, v_pool, hl, kvl, d, scale, True, out, table=table)


def rope_attn_split_paged(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, table: torch.Tensor, k_pool: torch.Tensor,
                          v_pool: torch.Tensor, hl: int, kvl: int, d: int, scale: float, scratch: torch.Tensor, nsplit: int,
                          out: torch.Tensor = None) -> torch.Tensor:
    """rope_attn_split(per_sequence=True) on a paged cache (rope_attn_online_paged): the one-barrier kernel with nsplit blocks per head."""
    return _rope_attn(_lib.DG_ATTN_SPLIT, qkv, cos, sin, pos, k_pool, v_pool, hl, kvl, d, scale, True, out, (scratch, nsplit), table=table)


def prefill_attn_paged(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, table: torch.Tensor, k_pool: torch.Tensor,
                       v_pool: torch.Tensor, hl: int, kvl: int, d: int, scale: float, T: int, out: torch.Tensor = None,
                       lengths: torch.Tensor = None, slots: torch.Tensor = None) -> torch.Tensor:
    """prefill_attn(per_sequence=True) on a paged cache (rope_attn_online_paged): `slots` names the table ROW of each sequence (default:
    row i, and n must be the table's rows)."""
    return prefill_attn(qkv, cos, sin, pos, k_pool, v_pool, hl, kvl, d, scale, T, out, lengths, slots, True, table=table)


def rope_attn_online_mx8_paged(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, table: torch.Tensor,
                               k_pool: torch.Tensor, v_pool: torch.Tensor, k_exp: torch.Tensor, v_exp: torch.Tensor, hl: int, kvl: int, d: int,
                               scale: float, scratch: torch.Tensor, nsplit: int, out: torch.Tensor = None) -> torch.Tensor:
    """rope_attn_online_mx8(per_sequence=True) on paged mx8 pools: codes float8_e4m3fn [num_pages, kvl, page_size, d] and exponents uint8
    [num_pages, kvl, page_size, d / 32] behind the one `table` (rope_attn_online_paged).  Always the one-barrier kernel, `nsplit` blocks per
    head (1 ... 64; `scratch` as for rope_attn_split); bytes written and output are rope_attn_online_mx8's on caches holding the same rows."""
    exps = _mx8_pools("rope_attn_online_mx8_paged", k_pool, v_pool, k_exp, v_exp, d)
    return _rope_attn(_lib.DG_ATTN_SPLIT, qkv, cos, sin, pos, k_pool, v_pool, hl, kvl, d, scale, True, out, (scratch, nsplit), exps, table,
                      one_barrier=True)


def prefill_attn_mx8_paged(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, table: torch.Tensor, k_pool: torch.Tensor,
                           v_pool: torch.Tensor, k_exp: torch.Tensor, v_exp: torch.Tensor, hl: int, kvl: int, d: int, scale: float, T: int,
                           out: torch.Tensor = None, lengths: torch.Tensor = None, slots: torch.Tensor = None) -> torch.Tensor:
    """prefill_attn(per_sequence=True) on paged mx8 pools (rope_attn_online_mx8_paged): `slots` names the table ROW of each sequence
    (default: row i, and n must be the table's rows)."""
    _mx8_pools("prefill_attn_mx8_paged", k_pool, v_pool, k_exp, v_exp, d)
    return prefill_attn(qkv, cos, sin, pos, k_pool, v_pool, hl, kvl, d, scale, T, out, lengths, slots, True, k_exp, v_exp, table)


def prefill_attn(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor,
                 v_cache: torch.Tensor, hl: int, kvl: int, d: int, scale: float, T: int, out: torch.Tensor = None,
                 lengths: torch.Tensor = None, slots: torch.Tensor = None, per_sequence: bool = False, k_exp: torch.Tensor = None,
                 v_exp: torch.Tensor = None, table: torch.Tensor = None) -> torch.Tensor:
    """A chunk of T tokens per sequence: qkv [bs * T, (hl + 2 kvl) d] (row b * T + t) -> context [bs * T, hl * d]; the T roped k rows and
    the v rows are appended to the caches at positions pos ... pos + T - 1 (`pos` [1] int64 on the device = position of token 0), and
    token t attends causally over cache rows 0 ... pos + t.  A token whose position is outside the cache writes nothing and leaves its
    row of `out` (allocated here unless given) as it was.
    per_sequence (also implied by `lengths` / `slots`): qkv is [n * T, ...], rows padded to the common T, and `pos` int64 [n] holds the
    position of token 0 of each sequence.  `lengths` int64 [n] on the device: only tokens t < min(lengths[i], T) exist (default: all T);
    `slots` int64 [n] on the device: sequence i lives in cache slot slots[i] (default: slot i, and n must be the caches' batch; with
    slots n may be smaller).  A sequence of length <= 0 or with a slot outside the caches does nothing; slots must be distinct.
    float8_e4m3fn caches with `k_exp`, `v_exp`: an mx8 cache, as in rope_attn_split.  table: prefill_attn_paged (with mx8 pools:
    prefill_attn_mx8_paged)."""
    exps = _mx8_exps("prefill_attn", k_cache, v_cache, k_exp, v_exp, d)
    out, rows, max_seq = _rope_front(qkv, cos, sin, pos, k_cache, v_cache, hl, d, lengths, slots, table, *exps, out=out)
    T = int(T)
    per_sequence = per_sequence or lengths is not None or slots is not None
    cache_bs = k_cache.shape[0] if table is None else table.shape[0]
    if T < 1 or qkv.dim() != 2 or rows % T or (rows // T != cache_bs and slots is None):
        raise RuntimeError(f"prefill_attn: qkv must be [bs * T, ...] with T = {T} and bs = {cache_bs} (the caches'), got {tuple(qkv.shape)}")
    if out.shape != (rows, hl * d) or out.dtype != qkv.dtype:
        raise RuntimeError(f"prefill_attn: out must be [{rows}, {hl * d}] {qkv.dtype}")
    more = {}
    if per_sequence:
        n = rows // T
        _per_sequence(pos, n, "prefill_attn")
        for name, t in (("lengths", lengths), ("slots", slots)):
            if t is not None and (t.dtype != torch.int64 or t.numel() != n):
                raise RuntimeError(f"prefill_attn: {name} must be int64 with {n} elements (one per sequence)")
        more = dict(len=lengths, slot=slots, cache_bs=cache_bs)
    if table is not None:
        more.update(_paged("prefill_attn_mx8_paged" if exps else "prefill_attn_paged", table, k_cache, v_cache, kvl, d, exps))
    else:
        more.update(k_cache=k_cache, v_cache=v_cache, max_seq=max_seq)
    _attn_launch(_lib.DG_ATTN_PREFILL, _attn_flags(per_sequence, exps, table), exps, qkv, cos=cos, sin=sin, pos=pos, out=out, bs=rows // T, T=T,
                 hl=hl, kvl=kvl, d=d, scale=float(scale), **more)
    return out


def sample(logits: torch.Tensor, ctr: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
           seed: torch.Tensor = None, ctr_add: int = 1, u: torch.Tensor = None, token_out: torch.Tensor = None, u_out: torch.Tensor = None,
           scratch: torch.Tensor = None, vocab: int = None) -> torch.Tensor:
    """Temperature / top-k / top-p sampling of logits [bs, ld] (16-bit; the first `vocab` columns, default all; the last dimension must be
    contiguous, rows may be `ld` apart) in one launch -- any4_amd/sampling.py: sample_ref is the definition.  Returns token_out int64 [bs]
    (allocated unless given).  temperature, top_p float32 [bs], top_k int32 [bs], seed int64 [bs], all on the device.  ctr int64 on the
    device, [bs] or [1] (one value for every sequence): sequence b draws sampling.uniform(seed[b], ctr + ctr_add), and a NEGATIVE value
    read from ctr makes it inactive (token -1).  u float32 [bs]: replaces that draw (seed may then be None).  u_out float32 [bs]: receives
    the u used."""
    if logits.dim() != 2 or logits.stride(1) != 1 or not logits.is_cuda:
        raise RuntimeError("sample: logits must be [bs, vocab] on a ROCm device with a contiguous last dimension (there is no CPU fallback)")
    bs, width = logits.shape
    ld = logits.stride(0) if bs > 1 else max(logits.stride(0), width)
    vocab = width if vocab is None else int(vocab)
    if token_out is None:
        token_out = torch.empty(bs, dtype=torch.int64, device=logits.device)
    _gpu(ctr, temperature, top_k, top_p, seed, u, token_out, u_out, scratch)
    for name, t, dt in (("temperature", temperature, torch.float32), ("top_k", top_k, torch.int32), ("top_p", top_p, torch.float32),
                        ("seed", seed, torch.int64), ("u", u, torch.float32), ("token_out", token_out, torch.int64), ("u_out", u_out, torch.float32)):
        if t is not None and (t.dtype != dt or t.numel() != bs):
            raise RuntimeError(f"sample: {name} must be {dt} with {bs} elements (one per sequence), got {t.dtype} {tuple(t.shape)}")
    if ctr.dtype != torch.int64 or ctr.numel() not in (1, bs):
        raise RuntimeError(f"sample: ctr must be int64 with 1 or {bs} elements, got {ctr.dtype} {tuple(ctr.shape)}")
    if seed is None and u is None:
        raise RuntimeError("sample: a seed per sequence is needed unless u is given")
    if not 1 <= vocab <= width or ld < vocab:
        raise RuntimeError(f"sample: vocab {vocab} outside the logits' {width} columns (row stride {ld})")
    ptr = lambda t: None if t is None else t.data_ptr()
    # (per_sequence: ctr has an element per sequence; with bs == 1 both readings are the same element)
    _lib.check(_lib.load().dg_sample(logits.data_ptr(), ctr.data_ptr(), temperature.data_ptr(), top_k.data_ptr(), top_p.data_ptr(), ptr(seed),
                                     ptr(u), token_out.data_ptr(), ptr(u_out), ptr(scratch), 0 if scratch is None else scratch.numel() * 4,
                                     bs, vocab, ld, int(ctr.numel() == bs), int(ctr_add), _dt(logits), logits.device.index, _stream(logits)),
               "dg_sample")
    return token_out


def _lora_ids(what, idx, rows, rows_per_id, n_adapters_of):
    rows_per_id = int(rows_per_id)
    if rows_per_id < 1:
        raise RuntimeError(f"{what}: rows_per_id must be >= 1, got {rows_per_id}")
    if idx.dtype != torch.int32 or idx.dim() != 1 or idx.numel() < -(-rows // rows_per_id):
        raise RuntimeError(f"{what}: idx must be int32 with at least ceil({rows} / {rows_per_id}) elements (one per sequence), got {idx.dtype} "
                           f"{tuple(idx.shape)}")
    if n_adapters_of.dim() != 3:
        raise RuntimeError(f"{what}: adapter weights must be [n_adapters, rows, columns], got {tuple(n_adapters_of.shape)}")
    return rows_per_id


def lora_shrink(x: torch.Tensor, A: torch.Tensor, idx: torch.Tensor, rows_per_id: int = 1, norm_weight: torch.Tensor = None,
                eps: float = 0.0, out: torch.Tensor = None) -> torch.Tensor:
    """t [m, r] float32 = A[idx[i // rows_per_id]] @ x[i] per activation row i (any4_amd/lora.py: lora_ref is the definition).  x [m, k]
    16-bit, A [n_adapters, r, k] of x's dtype, idx int32 on the device (an id outside [0, n_adapters): no adapter, t = 0).  norm_weight
    [k]: the RMSNorm of the activations in the "sum" convention, t = rs * A @ RNE16(x * norm_weight).  out: the float32 buffer to fill."""
    _gpu(x, A, idx, norm_weight, out)
    if x.dim() != 2:
        raise RuntimeError(f"lora_shrink: x must be [m, k], got {tuple(x.shape)}")
    m, k = x.shape
    rows_per_id = _lora_ids("lora_shrink", idx, m, rows_per_id, A)
    na, r = A.shape[0], A.shape[1]
    if A.dtype != x.dtype or A.shape[2] != k:
        raise RuntimeError(f"lora_shrink: A must be [n_adapters, r, k = {k}] {x.dtype}, got {tuple(A.shape)} {A.dtype}")
    if norm_weight is not None and (norm_weight.dtype != x.dtype or norm_weight.numel() != k):
        raise RuntimeError(f"lora_shrink: norm_weight must be [k = {k}] {x.dtype}, got {tuple(norm_weight.shape)} {norm_weight.dtype}")
    if out is None:
        out = torch.empty((m, r), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (m, r):
        raise RuntimeError(f"lora_shrink: out must be float32 [{m}, {r}], got {out.dtype} {tuple(out.shape)}")
    _lib.check(_lib.load().dg_lora_shrink(x.data_ptr(), None if norm_weight is None else norm_weight.data_ptr(), A.data_ptr(), idx.data_ptr(),
                                          out.data_ptr(), m, k, r, na, rows_per_id, float(eps), _dt(x), x.device.index, _stream(x)),
               "dg_lora_shrink")
    return out


def lora_expand(t: torch.Tensor, B: torch.Tensor, scale: torch.Tensor, idx: torch.Tensor, y: torch.Tensor, rows_per_id: int = 1) -> torch.Tensor:
    """y [m, n] += scale[a] * t[i] @ B[a].T IN PLACE, a = idx[i // rows_per_id]; rows without an adapter are not rewritten.  t [m, r] float32
    (lora_shrink's), B [n_adapters, n, r] of y's dtype, scale float32 [n_adapters]; y 16-bit with a contiguous last dimension (its rows may
    be further apart: a view into a wider tensor)."""
    _gpu(t, B, scale, idx)
    if y.dim() != 2 or y.stride(1) != 1 or not y.is_cuda:
        raise RuntimeError("lora_expand: y must be [m, n] on a ROCm device with a contiguous last dimension (there is no CPU fallback)")
    m, n = y.shape
    rows_per_id = _lora_ids("lora_expand", idx, m, rows_per_id, B)
    na, r = B.shape[0], B.shape[2]
    ldy = y.stride(0) if m > 1 else max(y.stride(0), n)
    if B.dtype != y.dtype or B.shape[1] != n:
        raise RuntimeError(f"lora_expand: B must be [n_adapters, n = {n}, r] {y.dtype}, got {tuple(B.shape)} {B.dtype}")
    if t.dtype != torch.float32 or tuple(t.shape) != (m, r):
        raise RuntimeError(f"lora_expand: t must be float32 [{m}, {r}], got {t.dtype} {tuple(t.shape)}")
    if scale.dtype != torch.float32 or scale.numel() != na:
        raise RuntimeError(f"lora_expand: scale must be float32 [{na}], got {scale.dtype} {tuple(scale.shape)}")
    _lib.check(_lib.load().dg_lora_expand(t.data_ptr(), B.data_ptr(), scale.data_ptr(), idx.data_ptr(), y.data_ptr(), m, n, r, ldy, na,
                                          rows_per_id, _dt(y), y.device.index, _stream(y)), "dg_lora_expand")
    return y


def moe_route(x: torch.Tensor, router_w: torch.Tensor, top_k: int, ids: torch.Tensor = None, gates: torch.Tensor = None):
    """(ids int32 [m, top_k], gates float32 [m, top_k]) of the top-k router (any4_amd/moe.py: moe_ref is the definition): x [m, k] 16-bit
    (normed), router_w [E, k] of x's dtype; f32 logits, softmax over all E, the top_k by (p descending, index ascending), gates
    renormalised over the selected.  ids / gates: the buffers to fill."""
    _gpu(x, router_w, ids, gates)
    if x.dim() != 2 or router_w.dim() != 2 or router_w.shape[1] != x.shape[1] or router_w.dtype != x.dtype:
        raise RuntimeError(f"moe_route: x [m, k] and router_w [E, k] of one 16-bit dtype needed, got {tuple(x.shape)} {x.dtype} and "
                           f"{tuple(router_w.shape)} {router_w.dtype}")
    m, k = x.shape
    E, top_k = router_w.shape[0], int(top_k)
    if ids is None:
        ids = torch.empty((m, top_k), dtype=torch.int32, device=x.device)
    if gates is None:
        gates = torch.empty((m, top_k), dtype=torch.float32, device=x.device)
    if ids.dtype != torch.int32 or gates.dtype != torch.float32 or tuple(ids.shape) != (m, top_k) or tuple(gates.shape) != (m, top_k):
        raise RuntimeError(f"moe_route: ids int32 and gates float32 [{m}, {top_k}] needed")
    _lib.check(_lib.load().dg_moe_route(x.data_ptr(), router_w.data_ptr(), ids.data_ptr(), gates.data_ptr(), m, k, E, top_k, _dt(x),
                                        x.device.index, _stream(x)), "dg_moe_route")
    return ids, gates


def _moe_struct(kernel: int, stage: int, stack, m: int, top_k: int, x=None, y=None, ids=None, gates=None, residual=None, group_ws=None,
                f32_ws=None, plan: bool = False) -> "_lib.Moe":
    """struct dg_moe for one stage on an `any4_amd.moe.ExpertStack` (its tensors are contiguous: a stride is one expert's bytes).  plan:
    the planner's call -- `stack` need only name the sizes, the pointers are non-NULL, aligned dummies (the planner dereferences nothing)."""
    if plan:
        operands = dict(x=64, w=64, qinfo=64, lut=64, y=64, ids=64, gates=64, stride_w=16, stride_qinfo=16, stride_lut=16)
    else:
        ptr = lambda t: None if t is None else t.data_ptr()
        per = lambda t: 0 if t is None else t.numel() // t.shape[0] * t.element_size()
        nbytes = lambda t: 0 if t is None else t.numel() * t.element_size()
        operands = dict(x=ptr(x), w=ptr(stack.words), qinfo=ptr(stack.qinfo), lut=ptr(stack.lut), y=ptr(y), ids=ptr(ids), gates=ptr(gates),
                        residual=ptr(residual), group_ws=ptr(group_ws), f32_ws=ptr(f32_ws), stride_w=per(stack.words),
                        stride_qinfo=per(stack.qinfo), stride_lut=per(stack.lut), group_ws_bytes=nbytes(group_ws), f32_ws_bytes=nbytes(f32_ws))
    return _lib.Moe(kernel=kernel, stage=stage, m=m, wrows=stack.n, k=stack.k, E=stack.E, top_k=top_k, group=stack.group, qtype=stack.qtype,
                    dtype=_dt(stack), inner_k_tiles=4, **operands)


def _moe_stage(what, kernel, stage, x, stack, ids, gates=None, residual=None, out=None, group_ws=None, f32_ws=None):
    """One stage of either kernel: the tensor checks, the call, the launch.  what: the public wrapper's name, for its messages."""
    down, grouped = stage == _lib.DG_MOE_DOWN, kernel == _lib.DG_MOE_GROUPED
    m, top_k = ids.shape
    rows, shape = (m * top_k, (m, stack.n)) if down else (m, (m * top_k, stack.n // 2))
    _gpu(x, stack.words, stack.qinfo, stack.lut, ids)
    if ids.dtype != torch.int32 or ids.dim() != 2:
        raise RuntimeError(f"{what}: ids must be int32 [m, top_k], got {ids.dtype} {tuple(ids.shape)}")
    if x.dim() != 2 or tuple(x.shape) != (rows, stack.k) or x.dtype != stack.dtype:
        raise RuntimeError(f"{what}: x must be [{rows}, {stack.k}] {stack.dtype}, got {tuple(x.shape)} {x.dtype}")
    if grouped:
        _gpu(group_ws)
        if group_ws is None or group_ws.dtype != torch.int32:
            raise RuntimeError(f"{what}: group_ws must be the int32 workspace moe_group filled")
    if down:
        _gpu(gates, residual, out, f32_ws)
        if gates.dtype != torch.float32 or tuple(gates.shape) != (m, top_k):
            raise RuntimeError(f"{what}: gates must be float32 [{m}, {top_k}]")
        if residual is not None and (residual.dtype != x.dtype or tuple(residual.shape) != shape):
            raise RuntimeError(f"{what}: residual must be [{m}, {stack.n}] {x.dtype}")
    if out is None:
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
    elif out.dtype != x.dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise RuntimeError(f"{what}: out must be contiguous [{shape[0]}, {shape[1]}] {x.dtype}")
    if grouped and down:
        if f32_ws is None:
            f32_ws = torch.empty((rows, stack.n), dtype=torch.float32, device=x.device)
        elif f32_ws.dtype != torch.float32 or f32_ws.numel() < rows * stack.n:
            raise RuntimeError(f"{what}: f32_ws must hold {rows} x {stack.n} float32")
    call = _moe_struct(kernel, stage, stack, m, top_k, x, out, ids, gates, residual, group_ws, f32_ws)
    _lib.check(_lib.load().dg_moe_launch(ctypes.byref(call), x.device.index, _stream(x)), "dg_moe_launch")
    return out


def _moe_plan(kernel, stage, stack, m, top_k, device, n):
    out = (ctypes.c_int64 * 8)()
    _lib.check(_lib.load().dg_moe_plan(ctypes.byref(_moe_struct(kernel, stage, stack, m, top_k, plan=True)), device, out), "dg_moe_plan")
    return tuple(out)[:n]


def moe_gate_up(x: torch.Tensor, stack, ids: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """act [m * top_k, il]: row i * top_k + s = SwiGLU of x[i] through the gate / up weights of expert ids[i, s] (DG_MOE_GEMV,
    DG_MOE_GATE_UP; `stack` an ExpertStack [2 il, k] with rows in blocks of 8 gate + 8 up).  A pair whose id is outside [0, E) gets zeros."""
    return _moe_stage("moe_gate_up", _lib.DG_MOE_GEMV, _lib.DG_MOE_GATE_UP, x, stack, ids, out=out)


def moe_down(act: torch.Tensor, stack, ids: torch.Tensor, gates: torch.Tensor, residual: torch.Tensor = None, out: torch.Tensor = None) -> torch.Tensor:
    """y [m, n] = RNE16(sum_s gates[i, s] * (act[i * top_k + s] through the down weights of expert ids[i, s]) (+ residual[i]))
    (DG_MOE_GEMV, DG_MOE_DOWN).  out may be `residual` itself (the residual stream, updated in place: an element is read and written by
    one thread)."""
    return _moe_stage("moe_down", _lib.DG_MOE_GEMV, _lib.DG_MOE_DOWN, act, stack, ids, gates, residual, out)


def moe_plan(stage: int, stack, m: int, top_k: int, device: int = -1):
    """(workgroups, 16-row units per workgroup, pairs per sweep, waves that own part of k) of a GEMV launch (dg_moe_plan, DG_MOE_GEMV;
    nothing is launched; device < 0: planned for 256 compute units, no GPU needed)."""
    return _moe_plan(_lib.DG_MOE_GEMV, stage, stack, m, top_k, device, 4)


def moe_grouped_plan(stage: int, stack, m: int, top_k: int, device: int = -1):
    """(bm, bn, the grid's m-extent bound, n tiles, 64-k super-tiles per step, group workspace bytes, f32 workspace bytes) of a grouped launch
    (dg_moe_plan, DG_MOE_GROUPED; nothing is launched; device < 0: no GPU needed).  bm is the tile height dg_moe_group sorts for."""
    return _moe_plan(_lib.DG_MOE_GROUPED, stage, stack, m, top_k, device, 7)


def moe_group(ids: torch.Tensor, E: int, bm: int, out: torch.Tensor = None) -> torch.Tensor:
    """The group workspace (int32, include/decode_glue_hip.h: dg_moe_group; any4_amd/moe.py: group_ref is the definition) of ids int32
    [m, top_k]: the pairs sorted by expert and the tile list the grouped GEMMs walk.  bm: moe_grouped_plan()[0].  out: the buffer to fill."""
    from .moe import group_ws_ints

    _gpu(ids, out)
    if ids.dtype != torch.int32 or ids.dim() != 2:
        raise RuntimeError(f"moe_group: ids must be int32 [m, top_k], got {ids.dtype} {tuple(ids.shape)}")
    m, top_k = ids.shape
    if out is None:
        out = torch.empty(group_ws_ints(m * top_k, E, bm), dtype=torch.int32, device=ids.device)
    elif out.dtype != torch.int32 or out.dim() != 1:
        raise RuntimeError("moe_group: out must be a flat int32 tensor")
    _lib.check(_lib.load().dg_moe_group(ids.data_ptr(), out.data_ptr(), out.numel() * 4, m, top_k, E, bm, ids.device.index, _stream(ids)),
               "dg_moe_group")
    return out


def moe_gate_up_grouped(x: torch.Tensor, stack, ids: torch.Tensor, group_ws: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """moe_gate_up for many rows (DG_MOE_GROUPED, DG_MOE_GATE_UP): the tile GEMM over the pairs sorted by expert; its numerics are
    any4_amd/moe.py: moe_grouped_ref's (16-bit weights).  group_ws: moe_group(ids, ...)."""
    return _moe_stage("moe_gate_up_grouped", _lib.DG_MOE_GROUPED, _lib.DG_MOE_GATE_UP, x, stack, ids, out=out, group_ws=group_ws)


def moe_down_grouped(act: torch.Tensor, stack, ids: torch.Tensor, gates: torch.Tensor, group_ws: torch.Tensor, residual: torch.Tensor = None,
                     out: torch.Tensor = None, f32_ws: torch.Tensor = None) -> torch.Tensor:
    """moe_down for many rows (DG_MOE_GROUPED, DG_MOE_DOWN: the tile GEMM into f32_ws [m * top_k, n] float32, then the combine).
    out may be `residual` itself.  f32_ws: the workspace to use (it is not cleared and need not be)."""
    return _moe_stage("moe_down_grouped", _lib.DG_MOE_GROUPED, _lib.DG_MOE_DOWN, act, stack, ids, gates, residual, out, group_ws, f32_ws)


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    """gu [bs, 2 il] = [gate | up] -> silu(gate) * up [bs, il]."""
    _gpu(gu)
    bs, il = gu.shape[0], gu.shape[1] // 2
    out = torch.empty((bs, il), dtype=gu.dtype, device=gu.device)
    _lib.check(_lib.load().dg_swiglu(gu.data_ptr(), out.data_ptr(), bs, il, _dt(gu), gu.device.index, _stream(gu)), "dg_swiglu")
    return out


def linear16(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """y = x @ weight.T for a ROW-MAJOR 16-bit weight [n][k] (an nn.Linear's) and 1 ... 4 rows of x: the decode step's LM head.
    Returns None when the library has no instantiation for the shape (the caller keeps its GEMM)."""
    _gpu(x)
    m, k = x.shape
    n = weight.shape[0]
    if not (1 <= m <= (2 if k == 8192 else 4) and k in (2048, 4096, 8192) and weight.dtype == x.dtype and weight.is_contiguous() and x.is_contiguous()
            and weight.shape[1] == k and x.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0):
        return None
    y = torch.empty((m, n), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().dg_linear16(x.data_ptr(), weight.data_ptr(), y.data_ptr(), m, n, k, _dt(x), x.device.index, _stream(x)), "dg_linear16")
    return y

