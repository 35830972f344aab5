"""GPU suite: per-sequence LoRA adapters (dg_lora_shrink / dg_lora_expand, any4_amd/csrc/lora.cuh) -- exact lookup probes, float64 checks at
every loop regime of both kernels (tests/lora_ref.py: reference and bound), and the decode stack's three schedules with an adapter per
sequence, eager and replayed from a captured graph."""
import numpy as np
import pytest
import torch

from tests import lora_ref as R
from tests.conftest import bits16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F16 = torch.bfloat16, torch.float16
INT32_MIN = -2 ** 31
# the kernels' constants (any4_amd/csrc/lora.cuh)
LSH_PASS, LEX_COLS, LEX_ROWS = 4096, 512, 8


def _ids(n, n_adapters=3):
    """-1, repeats, n_adapters itself and INT32_MIN among valid ids."""
    pattern = [0, -1, 2, 2, n_adapters, INT32_MIN, 1, 0, n_adapters + 5, 1]
    return [pattern[i % len(pattern)] for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------------
# lookup probes, exact
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("rows_per_id", [1, 5])
@pytest.mark.parametrize("m", [1, 3, 16, 17, 40])
def test_lookup_probes_are_exact(m, rows_per_id, dtype):
    """Which adapter, which row, which column was read: A[a][j] is one-hot at a position of its own (the last element of k among them,
    in the ragged last pass), so t[i][j] = x[i][pos(a, j)]; B[a][c] holds the code (a + 1) + 4 (c mod 7) at j = c mod r and zeros elsewhere;
    x[i][p] = 1 + (i + p) mod 8, y_in = (3 i + c) mod 4, scale = 1, 1/2, 1/4.  Every y = y_in + scale code x is a number of at most 8
    significant bits (asserted), so the kernels' answer is exact.  y has a row stride of n + 8 inside NaN guards; ids mix -1, repeats,
    n_adapters and INT32_MIN; rows without an adapter keep their bit patterns (NaN payloads included) and every guard stays intact."""
    from any4_amd import decode_ops as G

    na, r, k, n = 3, 8, LSH_PASS + 8, LEX_COLS + 24
    ids = _ids(-(-m // rows_per_id), na)
    row_a = R.row_ids(ids, rows_per_id, m, na)
    pos = {(a, j): ((a * r + j) * 171 + 7) % k for a in range(na) for j in range(r)}
    pos[2, r - 1] = k - 1
    assert len(set(pos.values())) == na * r
    A = torch.zeros(na, r, k)
    for (a, j), p in pos.items():
        A[a, j, p] = 1
    c = torch.arange(n)
    B = torch.zeros(na, n, r)
    for a in range(na):
        B[a, c, c % r] = ((a + 1) + 4 * (c % 7)).float()
    scale = torch.tensor([1.0, 0.5, 0.25])
    x = (1 + (torch.arange(m)[:, None] + torch.arange(k)[None, :]) % 8).float()
    y_in = ((3 * torch.arange(m)[:, None] + c[None, :]) % 4).float()
    want = y_in.clone()
    for i in range(m):
        a = int(row_a[i])
        if a >= 0:
            t = torch.tensor([x[i, pos[a, j]] for j in range(r)])
            want[i] = y_in[i] + scale[a] * B[a, c, c % r] * t[c % r]
    assert torch.equal(want.to(dtype).float(), want) and want.max() > 100  # representable: the kernels' answer must be these bits
    # rows without an adapter carry NaN payloads in y: they must come back bit for bit
    y16 = y_in.to(dtype)
    nan_rows = torch.from_numpy(row_a < 0)
    y16.view(torch.int16)[nan_rows] = 0x7FC1 if dtype == BF16 else 0x7E01
    guard, ld = 2048, n + 8
    whole = torch.full((2 * guard + m * ld,), float("nan"), dtype=dtype, device=DEV)
    y = whole[guard: guard + m * ld].view(m, ld)[:, :n]
    y.copy_(y16)
    before = whole.clone()
    idx = torch.tensor(ids, dtype=torch.int32, device=DEV)
    t = G.lora_shrink(x.to(dtype).to(DEV), A.to(dtype).to(DEV), idx, rows_per_id)
    G.lora_expand(t, B.to(dtype).to(DEV), scale.to(DEV), idx, y, rows_per_id)
    torch.cuda.synchronize()
    for i in range(m):
        a = int(row_a[i])
        want_t = [float(x[i, pos[a, j]]) for j in range(r)] if a >= 0 else [0.0] * r
        assert t[i].tolist() == want_t, (i, a)
    got = y.cpu()
    adapted = ~nan_rows
    assert torch.equal(got[adapted].float(), want[adapted]), (got[adapted].float() - want[adapted]).abs().max()
    assert np.array_equal(bits16(got[nan_rows]), bits16(y16[nan_rows]))
    mask = torch.ones_like(whole, dtype=torch.bool)
    mask[guard: guard + m * ld].view(m, ld)[:, :n] = False
    assert np.array_equal(bits16(whole[mask]), bits16(before[mask])), "something outside y's n columns was written"


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 at every loop regime
# ---------------------------------------------------------------------------------------------------------------------------------

F64_CASES = [
    # m, k, r, n, dtype, norm, rows_per_id
    (3, 520, 8, LEX_COLS - 8, BF16, False, 1),
    (LEX_ROWS + 1, 2 * LSH_PASS, 16, LEX_COLS, BF16, True, 1),
    (17, LSH_PASS + 8, 64, 2 * LEX_COLS + 8, F16, True, 5),
    (5, 14336, 16, 2 * LEX_COLS + 8, BF16, True, 1),
    (4, 14336, 64, LEX_COLS + 8, F16, False, 2),
    (1, LSH_PASS, 16, 6144, BF16, True, 1),
    (LEX_ROWS, LSH_PASS, 8, LEX_COLS, F16, False, 1),
]


@pytest.mark.parametrize("case", F64_CASES, ids=lambda c: f"m{c[0]}-k{c[1]}-r{c[2]}-n{c[3]}-{'bf16' if c[4] == BF16 else 'f16'}{'-norm' if c[5] else ''}-rpi{c[6]}")
def test_both_kernels_against_float64(case):
    """k regimes of the shrink's loop, from lora.cuh's constants (LSH_THREADS = 512 lanes x 8 elements: LSH_PASS = 4096 per pass): below
    one pass (k = 520: 65 of the 512 lanes have work), exact multiples (4096, 8192), a ragged last pass (4104: one lane; 14336 = 3.5 passes,
    the Llama-3-8B down projection -- a millisecond on the device).  r = 8, 16, 64; slot 1 holds an adapter of rank 3, zero-padded.  n below
    (504), at (512) and across (520, 1032, 6144) one expand workgroup's LEX_COLS = 512 columns; m below, at and across its LEX_ROWS = 8
    rows.  bf16 and fp16, with and without the norm weight, ids mixing every kind of "no adapter".
    Bound: tests/lora_ref.py -- 1/2 ulp16 + 2^-24 ((k + r + 4) scale sum_j |B| sum_c |A x~| + |y_in|), + 2^-18 scale sum |B| sum |A x~| for
    rs with a norm weight -- derived there from the kernels' arithmetic, fixed before the first run on a device.  t is held to its own
    share of it.  Rows without an adapter keep their bits; two launches on the same inputs are bit-equal."""
    from any4_amd import decode_ops as G

    m, k, r, n, dtype, norm, rpi = case
    x, g, A, B, scale, y = R.make_case(m, k, r, n, dtype, seed=m + r)
    ids = [0, 1, -1, 2, 3, INT32_MIN, 1, 2, 0][: -(-m // rpi)] if m > 1 else [1]  # (m = 1: the rank-3 adapter)
    ref, tol, adapted, t_ref, t_tol = R.lora_ref64(x, A, B, scale, ids, rpi, y, g if norm else None)
    assert adapted.any()
    dx, dA, dB, ds = x.to(DEV), A.to(DEV), B.to(DEV), scale.to(DEV)
    dg = g.to(DEV) if norm else None
    idx = torch.tensor(ids, dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        dy = y.to(DEV)
        t = G.lora_shrink(dx, dA, idx, rpi, dg, R.EPS)
        G.lora_expand(t, dB, ds, idx, dy, rpi)
        outs.append((t.cpu(), dy.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and np.array_equal(bits16(outs[0][1]), bits16(outs[1][1])), "two launches differ"
    t, got = outs[0]
    t_err = np.abs(t.double().numpy() - t_ref)
    err = np.abs(got.double().numpy() - ref)
    live = adapted[:, None] & np.ones_like(err, dtype=bool)
    print(f"largest share of the bound: y {float((err[live] / tol[live]).max()):.3f}, t {float((t_err[adapted] / (t_tol[adapted] + 1e-300)).max()):.2e}")
    assert (t_err <= t_tol).all(), float((t_err - t_tol).max())
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    assert np.array_equal(bits16(got[~torch.from_numpy(adapted)]), bits16(y[~torch.from_numpy(adapted)]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the stack
# ---------------------------------------------------------------------------------------------------------------------------------

_BASE = dict(hidden=2048, inter=4096, layers=2, heads=16, kv_heads=4, head_dim=128, vocab=512, max_seq=64)
BS, RANK, NA = 3, 16, 3


def _weights(cfg, rank, seed, gain=1.0):
    gen = torch.Generator().manual_seed(seed)
    return {(layer, name): ((torch.randn(rank, k, generator=gen) / k ** 0.5).to(BF16), (gain * torch.randn(n, rank, generator=gen) / rank ** 0.5).to(BF16))
            for layer in range(cfg.layers) for name, n, k in cfg.linear_shapes()}


def _adapter_set(cfg, loads):
    from any4_amd.lora import AdapterSet

    aset = AdapterSet(cfg, NA, RANK, DEV, BF16)
    for slot, (rank, seed) in loads.items():
        aset.load(slot, _weights(cfg, rank, seed), alpha=float(rank))
    return aset


def _tol(ref):
    return 0.03 * ref.abs().max() + 1e-3  # tests/test_gpu_fused.py's tolerance of a fused stack against plain torch


@pytest.mark.parametrize("interleave", [8, 0])
def test_three_schedules_agree_eager_and_replayed(interleave):
    """Five launches, eight launches and plain torch (lora_ref) with ids [0, -1, 2] (slot 2: an adapter of rank 8 in a set of rank 16):
    three eager steps, then three steps replayed from captured graphs, each within 0.03 max|y| + 1e-3 of the torch stack.  The adapters are
    large enough to be seen: the torch stack's logits with and without them differ by at least ten times that tolerance.  After capture a
    change of `adapter_ids` and a re-load of a slot both take effect on the next replay.  interleave = 0 also: with all ids -1 the fused
    stack's logits are bit for bit those of a fused stack built without adapters (the launches in front of the expand are the same)."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**dict(_BASE, gate_up_interleave=interleave))
    loads = {0: (RANK, 1), 2: (8, 2)}

    def stack(adapters=True, **kw):
        return DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=BS, seed=9, adapters=_adapter_set(cfg, loads) if adapters else None, **kw)

    five, eight, ref, bare = stack(), stack(fuse_gemm_stages=False), stack(fused=False), stack(adapters=False, fused=False)
    assert five._five_launch() and not eight._five_launch()
    gen = torch.Generator().manual_seed(4)
    toks = torch.randint(0, cfg.vocab, (BS, 9), generator=gen).to(DEV)
    ids = [0, -1, 2]

    def compare(i, adapters=None):
        want = ref.decode(toks[:, i], i, adapters=adapters)
        for name, s in (("five", five), ("eight", eight)):
            got = s.decode(toks[:, i], i, adapters=adapters)
            err = (got.float() - want.float()).abs().max()
            assert err <= _tol(want.float()), (name, i, float(err), float(_tol(want.float())))
        return want

    for i in range(3):
        want = compare(i, ids if i == 0 else None)
        plain = bare.decode(toks[:, i], i)
        moved = (want.float() - plain.float()).abs().amax(dim=1)
        assert moved[0] >= 10 * _tol(want.float()) and moved[2] >= 10 * _tol(want.float()), (i, moved.tolist(), float(_tol(want.float())))
    assert five.layers[0].launches() == 5 + 1 + 8 and five.layers[0]._fuse["mlp"] is False  # (gate_up gives up its SwiGLU store)
    five.capture()
    eight.capture()
    assert five.kernels_per_layer == 14 and five.graph_nodes == 2 * 14 + 3
    for i in range(3, 6):
        compare(i)
    compare(6, [2, 0, -1])                       # new ids, read by the captured step
    for s in (five, eight, ref):                 # a re-load of slot 0 in place
        s.adapters.load(0, _weights(cfg, RANK, 7), alpha=float(RANK))
    before = five._out.clone()
    compare(7)
    assert not torch.equal(before, five._out)
    if interleave == 0:
        none5 = stack(adapters=False)
        all_off = stack()
        for i in range(3):
            assert torch.equal(all_off.decode(toks[:, i], i, adapters=[-1, -1, -1]), none5.decode(toks[:, i], i)), i


def test_captured_stack_serves_generate_with_a_longer_prefill():
    """The serving order: `capture()`, then `generate()` whose prefill brings more rows (bs x T) than the captured step (bs).  The graph
    holds the address of the scratch `t` it was captured on, so that buffer must survive the prefill's larger one.  Checked against the
    `fused=False` twin fed with the captured stack's own tokens (so both see the same context at every step): the two stacks' logits
    are within tol = 0.03 max|y| + 1e-3 of each other, hence every generated token's twin logit is within 2 tol of the twin's maximum;
    and one more replayed step agrees with the twin's logits within tol."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**dict(_BASE, gate_up_interleave=8))
    loads = {0: (RANK, 1), 2: (8, 2)}
    ids, T, new = [0, -1, 2], 6, 4
    five = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=BS, seed=9, adapters=_adapter_set(cfg, loads))
    twin = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, bs=BS, seed=9, adapters=_adapter_set(cfg, loads), fused=False)
    five.set_adapters(ids)
    five.capture()
    captured_on = five.adapters.scratch(BS).data_ptr()
    prompt = torch.randint(0, cfg.vocab, (BS, T), generator=torch.Generator().manual_seed(6)).to(DEV)
    got = five.generate(prompt, new, adapters=ids)
    assert five._graph is not None and got.shape == (BS, new)
    assert five.adapters.scratch(BS).data_ptr() != captured_on, "the prefill was expected to outgrow the step's scratch"
    assert five.adapters._buffers[0].data_ptr() == captured_on  # still owned by the set: the graph's replays wrote into live memory
    logits = twin.prefill(prompt, adapters=ids)
    for i in range(new):
        lf = logits.float()
        picked = lf.gather(1, got[:, i: i + 1]).squeeze(1)
        assert (picked >= lf.amax(dim=1) - 2 * _tol(lf)).all(), (i, picked.tolist(), lf.amax(dim=1).tolist(), float(_tol(lf)))
        logits = twin.decode(got[:, i], T + i)
    if new > 1:  # `logits` is now the twin's answer to the last generated token; the captured stack's, by one more replay
        replayed = five.decode(got[:, new - 1], T + new - 1)
        err = (replayed.float() - logits.float()).abs().max()
        assert err <= _tol(logits.float()), (float(err), float(_tol(logits.float())))


def test_ragged_paged_mx8_generate_with_mixed_adapters():
    """A ragged stack with a paged mx8 cache: one `generate` with mixed adapters gives its `fused=False` twin's tokens under greedy
    decoding.  A row (sequence) is compared only if every step's top-2 gap of the twin's logits is at least the tolerance 0.03 max|y| +
    1e-3; with the prompt seed used here the twin keeps three of the four rows, and at least three quarters are required."""
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**dict(_BASE, gate_up_interleave=8))
    bs, new, ids, lens = 4, 3, [0, -1, 2, 0], [5, 2, 7, 4]
    loads = {0: (RANK, 1), 2: (8, 2)}
    kw = dict(bs=bs, seed=9, ragged=True, kv_cache="mx8", kv_pages=8, page_size=64, mx8_attention="online")
    fused = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, adapters=_adapter_set(cfg, loads), **kw)
    twin = DecodeStack(cfg, Any4Factory(cfg, DEV, seed=3), DEV, adapters=_adapter_set(cfg, loads), fused=False, **kw)
    gen = torch.Generator().manual_seed(103)
    prompts = [torch.randint(0, cfg.vocab, (n,), generator=gen).to(DEV) for n in lens]
    padded = torch.zeros(bs, max(lens), dtype=torch.long, device=DEV)
    for b, p in enumerate(prompts):
        padded[b, : lens[b]] = p
    logits = twin.prefill(padded, position=0, lengths=lens, adapters=ids)
    keep, want = torch.ones(bs, dtype=torch.bool, device=DEV), []
    for i in range(new):
        top2 = logits.float().topk(2, dim=1).values
        keep &= (top2[:, 0] - top2[:, 1]) >= _tol(logits.float())
        want.append(logits.argmax(-1))
        if i + 1 < new:
            logits = twin.decode(want[-1], [n + i for n in lens])
    print(f"rows kept {keep.tolist()}")
    assert int(keep.sum()) * 4 >= 3 * bs, keep.tolist()
    got = fused.generate(prompts, new, adapters=ids)
    want = torch.stack(want, dim=1)
    assert fused.adapter_ids.tolist() == ids
    assert torch.equal(got[keep], want[keep]), (got.tolist(), want.tolist(), keep.tolist())


def test_lora_linear_no_grad_is_the_stacks_per_linear_path():
    """LoRALinear under no_grad runs the two kernels: bit for bit what the stack adds behind the same linear with the module loaded into
    an AdapterSet (another slot, a set of three, an id per row)."""
    from any4_amd.decode import Any4Factory, DecodeConfig
    from any4_amd.lora import AdapterCall, AdapterSet, LoRALinear

    cfg = DecodeConfig(**dict(_BASE, layers=1))
    base = Any4Factory(cfg, DEV, seed=3)("o", 0, cfg.heads * cfg.head_dim, cfg.hidden)
    mod = LoRALinear(base, rank=RANK, alpha=32.0, seed=1)
    with torch.no_grad():
        mod.B.copy_(torch.randn(cfg.hidden, RANK, generator=torch.Generator().manual_seed(2)).to(BF16))
    x = torch.randn(BS, cfg.heads * cfg.head_dim, generator=torch.Generator().manual_seed(3)).to(BF16).to(DEV)
    with torch.no_grad():
        got = mod(x)
        plain = base(x)
    aset = AdapterSet(cfg, NA, RANK, DEV, BF16, targets=("o",))
    aset.load_modules(1, {(0, "o"): mod})
    call = AdapterCall(aset, torch.tensor([1, 1, 1], dtype=torch.int32, device=DEV), 1, fused=True)
    want = call.apply(0, "o", x, plain.clone())
    assert np.array_equal(bits16(got), bits16(want))
    assert (got.float() - plain.float()).abs().max() > 0.1  # (the adapter is not a no-op)
    y = mod(x.clone().requires_grad_(True))  # the training form: torch matmuls under autograd, the same numbers to 16-bit rounding
    assert y.requires_grad and (y.float() - got.float()).abs().max() <= 0.03 * got.float().abs().max()
