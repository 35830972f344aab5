"""CPU suite: the definition of sampling (any4_amd/sampling.py: Philox4x32-10, the uniform of a (seed, place), temperature / top-k / top-p in
float64) and `DecodeStack.generate(..., temperature=...)` on the plain-torch path.  No GPU, no HIP compute."""
import math

import pytest
import torch

from any4_amd import sampling
from any4_amd.decode import DecodeConfig, DecodeStack
from tests.test_decode_cpu import CFG, SeededDense

NINF = float("-inf")


# ---------------------------------------------------------------- Philox, uniform

def test_philox_known_answers():
    """The three known-answer vectors of Philox4x32-10 (Random123's kat_vectors: zeros, all ones, the digits of pi)."""
    kat = [
        ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
        ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
        ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
    ]
    for ctr, key, want in kat:
        assert sampling.philox4x32_10(ctr, key).tolist() == want
    # ... and batched: the same three in one call
    got = sampling.philox4x32_10([c for c, _, _ in kat], [k for _, k, _ in kat])
    assert got.tolist() == [w for _, _, w in kat]


def test_uniform_is_a_24_bit_fraction_of_seed_and_counter_only():
    seed = torch.tensor([0, 1, -1, 2 ** 40 + 3, -2 ** 63, 2 ** 63 - 1])[:, None]
    ctr = torch.tensor([0, 1, 17, 2 ** 32, 2 ** 32 + 1, 2 ** 45 + 7])[None, :]
    u = sampling.uniform(seed, ctr)
    assert u.dtype == torch.float32 and u.shape == (6, 6)
    assert (u >= 0).all() and (u < 1).all()
    scaled = u.double() * 2 ** 24
    assert torch.equal(scaled, scaled.round())
    assert u.unique().numel() == 36  # (36 draws of 2^24 values: a collision would be a bug, not chance)
    # the definition, word for word: key = the seed's halves, counter = (the counter's halves, 0, 0), first word >> 8
    w = sampling.philox4x32_10([1, 2, 0, 0], [3, 1])[0].item()
    assert sampling.uniform(2 ** 32 + 3, 2 * 2 ** 32 + 1).item() == (w >> 8) * 2.0 ** -24
    # the high halves matter
    assert sampling.uniform(3, 1).item() != sampling.uniform(2 ** 32 + 3, 1).item()
    assert sampling.uniform(3, 1).item() != sampling.uniform(3, 2 ** 32 + 1).item()


# ---------------------------------------------------------------- sample_ref on hand-built rows

def _one(row, temperature=1.0, top_k=0, top_p=1.0, u=0.5):
    return sampling.sample_ref(torch.tensor([row], dtype=torch.float64), [temperature], [top_k], [top_p], [u]).item()


def test_greedy_is_the_lowest_index_argmax():
    row = [0.5, 3.0, 1.0, 3.0, -2.0, 3.0, 2.5]  # the maximum tied at 1, 3, 5
    for u in (0.0, 0.3, 1 - 2.0 ** -24):
        assert _one(row, temperature=0.0, u=u) == 1
        assert _one(row, top_k=1, u=u) == 1
    assert _one([1.0, 2.0, 7.0, 3.0], temperature=0.0) == 2 and _one([1.0, 2.0, 7.0, 3.0], top_k=1) == 2


def test_small_top_p_keeps_one_token():
    row = [0.0, 1.0, 4.0, 2.0]
    for u in (0.0, 0.5, 1 - 2.0 ** -24):
        assert _one(row, top_p=1e-6, u=u) == 2
    # exactly at a boundary the prefix is the SHORTEST with mass >= top_p Z: two equal tokens, top_p = 0.5 keeps the first
    assert {_one([1.0, 1.0], top_p=0.5, u=u) for u in (0.0, 0.6, 0.99)} == {0}
    assert {_one([1.0, 1.0], top_p=0.51, u=u) for u in (0.0, 0.6, 0.99)} == {0, 1}


def test_minus_infinity_is_never_returned():
    row = torch.tensor([0.0, NINF, 1.0, NINF, -1.0, NINF], dtype=torch.float64)
    n = 10 ** 4
    u = sampling.uniform(5, torch.arange(n))
    got = sampling.sample_ref(row.expand(n, -1), [1.5] * n, [0] * n, [1.0] * n, u)
    assert set(got.tolist()) == {0, 2, 4}


def test_u_at_both_ends():
    row = [0.0, 2.0, NINF, 1.0, 2.0, -3.0]  # ranks: 1, 4, 3, 0, 5, 2
    assert _one(row, u=0.0) == 1
    assert _one(row, u=1 - 2.0 ** -24) == 5                  # the last rank with weight (a -inf token is behind it and has none)
    assert _one(row, top_k=3, u=1 - 2.0 ** -24) == 3         # the last kept rank
    assert _one(row, top_k=2, u=1 - 2.0 ** -24) == 4
    assert _one(row, top_k=2, u=0.49) == 1 and _one(row, top_k=2, u=0.51) == 4  # two equal weights: the halves of [0, 1)


def test_top_k_is_applied_before_top_p():
    """Weights 4 : 2 : 1 : 1.  top_k = 2 first: Z_k = 6, and top_p = 0.7 needs 4.2 -> both of the two are kept.  top-p first would
    need 5.6 of 8 -> {0, 1}, the same set here, so take top_p = 0.6: k first needs 3.6 of 6 -> {0} alone; p first needs 4.8 of 8 -> {0, 1},
    then k = 2 changes nothing -> {0, 1}."""
    row = [math.log(4.0), math.log(2.0), 0.0, 0.0]
    us = [i / 64 for i in range(64)]
    assert {_one(row, top_k=2, top_p=0.6, u=u) for u in us} == {0}
    assert {_one(row, top_k=2, top_p=0.7, u=u) for u in us} == {0, 1}
    assert {_one(row, top_k=0, top_p=0.6, u=u) for u in us} == {0, 1}


def test_frequencies_match_the_kept_set_probabilities():
    """2e5 Philox draws on V = 8 under top_k = 6, top_p = 0.9, temperature 0.8: every token's frequency within 4 standard errors."""
    row = torch.tensor([1.0, -0.5, 2.0, 0.25, 2.0, -1.0, 0.5, NINF], dtype=torch.float64)
    T, k, p, n = 0.8, 6, 0.9, 2 * 10 ** 5
    # the kept set, by hand: ranks 2, 4, 0, 6, 3, 1 | 5, 7; weights relative to the maximum
    order = [2, 4, 0, 6, 3, 1]
    w = [math.exp((row[i].item() - 2.0) / T) for i in order]
    kept = next(j + 1 for j in range(k) if sum(w[: j + 1]) >= p * sum(w))
    prob = {i: (w[j] / sum(w[:kept]) if j < kept else 0.0) for j, i in enumerate(order)}
    u = sampling.uniform(12345, torch.arange(n))
    got = sampling.sample_ref(row.expand(n, -1), [T] * n, [k] * n, [p] * n, u)
    counts = torch.bincount(got, minlength=8).tolist()
    assert kept < k  # (the nucleus cuts something off, or this row tests top-k alone)
    for i in range(8):
        q = prob.get(i, 0.0)
        assert abs(counts[i] / n - q) <= 4 * math.sqrt(q * (1 - q) / n), (i, counts[i] / n, q)


# ---------------------------------------------------------------- the C entry points (no launch)

def test_dg_sample_is_exported_and_refuses_bad_calls_before_any_launch():
    from any4_amd import _lib, decode_ops

    lib = _lib.load()
    assert "dg_sample" in _lib.SYMBOLS and "dg_sample_scratch_bytes" in _lib.SYMBOLS and callable(decode_ops.sample)
    assert lib.tg_abi_version() == 10
    assert lib.dg_sample_scratch_bytes(8, 128256) == 0
    P = 0x10000  # never dereferenced: every call below is refused on the host
    good = dict(logits=P, ctr=P, temperature=P, top_k=P, top_p=P, seed=P, u_in=None, token_out=P, u_out=None, scratch=None, scratch_bytes=0,
                bs=2, vocab=1003, ld=1003, per_sequence=1, ctr_add=1, dtype=_lib.TG_BF16, device=0, stream=None)
    call = lambda **kw: lib.dg_sample(*dict(good, **kw).values())
    for name in ("logits", "ctr", "temperature", "top_k", "top_p", "token_out", "seed"):
        assert call(**{name: None}) == -1, name                   # TG_E_NULL (seed: needed when u_in is not given)
    assert call(dtype=2) == -5                                      # TG_E_DTYPE
    for kw in (dict(bs=0), dict(vocab=0), dict(ld=1002)):
        assert call(**kw) == -7, kw                                 # TG_E_SHAPE
    assert call(vocab=2 ** 30 + 1, ld=2 ** 30 + 1) == -10           # TG_E_SIZE
    for kw in (dict(logits=P + 1), dict(ctr=P + 4), dict(seed=P + 4), dict(token_out=P + 4), dict(temperature=P + 2), dict(top_k=P + 1),
               dict(top_p=P + 2), dict(u_in=P + 2), dict(u_out=P + 3)):
        assert call(**kw) == -8, kw                                 # TG_E_ALIGN
    with pytest.raises(RuntimeError):
        decode_ops.sample(torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.long), torch.ones(2), torch.zeros(2, dtype=torch.int32),
                          torch.ones(2), torch.zeros(2, dtype=torch.long))  # a CPU tensor: there is no fallback


# ---------------------------------------------------------------- the stack, plain torch

def _stack(cfg, bs, ragged=False):
    return DecodeStack(cfg, SeededDense(cfg, 0, 1), "cpu", torch.float32, bs=bs, seed=7, ragged=ragged)


def _prompt(cfg, bs, T, seed=0):
    return torch.randint(0, cfg.vocab, (bs, T), generator=torch.Generator().manual_seed(seed))


def test_generate_is_reproducible_and_depends_on_the_seed():
    cfg = DecodeConfig(**CFG)
    prompt = _prompt(cfg, 2, 4)
    runs = [_stack(cfg, 2).generate(prompt, 8, temperature=0.8, top_k=5, seed=s) for s in (0, 0, 1)]
    assert runs[0].shape == (2, 8) and runs[0].dtype == torch.long
    assert torch.equal(runs[0], runs[1])
    assert not torch.equal(runs[0], runs[2])
    assert ((runs[0] >= 0) & (runs[0] < cfg.vocab)).all()
    # a stack that never sampled has no sampling buffers; one that did has them, and `sampled` holds the last tokens
    fresh, used = _stack(cfg, 2), _stack(cfg, 2)
    assert "sampled" not in dict(fresh.named_buffers())
    out = used.generate(prompt, 3, temperature=0.8, top_k=5, seed=0)
    assert torch.equal(used.sampled, out[:, -1]) and torch.equal(out, runs[0][:, :3])


def test_top_k_1_is_the_greedy_generate():
    cfg = DecodeConfig(**CFG)
    prompt = _prompt(cfg, 2, 5, seed=3)
    greedy = _stack(cfg, 2).generate(prompt, 7)
    assert torch.equal(_stack(cfg, 2).generate(prompt, 7, temperature=1.3, top_k=1, seed=11), greedy)
    assert torch.equal(_stack(cfg, 2).generate(prompt, 7, temperature=0.0, seed=[4, 5]), greedy)


def test_each_token_is_the_definition_applied_to_the_steps_logits():
    cfg = DecodeConfig(**CFG)
    prompt = _prompt(cfg, 2, 3, seed=5)
    T, k, p, seed = [0.7, 1.1], [0, 6], [0.9, 1.0], [2 ** 40, -3]
    toks = _stack(cfg, 2).generate(prompt, 5, temperature=T, top_k=k, top_p=p, seed=seed)
    ref = _stack(cfg, 2)
    logits = ref.prefill(prompt)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)  # (the stack keeps temperature and top_p in float32)
    for i in range(5):
        u = sampling.uniform(torch.tensor(seed), 3 + i)
        assert torch.equal(sampling.sample_ref(logits, f32(T), k, f32(p), u), toks[:, i]), i
        logits = ref.decode(toks[:, i], 3 + i)


def test_a_ragged_sequence_does_not_depend_on_its_neighbour():
    cfg = DecodeConfig(**CFG)
    first = _prompt(cfg, 1, 6, seed=1)[0]
    runs = []
    for x, other in ((1, _prompt(cfg, 1, 6, seed=2)[0]), (99, _prompt(cfg, 1, 4, seed=8)[0]), (-5, _prompt(cfg, 1, 2, seed=9)[0])):
        runs.append(_stack(cfg, 2, ragged=True).generate([first, other], 6, temperature=0.9, top_k=8, top_p=0.95, seed=[7, x]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][0], runs[2][0])
    assert not torch.equal(runs[0][1], runs[1][1])
    # ... and with eos: a sequence that drew eos emits eos from then on
    eos = int(runs[0][0, 2])
    out = _stack(cfg, 2, ragged=True).generate([first, _prompt(cfg, 1, 6, seed=2)[0]], 6, eos=eos, temperature=0.9, top_k=8, top_p=0.95, seed=[7, 1])
    stop = runs[0][0].tolist().index(eos)
    assert out[0].tolist() == runs[0][0, : stop + 1].tolist() + [eos] * (5 - stop)


def test_host_refusals():
    cfg = DecodeConfig(**CFG)
    prompt = _prompt(cfg, 2, 3)
    stack = _stack(cfg, 2)
    for kw in (dict(temperature=-0.1), dict(temperature=[0.5, -1.0]), dict(temperature=float("nan")), dict(temperature=1.0, top_p=0.0),
               dict(temperature=1.0, top_p=[0.5, -0.5]), dict(temperature=[1.0]), dict(temperature=1.0, top_k=[1, 2, 3]),
               dict(temperature=1.0, seed=[1]), dict(temperature=1.0, top_p=[0.9, 0.9, 0.9]), dict(temperature=1.0, seed=2 ** 63)):
        with pytest.raises(ValueError):
            stack.generate(prompt, 2, **kw)
    assert "sampled" not in dict(stack.named_buffers())  # refused before anything was registered or launched
    headless = DecodeStack(cfg, SeededDense(cfg, 0, 1), "cpu", torch.float32, bs=2, seed=7, lm_head=False)
    with pytest.raises(ValueError):
        headless.generate(prompt, 2, temperature=1.0)
    with pytest.raises(ValueError):
        headless.set_sampling(1.0)
