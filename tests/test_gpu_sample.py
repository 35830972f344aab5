"""GPU suite (-m gpu): the fused sampler (dg_sample, any4_amd/csrc/sample.cuh; decode_ops.sample) against its definition
(any4_amd/sampling.py), and DecodeStack.generate(..., temperature=...) on the fused path.

EPS -- the tolerance of the comparison against float64 -- follows from the kernel's arithmetic, not from what it was seen to do.
A token's weight is expf((l - l_max) / T) in float32, turned into a 64-bit integer multiple of 2^-s (s = 62 - bit_length(V)); everything
behind that is integer arithmetic (exact, whatever the order) and a handful of float64 products (2^-52 each):
  * the argument a = (l_max - l) / T is formed in float64 and rounded to float32 once (relative 2^-24; the bound below allows 2^-23,
    what two rounded float32 operations would give), so the weight e^-a carries a relative error of at most a 2^-23;
  * expf: at most 3 ulp (the bound OpenCL sets for exp, which the device library meets with margin): 3 x 2^-23 relative;
  * the floor to a multiple of 2^-s: at most 2^-s per token, V 2^-s <= 2^(2 bit_length(V) - 62) in any sum -- 2^-28 at V = 128256.
So a token's weight is off by a relative r_i <= 2^-23 (3 + a_i), and a NORMALISED cumulative mass S / Z by at most
  |dS| / Z + S |dZ| / Z^2  <=  2 sum_i p_i r_i  =  2^-22 (3 + sum_i p_i a_i),          p_i = e^-a_i / Z the token's probability.
sum_i p_i a_i = -sum_i p_i ln(p_i Z) = H(p) - ln Z <= H(p) <= ln V (Z >= 1: the largest logit has weight 1).  Hence
  EPS(V) = 2^-22 (3 + ln V) + 2^-27:   2.4e-6 at V = 1003, 3.2e-6 at 32000, 3.5e-6 at 128256  (the condition is EPS <= 1e-5).
test_against_float64 prints the largest excursion beyond the exact float64 interval that it saw; DESIGN.md 18 records both."""
import math

import pytest
import torch

from any4_amd import sampling

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")
U_LAST = 1 - 2.0 ** -24
DTYPES = [torch.bfloat16, torch.float16]


def eps_of(V):
    eps = 2.0 ** -22 * (3 + math.log(V)) + 2.0 ** -27
    assert eps <= 1e-5
    return eps


def _t(vals, dtype):
    return torch.as_tensor(vals, dtype=dtype, device=DEV).contiguous()


def _launch(logits, temperature, top_k, top_p, u=None, seed=None, ctr=None, ctr_add=1, want_u=False):
    """decode_ops.sample with per-sequence host lists or scalars; returns tokens (and the u used)."""
    from any4_amd import decode_ops as G

    bs = logits.shape[0]
    per = lambda x, dt: _t(x if isinstance(x, (list, tuple, torch.Tensor)) else [x] * bs, dt)
    u_out = torch.full((bs,), -1.0, dtype=torch.float32, device=DEV) if want_u else None
    tok = G.sample(logits, _t([0] if ctr is None else ctr, torch.long), per(temperature, torch.float32), per(top_k, torch.int32),
                   per(top_p, torch.float32), None if seed is None else per(seed, torch.long), ctr_add,
                   u=None if u is None else per(u, torch.float32), u_out=u_out)
    torch.cuda.synchronize()
    return (tok, u_out) if want_u else tok


def _randn_logits(V, dtype, rows, seed):
    return (4 * torch.randn(rows, V, generator=torch.Generator().manual_seed(seed))).to(dtype).to(DEV).contiguous()


def _first_argmax(logits):
    """Lowest index of the maximum of every row, without any of the code under test."""
    l = logits.double()
    m = l.max(dim=1, keepdim=True).values
    idx = torch.arange(l.shape[1], device=l.device).expand_as(l)
    return torch.where(l == m, idx, l.shape[1]).min(dim=1).values


# ---------------------------------------------------------------- the device's random numbers

def test_device_uniform_is_the_definitions_bit_for_bit():
    g = torch.Generator().manual_seed(11)
    seeds = [0, 1, -1, 2 ** 32 + 5, -2 ** 40, 2 ** 63 - 1, -2 ** 63, 2 ** 32 - 1] + \
        torch.randint(-2 ** 63, 2 ** 63 - 1, (56,), generator=g, dtype=torch.long).tolist()
    ctrs = [0, 5, 2 ** 32, 2 ** 32 - 1, 2 ** 40 + 3, 2 ** 62, 1, 2 ** 33 + 1] + torch.randint(0, 2 ** 62, (56,), generator=g, dtype=torch.long).tolist()
    logits = _randn_logits(7, torch.bfloat16, 64, seed=1)
    assert sum(s >= 2 ** 32 for s in seeds) > 8 and sum(s < 0 for s in seeds) > 8 and sum(c >= 2 ** 32 for c in ctrs) > 8
    # a counter per sequence, ctr_add = 1 and 0
    for add in (1, 0):
        tok, u = _launch(logits, 1.0, 0, 1.0, seed=seeds, ctr=ctrs, ctr_add=add, want_u=True)
        want = sampling.uniform(torch.tensor(seeds), torch.tensor(ctrs) + add)
        assert torch.equal(u.cpu(), want) and ((tok >= 0) & (tok < 7)).all()
        for b in range(64):  # ... and the token is the one that u selects
            assert _judge(logits[b], 1.0, 0, 1.0, u[b: b + 1], tok[b: b + 1], eps_of(7))[0].all(), b
    # one counter for all 64 sequences
    for c in (3, 2 ** 33 + 7):
        _, u = _launch(logits, 1.0, 0, 1.0, seed=seeds, ctr=[c], ctr_add=1, want_u=True)
        assert torch.equal(u.cpu(), sampling.uniform(torch.tensor(seeds), c + 1))
    # a negative counter: the sequence is inactive
    tok, u = _launch(logits[:3], 1.0, 0, 1.0, seed=[1, 2, 3], ctr=[-1, 3, -2 ** 40], want_u=True)
    assert tok[0].item() == -1 and tok[2].item() == -1 and 0 <= tok[1].item() < 7
    assert u.tolist() == [0.0, sampling.uniform(2, 4).item(), 0.0]
    tok = _launch(logits[:3], 1.0, 0, 1.0, seed=[1, 2, 3], ctr=[-5])
    assert tok.tolist() == [-1, -1, -1]


# ---------------------------------------------------------------- exact cases (u given)

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("V", [1, 7, 1003, 50257])
def test_exact_cases(V, dtype):
    """bs = 3, ld = V: rows 1 and 2 of an odd V start off a 16-byte (and off a 4-byte) boundary."""
    logits = _randn_logits(V, dtype, 3, seed=V)
    first = _first_argmax(logits)
    us = [0.25, 0.6, U_LAST]
    assert torch.equal(_launch(logits, 0.0, 0, 1.0, u=us), first)                       # temperature 0
    assert torch.equal(_launch(logits, 0.0, 5, 0.5, u=us), first)
    assert torch.equal(_launch(logits, 0.9, 1, 1.0, u=us), first)                       # top_k = 1
    assert torch.equal(_launch(logits, 1.1, 0, 1e-6, u=us), first)                      # a tiny top_p
    assert torch.equal(_launch(logits, 1.3, 0, 1.0, u=0.0), first)                      # u = 0
    assert torch.equal(_launch(logits, 1.3, 7, 0.9, u=0.0), first)
    # u = 1 - 2^-24 under top_k = 3 at a high temperature: the third rank (it holds far more than 2^-24 of the three's mass)
    k = min(3, V)
    vals, order = torch.sort(logits.double(), dim=1, descending=True, stable=True)
    w = torch.exp((vals[:, :k] - vals[:, :1]) / 50.0)
    assert (w[:, -1] / w.sum(1) > 0.2).all()
    assert torch.equal(_launch(logits, 50.0, k, 1.0, u=U_LAST), order[:, k - 1])
    # ties: the maximum at three indices (none of them the row's first or last vector only), top_k = 2 -> the two lowest, split at u = 1/2
    if V >= 3:
        tied = logits.clone()
        at = sorted({0, V // 2, V - 1}) if V < 64 else [V // 3, V // 3 + 1, V - 1]
        top = tied.float().max().item() + 1.0
        for i in at:
            tied[:, i] = top
        assert _launch(tied, 0.7, 2, 1.0, u=[0.0, 0.49, 0.51]).tolist() == [at[0], at[0], at[1]]
        assert _launch(tied, 0.7, 2, 1.0, u=[0.99, U_LAST, 0.5]).tolist() == [at[1], at[1], at[1]]
        assert _launch(tied, 0.7, 3, 1.0, u=[0.3, 0.4, 0.7]).tolist() == [at[0], at[1], at[2]]
        assert _launch(tied, 0.0, 0, 1.0, u=us).tolist() == [at[0]] * 3
    # the end of a nucleus: four tokens of weight 1 and nothing else that counts (e^-60 each) -> top_p = 0.6 needs 2.4 of 4 and keeps
    # the three lowest; u = 1 - 2^-24 gives the last KEPT rank, not the fourth; thirds of [0, 1) inside
    if V >= 7:
        four = torch.full((3, V), -30.0, dtype=dtype, device=DEV)
        at = [1, 3, 4, 6] if V < 64 else [V // 5, V // 5 + 1, V // 2, V - 1]
        for i in at:
            four[:, i] = 30.0
        assert _launch(four, 1.0, 0, 0.6, u=[U_LAST, 0.67, 0.66]).tolist() == [at[2], at[2], at[1]]
        assert _launch(four, 1.0, 4, 0.6, u=[U_LAST, 0.0, 0.34]).tolist() == [at[2], at[0], at[1]]
        assert _launch(four, 1.0, 0, 0.76, u=[U_LAST, 0.74, 0.76]).tolist() == [at[3], at[2], at[3]]   # 3.04 of 4: all four
        assert _launch(four, 1.0, 0, 0.75, u=[U_LAST, 0.67, 0.3]).tolist() == [at[2], at[2], at[0]]    # exactly 3 of 4: three suffice


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("V", [1, 7, 1003])
def test_a_row_of_one_value(V, dtype):
    """Every token has the same weight: the answer is min(floor(u V), V - 1).  u sits in the middle of a token's interval (0.5 / V from
    its edges, float32 rounding of u is 6e-8), at both ends of the tie run and inside it."""
    js = sorted({0, 1 % V, V // 3, V // 2, V - 2 if V > 1 else 0, V - 1})
    logits = torch.full((len(js), V), -1.5, dtype=dtype, device=DEV)
    for T in (1.0, 0.3):
        assert _launch(logits, T, 0, 1.0, u=[(j + 0.5) / V for j in js]).tolist() == js
    assert _launch(logits, 1.0, 0, 1.0, u=U_LAST).tolist() == [V - 1] * len(js)
    assert _launch(logits, 1.0, 0, 1.0, u=0.0).tolist() == [0] * len(js)
    k = max(1, V // 2)
    assert _launch(logits, 1.0, k, 1.0, u=[(j + 0.5) / V for j in js]).tolist() == [min(int((j + 0.5) / V * k), k - 1) for j in js]


# ---------------------------------------------------------------- against the float64 definition

PARAMS = [(0, 1.0, 1.0), (50, 1.0, 0.7), (0, 0.9, 1.0), (40, 0.95, 1.3)]  # (top_k, top_p, temperature)
DRAWS = 4096


def _f32(x):
    return torch.tensor(x, dtype=torch.float32).item()


def _judge(row, temperature, top_k, top_p, u, tok, eps):
    """The acceptance rule for draws `u` [n] -> tokens `tok` [n] from ONE row under one parameter set, in float64 on the row's device.
    Returns (accepted [n] bool, excursion beyond the exact float64 interval [n], smallest probability of a kept token)."""
    V = row.numel()
    T, p = _f32(temperature), _f32(top_p)
    vals, order = torch.sort(row.double(), descending=True, stable=True)
    rank = torch.empty(V, dtype=torch.long, device=row.device)
    rank[order] = torch.arange(V, device=row.device)
    k = V if top_k <= 0 or top_k >= V else top_k
    weights = torch.exp((vals[:k] - vals[0]) / T)
    cum = torch.cumsum(weights, 0)

    def kept(pp):
        return k if pp >= 1 else min(int(torch.searchsorted(cum, pp * cum[-1], right=False)) + 1, k)

    exact, fewer, more = (kept(p), kept(p - eps), kept(p + eps)) if p < 1 else (k, k, k)
    assert fewer <= exact <= more
    assert ((tok >= 0) & (tok < V)).all()
    assert torch.isfinite(row[tok].float()).all()  # strictly: a -inf token has an empty interval at the top end and is never returned
    r = rank[tok]
    rc = r.clamp(max=k - 1)
    hi, lo = cum[rc], torch.where(rc > 0, cum[(rc - 1).clamp(min=0)], 0.0)
    u = u.double()
    ok = (r < more) & (u >= lo / cum[more - 1] - eps) & (u <= hi / cum[fewer - 1] + eps)
    z = cum[exact - 1]
    exc = torch.maximum(lo / z - u, u - hi / z).clamp(min=0)
    w = weights[:exact]  # (not the differences of `cum`: a device cumsum is a tree, its differences carry rounding noise)
    return ok, exc, (w[w > 0].min() / z).item()


def _tie_heavy(V, dtype, seed):
    """8 distinct values, one of them -inf: 120 tokens on 7 finite values in random places, the rest -inf."""
    g = torch.Generator().manual_seed(seed)
    row = torch.full((V,), NINF)
    at = torch.randperm(V, generator=g)[:120]
    row[at] = 2.0 - 0.25 * torch.randint(0, 7, (120,), generator=g).float()
    return row.to(dtype)


@pytest.mark.parametrize("kind", ["randn", "ties"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("V", [1003, 32000, 128256])
def test_against_float64(V, dtype, kind, capsys):
    """4096 draws per launch from one row, the four parameter sets and one launch in which they alternate by row."""
    eps = eps_of(V)
    row = (_randn_logits(V, dtype, 1, seed=V + 1)[0] if kind == "randn" else _tie_heavy(V, dtype, seed=V + 2).to(DEV))
    logits = row.expand(DRAWS, V).contiguous()
    g = torch.Generator().manual_seed(V)
    u = torch.rand(DRAWS, generator=g).to(DEV)
    u[:4] = torch.tensor([0.0, U_LAST, 0.5, 2.0 ** -24], device=DEV)
    worst = 0.0
    for top_k, top_p, temperature in PARAMS:
        tok = _launch(logits, temperature, top_k, top_p, u=u)
        ok, exc, pmin = _judge(row, temperature, top_k, top_p, u, tok, eps)
        if kind == "ties":
            assert pmin >= 1e-3  # (on the reference alone: the check is then token equality, a token's interval is 300 EPS wide)
        assert ok.all(), (top_k, top_p, temperature, int((~ok).sum()), exc[~ok][:4].tolist())
        worst = max(worst, exc.max().item())
    # the parameters differ per row
    which = torch.arange(DRAWS) % len(PARAMS)
    tok = _launch(logits, [PARAMS[i][2] for i in which], [PARAMS[i][0] for i in which], [PARAMS[i][1] for i in which], u=u)
    for i, (top_k, top_p, temperature) in enumerate(PARAMS):
        sel = (which == i).to(DEV)
        ok, exc, _ = _judge(row, temperature, top_k, top_p, u[sel], tok[sel], eps)
        assert ok.all(), ("per row", i)
        worst = max(worst, exc.max().item())
    with capsys.disabled():
        print(f"\n[sample vs float64] V={V} {str(dtype)[6:]} {kind}: largest excursion beyond the float64 interval {worst:.3e} (EPS {eps:.3e})")


def _wide_row(V, dtype, seed):
    """Random 16-bit patterns: every binade of both signs occurs.  NaN and +inf patterns become finite ones, -inf patterns stay -inf."""
    ones, low = (0x7C00, 0x0400) if dtype == torch.float16 else (0x7F80, 0x0080)  # the exponent field, its lowest bit
    bits = torch.randint(0, 1 << 16, (V,), generator=torch.Generator().manual_seed(seed))
    special = (bits & ones) == ones
    bits = torch.where(special & (bits >= 0x8000), 0x8000 | ones, torch.where(special, bits & ~low, bits))
    return (bits - ((bits >= 0x8000).long() << 16)).to(torch.int16).view(dtype)


def _keys(row):
    """Every token's key: ascending key = descending value, -0 counted as +0 (restated here, not taken from the kernel)."""
    bits = row.cpu().view(torch.int16).long() & 0xFFFF
    bits = torch.where(bits == 0x8000, 0, bits)
    return torch.where(bits >= 0x8000, bits, 0x7FFF - bits)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_rows_wider_than_one_window(dtype, capsys):
    """A row that occupies about a thousand of the 64-value bins, so the kernel's tables hold it in two windows (the second begins inside
    the negative values).  At the temperatures of PARAMS all the mass sits on the largest value and only the walks that count ranks reach
    the second window; at a temperature of a third of the largest logit the mass is spread over both, so draws, nuclei and top-k cuts
    end in the first window, in the second, and (top_k next to the number of tokens in the first) on either side of the boundary."""
    V = 128256
    eps = eps_of(V)
    row = _wide_row(V, dtype, seed=17).to(DEV)
    keys = _keys(row)
    bins = torch.unique(keys >> 6)  # bins of 64 consecutive values that hold a token, ascending: the kernel's tables hold 512 of them
    assert bins.numel() > 900
    first = int(((keys >> 6) <= bins[511]).sum())
    assert V // 3 < first < 2 * V // 3  # tokens in the first 512 occupied bins: the others need the second window
    logits = row.expand(DRAWS, V).contiguous()
    u = torch.rand(DRAWS, generator=torch.Generator().manual_seed(3)).to(DEV)
    u[:4] = torch.tensor([0.0, U_LAST, 0.5, 2.0 ** -24], device=DEV)
    hot = _f32(row.float().max().item() / 3)
    sets = PARAMS + [(0, 1.0, hot), (50, 1.0, hot), (first - 1, 1.0, hot), (first, 1.0, hot), (first + 1, 1.0, hot), (first + 5000, 0.9, hot),
                     (0, 0.5, hot), (0, 0.97, hot), (V - 1, 0.999, hot)]
    worst, second = 0.0, 0
    rank_of = torch.empty(V, dtype=torch.long, device=DEV)
    rank_of[torch.sort(row.double(), descending=True, stable=True).indices] = torch.arange(V, device=DEV)
    for top_k, top_p, temperature in sets:
        tok = _launch(logits, temperature, top_k, top_p, u=u)
        ok, exc, _ = _judge(row, temperature, top_k, top_p, u, tok, eps)
        assert ok.all(), (top_k, top_p, temperature, int((~ok).sum()), exc[~ok][:4].tolist())
        worst = max(worst, exc.max().item())
        second += int((rank_of[tok] >= first).sum())
    assert second > DRAWS // 2  # draws that ended in the second window
    # top_k = 1 and temperature 0: the first token of the largest value
    top = _first_argmax(row[None])
    assert torch.equal(_launch(logits[:64], hot, 1, 1.0, u=u[:64]), top.expand(64))
    assert torch.equal(_launch(logits[:64], 0.0, 0, 1.0, u=u[:64]), top.expand(64))
    # ... and parameters that differ per row, so that neighbouring workgroups walk different windows
    which = torch.arange(DRAWS) % len(sets)
    tok = _launch(logits, [sets[i][2] for i in which], [sets[i][0] for i in which], [sets[i][1] for i in which], u=u)
    for i, (top_k, top_p, temperature) in enumerate(sets):
        sel = (which == i).to(DEV)
        assert _judge(row, temperature, top_k, top_p, u[sel], tok[sel], eps)[0].all(), ("per row", i)
    with capsys.disabled():
        print(f"\n[sample, two windows] {str(dtype)[6:]}: {bins.numel()} occupied bins, {first} tokens in the first 512; "
              f"largest excursion beyond the float64 interval {worst:.3e} (EPS {eps:.3e})")


# ---------------------------------------------------------------- determinism

@pytest.mark.parametrize("V", [1003, 32000])
def test_deterministic_and_row_independent(V):
    bs = 64
    wide = _randn_logits(V + 5, torch.bfloat16, bs, seed=3)
    logits = wide[:, 3: 3 + V]  # rows 2 (V + 5) bytes apart, starting 6 bytes into the row: ld > vocab
    g = torch.Generator().manual_seed(5)
    T = (0.5 + torch.rand(bs, generator=g)).tolist()
    k = torch.randint(0, 60, (bs,), generator=g).tolist()
    p = (0.5 + 0.5 * torch.rand(bs, generator=g)).tolist()
    seeds = torch.randint(-2 ** 62, 2 ** 62, (bs,), generator=g).tolist()
    ctr = torch.randint(0, 2 ** 40, (bs,), generator=g).tolist()
    a = _launch(logits, T, k, p, seed=seeds, ctr=ctr)
    assert torch.equal(a, _launch(logits, T, k, p, seed=seeds, ctr=ctr))
    assert torch.equal(a, _launch(logits.contiguous(), T, k, p, seed=seeds, ctr=ctr))
    perm = torch.randperm(bs, generator=g).tolist()
    pick = lambda x: [x[i] for i in perm]
    b = _launch(logits[perm].contiguous(), pick(T), pick(k), pick(p), seed=pick(seeds), ctr=pick(ctr))
    assert torch.equal(b, a[perm])
    # ... and it is the definition's token (these 64 draws keep their distance from every edge; test_against_float64 has the rule)
    u = sampling.uniform(torch.tensor(seeds), torch.tensor(ctr) + 1)
    ref = sampling.sample_ref(logits.cpu(), torch.tensor(T, dtype=torch.float32), k, torch.tensor(p, dtype=torch.float32), u)
    for i in range(bs):
        ok, _, _ = _judge(logits[i], T[i], k[i], p[i], u[i: i + 1].to(DEV), a[i: i + 1], eps_of(V))
        assert ok.all(), i
    assert (ref.to(DEV) == a).float().mean() > 0.9


# ---------------------------------------------------------------- the stack

CFG = dict(hidden=256, inter=512, layers=2, heads=4, kv_heads=2, head_dim=64, max_seq=128, group_size=64)
SAMPLING = dict(temperature=[0.8, 1.2], top_k=[20, 0], top_p=[1.0, 0.9], seed=[2 ** 40 + 1, -7])


def _stack(vocab, weights=3, **kw):
    from any4_amd.decode import Any4Factory, DecodeConfig, DecodeStack

    cfg = DecodeConfig(**dict(CFG, vocab=vocab))
    return DecodeStack(cfg, Any4Factory(cfg, DEV, seed=weights), DEV, **dict(dict(bs=2, seed=9), **kw))


def _prompt(vocab, bs=2, T=5, seed=0):
    return torch.randint(0, vocab, (bs, T), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _tokens_obey_the_definition(stack, logits, ctr, tok, params):
    """Each token against sample_ref's rule on the very logits it was drawn from (no GEMM tolerance: only EPS)."""
    V = logits.shape[1]
    for b in range(logits.shape[0]):
        if ctr[b] < 0:
            assert tok[b].item() == -1
            continue
        u = sampling.uniform(params["seed"][b], ctr[b]).reshape(1).to(DEV)
        ok, _, _ = _judge(logits[b], params["temperature"][b], params["top_k"][b], params["top_p"][b], u, tok[b: b + 1], eps_of(V))
        assert ok.all(), (b, ctr[b])


@pytest.mark.usefixtures("reference_numerics")
@pytest.mark.parametrize("vocab", [1003, 32000])
def test_generate_samples_reproducibly_eager_and_captured(vocab):
    prompt, n = _prompt(vocab), 6
    eager = _stack(vocab).generate(prompt, n, **SAMPLING)
    assert eager.shape == (2, n) and ((eager >= 0) & (eager < vocab)).all()
    assert torch.equal(eager, _stack(vocab).generate(prompt, n, **SAMPLING))
    assert not torch.equal(eager, _stack(vocab).generate(prompt, n, **dict(SAMPLING, seed=[5, 6])))
    inside = _stack(vocab)
    inside.capture(sample=True)
    behind = _stack(vocab)
    behind.capture()
    assert inside._graph_samples and not behind._graph_samples
    if inside._five_launch():
        assert inside.graph_nodes == behind.graph_nodes + 1
    assert torch.equal(inside.generate(prompt, n, **SAMPLING), eager)
    assert torch.equal(behind.generate(prompt, n, **SAMPLING), eager)
    # the captured sampler reads its parameters when it is replayed: other seeds, no new capture
    assert torch.equal(inside.generate(prompt, n, **dict(SAMPLING, seed=[5, 6])), _stack(vocab).generate(prompt, n, **dict(SAMPLING, seed=[5, 6])))
    # every token is the definition's, on the logits decode() returned for its step
    by_hand = _stack(vocab)
    by_hand.set_sampling(**SAMPLING)
    logits = by_hand.prefill(prompt)
    for i in range(n):
        ctr = [prompt.shape[1] + i] * 2
        tok = (by_hand.sample(logits, ctr[0], 0) if i == 0 else by_hand.sample(logits, by_hand.pos, 1)).clone()
        assert torch.equal(tok, eager[:, i]), i
        _tokens_obey_the_definition(by_hand, logits, ctr, tok, SAMPLING)
        logits = by_hand.decode(tok, prompt.shape[1] + i)


@pytest.mark.usefixtures("reference_numerics")
def test_top_k_1_is_greedy_where_the_maximum_is_unique():
    """The maximum of a 16-bit logits row can be tied; torch's argmax then promises no particular index.  So: the first of a few weight
    seeds whose greedy run has a unique maximum in every row of every step (asserted on the logits), and on it top_k = 1 and temperature 0
    are the greedy generate."""
    vocab, n = 1003, 5
    prompt = _prompt(vocab, seed=4)
    for weights in range(3, 13):
        probe = _stack(vocab, weights=weights)
        logits, greedy, unique = probe.prefill(prompt), [], True
        for i in range(n):
            top2 = logits.float().topk(2, dim=1).values
            unique = unique and bool((top2[:, 0] > top2[:, 1]).all())
            greedy.append(logits.argmax(-1))
            logits = probe.decode(greedy[-1], prompt.shape[1] + i)
        if unique:
            break
    assert unique, "no weight seed in 3 ... 12 without a tied maximum"
    greedy = torch.stack(greedy, 1)
    assert torch.equal(_stack(vocab, weights=weights).generate(prompt, n), greedy)
    assert torch.equal(_stack(vocab, weights=weights).generate(prompt, n, temperature=1.5, top_k=1, seed=3), greedy)
    assert torch.equal(_stack(vocab, weights=weights).generate(prompt, n, temperature=0.0), greedy)


@pytest.mark.usefixtures("reference_numerics")
@pytest.mark.parametrize("cache", ["16-bit", "paged-mx8"])
def test_ragged_generate_with_eos(cache):
    vocab, n = 1003, 8
    kw = dict(ragged=True) if cache == "16-bit" else dict(ragged=True, kv_cache="mx8", kv_pages=4, page_size=64)
    g = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, vocab, (t,), generator=g).to(DEV) for t in (7, 3)]
    free = _stack(vocab, **kw).generate(prompts, n, **SAMPLING)
    assert ((free >= 0) & (free < vocab)).all()
    assert torch.equal(free, _stack(vocab, **kw).generate(prompts, n, **SAMPLING))
    # eos: a token that sequence 1 emits for the first time at step j and sequence 0 never does -> sequence 1 stops there
    rows = free.tolist()
    j = next(j for j in range(1, n - 1) if rows[1][j] not in rows[1][:j] and rows[1][j] not in rows[0])
    eos = rows[1][j]
    captured = _stack(vocab, **kw)
    captured.capture(sample=True)
    outs = [stack.generate(prompts, n, eos=eos, **SAMPLING) for stack in (_stack(vocab, **kw), captured)]
    assert torch.equal(outs[0], outs[1])
    assert outs[0][1].tolist() == rows[1][: j + 1] + [eos] * (n - j - 1)
    assert ((outs[0][0] >= 0) & (outs[0][0] < vocab)).all() and outs[0][0, : j + 1].tolist() == rows[0][: j + 1]
    # the definition, step by step, with a sequence going inactive
    by_hand = _stack(vocab, **kw)
    by_hand.set_sampling(**SAMPLING)
    padded = torch.zeros(2, 7, dtype=torch.long, device=DEV)
    padded[0], padded[1, :3] = prompts[0], prompts[1]
    logits = by_hand.prefill(padded, position=0, lengths=[7, 3])
    tok = by_hand.sample(logits, torch.tensor([7, 3], device=DEV), 0).clone()
    _tokens_obey_the_definition(by_hand, logits, [7, 3], tok, SAMPLING)
    assert torch.equal(tok, free[:, 0])
    logits = by_hand.decode(tok, [7, 3])
    tok = by_hand.sample(logits, by_hand.pos_seq, 1).clone()
    _tokens_obey_the_definition(by_hand, logits, [8, 4], tok, SAMPLING)
    assert torch.equal(tok, free[:, 1])
    logits = by_hand.decode(torch.stack((tok[0], tok[1] * 0)), [8, -1])
    tok = by_hand.sample(logits, by_hand.pos_seq, 1).clone()
    _tokens_obey_the_definition(by_hand, logits, [9, -1], tok, SAMPLING)
    assert tok[1].item() == -1
