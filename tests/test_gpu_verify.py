"""GPU suite: dg_verify_attn (decode_ops.verify_attn), the split-KV attention of the speculative-decoding verify pass, on the launches,
float64 references and lookup / decoy probes of tests/glue_ref.py and with the checks of tests/test_gpu_ragged_f64.py, unchanged:

  lookup   each existing output row is BIT-equal to the V row its query points at (own position, own - 1, 0, the edges of a 64-position tile ...)
  decoy / peaked   e = max_d |got - ref64| / max_d |ref64| <= 2 max(e of the 16-bit torch formulation on that sequence, 2u)
  caches   bit-equal to the expected ones: the appended rows and every other byte (NaN tails, slots nobody named)
  rows that do not exist keep the caller's sentinel
  prefill  prefill_attn(lengths=, slots=) on the same launch: caches bit-equal, outputs within the same bound of each other

Positions are chosen at max_seq 1024 around the kernel's regimes: 0 (the chunk tile alone), 1, 63, 64, 65 (a second tile), 255, 256, 257 (one
tile per wave, then a fifth), 700; nsplit 1 / 2 / 3 / 5 leaves slices empty at the short ones."""
import pytest
import torch

from tests import glue_ref as R
from tests.test_gpu_glue_f64 import DTYPES
from tests.test_gpu_ragged_f64 import DEV, _args, _geo, _prefill_seq, _sentinel, allowances, check_caches, check_outputs

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("reference_numerics")]
POSITION_SETS = ([0, 1, 63], [64, 65, 255], [256, 257, 700])
SPLITS = (1, 2, 3, 5)
# (hl, kvl, d), T: one 16-row unit exactly; 24 rows of a group of 3; two workgroups per kv head, 20 rows; a decode step; 8 rows; 32 rows, 8 kv heads
SHAPES = [((4, 1, 128), 4), ((3, 1, 128), 8), ((8, 1, 64), 5), ((2, 2, 64), 1), ((4, 1, 128), 2), ((32, 8, 128), 8)]


def _verify(rc, nsplit, scratch=None, out=None):
    from any4_amd import decode_ops as G

    kc, vc, out = rc.kc0.clone(), rc.vc0.clone(), _sentinel(rc) if out is None else out
    if scratch is None:
        scratch = G.verify_attn_scratch(rc.n, rc.hl, rc.d, rc.T, nsplit, DEV)
    G.verify_attn(*_args(rc), kc, vc, *_geo(rc), rc.T, nsplit, scratch, out=out, lengths=rc.lengths, slots=rc.slots)
    return out, kc, vc


def _check(rc, splits):
    """Every check of the module docstring on one launch, at every split count."""
    allow = allowances(rc)
    pre, pkc, pvc = _prefill_seq(rc)
    for ns in splits:
        label = f"verify_attn/{ns}"
        out, kc, vc = _verify(rc, ns)
        check_caches(rc, kc, vc, label)
        assert R.same_bits(kc, pkc) and R.same_bits(vc, pvc), f"{label}: caches differ from prefill_attn's"
        check_outputs(rc, out, label, allow)
        o, p = out.view(rc.n, rc.T, rc.hl, rc.d), pre.view(rc.n, rc.T, rc.hl, rc.d)
        for i, c in enumerate(rc.seqs):
            if c is not None and rc.kind != "lookup":
                e = R.row_err(o[i:i + 1, :c.T], p[i:i + 1, :c.T].double()).max().item()
                assert e <= allow[i][0], f"{label} sequence {i}: {e:.3e} from prefill_attn, {allow[i][0]:.3e} allowed"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom,T", SHAPES)
def test_verify_attn_probes_and_float64(dtype, geom, T):
    sets = POSITION_SETS[1:2] if geom[0] == 32 else POSITION_SETS   # (the large geometry once)
    for positions in sets:
        for kind in ("lookup", "decoy", "peaked"):
            rc = R.ragged_prefill_case(kind, dtype, geom, [(T, p) for p in positions], list(range(3)), 3, 1024)
            _check(rc.to(DEV), SPLITS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["lookup", "peaked"])
def test_verify_attn_lengths_slots_and_cache_end(dtype, kind):
    """Lengths [T, 0, 3] in slots [2, 0, 1] of a cache of 4 (slot 3 is nobody's), and a sequence whose chunk of 5 runs past max_seq: its
    tokens at 1024, 1025 do not exist -- no cache row, no output row, nothing indexed."""
    T, S, geom = 5, 1024, (4, 1, 128)
    rc = R.ragged_prefill_case(kind, dtype, geom, [(T, 300), None, (3, 64)], [2, -1, 1], 4, S)
    rc.slots[1] = 0                                    # a named slot with length 0: a no-op
    _check(rc.to(DEV), SPLITS)
    rc = R.ragged_prefill_case(kind, dtype, geom, [(3, S - 3), (T, 129)], [1, 0], 2, S)
    rc.lengths[0] = T                                  # two more tokens than the cache has rows for
    _check(rc.to(DEV), (1, 3))


@pytest.mark.parametrize("dtype", DTYPES)
def test_verify_attn_at_the_end_of_8192_positions(dtype):
    rc = R.ragged_prefill_case("lookup", dtype, (32, 8, 128), [(8, 8192 - 8)], [0], 1, 8192).to(DEV)
    _check(rc, (8,))


@pytest.mark.parametrize("dtype", DTYPES)
def test_verify_attn_repeats_its_bits_and_replays_in_a_graph(dtype):
    """Two calls through one scratch and three replays of a captured launch give the bits of the first call."""
    from any4_amd import decode_ops as G

    rc = R.ragged_prefill_case("peaked", dtype, (8, 1, 64), [(5, 700), (5, 257), (2, 0)], [0, 1, 2], 3, 1024).to(DEV)
    scratch = G.verify_attn_scratch(rc.n, rc.hl, rc.d, rc.T, 3, DEV)
    first = _verify(rc, 3, scratch)[0]
    assert R.same_bits(_verify(rc, 3, scratch)[0], first)
    out = _sentinel(rc)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _verify(rc, 3, scratch, out)   # (warm-up on the capture stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            _verify(rc, 3, scratch, out)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(3):
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert R.same_bits(out, first)
