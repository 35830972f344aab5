"""GPU suite: the one-shot peer-write gather (include/peer_gather_hip.h, any4_amd.shard.PeerWriteGather).

SURVEY.md 8(e): rank r of G owns weight rows [r n/G, (r+1) n/G) and all ranks need y[m, n] after the GEMM.  The GPU boxes of this
build have ONE GPU, so the test runs two processes (two ranks) on the same device: the buffers still cross a process boundary
as IPC handles, every store is a peer store into memory the other process allocated, and the flags are polled by a kernel that
is already running -- only the xGMI hop itself is missing.
"""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu


def _place(rank, one_gpu_per_rank):
    """Device index of a rank: its own GPU when the box has one per rank (the xGMI hop, uncached cross-device stores and RCCL are
    then really exercised), else GPU 0 for every rank (one-GPU boxes)."""
    return rank if one_gpu_per_rank else 0


PLACEMENTS = [pytest.param(False, id="same_device"),
              pytest.param(True, id="one_gpu_per_rank",
                           marks=pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (runs unattended on a multi-GPU box)"))]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _expected(rank, call, m, cols, dtype):
    g = torch.Generator().manual_seed(1000 * call + rank)
    return torch.randn(m, cols, generator=g).to(dtype)


def _worker(rank, world, port, cols, m_max, calls, dtype_name, multi):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = _place(rank, multi)
    torch.cuda.set_device(dev)
    dtype = getattr(torch, dtype_name)
    from any4_amd.shard import PeerWriteGather

    pg = PeerWriteGather(m_max, cols, device=f"cuda:{dev}", dtype=dtype, timeout_us=5_000_000)
    try:
        for call in range(calls):
            m = 1 + call % m_max
            y_local = _expected(rank, call, m, cols, dtype).cuda()
            out = pg.gather(y_local)
            want = torch.cat([_expected(r, call, m, cols, dtype) for r in range(world)], dim=1)
            # the consumer runs on the same stream, behind the gather kernel
            got = out.clone()
            torch.cuda.synchronize()
            assert got.shape == (m, world * cols)
            assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), f"rank {rank} call {call}: gathered rows differ"
        pg.check()
    finally:
        pg.close()
        dist.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("multi", PLACEMENTS)
@pytest.mark.parametrize("cols,m_max,dtype_name", [(2048, 8, "bfloat16"), (512, 16, "float16")])
def test_peer_write_gather_two_processes(cols, m_max, dtype_name, multi):
    import torch.multiprocessing as mp

    mp.spawn(_worker, args=(2, _free_port(), cols, m_max, 24, dtype_name, multi), nprocs=2, join=True)


def _linear_worker(rank, world, port, multi, gather="peer"):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev = _place(rank, multi)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl" if gather == "rccl" else "gloo", rank=rank, world_size=world)
    DEVN = f"cuda:{dev}"
    import tinygemm  # noqa: F401
    from any4_amd.shard import build_row_sharded_any4

    n, k, g = 256, 512, 128
    gen = torch.Generator().manual_seed(5)
    codes = torch.randint(0, 16, (n, k), dtype=torch.int32, generator=gen)
    lut = torch.randn(n, 16, generator=gen).bfloat16()
    sz = torch.stack([torch.rand(k // g, n, generator=gen) * 0.02 + 0.005, torch.randn(k // g, n, generator=gen) * 0.01], dim=2).bfloat16()
    full = build_row_sharded_any4(codes, lut, sz, None, g, 0, 1, DEVN, torch.bfloat16)  # world 1: the unsharded layer
    shard = build_row_sharded_any4(codes, lut, sz, None, g, rank, world, DEVN, torch.bfloat16)
    shard.gather = gather
    try:
        for m in (1, 3, 8):
            x = torch.randn(m, k, generator=gen).bfloat16().to(DEVN)
            y = shard(x)  # (a copy by default: RowShardedLinear.alias_output=False)
            y_ref = full.local(x)
            torch.cuda.synchronize()
            assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16)), f"rank {rank} m={m}"
        if shard._peer is not None:
            shard._peer.check()
    finally:
        if shard._peer is not None:
            shard._peer.close()
        dist.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("multi", PLACEMENTS)
def test_row_sharded_any4_linear_with_peer_gather(multi):
    """Two ranks, each with half the weight rows of an Any4Linear, gather through PeerWriteGather: bit-equal to the unsharded layer."""
    import torch.multiprocessing as mp

    mp.spawn(_linear_worker, args=(2, _free_port(), multi), nprocs=2, join=True)


@pytest.mark.timeout(240)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one GPU per rank (runs unattended on a multi-GPU box)")
def test_row_sharded_any4_linear_with_rccl_all_gather():
    """The same layer with the exchange SURVEY 8(e) names first: RCCL all_gather_into_tensor over xGMI, one process per GPU."""
    import torch.multiprocessing as mp

    mp.spawn(_linear_worker, args=(2, _free_port(), True, "rccl"), nprocs=2, join=True)


def _decode_worker(rank, world, port, results, multi):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = _place(rank, multi)
    torch.cuda.set_device(dev)
    DEVN = f"cuda:{dev}"
    from any4_amd.decode import DecodeConfig, DecodeStack, shard_rows

    cfg = DecodeConfig(hidden=256, inter=512, layers=2, heads=4, kv_heads=2, head_dim=64, vocab=128, max_seq=32, group_size=128)

    def factory(r, w):
        def make(name, layer, in_features, rows):
            full_rows = {n: o for n, o, _ in cfg.linear_shapes()}[name]
            gen = torch.Generator().manual_seed(1000 * layer + sum(map(ord, name)))
            wt = torch.randn(full_rows, in_features, generator=gen) / in_features ** 0.5
            lin = torch.nn.Linear(in_features, rows, bias=False, device=DEVN, dtype=torch.bfloat16)
            lin.weight.data = wt[shard_rows(cfg, name, r, w)].contiguous().to(DEVN, torch.bfloat16)
            return lin
        return make

    toks = torch.randint(0, cfg.vocab, (5, 2), generator=torch.Generator().manual_seed(3)).to(DEVN)
    try:
        full = DecodeStack(cfg, factory(0, 1), DEVN, torch.bfloat16, bs=2, seed=7)
        tp = DecodeStack(cfg, factory(rank, world), DEVN, torch.bfloat16, bs=2, rank=rank, world=world, seed=7, gather="peer")
        ref = torch.stack([full.decode(t, i).float().clone() for i, t in enumerate(toks)])
        eager = torch.stack([tp.decode(t, i).float().clone() for i, t in enumerate(toks)])
        # ... and the same steps replayed from one captured hipGraph (the gather kernels keep their sequence number on the device)
        tp.capture()
        graph = torch.stack([tp.decode(t, i).float().clone() for i, t in enumerate(toks)])
        torch.cuda.synchronize()
        for pg in tp._peer.values():
            pg.check()
        scale = float(ref.abs().max())
        results[rank] = (float((eager - ref).abs().max()) / scale, float((graph - eager).abs().max()) / scale,
                         sorted(pg._calls for pg in tp._peer.values()))
    finally:
        for pg in tp._peer.values():
            pg.close()
        dist.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("multi", PLACEMENTS)
def test_tensor_parallel_decode_with_peer_gather(multi):
    """TP = 2 decode stack (heads / rows split, 4 exchanges per layer through PeerWriteGather, HIP glue kernels) against the
    unsharded stack, eager and replayed from a hipGraph; both ranks live on the one GPU of the box."""
    import torch.multiprocessing as mp

    results = mp.Manager().dict()
    mp.spawn(_decode_worker, args=(2, _free_port(), results, multi), nprocs=2, join=True)
    assert set(results.keys()) == {0, 1}
    for rank, (err_eager, err_graph, calls) in results.items():
        assert err_eager < 3e-2, (rank, err_eager)   # bf16 GEMMs of different shapes (row shards) and summation orders
        assert err_graph < 3e-2, (rank, err_graph)
        assert all(c % 2 == 0 for c in calls), calls  # every gather object ended on an even number of calls


@pytest.mark.timeout(120)
@pytest.mark.parametrize("world", [4, 8])
def test_peer_write_gather_fan_out_addressing(world):
    """Fan-out > 1 peer on a one-GPU box.  Several waiting kernels only make progress together if the GPU runs them concurrently,
    which it does for two processes but not reliably for four (measured: the four-process variant of the test above times out on
    some boxes).  So the `world` ranks' kernels run one after the other in THIS process, each finding its peers' flags already
    raised for the call (set from the host): what is checked is everything that changes with the fan-out -- the world - 1 peer
    stores land in the right column blocks of the right buffers, every flags[peer][rank] word is raised to the call's sequence
    number, the two-buffer alternation -- while the waiting itself is covered by the two-process tests."""
    import ctypes

    from any4_amd import _lib
    from any4_amd.shard import _DeviceBytes

    L = _lib.load()
    cols, m, calls = 512, 3, 5
    buf_bytes = m * cols * world * 2
    data, ctl = [], []
    for r in range(world):
        p, c = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.tg_peer_alloc(0, 2 * buf_bytes, ctypes.byref(p)), "tg_peer_alloc")
        _lib.check(L.tg_peer_alloc(0, 256, ctypes.byref(c)), "tg_peer_alloc")
        data.append(p.value)
        ctl.append(c.value)
    view = lambda ptr, n, dt: torch.as_tensor(_DeviceBytes(ptr, n), device="cuda:0").view(dt)  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    try:
        for call in range(calls):
            parity = call & 1
            srcs = [_expected(r, call, m, cols, torch.bfloat16).cuda() for r in range(world)]
            for r in range(world):  # "the peers have arrived": flags[r][*] ahead of this call's sequence number; buffers cleared
                view(ctl[r], 64, torch.int32).fill_(call + 1000)
                view(data[r] + parity * buf_bytes, buf_bytes, torch.int16).fill_(-1)
            for r in range(world):
                a = _lib.PeerGather()
                for q in range(world):
                    a.dst[q] = data[q] + parity * buf_bytes
                    a.flags[q] = ctl[q]
                a.seq, a.status = ctl[r] + 64, ctl[r] + 128
                a.world, a.rank, a.cols_local, a.timeout_us = world, r, cols, 2_000_000
                a.src, a.m = srcs[r].data_ptr(), m
                _lib.check(L.tg_peer_gather_launch(ctypes.byref(a), 0, st), "tg_peer_gather_launch")
            torch.cuda.synchronize()
            want = torch.cat([_expected(r, call, m, cols, torch.bfloat16) for r in range(world)], dim=1)
            for r in range(world):
                got = view(data[r] + parity * buf_bytes, buf_bytes, torch.bfloat16).view(m, world * cols)
                assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), (call, r)
                other = view(data[r] + (1 - parity) * buf_bytes, buf_bytes, torch.int16)
                assert call == 0 or not bool((other == -1).all()), "the other buffer still holds the previous call"
                assert int(view(ctl[r] + 128, 4, torch.int32).item()) == 0, (call, r)
                assert view(ctl[r] + 64, 64, torch.int32)[:world].tolist() == [call + 1] * world  # every workgroup counted the call
                # every rank's launch wrote its flag word here: the host's "ahead" values are all replaced by the sequence number
                assert view(ctl[r], 64, torch.int32)[:world].tolist() == [call + 1] * world
    finally:
        torch.cuda.synchronize()
        for p in data + ctl:
            L.tg_peer_free(0, p)


def _absent_peer_worker(rank, world, port, results):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from any4_amd.shard import PeerWriteGather

    cols, m = 256, 2
    pg = PeerWriteGather(4, cols, device="cuda:0", dtype=torch.bfloat16, timeout_us=300_000)
    try:
        # call 0: both ranks take part
        out = pg.gather(torch.full((m, cols), float(rank + 1), dtype=torch.bfloat16, device="cuda:0")).clone()
        torch.cuda.synchronize()
        assert torch.equal(out[:, :cols].float().cpu(), torch.full((m, cols), 1.0)) and torch.equal(out[:, cols:].float().cpu(), torch.full((m, cols), 2.0))
        pg.check()
        dist.barrier()
        if rank == 0:
            # call 1: rank 1 never arrives -> the wait ends after the timeout, *status is set, rank 1's slice is NaN
            import time

            t0 = time.perf_counter()
            out = pg.gather(torch.full((m, cols), 5.0, dtype=torch.bfloat16, device="cuda:0")).clone()
            torch.cuda.synchronize()
            waited = time.perf_counter() - t0
            own_ok = bool((out[:, :cols].float() == 5.0).all())
            peer_nan = bool(torch.isnan(out[:, cols:].float()).all())
            raised_check = raised_poll = False
            try:
                pg.check()
            except RuntimeError:
                raised_check = True
            try:  # poll(): the first call queues the read-back, a later one sees it
                for _ in range(50):
                    pg.poll()
                    torch.cuda.synchronize()
            except RuntimeError:
                raised_poll = True
            results[0] = (waited, own_ok, peer_nan, raised_check, raised_poll)
        dist.barrier()
    finally:
        pg.close()
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_peer_that_never_arrives_sets_status_and_poisons_its_slice():
    import torch.multiprocessing as mp

    results = mp.Manager().dict()
    mp.spawn(_absent_peer_worker, args=(2, _free_port(), results), nprocs=2, join=True)
    waited, own_ok, peer_nan, raised_check, raised_poll = results[0]
    assert 0.25 < waited < 5.0, waited          # bounded by timeout_us = 0.3 s, never a hang
    assert own_ok and peer_nan                  # own slice intact, the missing slice is NaN (loud)
    assert raised_check and raised_poll         # both the synchronising and the non-blocking check report it


def _run_bench_two_ranks(backend, extra=(), timeout=420):
    """`python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2 ...` exactly as the driver launches it, with both ranks on
    GPU 0 (--same-device) when the box has one GPU.  Returns (returncode, parsed JSON line or None, tail of the output)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    multi = torch.cuda.device_count() >= 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "4", "--warmup", "2",
           "--layers", "64", "--settle-s", "0", "--no-pmc", "--no-decode", "--no-cpu-baseline", "--dist-backend", backend,
           *([] if multi else ["--same-device"]), *extra]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    try:
        r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        return -9, None, f"timeout: {(e.stdout or b'')[-2000:]!r} {(e.stderr or b'')[-2000:]!r}"
    line = None
    for ln in r.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = json.loads(ln)
    return r.returncode, line, (r.stdout[-1500:] + "\n" + r.stderr[-3000:])


def test_bench_strong_scaling_leg_two_ranks(tmp_path):
    """SURVEY.md 8(e) / north_star: `bench.py --gpus 2` partitions ONE stack of n = 4096 layers into rows [r n/2, (r+1) n/2) per rank,
    gathers the layer batch's outputs once per step and reports the WHOLE problem's GB/s ("scaling": "strong") with the per-rank
    roofline fraction, the weak-scaling protocol as an extra key and the decode-shaped (latency) exchange.  Two ranks: on two GPUs over
    RCCL where the box has them; on a one-GPU box RCCL is tried first (it refuses two ranks on one device) and the same code path then
    runs with the gloo control plane and the peer-write gather over IPC -- so the first run on a real node is not the first run of this
    code."""
    dump = ("--dump-outputs", str(tmp_path))
    rc, line, tail = _run_bench_two_ranks("nccl", dump, timeout=420 if torch.cuda.device_count() >= 2 else 150)
    used = "nccl"
    if rc != 0 or line is None:
        assert torch.cuda.device_count() < 2, f"RCCL run failed on a multi-GPU box:\n{tail}"
        rc, line, tail = _run_bench_two_ranks("gloo", dump)
        used = "gloo"
    assert rc == 0 and line is not None, tail
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["unit"] == "GB/s" and line["value"] > 0
    cfg = line["config"]
    assert cfg["n"] == 4096 and cfg["rows_per_rank"] == 2048 and cfg["layers_per_step"] == 64
    assert cfg["exchange"] == ("rccl_all_gather_into_tensor" if used == "nccl" else "peer_write_gather")
    assert cfg["algorithmic_bytes_per_layer"] == 9060352
    ss, ws = line["strong_scaling"], line["weak_scaling"]
    assert ss["rows_per_rank"] == 2048 and 0 < ss["per_rank_roofline_frac"] < 1 and ss["ms_per_step_no_exchange"] > 0
    assert ws["scaling"] == "weak" and ws["value"] > 0
    # the whole problem's rate from the line's own numbers
    assert abs(line["value"] - 64 * 9060352 / (line["ms_per_step"] * 1e-3) / 1e9) <= 0.02 * line["value"]
    assert line["numerics_check"]["max_abs_err_vs_reference"] <= 1e-2          # rank 0's shard of the timed launch against the oracle
    ex = line["decode_shaped_exchange"]
    assert ex["us_per_layer_gemv_only"] > 0 and ("us_per_layer_gemv_plus_peer_write_gather" in ex or "peer_write_gather_error" in ex)
    if used == "nccl":
        assert ex["us_per_layer_gemv_plus_rccl_all_gather"] > 0
    # --dump-outputs: the gathered output of the whole problem (both ranks' rows), as a caller of the sharded layer batch receives it
    import numpy as np

    assert line["dumped_outputs"] == {"y.npy": [64, 1, 4096]}
    y = np.load(tmp_path / "y.npy")
    assert y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y[..., :2048]).max() > 0 and np.abs(y[..., 2048:]).max() > 0
    print(f"bench.py --gpus 2 ran with backend {used}: value {line['value']} GB/s, per-rank frac {ss['per_rank_roofline_frac']}")
