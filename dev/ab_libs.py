"""Same-process A/B of several builds of the library on one stacked tg_gemm_w4 launch: every build is loaded side by side (ctypes), runs on
the SAME operands, and the builds take turns round by round in the sustained state -- so a round of each build sees the same box, the same
clocks and the same data.  The first build is the baseline: its result is checked against the CPU oracle (bench.check_layers), every other
build's result must be the same bits.
    python dev/ab_libs.py [--cfg m,n,k,on_right,qtype,g[,L]] [--rounds 6] [--launches 60] [--hold 3] [--out FILE] NAME=LIB.so [NAME=LIB.so ...]
One round of a build = `--launches` stacked launches between one HIP-event pair.  Prints one line per round and build (us per launch) and
a summary: min / mean / max per build, the baseline's round-to-round spread, and for every other build whether its slowest round beats the
baseline's fastest."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from any4_amd import _lib, ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="1,4096,4096,1,any4_rowwise,128,512")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--hold", type=float, default=3.0)
    ap.add_argument("--out")
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    f = a.cfg.split(",")
    m, n, k, on_right, qtype, g = int(f[0]), int(f[1]), int(f[2]), int(f[3]) == 1, f[4], int(f[5])
    L = int(f[6]) if len(f) > 6 else 512
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    main_lib = _lib.load()
    w, x, q, lut, y = bench.make_batch(L, m, n, k, g, 4, dev, 7, qtype, on_right)
    aa = bench.make_args(_lib, w, x, q, lut, y, m, n, k, g, qtype, on_right, 4, L, "fast")
    ws = bench.attach_workspace(main_lib, aa, dev)  # noqa: F841  (kept alive)
    plan = ops.gemm_w4_plan(m, n, k, g, bench.QT[qtype], on_right, 4, torch.bfloat16, L, "fast", weight_format="reference")

    builds = []
    for spec in a.libs:
        name, path = spec.split("=", 1)
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.tg_gemm_w4.argtypes = _lib.SYMBOLS["tg_gemm_w4"]
        lib.tg_gemm_w4.restype = ctypes.c_int

        def launch(lib=lib, name=name):
            rc = lib.tg_gemm_w4(ctypes.byref(aa), 0, st.cuda_stream)
            if rc != 0:
                raise RuntimeError(f"{name}: tg_gemm_w4 returned {rc}")

        builds.append((name, launch))

    bench.calibrate_x(builds[0][1], x, y)
    say(f"# cfg {a.cfg} plan={plan} rounds={a.rounds} launches/round={a.launches} hold={a.hold}s")
    base = None
    for name, launch in builds:
        y.fill_(float("nan"))
        launch()
        torch.cuda.synchronize()
        if base is None:
            err = bench.check_layers(w, x, q, lut, y, g, qtype, on_right, 4, plan, layers=(0, L // 2, -1), rows=128)
            base = y.clone()
            say(f"# {name}: oracle ok, max|err| vs kernel formula {err['max_abs_err_vs_kernel_formula']:.3e}")
        else:
            same = torch.equal(y.view(torch.int16), base.view(torch.int16))
            say(f"# {name}: output {'bit-identical to' if same else 'DIFFERS from'} {builds[0][0]}")
            if not same:
                raise SystemExit(1)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.hold:
        for name, launch in builds:
            for _ in range(10):
                launch()
        torch.cuda.synchronize()
    times = {name: [] for name, _ in builds}
    for rd in range(a.rounds):
        for name, launch in builds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.launches):
                launch()
            e1.record(st)
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / a.launches * 1e3
            times[name].append(us)
            say(f"round {rd} {name:16s} {us:9.3f} us/launch")
    b0 = times[builds[0][0]]
    spread = max(b0) - min(b0)
    mean0 = sum(b0) / len(b0)
    say(f"# {builds[0][0]:16s} min {min(b0):.3f} mean {mean0:.3f} max {max(b0):.3f}  spread {spread:.3f} us ({spread / mean0 * 100:.2f} %)")
    for name, _ in builds[1:]:
        t = times[name]
        mean = sum(t) / len(t)
        say(f"# {name:16s} min {min(t):.3f} mean {mean:.3f} max {max(t):.3f}  mean gain {mean0 - mean:+.3f} us ({(mean0 - mean) / mean0 * 100:+.2f} %, "
            f"{(mean0 - mean) / spread if spread > 0 else float('inf'):.1f} x baseline spread)  "
            f"slowest round {'beats' if max(t) < min(b0) else 'does NOT beat'} baseline's fastest")


if __name__ == "__main__":
    main()
