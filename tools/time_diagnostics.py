#!/usr/bin/env python
"""What do the flow diagnostics cost beside a step, and beside doing without them?  (profiles/diag_timing.json)

On the benchmark's flagship workload (1,747,584 fluid particles), settled by `--settle` steps, in ONE process:
  (a) sph_diag_reduce (+ sph_diag_download): HIP events on the context's stream around `--inner` reductions enqueued back
      to back (the kernels alone, the aux record already folded), HIP events around ONE reduction right behind a step (what
      a controller pays: the fold of density / pressure out of the fused step's record comes with it), and the host clock
      around reduce + download (ends in a synchronise);
  (b) what a user does without them for the four maxima of the reference's older engine: four `to_numpy()` downloads
      (v, acceleration, density, pressure) and the numpy reductions, by the host clock;
  (c) one solver step: the host clock around `--steps` steps ending in a synchronise, per step, and around a single step.
Repetitions alternate (a), (b), (c) so that drift hits all alike; medians with min / max.  The effective bandwidth of (a) is
its 64 bytes per particle over the event time of the kernels alone.  A run without a GPU fails; nothing is estimated.

    python tools/time_diagnostics.py --out profiles/diag_timing.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench        # noqa: E402  (scene dictionaries of the benchmark's workloads)
from sph_taichi_amd import ParticleSystem, _lib, diagnostics  # noqa: E402
from sph_taichi_amd.config_builder import SimConfig  # noqa: E402


def hip_runtime():
    """The HIP runtime this process has already mapped (the one libsph_hip.so runs on), for streams and events."""
    _lib.load()
    with open("/proc/self/maps") as fh:
        paths = {line.split()[-1] for line in fh if "libamdhip64" in line}
    if not paths:
        raise RuntimeError("no libamdhip64 mapped")
    hip = C.CDLL(sorted(paths)[0])
    for name, args in (("hipStreamCreate", [C.POINTER(C.c_void_p)]), ("hipEventCreate", [C.POINTER(C.c_void_p)]),
                       ("hipEventRecord", [C.c_void_p, C.c_void_p]), ("hipEventSynchronize", [C.c_void_p]),
                       ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p])):
        getattr(hip, name).argtypes, getattr(hip, name).restype = args, C.c_int
    return hip


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: hipError {rc}")


def stats(samples):
    v = sorted(samples)
    return {"median_ms": round(statistics.median(v), 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5), "repetitions": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", default="c3p_uniform_1.75M")
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--inner", type=int, default=20, help="reductions per event pair")
    ap.add_argument("--steps", type=int, default=20, help="steps per timed block")
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()

    hip = hip_runtime()
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    sd = bench.scene_dict(args.workload)
    ps = ParticleSystem(SimConfig(config=sd), stream=stream.value)
    solver = ps.build_solver()
    solver.initialize()
    solver.step(args.settle)
    n = int(ps.particle_max_num)
    n_rows = int(ps._params.n_objects) + 1
    rows = (_lib.SphDiagRow * n_rows)()

    def events(fn):
        ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        fn()
        ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value)

    def wall(fn):
        ps.sync()
        t = time.perf_counter()
        fn()
        ps.sync()
        return (time.perf_counter() - t) * 1e3

    def reduce_and_download():
        ps._call("sph_diag_reduce")
        ps._call("sph_diag_download", rows, n_rows)

    def by_hand():
        v, a = ps.v.to_numpy(), ps.acceleration.to_numpy()
        rho, p = ps.density.to_numpy(), ps.pressure.to_numpy()
        return (np.sqrt((v.astype(np.float64) ** 2).sum(axis=1).max()), np.sqrt((a.astype(np.float64) ** 2).sum(axis=1).max()),
                rho.max(), p.max())

    # warm-up of every shape the timed window uses
    for _ in range(3):
        reduce_and_download(); by_hand(); solver.step(2)
    d = diagnostics.reduce(ps)
    hand = by_hand()
    assert abs(d.total.v_max - hand[0]) <= 1e-12 * hand[0] and d.total.density_max == float(hand[2]), (d.total.as_dict(), hand)

    t_kernels, t_behind_step, t_call, t_hand, t_step, t_step1 = [], [], [], [], [], []
    for _ in range(args.reps):
        solver.step(1)                        # the aux record is in the fused step's lean form again
        t_behind_step.append(events(lambda: ps._call("sph_diag_reduce")))
        t_kernels.append(events(lambda: [ps._call("sph_diag_reduce") for _ in range(args.inner)]) / args.inner)
        t_call.append(wall(reduce_and_download))
        t_hand.append(wall(by_hand))
        t_step.append(wall(lambda: solver.step(args.steps)) / args.steps)
        t_step1.append(wall(lambda: solver.step(1)))

    a = stats(t_kernels)
    out = {
        "workload": args.workload, "particles": n, "rows": n_rows, "settle_steps": args.settle,
        "method": f"{args.reps} repetitions, alternating, after {args.settle} settling steps and 3 warm-up rounds; events = HIP events on the "
                  f"context's stream ({args.inner} reductions per pair for the kernels alone), wall = host clock around work that ends in a synchronise",
        "a_reduce_kernels_events": a,
        "a_reduce_behind_a_step_events": stats(t_behind_step),
        "a_reduce_and_download_wall": stats(t_call),
        "b_four_downloads_and_numpy_wall": stats(t_hand),
        "c_step_wall_per_step": stats(t_step),
        "c_single_step_wall": stats(t_step1),
        "bytes_read_per_particle": 64,
        "a_effective_bandwidth_GBps": round(64.0 * n / (a["median_ms"] * 1e-3) / 1e9, 1),
    }
    out["a_over_c"] = round(out["a_reduce_behind_a_step_events"]["median_ms"] / out["c_step_wall_per_step"]["median_ms"], 4)
    out["b_over_a"] = round(out["b_four_downloads_and_numpy_wall"]["median_ms"] / out["a_reduce_and_download_wall"]["median_ms"], 1)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ps.close()


if __name__ == "__main__":
    main()
