#!/usr/bin/env python
"""What does a column map cost beside the flow diagnostics?  (DESIGN.md, section on the column maps)

On the benchmark's flagship workload (1,747,584 fluid particles), settled by `--settle` steps, in ONE process and on one
state: HIP events on the context's stream around `--inner` calls enqueued back to back of
  (a) sph_columns_reduce, axis = 1 at the default cell (the support radius): clear + scatter + finish;
  (b) sph_diag_reduce (its aux record already folded): the yardstick -- it streams twice the bytes and uses no atomic.
Repetitions alternate (a) and (b) so that drift hits both alike; medians with min / max, the ratio of the medians, the map
size, and the map pass's effective bandwidth (32 bytes per particle over its time).  `--cell` / `--axis` time other maps.
A run without a GPU fails; nothing is estimated.

    python tools/columns_timing.py --out profiles/columns_timing.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench        # noqa: E402  (scene dictionaries of the benchmark's workloads)
from sph_taichi_amd import ParticleSystem, _lib, columns  # noqa: E402
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
    ap.add_argument("--inner", type=int, default=20, help="calls per event pair")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--axis", type=int, default=1)
    ap.add_argument("--cell", type=float, default=None, help="default: the support radius")
    args = ap.parse_args()

    hip = hip_runtime()
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    ps = ParticleSystem(SimConfig(config=bench.scene_dict(args.workload)), stream=stream.value)
    solver = ps.build_solver()
    solver.initialize()
    solver.step(args.settle)
    n = int(ps.particle_max_num)

    axis, cell, origin, shape, oid = columns.map_params(ps, axis=args.axis, cell=args.cell)
    p = _lib.SphColumnParams()
    p.axis, p.object_id = axis, oid
    p.n = (C.c_int32 * 2)(*shape)
    p.origin = (C.c_float * 2)(*[float(np.float32(o)) for o in origin])
    p.inv_cell = (C.c_float * 2)(*[float(v) for v in columns.inv_cell_f32(cell)])

    def events(fn):
        ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        for _ in range(args.inner):
            fn()
        ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value) / args.inner

    reduce_map = lambda: ps._call("sph_columns_reduce", C.byref(p))
    reduce_diag = lambda: ps._call("sph_diag_reduce")
    for _ in range(3):                      # warm-up: allocations, the fold of the aux record, clocks
        reduce_map(); reduce_diag()
    ps.sync()
    cm = ps.column_map(axis=axis, cell=cell)
    assert cm.selected == n == cm.binned + cm.outside, (cm.selected, cm.binned, cm.outside, n)

    t_map, t_diag = [], []
    for _ in range(args.reps):
        t_map.append(events(reduce_map))
        t_diag.append(events(reduce_diag))
    a, b = stats(t_map), stats(t_diag)
    wet = int(cm.wet.sum())
    out = {
        "workload": args.workload, "particles": n, "settle_steps": args.settle, "axis": axis, "cell": list(cell),
        "map_shape": list(shape), "map_columns": shape[0] * shape[1], "wet_columns": wet,
        "particles_per_wet_column": round(n / max(wet, 1), 1), "outside": cm.outside,
        "method": f"{args.reps} repetitions, alternating, {args.inner} calls per HIP-event pair on the context's stream, after "
                  f"{args.settle} settling steps and 3 warm-up rounds",
        "columns_reduce_events": a, "diag_reduce_events": b,
        "columns_over_diag": round(a["median_ms"] / b["median_ms"], 3),
        "columns_bytes_read_per_particle": 32,
        "columns_effective_bandwidth_GBps": round(32.0 * n / (a["median_ms"] * 1e-3) / 1e9, 1),
        "diag_effective_bandwidth_GBps": round(64.0 * n / (b["median_ms"] * 1e-3) / 1e9, 1),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ps.close()


if __name__ == "__main__":
    main()
