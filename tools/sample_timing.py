#!/usr/bin/env python
"""What does field sampling cost?  (DESIGN.md, section on the field sampling)

On the benchmark's flagship workload (1,747,584 fluid particles), settled by `--settle` steps, in ONE process and on one
state: HIP events on the context's stream around `--inner` calls enqueued back to back of
  (a) sph_sample_grid over the whole domain at spacing = the particle diameter, velocity + pressure;
  (b) one slice of that grid (the plane through the middle of the third axis);
  (c) sph_sample_points at 64 probe points spread through the fluid;
the three alternating so that drift hits all alike.  Beside each time: the bytes the pass must read (32 per particle, + 16
when density or pressure is asked) and the bandwidth that makes.  (The side-by-side of the grid kernel's two stages, made
before the LDS-tiled stage was dropped, is profiles/archive/sample_timing_tiled_vs_plain.json; DESIGN_HISTORY.md has the
story.)  A run without a GPU fails; nothing is estimated.

    python tools/sample_timing.py --out profiles/sample_timing.json
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
from sph_taichi_amd import ParticleSystem, _lib, sample  # noqa: E402
from sph_taichi_amd.config_builder import SimConfig  # noqa: E402

FIELDS = ("velocity", "pressure")


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


def stats(samples, bytes_read):
    v = sorted(samples)
    med = statistics.median(v)
    return {"median_ms": round(med, 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5), "repetitions": len(v),
            "bytes_read": bytes_read, "effective_bandwidth_GBps": round(bytes_read / (med * 1e-3) / 1e9, 1)}


def grid_struct(ps, ga, sel):
    g = _lib.SphSampleGrid()
    g.n = (C.c_int32 * 3)(*ga["shape"])
    g.origin, g.spacing = (C.c_float * 3)(*ga["origin"]), (C.c_float * 3)(*ga["spacing"])
    g.inv_h, g.fields, g.select = sample.inv_h_f32(ps.support_radius), sel["mask"], sample.make_select(sel)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", default="c3p_uniform_1.75M")
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--inner", type=int, default=4, help="calls per event pair")
    ap.add_argument("--reps", type=int, default=7)
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

    sel = sample.select_args(fields=FIELDS)
    full = sample.grid_args(particle_diameter=ps.particle_diameter, domain_size=ps.domain_size)
    mid = full["shape"][2] // 2
    cut = {"spacing": full["spacing"], "shape": full["shape"][:2] + (1,),
           "origin": full["origin"][:2] + (float(np.float32(full["origin"][2]) + np.float32(mid) * np.float32(full["spacing"][2])),)}
    g_full, g_cut = grid_struct(ps, full, sel), grid_struct(ps, cut, sel)
    x = ps.x.to_numpy()
    pts = np.ascontiguousarray(x[np.linspace(0, n - 1, 64).astype(np.int64)] + np.float32(0.004), dtype=np.float32)
    psel = sample.make_select(sel)
    inv_h = sample.inv_h_f32(ps.support_radius)

    def events(fn):
        ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        for _ in range(args.inner):
            fn()
        ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value) / args.inner

    call_full = lambda: ps._call("sph_sample_grid", C.byref(g_full))
    call_cut = lambda: ps._call("sph_sample_grid", C.byref(g_cut))
    call_pts = lambda: ps._call("sph_sample_points", pts.ctypes.data_as(C.c_void_p), 64, sel["mask"], C.byref(psel), inv_h)

    for _ in range(2):                          # warm-up: allocations, the fold of the aux record, clocks
        call_full(); call_pts()
    w, c, s = sample.download_grid_raw(ps, g_cut, len(sel["planes"]))
    wet_nodes = int(np.count_nonzero(c))
    assert wet_nodes > 0 and int(c.sum()) > 0

    t = {k: [] for k in ("grid_full", "grid_slice", "points64")}
    for _ in range(args.reps):
        t["grid_full"].append(events(call_full))
        t["grid_slice"].append(events(call_cut))
        t["points64"].append(events(call_pts))
    ps.sync()
    per_particle = 32 + 16                      # xm + vf, + aux because pressure is asked
    out = {
        "workload": args.workload, "particles": n, "settle_steps": args.settle, "fields": list(FIELDS),
        "bytes_read_per_particle": per_particle,
        "grid_shape": list(full["shape"]), "grid_nodes": int(np.prod(full["shape"])), "grid_spacing": list(full["spacing"]),
        "slice_shape": list(cut["shape"]), "slice_origin": list(cut["origin"]), "slice_wet_nodes": wet_nodes,
        "method": f"{args.reps} repetitions, the three cases alternating, {args.inner} calls per HIP-event pair on the context's stream, "
                  f"after {args.settle} settling steps and a warm-up round; each call is clear + scatter",
    }
    for k, v in t.items():
        out[k] = stats(v, per_particle * n)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ps.close()


if __name__ == "__main__":
    main()
