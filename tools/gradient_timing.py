#!/usr/bin/env python
"""What do the gradient sums add to field sampling?  (DESIGN.md, section on the field sampling)

The set-up of tools/sample_timing.py -- the benchmark's flagship workload (1,747,584 fluid particles), settled by `--settle`
steps, ONE process, one state, HIP events on the context's stream around `--inner` calls enqueued back to back -- for the
whole-domain grid at spacing = the particle diameter, one slice of it and 64 probe points, each with
  plain     : velocity + pressure through the plain entry: the case profiles/sample_timing.json holds (must not have moved);
  v         : velocity only, plain entry                                     (5 channels)
  v_grad    : velocity plus its gradient, gradient-carrying entry             (5 + 3 + 9 = 17 channels)
  all       : velocity, density, pressure and all their gradients             (25 channels)
all twelve alternating so that drift hits all alike.  A run without a GPU fails; nothing is estimated.

    python tools/gradient_timing.py --out profiles/gradient_timing.json
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import bench        # noqa: E402  (scene dictionaries of the benchmark's workloads)
import sample_timing as st  # noqa: E402  (the HIP-event plumbing and the statistics of the plain measurement)
from sph_taichi_amd import ParticleSystem, sample  # noqa: E402
from sph_taichi_amd.config_builder import SimConfig  # noqa: E402

# case -> (fields, gradients or None for the plain entry)
CASES = {"plain": (("velocity", "pressure"), None), "v": (("velocity",), None), "v_grad": (("velocity",), ("velocity",)),
         "all": (("velocity", "density", "pressure"), ("velocity", "density", "pressure"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", default="c3p_uniform_1.75M")
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--inner", type=int, default=4, help="calls per event pair")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    hip = st.hip_runtime()
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st.ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    st.ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    st.ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    ps = ParticleSystem(SimConfig(config=bench.scene_dict(args.workload)), stream=stream.value)
    solver = ps.build_solver()
    solver.initialize()
    solver.step(args.settle)
    n = int(ps.particle_max_num)

    full = sample.grid_args(particle_diameter=ps.particle_diameter, domain_size=ps.domain_size)
    mid = full["shape"][2] // 2
    cut = {"spacing": full["spacing"], "shape": full["shape"][:2] + (1,),
           "origin": full["origin"][:2] + (float(np.float32(full["origin"][2]) + np.float32(mid) * np.float32(full["spacing"][2])),)}
    x = ps.x.to_numpy()
    pts = np.ascontiguousarray(x[np.linspace(0, n - 1, 64).astype(np.int64)] + np.float32(0.004), dtype=np.float32)
    inv_h = sample.inv_h_f32(ps.support_radius)

    def events(fn):
        st.ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        for _ in range(args.inner):
            fn()
        st.ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        st.ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        st.ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value) / args.inner

    calls, channels, keep = {}, {}, []
    for case, (fields, gradients) in CASES.items():
        sel = sample.select_args(fields=fields)
        g_full, g_cut, psel = st.grid_struct(ps, full, sel), st.grid_struct(ps, cut, sel), sample.make_select(sel)
        keep += [g_full, g_cut, psel]
        if gradients is None:
            channels[case] = 2 + len(sel["planes"])
            calls[f"grid_full/{case}"] = lambda g=g_full: ps._call("sph_sample_grid", C.byref(g))
            calls[f"grid_slice/{case}"] = lambda g=g_cut: ps._call("sph_sample_grid", C.byref(g))
            calls[f"points64/{case}"] = lambda m=sel["mask"], s=psel: ps._call("sph_sample_points", pts.ctypes.data_as(C.c_void_p), 64, m, C.byref(s), inv_h)
        else:
            gm = sample.gradient_args(gradients, sel["fields"])["mask"]
            channels[case] = 2 + len(sel["planes"]) + 3 + 3 * bin(gm).count("1")
            calls[f"grid_full/{case}"] = lambda g=g_full, k=gm: ps._call("sph_sample_grid_gradients", C.byref(g), k)
            calls[f"grid_slice/{case}"] = lambda g=g_cut, k=gm: ps._call("sph_sample_grid_gradients", C.byref(g), k)
            calls[f"points64/{case}"] = lambda m=sel["mask"], s=psel, k=gm: ps._call("sph_sample_points_gradients", pts.ctypes.data_as(C.c_void_p), 64, m, k,
                                                                                   C.byref(s), inv_h)

    for _ in range(2):                          # warm-up: the largest allocation first, the fold of the aux record, clocks
        for name in sorted(calls, key=lambda k: -channels[k.split("/")[1]]):
            calls[name]()
    ps.sync()
    t = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, fn in calls.items():
            t[name].append(events(fn))
    ps.sync()
    out = {
        "workload": args.workload, "particles": n, "settle_steps": args.settle,
        "cases": {k: {"fields": list(f), "gradients": None if g is None else list(g), "channels": channels[k]} for k, (f, g) in CASES.items()},
        "grid_shape": list(full["shape"]), "grid_nodes": int(np.prod(full["shape"])), "slice_shape": list(cut["shape"]),
        "method": f"{args.reps} repetitions, the twelve cases alternating, {args.inner} calls per HIP-event pair on the context's stream, "
                  f"after {args.settle} settling steps and two warm-up rounds; each call is clear + scatter",
    }
    for name, v in t.items():
        case = name.split("/")[1]
        out[name] = st.stats(v, (32 + (16 if {"density", "pressure"} & set(CASES[case][0]) else 0)) * n)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ps.close()


if __name__ == "__main__":
    main()
