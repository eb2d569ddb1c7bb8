#!/usr/bin/env python
"""What does colouring a frame by a field cost?  (DESIGN.md, section on the field colouring)

On the benchmark's flagship workload (1,747,584 fluid particles), settled by `--settle` steps, in ONE process and on one state, at
`--size` x `--size` pixels, from the reference's window camera and from one close camera:
  frames : HIP events on the context's stream around `--inner` frames enqueued back to back -- the sphere frame and the surface
           frame, each without a colouring and coloured by speed and by pressure over a fixed range, in turn, `--reps` times;
  range  : the host clock around ParticleSystem.field_range after a sync (the reduction ends in a 24-byte download, so it has no
           enqueue-only form), beside the bytes it reads: 16 N for a velocity field, 32 N for a position, density or pressure.
Medians with min / max.  A run without a GPU fails; nothing is estimated.

    python tools/fieldcolour_timing.py --out profiles/fieldcolour_timing.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench        # noqa: E402  (scene dictionaries of the benchmark's workloads)
from sph_taichi_amd import ParticleSystem, render  # noqa: E402
from sph_taichi_amd.benchutil import HBM_PEAK_GBS  # noqa: E402
from sph_taichi_amd.config_builder import SimConfig  # noqa: E402
from tools.columns_timing import hip_runtime, ok, stats  # noqa: E402
from tools.surface_timing import CAMERAS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", default="c3p_uniform_1.75M")
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="frames per event pair")
    ap.add_argument("--reps", type=int, default=9)
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
    ps.sync()
    size = (args.size, args.size)
    N = int(ps.particle_max_num)

    def events(symbol):
        ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        for _ in range(args.inner):
            ps._call(symbol)
        ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value) / args.inner

    ranges = {}
    for field in ("speed", "pressure", "y"):
        lo, hi, count, bad = ps.field_range(field)
        ranges[field] = (lo, hi) if lo < hi else (lo, lo + 1.0)
    colourings = {"none": None, "speed": render.FieldColour("speed", range=ranges["speed"]),
                  "pressure": render.FieldColour("pressure", range=ranges["pressure"])}
    result = {"workload": args.workload, "particles": N, "settle_steps": args.settle, "image": list(size), "hbm_peak_GBps": HBM_PEAK_GBS,
              "ranges": {k: list(v) for k, v in ranges.items()},
              "method": f"{args.reps} repetitions after {args.warmup} warm-up frames; {args.inner} frames per HIP-event pair on the context's "
                        "stream, the colourings in turn inside every repetition; field_range: time.perf_counter around the call after a sync",
              "cameras": {}, "field_range": {}}
    for name, cam in CAMERAS.items():
        times = {(style, key): [] for style in ("spheres", "surface") for key in colourings}
        pictures = {}
        for rep in range(args.warmup + args.reps):
            for key, colour in colourings.items():
                # the Python call sets view, style and colouring and makes one frame; the events then time that frame again
                pictures[("spheres", key)] = ps.render(cam, size=size, colour=colour)
                t_sph = events("sph_render_frame")
                pictures[("surface", key)] = ps.render_surface(cam, size=size, colour=colour)
                t_sur = events("sph_surface_frame")
                if rep >= args.warmup:
                    times[("spheres", key)].append(t_sph)
                    times[("surface", key)].append(t_sur)
        cams = {"camera": {"eye": list(cam.eye), "lookat": list(cam.lookat)}}
        for style in ("spheres", "surface"):
            base = stats(times[(style, "none")])
            cams[style] = {"none": base}
            for key in ("speed", "pressure"):
                s = stats(times[(style, key)])
                s["over_uncoloured"] = round(s["median_ms"] / base["median_ms"], 3)
                s["pixels_that_differ"] = int((pictures[(style, key)] != pictures[(style, "none")]).any(axis=-1).sum())
                cams[style][key] = s
        result["cameras"][name] = cams
    for field, per_particle in (("speed", 16), ("pressure", 32), ("y", 32)):
        t = []
        for rep in range(args.warmup + args.reps):
            ps.sync()
            t0 = time.perf_counter()
            ps.field_range(field)
            if rep >= args.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        s = stats(t)
        s["bytes_read"] = per_particle * N
        s["GBps_at_median"] = round(per_particle * N / (s["median_ms"] * 1e-3) / 1e9, 1)
        result["field_range"][field] = s
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    ps.close()


if __name__ == "__main__":
    main()
