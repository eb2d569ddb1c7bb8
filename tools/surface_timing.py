#!/usr/bin/env python
"""What does a surface frame cost, pass by pass, beside the sphere frame of the same state?  (DESIGN.md, section on the surface frame)

On the benchmark's flagship workload (1,747,584 fluid particles), settled by `--settle` steps, in ONE process and on one state,
at `--size` x `--size` pixels, from the reference's window camera and from one close camera:
  passes : sph_surface_frame_timed -- one frame with a HIP event between its six passes (clear, opaque splat, fluid splat, depth
           smoothing over all iterations, thickness smoothing, shade and resolve), `--reps` times after `--warmup` frames;
  frames : HIP events on the context's stream around `--inner` frames enqueued back to back, the surface frame and the sphere
           frame alternating, `--reps` times; and the host clock of ps.render_surface / ps.render (parameters, frame, download of
           the image, one synchronisation) after a sync;
  filter : taps per pixel the depth filter makes on this picture (from the downloaded depth: (2 R + 1)^2 per pass over the
           pixels that have fluid), and the bytes each pass moves (csrc/sph_surface.hip), beside the HBM peak of the rooflines.
Medians with min / max.  A run without a GPU fails; nothing is estimated.

    python tools/surface_timing.py --out profiles/surface_timing.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench        # noqa: E402  (scene dictionaries of the benchmark's workloads)
from sph_taichi_amd import ParticleSystem, _lib, render  # noqa: E402
from sph_taichi_amd.benchutil import HBM_PEAK_GBS  # noqa: E402
from sph_taichi_amd.config_builder import SimConfig  # noqa: E402
from tools.columns_timing import hip_runtime, ok, stats  # noqa: E402

CAMERAS = {"window": render.Camera(), "close": render.Camera(eye=(2.6, 1.9, 2.8), lookat=(2.2, 0.4, 1.0))}


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
    n_pix = args.size * args.size
    style = render.resolve_style(None, ps.particle_radius, ps._first_fluid_colour())

    def events(symbol):
        ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        for _ in range(args.inner):
            ps._call(symbol)
        ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value) / args.inner

    result = {"workload": args.workload, "particles": int(ps.particle_max_num), "settle_steps": args.settle, "image": list(size),
              "hbm_peak_GBps": HBM_PEAK_GBS, "style": {k: (list(v) if isinstance(v, tuple) else v) for k, v in vars(style).items()},
              "method": f"{args.reps} repetitions after {args.warmup} warm-up frames; passes: one frame with a HIP event between its "
                        f"passes; frames: {args.inner} frames per HIP-event pair on the context's stream, surface and sphere frame "
                        "alternating; host: time.perf_counter around the Python call after a sync", "cameras": {}}
    for name, cam in CAMERAS.items():
        for _ in range(args.warmup):                      # allocations, code objects, caches; also sets both parameter blocks
            img = ps.render_surface(cam, size=size)
            ps.render(cam, size=size)
        depth, thick = ps.render_surface_depth(), ps.render_surface_thickness()
        spheres = ps.render(cam, size=size)
        shown = thick > 0
        passes = {k: [] for k in _lib.SURFACE_PASS_NAMES}
        ms = (C.c_float * _lib.SURFACE_PASSES)()
        for _ in range(args.reps):
            ps._call("sph_surface_frame_timed", ms, _lib.SURFACE_PASSES)
            for k, v in zip(_lib.SURFACE_PASS_NAMES, ms):
                passes[k].append(float(v))
        t_surface, t_spheres, h_surface, h_spheres = [], [], [], []
        for _ in range(args.reps):
            t_surface.append(events("sph_surface_frame"))
            t_spheres.append(events("sph_render_frame"))
            ps.sync()
            t0 = time.perf_counter()
            ps.render_surface(cam, size=size)
            t1 = time.perf_counter()
            ps.render(cam, size=size)
            t2 = time.perf_counter()
            h_surface.append((t1 - t0) * 1e3); h_spheres.append((t2 - t1) * 1e3)
        # taps of the depth filter on THIS picture: the radius follows the shown depth (an estimate from the smoothed depth: the
        # kernel takes it from each pass's input plane, which differs from it by less than the depth range)
        fw = np.float32(style.filter_radius) * render.view_basis(cam, size[1])[3]
        with np.errstate(all="ignore"):
            R = np.where(shown, np.clip(np.ceil(fw / depth), 1, _lib.SURFACE_MAX_FILTER_R), 0)
        taps = float(((2 * R[shown] + 1) ** 2).sum())
        pass_stats = {k: stats(v) for k, v in passes.items()}
        total = sum(s["median_ms"] for s in pass_stats.values())
        smooth_ms = pass_stats["depth_smoothing"]["median_ms"]
        frame, sphere = stats(t_surface), stats(t_spheres)
        result["cameras"][name] = {
            "camera": {"eye": list(cam.eye), "lookat": list(cam.lookat)},
            "fluid_pixels": int(shown.sum()), "fluid_pixel_fraction": round(float(shown.mean()), 4),
            "filter_radius_px": [int(R[shown].min()), int(R[shown].max())] if shown.any() else None,
            "differs_from_sphere_frame_pixels": int((img != spheres).any(axis=-1).sum()),
            "passes": pass_stats, "passes_total_ms": round(total, 5),
            "share_of_frame": {k: round(s["median_ms"] / total, 3) for k, s in pass_stats.items()},
            "surface_frame_events": frame, "sphere_frame_events": sphere,
            "surface_over_sphere": round(frame["median_ms"] / sphere["median_ms"], 2),
            "render_surface_host": stats(h_surface), "render_host": stats(h_spheres),
            "depth_filter": {
                "iterations": int(style.iterations), "window_taps_per_pass": taps,
                "window_taps_per_fluid_pixel": round(taps / max(int(shown.sum()), 1), 1),
                "lds_bytes_per_block": 48 * 48 * 4,
                "global_bytes_per_pass": {"read_with_halo": 36 * n_pix, "read_new": 4 * n_pix, "written": 4 * n_pix},
                "window_taps_per_ns": round(taps * style.iterations / (smooth_ms * 1e6), 2) if smooth_ms > 0 else None,
                "traffic_over_hbm_peak_ms": round(style.iterations * 8 * n_pix / (HBM_PEAK_GBS * 1e9) * 1e3, 5)},
            "bytes": {"clear": 16 * n_pix, "thickness_smoothing": {"read_with_halo": 72 * n_pix, "written": 4 * n_pix},
                      "shade_resolve": {"read": 32 * n_pix, "written": 11 * n_pix},
                      "splats_per_particle_read": 32},
        }
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    ps.close()


if __name__ == "__main__":
    main()
