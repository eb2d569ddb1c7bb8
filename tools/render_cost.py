#!/usr/bin/env python
"""What does a frame cost beside a step?  (profiles/render_cost.json)

For each workload (the 1.75 M-particle box and the dragon bath of bench.py): after a warm-up, `reps` repetitions of
  * `steps` solver steps,
  * `frames` frames enqueued back to back (sph_render_frame only: clear + splat + large + resolve),
  * `frames` calls of ParticleSystem.render (parameters, frame, download of the 8-bit image),
each timed by the host clock around work that ends in a device synchronise; median and min / max over the repetitions.
From the reference's window camera at 1024 x 1024.

    python tools/render_cost.py --out profiles/render_cost.json
    python tools/render_cost.py --trace-only      # 10 frames and 10 steps per workload, for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench      # noqa: E402  (scene dictionaries of the benchmark's workloads)
import scenes     # noqa: E402
from sph_taichi_amd import render  # noqa: E402


def timed(fn, ps):
    ps.sync()
    t = time.perf_counter()
    fn()
    ps.sync()
    return (time.perf_counter() - t) * 1e3


def stats(samples, per):
    v = sorted(s / per for s in samples)
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "repetitions": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--workloads", nargs="*", default=["c3p_uniform_1.75M", "c2_dragon_bath"])
    ap.add_argument("--size", type=int, nargs=2, default=[1024, 1024])
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    cam, size = render.Camera(), tuple(args.size)
    out = {"camera": "the reference's window camera: eye (5.5, 2.5, 4.0), lookat (-1, 0, 0), fov 70", "image": list(size),
           "method": "host clock around work that ends in a device synchronise; per-step / per-frame = block time / count; "
                     f"{args.reps} repetitions after {args.warmup} warm-up steps and 3 warm-up frames", "workloads": {}}
    for w in args.workloads:
        sd = bench.scene_dict(w)
        ps, solver = scenes.make_ps(sd)
        solver.initialize()
        solver.step(args.warmup)
        for _ in range(3):
            img = ps.render(cam, size=size)
        frame = lambda n: [ps._call("sph_render_frame") for _ in range(n)]
        full = lambda n: [ps.render(cam, size=size) for _ in range(n)]
        if args.trace_only:
            solver.step(10); frame(10); ps.sync()
            ps.close()
            continue
        t_step, t_frame, t_full = [], [], []
        for _ in range(args.reps):      # alternating, so that drift hits all three alike
            t_step.append(timed(lambda: solver.step(args.steps), ps))
            t_frame.append(timed(lambda: frame(args.frames), ps))
            t_full.append(timed(lambda: full(args.frames), ps))
        depth = ps.render_depth()
        import numpy as np
        r = {"particles": int(ps.particle_max_num), "covered_pixels": int(np.isfinite(depth).sum()),
             "step": stats(t_step, args.steps), "frame_kernels": stats(t_frame, args.frames),
             "render_call_with_download": stats(t_full, args.frames)}
        r["frame_in_steps"] = round(r["frame_kernels"]["median_ms"] / r["step"]["median_ms"], 2)
        r["steps_per_render_update"] = sd["Configuration"]["numberOfStepsPerRenderUpdate"]
        out["workloads"][w] = r
        print(w, json.dumps(r), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            render.write_png(os.path.splitext(args.out)[0] + f"_{w}.png", img)
        ps.close()
    if args.out and not args.trace_only:
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
