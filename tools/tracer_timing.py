#!/usr/bin/env python
"""What does one tracer advance cost, and is the step untouched without tracers?  (DESIGN.md, section on the passive tracers)

On the benchmark's flagship workload (1,747,584 fluid particles), ONE process, HIP events on the context's stream around
`--inner` steps enqueued in one sph_step call: the step without a set and with m = 64, 4,096, 262,144 and 2^20 tracers seeded on
a lattice inside the fluid, all five cases alternating so that drift hits all alike; the advance is the difference of the medians
to the case without a set.  Once from rest (after `--warmup` steps) and once on the settled box (`--settle` steps).  Each case
re-seeds its lattice before it is timed, so the tracers sit in the fluid in every repetition.  Beside each time the algorithmic
bytes -- the candidates of a tracer are the records of its 27 cells, 32 B each (xm + vf), at the rest occupancy of a cell, plus
44 B of tracer state -- and the fraction of the HBM peak they amount to; the mean `count` and the wet fraction of each set are
reported too.  Most of those bytes are served by the caches (neighbouring tracers share their cells), so the fraction says how far
the kernel is from a streaming bound, not what crossed the memory interface.

With `--parent DIR` (a checkout of the parent commit with its library built) `bench.py --gpus 1 --steps 200 --warmup 20` is run
in this tree and in that one, alternating, `--bench-runs` times each, every run a process of its own: the step with no set
registered must not have moved.  A run without a GPU fails; nothing is estimated.

    python tools/tracer_timing.py --parent ../parent --out profiles/tracer_timing.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

HBM_PEAK_GBPS = 8000.0          # MI355X: 8 TB/s
SIZES = (64, 4096, 262144, 1 << 20)


def bench_once(tree):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=tree, check=True,
                         stdout=subprocess.PIPE, timeout=400).stdout.decode()
    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    return {"ms_per_step": line["ms_per_step"], "value": line["value"], "breakdown_ms": line.get("breakdown_ms")}


def seed(lo, hi, m):
    """About m points on a lattice inside the box [lo, hi], cut to exactly m."""
    from sph_taichi_amd import tracers
    ext = (hi - lo).astype(np.float64)
    s = float((ext.prod() / m) ** (1.0 / 3.0))
    while True:
        pts = tracers.lattice(lo, hi, s)
        if pts.shape[0] >= m:
            return np.ascontiguousarray(pts[np.linspace(0, pts.shape[0] - 1, m).astype(np.int64)])
        s *= 0.98


def measure(ps, solver, hip, stream, ev0, ev1, args, st):
    x = ps.x.to_numpy()
    d = float(ps.particle_diameter)
    lo, hi = x.min(axis=0).astype(np.float64) + 2 * d, x.max(axis=0).astype(np.float64) - 2 * d
    sets = {m: seed(lo, hi, m) for m in SIZES}

    def events():
        st.ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        solver.step(args.inner)
        st.ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        st.ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        st.ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value) / args.inner

    def arm(m):
        if m:
            ps.set_tracers(sets[m])
        elif ps.tracers is not None:
            ps.clear_tracers()

    for m in (SIZES[-1], 0):                    # warm-up: the largest allocation first
        arm(m)
        solver.step(args.inner)
    ps.sync()
    t = {m: [] for m in (0,) + SIZES}
    occ = {}
    for _ in range(args.reps):
        for m in t:
            arm(m)
            t[m].append(events())
            if m and m not in occ:
                s = ps.tracers.state()
                wet = s["wet_steps"] > 0
                occ[m] = {"wet_fraction": round(float(wet.mean()), 4), "mean_count": round(float(s["count"].mean()), 2)}
    ps.clear_tracers()
    base = statistics.median(t[0])
    # records per 27 cells: the fluid's rest occupancy of a cell is (cell / diameter)^3
    per_cell = (float(ps.grid_size) / d) ** 3
    out = {"no_set": {"median_ms_per_step": round(base, 5), "min_ms": round(min(t[0]), 5), "max_ms": round(max(t[0]), 5)}}
    for m in SIZES:
        med = statistics.median(t[m])
        adv = med - base
        alg = m * (27 * per_cell * 32 + 44)
        out[f"m={m}"] = {"median_ms_per_step": round(med, 5), "min_ms": round(min(t[m]), 5), "max_ms": round(max(t[m]), 5),
                         "advance_ms": round(adv, 5), "algorithmic_bytes": int(alg), **occ[m],
                         "algorithmic_GBps": round(alg / (adv * 1e-3) / 1e9, 1) if adv > 0 else None,
                         "fraction_of_hbm_peak": round(alg / (adv * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4) if adv > 0 else None}
    out["records_per_cell_at_rest"] = per_cell
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", default="c3p_uniform_1.75M")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--settle", type=int, default=2000)
    ap.add_argument("--inner", type=int, default=10, help="steps per event pair")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent", default="", help="a checkout of the parent commit, library built: bench.py alternates between the two trees")
    ap.add_argument("--bench-runs", type=int, default=2)
    args = ap.parse_args()

    out = {"workload": args.workload,
           "method": f"{args.reps} repetitions, the five cases alternating, {args.inner} steps per HIP-event pair on the context's stream; "
                     f"advance_ms = median with the set - median without; from rest after {args.warmup} steps, settled after "
                     f"{args.settle} more; algorithmic bytes = m * (27 cells * records per cell at rest * 32 B + 44 B of tracer state); "
                     f"HBM peak taken as {HBM_PEAK_GBPS:.0f} GB/s"}
    if args.parent:                              # before this process opens the GPU: every bench run is a process of its own
        runs = []
        for k in range(args.bench_runs):
            for build, tree in (("parent", os.path.abspath(args.parent)), ("this", ROOT)):
                runs.append({"build": build, "run": k + 1, **bench_once(tree)})
                print(json.dumps(runs[-1]), flush=True)
        ms = {b: [r["ms_per_step"] for r in runs if r["build"] == b] for b in ("parent", "this")}
        out["bench_no_set"] = {"command": "bench.py --gpus 1 --steps 200 --warmup 20", "runs": runs,
                               "parent_mean": round(statistics.mean(ms["parent"]), 4), "this_mean": round(statistics.mean(ms["this"]), 4),
                               "parent_spread": round(max(ms["parent"]) - min(ms["parent"]), 4),
                               "this_spread": round(max(ms["this"]) - min(ms["this"]), 4)}

    import bench        # noqa: E402  (scene dictionaries of the benchmark's workloads)
    import sample_timing as st  # noqa: E402  (the HIP-event plumbing)
    from sph_taichi_amd import ParticleSystem  # noqa: E402
    from sph_taichi_amd.config_builder import SimConfig  # noqa: E402
    hip = st.hip_runtime()
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st.ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    st.ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    st.ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")
    ps = ParticleSystem(SimConfig(config=bench.scene_dict(args.workload)), stream=stream.value)
    solver = ps.build_solver()
    solver.initialize()
    solver.step(args.warmup)
    out["particles"] = int(ps.particle_max_num)
    out["from_rest"] = measure(ps, solver, hip, stream, ev0, ev1, args, st)
    print(json.dumps(out["from_rest"]), flush=True)
    solver.step(args.settle)
    out["settled"] = measure(ps, solver, hip, stream, ev0, ev1, args, st)
    print(json.dumps(out["settled"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ps.close()


if __name__ == "__main__":
    main()
