#!/usr/bin/env python
"""What does one sample of the running flow statistics cost, and is the step untouched without a set?  ("Running flow
statistics")

On the benchmark's flagship workload (1,747,584 fluid particles), ONE process, HIP events on the context's stream, for three grids:
the whole domain at the particle diameter, a slice through the middle of the fluid, and a 32^3 box inside it.  Per grid:
  * in_step: `--inner` steps enqueued in one sph_step call without a set and with the set at every=1, alternating; the in-step
    sample is the difference of the medians;
  * stand_alone: `--inner` sph_stats_sample calls between two events, with the set as registered (scatter + fold) and with the same
    set under a wet threshold no node reaches (scatter + a fold that only reads and zeroes the scratch: 32 B read, 40 B written per
    node).  The difference is the accumulator part of the fold: 88 B read and 88 B written per wet node, for which the achieved
    bytes per second are recorded next to the HBM peak.  The scatter on its own is the sampler's kernel, measured in
    profiles/gradient_timing.json and profiles/sample_timing.json; it is not isolated further here.
Once from rest (after `--warmup` steps) and once on the settled box (`--settle` steps).

With `--parent DIR` (a checkout of the parent commit with its library built) `bench.py --gpus 1 --steps 200 --warmup 20` is run in
this tree and in that one, alternating, `--bench-runs` times each, every run a process of its own, and both trees run the workload
for 220 steps with no set registered and hash positions, velocities and ids: the step must not have moved and the bits must be the
same.  A run without a GPU fails; nothing is estimated.

    python tools/stats_timing.py --parent ../parent --out profiles/stats_timing.json
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK_GBPS = 8000.0          # MI355X: 8 TB/s
NEVER_WET = 1 << 62


def state_hash(tree, workload, steps):
    """sha256 over x, v and pid after `steps` steps of the workload with the library and the package of `tree` (this process)."""
    sys.path.insert(0, tree)
    import numpy as np
    import bench
    from sph_taichi_amd import ParticleSystem
    from sph_taichi_amd.config_builder import SimConfig
    ps = ParticleSystem(SimConfig(config=bench.scene_dict(workload)))
    solver = ps.build_solver()
    solver.initialize()
    solver.step(steps)
    h = hashlib.sha256()
    for name in ("x", "v", "pid"):
        h.update(np.ascontiguousarray(getattr(ps, name).to_numpy()).tobytes())
    ps.close()
    return h.hexdigest()


def bench_once(tree):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=tree, check=True,
                         stdout=subprocess.PIPE, timeout=400).stdout.decode()
    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    return {"ms_per_step": line["ms_per_step"], "value": line["value"], "breakdown_ms": line.get("breakdown_ms")}


def hash_once(tree, workload):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--hash-tree", tree, "--workload", workload], check=True,
                         stdout=subprocess.PIPE, timeout=400).stdout.decode()
    return out.strip().splitlines()[-1]


def grids(ps, np):
    """The three grids, as keyword arguments of set_statistics."""
    x = ps.x.to_numpy()
    d = float(ps.particle_diameter)
    lo, hi = x.min(axis=0).astype(np.float64), x.max(axis=0).astype(np.float64)
    mid = 0.5 * (lo + hi)
    nx = int(np.ceil(float(ps.domain_size[0]) / d)) + 1
    ny = int(np.ceil(float(ps.domain_size[1]) / d)) + 1
    box = np.maximum(mid - 16 * d, lo)
    return {"whole_domain": {}, "slice_z": {"origin": (0.0, 0.0, float(mid[2])), "spacing": d, "shape": (nx, ny, 1)},
            "box_32": {"origin": tuple(float(v) for v in box), "spacing": d, "shape": (32, 32, 32)}}


def measure(ps, solver, hip, stream, ev0, ev1, args, st, np):
    def timed(fn):
        st.ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        fn()
        st.ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        st.ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        st.ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value) / args.inner

    def samples():
        for _ in range(args.inner):
            ps._call("sph_stats_sample")

    med = statistics.median
    out = {}
    for name, kw in grids(ps, np).items():
        s = ps.set_statistics(every=1, **kw)
        solver.step(args.inner)                          # warm-up with the set
        ps.clear_statistics()
        solver.step(args.inner)
        ps.sync()
        t_off, t_on = [], []
        for _ in range(args.reps):
            ps.clear_statistics()
            t_off.append(timed(lambda: solver.step(args.inner)))
            s = ps.set_statistics(every=1, **kw)
            t_on.append(timed(lambda: solver.step(args.inner)))
        acc = s.accumulators()
        wet_nodes = int((acc.n_wet > 0).sum())
        t_full, t_dry = [], []
        for _ in range(args.reps):
            s = ps.set_statistics(every=1, **kw)
            t_full.append(timed(samples))
            p = stats_mod.stats_params(ps, stats_mod.set_args(every=1, particle_diameter=ps.particle_diameter, domain_size=ps.domain_size, **kw))
            p.wet_min = NEVER_WET
            ps._call("sph_stats_set", C.byref(p))
            t_dry.append(timed(samples))
        ps.clear_statistics()
        acc_ms = med(t_full) - med(t_dry)
        acc_bytes = wet_nodes * 176
        out[name] = {"shape": list(s.shape), "nodes": s.nodes, "wet_nodes": wet_nodes,
                     "in_step": {"step_no_set_ms": round(med(t_off), 5), "step_with_set_ms": round(med(t_on), 5),
                                 "sample_ms": round(med(t_on) - med(t_off), 5), "no_set_min_max_ms": [round(min(t_off), 5), round(max(t_off), 5)],
                                 "with_set_min_max_ms": [round(min(t_on), 5), round(max(t_on), 5)]},
                     "stand_alone": {"sample_ms": round(med(t_full), 5), "scatter_plus_dry_fold_ms": round(med(t_dry), 5),
                                     "fold_accumulator_part_ms": round(acc_ms, 5), "fold_accumulator_bytes": acc_bytes,
                                     "fold_accumulator_GBps": round(acc_bytes / (acc_ms * 1e-3) / 1e9, 1) if acc_ms > 0 else None,
                                     "fraction_of_hbm_peak": round(acc_bytes / (acc_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4) if acc_ms > 0 else None,
                                     "dry_fold_bytes": s.nodes * 72}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", default="c3p_uniform_1.75M")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--settle", type=int, default=2000)
    ap.add_argument("--inner", type=int, default=10, help="steps (or samples) per event pair")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent", default="", help="a checkout of the parent commit, library built: bench.py alternates between the two trees")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--hash-tree", default="", help="(child process) print the state hash of 220 steps with the package of this tree")
    args = ap.parse_args()
    if args.hash_tree:
        print(state_hash(os.path.abspath(args.hash_tree), args.workload, 220))
        return

    out = {"workload": args.workload,
           "method": f"{args.reps} repetitions, the cases alternating, {args.inner} steps or samples per HIP-event pair on the context's stream; "
                     f"in_step.sample_ms = median step with the set at every=1 - median step without; stand_alone: sph_stats_sample as "
                     f"registered, and under a wet threshold no node reaches (the fold then only reads and zeroes the scratch); their "
                     f"difference is the fold's accumulator traffic, 176 B per wet node; from rest after {args.warmup} steps, settled after "
                     f"{args.settle} more; HBM peak taken as {HBM_PEAK_GBPS:.0f} GB/s"}
    if args.parent:                              # before this process opens the GPU: every run is a process of its own
        parent = os.path.abspath(args.parent)
        runs = []
        for k in range(args.bench_runs):
            for build, tree in (("parent", parent), ("this", ROOT)):
                runs.append({"build": build, "run": k + 1, **bench_once(tree)})
                print(json.dumps(runs[-1]), flush=True)
        ms = {b: [r["ms_per_step"] for r in runs if r["build"] == b] for b in ("parent", "this")}
        hashes = {"parent": hash_once(parent, args.workload), "this": hash_once(ROOT, args.workload)}
        out["bench_no_set"] = {"command": "bench.py --gpus 1 --steps 200 --warmup 20", "runs": runs,
                               "parent_mean": round(statistics.mean(ms["parent"]), 4), "this_mean": round(statistics.mean(ms["this"]), 4),
                               "parent_min_max": [min(ms["parent"]), max(ms["parent"])], "this_min_max": [min(ms["this"]), max(ms["this"])],
                               "this_inside_parent_spread": min(ms["parent"]) <= statistics.mean(ms["this"]) <= max(ms["parent"]),
                               "state_sha256_after_220_steps": hashes, "bit_identical": hashes["parent"] == hashes["this"]}
        print(json.dumps({k: v for k, v in out["bench_no_set"].items() if k != "runs"}), flush=True)

    global stats_mod
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import bench        # noqa: E402  (scene dictionaries of the benchmark's workloads)
    import sample_timing as st  # noqa: E402  (the HIP-event plumbing)
    from sph_taichi_amd import ParticleSystem, stats as stats_mod  # noqa: E402
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
    out["from_rest"] = measure(ps, solver, hip, stream, ev0, ev1, args, st, np)
    print(json.dumps(out["from_rest"]), flush=True)
    if args.settle > 0:
        solver.step(args.settle)
        out["settled"] = measure(ps, solver, hip, stream, ev0, ev1, args, st, np)
        print(json.dumps(out["settled"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ps.close()


if __name__ == "__main__":
    main()
