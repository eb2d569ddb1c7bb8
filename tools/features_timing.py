#!/usr/bin/env python
"""What does one in-step sample of the particle features cost, and is the step untouched without a set?  (include/sph_hip.h,
"Particle features")

A workload of the benchmark (default: the 1,747,584-particle box, every fluid particle a target) in ONE process with HIP events on the
context's stream.  From rest (after `--warmup` steps) and settled (after `--settle` more):
  * in_step: `--inner` steps enqueued in one sph_step call without a set and with the set at every = 1, alternating, `--reps` times;
    the in-step sample is the difference of the medians (the two clears, the target list, the gather with its finish -- and whatever
    the step loses by not taking its lean sort while a set is registered);
  * stand_alone: `--inner` sph_features_sample calls between two events.

With `--parent DIR` (a checkout of the parent commit with its library built) `bench.py --gpus 1 --steps 200 --warmup 20` is run in this
tree and in that one, alternating, `--bench-runs` times each, every run a process of its own, and both trees run the flagship workload
for 220 steps with no set registered and hash positions, velocities and ids (tools/stats_timing.py's own functions).  A run without
a GPU fails; nothing is estimated.

    python tools/features_timing.py --parent ../parent --out profiles/features_timing.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FLAGSHIP = "c3p_uniform_1.75M"
# of k_features_gather, from hipcc -Rpass-analysis=kernel-resource-usage on csrc/sph_features.hip (gfx950, the product's flags)
GATHER_KERNEL = {"vgprs": 98, "scratch_bytes_per_lane": 0, "vgpr_spills": 0, "sgpr_spills": 0, "occupancy_waves_per_simd": 4}


def measure(ps, solver, hip, stream, ev0, ev1, args, st):
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
            ps._call("sph_features_sample")

    med = statistics.median
    ps.set_features(every=1)
    solver.step(args.inner)                              # warm-up with the set
    ps.clear_features()
    solver.step(args.inner)
    ps.sync()
    t_off, t_on = [], []
    for _ in range(args.reps):
        ps.clear_features()
        t_off.append(timed(lambda: solver.step(args.inner)))
        ft = ps.set_features(every=1)
        t_on.append(timed(lambda: solver.step(args.inner)))
    rows = ft.rows()
    valid = (rows["flags"] & 1) != 0
    ps.initialize_particle_system()
    t_alone = [timed(samples) for _ in range(args.reps)]
    ps.clear_features()
    return {"targets": int(valid.sum()), "surface": int(((rows["flags"] & 2) != 0).sum()), "saturated": int(((rows["flags"] & 4) != 0).sum()),
            "mean_neighbours": round(float((rows["n_fluid"] + rows["n_solid"])[valid].mean()), 2),
            "in_step": {"step_no_set_ms": round(med(t_off), 5), "step_with_set_ms": round(med(t_on), 5), "sample_ms": round(med(t_on) - med(t_off), 5),
                        "no_set_min_max_ms": [round(min(t_off), 5), round(max(t_off), 5)],
                        "with_set_min_max_ms": [round(min(t_on), 5), round(max(t_on), 5)]},
            "stand_alone": {"sample_ms": round(med(t_alone), 5), "min_max_ms": [round(min(t_alone), 5), round(max(t_alone), 5)]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--settle", type=int, default=2000)
    ap.add_argument("--inner", type=int, default=10, help="steps (or samples) per event pair")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--workloads", nargs="*", default=[FLAGSHIP])
    ap.add_argument("--parent", default="", help="a checkout of the parent commit, library built: bench.py alternates between the two trees")
    ap.add_argument("--bench-runs", type=int, default=3)
    args = ap.parse_args()

    out = {"method": f"{args.reps} repetitions, the cases alternating, {args.inner} steps or samples per HIP-event pair on the context's stream; "
                     f"in_step.sample_ms = median step with the set at every=1 - median step without; stand_alone: sph_features_sample; from rest "
                     f"after {args.warmup} steps, settled after {args.settle} more; every fluid particle is a target",
           "gather_kernel": GATHER_KERNEL}
    if args.parent:                              # before this process opens the GPU: every run is a process of its own
        import stats_timing as stt
        parent = os.path.abspath(args.parent)
        runs = []
        for k in range(args.bench_runs):
            for build, tree in (("parent", parent), ("this", ROOT)):
                runs.append({"build": build, "run": k + 1, **stt.bench_once(tree)})
                print(json.dumps(runs[-1]), flush=True)
        ms = {b: [r["ms_per_step"] for r in runs if r["build"] == b] for b in ("parent", "this")}
        hashes = {"parent": stt.hash_once(parent, FLAGSHIP), "this": stt.hash_once(ROOT, FLAGSHIP)}
        out["bench_no_set"] = {"command": "bench.py --gpus 1 --steps 200 --warmup 20", "runs": runs,
                               "parent_mean": round(statistics.mean(ms["parent"]), 4), "this_mean": round(statistics.mean(ms["this"]), 4),
                               "parent_min_max": [min(ms["parent"]), max(ms["parent"])], "this_min_max": [min(ms["this"]), max(ms["this"])],
                               "this_inside_parent_spread": min(ms["parent"]) <= statistics.mean(ms["this"]) <= max(ms["parent"]),
                               "state_sha256_after_220_steps": hashes, "bit_identical": hashes["parent"] == hashes["this"]}
        print(json.dumps({k: v for k, v in out["bench_no_set"].items() if k != "runs"}), flush=True)

    if args.workloads:
        import bench        # noqa: E402  (scene dictionaries of the benchmark's workloads)
        import sample_timing as st  # noqa: E402  (the HIP-event plumbing)
        from sph_taichi_amd import ParticleSystem  # noqa: E402
        from sph_taichi_amd.config_builder import SimConfig  # noqa: E402
        hip = st.hip_runtime()
        stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        st.ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
        st.ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
        st.ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")
        for name in args.workloads:
            ps = ParticleSystem(SimConfig(config=bench.scene_dict(name)), stream=stream.value)
            solver = ps.build_solver()
            solver.initialize()
            solver.step(args.warmup)
            w = {"particles": int(ps.particle_max_num)}
            w["from_rest"] = measure(ps, solver, hip, stream, ev0, ev1, args, st)
            print(json.dumps({name: {"from_rest": w["from_rest"]}}), flush=True)
            if args.settle > 0:
                solver.step(args.settle)
                w["settled"] = measure(ps, solver, hip, stream, ev0, ev1, args, st)
                print(json.dumps({name: {"settled": w["settled"]}}), flush=True)
            out[name] = w
            ps.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if os.path.exists(args.out):             # the bench alternation and the workloads may be taken in separate invocations
            with open(args.out) as fh:
                out = {**json.load(fh), **out}
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
