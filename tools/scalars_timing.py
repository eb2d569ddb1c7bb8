#!/usr/bin/env python
"""What does one in-step sample of the carried scalars cost, and is the step untouched without a set?  ("Carried scalars")

The flagship workload (the 1,747,584-particle box, every particle a carrier) in ONE process with HIP events on the context's stream.
From rest (after `--warmup` steps) and settled (after `--settle` more), for K = 1 and K = 4:
  * in_step: `--inner` steps enqueued in one sph_step call without a set and with the set at every = 1, alternating, `--reps` times;
    the in-step sample is the difference of the medians (stage + diffusion + the 4-byte clear);
  * stand_alone: `--inner` sph_scalars_sample calls between two events.
The split stage / diffusion is NOT measured: two event pairs inside one sample would need events between the two launches of the
library's own sample, which the ABI does not offer.

With `--parent DIR` (a checkout of the parent commit with its library built) `bench.py --gpus 1 --steps 200 --warmup 20` is run in this
tree and in that one, alternating, `--bench-runs` times each, every run a process of its own, and both trees run the flagship workload
for 220 steps with no set registered and hash positions, velocities and ids (tools/stats_timing.py's own functions).  A run without
a GPU fails; nothing is estimated.

    python tools/scalars_timing.py --parent ../parent --out profiles/scalars_timing.json
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

WORKLOAD = "c3p_uniform_1.75M"
KAPPA = 1.0e-4


def measure(ps, solver, k, hip, stream, ev0, ev1, args, st):
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
            ps._call("sph_scalars_sample")

    med = statistics.median
    names = tuple(f"c{j}" for j in range(k))
    kw = {"channels": names, "diffusivity": (KAPPA,) * k, "values": {0: tuple(float(j + 1) for j in range(k))}, "every": 1}
    ps.set_scalars(**kw)
    solver.step(args.inner)                              # warm-up with the set
    ps.clear_scalars()
    solver.step(args.inner)
    ps.sync()
    t_off, t_on = [], []
    for _ in range(args.reps):
        ps.clear_scalars()
        t_off.append(timed(lambda: solver.step(args.inner)))
        sc = ps.set_scalars(**kw)
        t_on.append(timed(lambda: solver.step(args.inner)))
    info = sc.info()
    ps.initialize_particle_system()
    t_alone = [timed(samples) for _ in range(args.reps)]
    ps.clear_scalars()
    return {"K": k, "overshoot": info.overshoot, "saturated": info.saturated,
            "in_step": {"step_no_set_ms": round(med(t_off), 5), "step_with_set_ms": round(med(t_on), 5), "sample_ms": round(med(t_on) - med(t_off), 5),
                        "no_set_min_max_ms": [round(min(t_off), 5), round(max(t_off), 5)],
                        "with_set_min_max_ms": [round(min(t_on), 5), round(max(t_on), 5)]},
            "stand_alone": {"sample_ms": round(med(t_alone), 5), "min_max_ms": [round(min(t_alone), 5), round(max(t_alone), 5)]},
            "split_stage_diffuse": "not measured"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--settle", type=int, default=2000)
    ap.add_argument("--inner", type=int, default=10, help="steps (or samples) per event pair")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--channels", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--parent", default="", help="a checkout of the parent commit, library built: bench.py alternates between the two trees")
    ap.add_argument("--bench-runs", type=int, default=3)
    args = ap.parse_args()

    out = {"method": f"{args.reps} repetitions, the cases alternating, {args.inner} steps or samples per HIP-event pair on the context's stream; "
                     f"in_step.sample_ms = median step with the set at every=1 - median step without; stand_alone: sph_scalars_sample; from rest "
                     f"after {args.warmup} steps, settled after {args.settle} more; every particle of {WORKLOAD} is a carrier"}
    if args.parent:                              # before this process opens the GPU: every run is a process of its own
        import stats_timing as stt
        parent = os.path.abspath(args.parent)
        runs = []
        for k in range(args.bench_runs):
            for build, tree in (("parent", parent), ("this", ROOT)):
                runs.append({"build": build, "run": k + 1, **stt.bench_once(tree)})
                print(json.dumps(runs[-1]), flush=True)
        ms = {b: [r["ms_per_step"] for r in runs if r["build"] == b] for b in ("parent", "this")}
        hashes = {"parent": stt.hash_once(parent, WORKLOAD), "this": stt.hash_once(ROOT, WORKLOAD)}
        out["bench_no_set"] = {"command": "bench.py --gpus 1 --steps 200 --warmup 20", "runs": runs,
                               "parent_mean": round(statistics.mean(ms["parent"]), 4), "this_mean": round(statistics.mean(ms["this"]), 4),
                               "parent_min_max": [min(ms["parent"]), max(ms["parent"])], "this_min_max": [min(ms["this"]), max(ms["this"])],
                               "this_inside_parent_spread": min(ms["parent"]) <= statistics.mean(ms["this"]) <= max(ms["parent"]),
                               "state_sha256_after_220_steps": hashes, "bit_identical": hashes["parent"] == hashes["this"]}
        print(json.dumps({k: v for k, v in out["bench_no_set"].items() if k != "runs"}), flush=True)

    if args.channels:
        import bench        # noqa: E402  (scene dictionaries of the benchmark's workloads)
        import sample_timing as st  # noqa: E402  (the HIP-event plumbing)
        from sph_taichi_amd import ParticleSystem  # noqa: E402
        from sph_taichi_amd.config_builder import SimConfig  # noqa: E402
        hip = st.hip_runtime()
        stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        st.ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
        st.ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
        st.ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")
        ps = ParticleSystem(SimConfig(config=bench.scene_dict(WORKLOAD)), stream=stream.value)
        solver = ps.build_solver()
        solver.initialize()
        solver.step(args.warmup)
        w = {"particles": int(ps.particle_max_num)}
        w["from_rest"] = [measure(ps, solver, k, hip, stream, ev0, ev1, args, st) for k in args.channels]
        print(json.dumps({"from_rest": w["from_rest"]}), flush=True)
        if args.settle > 0:
            solver.step(args.settle)
            w["settled"] = [measure(ps, solver, k, hip, stream, ev0, ev1, args, st) for k in args.channels]
            print(json.dumps({"settled": w["settled"]}), flush=True)
        out[WORKLOAD] = w
        ps.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if os.path.exists(args.out):             # the bench alternation and the workload may be taken in separate invocations
            with open(args.out) as fh:
                out = {**json.load(fh), **out}
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
