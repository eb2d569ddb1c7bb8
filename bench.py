#!/usr/bin/env python
"""bench.py -- WCSPH steps/s + ms/step breakdown (sort / neighbour / force) on MI355X.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one WCSPHSolver.step() (SPHBase.step(), reference sph_base.py:263-271)
over the synthetic uniform box of BASELINE.md (C3': 246x74x96 = 1,747,584 fluid
particles in the armadillo scene's (5,3,2) domain; BASELINE.json's metric is quoted
at 1.74 M particles).  Inputs are resident in HBM before the timed region.

`value` = particle-steps/s / 1,747,584, i.e. "steps/s at 1.74 M particles": at
N = 1 it is exactly the job's steps/s; at N > 1 (x-slab sharding, every rank owns
one 1.75 M slab: weak scaling) it is the whole-job aggregate.

The JSON line also carries
  roofline      : the dominant kernel, ALWAYS the density + EOS sweep (largest duration in the committed
                  kernel traces; `roofline_force` is the force sweep's object) -- algorithmic bytes per
                  launch (32*N + 4*G) / its mean launch time from HIP events
                  on the kernel's own stream, against the 8 TB/s HBM peak; `traffic`
                  (rocprofv3 FETCH_SIZE*2 + WRITE_SIZE) and the VALU figures come from
                  profiles/pmc_traffic.json and are quoted only if that file was
                  measured on the same kernel sources (fingerprint), else null;
  roofline_valu : wave-level VALU instructions per launch / launch time against
                  1024 SIMD-32 x 2.4 GHz / 2 cycles, and the useful FLOP rate of
                  SURVEY 8d against 157.3 TFLOP/s;
  cpu_baseline  : the CPU oracle (oracle/sph_oracle.c, "port" of the reference
                  algorithm with OpenMP; timing build -O3 -march=native) on the CPUs
                  this container may use (cgroup quota), median of three bounded
                  samples of the same workload;
  neighbourhood : list lengths / cell occupancy of the last density sweep;
  reps, first_rep: the contract's block (W untimed + exactly K timed steps from the initial lattice) repeated
                  from the restored initial state until --min-seconds of timed steps have run: value /
                  ms_per_step / breakdown_ms are the means;
  preheat_ms, cold_block: every block starts behind that many ms of unrelated GPU load (the clock ramp after
                  the host-side set-up is 8 % of a 25-step block); cold_block = one block without it;
  settled       : the same box after --settled-after further steps (what a long run sees), with its own value,
                  ms_per_step, breakdown_ms, neighbourhood, roofline_kernels, roofline_step;
  roofline_kernels, roofline_step: both sweeps of each state (bytes, event time, counter traffic, VALU share).
--settle K times a developed flow, --variant M an A/B kernel instance, --ablate the
section table of DESIGN.md section 4.4 (stderr).

A plain run (no --full) is lean: set-up, W warm-up steps, exactly K timed steps (one block), the outputs if
--dump-outputs DIR is given, the line.  `reps` is 1 and `cold_block`, `settled`, `with_bodies` and `cpu_baseline`
are null (the DFSPH line's `runahead_ab` too).  --full adds everything else listed above: the repeated blocks until
--min-seconds, the cold block, the settled state, the with-bodies workload, the CPU baseline and the DFSPH run-ahead A/B.

--dump-outputs DIR writes what the timed path computed in its last step -- the particle arrays x, v, density and
pressure a caller of WCSPHSolver.step() reads back -- as DIR/<name>.npy (float32), rows ordered by persistent particle id
so that two builds compare element by element.  Above 64 MB in all, a fixed seeded sample of the particles is written
instead, with their ids in DIR/sample_ids.npy (float64).
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# several processes sharing GPU memory handles (RCCL between ranks): the host driver of this pool supports dmabuf IPC only;
# the launcher's environment normally carries this already
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

from sph_taichi_amd.benchutil import REF_PARTICLES, HBM_PEAK_GBS, gpu_preheat, _HEAT  # noqa: E402

CFG = {
    "domainStart": [0.0, 0.0, 0.0], "domainEnd": [5.0, 3.0, 2.0], "particleRadius": 0.01,
    "numberOfStepsPerRenderUpdate": 1, "density0": 1000, "simulationMethod": 0,
    "gravitation": [0.0, -9.81, 0.0], "timeStepSize": 0.0004, "stiffness": 50000, "exponent": 7,
    "boundaryHandlingMethod": 0, "exportFrame": False, "exportPly": False, "exportObj": False,
}

WORKLOADS = {
    # name: (domainEnd, fluid lattice counts, lower corner)
    "c3p_uniform_1.75M": ([5.0, 3.0, 2.0], (246, 74, 96), (0.04, 0.04, 0.04)),
    "c1_dambreak_262k": ([3.2, 2.0, 1.4], (64, 64, 64), (0.04, 0.04, 0.04)),
    "c0_dragon_fluid_423k": ([5.0, 3.0, 2.0], (55, 140, 55), (0.3, 0.1, 0.7)),
    # the headline box thrown against its +x / +z walls: with --settle K the timed steps run on a developed,
    # compressed / sloshing state instead of the rest lattice (VERDICT r01 "weak" #3)
    "c3p_slosh_1.75M": ([5.0, 3.0, 2.0], (246, 74, 96), (0.04, 0.04, 0.04)),
    # BASELINE.json config 5 in its own geometry: at N = 1 one context holds all 13.9 M particles; with
    # --gpus N the ranks cut it by particle count and re-plan the cuts every --recut-every steps (distributed.run_c4_dambreak)
    "c4_dambreak": ([16.0, 4.0, 3.4], (512, 165, 165), (0.04, 0.04, 0.04)),
}
INITIAL_VELOCITY = {"c0_dragon_fluid_423k": [0.0, -1.0, 0.0], "c3p_slosh_1.75M": [1.0, -0.5, 0.5]}


# armadillo_bath_dynamic.json equivalent: the three bodies are released with their lowest voxels just above the fluid's
# surface (y = 1.50) -- at the scene file's own height they would still be in free fall when a bench block ends and the
# two-way coupling would be idle in the number (VERDICT r03 "missing" #4)
BODY_Y = 1.74

DFSPH_DT = 0.004    # timeStepSize of every *_dfsph.json scene of the reference (data/scenes/)


def scene_dict(workload: str, solver: str = "wcsph"):
    sd = _scene_dict(workload)
    if solver == "dfsph":
        sd["Configuration"]["simulationMethod"] = 4
        sd["Configuration"]["timeStepSize"] = DFSPH_DT
    return sd


def _scene_dict(workload: str):
    if workload in ("c2_dragon_bath", "c3_armadillo_equiv"):
        # the reference's two demo scenes with their bodies taken from the committed voxel fixtures
        # (sph_taichi_amd/data/bodies/*.npy; /root/reference does not exist on the GPU box)
        from sph_taichi_amd import workloads
        return workloads.dragon_bath_scene() if workload == "c2_dragon_bath" else workloads.armadillo_equiv_scene(body_y=BODY_Y)
    dom, counts, corner = WORKLOADS[workload]
    cfg = copy.deepcopy(CFG)
    cfg["domainEnd"] = dom
    d = 2 * cfg["particleRadius"]
    end = [c + (n - 0.5) * d for c, n in zip(corner, counts)]
    vel = INITIAL_VELOCITY.get(workload, [0.0, 0.0, 0.0])
    return {"Configuration": cfg,
            "FluidBlocks": [{"objectId": 0, "start": list(corner), "end": end, "translation": [0.0, 0.0, 0.0],
                             "scale": [1, 1, 1], "velocity": vel, "density": 1000.0, "color": [50, 100, 200]}]}


def cpu_baseline(sd, sample_steps: int, repeats: int = 3):
    """Time the CPU oracle on a bounded sample of the same workload (rank 0, N=1 only): the timing build of
    oracle/sph_oracle.c (-O3 -march=native, compiled here on this host), OpenMP over every
    core the process may use, median of `repeats` samples of `sample_steps` steps each."""
    from oracle.oracle import Oracle, lib
    from sph_taichi_amd.config_builder import SimConfig
    from sph_taichi_amd import scene as scene_mod
    cfg = SimConfig(config=copy.deepcopy(sd))
    sc = scene_mod.build_scene(cfg)
    g = sc.geom
    params = dict(particle_radius=g.particle_radius, domain_size=list(g.domain_size),
                  density_0=cfg.get_cfg("density0"), stiffness=cfg.get_cfg("stiffness"),
                  exponent=cfg.get_cfg("exponent"), dt=cfg.get_cfg("timeStepSize"), g=cfg.get_cfg("gravitation"),
                  simulation_method=cfg.get_cfg("simulationMethod") or 0, fluid_particle_num=sc.fluid_particle_num)
    build = "-O3 -march=native (oracle/Makefile: libsph_oracle_timing.so)"
    try:
        L = lib(timing=True)
        timing = True
    except Exception as e:      # no compiler on this host: time the parity build and say so
        L = lib()
        timing = False
        build = f"-O2 -ffp-contract=off parity build (timing build failed: {type(e).__name__})"
    from oracle.oracle import usable_cpus
    threads = usable_cpus()          # scheduler affinity capped by the cgroup CPU quota (16 on the GPU boxes, whose nproc is 256)
    o = Oracle(params, sc.arrays, n_objects=max(sc.n_objects, 1), rigid_body_ids=sorted(sc.object_id_rigid_body),
               dynamic_ids=sorted(sc.dynamic_rigid_ids), omp_threads=threads, timing_build=timing)
    o.initialize()
    o.step(1)                                   # warm-up (page faults, first sort)
    samples, phases = [], None
    for _ in range(max(repeats, 1)):
        t0 = time.perf_counter()
        ms = o.step(sample_steps)
        samples.append(time.perf_counter() - t0)
        phases = ms
    samples.sort()
    dt = samples[len(samples) // 2]
    n = sc.particle_max_num
    return {"value": round(sample_steps / dt * n / REF_PARTICLES, 4), "unit": "steps/s at 1.74M particles",
            "cores": threads, "threads": threads, "nproc": os.cpu_count(), "kind": "port",
            "cores_note": "cores = CPUs this container may use (affinity capped by the cgroup quota); nproc = what the host reports",
            "sample": f"median of {len(samples)} samples of {sample_steps} steps of the same {n}-particle workload "
                      f"after 1 warm-up step; oracle/sph_oracle.c, {build}, {threads} OpenMP threads",
            "ms_per_step": round(dt / sample_steps * 1e3, 2),
            "samples_ms_per_step": [round(x / sample_steps * 1e3, 2) for x in samples],
            "phase_ms": {k: round(v / sample_steps, 2) for k, v in zip(("sort", "neighbour", "force", "integrate"), phases)}}


def with_bodies(args, local_rank, immerse_steps=300):
    """BASELINE.json config 4 (armadillo_bath_dynamic.json equivalent: 1,723,968 fluid particles + three dynamic bodies of
    density 7874 / 1700 / 300, two-way coupling + shape matching) timed AFTER the bodies are in the fluid: released just above
    the surface with the scene's own v0 = -5 m/s, `immerse_steps` untimed steps, then exactly K timed steps.  The line
    asserts that the coupling was at work: the light body must be far from free fall and most rigid particles below the
    initial surface.  `rigid_phase` = the integrate bucket with solve_rigid_body() batched (three launches for all bodies, the
    default) and body by body (4 launches each, SPH_OPT_RIGID_BATCH 0), measured on the same state."""
    import copy
    import numpy as np
    import torch
    from sph_taichi_amd import ParticleSystem, SimConfig, _lib
    sd = scene_dict("c3_armadillo_equiv")
    ps = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), device=local_rank)
    solver = ps.build_solver()
    N = ps.particle_max_num
    solver.initialize()
    solver.step(immerse_steps)
    ps.sync()

    def block(batch, steps):
        ps.set_option(_lib.OPT_RIGID_BATCH, batch)
        gpu_preheat(local_rank, args.preheat_ms)
        solver.step(args.warmup)
        ps.set_option(_lib.OPT_TIMING, args.time_every)
        ps._call("sph_reset_timings")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.step(steps)
        ps.sync()
        dt = time.perf_counter() - t0
        tm = _lib.SphTimings()
        ps._call("sph_get_timings", tm)
        ps.set_option(_lib.OPT_TIMING, 0)
        k = max(int(tm.steps), 1)
        return dt, {"sort": round(tm.sort_ms / k, 4), "neighbour": round(tm.neighbour_ms / k, 4), "force": round(tm.force_ms / k, 4),
                    "integrate": round(tm.integrate_ms / k, 4), "sum_of_phases": round(tm.total_ms / k, 4)}

    steps = max(args.steps, 100)
    dt, bd = block(1, steps)
    _, bd_seq = block(0, min(steps, 50))
    ps.set_option(_lib.OPT_RIGID_BATCH, 1)
    oid = ps.object_id.to_numpy()
    mat = ps.material.to_numpy()
    x, v = ps.x.to_numpy(), ps.v.to_numpy()
    done = immerse_steps + 2 * args.warmup + steps + min(steps, 50)
    free_fall = -5.0 - 9.81 * done * CFG["timeStepSize"]
    rigid = mat == 0
    light = oid == 3
    out = {"workload": "c3_armadillo_equiv (armadillo_bath_dynamic.json: stand-in mesh, bodies released at y = %.2f)" % BODY_Y,
           "particles": N, "rigid_particles": int(rigid.sum()), "immerse_steps": immerse_steps,
           "value": round(steps / dt * N / REF_PARTICLES, 3), "ms_per_step": round(dt / steps * 1e3, 4), "steps_timed": steps,
           "breakdown_ms": bd,
           "rigid_phase": {"integrate_ms_batched": bd["integrate"], "integrate_ms_body_by_body": bd_seq["integrate"],
                           "launches_batched": "3 for all bodies (the dynamic solids' advect and every solid wall pass inside)",
                           "launches_body_by_body": "advect + 4 per body"},
           "immersed_fraction_of_rigid_particles": round(float((x[rigid, 1] < 1.5).mean()), 4),
           "light_body_mean_vy": round(float(v[light, 1].mean()), 4), "free_fall_vy": round(free_fall, 4),
           "coupling_active": bool(v[light, 1].mean() > free_fall + 1.0)}
    ps.close()
    if not out["coupling_active"]:
        raise RuntimeError(f"the light body is still in free fall ({out['light_body_mean_vy']} vs {out['free_fall_vy']}): the coupling was idle")
    return out


DUMP_FIELDS = ("x", "v", "density", "pressure")
DUMP_BUDGET_BYTES = 64_000_000


def dump_outputs(ps, out_dir):
    """The arrays a caller of the timed path reads back after its last step, as out_dir/<name>.npy (float32), rows in
    persistent-id order.  Above DUMP_BUDGET_BYTES in all, a fixed seeded sample of the particles (same rows in every
    array; their ids in sample_ids.npy)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    pid = ps.pid.to_numpy()
    n = pid.shape[0]
    arrays = {}
    for name in DUMP_FIELDS:
        a = getattr(ps, name).to_numpy()
        by_pid = np.empty_like(a)
        by_pid[pid] = a
        arrays[name] = by_pid.astype(np.float32, copy=False)
    row_bytes = sum(a.itemsize * (a.size // n) for a in arrays.values())
    if row_bytes * n > DUMP_BUDGET_BYTES:
        keep = DUMP_BUDGET_BYTES // (row_bytes + 8)
        ids = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
        arrays = {k: np.ascontiguousarray(a[ids]) for k, a in arrays.items()}
        arrays["sample_ids"] = ids.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="c3p_uniform_1.75M",
                    choices=sorted(WORKLOADS) + ["c2_dragon_bath", "c3_armadillo_equiv"])
    ap.add_argument("--solver", default="wcsph", choices=["wcsph", "dfsph"],
                    help="dfsph: the same workload under DFSPHSolver (simulationMethod 4, dt = 4e-3) -- a supplementary "
                         "line, not BASELINE.json's metric")
    ap.add_argument("--settle", type=int, default=0,
                    help="run this many untimed steps first, so that the timed ones see a developed flow (dam-break front, "
                         "sloshing, compression at the walls) instead of the initial lattice")
    ap.add_argument("--settled-after", type=int, default=2000,
                    help="--full: the line also times the box after this many further untimed steps (`settled` object); 0 = skip")
    ap.add_argument("--min-seconds", type=float, default=0.5,
                    help="--full: each state is timed for at least this long: from rest by repeating the K-step block from the "
                         "re-uploaded initial state (`reps`), settled as one longer block")
    ap.add_argument("--max-reps", type=int, default=80)
    ap.add_argument("--preheat-ms", type=float, default=50.0,
                    help="untimed GPU work (a matrix product loop on the same device, nothing of the solver's) right before "
                         "every block's warm-up steps: the GPU idles while the host builds / restores the scene and comes back "
                         "at a lower clock for the first milliseconds (0 = off; the line reports a block without it beside)")
    ap.add_argument("--recut-every", type=int, default=0,
                    help="--gpus N: re-cut the slabs every K steps (0 = never for the tiled workload, which is balanced by "
                         "construction; the c4_dambreak workload defaults to 10)")
    ap.add_argument("--c4", type=int, default=1,
                    help="--gpus N: after the tiled weak-scaling line also run BASELINE.json's config 5 (the 13.9 M dam-break in its "
                         "own tank, travelling cuts) and attach it as `c4_dambreak` (0 = skip)")
    ap.add_argument("--watchdog-s", type=float, default=900.0,
                    help="--gpus N: wall-clock budget of the whole job; a rank that exceeds it (or the c4_dambreak object its own "
                         "share, --c4-budget-s) prints a JSON line naming the stage it hung in and every rank exits (0 = off)")
    ap.add_argument("--c4-budget-s", type=float, default=300.0,
                    help="--gpus N: wall-clock budget of the supplementary c4_dambreak object; when it is exceeded the finished "
                         "tiled line is printed with c4_dambreak = {error: watchdog, stage: ...}")
    ap.add_argument("--with-bodies", type=int, default=1,
                    help="--full: the line also times the armadillo_bath_dynamic.json equivalent (1.72 M fluid + 3 dynamic bodies, "
                         "two-way coupling) once the bodies are immersed: `with_bodies` object (0 = skip)")
    ap.add_argument("--gather-impl", type=int, default=1)
    ap.add_argument("--brick-shape", type=int, default=0)
    ap.add_argument("--fused", type=int, default=1)
    ap.add_argument("--variant", type=int, default=-1, help="SPH_OPT_KERNEL_VARIANT mask (-1 = the library's default)")
    ap.add_argument("--brick-records", type=int, default=1, choices=[0, 1],
                    help="SPH_OPT_BRICK_RECORDS: 1 (default) = the list-reading sweeps load the brick column tables the density sweep left "
                         "behind, 0 = every sweep recomputes them from the cell array (A/B; bit-identical results)")
    ap.add_argument("--df-fuse-error", type=int, default=1, choices=[0, 1],
                    help="SPH_OPT_DF_FUSE_ERROR (--solver dfsph): 1 (default) = the refresh sweep of a solver iteration reduces the density error "
                         "itself, 0 = a streaming kernel re-reads the particles (A/B)")
    ap.add_argument("--cpu-steps", type=int, default=10, help="--full: CPU-oracle sample size (0 = skip the baseline leg)")
    ap.add_argument("--sweep", action="store_true", help="also time every gather variant (stderr table)")
    ap.add_argument("--time-every", type=int, default=8,
                    help="per-phase HIP events (breakdown_ms, roofline.avg_launch_ms) in every k-th step of the timed region: an "
                         "event record is a packet between two kernels, five per step cost 4 %% of the step (k = 1), k = 8 costs 0.5 %%")
    ap.add_argument("--ablate", action="store_true", help="profiling: time the sweeps with sections skipped (stderr)")
    ap.add_argument("--ablate-mask", type=int, default=0, help="profiling: run the whole bench with this ablation mask (results invalid)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline block: repeated blocks until --min-seconds, the cold block, the settled "
                         "state, the with-bodies workload, the CPU baseline, the DFSPH run-ahead A/B (a plain run times one "
                         "block of exactly --steps steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the particle arrays of the last timed step (x, v, density, pressure; float32, by persistent id) "
                         "as DIR/<name>.npy")
    args = ap.parse_args()
    if args.dump_outputs and args.gpus > 1:
        ap.error("--dump-outputs is a single-GPU option (--gpus 1)")
    if args.ablate or args.ablate_mask:
        # section ablation lives in the PROFILING build of the library only (csrc: -DSPH_PROFILE); build / load that one
        os.environ["SPH_HIP_LIB_VARIANT"] = "profile"

    metric = "WCSPH steps/sec at 1.74 M particles (+ ms/step breakdown sort/neighbour/force)"
    if args.gpus > 1 and not ("RANK" in os.environ and "WORLD_SIZE" in os.environ):
        # No launcher: this process becomes the supervisor of its own N ranks (VERDICT r04 "next" #2a).
        from sph_taichi_amd.benchutil import self_launch
        sys.exit(self_launch(os.path.abspath(__file__), sys.argv[1:], args.gpus, args.watchdog_s, metric=metric))
    # A launcher is present iff it set RANK and WORLD_SIZE (torch.distributed.run sets both); a WORLD_SIZE merely inherited
    # from some outer environment is not a job to join.
    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    world = int(os.environ["WORLD_SIZE"]) if launched else 1
    rank = int(os.environ.get("RANK", "0")) if launched else 0
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if launched else 0
    gpus_given = any(a == "--gpus" or a.startswith("--gpus=") for a in sys.argv[1:])
    if launched and not gpus_given:
        args.gpus = world           # `torchrun ... bench.py` without --gpus: the launcher's world is the job
    if world != args.gpus:
        # never die without a line: the driver parses stdout (exit code 2 = bad invocation)
        if rank == 0:
            print(json.dumps({"metric": metric, "value": None, "unit": "steps/s", "n_gpus": args.gpus, "error": "invocation",
                              "stage": "argument check", "rank": rank,
                              "detail": f"--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks"}), flush=True)
        sys.exit(2)
    from sph_taichi_amd.benchutil import Watchdog
    wd = Watchdog(rank, world, total_s=args.watchdog_s, metric=metric, enabled=world > 1, take_sigterm=world > 1)
    wd.stage("import torch")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    # SPH_DIST_BACKEND=gloo lets several ranks share one GPU (how the N>1 path is exercised on a 1-GPU box)
    backend = os.environ.get("SPH_DIST_BACKEND", "nccl")
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    if world > 1:
        import datetime
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")     # one node by contract; the container's hostname may not resolve
        wd.stage(f"init_process_group({backend})")
        to = datetime.timedelta(seconds=max(min(args.watchdog_s, 600.0), 60.0))
        try:
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=to)
            else:
                dist.init_process_group(backend, timeout=to)
            from sph_taichi_amd.distributed import run_slab_bench
            line = run_slab_bench(args, rank, world, local_rank, wd=wd)
        except BaseException as e:      # noqa: BLE001 -- a rank that fails must say so and LEAVE: its peers sit in collectives
            import traceback
            traceback.print_exc()
            wd.fail(f"{type(e).__name__}: {e}")
        if rank == 0:
            wd.emit(line)
        wd.stage("destroy_process_group", budget_s=30.0)
        dist.destroy_process_group()
        return

    from sph_taichi_amd import ParticleSystem, SimConfig, _lib
    sd = scene_dict(args.workload, args.solver)
    ps = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), device=local_rank)
    solver = ps.build_solver()
    ps.set_option(_lib.OPT_BRICK_RECORDS, args.brick_records)
    ps.set_option(_lib.OPT_DF_FUSE_ERROR, args.df_fuse_error)
    N = ps.particle_max_num
    G = int(ps.grid_num[0] * ps.grid_num[1] * ps.grid_num[2])

    def run(impl, shape, fused, steps, warmup, heat_ms=None):
        ps.set_option(_lib.OPT_GATHER_IMPL, impl)
        ps.set_option(_lib.OPT_BRICK_SHAPE, shape)
        ps.set_option(_lib.OPT_FUSED_STEP, fused)
        ps.set_option(_lib.OPT_TIMING, 0)
        gpu_preheat(local_rank, args.preheat_ms if heat_ms is None else heat_ms)
        solver.step(warmup)
        ps.set_option(_lib.OPT_TIMING, args.time_every)
        ps._call("sph_reset_timings")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.step(steps)
        ps.sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tm = _lib.SphTimings()
        ps._call("sph_get_timings", tm)
        return dt, tm

    solver.initialize()
    ps.set_option(_lib.OPT_KERNEL_VARIANT, args.variant)
    if args.settle > 0:
        solver.step(args.settle)
        ps.sync()
    if args.ablate_mask:
        solver.step(args.warmup)
        solver.dt[None] = 0.0
        ps.set_option(_lib.OPT_DEBUG_ABLATE, args.ablate_mask)
    if args.sweep:
        for impl, shape, fused in [(0, 0, 1), (1, 0, 1), (1, 1, 1), (1, 0, 0)]:
            dt, tm = run(impl, shape, fused, max(args.steps // 4, 10), 5)
            k = max(tm.steps, 1)
            print(f"[sweep] impl={impl} shape={shape} fused={fused}: {dt / max(args.steps // 4, 10) * 1e3:.3f} ms/step "
                  f"sort={tm.sort_ms / k:.3f} neigh={tm.neighbour_ms / k:.3f} force={tm.force_ms / k:.3f} "
                  f"integ={tm.integrate_ms / k:.3f}", file=sys.stderr, flush=True)

    if args.ablate:
        # same particle state for every variant: sweeps only (no advect), positions frozen by dt = 0
        solver.step(args.warmup)
        solver.dt[None] = 0.0
        for mask, what in [(0, "full"), (1, "no phase 2"), (2, "no list write-out (force sweep reads stale lists)"),
                           (128, "force: no neighbour gather (profiling build, -DSPH_PROFILE)"),
                           (16, "filter only, no hit emitted"), (32, "no pair term in the emission loop"), (34, "emission: bit loop only"),
                           (4, "no phase 1"), (7, "staging + target setup only")]:
            ps.set_option(_lib.OPT_DEBUG_ABLATE, mask)
            dt, tm = run(args.gather_impl, args.brick_shape, 1, 20, 2)
            kk = max(tm.steps, 1)
            print(f"[ablate {mask}] {what:32s} neigh={tm.neighbour_ms / kk:.3f} force={tm.force_ms / kk:.3f}",
                  file=sys.stderr, flush=True)
        ps.set_option(_lib.OPT_DEBUG_ABLATE, 0)
        solver.dt[None] = CFG["timeStepSize"]
    if args.solver == "dfsph":
        import numpy as np
        if args.full:
            pid0 = ps.pid.to_numpy()
            x_by_pid = np.empty_like(ps.x.to_numpy()); x_by_pid[pid0] = ps.x.to_numpy()
            v_by_pid = np.empty_like(ps.v.to_numpy()); v_by_pid[pid0] = ps.v.to_numpy()
        it0 = solver.stats()
        dt, tm = run(args.gather_impl, args.brick_shape, 1, args.steps, args.warmup)
        it1 = solver.stats()
        if args.dump_outputs:
            dump_outputs(ps, args.dump_outputs)
        runahead_ab = None
        if args.full:
            # A/B on the same box over the SAME steps (the run is deterministic: the initial state is restored by persistent id):
            # the solver loops running AHEAD of their convergence tests (SPH_OPT_DF_RUNAHEAD 1: iteration k + 1 enqueued before
            # the host waits for iteration k's device-side test) against the default above (enqueue, wait, decide)
            pid = ps.pid.to_numpy()
            ps.x.from_numpy(x_by_pid[pid]); ps.v.from_numpy(v_by_pid[pid])
            solver.initialize()
            ps.set_option(_lib.OPT_DF_RUNAHEAD, 1)
            dt_ab1, _ = run(args.gather_impl, args.brick_shape, 1, args.steps, args.warmup)
            it2 = solver.stats()
            ps.set_option(_lib.OPT_DF_RUNAHEAD, 0)
            dt_ab0 = dt
            same_counts = (it2["total_iterations_v"] - it1["total_iterations_v"] == it1["total_iterations_v"] - it0["total_iterations_v"] and
                           it2["total_iterations"] - it1["total_iterations"] == it1["total_iterations"] - it0["total_iterations"])
            runahead_ab = {"ms_per_step_host_round_trip_per_iteration": round(dt_ab0 / args.steps * 1e3, 4),
                           "ms_per_step_run_ahead": round(dt_ab1 / args.steps * 1e3, 4),
                           "same_iteration_counts": bool(same_counts),
                           "note": "the same W + K steps from the restored initial state with SPH_OPT_DF_RUNAHEAD 1; "
                                   "host_round_trip_per_iteration = the line's own block (the default).  The second block starts "
                                   "from the same positions and velocities in ANOTHER particle order (the one the first block ended in; "
                                   "the stable sort keeps ties in their previous order), so its f32 sums differ in the last bit and "
                                   "same_iteration_counts holds only until round-off moves one convergence test (~40 steps at 1.75 M); "
                                   "bit-identity of the two modes on one order: test_dfsph_solver_loops_running_ahead_of_their_convergence_tests"}
        k = max(int(tm.steps), 1)
        iv = (it1["total_iterations_v"] - it0["total_iterations_v"]) / (args.warmup + args.steps)
        ip = (it1["total_iterations"] - it0["total_iterations"]) / (args.warmup + args.steps)
        sweeps = 2 + (1 + 2 * iv) + 1 + (1 + 2 * ip)     # density, factor | divergence solve | forces | pressure solve
        line = {
            "metric": "DFSPH steps/sec at 1.74 M particles (supplementary; BASELINE.json's metric is the WCSPH step)",
            "value": round(args.steps / dt * N / REF_PARTICLES, 3), "unit": "steps/s", "n_gpus": 1,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": args.workload, "solver": "dfsph", "particles": N, "cells": G, "dt": DFSPH_DT,
                       "gather_impl": args.gather_impl, "brick_records": args.brick_records, "parallelism": "1 GPU"},
            "breakdown_ms": {"sort": round(tm.sort_ms / k, 4), "neighbour": round(tm.neighbour_ms / k, 4),
                             "force": round(tm.force_ms / k, 4), "integrate": round(tm.integrate_ms / k, 4),
                             "sum_of_phases": round(tm.total_ms / k, 4)},
            "dfsph": {"divergence_iterations_per_step": round(iv, 2), "pressure_iterations_per_step": round(ip, 2),
                      "neighbour_sweeps_per_step": round(sweeps, 2),
                      "ms_per_sweep": round((tm.neighbour_ms + tm.force_ms) / k / sweeps, 4),
                      "simulated_time_per_wall_second": round(args.steps / dt * DFSPH_DT, 3),
                      "runahead_ab": runahead_ab},
            "roofline": None,
        }
        # The step is ~37 neighbour sweeps over unchanged positions; all but the first read the neighbour lists.  Algorithmic
        # bytes of ONE list-reading Jacobi sweep (DFSPH.py:285-321 / 356-394), minimal-fused like SURVEY 8(d)'s WCSPH rows: read
        # x 12, v 12, (factor, density_adv) 8, m_V 4, material / is_dynamic 8; write v 12 => 56 N + 4 G.  Duration = the mean
        # over ALL sweeps of the step (HIP events of the neighbour + force buckets / sweeps, read-backs included), so the
        # fraction is a lower bound for the Jacobi sweeps themselves (111-113 us in the kernel trace).
        ms_sweep = line["dfsph"]["ms_per_sweep"]
        ab = 56.0 * N + 4.0 * G
        # counter traffic of the Jacobi sweep (profiles/pmc_traffic_dfsph.json: tools/gpu_pmc.sh over this command line +
        # tools/refresh_pmc.py --solver dfsph), quoted only for the kernel sources this library was built from
        traffic, traffic_note, per_kernel = None, "no PMC file for this revision", None
        try:
            from sph_taichi_amd import build as _build
            pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic_dfsph.json")))
            if pm.get("kernel_fingerprint") != _build._fingerprint():
                traffic_note = "profiles/pmc_traffic_dfsph.json was measured on other kernel sources (fingerprint differs): not quoted"
            elif pm.get("workload") != args.workload:
                traffic_note = "profiles/pmc_traffic_dfsph.json covers another workload: not quoted"
            else:
                ks = pm["kernels"]
                per_kernel = {k_: {"traffic": v["fetch_kb"] * 1024 * 2 + v["write_kb"] * 1024, "dispatches": v.get("dispatches")}
                              for k_, v in ks.items() if "GM_DF" in k_ and "fetch_kb" in v and "write_kb" in v}
                it = per_kernel.get("k_gather_brick<GM_DF_DIV_ITER_U>") or per_kernel.get("k_gather_brick<GM_DF_DIV_ITER>")
                traffic = it["traffic"] if it else None
                traffic_note = (f"profiles/pmc_traffic_dfsph.json ({pm.get('source')}), same kernel fingerprint; mean over ALL dispatches of "
                                "the divergence solver's Jacobi sweep, i.e. including the ones enqueued past convergence, which leave at once")
        except Exception as e:      # noqa: BLE001
            traffic_note = f"PMC file unusable ({type(e).__name__})"
        if ms_sweep > 0:
            ach = ab / (ms_sweep * 1e-3) / 1e9
            line["roofline"] = {"kernel": "k_gather_brick<GM_DF_*_ITER_U> (list-reading Jacobi sweep; mean over the step's sweeps)",
                                "bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": round(ach / HBM_PEAK_GBS, 5), "traffic": traffic, "alg_bytes_per_launch": ab,
                                "avg_launch_ms": ms_sweep, "counters": traffic_note, "traffic_by_kernel": per_kernel,
                                "note": "gather sweeps are VALU- / vector-memory-bound, not HBM-bound (DESIGN.md section 4)"}
        ps.close()
        line["cpu_baseline"] = cpu_baseline(sd, args.cpu_steps) if args.full and args.cpu_steps > 0 else None
        print(json.dumps(line), flush=True)
        return
    # ---- the headline line: state A = from rest, state B = the same box settled ----
    # Counter-derived figures (HBM bytes, VALU instruction counts) come from the committed rocprofv3 PMC passes
    # (profiles/pmc_traffic.json, tools/gpu_pmc.sh + tools/refresh_pmc.py).  They are quoted ONLY when that file was
    # measured on the kernel sources this library was built from (same fingerprint), on this workload and variant;
    # otherwise they are null -- never a number from another revision next to a live launch time.
    pmc_states = {}
    pmc_note = "no PMC file for this revision"
    try:
        from sph_taichi_amd import build as _build
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        if pm.get("kernel_fingerprint") != _build._fingerprint():
            pmc_note = "profiles/pmc_traffic.json was measured on other kernel sources (fingerprint differs): not quoted"
        elif not (pm["workload"] == args.workload and args.gather_impl == 1 and args.brick_shape == 0 and args.fused == 1
                  and args.variant == -1 and args.settle == 0):
            pmc_note = "profiles/pmc_traffic.json covers the default line only (workload / variant / state differ): not quoted"
        else:
            pmc_states = pm.get("states") or {"rest": pm["kernels"]}
            pmc_note = f"profiles/pmc_traffic.json ({pm.get('source')}), same kernel fingerprint"
    except Exception as e:
        pmc_note = f"PMC file unusable ({type(e).__name__})"
    one_gather = None
    VALU_PEAK_GINST = 1024 * 2.4 / 2.0

    def report(dt, tm, steps, state):
        """value / breakdown / rooflines of one timed block (`state` selects the PMC table: "rest" or "settled")."""
        nonlocal one_gather
        k = max(int(tm.steps), 1)
        ms_per_step = dt / steps * 1e3
        force_ms, neigh_ms = tm.force_ms / k, tm.neighbour_ms / k
        # Per-launch algorithmic bytes: density+EOS sweep 32 N + 4 G, fused force sweep 60 N + 4 G.  With no
        # dynamic rigid body each phase is one sweep launch (+ the brick-list kernel in the neighbour phase, ~12 us):
        # the HIP-event phase time is an upper bound of the sweep's duration, the rocprofv3 kernel trace has the kernel alone.
        kernels = {"k_gather_brick<GM_DENSITY_EOS>": (32.0 * N + 4.0 * G, neigh_ms),
                   "k_gather_brick<GM_FORCE_FUSED>": (60.0 * N + 4.0 * G, force_ms)}
        if one_gather is None:
            one_gather = ps.get_option(_lib.OPT_UNIFORM_FLUID_STATE) == 1 and args.fused == 1
        if one_gather:      # the force sweep that actually ran (SPH_OPT_UNIFORM_FLUID: all fluid masses equal)
            kernels["k_gather_brick<GM_FORCE_FUSED_U>"] = kernels.pop("k_gather_brick<GM_FORCE_FUSED>")
        if not args.gather_impl:
            kernels = {k_.replace("brick", "simple"): v for k_, v in kernels.items()}
        pmc_k = pmc_states.get(state, {})
        rk = {}
        for k_, (ab, ms) in kernels.items():
            e = {"alg_bytes": ab, "avg_launch_ms": round(ms, 4), "achieved_GBs": round(ab / (ms * 1e-3) / 1e9, 2) if ms > 0 else 0.0,
                 "frac_of_hbm_peak": round(ab / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if ms > 0 else 0.0,
                 "traffic": None, "traffic_over_alg": None}
            if k_ in pmc_k and "fetch_kb" in pmc_k[k_] and "write_kb" in pmc_k[k_]:
                e["traffic"] = pmc_k[k_]["fetch_kb"] * 1024 * 2 + pmc_k[k_]["write_kb"] * 1024
                e["traffic_over_alg"] = round(e["traffic"] / ab, 2)
                if pmc_k[k_].get("valu_wave_insts") and ms > 0:
                    wi = pmc_k[k_]["valu_wave_insts"]
                    e["valu_wave_insts"] = wi
                    e["valu_issue_frac"] = round(wi / (ms * 1e-3) / 1e9 / VALU_PEAK_GINST, 4)
            rk[k_] = e
        # ALWAYS the density + EOS sweep: by the committed kernel trace (profiles/r05f_kernel_stats_c3p_rest.csv and the r06 one) it
        # is the kernel with the largest duration in both states.  Never an argmax over two phase times 0.1 % apart: that made
        # the object flip to the force sweep between rounds and its fraction double with no kernel faster;
        # the force sweep has its own object, `roofline_force`.
        dominant = next(k_ for k_ in kernels if "DENSITY" in k_)
        st = _lib.SphStats()
        ps._call("sph_get_stats", st)
        step_bytes = 360.0 * N + 20.0 * G
        return {
            "value": round(steps / dt * N / REF_PARTICLES, 3), "ms_per_step": round(ms_per_step, 4),
            "steps_timed": steps,
            "breakdown_ms": {"sort": round(tm.sort_ms / k, 4), "neighbour": round(neigh_ms, 4), "force": round(force_ms, 4),
                             "integrate": round(tm.integrate_ms / k, 4), "sum_of_phases": round(tm.total_ms / k, 4)},
            "dominant": dominant, "roofline_kernels": rk,
            "roofline_step": {"alg_bytes": step_bytes, "achieved_GBs": round(step_bytes / (ms_per_step * 1e-3) / 1e9, 2),
                              "frac": round(step_bytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)},
            "neighbourhood": {
                "mean_list_entries": round(st.list_entries / max(st.targets - st.list_overflow_targets - st.lds_overflow_targets, 1), 2),
                "max_list_entries": st.max_list, "list_overflow_targets": st.list_overflow_targets,
                "lds_overflow_targets": st.lds_overflow_targets, "max_cell_occupancy": st.max_cell_occupancy,
                "mean_cell_occupancy": round(N / max(st.nonempty_cells, 1), 2)},
        }

    # State A.  The contract's timed region: W untimed + exactly K timed steps.  A plain run times that one block.  With
    # --full, since K = 20 is 8 ms of GPU time, too short for anything outside this process to see, the block is REPEATED
    # from the same initial state (positions and velocities re-uploaded by persistent id, untimed) until >= 0.5 s of timed
    # steps have run; the line reports the mean over the repetitions (`reps`) and the first one beside it.
    import numpy as np
    restore = args.full and args.settle == 0 and not args.ablate_mask
    if restore:
        x0, v0 = ps.x.to_numpy(), ps.v.to_numpy()
        pid0 = ps.pid.to_numpy()
        x_by_pid = np.empty_like(x0); x_by_pid[pid0] = x0
        v_by_pid = np.empty_like(v0); v_by_pid[pid0] = v0
    blocks = []
    t_timed, reps = 0.0, 0
    cold = None
    if restore and args.preheat_ms > 0:     # one block straight after the host-side idle, reported beside the others
        dt, tm = run(args.gather_impl, args.brick_shape, args.fused, args.steps, args.warmup, heat_ms=0.0)
        cold = report(dt, tm, args.steps, "rest")
        pid = ps.pid.to_numpy()
        ps.x.from_numpy(x_by_pid[pid]); ps.v.from_numpy(v_by_pid[pid])
        solver.initialize()
    while True:
        dt, tm = run(args.gather_impl, args.brick_shape, args.fused, args.steps, args.warmup)
        blocks.append((dt, tm))
        t_timed += dt
        reps += 1
        if not restore or t_timed >= args.min_seconds or reps >= args.max_reps:
            break
        pid = ps.pid.to_numpy()
        ps.x.from_numpy(x_by_pid[pid]); ps.v.from_numpy(v_by_pid[pid])
        solver.initialize()
    if args.dump_outputs:
        dump_outputs(ps, args.dump_outputs)
    dt_mean = sum(b[0] for b in blocks) / len(blocks)
    tm_sum = _lib.SphTimings()
    for _, tm in blocks:
        for f in ("sort_ms", "neighbour_ms", "force_ms", "integrate_ms", "total_ms", "steps"):
            setattr(tm_sum, f, getattr(tm_sum, f) + getattr(tm, f))
    rest = report(dt_mean, tm_sum, args.steps, "settled" if args.settle else "rest")
    first = report(blocks[0][0], blocks[0][1], args.steps, "rest")
    dominant = rest["dominant"]
    dk = rest["roofline_kernels"][dominant]
    flop_per_particle = 2300.0 if "DENSITY" in dominant else 4600.0
    dom_ms = dk["avg_launch_ms"]
    # VALU roofline of the same kernel.  Peak issue rate: 1024 SIMD-32 x 2.4 GHz / 2 cycles per wave64 instruction
    # (MI355X_MICROARCH.md; measured here 0.85-0.9 G wave-instructions/s per SIMD at the clock the chip sustains,
    # profiles/archive/r02a_ubench_valu_table1.txt -- and half / a quarter of that for the 4- and 8-cycle opcode classes).
    # Useful work: SURVEY 8d's ~2.3 kFLOP (density) / ~4.6 kFLOP (force) per particle against 157.3 TFLOP/s.
    roofline_valu = {"kernel": dominant, "unit": "G wave-instructions/s", "peak": VALU_PEAK_GINST,
                     "peak_measured_full_rate_ops": round(1024 * 0.875, 1),
                     "useful_tflops": round(flop_per_particle * N / (dom_ms * 1e-3) / 1e12, 2) if dom_ms > 0 else None,
                     "peak_tflops": 157.3, "achieved": None, "frac": dk.get("valu_issue_frac"),
                     "valu_wave_insts_per_launch": dk.get("valu_wave_insts"), "insts_per_particle": None, "source": pmc_note}
    if dom_ms > 0:
        roofline_valu["useful_frac_of_fp32_peak"] = round(roofline_valu["useful_tflops"] / 157.3, 4)
    if dk.get("valu_wave_insts") and dom_ms > 0:
        roofline_valu.update(achieved=round(dk["valu_wave_insts"] / (dom_ms * 1e-3) / 1e9, 1),
                             insts_per_particle=round(dk["valu_wave_insts"] * 64 / N, 1))
    line = {
        "metric": "WCSPH steps/sec at 1.74 M particles (+ ms/step breakdown sort/neighbour/force)",
        "value": rest["value"], "unit": "steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": rest["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": args.workload, "particles": N, "cells": G, "dt": CFG["timeStepSize"],
                   "gather_impl": args.gather_impl, "brick_shape": args.brick_shape, "fused": args.fused,
                   "kernel_variant": ps.get_option(_lib.OPT_KERNEL_VARIANT), "brick_records": args.brick_records, "parallelism": "1 GPU",
                   "settle_steps": args.settle, "state": "settled" if args.settle else "from rest (steps W..W+K of the initial lattice)",
                   "full": args.full},
        "reps": reps, "timed_seconds": round(t_timed, 3),
        "first_rep": {"value": first["value"], "ms_per_step": first["ms_per_step"]},
        "preheat_ms": 0.0 if _HEAT.get("broken") else args.preheat_ms,
        "cold_block": None if cold is None else {
            "value": cold["value"], "ms_per_step": cold["ms_per_step"], "breakdown_ms": cold["breakdown_ms"],
            "note": "the same W + K steps started straight after the host-side set-up, GPU idle before them (no preheat): the "
                    "clock ramp of the first milliseconds is inside the timed region"},
        "breakdown_ms": rest["breakdown_ms"],
        "phase_events": {"every": args.time_every,
                         "note": "breakdown_ms and roofline.avg_launch_ms are HIP-event means over every k-th step of the timed region "
                                 "(five event records per step cost 4 % of it, DESIGN.md section 5); value / ms_per_step are the wall clock "
                                 "of all K steps between two device synchronisations"},
        "steps_per_s_job": round(args.steps / dt_mean, 3),
        "roofline": {"kernel": dominant, "bound": "hbm", "achieved": dk["achieved_GBs"], "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": dk["frac_of_hbm_peak"], "traffic": dk["traffic"],
                     "alg_bytes_per_launch": dk["alg_bytes"], "avg_launch_ms": dk["avg_launch_ms"],
                     "counters": pmc_note,
                     "note": "fraction of the HBM roof on ALGORITHMIC bytes, as the contract asks; the sweep itself is "
                             "bound by VALU issue and the LDS / vector-memory pipes (roofline_valu, DESIGN.md section 4), "
                             "so this fraction measures how far the sweep is from a pure streaming pass, not HBM "
                             "saturation; traffic = rocprofv3 FETCH_SIZE*2 + WRITE_SIZE per launch; avg_launch_ms is the "
                             "HIP-event time of the phase the kernel runs in (neighbour phase = brick-list kernel + sweep)"},
        "roofline_force": None,
        "roofline_valu": roofline_valu,
        "roofline_kernels": rest["roofline_kernels"],
        "roofline_step": rest["roofline_step"],
        "neighbourhood": dict(rest["neighbourhood"], note="last density sweep of the timed region (sph_get_stats); list entries = superset filter incl. self"),
    }
    fk_name = next(k_ for k_ in rest["roofline_kernels"] if "FORCE" in k_)
    fk = rest["roofline_kernels"][fk_name]
    line["roofline_force"] = {
        "kernel": fk_name, "bound": "hbm", "achieved": fk["achieved_GBs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": fk["frac_of_hbm_peak"], "traffic": fk["traffic"], "alg_bytes_per_launch": fk["alg_bytes"],
        "avg_launch_ms": fk["avg_launch_ms"], "counters": pmc_note,
        "bytes_as_moved": {"note": "the fraction is quoted on SURVEY 8(d)'s minimal-fused force row, 60 N + 4 G (read x, v, m_V, density, "
                                   "pressure, flags of the target + write its acceleration), as the contract asks.  What THIS launch moves is "
                                   "not that row: inside sph_step(K) the sweep has absorbed the fluid's advect + wall pass (read / write x, v: "
                                   "68 N more), and on every step of a call but the last it does NOT write the acceleration out (skip_acc: the "
                                   "field is dead until the next step rewrites it; 16 N less) -- parity-neutral, but neither the "
                                   "reference-shaped step's bytes nor this kernel's.",
                           "absorbed_advect_bytes": 68.0 * N, "acceleration_store_skipped_bytes": 16.0 * N,
                           "alg_bytes_of_sweep_plus_absorbed_advect": fk["alg_bytes"] + 68.0 * N}}
    # State B: the same box after `--settled-after` untimed steps (the fluid has sunk to its rest density: 10 particles
    # per cell instead of the lattice's 8, 43 neighbours instead of 33) -- what a long run sees.  One contiguous block
    # of at least K steps and at least --min-seconds.
    if args.full and args.settle == 0 and args.settled_after > 0 and not args.ablate_mask:
        ps.set_option(_lib.OPT_TIMING, 0)
        solver.step(args.settled_after)
        ps.sync()
        dt_probe, _ = run(args.gather_impl, args.brick_shape, args.fused, args.steps, args.warmup)
        n_set = max(args.steps, int(np.ceil(args.min_seconds / max(dt_probe / args.steps, 1e-9))))
        n_set = min(n_set, args.steps * args.max_reps)
        dt_s, tm_s = run(args.gather_impl, args.brick_shape, args.fused, n_set, 0)
        settled = report(dt_s, tm_s, n_set, "settled")
        settled.pop("dominant")
        settled["after_steps"] = args.settled_after + 2 * args.warmup + args.steps
        settled["timed_seconds"] = round(dt_s, 3)
        line["settled"] = settled
    ps.close()
    # The spread a reader of the parsed line alone should see: `value` = mean of the preheated blocks;
    # value_single_block = ONE literal "W warm-up + K timed steps" block straight after set-up, no preheat (= cold_block).
    line["value_single_block"] = (cold or first)["value"]
    if (args.full and args.with_bodies and args.workload == "c3p_uniform_1.75M" and args.settle == 0 and not args.ablate_mask
            and args.gather_impl == 1 and args.fused == 1):
        try:
            line["with_bodies"] = with_bodies(args, local_rank)
        except Exception as e:      # noqa: BLE001 -- a supplementary object never costs the headline line
            line["with_bodies"] = {"error": f"{type(e).__name__}: {e}"}
    # ... and as top-level scalars, so that a reader of the parsed line alone sees all four numbers (VERDICT r04 "weak" #8):
    # value (mean of the preheated blocks from rest) >= value_single_block >= value_with_bodies / value_settled
    line["value_settled"] = line["settled"]["value"] if isinstance(line.get("settled"), dict) else None
    line["value_with_bodies"] = (line["with_bodies"].get("value") if isinstance(line.get("with_bodies"), dict) else None)
    # ... and inside `config`, which every parser of the contract line keeps (the top-level extras landed in
    # `extra_keys` without their values)
    line["config"].update(value_is="mean of `reps` preheated W+K blocks from the rest lattice",
                          value_single_block=line["value_single_block"], value_settled=line["value_settled"],
                          value_with_bodies=line["value_with_bodies"])
    if args.full and args.cpu_steps > 0:
        line["cpu_baseline"] = cpu_baseline(sd, args.cpu_steps)
    else:
        line["cpu_baseline"] = None
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
