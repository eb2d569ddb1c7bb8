#!/usr/bin/env python
"""What does the surface mesh cost?  (DESIGN.md, section on the surface mesh)

On the benchmark's flagship workload (1,747,584 fluid particles), settled by `--settle` steps, in ONE process and on one state,
the whole domain at spacing = the particle diameter (the 3.9 M nodes of profiles/sample_timing.json):
  (a) HIP events round sph_sample_grid with no field planes: the scatter that feeds the extraction (clear included);
  (b) HIP events round sph_mesh_extract (four kernels and its one synchronisation);
  (c) a host clock round sph_mesh_counts + sph_mesh_download, and round SurfaceMesh.write_ply;
the cases alternating.  `--trace-only` makes a few extracts and nothing else: run THAT under `rocprofv3 --kernel-trace` (a run of its own) and hand
the resulting rocpd database (or kernel_trace CSV) to a second, unprofiled run with `--kernel-trace` to have the per-kernel times
of k_mesh_* (and of k_sample_grid beside them) folded into the output; `--fold JSON` folds them into a file an earlier run wrote,
without a GPU.  A timing run without a GPU fails; nothing is estimated.

    rocprofv3 --kernel-trace -d out -o mesh -- python tools/mesh_timing.py --trace-only
    python tools/mesh_timing.py --kernel-trace out/mesh_results.db --out profiles/mesh_timing.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from rocpd_summary import rows_from_csv, rows_from_db  # noqa: E402

KERNELS = ("k_mesh_classify", "k_mesh_scan", "k_mesh_vertices", "k_mesh_faces")


def med(v):
    v = sorted(v)
    return {"median_ms": round(statistics.median(v), 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5), "repetitions": len(v)}


def kernel_stats(path):
    """{kernel: average / min / max ms, calls} of a rocprofv3 kernel trace for the mesh kernels and the sampler's scatter."""
    rows = rows_from_db(path) if path.endswith(".db") else rows_from_csv(path)
    out = {}
    for k in KERNELS + ("k_sample_grid", "k_sample_clear"):
        v = [t * 1e-6 for name, t in rows if k in name]
        if v:
            out[k] = {"average_ms": round(sum(v) / len(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5), "calls": len(v)}
    return out


def fold_kernels(out, path):
    ks = kernel_stats(path)
    out["kernels"] = ks
    out["kernels_sum_ms"] = round(sum(ks[k]["average_ms"] for k in KERNELS if k in ks), 5)
    out["kernels_source"] = "rocprofv3 --kernel-trace of a run of its own (--trace-only), over its calls (warm-up included)"
    if "k_sample_grid" in ks:
        out["kernels_sum_over_scatter_kernel"] = round(out["kernels_sum_ms"] / ks["k_sample_grid"]["average_ms"], 4)


def write(out, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", default="c3p_uniform_1.75M")
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iso", type=float, default=0.4)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kernel-trace", default="", metavar="DB_OR_CSV")
    ap.add_argument("--fold", default="", metavar="JSON", help="fold --kernel-trace into this earlier output and write --out; no GPU needed")
    ap.add_argument("--ply", default="", help="where the timed PLY goes (default: next to --out, removed afterwards)")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as fh:
            out = json.load(fh)
        fold_kernels(out, args.kernel_trace)
        write(out, args.out)
        return

    import bench        # (scene dictionaries of the benchmark's workloads)
    from sample_timing import hip_runtime, ok
    from sph_taichi_amd import ParticleSystem, _lib, mesh, sample
    from sph_taichi_amd.config_builder import SimConfig

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

    sel = sample.select_args(fields=())
    ga = mesh.grid_args(particle_diameter=ps.particle_diameter, domain_size=ps.domain_size)
    g = _lib.SphSampleGrid()
    g.n = (C.c_int32 * 3)(*ga["shape"])
    g.origin, g.spacing = (C.c_float * 3)(*ga["origin"]), (C.c_float * 3)(*ga["spacing"])
    g.inv_h, g.fields, g.select = sample.inv_h_f32(ps.support_radius), 0, sample.make_select(sel)
    spec = _lib.SphMeshSpec()
    spec.iso, spec.cap = args.iso, 1
    scatter = lambda: ps._call("sph_sample_grid", C.byref(g))
    extract = lambda: ps._call("sph_mesh_extract", C.byref(spec))

    def events(fn):
        ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        fn()
        ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value)

    for _ in range(2):                          # warm-up: allocations, code objects, clocks
        scatter(); extract()
    if args.trace_only:
        for _ in range(args.reps):
            scatter(); extract()
        ps.sync()
        ps.close()
        return

    ply = args.ply or (os.path.splitext(os.path.abspath(args.out))[0] + ".tmp.ply" if args.out else "mesh_timing.tmp.ply")
    t = {k: [] for k in ("scatter", "extract", "download", "write_ply")}
    sm = None
    for _ in range(args.reps):
        t["scatter"].append(events(scatter))
        t["extract"].append(events(extract))
        t0 = time.perf_counter()
        nv, nt = C.c_int64(), C.c_int64()
        ps._call("sph_mesh_counts", C.byref(nv), C.byref(nt))
        pos, nrm = np.empty((nv.value, 3), dtype=np.float32), np.empty((nv.value, 3), dtype=np.float32)
        tri = np.empty((nt.value, 3), dtype=np.int32)
        ps._call("sph_mesh_download", pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p), tri.ctypes.data_as(C.c_void_p), nv.value, nt.value)
        t1 = time.perf_counter()
        sm = mesh.SurfaceMesh(pos, nrm, tri, time=ps.time, iso=args.iso, origin=ga["origin"], spacing=ga["spacing"], shape=ga["shape"])
        sm.write_ply(ply)
        t2 = time.perf_counter()
        t["download"].append((t1 - t0) * 1e3)
        t["write_ply"].append((t2 - t1) * 1e3)
    if not args.ply:
        os.remove(ply)
    nodes = int(np.prod(ga["shape"]))
    V, T = int(sm.vertices.shape[0]), int(sm.triangles.shape[0])
    out = {
        "workload": args.workload, "particles": n, "settle_steps": args.settle, "iso": args.iso, "cap": True,
        "grid_shape": list(ga["shape"]), "grid_nodes": nodes, "grid_spacing": list(ga["spacing"]),
        "vertices": V, "triangles": T, "closed": sm.is_closed(), "volume": sm.volume(), "area": sm.area(),
        "bytes": {"weights_read_per_pass": 8 * nodes, "flags": nodes, "vertex_map": 4 * nodes, "mesh": 24 * V + 12 * T},
        "method": f"{args.reps} repetitions, the cases alternating, one call per HIP-event pair on the context's stream (scatter, extract) or per "
                  f"host-clock interval (download, write_ply), after {args.settle} settling steps and a warm-up round; the scatter is clear + "
                  "k_sample_grid with no field planes; the extract includes its one host synchronisation",
    }
    for k, v in t.items():
        out[k] = med(v)
    out["extract_over_scatter"] = round(out["extract"]["median_ms"] / out["scatter"]["median_ms"], 4)
    if args.kernel_trace:
        fold_kernels(out, args.kernel_trace)
    print(json.dumps(out), flush=True)
    if args.out:
        write(out, args.out)
    ps.close()


if __name__ == "__main__":
    main()
