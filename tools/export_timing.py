#!/usr/bin/env python
"""What does a particle export cost, stage by stage, beside the path it replaces?  (DESIGN.md, section on the particle export)

On the benchmark's flagship workload (1,747,584 fluid particles, all of object 0), settled by `--settle` steps, in ONE process
and on one state, for an export of object 0 with positions only and one with all fields:
  device   : HIP events on the context's stream around `--inner` sph_export_select calls enqueued back to back (five launches
             each), and the host clock from sph_export_select to the return of sph_export_info (one synchronisation);
  download : the host clock of sph_export_download into a fresh numpy array;
  write    : the host clock of export.write_ply (header + data.tobytes()) into `--dir`;
  traffic  : the bytes the kernels are expected to move (csrc/sph_export.hip: record loads, table clear / write / two reads, row
             gather and row store) over the event time, beside the HBM peak the benchmark's rooflines use.
The pack kernel's two store forms (rows staged in LDS and stored as consecutive dwords / per-lane row stores) are timed on two
contexts of the same scene and state, the second created with SPH_EXPORT_PACK=direct in the environment.
Beside it the parent path for the same object: ps.dump(0) (downloads object_id, x and v of all particles, masks on the host)
plus run_simulation.write_ply_ascii (np.savetxt), `--parent-reps` times.
Medians with min / max.  A run without a GPU fails; nothing is estimated.

    python tools/export_timing.py --out profiles/export_timing.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench        # noqa: E402  (scene dictionaries of the benchmark's workloads)
from sph_taichi_amd import ParticleSystem, _lib, export  # noqa: E402
from sph_taichi_amd.benchutil import HBM_PEAK_GBS  # noqa: E402
from sph_taichi_amd.config_builder import SimConfig  # noqa: E402
from sph_taichi_amd.run_simulation import write_ply_ascii  # noqa: E402
from tools.columns_timing import hip_runtime, ok, stats  # noqa: E402

CASES = {"positions_only": (), "all_fields": ("velocity", "density", "pressure", "mass", "id", "object")}


def expected_bytes_per_particle(args: dict) -> dict:
    """Bytes per SELECTED record when every live record is selected and cold_capacity == N (the single-domain case)."""
    mask = args["mask"]
    mark = 16 + (16 if (args["material"] >= 0 or args["objects"]) else 0) + (16 if args["box"] is not None else 0)
    gather = 16 + (16 if mask & (2 | 64) else 0) + (16 if mask & (4 | 8 | 16 | 32) else 0)
    row = export.row_dtype(args["fields"]).itemsize
    parts = {"table_clear": 4, "mark_record_loads": mark, "mark_table_write": 4, "count_table_read": 4, "pack_table_read": 4,
             "pack_record_gather": gather, "pack_row_store": row}
    parts["total"] = sum(parts.values())
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", default="c3p_uniform_1.75M")
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--inner", type=int, default=10, help="selects per event pair")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-reps", type=int, default=2)
    ap.add_argument("--dir", default="", help="where the files are written (default: a temporary directory)")
    args = ap.parse_args()

    hip = hip_runtime()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    def context(pack):
        if pack == "direct":
            os.environ["SPH_EXPORT_PACK"] = "direct"     # read by the context's first select
        else:
            os.environ.pop("SPH_EXPORT_PACK", None)
        stream = C.c_void_p()
        ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
        ps = ParticleSystem(SimConfig(config=bench.scene_dict(args.workload)), stream=stream.value)
        solver = ps.build_solver()
        solver.initialize()
        solver.step(args.settle)
        ps.export_particles(objects=[0], fields=CASES["all_fields"])     # warm-up: allocations, the fold of the aux record
        ps.sync()
        return ps, stream

    def events(ps, stream, params):
        ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        for _ in range(args.inner):
            ps._call("sph_export_select", C.byref(params))
        ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value) / args.inner

    staged, stream_s = context("staged")
    direct, stream_d = context("direct")
    n = int(staged.particle_max_num)
    out_dir = args.dir or tempfile.mkdtemp(prefix="export_timing_")
    os.makedirs(out_dir, exist_ok=True)

    result = {"workload": args.workload, "particles": n, "settle_steps": args.settle, "hbm_peak_GBps": HBM_PEAK_GBS,
              "method": f"{args.reps} repetitions; device: {args.inner} selects per HIP-event pair on the context's stream, the two "
                        f"pack forms alternating; host stages by time.perf_counter after a sync; after {args.settle} settling steps "
                        "and one warm-up export", "cases": {}}
    reference_rows = {}
    for case, fields in CASES.items():
        a = export.select_args(objects=[0], fields=fields)
        params = export.make_params(a)
        dtype = export.row_dtype(a["fields"])
        t_staged, t_direct, t_info, t_down, t_write = [], [], [], [], []
        for _ in range(args.reps):
            t_staged.append(events(staged, stream_s, params))
            t_direct.append(events(direct, stream_d, params))
            staged.sync()
            t0 = time.perf_counter()
            info = export.select_info(staged, params)
            t1 = time.perf_counter()
            data = export.download_rows(staged, info, dtype)
            t2 = time.perf_counter()
            export.write_ply(os.path.join(out_dir, f"{case}.ply"), data)
            t3 = time.perf_counter()
            t_info.append((t1 - t0) * 1e3); t_down.append((t2 - t1) * 1e3); t_write.append((t3 - t2) * 1e3)
        assert info.selected == n == info.rows and info.duplicate_ids == 0, (info.selected, info.rows, info.duplicate_ids, n)
        other = direct.export_particles(objects=[0], fields=fields)
        assert other.data.tobytes() == data.tobytes(), "the two pack forms disagree"
        reference_rows[case] = data
        exp = expected_bytes_per_particle(a)
        dev = stats(t_staged)
        total_ms = statistics.median(t_info) + statistics.median(t_down) + statistics.median(t_write)
        result["cases"][case] = {
            "fields": list(a["fields"]), "row_bytes": dtype.itemsize, "rows": int(info.rows), "file_MB": round(data.nbytes / 1e6, 2),
            "device_select_events": dev, "device_select_events_direct_stores": stats(t_direct),
            "staged_over_direct": round(dev["median_ms"] / statistics.median(t_direct), 3),
            "select_to_info_host": stats(t_info), "download_host": stats(t_down), "write_ply_host": stats(t_write),
            "export_total_ms": round(total_ms, 3),
            "expected_bytes_per_particle": exp,
            "expected_traffic_MB": round(exp["total"] * n / 1e6, 1),
            "expected_traffic_over_hbm_peak_ms": round(exp["total"] * n / (HBM_PEAK_GBS * 1e9) * 1e3, 5),
            "effective_bandwidth_GBps": round(exp["total"] * n / (dev["median_ms"] * 1e-3) / 1e9, 1),
            "download_GBps": round(data.nbytes / (statistics.median(t_down) * 1e-3) / 1e9, 2),
        }

    # the parent path: whole-array downloads, a host mask, text
    t_dump, t_ascii = [], []
    for _ in range(args.parent_reps):
        staged.sync()
        t0 = time.perf_counter()
        pos = staged.dump(0)["position"]
        t1 = time.perf_counter()
        write_ply_ascii(os.path.join(out_dir, "parent_ascii.ply"), pos)
        t2 = time.perf_counter()
        t_dump.append((t1 - t0) * 1e3); t_ascii.append((t2 - t1) * 1e3)
    # same particles: the parent's rows are in the current cell-sorted order, the export's by id
    by_id = np.empty_like(pos)
    by_id[staged.pid.to_numpy()[staged.object_id.to_numpy() == 0]] = pos
    rows = reference_rows["positions_only"]
    assert np.array_equal(by_id, np.stack([rows["x"], rows["y"], rows["z"]], axis=1)), "the export and ps.dump(0) disagree"
    parent_ms = statistics.median(t_dump) + statistics.median(t_ascii)
    result["parent_path"] = {"dump_host": stats(t_dump), "write_ply_ascii_host": stats(t_ascii), "total_ms": round(parent_ms, 3),
                             "ascii_file_MB": round(os.path.getsize(os.path.join(out_dir, "parent_ascii.ply")) / 1e6, 2),
                             "dump_bytes_per_particle": 28}
    for case in CASES:
        result["cases"][case]["parent_over_export"] = round(parent_ms / result["cases"][case]["export_total_ms"], 1)
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    staged.close(); direct.close()


if __name__ == "__main__":
    main()
