"""Headless counterpart of the reference's run_simulation.py (argument parsing,
substep loop and exporters of /root/reference/run_simulation.py:12-35, 79-113).
There is no window (:37, 87, 118); what it would show -- camera, light, particles,
domain box of :39-74, 90-94 -- is rendered on the GPU into the frames that
`exportFrame` writes (:27-28, 96-98).

    python -m sph_taichi_amd.run_simulation --scene_file data/scenes/dragon_bath.json --frames 100

Per frame: `numberOfStepsPerRenderUpdate` solver steps; every int(0.016/dt)
frames optional ASCII-PLY particle export (`exportPly`), OBJ rigid-body export
(`exportObj`) and PNG frame export (`exportFrame`, without the objects listed in
`invisibleObjects`), written where the reference writes them.  `--timing` prints the
per-phase HIP-event breakdown (sort / neighbour / force / integrate).

A scene whose Configuration holds an "adaptiveTimeStep" object gets its dt from the CFL criteria of timestep.py, once per
frame (one reduction on the device and one host synchronisation; dt never changes inside a frame's steps).
`--diagnostics PATH` writes one JSON line per exported interval: frame, time, dt and the all-particle diagnostics row.
`--gauges PATH` writes one JSON line per exported interval from a column map of the fluid (columns.py): frame, time, the wet
extent (the front), selected / outside counts and, if the scene's Configuration holds
"gauges": {"axis": 1, "cell": c, "points": [[a, b], ...]}, depth / surface / velocity at those points; without the key the
defaults apply and no point rows are written.  `--heightmap_dir DIR` writes the map's surface elevation as an 8-bit grey PNG
per interval, scaled by the domain's extent along the map's axis.  Both are independent of `exportFrame` and `--diagnostics`;
with neither given no map is made.
A scene whose Configuration holds "exportParticles": {"objects": [0], "material": "fluid", "fields": ["velocity", "id"],
"box": [[lo], [hi]], "every": 1, "phase": 0} (every key optional; {} = every particle, positions only) writes
`{scene}_output/particles_{cnt_ply:06}.ply` per interval: a binary PLY whose vertices are selected, ordered by persistent id and
packed on the device (export.py), so vertex k is the same particle in every file.  `exportPly` is untouched.
`"frameStyle": "surface"` in the Configuration, or `--frame_style surface`, makes the `exportFrame` images surface frames
(ParticleSystem.render_surface: the fluid as one shaded surface over the solids) instead of the reference's spheres; an optional
"surfaceStyle": {"iterations", "filterRadius", "depthRange", "fluidColor", "absorb", "sky", "f0", "specular"} overrides the
defaults of render.SurfaceStyle.  Absent or "spheres": the frames are what they were.
`"frameColour": {"field": "speed", "range": [0, 3], "colormap": "heat", "material": "fluid", "objects": [0], "axisOrigin": 0}` (only
"field" is needed; `--frame_colour FIELD` is the short form) colours the selected particles of either frame style by a field
(render.FieldColour); without "range" each frame takes the range of its own particles, reduced on the device.  Each PNG then
carries field, lo, hi and colormap as tEXt chunks, and the final report holds `frame_colour_range`, the range of the last frame.
A Configuration with "sampleGrid": {"spacing": s, "origin": [..], "shape": [..], "fields": ["velocity", "pressure"], "objects": [0]}
(every key optional) writes `{scene}_output/grid_{cnt:06}.vtk` per exported interval: the fluid's fields interpolated on a regular
grid on the device (sample.py), a legacy binary STRUCTURED_POINTS volume ("gradients": ["velocity"] adds vorticity, divergence, Q and the fill gradient;
the same key in "probes" adds them to the rows).  "probes": {"points": [[x, y, z], ...], "fields": [...]}
with `--probes PATH` writes one JSON line per exported interval: frame, time and one row per point (count, fill, the fields).
Without the keys nothing changes.
A Configuration with "exportMesh": {"spacing": s, "origin": [..], "shape": [..], "iso": 0.4, "cap": true, "objects": [0]} (every key
optional) writes `{scene}_output/surface_{cnt:06}.ply` per exported interval: the fluid surface as an indexed triangle mesh with
normals, extracted on the device from such a grid (mesh.py), a binary PLY.
A Configuration with "tracers": {"points": [[x, y, z], ...]} or {"lattice": {"start": [..], "end": [..], "spacing": s}}, plus
"recordEvery" (default 1), "minFill" (default 0.2) and "objects", registers passive tracers after initialize() (tracers.py): they
are advected on the device inside every step, and `{scene}_output/tracers_{cnt:06}.vtk` per exported interval holds the pathlines
so far (legacy ASCII POLYDATA, one polyline per tracer, point data `time`); `--tracers out.vtk` writes the final pathlines.
A Configuration with "statistics": {"spacing": s, "origin": [..], "shape": [..], "objects": [0], "every": 10, "capacity": n,
"wet": 0.4} (every key optional) registers running flow statistics after initialize() (stats.py): every `every`-th step is sampled
on the device inside the step, and `{scene}_output/statistics.vtk` at the end of the run holds intermittency, mean fill, mean and
RMS velocity, turbulent kinetic energy and the Reynolds stresses on that grid (a legacy binary STRUCTURED_POINTS volume);
`--statistics out.vtk` writes the same file there as well.
A Configuration with "loads": {"objects": [1], "about": [x, y, z], "every": 1, "capacity": n} ("objects" required) registers fluid
loads after initialize() (loads.py): every `every`-th step samples the force and torque of the fluid on each listed solid object on
the device inside the step, and `{scene}_output/loads.csv` at the end of the run holds the series (one row per sample and object);
`--loads out.csv` writes the same file there as well.
A Configuration with "scalars": {"channels": ["dye"], "diffusivity": [1e-4], "values": {"0": [1.0]}, "sources": {"1": [350.0]},
"every": 10, "material": "fluid", "objects": [...], "paint": {"channel": 0, "range": [lo, hi], "colormap": "heat"}} (every key optional)
registers carried scalars after initialize() (scalars.py): they diffuse on the device inside the step, `{scene}_output/scalars_{cnt:06}.npz`
per exported interval holds ids and values, and with "paint" every exported frame shows the participants in the table colour of
their value; `--scalars DIR` writes the same files into DIR as well.
A Configuration with "features": {"every": 10, "material": "fluid", "objects": [0], "minNeighbours": 24, "normalMin": 0.0,
"export": "surface" | "all", "fields": [...], "paint": {"field": "vorticity", "range": [lo, hi], "colormap": "heat"}} (every key
optional) registers per-particle flow features after initialize() (features.py): every `every`-th step evaluates vorticity,
divergence, surface normal, kernel fill, neighbour counts and a free-surface flag at the particles on the device inside the step;
with "export", `{scene}_output/features_{cnt:06}.ply` per exported interval holds the latest sample (the surface shell alone, or
every target), and with "paint" every exported frame shows the targets in the table colour of that field; `--features DIR` writes
the same files into DIR as well.
`output_interval` stays the reference's expression on the configured `timeStepSize`.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import time

import numpy as np

from . import _lib
from .config_builder import SimConfig
from .particle_system import ParticleSystem


def write_ply_ascii(path: str, pos: np.ndarray):
    """Vertex-only ASCII PLY, the layout ti.tools.PLYWriter.export_frame_ascii produces."""
    with open(path, "w") as fh:
        fh.write("ply\nformat ascii 1.0\ncomment created by sph_taichi_amd\n")
        fh.write(f"element vertex {pos.shape[0]}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        np.savetxt(fh, pos, fmt="%.6f")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="SPH (MI355X)")
    ap.add_argument("--scene_file", default="", help="scene file")
    ap.add_argument("--frames", type=int, default=100, help="number of frames (the reference loops until the window closes)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--dump_npz", default="", help="write the final per-particle state here")
    ap.add_argument("--save_state", default="", help="write a restartable checkpoint (.npz) after the last frame")
    ap.add_argument("--load_state", default="", help="continue from a checkpoint written by --save_state")
    ap.add_argument("--diagnostics", default="", metavar="PATH",
                    help="write one JSON line per exported interval here: frame, time, dt, the all-particle diagnostics row")
    ap.add_argument("--gauges", default="", metavar="PATH",
                    help="write one JSON line per exported interval here: frame, time, wet extent, selected / outside, and the "
                         "scene's gauge points read off a column map")
    ap.add_argument("--probes", default="", metavar="PATH",
                    help="write one JSON line per exported interval here: frame, time and the scene's \"probes\" points sampled "
                         "from the fluid (count, fill, the fields)")
    ap.add_argument("--tracers", default="", metavar="PATH",
                    help="write the pathlines of the scene's \"tracers\" here after the last frame (legacy ASCII VTK polylines)")
    ap.add_argument("--statistics", default="", metavar="PATH",
                    help="write the running flow statistics of the scene's \"statistics\" grid here after the last frame (legacy binary VTK volume)")
    ap.add_argument("--loads", default="", metavar="PATH",
                    help="write the force / torque series of the scene's \"loads\" objects here after the last frame (CSV)")
    ap.add_argument("--features", default="", metavar="DIR",
                    help="write the per-particle feature files of the scene's \"features\" per exported interval into DIR as well (PLY)")
    ap.add_argument("--scalars", default="", metavar="DIR",
                    help="write the values of the scene's \"scalars\" per exported interval into DIR as well (npz of ids and values)")
    ap.add_argument("--heightmap_dir", default="", metavar="DIR",
                    help="write the column map's surface elevation as an 8-bit grey PNG per exported interval into DIR")
    ap.add_argument("--image_size", type=int, nargs=2, default=[1024, 1024], metavar=("W", "H"),
                    help="size of the exportFrame images (the reference's window is 1024 x 1024)")
    ap.add_argument("--camera", type=float, nargs=6, default=None, metavar=("EX", "EY", "EZ", "LX", "LY", "LZ"),
                    help="camera position and look-at point of the exportFrame images (default: the reference's window camera)")
    ap.add_argument("--frame_style", choices=["spheres", "surface"], default=None,
                    help="style of the exportFrame images: every particle a sphere (the reference's window), or the fluid as one "
                         "shaded surface over the solids (default: the scene's \"frameStyle\", else spheres)")
    ap.add_argument("--frame_colour", default=None, metavar="FIELD",
                    help="colour the fluid of the exportFrame images by a field (speed, vx, vy, vz, density, pressure, x, y, z) over its "
                         "range in each frame; short for the scene's \"frameColour\": {\"field\": FIELD}, which it overrides")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)

    scene_path = args.scene_file
    config = SimConfig(scene_file_path=scene_path)
    scene_name = scene_path.split("/")[-1].split(".")[0]
    substeps = config.get_cfg("numberOfStepsPerRenderUpdate")
    output_interval = int(0.016 / config.get_cfg("timeStepSize"))
    output_frames = config.get_cfg("exportFrame")
    output_ply = config.get_cfg("exportPly")
    output_obj = config.get_cfg("exportObj")
    series_prefix = "{}_output/particle_object_{}.ply".format(scene_name, "{}")
    if output_frames:
        os.makedirs(f"{scene_name}_output_img", exist_ok=True)
    from . import export as _export
    export_spec = _export.export_config(config)        # "exportParticles": None when the key is absent
    from . import sample as _sample
    grid_spec = _sample.sample_grid_config(config)     # "sampleGrid": None when the key is absent
    probes_spec = _sample.probes_config(config) if args.probes else None
    if args.probes and probes_spec is None:
        raise ValueError('--probes needs a "probes" object in the scene\'s Configuration')
    from . import mesh as _mesh
    mesh_spec = _mesh.mesh_config(config)              # "exportMesh": None when the key is absent
    from . import tracers as _tracers
    tracers_spec = _tracers.tracers_config(config)     # "tracers": None when the key is absent
    if args.tracers and tracers_spec is None:
        raise ValueError('--tracers needs a "tracers" object in the scene\'s Configuration')
    from . import stats as _stats
    stats_spec = _stats.statistics_config(config)      # "statistics": None when the key is absent
    if args.statistics and stats_spec is None:
        raise ValueError('--statistics needs a "statistics" object in the scene\'s Configuration')
    from . import loads as _loads
    loads_spec = _loads.loads_config(config)           # "loads": None when the key is absent
    if args.loads and loads_spec is None:
        raise ValueError('--loads needs a "loads" object in the scene\'s Configuration')
    from . import scalars as _scalars
    scalars_spec = _scalars.scalars_config(config)     # "scalars": None when the key is absent
    if args.scalars and scalars_spec is None:
        raise ValueError('--scalars needs a "scalars" object in the scene\'s Configuration')
    if scalars_spec is not None and args.scalars:
        os.makedirs(args.scalars, exist_ok=True)
    from . import features as _features
    features_spec = _features.features_config(config)  # "features": None when the key is absent
    if args.features and features_spec is None:
        raise ValueError('--features needs a "features" object in the scene\'s Configuration')
    if features_spec is not None and args.features:
        os.makedirs(args.features, exist_ok=True)
    if (output_ply or output_obj or export_spec is not None or grid_spec is not None or mesh_spec is not None or tracers_spec is not None
            or stats_spec is not None or loads_spec is not None or scalars_spec is not None or features_spec is not None):
        os.makedirs(f"{scene_name}_output", exist_ok=True)
    invisible_objects = config.get_cfg("invisibleObjects") or []
    camera = surface_style = None
    frame_style = args.frame_style or config.get_cfg("frameStyle") or "spheres"
    if frame_style not in ("spheres", "surface"):
        raise ValueError(f"frameStyle must be \"spheres\" or \"surface\", not {frame_style!r}")
    from .render import field_colour_from_config
    frame_colour = field_colour_from_config(args.frame_colour if args.frame_colour is not None else config.get_cfg("frameColour"))
    frame_colour_range = None
    if output_frames:
        from .render import Camera, surface_style_from_config, write_png
        if frame_style == "surface":
            surface_style = surface_style_from_config(config.get_cfg("surfaceStyle"))
        camera = Camera()
        if args.camera is not None:
            camera.eye, camera.lookat = tuple(args.camera[:3]), tuple(args.camera[3:])

    scene_dir = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(scene_path)))) or "."
    ps = ParticleSystem(config, GGUI=False, device=args.device, scene_dir=scene_dir, verbose=True)
    solver = ps.build_solver()
    solver.initialize()
    if args.load_state:
        meta = ps.load_state(args.load_state)
        print(f"restored {args.load_state} (frames done: {int(meta.get('frames', 0))})")
    if args.timing:
        ps.set_option(_lib.OPT_TIMING, 1)
    if tracers_spec is not None:
        m = tracers_spec["points"].shape[0]
        ps.set_tracers(tracers_spec["points"], min_fill=tracers_spec["min_fill"], record_every=tracers_spec["record_every"],
                       record_capacity=_tracers.history_capacity(m, args.frames * substeps, tracers_spec["record_every"]),
                       objects=tracers_spec["objects"])
    if stats_spec is not None:
        ps.set_statistics(**stats_spec)
    if loads_spec is not None:
        ps.set_loads(**loads_spec)
    if scalars_spec is not None:
        ps.set_scalars(**scalars_spec[0])
    if features_spec is not None:
        ps.set_features(**features_spec[0])
    controller = ps.build_time_step_controller(solver) if config.get_cfg("adaptiveTimeStep") is not None else None
    diag_out = open(args.diagnostics, "w") if args.diagnostics else None
    probes_out = open(args.probes, "w") if probes_spec is not None else None
    gauges = gauges_out = None
    if args.gauges or args.heightmap_dir:
        from . import columns as _columns
        from .render import write_png as write_heightmap
        gauges = _columns.gauges_config(config)
        gauges_out = open(args.gauges, "w") if args.gauges else None
        if args.heightmap_dir:
            os.makedirs(args.heightmap_dir, exist_ok=True)

    cnt = cnt_ply = frames_written = particle_files = grid_files = mesh_files = tracer_files = 0
    scalar_files = feature_files = 0
    render_s = export_s = 0.0
    t0 = time.perf_counter()
    for _ in range(args.frames):
        solver.step(substeps)
        diag = controller.update()[1] if controller is not None else None     # dt of the NEXT frame's steps
        if diag_out is not None and cnt % output_interval == 0:
            diag = diag if diag is not None else ps.diagnostics()
            diag_out.write(json.dumps({"frame": cnt, "time": diag.time, "dt": float(np.float32(solver.dt[None])),
                                       "total": diag.total.as_dict()}) + "\n")
        if gauges is not None and cnt % output_interval == 0:
            cmap = ps.column_map(axis=gauges["axis"], cell=gauges["cell"])
            if gauges_out is not None:
                ext = cmap.wet_extent()
                row = {"frame": cnt, "time": cmap.time, "wet_extent": [list(e) for e in ext] if ext is not None else None,
                       "selected": cmap.selected, "outside": cmap.outside}
                if gauges["points"]:
                    row["gauges"] = _columns.gauge_rows(cmap, gauges["points"])
                gauges_out.write(json.dumps(row) + "\n")
            if args.heightmap_dir:
                write_heightmap(os.path.join(args.heightmap_dir, f"{cnt:06}.png"),
                                _columns.heightmap_image(cmap, float(ps.domain_size[cmap.axis])))
        if grid_spec is not None and cnt % output_interval == 0:
            ps.sample_grid(**grid_spec).write_vtk(f"{scene_name}_output/grid_{cnt:06}.vtk")
            grid_files += 1
        if mesh_spec is not None and cnt % output_interval == 0:
            ps.surface_mesh(**mesh_spec).write_ply(f"{scene_name}_output/surface_{cnt:06}.ply", comments=(f"frame {cnt}",))
            mesh_files += 1
        if tracers_spec is not None and cnt % output_interval == 0:
            ps.tracers.write_vtk(f"{scene_name}_output/tracers_{cnt:06}.vtk")
            tracer_files += 1
        if scalars_spec is not None and cnt % output_interval == 0:
            ps.scalars.save(f"{scene_name}_output/scalars_{cnt:06}.npz")
            if args.scalars:
                ps.scalars.save(os.path.join(args.scalars, f"scalars_{cnt:06}.npz"))
            scalar_files += 1
            paint = scalars_spec[1]
            if paint is not None and output_frames:          # before the frame: the participants in the colour of their value
                ps.scalars.paint(paint["channel"], range=paint["range"], colormap=paint["colormap"])
        if features_spec is not None and cnt % output_interval == 0 and ps.features.info().samples > 0:
            out = features_spec[1]
            if out["export"] is not None:
                name = f"features_{cnt:06}.ply"
                for d in [f"{scene_name}_output"] + ([args.features] if args.features else []):
                    ps.features.write_ply(os.path.join(d, name), surface_only=out["export"] == "surface", fields=out["fields"])
                feature_files += 1
            paint = out["paint"]
            if paint is not None and output_frames:          # before the frame: the targets in the colour of the field
                ps.features.paint(paint["field"], range=paint["range"], colormap=paint["colormap"])
        if probes_out is not None and cnt % output_interval == 0:
            probes = ps.sample_points(**probes_spec)
            probes_out.write(json.dumps({"frame": cnt, "time": probes.time, "probes": probes.rows()}) + "\n")
        if output_frames and cnt % output_interval == 0:
            ps.sync()                          # the frame's cost, not the steps still in flight before it
            tr = time.perf_counter()
            coloured = {"colour": frame_colour} if frame_colour is not None else {}     # (without the key: the calls as they were)
            if surface_style is not None:
                img = ps.render_surface(camera=camera, invisible_objects=invisible_objects, size=tuple(args.image_size),
                                        style=surface_style, **coloured)
            else:
                img = ps.render(camera=camera, invisible_objects=invisible_objects, size=tuple(args.image_size), **coloured)
            render_s += time.perf_counter() - tr
            if frame_colour is not None:
                frame_colour_range = ps.frame_colour_range
                write_png(f"{scene_name}_output_img/{cnt:06}.png", img,
                          text={"field": frame_colour.field, "lo": repr(frame_colour_range[0]), "hi": repr(frame_colour_range[1]),
                                "colormap": frame_colour.colormap_name()})
            else:
                write_png(f"{scene_name}_output_img/{cnt:06}.png", img)
            frames_written += 1
        if cnt % output_interval == 0:
            if output_ply:
                obj_id = 0
                np_pos = ps.dump(obj_id=obj_id)["position"]
                write_ply_ascii(series_prefix.format(0).replace(".ply", f"_{cnt_ply:06}.ply"), np_pos)
            if export_spec is not None:
                ps.sync()                      # the file's cost, not the steps still in flight before it
                te = time.perf_counter()
                ps.export_particles(**export_spec).write_ply(f"{scene_name}_output/particles_{cnt_ply:06}.ply",
                                                             comments=(f"frame {cnt}",))
                export_s += time.perf_counter() - te
                particle_files += 1
            if output_obj:
                ps.update_kinematic_meshes()       # kinematic bodies ("motion"): the mesh at the current pose
                for r_body_id in ps.object_id_rigid_body:
                    with open(f"{scene_name}_output/obj_{r_body_id}_{cnt_ply:06}.obj", "w") as f:
                        f.write(ps.object_collection[r_body_id]["mesh"].export(file_type="obj"))
            cnt_ply += 1
        cnt += 1
    ps.sync()
    dt = time.perf_counter() - t0
    steps = args.frames * substeps
    report = {"scene": scene_name, "particles": ps.particle_max_num, "steps": steps,
              "steps_per_s": round(steps / dt, 2), "ms_per_step": round(dt / steps * 1e3, 4)}
    sim_time = C.c_double()
    ps._call("sph_get_time", C.byref(sim_time))            # the context's clock: the sum of the dt of every step made
    report["sim_time"] = sim_time.value
    if controller is not None:
        report["dt_min_used"], report["dt_max_used"] = controller.dt_min_used, controller.dt_max_used
    if diag_out is not None:
        diag_out.close()
    if gauges_out is not None:
        gauges_out.close()
    if probes_out is not None:
        probes_out.close()
    if grid_files:
        report["grid_files_written"] = grid_files
    if mesh_files:
        report["mesh_files_written"] = mesh_files
    if tracers_spec is not None:
        info = ps.tracers.info()
        report["tracer_files_written"] = tracer_files
        report["tracers"] = {"m": info.m, "advances": info.advances, "frames": info.frames, "dropped": info.dropped}
        if args.tracers:
            ps.tracers.write_vtk(args.tracers)
    if stats_spec is not None:
        info = ps.statistics.info()
        report["statistics"] = {"shape": list(info.shape), "every": info.every, "samples": info.samples, "dropped": info.dropped,
                                "steps_seen": info.steps_seen, "t_first": info.t_first, "t_last": info.t_last}
        ps.statistics.write_vtk(f"{scene_name}_output/statistics.vtk")
        if args.statistics:
            ps.statistics.write_vtk(args.statistics)
    if loads_spec is not None:
        info = ps.loads.info()
        report["loads"] = {"objects": list(ps.loads.objects), "every": info.every, "samples": info.samples, "dropped": info.dropped,
                           "steps_seen": info.steps_seen}
        ps.loads.write_csv(f"{scene_name}_output/loads.csv")
        if args.loads:
            ps.loads.write_csv(args.loads)
    if scalars_spec is not None:
        info = ps.scalars.info()
        report["scalars"] = {"channels": list(ps.scalars.channels), "every": info.every, "samples": info.samples, "steps_seen": info.steps_seen,
                             "overshoot": info.overshoot, "saturated": info.saturated, "files_written": scalar_files}
    if features_spec is not None:
        info = ps.features.info()
        report["features"] = {"every": info.every, "samples": info.samples, "steps_seen": info.steps_seen, "step": info.step,
                              "time": info.time, "files_written": feature_files}
    if frames_written:
        report["frames_written"] = frames_written
        report["render_ms_per_frame"] = round(render_s / frames_written * 1e3, 4)
        if frame_colour_range is not None:
            report["frame_colour_range"] = list(frame_colour_range)     # of the last frame
    if particle_files:
        report["particle_files_written"] = particle_files
        report["export_ms_per_file"] = round(export_s / particle_files * 1e3, 4)
    if args.timing:
        tm = _lib.SphTimings()
        ps._call("sph_get_timings", tm)
        k = max(int(tm.steps), 1)
        report["breakdown_ms"] = {"sort": tm.sort_ms / k, "neighbour": tm.neighbour_ms / k, "force": tm.force_ms / k,
                                  "integrate": tm.integrate_ms / k}
    print(json.dumps(report))
    if args.save_state:
        ps.save_state(args.save_state, frames=args.frames, scene=scene_name)
    if args.dump_npz:
        np.savez_compressed(args.dump_npz, **{f: getattr(ps, f).to_numpy() for f in
                                              ("object_id", "x", "v", "density", "pressure", "m_V", "pid")})
    ps.close()


if __name__ == "__main__":
    main()
