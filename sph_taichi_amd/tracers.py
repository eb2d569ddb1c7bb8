"""Passive tracers: what `ParticleSystem.set_tracers()` registers and `ParticleSystem.tracers` is (include/sph_hip.h, section
"Passive tracers"; csrc/sph_tracers.hip).

Massless points that follow the flow: while a set is registered, every step of the device loop (`solver.step(n)`) moves each
tracer by dt times the Shepard mean of the velocity of the selected particles in the 27 cells around it, on the device, with
nothing crossing to the host.  A tracer whose Shepard sum stays below `min_fill` is dry for that step and stays where it is.  With
`record_every=k` every k-th advance also stores the positions in a device buffer of `record_capacity` frames, so that a
`solver.step(1000)` yields whole pathlines in one download.  Nothing in this module touches the GPU when it is imported.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import sample as _sample
from . import selection

MAX_TRACERS = 1 << 22
MAX_HISTORY_BYTES = 1 << 31
SCALE_LOG2 = 30
CONFIG_KEYS = ("points", "lattice", "recordEvery", "minFill", "objects")
LATTICE_KEYS = ("start", "end", "spacing")


def lattice(start, end, spacing) -> np.ndarray:
    """Seed points on a regular lattice, f32 [m, 3]: start_a + k * spacing_a for every k with start_a + k * spacing_a <= end_a
    (formed in f64, x slowest).  `spacing` is one number or one per axis."""
    def triple(value, name):      # f64: the count of an axis must not hang on the f32 rounding of its ends
        _sample._triple(value, name)
        a = np.asarray(value, dtype=np.float64).reshape(-1)
        return tuple(float(v) for v in (np.repeat(a, 3) if a.size == 1 else a))
    start, end, spacing = triple(start, "start"), triple(end, "end"), triple(spacing, "spacing")
    if not all(s > 0 for s in spacing):
        raise ValueError("spacing must be positive")
    if any(e < s for s, e in zip(start, end)):
        raise ValueError("end must not lie below start")
    counts = [int(np.floor((end[a] - start[a]) / spacing[a] + 1e-9)) + 1 for a in range(3)]
    if counts[0] * counts[1] * counts[2] > MAX_TRACERS:
        raise ValueError(f"{counts[0]} x {counts[1]} x {counts[2]} lattice points: a set holds at most {MAX_TRACERS} tracers")
    axes = [start[a] + np.arange(counts[a], dtype=np.float64) * spacing[a] for a in range(3)]
    g = np.meshgrid(*axes, indexing="ij")
    return np.stack([a.reshape(-1) for a in g], axis=1).astype(np.float32)


def points_arg(points) -> np.ndarray:
    """Tracer positions as a contiguous f32 [m, 3]; ValueError unless 1 <= m <= 2^22 and every coordinate is finite as f32."""
    try:
        p = np.asarray(points, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("points must be a list of [x, y, z] triples") from e
    if p.ndim == 1 and p.size == 3:
        p = p.reshape(1, 3)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be a list of [x, y, z] triples")
    if not 1 <= p.shape[0] <= MAX_TRACERS:
        raise ValueError(f"between 1 and {MAX_TRACERS} tracers can be set, not {p.shape[0]} (clear_tracers() removes the set)")
    with np.errstate(over="ignore"):
        f = np.ascontiguousarray(p, dtype=np.float32)
    if not np.isfinite(f).all():
        raise ValueError("points must be finite (as f32)")
    return f


def set_args(points, min_fill=0.2, record_every=0, record_capacity=0, material="fluid", objects=None) -> dict:
    """The arguments of `set_tracers`, checked without a context: {"points" f32 [m, 3], "min_fill", "record_every",
    "record_capacity", "material": -1 or the id, "objects": list}.  ValueError otherwise."""
    pts = points_arg(points)
    try:
        mf = float(np.float32(min_fill))
    except (TypeError, ValueError) as e:
        raise ValueError("min_fill must be a number") from e
    if not np.isfinite(mf) or not 0.0 < mf <= 4.0:
        raise ValueError("min_fill must be finite and in (0, 4]")
    every = selection.integer(record_every, "record_every")
    cap = selection.integer(record_capacity, "record_capacity")
    if every < 0 or cap < 0:
        raise ValueError("record_every and record_capacity must not be negative")
    if cap * pts.shape[0] * 12 > MAX_HISTORY_BYTES:
        raise ValueError(f"a history of {cap} frames of {pts.shape[0]} tracers takes more than 2^31 bytes")
    mat, ids = selection.parse(material, objects)
    return {"points": pts, "min_fill": mf, "record_every": every, "record_capacity": cap, "material": mat, "objects": ids}


def tracers_config(config):
    """The scene's "tracers" object in the Configuration: {"points": [[x, y, z], ...]} or {"lattice": {"start", "end", "spacing"}},
    plus "recordEvery" (default 1), "minFill" (default 0.2) and "objects".  Returns {"points", "min_fill", "record_every",
    "objects"} -- keyword arguments of `set_tracers` except for the capacity, which the run decides -- or None when the key is
    absent.  A misspelt key or a bad value raises ValueError."""
    spec = selection.config_object(config, "tracers", CONFIG_KEYS)
    if spec is None:
        return None
    if ("points" in spec) == ("lattice" in spec):
        raise ValueError('"tracers": give either points or lattice')
    try:
        if "lattice" in spec:
            lat = spec["lattice"]
            if not isinstance(lat, dict) or set(lat) != set(LATTICE_KEYS):
                raise ValueError(f"lattice must be an object with the keys {list(LATTICE_KEYS)}")
            pts = lattice(lat["start"], lat["end"], lat["spacing"])
        else:
            pts = spec["points"]
        a = set_args(pts, min_fill=spec.get("minFill", 0.2), record_every=spec.get("recordEvery", 1), objects=spec.get("objects"))
    except ValueError as e:
        raise ValueError(f'"tracers": {e}') from e
    return {"points": a["points"], "min_fill": a["min_fill"], "record_every": a["record_every"], "objects": spec.get("objects")}


def history_capacity(m: int, steps: int, record_every: int) -> int:
    """Frames a run of `steps` steps stores, cut to what the 2^31-byte history holds for m tracers."""
    if record_every <= 0:
        return 0
    return max(min(steps // record_every, MAX_HISTORY_BYTES // (12 * max(m, 1))), 0)


def write_vtk(path, paths, times, comment="tracer pathlines"):
    """Legacy ASCII POLYDATA: the points of `paths` [frames, m, 3] tracer by tracer, one polyline per tracer, point data `time`."""
    paths = np.asarray(paths, dtype=np.float32)
    if paths.ndim != 3 or paths.shape[2] != 3:
        raise ValueError("paths must be [frames, m, 3]")
    frames, m = paths.shape[0], paths.shape[1]
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    if times.shape[0] != frames:
        raise ValueError(f"{times.shape[0]} times for {frames} frames")
    pts = np.transpose(paths, (1, 0, 2)).reshape(-1, 3)            # tracer-major: the points of one line are consecutive
    with open(path, "w") as fh:
        fh.write(f"# vtk DataFile Version 3.0\n{comment}\nASCII\nDATASET POLYDATA\n")
        fh.write(f"POINTS {pts.shape[0]} float\n")
        np.savetxt(fh, pts, fmt="%.9g")
        n_lines = m if frames > 0 else 0
        fh.write(f"LINES {n_lines} {n_lines * (frames + 1)}\n")
        if n_lines:
            idx = np.arange(m * frames, dtype=np.int64).reshape(m, frames)
            np.savetxt(fh, np.concatenate([np.full((m, 1), frames, dtype=np.int64), idx], axis=1), fmt="%d")
        fh.write(f"POINT_DATA {pts.shape[0]}\nSCALARS time double 1\nLOOKUP_TABLE default\n")
        np.savetxt(fh, np.tile(times, m), fmt="%.17g")


def read_vtk(path):
    """What `write_vtk` wrote: (paths f32 [frames, m, 3], times f64 [frames])."""
    with open(path) as fh:
        tok = fh.read().split("\n")
    at = next(k for k, line in enumerate(tok) if line.startswith("POINTS "))
    n = int(tok[at].split()[1])
    pts = np.array([[float(v) for v in line.split()] for line in tok[at + 1:at + 1 + n]], dtype=np.float32).reshape(n, 3)
    at = next(k for k, line in enumerate(tok) if line.startswith("LINES "))
    m = int(tok[at].split()[1])
    lines = [[int(v) for v in line.split()] for line in tok[at + 1:at + 1 + m]]
    frames = lines[0][0] if m else 0
    for k, line in enumerate(lines):
        if line != [frames] + list(range(k * frames, (k + 1) * frames)):
            raise ValueError(f"{path}: polyline {k} is not the points of tracer {k}")
    at = next(k for k, line in enumerate(tok) if line.startswith("LOOKUP_TABLE"))
    t = np.array([float(line) for line in tok[at + 1:at + 1 + n]], dtype=np.float64)
    if m == 0:
        return np.zeros((0, 0, 3), np.float32), np.zeros(0)
    return np.transpose(pts.reshape(m, frames, 3), (1, 0, 2)).copy(), t[:frames].copy()


class TracerInfo:
    def __init__(self, m, advances, frames, dropped):
        self.m, self.advances, self.frames, self.dropped = int(m), int(advances), int(frames), int(dropped)

    def __repr__(self):
        return f"TracerInfo(m={self.m}, advances={self.advances}, frames={self.frames}, dropped={self.dropped})"


class Tracers:
    """The registered set of a ParticleSystem.  Every accessor downloads (and synchronises); `info()` does not."""

    def __init__(self, ps, m, record_every, record_capacity):
        self._ps = ps
        self.m, self.record_every, self.record_capacity = int(m), int(record_every), int(record_capacity)
        self.times = []          # simulated time of each stored history frame: the end of the step that stored it
        self._advances = 0       # the host's copy of info().advances, brought up to date behind every step call

    def _ptr(self, a):
        return a.ctypes.data_as(C.c_void_p)

    def _download(self, **want):
        m = self.m
        arrs = {"x": np.empty((m, 3), np.float32), "u": np.empty((m, 3), np.float32), "weight": np.empty(m, np.int64),
                "count": np.empty(m, np.int32), "wet_steps": np.empty(m, np.int32), "dry_steps": np.empty(m, np.int32)}
        args = [self._ptr(arrs[k]) if want.get(k) else None for k in ("x", "u", "weight", "count", "wet_steps", "dry_steps")]
        self._ps._call("sph_tracers_download", *args, m)
        return {k: v for k, v in arrs.items() if want.get(k)}

    def state(self) -> dict:
        """Everything at once: {"x", "u" f32 [m, 3], "weight" i64 [m], "count", "wet_steps", "dry_steps" i32 [m]}."""
        return self._download(x=True, u=True, weight=True, count=True, wet_steps=True, dry_steps=True)

    def positions(self) -> np.ndarray:
        return self._download(x=True)["x"]

    def velocities(self) -> np.ndarray:
        """The velocity each tracer moved with in the last advance (0 for a dry one)."""
        return self._download(u=True)["u"]

    def weight(self) -> np.ndarray:
        """The Shepard sum of the last advance as raw i64 fixed point (scale 2^30); `fill()` is the f64 view."""
        return self._download(weight=True)["weight"]

    def fill(self) -> np.ndarray:
        return self.weight().astype(np.float64) / float(1 << SCALE_LOG2)

    def count(self) -> np.ndarray:
        return self._download(count=True)["count"]

    def wet_steps(self) -> np.ndarray:
        return self._download(wet_steps=True)["wet_steps"]

    def dry_steps(self) -> np.ndarray:
        return self._download(dry_steps=True)["dry_steps"]

    def info(self) -> TracerInfo:
        from . import _lib
        i = _lib.SphTracerInfo()
        self._ps._call("sph_tracers_info", C.byref(i))
        return TracerInfo(i.m, i.advances, i.frames, i.dropped)

    def paths(self) -> np.ndarray:
        """The stored history, f32 [frames, m, 3]."""
        frames = self.info().frames
        out = np.empty((frames, self.m, 3), np.float32)
        self._ps._call("sph_tracers_history_download", self._ptr(out) if out.size else None, frames, self.m)
        return out

    def write_vtk(self, path):
        """The pathlines so far as legacy ASCII POLYDATA (one polyline per tracer, point data `time`); a set without stored
        frames writes its current positions as one-point lines at the current time."""
        paths, times = self.paths(), list(self.times)
        if paths.shape[0] == 0:
            paths, times = self.positions()[None, :, :], [self._ps.time]
        write_vtk(path, paths, times[:paths.shape[0]])

    def _after_steps(self, t_before: float, dt: float):
        """Behind a step call that began at simulated time t_before with time step dt: the times of the frames it stored."""
        adv = self.info().advances
        t = float(t_before)
        for a in range(self._advances + 1, adv + 1):
            t += float(np.float32(dt))
            if self.record_every > 0 and a % self.record_every == 0 and len(self.times) < self.record_capacity:
                self.times.append(t)
        self._advances = adv


def set_tracers(ps, points, min_fill=0.2, record_every=0, record_capacity=0, material="fluid", objects=None) -> Tracers:
    from . import _lib
    a = set_args(points, min_fill, record_every, record_capacity, material, objects)
    if ps.slab is not None:
        raise NotImplementedError("tracers exist on single-domain contexts only: a tracer that crossed to another rank would "
                                  "have to travel with the halo")
    p = _lib.SphTracerParams()
    p.min_fill, p.record_every, p.record_capacity = a["min_fill"], a["record_every"], a["record_capacity"]
    selection.fill(p.select, a["material"], a["objects"])
    pts = a["points"]
    ps._call("sph_tracers_set", pts.ctypes.data_as(C.c_void_p), pts.shape[0], C.byref(p))
    return Tracers(ps, pts.shape[0], a["record_every"], a["record_capacity"])


def clear_tracers(ps) -> Tracers:
    from . import _lib
    p = _lib.SphTracerParams()
    p.min_fill = 0.2
    selection.fill(p.select, -1, [])
    ps._call("sph_tracers_set", None, 0, C.byref(p))
    return Tracers(ps, 0, 0, 0)
