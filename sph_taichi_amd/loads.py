"""Fluid loads on solid objects: what `ParticleSystem.set_loads()` registers and `ParticleSystem.loads` is
(include/sph_hip.h, section "Fluid loads"; csrc/sph_loads.hip).

While a set is registered, every `every`-th WCSPH step of the device loop (`solver.step(n)`) samples, right behind the step's density
and pressure and before its force sweep, the force and the torque the fluid exerts on each selected solid object (static, kinematic
or dynamic): the Akinci boundary term of WCSPH.py:58-68 summed over the object's particles, nine i64 per object and sample on the
device -- Fx Fy Fz Tx Ty Tz at scale 2^24, then the contributing pairs, the wet solid particles and the saturated terms.  Nothing
crosses to the host until an accessor asks.  Nothing in this module touches the GPU when it is imported.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import selection

MAX_OBJECTS = 32
ROW_WORDS = 9                                    # Fx Fy Fz Tx Ty Tz pairs wet saturated
SCALE_LOG2 = 24
MAX_HISTORY_BYTES = 1 << 31
CONFIG_KEYS = ("objects", "about", "every", "capacity")
CSV_HEADER = ("time", "object", "fx", "fy", "fz", "tx", "ty", "tz", "pairs", "wet_particles", "saturated")


def _about(about):
    try:
        a = np.asarray(about, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError) as e:
        raise ValueError("about must be three numbers") from e
    if a.size != 3:
        raise ValueError("about must be three numbers")
    with np.errstate(over="ignore"):
        f = a.astype(np.float32)
    if not np.isfinite(f).all():
        raise ValueError("about must be finite (as f32)")
    return tuple(float(v) for v in f)


def set_args(objects=(1,), about=(0.0, 0.0, 0.0), every=1, capacity=4096) -> dict:
    """The arguments of `set_loads`, checked without a context: {"objects": list of 1 to 32 distinct ids, "about": three f32 values,
    "every", "capacity"}.  ValueError otherwise."""
    if objects is None:
        raise ValueError("objects must name the solid objects to load (1 to 32 ids)")
    _, ids = selection.parse(None, objects)
    if len(set(ids)) != len(ids):
        raise ValueError(f"objects holds a duplicate id: {ids}")
    every = selection.integer(every, "every")
    if every < 1:
        raise ValueError("every must be at least 1")
    capacity = selection.integer(capacity, "capacity")
    if capacity < 1:
        raise ValueError("capacity must be at least 1")
    if capacity * len(ids) * ROW_WORDS * 8 > MAX_HISTORY_BYTES:
        raise ValueError(f"a history of {capacity} samples of {len(ids)} objects takes more than 2^31 bytes")
    return {"objects": ids, "about": _about(about), "every": every, "capacity": capacity}


def loads_config(config):
    """The scene's "loads" object in the Configuration: {"objects": [...], "about": [x, y, z], "every": n, "capacity": n}; "objects"
    is required, the rest optional.  Returns the keyword arguments of `set_loads`, or None when the key is absent.  A misspelt key or
    a bad value raises ValueError."""
    spec = selection.config_object(config, "loads", CONFIG_KEYS)
    if spec is None:
        return None
    if "objects" not in spec:
        raise ValueError('"loads": objects is required')
    kw = {"objects": spec["objects"], "about": spec.get("about", (0.0, 0.0, 0.0)), "every": spec.get("every", 1),
          "capacity": spec.get("capacity", 4096)}
    try:
        set_args(**kw)
    except ValueError as e:
        raise ValueError(f'"loads": {e}') from e
    return kw


def transport_torque(torque, force, about_from, about_to):
    """The torque about `about_to` of a force system whose torque about `about_from` is `torque`: T - (c' - c) x F, f64."""
    shift = np.asarray(about_to, dtype=np.float64) - np.asarray(about_from, dtype=np.float64)
    return np.asarray(torque, dtype=np.float64) - np.cross(np.broadcast_to(shift, np.shape(force)), np.asarray(force, dtype=np.float64))


class LoadHistory:
    """The raw rows i64 [samples, n_objects, 9] with their f64 `times` [samples], and what follows from them."""

    def __init__(self, rows, times, objects, about):
        self.objects = [int(o) for o in objects]
        self.raw = np.asarray(rows, dtype=np.int64).reshape(-1, len(self.objects), ROW_WORDS)
        self.times = np.asarray(times, dtype=np.float64).reshape(-1)
        if self.times.shape[0] != self.raw.shape[0]:
            raise ValueError("rows and times differ in their number of samples")
        self.about = tuple(float(v) for v in about)

    @property
    def samples(self) -> int:
        return self.raw.shape[0]

    def force(self):
        """[samples, n_objects, 3] f64, in N: the force of the fluid on each object."""
        return self.raw[..., 0:3].astype(np.float64) / float(1 << SCALE_LOG2)

    def torque(self, about=None):
        """[samples, n_objects, 3] f64, in N m: about the set's point, or transported on the host to `about` by T - (c' - c) x F."""
        t = self.raw[..., 3:6].astype(np.float64) / float(1 << SCALE_LOG2)
        return t if about is None else transport_torque(t, self.force(), self.about, _about(about))

    def pairs(self):
        return self.raw[..., 6].copy()

    def wet_particles(self):
        return self.raw[..., 7].copy()

    def saturated(self):
        return self.raw[..., 8].copy()

    def impulse(self):
        """[n_objects, 3] f64, in N s: the trapezoid of the force over `times` (zero with fewer than two samples)."""
        f = self.force()
        if self.samples < 2:
            return np.zeros(f.shape[1:], dtype=np.float64)
        dt = np.diff(self.times)[:, None, None]
        return (0.5 * (f[1:] + f[:-1]) * dt).sum(axis=0)

    def rows(self):
        """One dict per (sample, object), for JSON and the CSV."""
        f, t = self.force(), self.torque()
        out = []
        for k in range(self.samples):
            for o, oid in enumerate(self.objects):
                out.append({"time": float(self.times[k]), "object": oid, "force": [float(v) for v in f[k, o]], "torque": [float(v) for v in t[k, o]],
                            "pairs": int(self.raw[k, o, 6]), "wet_particles": int(self.raw[k, o, 7]), "saturated": int(self.raw[k, o, 8])})
        return out

    def write_csv(self, path):
        """time, object, fx fy fz, tx ty tz (repr of the f64 values: they read back exactly), pairs, wet_particles, saturated; the
        point the torques are about stands in the comment line."""
        with open(path, "w") as fh:
            fh.write("# about {!r} {!r} {!r}\n".format(*self.about))
            fh.write(",".join(CSV_HEADER) + "\n")
            for r in self.rows():
                vals = [repr(r["time"]), str(r["object"])] + [repr(v) for v in r["force"] + r["torque"]]
                fh.write(",".join(vals + [str(r["pairs"]), str(r["wet_particles"]), str(r["saturated"])]) + "\n")


def read_csv(path) -> dict:
    """What `write_csv` wrote: {"about", "time" [rows], "object" [rows], "force" [rows, 3], "torque" [rows, 3], "pairs",
    "wet_particles", "saturated" [rows]}."""
    with open(path) as fh:
        lines = [l.rstrip("\n") for l in fh]
    if len(lines) < 2 or not lines[0].startswith("# about ") or lines[1] != ",".join(CSV_HEADER):
        raise ValueError(f"{path}: not a loads CSV")
    body = [l.split(",") for l in lines[2:] if l]
    col = lambda k, t: np.array([t(r[k]) for r in body], dtype=np.float64 if t is float else np.int64)
    return {"about": tuple(float(v) for v in lines[0].split()[2:]), "time": col(0, float), "object": col(1, int),
            "force": np.stack([col(k, float) for k in (2, 3, 4)], axis=1) if body else np.zeros((0, 3)),
            "torque": np.stack([col(k, float) for k in (5, 6, 7)], axis=1) if body else np.zeros((0, 3)),
            "pairs": col(8, int), "wet_particles": col(9, int), "saturated": col(10, int)}


class LoadInfo:
    def __init__(self, i):
        self.n_objects, self.every = int(i.n_objects), int(i.every)
        self.samples, self.dropped, self.steps_seen = int(i.samples), int(i.dropped), int(i.steps_seen)

    def __repr__(self):
        return (f"LoadInfo(n_objects={self.n_objects}, every={self.every}, samples={self.samples}, dropped={self.dropped}, "
                f"steps_seen={self.steps_seen})")


class Loads:
    """The registered set of a ParticleSystem.  Every accessor downloads (and synchronises); `info()` does not."""

    def __init__(self, ps, args):
        self._ps = ps
        self.objects, self.about = list(args["objects"]), tuple(args["about"])
        self.every, self.capacity = int(args["every"]), int(args["capacity"])

    def info(self) -> LoadInfo:
        from . import _lib
        i = _lib.SphLoadInfo()
        self._ps._call("sph_loads_info", C.byref(i))
        return LoadInfo(i)

    @property
    def samples(self) -> int:
        return self.info().samples

    def sample(self):
        """One sample of the current state outside a step (sph_loads_sample), for callers that drive the kernels stage by stage."""
        self._ps._call("sph_loads_sample")

    def history(self) -> LoadHistory:
        """The raw rows and their times, downloaded."""
        n = self.info().samples
        rows, times = np.zeros((n, len(self.objects), ROW_WORDS), np.int64), np.zeros(n, np.float64)
        self._ps._call("sph_loads_download", rows.ctypes.data_as(C.c_void_p), times.ctypes.data_as(C.c_void_p), n, len(self.objects))
        return LoadHistory(rows, times, self.objects, self.about)

    @property
    def times(self):
        return self.history().times

    def force(self):
        return self.history().force()

    def torque(self, about=None):
        return self.history().torque(about)

    def pairs(self):
        return self.history().pairs()

    def wet_particles(self):
        return self.history().wet_particles()

    def saturated(self):
        return self.history().saturated()

    def impulse(self):
        return self.history().impulse()

    def rows(self):
        return self.history().rows()

    def write_csv(self, path):
        self.history().write_csv(path)

    def reset(self):
        """Zero the history and the counters; the set stays registered."""
        self._ps._call("sph_loads_reset")


def _refuse_slab(ps):
    if ps.slab is not None:
        raise NotImplementedError("fluid loads are sampled on single-domain contexts only: a solid's fluid neighbours beyond the halo "
                                  "belong to another rank (the rows of the ranks would have to be all-reduced)")


def load_params(a):
    """SphLoadParams of checked arguments (`set_args`)."""
    from . import _lib
    p = _lib.SphLoadParams()
    for k, oid in enumerate(a["objects"]):
        p.object_ids[k] = oid
    p.n_objects = len(a["objects"])
    p.about = (C.c_float * 3)(*a["about"])
    p.every, p.capacity = a["every"], a["capacity"]
    return p


def set_loads(ps, objects=(1,), about=(0.0, 0.0, 0.0), every=1, capacity=4096) -> Loads:
    a = set_args(objects, about, every, capacity)
    _refuse_slab(ps)
    p = load_params(a)
    ps._call("sph_loads_set", C.byref(p))
    return Loads(ps, a)


def clear_loads(ps):
    _refuse_slab(ps)
    ps._call("sph_loads_set", None)
