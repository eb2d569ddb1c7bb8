"""Running flow statistics: what `ParticleSystem.set_statistics()` registers and `ParticleSystem.statistics` is
(include/sph_hip.h, section "Running flow statistics"; csrc/sph_stats.hip).

A grid (a volume, or a slice when the shape has a 1 in it) whose nodes accumulate on the device, across steps: while a set is
registered, every `every`-th step of the device loop (`solver.step(n)`) samples the Shepard-mean velocity of the selected particles
at the nodes and folds it into eleven i64 planes -- `n_wet` (samples in which the node was wet), `sum_w` (their Shepard sums, scale
2^30), `sum_u` [3] (scale 2^32) and `sum_uu` [6] (xx xy xz yy yz zz, scale 2^24).  Nothing crosses to the host until an accessor
asks.  From the integers follow, in f64 and CONDITIONAL ON THE NODE BEING WET: the time-mean velocity <u>, the Reynolds stresses
R_ab = <u_a u_b> - <u_a><u_b>, the RMS fluctuations sqrt(R_aa), the turbulent kinetic energy tr(R) / 2, the mean fill, and the
intermittency n_wet / samples.  A node that was never wet is NaN in every derived field.  Nothing in this module touches the GPU
when it is imported.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import sample as _sample
from . import selection

MAX_SAMPLES = 1 << 19
W_SCALE_LOG2, U_SCALE_LOG2, UU_SCALE_LOG2 = 30, 32, 24
UU_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))     # the order of the sum_uu planes
UU_NAMES = ("xx", "xy", "xz", "yy", "yz", "zz")
CONFIG_KEYS = ("spacing", "origin", "shape", "objects", "every", "capacity", "wet")
VELOCITY_MASK = 1 | 2 | 4


def wet_min_of(wet) -> int:
    """The `wet` Shepard sum in the units of the sampler's weight plane, converted once."""
    try:
        w = np.float64(wet)
    except (TypeError, ValueError) as e:
        raise ValueError("wet must be a number") from e
    if not np.isfinite(w) or w < 0 or w > 4:
        raise ValueError("wet must be finite and in [0, 4]")
    return int(np.rint(np.float64(wet) * 2 ** 30))


def set_args(spacing=None, origin=None, shape=None, objects=None, material="fluid", every=10, capacity=None, wet=0.4, *,
             particle_diameter, domain_size) -> dict:
    """The arguments of `set_statistics`, checked without a context: the grid of `sample.grid_args` ("spacing", "origin",
    "shape"), the selection ("material": -1 or the id, "objects": list), "every", "capacity" and "wet_min".  ValueError otherwise."""
    a = _sample.grid_args(spacing, origin, shape, particle_diameter=particle_diameter, domain_size=domain_size)
    sel = _sample.select_args(fields=("velocity",), material=material, objects=objects)
    every = selection.integer(every, "every")
    if every < 1:
        raise ValueError("every must be at least 1")
    capacity = MAX_SAMPLES if capacity is None else selection.integer(capacity, "capacity")
    if not 1 <= capacity <= MAX_SAMPLES:
        raise ValueError(f"capacity must be in [1, {MAX_SAMPLES}]")
    a.update(material=sel["material"], objects=sel["objects"], every=every, capacity=capacity, wet_min=wet_min_of(wet))
    return a


def statistics_config(config):
    """The scene's "statistics" object in the Configuration: {"spacing": s, "origin": [..], "shape": [..], "objects": [..],
    "every": 10, "capacity": n, "wet": 0.4}, every key optional ({} = the whole domain at the particle diameter, every 10th step).
    Returns the keyword arguments of `set_statistics`, or None when the key is absent.  A misspelt key or a bad value raises
    ValueError."""
    spec = selection.config_object(config, "statistics", CONFIG_KEYS)
    if spec is None:
        return None
    kw = {"spacing": spec.get("spacing"), "origin": spec.get("origin"), "shape": spec.get("shape"), "objects": spec.get("objects"),
          "every": spec.get("every", 10), "capacity": spec.get("capacity"), "wet": spec.get("wet", 0.4)}
    try:
        set_args(**kw, particle_diameter=1.0, domain_size=(1.0, 1.0, 1.0))
    except ValueError as e:
        raise ValueError(f'"statistics": {e}') from e
    return kw


class Accumulators:
    """The eleven raw planes over a grid of `shape` -- `n_wet`, `sum_w` i64 [n0, n1, n2], `sum_u` i64 [3, ...], `sum_uu` i64
    [6, ...] -- with the number of `samples` taken, and the f64 fields that follow from them."""

    def __init__(self, n_wet, sum_w, sum_u, sum_uu, *, samples, shape, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), times=(0.0, 0.0)):
        self.shape = tuple(int(n) for n in shape)
        if len(self.shape) != 3:
            raise ValueError("shape must be three node counts")
        self.n_wet = np.asarray(n_wet, dtype=np.int64).reshape(self.shape)
        self.sum_w = np.asarray(sum_w, dtype=np.int64).reshape(self.shape)
        self.sum_u = np.asarray(sum_u, dtype=np.int64).reshape((3,) + self.shape)
        self.sum_uu = np.asarray(sum_uu, dtype=np.int64).reshape((6,) + self.shape)
        self.samples = int(samples)
        self.origin, self.spacing = _sample._triple(origin, "origin"), _sample._triple(spacing, "spacing")
        self.times = (float(times[0]), float(times[1]))

    def _per_wet(self, sums, scale_log2):
        """sums / 2^scale / n_wet in f64, NaN where the node was never wet."""
        has = self.n_wet > 0
        n = np.where(has, self.n_wet, 1).astype(np.float64)
        return np.where(has, sums.astype(np.float64) / float(1 << scale_log2) / n, np.nan)

    def intermittency(self):
        """n_wet / samples: the fraction of the samples in which the node was wet (NaN before the first sample)."""
        if self.samples <= 0:
            return np.full(self.shape, np.nan)
        return self.n_wet.astype(np.float64) / float(self.samples)

    def mean_fill(self):
        """The mean Shepard sum of the node's wet samples."""
        return self._per_wet(self.sum_w, W_SCALE_LOG2)

    def mean_velocity(self):
        """[..., 3] f64: the mean over the node's wet samples."""
        return np.moveaxis(self._per_wet(self.sum_u, U_SCALE_LOG2), 0, -1)

    def second_moment(self):
        """[..., 3, 3] f64, symmetric: <u_a u_b> over the node's wet samples."""
        m = self._per_wet(self.sum_uu, UU_SCALE_LOG2)
        out = np.empty(self.shape + (3, 3), dtype=np.float64)
        for k, (a, b) in enumerate(UU_PAIRS):
            out[..., a, b] = out[..., b, a] = m[k]
        return out

    def reynolds_stress(self):
        """[..., 3, 3] f64, symmetric: R_ab = <u_a u_b> - <u_a><u_b>."""
        u = self.mean_velocity()
        return self.second_moment() - u[..., :, None] * u[..., None, :]

    def rms_velocity(self):
        """[..., 3] f64: sqrt(R_aa), the diagonal cut at 0 (the fixed point can leave it a few 2^-25 below)."""
        r = self.reynolds_stress()
        return np.sqrt(np.maximum(np.stack([r[..., a, a] for a in range(3)], axis=-1), 0.0))

    def tke(self):
        """tr(R) / 2."""
        r = self.reynolds_stress()
        return 0.5 * (r[..., 0, 0] + r[..., 1, 1] + r[..., 2, 2])

    def vtk_arrays(self):
        """(name, components, f32 array in VTK point order: x fastest) of what `write_vtk` writes."""
        order = lambda a: np.ascontiguousarray(np.transpose(a, (2, 1, 0) + tuple(range(3, a.ndim))))
        r = self.reynolds_stress()
        out = [("intermittency", 1, self.intermittency()), ("mean_fill", 1, self.mean_fill()), ("mean_velocity", 3, self.mean_velocity()),
               ("rms_velocity", 3, self.rms_velocity()), ("tke", 1, self.tke())]
        out += [(f"reynolds_{name}", 1, r[..., a, b]) for name, (a, b) in zip(UU_NAMES, UU_PAIRS)]
        return [(name, comps, order(a).astype(np.float32)) for name, comps, a in out]

    def write_vtk(self, path):
        """A legacy binary STRUCTURED_POINTS file like the sampler's: ASCII header, big-endian f32; scalars as SCALARS, the mean
        and the RMS velocity as VECTORS.  Never-wet nodes are NaN."""
        n = self.shape[0] * self.shape[1] * self.shape[2]
        head = ["# vtk DataFile Version 3.0",
                f"sph_taichi_amd flow statistics, {self.samples} samples, time {self.times[0]!r} to {self.times[1]!r}", "BINARY",
                "DATASET STRUCTURED_POINTS", "DIMENSIONS {} {} {}".format(*self.shape), "ORIGIN {!r} {!r} {!r}".format(*self.origin),
                "SPACING {!r} {!r} {!r}".format(*self.spacing), f"POINT_DATA {n}"]
        with open(path, "wb") as fh:
            fh.write(("\n".join(head) + "\n").encode("ascii"))
            for name, comps, a in self.vtk_arrays():
                if comps == 3:
                    fh.write(f"VECTORS {name} float\n".encode("ascii"))
                else:
                    fh.write(f"SCALARS {name} float 1\nLOOKUP_TABLE default\n".encode("ascii"))
                fh.write(a.astype(">f4").tobytes())
                fh.write(b"\n")


def read_vtk(path) -> dict:
    """What `write_vtk` wrote: {"comment", "shape", "origin", "spacing", "arrays": {name: f32 [n0, n1, n2] or [n0, n1, n2, 3]}}."""
    with open(path, "rb") as fh:
        raw = fh.read()
    at = 0

    def line():
        nonlocal at
        end = raw.index(b"\n", at)
        text = raw[at:end].decode("ascii")
        at = end + 1
        return text

    line()
    out = {"comment": line()}
    if line() != "BINARY" or line() != "DATASET STRUCTURED_POINTS":
        raise ValueError(f"{path}: not a binary STRUCTURED_POINTS file")
    shape = tuple(int(v) for v in line().split()[1:])
    out["shape"] = shape
    out["origin"] = tuple(float(v) for v in line().split()[1:])
    out["spacing"] = tuple(float(v) for v in line().split()[1:])
    n = int(line().split()[1])
    arrays = {}
    while at < len(raw):
        kind, name = line().split()[:2]
        comps = 3 if kind == "VECTORS" else 1
        if kind == "SCALARS":
            line()                                           # LOOKUP_TABLE default
        a = np.frombuffer(raw, dtype=">f4", count=n * comps, offset=at).astype(np.float32)
        at += n * comps * 4 + 1
        a = a.reshape((shape[2], shape[1], shape[0]) + ((3,) if comps == 3 else ()))
        arrays[name] = np.ascontiguousarray(np.transpose(a, (2, 1, 0) + ((3,) if comps == 3 else ())))
    out["arrays"] = arrays
    return out


class StatsInfo:
    def __init__(self, i):
        self.nodes, self.shape, self.every = int(i.nodes), (int(i.n[0]), int(i.n[1]), int(i.n[2])), int(i.every)
        self.samples, self.dropped, self.steps_seen = int(i.samples), int(i.dropped), int(i.steps_seen)
        self.t_first, self.t_last = float(i.t_first), float(i.t_last)

    def __repr__(self):
        return (f"StatsInfo(shape={self.shape}, every={self.every}, samples={self.samples}, dropped={self.dropped}, "
                f"steps_seen={self.steps_seen}, t_first={self.t_first!r}, t_last={self.t_last!r})")


class Statistics:
    """The registered set of a ParticleSystem.  Every accessor downloads (and synchronises); `info()` does not."""

    def __init__(self, ps, args):
        self._ps = ps
        self.shape, self.origin, self.spacing = tuple(args["shape"]), tuple(args["origin"]), tuple(args["spacing"])
        self.every, self.capacity, self.wet_min = int(args["every"]), int(args["capacity"]), int(args["wet_min"])
        self.nodes = self.shape[0] * self.shape[1] * self.shape[2]

    def info(self) -> StatsInfo:
        from . import _lib
        i = _lib.SphStatsInfo()
        self._ps._call("sph_stats_info", C.byref(i))
        return StatsInfo(i)

    @property
    def samples(self) -> int:
        return self.info().samples

    @property
    def times(self):
        """(t_first, t_last): the simulated times of the first and the last sample taken."""
        i = self.info()
        return (i.t_first, i.t_last)

    def sample(self):
        """One sample of the current state outside a step (sph_stats_sample); the step count is not touched."""
        self._ps._call("sph_stats_sample")

    def accumulators(self) -> Accumulators:
        """The raw i64 planes, downloaded."""
        n = self.nodes
        n_wet, sum_w = np.empty(n, np.int64), np.empty(n, np.int64)
        sum_u, sum_uu = np.empty((3, n), np.int64), np.empty((6, n), np.int64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        self._ps._call("sph_stats_download", ptr(n_wet), ptr(sum_w), ptr(sum_u), ptr(sum_uu), n)
        i = self.info()
        return Accumulators(n_wet, sum_w, sum_u, sum_uu, samples=i.samples, shape=self.shape, origin=self.origin, spacing=self.spacing,
                            times=(i.t_first, i.t_last))

    def intermittency(self):
        return self.accumulators().intermittency()

    def mean_fill(self):
        return self.accumulators().mean_fill()

    def mean_velocity(self):
        return self.accumulators().mean_velocity()

    def reynolds_stress(self):
        return self.accumulators().reynolds_stress()

    def rms_velocity(self):
        return self.accumulators().rms_velocity()

    def tke(self):
        return self.accumulators().tke()

    def write_vtk(self, path):
        self.accumulators().write_vtk(path)

    def reset(self):
        """Zero the accumulators and the counters; the set stays registered."""
        self._ps._call("sph_stats_reset")


def _refuse_slab(ps):
    if ps.slab is not None:
        raise NotImplementedError("statistics are accumulated on single-domain contexts only: a slab rank's ghost records would be "
                                  "counted twice (the planes of the ranks' owned ranges would have to be all-reduced)")


def stats_params(ps, a):
    """SphStatsParams of checked arguments (`set_args`)."""
    from . import _lib
    p = _lib.SphStatsParams()
    g = p.grid
    g.n = (C.c_int32 * 3)(*a["shape"])
    g.origin, g.spacing = (C.c_float * 3)(*a["origin"]), (C.c_float * 3)(*a["spacing"])
    g.inv_h, g.fields = _sample.inv_h_f32(ps.support_radius), VELOCITY_MASK
    selection.fill(g.select, a["material"], a["objects"])
    p.every, p.capacity, p.wet_min = a["every"], a["capacity"], a["wet_min"]
    return p


def set_statistics(ps, spacing=None, origin=None, shape=None, objects=None, material="fluid", every=10, capacity=None, wet=0.4) -> Statistics:
    a = set_args(spacing, origin, shape, objects, material, every, capacity, wet, particle_diameter=ps.particle_diameter,
                 domain_size=ps.domain_size)
    _refuse_slab(ps)
    p = stats_params(ps, a)
    ps._call("sph_stats_set", C.byref(p))
    return Statistics(ps, a)


def clear_statistics(ps):
    _refuse_slab(ps)
    ps._call("sph_stats_set", None)
