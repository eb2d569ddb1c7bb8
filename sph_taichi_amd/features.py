"""Per-particle flow features: what `ParticleSystem.set_features()` registers and `ParticleSystem.features` is
(include/sph_hip.h, section "Particle features"; csrc/sph_features.hip).

While a set is registered, every `every`-th WCSPH step of the device loop (`solver.step(n)`) evaluates, right behind the step's
density and pressure and before its force sweep, the flow at the selected particles themselves: vorticity and divergence of the
velocity (difference form, no renormalisation), the colour gradient (a raw surface normal), the kernel fill, the neighbour counts
and a free-surface flag -- one 64-byte row per persistent id on the device, the latest sample only.  Nothing crosses to the host
until an accessor asks.  Nothing in this module touches the GPU when it is imported.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import selection

SCALE_LOG2, FILL_SCALE_LOG2 = 24, 30
VALID, SURFACE, SATURATED = 1, 2, 4
FIELDS = ("vorticity", "divergence", "fill", "neighbours", "surface")            # enum SphFeatureField; "vorticity" paints |w|
MAX_NEIGHBOURS = 1 << 20
ROW_DTYPE = np.dtype([("x", "<f4", 3), ("vorticity", "<f4", 3), ("divergence", "<f4"), ("normal", "<f4", 3), ("fill", "<f4"),
                      ("n_fluid", "<i4"), ("n_solid", "<i4"), ("flags", "<i4"), ("reserved_", "<i4", 2)])
assert ROW_DTYPE.itemsize == 64
CONFIG_KEYS = ("every", "material", "objects", "minNeighbours", "normalMin", "export", "fields", "paint")
PAINT_KEYS = ("field", "range", "colormap")
# columns a PLY can carry beside x y z: name -> columns of the structured array
PLY_COLUMNS = {"vorticity": ("wx", "wy", "wz"), "divergence": ("divergence",), "normal": ("nx", "ny", "nz"), "fill": ("fill",),
               "neighbours": ("n_fluid", "n_solid"), "surface": ("surface",), "id": ("id",)}
PLY_INT = ("n_fluid", "n_solid", "surface", "id")
PLY_DEFAULT = ("vorticity", "divergence", "normal", "fill", "neighbours", "surface", "id")


def set_args(every=10, material="fluid", objects=None, min_neighbours=24, normal_min=0.0) -> dict:
    """The arguments of `set_features`, checked without a context: {"every", "material": -1 or the id, "objects": list,
    "min_neighbours", "normal_min": an f32 value}.  ValueError otherwise."""
    mat, ids = selection.parse(material, objects)
    every = selection.integer(every, "every")
    if every < 1:
        raise ValueError("every must be at least 1")
    min_neighbours = selection.integer(min_neighbours, "min_neighbours")
    if not 0 <= min_neighbours <= MAX_NEIGHBOURS:
        raise ValueError("min_neighbours must be in [0, 2^20]")
    if isinstance(normal_min, (bool, np.bool_)) or not isinstance(normal_min, (int, float, np.integer, np.floating)):
        raise ValueError(f"normal_min must be a number, not {normal_min!r}")
    with np.errstate(over="ignore"):
        nm = float(np.float32(normal_min))
    if not math.isfinite(nm) or nm < 0:
        raise ValueError("normal_min must be finite (as f32) and not negative")
    return {"every": every, "material": mat, "objects": ids, "min_neighbours": min_neighbours, "normal_min": nm}


def check_fields(fields) -> tuple:
    """The PLY columns asked for, in the order of PLY_COLUMNS.  ValueError for an unknown or repeated name."""
    if isinstance(fields, str):
        raise ValueError("fields must be a sequence of names, not one string")
    fields = list(fields)
    unknown = [f for f in fields if f not in PLY_COLUMNS]
    if unknown:
        raise ValueError(f"unknown field(s) {unknown}: choose from {list(PLY_COLUMNS)} (the position is always written)")
    if len(set(fields)) != len(fields):
        raise ValueError("a field is named twice")
    return tuple(n for n in PLY_COLUMNS if n in fields)


def check_paint(paint) -> dict:
    """{"field": name, "range": (lo, hi) or None, "colormap"} of a paint entry.  ValueError otherwise."""
    from . import render, scalars
    spec = selection.config_object(paint, "paint", PAINT_KEYS)
    field = spec.get("field", "vorticity")
    if not isinstance(field, str) or field not in FIELDS:
        raise ValueError(f"paint: field must be one of {list(FIELDS)}, not {field!r}")
    rng = spec.get("range")
    if rng is not None:
        rng = render.check_range(rng)
    scalars.lut(spec.get("colormap", "heat"))
    return {"field": field, "range": rng, "colormap": spec.get("colormap", "heat")}


def features_config(config):
    """The scene's "features" object in the Configuration: {"every": 10, "material": "fluid", "objects": [0], "minNeighbours": 24,
    "normalMin": 0.0, "export": "surface" | "all", "fields": [...], "paint": {"field": "vorticity", "range": [0, 50], "colormap":
    "heat"}}, every key optional.  Returns (keyword arguments of `set_features`, {"export": "surface" | "all" | None, "fields",
    "paint": checked entry or None}), or None when the key is absent.  A misspelt key or a bad value raises ValueError."""
    spec = selection.config_object(config, "features", CONFIG_KEYS)
    if spec is None:
        return None
    kw = {"every": spec.get("every", 10), "material": spec.get("material", "fluid"), "objects": spec.get("objects"),
          "min_neighbours": spec.get("minNeighbours", 24), "normal_min": spec.get("normalMin", 0.0)}
    try:
        set_args(**kw)
        export = spec.get("export")
        if export is not None and export not in ("surface", "all"):
            raise ValueError(f'export must be "surface" or "all", not {export!r}')
        out = {"export": export, "fields": check_fields(spec.get("fields", PLY_DEFAULT)),
               "paint": check_paint(spec["paint"]) if "paint" in spec else None}
    except ValueError as e:
        raise ValueError(f'"features": {e}') from e
    return kw, out


def unit_outward(normal) -> np.ndarray:
    """f32 [n, 3]: -N / |N| (N points into the fluid), zero where N == 0; the norm in f64."""
    n = np.asarray(normal, dtype=np.float64)
    length = np.sqrt((n * n).sum(axis=-1))
    out = np.zeros(n.shape, dtype=np.float64)
    ok = length > 0
    out[ok] = -n[ok] / length[ok][:, None]
    return out.astype(np.float32)


def ply_table(rows, fields=PLY_DEFAULT, surface_only=False) -> np.ndarray:
    """The packed structured array `export.write_ply` takes, of the VALID rows (of those flagged surface with `surface_only`), in
    ascending persistent id: x y z, then the columns of `fields` (PLY_COLUMNS).  `normal` is the unit outward one."""
    fields = check_fields(fields)
    rows = np.asarray(rows)
    take = (rows["flags"] & VALID) != 0
    if surface_only:
        take &= (rows["flags"] & SURFACE) != 0
    ids = np.flatnonzero(take)
    r = rows[ids]
    cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    for f in fields:
        cols.extend((c, "<i4" if c in PLY_INT else "<f4") for c in PLY_COLUMNS[f])
    out = np.zeros(ids.shape[0], dtype=np.dtype(cols))
    for k, c in enumerate("xyz"):
        out[c] = r["x"][:, k]
    if "vorticity" in fields:
        for k, c in enumerate(PLY_COLUMNS["vorticity"]):
            out[c] = r["vorticity"][:, k]
    if "divergence" in fields:
        out["divergence"] = r["divergence"]
    if "normal" in fields:
        n = unit_outward(r["normal"])
        for k, c in enumerate(PLY_COLUMNS["normal"]):
            out[c] = n[:, k]
    if "fill" in fields:
        out["fill"] = r["fill"]
    if "neighbours" in fields:
        out["n_fluid"], out["n_solid"] = r["n_fluid"], r["n_solid"]
    if "surface" in fields:
        out["surface"] = (r["flags"] & SURFACE) != 0
    if "id" in fields:
        out["id"] = ids
    return out


def read_ply(path) -> np.ndarray:
    """What `write_ply` wrote, as the structured array (binary little-endian vertex list of f32 / i32 columns)."""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    head = blob[:end].decode("ascii").splitlines()
    if head[0] != "ply" or head[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    count = next(int(l.split()[2]) for l in head if l.startswith("element vertex "))
    cols = [(l.split()[2], {"float": "<f4", "int": "<i4"}[l.split()[1]]) for l in head if l.startswith("property ")]
    return np.frombuffer(blob[end:], dtype=np.dtype(cols), count=count)


def paint_values(rows, field) -> np.ndarray:
    """f32 [n]: the value `paint` maps through the table, per row (the device's arithmetic: |w| summed as (x*x + y*y) + z*z in f32)."""
    rows = np.asarray(rows)
    if field == "vorticity":
        w = rows["vorticity"].astype(np.float32)
        with np.errstate(all="ignore"):
            return np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    if field in ("divergence", "fill"):
        return rows[field].astype(np.float32)
    if field == "neighbours":
        return (rows["n_fluid"] + rows["n_solid"]).astype(np.float32)
    if field == "surface":
        return ((rows["flags"] & SURFACE) != 0).astype(np.float32)
    raise ValueError(f"field must be one of {list(FIELDS)}, not {field!r}")


class FeatureInfo:
    def __init__(self, i):
        self.every, self.rows = int(i.every), int(i.rows)
        self.samples, self.steps_seen, self.step, self.time = int(i.samples), int(i.steps_seen), int(i.step), float(i.time)

    def __repr__(self):
        return (f"FeatureInfo(every={self.every}, rows={self.rows}, samples={self.samples}, steps_seen={self.steps_seen}, "
                f"step={self.step}, time={self.time!r})")


class Features:
    """The registered set of a ParticleSystem.  Every accessor but `info()` and what reads it downloads the rows (and synchronises);
    the arrays are indexed by persistent id (`ids`), and a row that was no target of the latest sample is all zero."""

    def __init__(self, ps, args, m_V0):
        self._ps = ps
        self.every, self.min_neighbours, self.normal_min = int(args["every"]), int(args["min_neighbours"]), float(args["normal_min"])
        self.material, self.objects = int(args["material"]), list(args["objects"])
        self._m_V0 = float(m_V0)

    def info(self) -> FeatureInfo:
        from . import _lib
        i = _lib.SphFeatureInfo()
        self._ps._call("sph_features_info", C.byref(i))
        return FeatureInfo(i)

    @property
    def samples(self) -> int:
        return self.info().samples

    @property
    def time(self) -> float:
        """Simulated time of the latest sample."""
        return self.info().time

    @property
    def step(self) -> int:
        """Step index (the set's count of steps) of the latest sample; -1 before the first."""
        return self.info().step

    @property
    def ids(self) -> np.ndarray:
        return np.arange(self.info().rows, dtype=np.int64)

    def sample(self):
        """One sample of the current state outside a step (sph_features_sample); needs the neighbour structure."""
        self._ps._call("sph_features_sample")

    def rows(self) -> np.ndarray:
        """The rows of the latest sample, ROW_DTYPE [n] by persistent id."""
        out = np.zeros(self.info().rows, dtype=ROW_DTYPE)
        self._ps._call("sph_features_download", out.ctypes.data_as(C.c_void_p), out.shape[0])
        return out

    def vorticity(self):
        return self.rows()["vorticity"].copy()

    def divergence(self):
        return self.rows()["divergence"].copy()

    def fill(self):
        return self.rows()["fill"].copy()

    def neighbours(self):
        """(n_fluid, n_solid), i32 [n] each."""
        r = self.rows()
        return r["n_fluid"].copy(), r["n_solid"].copy()

    def normal(self):
        """f32 [n, 3]: unit, outward, zero where the colour gradient vanishes."""
        return unit_outward(self.rows()["normal"])

    def surface(self):
        return (self.rows()["flags"] & SURFACE) != 0

    def valid(self):
        return (self.rows()["flags"] & VALID) != 0

    def saturated(self):
        return (self.rows()["flags"] & SATURATED) != 0

    def positions(self):
        return self.rows()["x"].copy()

    def enstrophy(self) -> float:
        """sum over the valid rows of 0.5 * m_V0 * |w|^2, f64 on the host (m^5 / s^2: times the density, an energy-like rate)."""
        r = self.rows()
        w = r["vorticity"][(r["flags"] & VALID) != 0].astype(np.float64)
        return float(0.5 * self._m_V0 * (w * w).sum())

    def write_ply(self, path, surface_only=False, fields=PLY_DEFAULT):
        """A binary PLY of the valid rows (`surface_only`: of the surface shell alone) through export.write_ply; returns the count."""
        from . import export
        i = self.info()
        data = ply_table(self.rows(), fields, surface_only)
        export.write_ply(path, data, comments=(f"time {i.time!r}", f"step {i.step}", "surface only" if surface_only else "all targets"))
        return int(data.shape[0])

    def paint(self, field="vorticity", range=None, colormap="heat"):
        """Write the table colour of `field` (FIELDS; "vorticity" is its magnitude) of every valid row into the object colour of
        its particle (`ps.color`), which both frame styles draw.  `range` None: (min, max) over the valid finite values, (lo, lo + 1)
        where that is no usable range.  Returns the range used."""
        from . import render, scalars
        if not isinstance(field, str) or field not in FIELDS:
            raise ValueError(f"field must be one of {list(FIELDS)}, not {field!r}")
        table = scalars.lut(colormap)
        if range is None:
            r = self.rows()
            v = paint_values(r, field)[(r["flags"] & VALID) != 0]
            v = v[np.isfinite(v)]
            rng = render.auto_range(float(v.min()), float(v.max()), v.size) if v.size else render.auto_range(0.0, 0.0, 0)
        else:
            rng = render.check_range(range)
        self._ps._call("sph_features_paint", FIELDS.index(field), C.c_float(rng[0]), C.c_float(rng[1]), table.ctypes.data_as(C.c_void_p))
        return rng


def _refuse_slab(ps):
    if ps.slab is not None:
        raise NotImplementedError("particle features exist on single-domain contexts only: a particle's neighbours beyond the halo "
                                  "belong to another rank and the rows are indexed by global id")


def feature_params(a):
    """SphFeatureParams of checked arguments (`set_args`)."""
    from . import _lib
    p = _lib.SphFeatureParams()
    selection.fill(p.select, a["material"], a["objects"])
    p.every, p.min_neighbours, p.normal_min = a["every"], a["min_neighbours"], a["normal_min"]
    return p


def set_features(ps, every=10, material="fluid", objects=None, min_neighbours=24, normal_min=0.0) -> Features:
    a = set_args(every, material, objects, min_neighbours, normal_min)
    _refuse_slab(ps)
    p = feature_params(a)
    ps._call("sph_features_set", C.byref(p))
    return Features(ps, a, ps.m_V0)


def clear_features(ps):
    _refuse_slab(ps)
    ps._call("sph_features_set", None)
