"""Carried scalars: what `ParticleSystem.set_scalars()` registers and `ParticleSystem.scalars` is
(include/sph_hip.h, section "Carried scalars"; csrc/sph_scalars.hip).

A set holds 1 to 4 channels of a quantity that rides on the particles -- dye, heat, a concentration -- as 2^32 fixed point by
persistent id on the device.  While it is registered, every `every`-th step of the device loop (`solver.step(n)`, WCSPH or DFSPH)
diffuses it between neighbouring carriers right behind the step's sort: one explicit Jacobi step of Brookshaw's Laplacian with
a = dt * every * diffusivity, all sums integers.  Source objects hold a prescribed value (Dirichlet); every other particle is
invisible to the sum (insulation).  Nothing crosses to the host until an accessor asks.  Nothing in this module touches the GPU
when it is imported.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import selection

MAX_CHANNELS = 4
MAX_SOURCES = 8
SCALE_LOG2 = 32
VALUE_MAX = float(1 << 20)
CONFIG_KEYS = ("channels", "diffusivity", "values", "sources", "every", "material", "objects", "paint")
PAINT_KEYS = ("channel", "range", "colormap")


def _row(row, k, what) -> tuple:
    """`row` as K finite floats within +-2^20 (a single number stands for a row of one channel)."""
    try:
        a = np.asarray(row, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be {k} number(s), not {row!r}") from None
    if a.size != k:
        raise ValueError(f"{what} must hold {k} number(s) (one per channel), not {a.size}")
    if not np.isfinite(a).all() or (np.abs(a) > VALUE_MAX).any():
        raise ValueError(f"{what} must be finite and at most 2^20 in magnitude, not {a.tolist()}")
    return tuple(float(v) for v in a)


def _object_rows(d, k, what) -> dict:
    if not isinstance(d, dict):
        raise ValueError(f"{what} must map object ids to rows of {k} value(s), not {d!r}")
    out = {}
    for key, row in d.items():
        try:
            oid = int(key) if isinstance(key, str) else selection.integer(key, f"an object id in {what}")
        except ValueError:
            raise ValueError(f"an object id in {what} must be an integer, not {key!r}") from None
        if oid < 0:
            raise ValueError(f"an object id in {what} is not negative")
        if oid in out:
            raise ValueError(f"{what} names object {oid} twice")
        out[oid] = _row(row, k, f"{what}[{oid}]")
    return out


def set_args(channels=("dye",), diffusivity=(1e-4,), values=None, sources=None, every=1, material="fluid", objects=None) -> dict:
    """The arguments of `set_scalars`, checked without a context.  Returns {"channels": names, "diffusivity": f32 values, "values":
    None | f64 array [n, K] | {object id: row}, "sources": {object id: row}, "every", "material": id or -1, "objects": ids}.
    ValueError otherwise."""
    if isinstance(channels, str):
        channels = (channels,)
    try:
        names = list(channels)
    except TypeError:
        raise ValueError(f"channels must be 1 to {MAX_CHANNELS} names, not {channels!r}") from None
    if not 1 <= len(names) <= MAX_CHANNELS or not all(isinstance(n, str) and n for n in names):
        raise ValueError(f"channels must be 1 to {MAX_CHANNELS} non-empty names, not {channels!r}")
    if len(set(names)) != len(names):
        raise ValueError(f"channels holds a duplicate name: {names}")
    k = len(names)
    try:
        kap = np.asarray(diffusivity, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"diffusivity must be {k} number(s), not {diffusivity!r}") from None
    if kap.size != k:
        raise ValueError(f"diffusivity must hold one value per channel ({k}), not {kap.size}")
    with np.errstate(over="ignore"):
        kap32 = kap.astype(np.float32)
    if not np.isfinite(kap32).all() or (kap32 < 0).any():
        raise ValueError(f"diffusivity must be finite (as f32) and not negative, not {kap.tolist()}")
    every = selection.integer(every, "every")
    if every < 1:
        raise ValueError("every must be at least 1")
    mat, ids = selection.parse(material, objects)
    src = {} if sources is None else _object_rows(sources, k, "sources")
    if len(src) > MAX_SOURCES:
        raise ValueError(f"at most {MAX_SOURCES} source objects")
    if values is None or isinstance(values, dict):
        vals = None if values is None else _object_rows(values, k, "values")
    else:
        try:
            vals = np.array(values, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("values must be None, an array [n_ids, K] or {object id: row}") from None
        if vals.ndim == 1 and k == 1:
            vals = vals.reshape(-1, 1)
        if vals.ndim != 2 or vals.shape[1] != k or vals.shape[0] < 1:
            raise ValueError(f"values must have shape [n_ids, {k}], not {list(vals.shape)}")
        if not np.isfinite(vals).all() or (np.abs(vals) > VALUE_MAX).any():
            raise ValueError("values must be finite and at most 2^20 in magnitude")
    return {"channels": names, "diffusivity": tuple(float(v) for v in kap32), "values": vals, "sources": src, "every": every,
            "material": mat, "objects": ids}


def check_paint(paint, channels) -> dict:
    """{"channel": index, "range": (lo, hi) or None, "colormap"} of a paint entry / of `paint`'s arguments.  ValueError otherwise."""
    from . import render
    spec = selection.config_object(paint, "paint", PAINT_KEYS)
    ch = spec.get("channel", 0)
    if isinstance(ch, str):
        if ch not in channels:
            raise ValueError(f"paint: channel must be one of {list(channels)} or an index, not {ch!r}")
        ch = list(channels).index(ch)
    ch = selection.integer(ch, "paint: channel")
    if not 0 <= ch < len(channels):
        raise ValueError(f"paint: channel {ch} is outside [0, {len(channels)})")
    rng = spec.get("range")
    if rng is not None:
        rng = render.check_range(rng)
    return {"channel": ch, "range": rng, "colormap": spec.get("colormap", "heat"), "lut": lut(spec.get("colormap", "heat"))}


def lut(colormap) -> np.ndarray:
    """int32 [256, 3] of a built-in map's name or a uint8 [256, 3] array (render.FieldColour's rule)."""
    from . import render
    if isinstance(colormap, str):
        return render.colormap(colormap).astype(np.int32)
    a = np.asarray(colormap)
    if a.dtype != np.uint8 or a.shape != (256, 3):
        raise ValueError(f"colormap must be a built-in name or a uint8 [256, 3] array, not {a.dtype} {list(a.shape)}")
    return np.ascontiguousarray(a, dtype=np.int32)


def scalars_config(config):
    """The scene's "scalars" object in the Configuration: {"channels": [...], "diffusivity": [...], "values": {object id: row},
    "sources": {object id: row}, "every": n, "material": "fluid", "objects": [...], "paint": {"channel", "range", "colormap"}}, every key
    optional.  Returns (keyword arguments of `set_scalars`, checked paint entry or None), or None when the key is absent.  A misspelt
    key or a bad value raises ValueError."""
    spec = selection.config_object(config, "scalars", CONFIG_KEYS)
    if spec is None:
        return None
    kw = {"channels": spec.get("channels", ("dye",)), "diffusivity": spec.get("diffusivity", (1e-4,)), "values": spec.get("values"),
          "sources": spec.get("sources"), "every": spec.get("every", 1), "material": spec.get("material", "fluid"),
          "objects": spec.get("objects")}
    try:
        if kw["values"] is not None and not isinstance(kw["values"], dict):
            raise ValueError("values must map object ids to rows in a scene file")
        a = set_args(**kw)
        paint = check_paint(spec["paint"], a["channels"]) if "paint" in spec else None
    except ValueError as e:
        raise ValueError(f'"scalars": {e}') from e
    return kw, paint


def expand(values, sources, object_of_id, k) -> np.ndarray:
    """The f64 [n_ids, K] initial values in id order: zeros, an array as given (its length must be n_ids) or {object id: row}
    spread over the ids of each object; then the rows of `sources` over the ids of the source objects, so that `values()`
    shows a source's particles at their prescribed value.  `object_of_id`: int [n_ids]."""
    object_of_id = np.asarray(object_of_id)
    n = object_of_id.shape[0]
    if isinstance(values, np.ndarray):
        if values.shape[0] != n:
            raise ValueError(f"values has {values.shape[0]} rows, the particle set has {n} ids")
        out = values.astype(np.float64, copy=True)
    else:
        out = np.zeros((n, k), dtype=np.float64)
        for oid, row in (values or {}).items():
            out[object_of_id == oid] = row
    for oid, row in sources.items():
        out[object_of_id == oid] = row
    return out


def scalar_params(a):
    """SphScalarParams of checked arguments (`set_args`)."""
    from . import _lib
    p = _lib.SphScalarParams()
    p.K = len(a["channels"])
    for k, v in enumerate(a["diffusivity"]):
        p.kappa[k] = v
    p.every = a["every"]
    selection.fill(p.select, a["material"], a["objects"])
    p.n_sources = len(a["sources"])
    for s, (oid, row) in enumerate(a["sources"].items()):
        p.source_object[s] = oid
        for k, v in enumerate(row):
            p.source_value[s][k] = v
    return p


class ScalarInfo:
    def __init__(self, i):
        self.K, self.every, self.ids = int(i.K), int(i.every), int(i.ids)
        self.samples, self.steps_seen = int(i.samples), int(i.steps_seen)
        self.overshoot = [int(i.overshoot[k]) for k in range(self.K)]
        self.saturated = [int(i.saturated[k]) for k in range(self.K)]

    def __repr__(self):
        return (f"ScalarInfo(K={self.K}, every={self.every}, ids={self.ids}, samples={self.samples}, steps_seen={self.steps_seen}, "
                f"overshoot={self.overshoot}, saturated={self.saturated})")


class Scalars:
    """The registered set of a ParticleSystem.  Every accessor downloads (and synchronises)."""

    def __init__(self, ps, args, n_ids):
        self._ps = ps
        self.channels = list(args["channels"])
        self.diffusivity = tuple(args["diffusivity"])
        self.sources = dict(args["sources"])
        self.every, self.n_ids = int(args["every"]), int(n_ids)
        self._material, self._objects = int(args["material"]), list(args["objects"])     # the carriers' selection (carriers())

    def _channel(self, channel) -> int:
        if isinstance(channel, str):
            if channel not in self.channels:
                raise ValueError(f"channel must be one of {self.channels} or an index, not {channel!r}")
            return self.channels.index(channel)
        ch = selection.integer(channel, "channel")
        if not 0 <= ch < len(self.channels):
            raise ValueError(f"channel {ch} is outside [0, {len(self.channels)})")
        return ch

    def info(self) -> ScalarInfo:
        from . import _lib
        i = _lib.SphScalarInfo()
        self._ps._call("sph_scalars_info", C.byref(i))
        return ScalarInfo(i)

    @property
    def samples(self) -> int:
        return self.info().samples

    def sample(self):
        """One sample of the current state outside a step (sph_scalars_sample); needs the neighbour structure."""
        self._ps._call("sph_scalars_sample")

    def raw(self) -> np.ndarray:
        """i64 [n_ids, K] by persistent id: the value times 2^32."""
        out = np.zeros((self.n_ids, len(self.channels)), np.int64)
        self._ps._call("sph_scalars_download", out.ctypes.data_as(C.c_void_p), None, self.n_ids)
        return out

    def values(self) -> np.ndarray:
        """f64 [n_ids, K] by persistent id."""
        out = np.zeros((self.n_ids, len(self.channels)), np.float64)
        self._ps._call("sph_scalars_download", None, out.ctypes.data_as(C.c_void_p), self.n_ids)
        return out

    def carriers(self) -> np.ndarray:
        """bool [n_ids]: the ids the registered selection makes carriers (one download of material and object by id)."""
        ps = self._ps
        pid = ps.pid.to_numpy()
        mat, obj = np.zeros(self.n_ids, np.int64), np.zeros(self.n_ids, np.int64)
        mat[pid], obj[pid] = ps.material.to_numpy(), ps.object_id.to_numpy()
        sel = np.ones(self.n_ids, bool)
        if self._material >= 0:
            sel &= mat == self._material
        if self._objects:
            sel &= np.isin(obj, self._objects)
        return sel & ~np.isin(obj, list(self.sources))

    def total(self, channel=0) -> int:
        """The integer sum of the carriers' raw values of `channel`: with one fluid of equal volumes and no sources it never changes."""
        return int(self.raw()[self.carriers(), self._channel(channel)].sum(dtype=np.int64))

    def range(self, channel=0) -> tuple:
        """(min, max) of the carriers' values of `channel`; (0.0, 0.0) with no carrier."""
        v = self.values()[self.carriers(), self._channel(channel)]
        return (float(v.min()), float(v.max())) if v.size else (0.0, 0.0)

    def overshoot(self) -> list:
        """Per channel: carriers (summed over the samples) whose weights exceeded 1 -- the explicit step beyond its stability limit."""
        return self.info().overshoot

    def saturated(self) -> list:
        return self.info().saturated

    def paint(self, channel=0, range=None, colormap="heat"):
        """Write the table colour of every carrier's and source's value of `channel` into its object colour (`ps.color`), which both
        frame styles draw.  `range` None: the carriers' (min, max), (lo, lo + 1) where that is no usable range.  Returns the range used."""
        from . import render
        ch = self._channel(channel)
        table = lut(colormap)
        if range is None:
            lo, hi = self.range(ch)
            rng = render.auto_range(lo, hi, 1)
        else:
            rng = render.check_range(range)
        self._ps._call("sph_scalars_paint", ch, C.c_float(rng[0]), C.c_float(rng[1]), table.ctypes.data_as(C.c_void_p))
        return rng

    def save(self, path):
        """npz of `ids` (0 .. n_ids - 1), `values` f64 [n_ids, K], `raw` i64 and the channel names: `set_scalars(values=...)` restores them."""
        raw = self.raw()
        np.savez(path, ids=np.arange(self.n_ids, dtype=np.int64), values=raw.astype(np.float64) / float(1 << SCALE_LOG2), raw=raw,
                 channels=np.array(self.channels))


def _refuse_slab(ps):
    if ps.slab is not None:
        raise NotImplementedError("carried scalars exist on single-domain contexts only: a carrier's neighbours beyond the halo "
                                  "belong to another rank and the store is indexed by global id")


def set_scalars(ps, channels=("dye",), diffusivity=(1e-4,), values=None, sources=None, every=1, material="fluid", objects=None) -> Scalars:
    a = set_args(channels, diffusivity, values, sources, every, material, objects)
    _refuse_slab(ps)
    n_ids = int(ps.particle_max_num)
    k = len(a["channels"])
    if isinstance(a["values"], dict) or a["sources"]:
        object_of_id = np.zeros(n_ids, np.int64)
        object_of_id[ps.pid.to_numpy()] = ps.object_id.to_numpy()      # one download of object ids by pid
        init = expand(a["values"], a["sources"], object_of_id, k)
    elif a["values"] is None:
        init = None
    else:
        if a["values"].shape[0] != n_ids:
            raise ValueError(f"values has {a['values'].shape[0]} rows, the particle set has {n_ids} ids")
        init = a["values"]
    p = scalar_params(a)
    init = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
    ps._call("sph_scalars_set", None if init is None else init.ctypes.data_as(C.c_void_p), n_ids, C.byref(p))
    return Scalars(ps, a, n_ids)


def clear_scalars(ps):
    _refuse_slab(ps)
    ps._call("sph_scalars_set", None, 0, None)
