"""Depth-integrated column maps: what `ParticleSystem.column_map()` returns (include/sph_hip.h, section "Depth-integrated
column maps"; csrc/sph_columns.hip).

The Eulerian view of a free-surface run: a 2-D map of columns along a chosen up axis with, per column, the number of fluid
particles, the top and the bottom of the fluid and the summed velocity -- wave gauges, depth profiles h(x, z), the position
of the wet front.  One streaming pass on the device; only the map crosses to the host.  Nothing in this module touches the
GPU when it is imported: the library is reached through the ParticleSystem handed to `reduce`.

The index arithmetic is the kernel's, operation by operation in f32: k = floor((x - origin) * inv_cell) with
inv_cell = f32(1) / f32(cell); a point is inside when 0 <= k < n on both horizontal axes.
"""
from __future__ import annotations

import math

import numpy as np

from . import selection

V_SCALE_LOG2 = 20                    # the velocity sums are fixed point: llrint(v * 2^20) per particle and component
COLUMNS_MAX = 1 << 20


def horizontal_axes(axis: int):
    """The two axes a map spans, ascending: the axes other than `axis`."""
    if axis not in (0, 1, 2):
        raise ValueError(f"axis must be 0, 1 or 2, not {axis!r}")
    return tuple(j for j in range(3) if j != axis)


def _pair(value, name):
    a = np.asarray(value, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 2)
    if a.size != 2:
        raise ValueError(f"{name} must be one number or one per horizontal axis")
    return float(a[0]), float(a[1])


def inv_cell_f32(cell):
    """f32(1) / f32(cell) per horizontal axis: the factor handed to the kernel."""
    return tuple(np.float32(1) / np.float32(c) for c in cell)


def column_index(points, origin, inv_cell, shape):
    """The kernel's index arithmetic on points [..., 2] (the two horizontal coordinates): (k0, k1, inside) with k as f32
    floors cast to int64 (meaningless where `inside` is False)."""
    p = np.asarray(points, dtype=np.float32)
    if p.shape[-1] != 2:
        raise ValueError("points must hold the two horizontal coordinates in their last dimension")
    ks, inside = [], np.ones(p.shape[:-1], dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(2):
            f = np.floor((p[..., j] - np.float32(origin[j])) * np.float32(inv_cell[j]))       # f32 subtract, f32 multiply, floor
            ok = (f >= np.float32(0)) & (f < np.float32(shape[j]))                            # on the float: NaN is outside
            inside &= ok
            ks.append(np.where(ok, f, np.float32(0)).astype(np.int64))
    return ks[0], ks[1], inside


class ColumnMap:
    """The raw arrays of one map -- `count` [n0, n1] i64, `sum_v` [3, n0, n1] i64 (fixed point, 2^-20), `top`, `bottom`
    [n0, n1] f32 (0 where empty) -- the scalars `selected`, `binned`, `outside`, `time`, `axis`, `cell`, `origin`, and what
    follows from them.  The first map index runs along the lower horizontal axis, the second along the higher."""

    def __init__(self, count, sum_v, top, bottom, *, selected, binned, outside, time, axis, cell, origin, particle_diameter,
                 object_id=None):
        self.count = np.asarray(count, dtype=np.int64)
        if self.count.ndim != 2:
            raise ValueError("count must be [n0, n1]")
        self.shape = tuple(int(n) for n in self.count.shape)
        self.sum_v = np.asarray(sum_v, dtype=np.int64).reshape((3,) + self.shape)
        self.top = np.asarray(top, dtype=np.float32).reshape(self.shape)
        self.bottom = np.asarray(bottom, dtype=np.float32).reshape(self.shape)
        self.selected, self.binned, self.outside = int(selected), int(binned), int(outside)
        self.time = float(time)
        self.axis = int(axis)
        self.axes = horizontal_axes(self.axis)
        self.cell = _pair(cell, "cell")
        self.origin = _pair(origin, "origin")
        self.inv_cell = inv_cell_f32(self.cell)
        self.particle_diameter = float(particle_diameter)
        self.particle_radius = 0.5 * self.particle_diameter
        self.object_id = None if object_id is None else int(object_id)

    # ---- derived views ----
    @property
    def wet(self):
        return self.count > 0

    @property
    def depth(self):
        """Equivalent water depth: count * particle_diameter^3 / (cell_0 * cell_1); a rest lattice of height H gives H."""
        return self.count * (self.particle_diameter ** 3 / (self.cell[0] * self.cell[1]))

    @property
    def surface(self):
        """Surface elevation: top + particle_radius (f64), NaN where the column is empty."""
        return np.where(self.wet, self.top.astype(np.float64) + self.particle_radius, np.nan)

    @property
    def velocity(self):
        """Column-averaged velocity [n0, n1, 3] in f64: sum_v / 2^20 / count, NaN where the column is empty."""
        n = np.where(self.wet, self.count, 1).astype(np.float64)
        v = self.sum_v.astype(np.float64) / float(1 << V_SCALE_LOG2) / n
        return np.moveaxis(np.where(self.wet, v, np.nan), 0, -1)

    def column_of(self, points):
        """Flat column index k0 * n1 + k1 of points [..., 2] (horizontal coordinates, ascending axis order) by the
        kernel's f32 arithmetic; -1 for points outside the map."""
        k0, k1, inside = column_index(points, self.origin, self.inv_cell, self.shape)
        return np.where(inside, k0 * self.shape[1] + k1, -1)

    def gauge(self, points):
        """depth, surface and velocity at the columns of `points`; NaN for points outside the map."""
        col = np.atleast_1d(self.column_of(points))
        inside = col >= 0
        safe = np.where(inside, col, 0)
        depth = np.where(inside, self.depth.reshape(-1)[safe], np.nan)
        surface = np.where(inside, self.surface.reshape(-1)[safe], np.nan)
        velocity = np.where(inside[..., None], self.velocity.reshape(-1, 3)[safe], np.nan)
        return {"column": col, "depth": depth, "surface": surface, "velocity": velocity}

    def wet_extent(self, min_count: int = 1):
        """Per horizontal axis (low edge of the first wet column, high edge of the last wet column), a column being wet
        when it holds at least `min_count` particles; None when no column is: the position of the front."""
        wet = self.count >= max(int(min_count), 1)
        if not wet.any():
            return None
        out = []
        for j in range(2):
            idx = np.flatnonzero(wet.any(axis=1 - j))
            out.append((self.origin[j] + float(idx[0]) * self.cell[j], self.origin[j] + float(idx[-1] + 1) * self.cell[j]))
        return tuple(out)

    def as_dict(self) -> dict:
        nan_to_none = lambda a: [[None if (isinstance(v, float) and math.isnan(v)) else v for v in row] for row in a]
        ext = self.wet_extent()
        return {"time": self.time, "axis": self.axis, "axes": list(self.axes), "shape": list(self.shape), "cell": list(self.cell),
                "origin": list(self.origin), "object_id": self.object_id, "selected": self.selected, "binned": self.binned,
                "outside": self.outside, "wet_extent": [list(e) for e in ext] if ext is not None else None,
                "count": self.count.tolist(), "sum_v": self.sum_v.tolist(), "top": self.top.tolist(),
                "bottom": self.bottom.tolist(), "depth": self.depth.tolist(), "surface": nan_to_none(self.surface.tolist())}


def gauge_rows(cmap: ColumnMap, points):
    """JSON-ready rows of `gauge(points)` (None for NaN), one per point."""
    g = cmap.gauge(points)
    num = lambda v: None if math.isnan(v) else float(v)
    return [{"point": [float(p[0]), float(p[1])], "column": int(c), "depth": num(d), "surface": num(s),
             "velocity": [num(x) for x in v]}
            for p, c, d, s, v in zip(np.asarray(points, dtype=np.float64).reshape(-1, 2), g["column"], g["depth"], g["surface"],
                                     g["velocity"])]


def gauges_config(config) -> dict:
    """The scene's "gauges" object: {"axis": 1, "cell": c, "points": [[a, b], ...]}.  Key absent: axis 1, the default cell
    (None: the support radius) and no points.  A misspelt key raises."""
    out = {"axis": 1, "cell": None, "points": []}
    spec = selection.config_object(config, "gauges", out)
    if spec is None:
        return out
    out["axis"] = int(spec.get("axis", 1))
    horizontal_axes(out["axis"])
    if spec.get("cell") is not None:
        out["cell"] = spec["cell"]
        if min(_pair(out["cell"], "cell")) <= 0:
            raise ValueError('"gauges": cell must be positive')
    pts = np.asarray(spec.get("points", []), dtype=np.float64)
    if pts.size and (pts.ndim != 2 or pts.shape[1] != 2):
        raise ValueError('"gauges": points must be a list of [a, b] pairs (the two horizontal coordinates)')
    out["points"] = pts.reshape(-1, 2).tolist()
    return out


def heightmap_image(cmap: ColumnMap, height: float) -> np.ndarray:
    """`surface` as 8-bit grey, uint8 [n0, n1, 3]: round(255 * surface / height) clipped to [0, 255], 0 where empty."""
    s = np.nan_to_num(cmap.surface, nan=0.0) / float(height)
    g = np.rint(np.clip(s, 0.0, 1.0) * 255.0).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)


def map_params(ps, axis=1, cell=None, origin=None, shape=None, object_id=None):
    """Defaults resolved against a ParticleSystem: cell = support radius, origin = 0, shape = ceil(domain_size_j / cell_j).
    Returns (axis, cell pair, origin pair, shape pair, object id or -1)."""
    axes = horizontal_axes(int(axis))
    cell = _pair(ps.support_radius if cell is None else cell, "cell")
    if not all(c > 0 and math.isfinite(c) for c in cell):
        raise ValueError("cell must be positive")
    origin = _pair(0.0 if origin is None else origin, "origin")
    if shape is None:
        shape = tuple(max(int(math.ceil(float(ps.domain_size[j]) / c)), 1) for j, c in zip(axes, cell))
    shape = (int(shape[0]), int(shape[1]))
    return int(axis), cell, origin, shape, -1 if object_id is None else int(object_id)


def download_raw(ps, axis, cell, origin, shape, object_id):
    """sph_columns_reduce + sph_columns_download: (count, sum_v, top, bottom, totals) as numpy arrays and the totals struct
    (synchronises)."""
    import ctypes as C
    from . import _lib
    p = _lib.SphColumnParams()
    p.axis, p.object_id = int(axis), int(object_id)
    p.n = (C.c_int32 * 2)(int(shape[0]), int(shape[1]))
    p.origin = (C.c_float * 2)(*[float(np.float32(o)) for o in origin])
    p.inv_cell = (C.c_float * 2)(*[float(v) for v in inv_cell_f32(cell)])
    ps._call("sph_columns_reduce", C.byref(p))
    nc = int(shape[0]) * int(shape[1])
    count, sum_v = np.empty(nc, dtype=np.int64), np.empty(3 * nc, dtype=np.int64)
    top, bottom = np.empty(nc, dtype=np.float32), np.empty(nc, dtype=np.float32)
    totals = _lib.SphColumnTotals()
    ps._call("sph_columns_download", count.ctypes.data_as(C.c_void_p), sum_v.ctypes.data_as(C.c_void_p),
             top.ctypes.data_as(C.c_void_p), bottom.ctypes.data_as(C.c_void_p), nc, C.byref(totals))
    return count.reshape(shape), sum_v.reshape((3,) + tuple(shape)), top.reshape(shape), bottom.reshape(shape), totals


def reduce(ps, axis=1, cell=None, origin=None, shape=None, object_id=None) -> ColumnMap:
    if ps.slab is not None:
        raise NotImplementedError("column maps exist on single-domain contexts only: a slab rank's ghost records would be "
                                  "counted twice (the maps of the ranks' owned ranges would have to be all-reduced)")
    axis, cell, origin, shape, oid = map_params(ps, axis, cell, origin, shape, object_id)
    count, sum_v, top, bottom, totals = download_raw(ps, axis, cell, origin, shape, oid)
    return ColumnMap(count, sum_v, top, bottom, selected=totals.selected, binned=totals.binned, outside=totals.outside,
                     time=ps.time, axis=axis, cell=cell, origin=origin, particle_diameter=ps.particle_diameter,
                     object_id=None if oid < 0 else oid)
