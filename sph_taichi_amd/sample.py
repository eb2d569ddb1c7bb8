"""Field sampling: what `ParticleSystem.sample_grid()` and `ParticleSystem.sample_points()` return, and the legacy VTK volume
a grid writes (include/sph_hip.h, section "Field sampling"; csrc/sph_sample.hip).

The SPH interpolation of velocity, density and pressure at places: the nodes of a regular grid (a volume, or a slice when the
shape has a 1 in it) or a handful of probe points.  One streaming pass on the device in which every selected particle adds its
kernel-weighted share to the sample positions inside its support radius; only the planes cross to the host.  The raw planes are
i64 fixed-point sums (scale 2^30): `weight` = sum of w, `sums[f]` = sum of w * A_f, `count` = number of contributing particles;
a value is sums[f] / weight.  With `gradients=` the same pass also sums the kernel-gradient terms (section "Field sampling:
gradients"): `grad_fill` = sum of h grad w, `grad_sums[f]` = sum of h grad w * A_f, from which the analytic gradient of the
interpolant follows, grad A = inv_h (grad_sums[f] - A grad_fill) / weight, and with it vorticity, divergence, strain rate, the
Q-criterion, the pressure gradient and the free-surface normal.  Nothing in this module touches the GPU when it is imported: the library is reached through the
ParticleSystem handed to `sample_grid` / `sample_points`.
"""
from __future__ import annotations

import math

import numpy as np

from . import selection
from .selection import MATERIALS, MAX_OBJECTS   # noqa: F401  (part of this module's surface)

SCALE_LOG2 = 30                      # the sums are fixed point: llrint(w * 2^30), llrint(w * A * 2^30) per contributing pair
MAX_NODES, MAX_POINTS = 1 << 24, 1024
# user-level field -> the planes it asks for, in the order of the SPH_SAMPLE_* bits
FIELD_PLANES = {"velocity": ("vx", "vy", "vz"), "density": ("density",), "pressure": ("pressure",)}
PLANE_BITS = {"vx": 1, "vy": 2, "vz": 4, "density": 8, "pressure": 16}
GRID_CONFIG_KEYS = ("spacing", "origin", "shape", "fields", "objects", "gradients")
PROBES_CONFIG_KEYS = ("points", "fields", "gradients")
FILL = "fill"                        # the one name `gradients` takes beside those of FIELD_PLANES: the fill gradient alone


def _triple(value, name):
    try:
        a = np.asarray(value, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{name} must be one number or one per axis") from e
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise ValueError(f"{name} must be one number or one per axis")
    with np.errstate(over="ignore"):
        f = a.astype(np.float32)
    if not np.isfinite(f).all():
        raise ValueError(f"{name} must be finite (as f32)")
    return tuple(float(v) for v in f)


def select_args(fields=("velocity",), material="fluid", objects=None) -> dict:
    """The selection and field arguments of `sample_grid` / `sample_points`, checked without a context: {"fields": names in
    plane order, "planes": plane names, "mask", "material": -1 or the id, "objects": list}.  ValueError otherwise."""
    if isinstance(fields, str):
        raise ValueError("fields must be a sequence of names, not one string")
    fields = list(fields)
    unknown = [f for f in fields if f not in FIELD_PLANES]
    if unknown:
        raise ValueError(f"unknown field(s) {unknown}: choose from {list(FIELD_PLANES)}")
    if len(set(fields)) != len(fields):
        raise ValueError("a field is named twice")
    names = tuple(n for n in FIELD_PLANES if n in fields)
    planes = tuple(p for n in names for p in FIELD_PLANES[n])
    mask = 0
    for p in planes:
        mask |= PLANE_BITS[p]
    mat, ids = selection.parse(material, objects)
    return {"fields": names, "planes": planes, "mask": mask, "material": mat, "objects": ids}


def gradient_args(gradients=(), fields=("velocity",)) -> dict:
    """The `gradients` argument of `sample_grid` / `sample_points`, checked without a context against the (checked) `fields`:
    {"names": field names in plane order, "planes": the planes whose gradient sums are asked for, "mask", "any": whether the
    gradient-carrying entry is called at all}.  The fill gradient comes with any non-empty `gradients`; ("fill",) asks for it
    alone.  ValueError for one string, an unknown name, a name given twice and a name that is not in `fields`."""
    if isinstance(gradients, str):
        raise ValueError("gradients must be a sequence of names, not one string")
    gradients = list(gradients)
    unknown = [g for g in gradients if g != FILL and g not in FIELD_PLANES]
    if unknown:
        raise ValueError(f"unknown gradient(s) {unknown}: choose from {list(FIELD_PLANES) + [FILL]}")
    if len(set(gradients)) != len(gradients):
        raise ValueError("a gradient is named twice")
    missing = [g for g in gradients if g != FILL and g not in fields]
    if missing:
        raise ValueError(f"the gradient of {missing} needs that field's sums: name it in fields as well")
    names = tuple(n for n in FIELD_PLANES if n in gradients)
    planes = tuple(p for n in names for p in FIELD_PLANES[n])
    mask = 0
    for p in planes:
        mask |= PLANE_BITS[p]
    return {"names": names, "planes": planes, "mask": mask, "any": bool(gradients)}


def grid_args(spacing=None, origin=None, shape=None, *, particle_diameter, domain_size) -> dict:
    """Defaults resolved: spacing = the particle diameter (one number: all three axes), origin = 0, shape = the nodes that
    cover the domain from the origin, ceil((domain_size - origin) / spacing) + 1 per axis.  Returns {"spacing", "origin"
    (f32 values as float triples), "shape"}.  ValueError for what no grid can have."""
    spacing = _triple(particle_diameter if spacing is None else spacing, "spacing")
    if not all(s > 0 for s in spacing):
        raise ValueError("spacing must be positive")
    origin = _triple(0.0 if origin is None else origin, "origin")
    if shape is None:
        shape = tuple(max(int(math.ceil((float(domain_size[a]) - origin[a]) / spacing[a])) + 1, 1) for a in range(3))
    else:
        try:
            shape = tuple(shape)
        except TypeError as e:
            raise ValueError("shape must be three node counts") from e
        if len(shape) != 3:
            raise ValueError("shape must be three node counts")
        shape = tuple(selection.integer(n, "a node count") for n in shape)
    if min(shape) < 1:
        raise ValueError("every node count must be at least 1 (a slice is a shape with a 1 in it)")
    if shape[0] * shape[1] * shape[2] > MAX_NODES:
        raise ValueError(f"{shape[0]} x {shape[1]} x {shape[2]} nodes: a grid holds at most {MAX_NODES}")
    return {"spacing": spacing, "origin": origin, "shape": shape}


def points_arg(points) -> np.ndarray:
    """Probe points as a contiguous f32 [m, 3]; ValueError unless 1 <= m <= 1024 and every coordinate is finite as f32."""
    try:
        p = np.asarray(points, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("points must be a list of [x, y, z] triples") from e
    if p.ndim == 1 and p.size == 3:
        p = p.reshape(1, 3)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be a list of [x, y, z] triples")
    if not 1 <= p.shape[0] <= MAX_POINTS:
        raise ValueError(f"between 1 and {MAX_POINTS} points can be sampled at once, not {p.shape[0]}")
    with np.errstate(over="ignore"):
        f = np.ascontiguousarray(p, dtype=np.float32)
    if not np.isfinite(f).all():
        raise ValueError("points must be finite (as f32)")
    return f


def node_positions(origin, spacing, shape) -> np.ndarray:
    """The kernel's node positions, f32 [n0, n1, n2, 3]: origin_a + f32(k_a) * spacing_a, one multiply and one add in f32."""
    axes = [np.float32(origin[a]) + np.arange(shape[a], dtype=np.float32) * np.float32(spacing[a]) for a in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).astype(np.float32)


class _Sampled:
    """The raw planes over any shape -- `weight`, `count` i64 [...], `sums` i64 [F, ...] with F = len(planes) -- and the f64
    views that follow from them.  A sample that carried gradients also has `grad_fill` i64 [3, ...], `grad_sums` i64
    [Fg, 3, ...] with Fg = len(grad_planes), and `inv_h`, the factor that gives the dimensionless sums their 1 / length; without
    gradients `grad_fill` is None and `grad_sums` is empty."""

    def __init__(self, weight, count, sums, planes, time, grad_fill=None, grad_sums=None, grad_planes=(), inv_h=None):
        self.weight = np.asarray(weight, dtype=np.int64)
        self.count = np.asarray(count, dtype=np.int64).reshape(self.weight.shape)
        self.planes = tuple(planes)
        self.sums = np.asarray(sums, dtype=np.int64).reshape((len(self.planes),) + self.weight.shape)
        self.fields = tuple(n for n in FIELD_PLANES if all(p in self.planes for p in FIELD_PLANES[n]))
        self.time = float(time)
        self.grad_planes = tuple(grad_planes) if grad_fill is not None else ()
        if any(p not in self.planes for p in self.grad_planes):
            raise ValueError("a gradient plane needs the sums of that plane")
        self.grad_fill = None if grad_fill is None else np.asarray(grad_fill, dtype=np.int64).reshape((3,) + self.weight.shape)
        self.grad_sums = (np.zeros((0, 3) + self.weight.shape, dtype=np.int64) if grad_fill is None or grad_sums is None else
                          np.asarray(grad_sums, dtype=np.int64).reshape((len(self.grad_planes), 3) + self.weight.shape))
        self.gradients = tuple(n for n in FIELD_PLANES if all(p in self.grad_planes for p in FIELD_PLANES[n]))
        if grad_fill is not None and inv_h is None:
            raise ValueError("gradient sums need inv_h")
        self.inv_h = None if inv_h is None else float(inv_h)

    @property
    def fill(self):
        """The Shepard sum, weight / 2^30: 0.8 inside a fluid at rest spacing (m_V0 = 0.8 d^3), falling to 0 across its surface."""
        return self.weight.astype(np.float64) / float(1 << SCALE_LOG2)

    def wet(self, threshold: float = 0.5):
        return self.fill >= float(threshold)

    def _value(self, plane):
        if plane not in self.planes:
            raise ValueError(f"{plane} was not sampled: the fields are {list(self.fields)}")
        s = self.sums[self.planes.index(plane)].astype(np.float64)
        has = self.weight != 0
        return np.where(has, s / np.where(has, self.weight, 1).astype(np.float64), np.nan)

    @property
    def velocity(self):
        """[..., 3] f64: sum / weight, NaN where weight == 0."""
        return np.stack([self._value(p) for p in FIELD_PLANES["velocity"]], axis=-1)

    @property
    def density(self):
        return self._value("density")

    @property
    def pressure(self):
        return self._value("pressure")

    # ---- gradients: every view is f64 and NaN where weight == 0 ----
    def _no_gradient(self, what):
        return ValueError(f"the gradient of {what} was not sampled: the gradients are {list(self.gradients) + ([FILL] if self.grad_fill is not None else [])}")

    @property
    def fill_gradient(self):
        """[..., 3] f64: inv_h * grad_fill / 2^30, the gradient of `fill` (it points into the fluid)."""
        if self.grad_fill is None:
            raise self._no_gradient(FILL)
        g = np.moveaxis(self.grad_fill.astype(np.float64), 0, -1) * (self.inv_h / float(1 << SCALE_LOG2))
        return np.where((self.weight != 0)[..., None], g, np.nan)

    @property
    def surface_normal(self):
        """[..., 3] f64: -fill_gradient / |fill_gradient|, out of the fluid; NaN where that length is 0."""
        g = self.fill_gradient
        length = np.sqrt((g * g).sum(axis=-1))
        ok = length > 0
        return np.where(ok[..., None], -g / np.where(ok, length, 1.0)[..., None], np.nan)

    def _gradient(self, plane):
        """[..., 3] f64: inv_h * (grad_sums[f] - A grad_fill) / weight, the gradient of the interpolant A = sums[f] / weight."""
        if plane not in self.grad_planes:
            raise self._no_gradient(plane)
        has = self.weight != 0
        w = np.where(has, self.weight, 1).astype(np.float64)
        a = self.sums[self.planes.index(plane)].astype(np.float64) / w
        s = self.grad_sums[self.grad_planes.index(plane)].astype(np.float64)
        g = (s - a[None] * self.grad_fill.astype(np.float64)) / w[None] * self.inv_h
        return np.where(has[..., None], np.moveaxis(g, 0, -1), np.nan)

    @property
    def velocity_gradient(self):
        """[..., 3, 3] f64, (component, axis): velocity_gradient[..., c, a] = d v_c / d x_a."""
        return np.stack([self._gradient(p) for p in FIELD_PLANES["velocity"]], axis=-2)

    @property
    def density_gradient(self):
        return self._gradient("density")

    @property
    def pressure_gradient(self):
        return self._gradient("pressure")

    @property
    def vorticity(self):
        """[..., 3] f64: curl v."""
        j = self.velocity_gradient
        return np.stack([j[..., 2, 1] - j[..., 1, 2], j[..., 0, 2] - j[..., 2, 0], j[..., 1, 0] - j[..., 0, 1]], axis=-1)

    @property
    def divergence(self):
        j = self.velocity_gradient
        return j[..., 0, 0] + j[..., 1, 1] + j[..., 2, 2]

    @property
    def strain_rate(self):
        """The Frobenius norm of the symmetric part S = (J + J^T) / 2 of the velocity gradient."""
        j = self.velocity_gradient
        s = 0.5 * (j + np.swapaxes(j, -1, -2))
        return np.sqrt((s * s).sum(axis=(-1, -2)))

    @property
    def q_criterion(self):
        """(|Omega|^2 - |S|^2) / 2 with Omega = (J - J^T) / 2: positive where rotation dominates strain."""
        j = self.velocity_gradient
        s, o = 0.5 * (j + np.swapaxes(j, -1, -2)), 0.5 * (j - np.swapaxes(j, -1, -2))
        return 0.5 * ((o * o).sum(axis=(-1, -2)) - (s * s).sum(axis=(-1, -2)))

    def gradient_views(self):
        """(name, f64 array) of the derived gradient fields that were sampled, in the order the VTK writer and `rows()` use."""
        out = []
        if self.grad_fill is not None:
            out.append(("fill_gradient", self.fill_gradient))
        if "velocity" in self.gradients:
            out += [("vorticity", self.vorticity), ("divergence", self.divergence), ("q_criterion", self.q_criterion)]
        for name in ("pressure", "density"):
            if name in self.gradients:
                out.append((f"{name}_gradient", self._gradient(name)))
        return out


class FieldGrid(_Sampled):
    """One sampled grid: the raw planes [n0, n1, n2] plus `time`, `origin`, `spacing`, `shape`; `fill`, `velocity`, `density`,
    `pressure`, `wet()` as f64 views; `write_vtk(path)`.  Node (k0, k1, k2) is at origin + k * spacing."""

    def __init__(self, weight, count, sums, planes, *, time, origin, spacing, shape, grad_fill=None, grad_sums=None, grad_planes=(), inv_h=None):
        self.shape = tuple(int(n) for n in shape)
        if len(self.shape) != 3:
            raise ValueError("shape must be three node counts")
        super().__init__(np.asarray(weight, dtype=np.int64).reshape(self.shape), count, sums, planes, time, grad_fill, grad_sums, grad_planes, inv_h)
        self.origin = _triple(origin, "origin")
        self.spacing = _triple(spacing, "spacing")

    @property
    def positions(self):
        return node_positions(self.origin, self.spacing, self.shape)

    def vtk_arrays(self):
        """(name, components, f32 array in VTK point order: x fastest) of what `write_vtk` writes: fill, then the fields, then
        the gradient fields of a sample that carried gradients (`gradient_views`)."""
        order = lambda a: np.ascontiguousarray(np.transpose(a, (2, 1, 0) + tuple(range(3, a.ndim))))
        out = [("fill", 1, order(self.fill).astype(np.float32))]
        for name in self.fields:
            a = getattr(self, name)
            out.append((name, 3 if name == "velocity" else 1, order(a).astype(np.float32)))
        for name, a in self.gradient_views():
            out.append((name, 3 if a.ndim == 4 else 1, order(a).astype(np.float32)))
        return out

    def write_vtk(self, path):
        """A legacy binary STRUCTURED_POINTS file: ASCII header, big-endian f32; `fill` and every scalar field as SCALARS,
        the velocity as VECTORS.  Values where nothing contributed are NaN."""
        n =self.shape[0] * self.shape[1] * self.shape[2]
        head = ["# vtk DataFile Version 3.0", f"sph_taichi_amd field grid, time {self.time!r}", "BINARY", "DATASET STRUCTURED_POINTS",
                "DIMENSIONS {} {} {}".format(*self.shape), "ORIGIN {!r} {!r} {!r}".format(*self.origin),
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


class FieldProbes(_Sampled):
    """The same views per probe point: raw planes [m], `points` f32 [m, 3]; `rows()` for JSON."""

    def __init__(self, points, weight, count, sums, planes, *, time, grad_fill=None, grad_sums=None, grad_planes=(), inv_h=None):
        self.points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        super().__init__(np.asarray(weight, dtype=np.int64).reshape(self.points.shape[0]), count, sums, planes, time, grad_fill, grad_sums,
                         grad_planes, inv_h)

    def rows(self):
        """One JSON-ready dict per point: point, count, fill, the sampled fields and the gradient fields of `gradient_views`
        (None where nothing contributed)."""
        num = lambda v: None if math.isnan(v) else float(v)
        views = {name: getattr(self, name) for name in self.fields}
        views.update(self.gradient_views())
        fill = self.fill
        out = []
        for k in range(self.points.shape[0]):
            row = {"point": [float(v) for v in self.points[k]], "count": int(self.count[k]), "fill": float(fill[k])}
            for name, a in views.items():
                row[name] = [num(v) for v in a[k]] if a.ndim == 2 else num(a[k])
            out.append(row)
        return out


def _fields_from_spec(spec, key, default, name="fields"):
    fields = spec.get(name, default)
    if isinstance(fields, str) or not isinstance(fields, (list, tuple)):
        raise ValueError(f'"{key}": {name} must be a list of names')
    return tuple(fields)


def sample_grid_config(config):
    """The scene's "sampleGrid" object: {"spacing": s, "origin": [..], "shape": [..], "fields": [..], "objects": [..],
    "gradients": [..]}, every key optional ({} = velocity on the default grid).  Returns the keyword arguments of `sample_grid`
    ("gradients" among them only when the scene names it), or None when the key is absent.  A misspelt key or a bad value
    raises ValueError."""
    spec = selection.config_object(config, "sampleGrid", GRID_CONFIG_KEYS)
    if spec is None:
        return None
    kw = {"spacing": spec.get("spacing"), "origin": spec.get("origin"), "shape": spec.get("shape"),
          "fields": _fields_from_spec(spec, "sampleGrid", ("velocity",)), "objects": spec.get("objects")}
    if "gradients" in spec:
        kw["gradients"] = _fields_from_spec(spec, "sampleGrid", (), "gradients")
    try:
        sel = select_args(fields=kw["fields"], objects=kw["objects"])
        gradient_args(kw.get("gradients", ()), sel["fields"])
        grid_args(kw["spacing"], kw["origin"], kw["shape"], particle_diameter=1.0, domain_size=(1.0, 1.0, 1.0))
    except ValueError as e:
        raise ValueError(f'"sampleGrid": {e}') from e
    return kw


def probes_config(config):
    """The scene's "probes" object: {"points": [[x, y, z], ...], "fields": [..], "gradients": [..]}.  Returns the keyword
    arguments of `sample_points` ("gradients" among them only when the scene names it), or None when the key is absent.  A
    misspelt key or a bad value raises ValueError."""
    spec = selection.config_object(config, "probes", PROBES_CONFIG_KEYS)
    if spec is None:
        return None
    if "points" not in spec:
        raise ValueError('"probes": points is missing')
    try:
        pts = points_arg(spec["points"])
        fields = _fields_from_spec(spec, "probes", ("velocity",))
        sel = select_args(fields=fields)
        kw = {"points": pts.astype(np.float64).tolist(), "fields": fields}
        if "gradients" in spec:
            kw["gradients"] = _fields_from_spec(spec, "probes", (), "gradients")
            gradient_args(kw["gradients"], sel["fields"])
    except ValueError as e:
        raise ValueError(f'"probes": {e}') from e
    return kw


def inv_h_f32(support_radius) -> float:
    """f32(1) / f32(support_radius): the factor handed to the kernels."""
    return float(np.float32(1) / np.float32(support_radius))


def make_select(args: dict):
    """SphSampleSelect of checked arguments (`select_args`)."""
    from . import _lib
    return selection.fill(_lib.SphSampleSelect(), args["material"], args["objects"])


def download_grid_raw(ps, grid, n_planes, gradients=None):
    """sph_sample_grid + sph_sample_grid_download: (weight, count, sums) as flat i64 arrays (synchronises).  With `gradients`
    (a mask of plane bits; 0 = the fill gradient alone) the gradient-carrying entry is called instead and the gradient planes
    [3 + 3 Fg, nodes] come fourth."""
    import ctypes as C
    if gradients is None:
        ps._call("sph_sample_grid", C.byref(grid))
    else:
        ps._call("sph_sample_grid_gradients", C.byref(grid), int(gradients))
    nodes = int(grid.n[0]) * int(grid.n[1]) * int(grid.n[2])
    weight, count = np.empty(nodes, dtype=np.int64), np.empty(nodes, dtype=np.int64)
    sums = np.empty((n_planes, nodes), dtype=np.int64)
    ps._call("sph_sample_grid_download", weight.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
             sums.ctypes.data_as(C.c_void_p) if n_planes else None, nodes)
    if gradients is None:
        return weight, count, sums
    grads = np.empty((3 + 3 * bin(int(gradients)).count("1"), nodes), dtype=np.int64)
    ps._call("sph_sample_grid_gradients_download", grads.ctypes.data_as(C.c_void_p), nodes)
    return weight, count, sums, grads


def _gradient_kw(ps, grads, ga) -> dict:
    """The gradient arguments of FieldGrid / FieldProbes from the downloaded planes [3 + 3 Fg, ...]."""
    return {"grad_fill": grads[:3], "grad_sums": grads[3:].reshape((len(ga["planes"]), 3) + grads.shape[1:]), "grad_planes": ga["planes"],
            "inv_h": inv_h_f32(ps.support_radius)}


def _refuse_slab(ps):
    if ps.slab is not None:
        raise NotImplementedError("fields are sampled on single-domain contexts only: a slab rank's ghost records would be "
                                  "counted twice (the planes of the ranks' owned ranges would have to be all-reduced)")


def sample_grid(ps, spacing=None, origin=None, shape=None, fields=("velocity",), material="fluid", objects=None, gradients=()) -> FieldGrid:
    import ctypes as C
    from . import _lib
    sel = select_args(fields=fields, material=material, objects=objects)
    gr = gradient_args(gradients, sel["fields"])
    ga = grid_args(spacing, origin, shape, particle_diameter=ps.particle_diameter, domain_size=ps.domain_size)
    _refuse_slab(ps)
    g = _lib.SphSampleGrid()
    g.n = (C.c_int32 * 3)(*ga["shape"])
    g.origin, g.spacing = (C.c_float * 3)(*ga["origin"]), (C.c_float * 3)(*ga["spacing"])
    g.inv_h, g.fields, g.select = inv_h_f32(ps.support_radius), sel["mask"], make_select(sel)
    if not gr["any"]:
        weight, count, sums = download_grid_raw(ps, g, len(sel["planes"]))
        return FieldGrid(weight, count, sums, sel["planes"], time=ps.time, origin=ga["origin"], spacing=ga["spacing"], shape=ga["shape"])
    weight, count, sums, grads = download_grid_raw(ps, g, len(sel["planes"]), gr["mask"])
    return FieldGrid(weight, count, sums, sel["planes"], time=ps.time, origin=ga["origin"], spacing=ga["spacing"], shape=ga["shape"],
                     **_gradient_kw(ps, grads, gr))


def sample_points(ps, points, fields=("velocity",), material="fluid", objects=None, gradients=()) -> FieldProbes:
    import ctypes as C
    sel = select_args(fields=fields, material=material, objects=objects)
    gr = gradient_args(gradients, sel["fields"])
    pts = points_arg(points)
    _refuse_slab(ps)
    m, n_planes = pts.shape[0], len(sel["planes"])
    s = make_select(sel)
    if gr["any"]:
        ps._call("sph_sample_points_gradients", pts.ctypes.data_as(C.c_void_p), m, sel["mask"], gr["mask"], C.byref(s), inv_h_f32(ps.support_radius))
    else:
        ps._call("sph_sample_points", pts.ctypes.data_as(C.c_void_p), m, sel["mask"], C.byref(s), inv_h_f32(ps.support_radius))
    weight, count = np.empty(m, dtype=np.int64), np.empty(m, dtype=np.int64)
    sums = np.empty((n_planes, m), dtype=np.int64)
    ps._call("sph_sample_points_download", weight.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
             sums.ctypes.data_as(C.c_void_p) if n_planes else None, m)
    if not gr["any"]:
        return FieldProbes(pts, weight, count, sums, sel["planes"], time=ps.time)
    grads = np.empty((3 + 3 * len(gr["planes"]), m), dtype=np.int64)
    ps._call("sph_sample_points_gradients_download", grads.ctypes.data_as(C.c_void_p), m)
    return FieldProbes(pts, weight, count, sums, sel["planes"], time=ps.time, **_gradient_kw(ps, grads, gr))
