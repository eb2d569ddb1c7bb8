"""The fluid surface as a triangle mesh: what `ParticleSystem.surface_mesh()` returns and the binary PLY it writes
(include/sph_hip.h, section "Surface mesh"; csrc/sph_mesh.hip).

Surface nets on the sampler's weight plane (sample.py: weight / 2^30 is about 0.8 inside a fluid at rest spacing and falls to 0
across the free surface): one vertex per grid cell whose corners are partly inside, one quad per grid edge that crosses the
surface.  The field is a plane of integers, so inside / outside is an integer compare and the mesh is the same bytes for any
particle order.  Classification, numbering, vertices and faces are made on the device; only the mesh crosses to the host.
Nothing in this module touches the GPU when it is imported: the library is reached through the ParticleSystem handed to
`surface_mesh`.
"""
from __future__ import annotations

import math

import numpy as np

from . import sample as _sample
from . import selection

ISO_MAX = 4.0
CONFIG_KEYS = ("spacing", "origin", "shape", "iso", "cap", "objects")


def mesh_args(iso=0.4, cap=True) -> dict:
    """`iso` and `cap` checked without a context: {"iso": the f32 value as a float, "cap": bool}.  ValueError otherwise."""
    if isinstance(iso, (bool, np.bool_)) or not isinstance(iso, (int, float, np.integer, np.floating)):
        raise ValueError(f"iso must be a number, not {iso!r}")
    with np.errstate(over="ignore"):
        f = float(np.float32(iso))
    if not math.isfinite(f) or not 0.0 < f <= ISO_MAX:
        raise ValueError(f"iso must be finite and in (0, {ISO_MAX:g}] (as f32), not {iso!r}")
    if not isinstance(cap, (bool, np.bool_)):
        raise ValueError(f"cap must be true or false, not {cap!r}")
    return {"iso": f, "cap": bool(cap)}


def grid_args(spacing=None, origin=None, shape=None, *, particle_diameter, domain_size) -> dict:
    """`sample.grid_args`, and every node count at least 2: a mesh needs cells."""
    ga = _sample.grid_args(spacing, origin, shape, particle_diameter=particle_diameter, domain_size=domain_size)
    if min(ga["shape"]) < 2:
        raise ValueError(f"every node count must be at least 2 for a mesh (a slice has no cells), not {ga['shape']}")
    return ga


class SurfaceMesh:
    """One extracted mesh: `vertices` f32 [V, 3], `normals` f32 [V, 3] (unit, out of the fluid), `triangles` i32 [T, 3]
    (counter-clockwise seen from outside), plus `time`, `iso` and the `origin`, `spacing`, `shape` of the grid it was cut from."""

    def __init__(self, vertices, normals, triangles, *, time, iso, origin, spacing, shape):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        self.triangles = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        if self.normals.shape != self.vertices.shape:
            raise ValueError("one normal per vertex")
        self.time, self.iso = float(time), float(iso)
        self.origin, self.spacing = _sample._triple(origin, "origin"), _sample._triple(spacing, "spacing")
        self.shape = tuple(int(n) for n in shape)

    def _corners(self):
        v = self.vertices.astype(np.float64)
        t = self.triangles
        return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]

    def volume(self) -> float:
        """The enclosed volume by the divergence theorem, sum of a . (b x c) / 6 over the triangles, in f64: positive for
        outward orientation.  It means something for a closed mesh only."""
        a, b, c = self._corners()
        return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)

    def area(self) -> float:
        a, b, c = self._corners()
        return float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)

    def directed_edges(self) -> np.ndarray:
        """i64 [3 T, 2]: the directed edges (from, to) of every triangle."""
        t = self.triangles.astype(np.int64)
        return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=0)

    def boundary_edges(self) -> np.ndarray:
        """The directed edges that have no reverse (with multiplicity), i64 [B, 2]: empty for a closed mesh."""
        e = self.directed_edges()
        n = max(int(self.vertices.shape[0]), 1)
        fwd, rev = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
        codes, counts = np.unique(fwd, return_counts=True)
        rcodes, rcounts = np.unique(rev, return_counts=True)
        have = dict(zip(rcodes.tolist(), rcounts.tolist()))
        out = []
        for code, k in zip(codes.tolist(), counts.tolist()):
            out += [(code // n, code % n)] * max(k - have.get(code, 0), 0)
        return np.asarray(out, dtype=np.int64).reshape(-1, 2)

    def is_closed(self) -> bool:
        """True iff every directed edge is matched by its reverse."""
        e = self.directed_edges()
        n = max(int(self.vertices.shape[0]), 1)
        return bool(np.array_equal(np.sort(e[:, 0] * n + e[:, 1]), np.sort(e[:, 1] * n + e[:, 0])))

    def write_ply(self, path, comments=()):
        """Binary little-endian PLY: vertices `x y z nx ny nz` float, faces `list uchar int vertex_indices`."""
        V, T = self.vertices.shape[0], self.triangles.shape[0]
        head = ["ply", "format binary_little_endian 1.0", "comment created by sph_taichi_amd", f"comment time {self.time!r}",
                f"comment iso {self.iso!r}"] + [f"comment {c}" for c in comments]
        head += [f"element vertex {V}"] + [f"property float {p}" for p in ("x", "y", "z", "nx", "ny", "nz")]
        head += [f"element face {T}", "property list uchar int vertex_indices", "end_header"]
        rows = np.empty(V, dtype=np.dtype([("p", "<f4", 3), ("n", "<f4", 3)]))
        rows["p"], rows["n"] = self.vertices, self.normals
        faces = np.empty(T, dtype=np.dtype([("k", "u1"), ("i", "<i4", 3)]))
        faces["k"], faces["i"] = 3, self.triangles
        with open(path, "wb") as fh:
            fh.write(("\n".join(head) + "\n").encode("ascii"))
            fh.write(rows.tobytes())
            fh.write(faces.tobytes())


def mesh_config(config):
    """The scene's "exportMesh" object: {"spacing": s, "origin": [..], "shape": [..], "iso": 0.4, "cap": true, "objects": [..]},
    every key optional ({} = the fluid on the default grid).  Returns the keyword arguments of `surface_mesh`, or None when the key
    is absent.  A misspelt key or a bad value raises ValueError."""
    spec = selection.config_object(config, "exportMesh", CONFIG_KEYS)
    if spec is None:
        return None
    kw = {"spacing": spec.get("spacing"), "origin": spec.get("origin"), "shape": spec.get("shape"), "iso": spec.get("iso", 0.4),
          "cap": spec.get("cap", True), "objects": spec.get("objects")}
    try:
        mesh_args(kw["iso"], kw["cap"])
        selection.parse("fluid", kw["objects"])
        if kw["shape"] is not None:
            grid_args(kw["spacing"], kw["origin"], kw["shape"], particle_diameter=1.0, domain_size=(1.0, 1.0, 1.0))
        else:
            _sample.grid_args(kw["spacing"], kw["origin"], None, particle_diameter=1.0, domain_size=(1.0, 1.0, 1.0))
    except ValueError as e:
        raise ValueError(f'"exportMesh": {e}') from e
    return kw


def extract_raw(ps, iso, cap):
    """sph_mesh_extract on the last sampled grid + counts + download: (vertices, normals, triangles) (synchronises)."""
    import ctypes as C
    from . import _lib
    spec = _lib.SphMeshSpec()
    spec.iso, spec.cap = iso, 1 if cap else 0
    ps._call("sph_mesh_extract", C.byref(spec))
    nv, nt = C.c_int64(), C.c_int64()
    ps._call("sph_mesh_counts", C.byref(nv), C.byref(nt))
    pos, nrm = np.empty((nv.value, 3), dtype=np.float32), np.empty((nv.value, 3), dtype=np.float32)
    tri = np.empty((nt.value, 3), dtype=np.int32)
    ps._call("sph_mesh_download", pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p), tri.ctypes.data_as(C.c_void_p),
             nv.value, nt.value)
    return pos, nrm, tri


def surface_mesh(ps, spacing=None, origin=None, shape=None, iso=0.4, cap=True, material="fluid", objects=None) -> SurfaceMesh:
    import ctypes as C
    from . import _lib
    ma = mesh_args(iso, cap)
    mat, ids = selection.parse(material, objects)
    ga = grid_args(spacing, origin, shape, particle_diameter=ps.particle_diameter, domain_size=ps.domain_size)
    if ps.slab is not None:
        raise NotImplementedError("meshes are extracted on single-domain contexts only: a slab rank's ghost records would be "
                                  "counted twice in the grid the surface is cut from")
    g = _lib.SphSampleGrid()
    g.n = (C.c_int32 * 3)(*ga["shape"])
    g.origin, g.spacing = (C.c_float * 3)(*ga["origin"]), (C.c_float * 3)(*ga["spacing"])
    g.inv_h, g.fields, g.select = _sample.inv_h_f32(ps.support_radius), 0, selection.fill(_lib.SphSampleSelect(), mat, ids)   # no field planes: the weight alone
    ps._call("sph_sample_grid", C.byref(g))
    pos, nrm, tri = extract_raw(ps, ma["iso"], ma["cap"])
    return SurfaceMesh(pos, nrm, tri, time=ps.time, iso=ma["iso"], origin=ga["origin"], spacing=ga["spacing"], shape=ga["shape"])
