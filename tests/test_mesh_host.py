"""Host side of the surface mesh (no GPU): the C ABI additions and their ctypes mirror, the numpy model of tests/mesh_model.py on
synthetic weight planes (topology, ordering, the volume sandwich), `SurfaceMesh` and its PLY writer, and the driver's scene key."""
import ctypes
import os
import re

import numpy as np
import pytest

from sph_taichi_amd import _lib, build, mesh
from sph_taichi_amd.config_builder import SimConfig
from tests import mesh_model as model
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
F32 = np.float32
ENTRIES = ("sph_mesh_extract", "sph_mesh_counts", "sph_mesh_download")
FULL = int(0.8 * 2 ** 30)
ORIGIN, SPACING, ISO = (0.1, -0.2, 0.3), (0.02, 0.025, 0.03), 0.4


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_section():
    assert re.search(r"typedef\s+struct\s+SphMeshSpec\s*\{\s*float\s+iso\s*;\s*int32_t\s+cap\s*;\s*\}\s*SphMeshSpec\s*;", HEADER)
    assert re.search(r"int32_t\s+sph_mesh_extract\s*\(\s*SphContext\s*\*\s*\w*\s*,\s*const\s+SphMeshSpec\s*\*\s*\w*\s*\)\s*;", HEADER)
    assert re.search(r"int32_t\s+sph_mesh_counts\s*\(\s*SphContext\s*\*\s*\w*\s*,\s*int64_t\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*\w+\s*\)\s*;", HEADER)
    assert re.search(r"int32_t\s+sph_mesh_download\s*\(\s*SphContext\s*\*\s*\w*\s*,\s*float\s*\*\s*\w+[^;]*int32_t\s*\*\s*\w+[^;]*int64_t\s+\w+\s*,\s*int64_t\s+\w+\s*\)\s*;", HEADER)
    assert re.search(r"#define\s+SPH_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6      # additive: the version stays
    assert HEADER.index("sph_mesh_extract") > HEADER.index("sph_sample_points_download")
    section = HEADER[HEADER.index("Surface mesh"):]
    for word in ("SURFACE NETS", "llrint((double)iso * 2^30)", "(0, 4]", "CAPPED FIELD", "2^41", "3 * L + a", "(C0, C1, C2)", "(C0, C3, C2)",
                 "not contracted", "SPH_E_STATE", "SPH_E_INVALID", "last good mesh"):
        assert word in section, word


def test_binding_and_build_list():
    assert ctypes.sizeof(_lib.SphMeshSpec) == 8 and _lib.SphMeshSpec.iso.offset == 0 and _lib.SphMeshSpec.cap.offset == 4
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ENTRIES:
        assert name in bound and bound[name][0] is ctypes.c_int32, name
    assert bound["sph_mesh_extract"][1] == [ctypes.c_void_p, ctypes.POINTER(_lib.SphMeshSpec)]
    assert bound["sph_mesh_counts"][1] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    assert bound["sph_mesh_download"][1] == [ctypes.c_void_p] * 4 + [ctypes.c_int64] * 2
    assert "sph_mesh.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "sph_mesh.hip"))


# ---- synthetic planes --------------------------------------------------------------------------------------------------------
def _nodes(shape):
    return np.stack(np.meshgrid(*[np.arange(k, dtype=np.float64) for k in shape], indexing="ij"), axis=-1)


def _ball(k, centre, radius):
    """A smooth blob: FULL inside, falling to 0 over two node spacings round `radius` (in node units)."""
    r = np.linalg.norm(k - np.asarray(centre, dtype=np.float64), axis=-1)
    return np.rint(FULL * np.clip((radius - r) / 2.0 + 0.5, 0.0, 1.0)).astype(np.int64)


def _plane(case):
    shape = (15, 13, 17)
    k = _nodes(shape)
    if case == "ball":
        return _ball(k, (7.2, 6.1, 8.4), 4.3)
    if case == "two balls touching":
        return np.maximum(_ball(k, (4.0, 6.0, 5.0), 2.5), _ball(k, (9.0, 6.0, 10.0), 2.5 + 0.55))   # centres sqrt(50) apart: 7.07 = the two radii + the ramps' overlap
    if case == "slab reaching the border":
        return np.rint(FULL * np.clip((6.3 - k[..., 1]) / 2.0 + 0.5, 0.0, 1.0)).astype(np.int64)     # full below k1 = 6.3 on every k0, k2
    if case == "checkerboard":
        w = np.where((k.sum(axis=-1).astype(np.int64) % 2) == 0, FULL, 0).astype(np.int64)          # every face of the interior is ambiguous
        w[5:9, 4:8, 6:10] += 1000 * np.arange(64, dtype=np.int64).reshape(4, 4, 4)                    # not all crossings at t = 1/2
        return w
    raise AssertionError(case)


CASES = ("ball", "two balls touching", "slab reaching the border", "checkerboard")
_MODEL = {}


def _mesh(case, cap):
    """The model's mesh of a case, computed once and shared (nothing changes it)."""
    if (case, cap) not in _MODEL:
        w = _plane(case)
        out = model.extract(w, ORIGIN, SPACING, ISO, cap)
        sm = mesh.SurfaceMesh(out["vertices"], out["normals"], out["triangles"], time=0.5, iso=ISO, origin=ORIGIN, spacing=SPACING, shape=w.shape)
        for a in (out["vertices"], out["normals"], out["triangles"], out["cells"], out["keys"], w):
            a.setflags(write=False)
        _MODEL[(case, cap)] = (w, out, sm)
    return _MODEL[(case, cap)]


@pytest.mark.parametrize("case", CASES)
def test_capped_mesh_is_closed_ordered_and_sandwiched(case):
    w, out, sm = _mesh(case, True)
    V, T = sm.vertices.shape[0], sm.triangles.shape[0]
    assert V > 0 and T > 0 and T % 2 == 0 and out["triangles"].dtype == np.int32 and out["vertices"].dtype == F32
    assert sm.triangles.min() >= 0 and sm.triangles.max() < V
    # every directed edge has its reverse
    assert sm.is_closed() and sm.boundary_edges().shape == (0, 2)
    # no triangle repeats a vertex index
    t = sm.triangles
    assert ((t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])).all()
    # every vertex lies inside its own cell's box (the box's corners in the same f32 arithmetic; u in [0, 1] and the rounding is monotone)
    cc = np.stack(np.unravel_index(out["cells"], tuple(k - 1 for k in w.shape)), axis=1)
    for a in range(3):
        lo = F32(ORIGIN[a]) + cc[:, a].astype(F32) * F32(SPACING[a])
        hi = F32(ORIGIN[a]) + (cc[:, a].astype(F32) + F32(1)) * F32(SPACING[a])
        assert ((sm.vertices[:, a] >= lo) & (sm.vertices[:, a] <= hi)).all(), a
    # vertex order and quad order ascend in their keys
    assert (np.diff(out["cells"]) > 0).all() and (np.diff(out["keys"]) > 0).all() and out["keys"].size * 2 == T
    # normals: unit or zero
    length = np.linalg.norm(sm.normals.astype(np.float64), axis=1)
    assert (np.isclose(length, 1.0, atol=1e-6) | (length == 0)).all()
    # the volume sandwich, tolerance-free but for the rounding of the f32 positions (relative 1e-6, from 24-bit positions)
    n_full, n_touched = model.cell_counts(w, ISO, True)
    cell = float(np.prod([float(F32(s)) for s in SPACING]))
    vol = sm.volume()
    print(f"{case}: V = {V}, T = {T}, volume = {vol!r}, sandwich [{n_full * cell!r}, {n_touched * cell!r}], area = {sm.area()!r}")
    assert vol > 0
    assert n_full * cell * (1 - 1e-6) <= vol <= n_touched * cell * (1 + 1e-6)
    assert sm.area() > 0


def test_ball_volume_and_normals_make_sense():
    w, out, sm = _mesh("ball", True)
    sphere = 4.0 / 3.0 * np.pi * 4.3 ** 3 * float(np.prod(SPACING))          # the ramp's middle (0.5 FULL = 0.4 * 2^30) sits at radius 4.3 nodes
    # A vertex is a mean of points near the sphere, so it lies inside it, by at most the sagitta of a chord as long as a cell's
    # diagonal: 4.3 - sqrt(4.3^2 - 3 / 4) = 0.088 nodes, 2 % of the radius, 6 % of the volume; 10 % leaves room for the crossings
    # themselves (the distance is not linear along an edge).  Never larger than the sphere but for that.
    assert 0.90 < sm.volume() / sphere < 1.01
    centre = np.asarray(ORIGIN) + np.asarray((7.2, 6.1, 8.4)) * np.asarray(SPACING)
    outward = (sm.vertices.astype(np.float64) - centre) / np.asarray(SPACING)  # in node units: the blob is a sphere there
    nn = sm.normals.astype(np.float64)
    assert (np.einsum("ij,ij->i", nn, outward) > 0).all()                    # out of the fluid


def test_uncapped_slab_is_open_on_the_border_only():
    w, out, sm = _mesh("slab reaching the border", False)
    assert not sm.is_closed()
    be = sm.boundary_edges()
    assert be.shape[0] > 0
    # a boundary edge joins two vertices of cells in the outermost cell layer of the same border face
    cc = np.stack(np.unravel_index(out["cells"], tuple(k - 1 for k in w.shape)), axis=1)
    a, b = cc[be[:, 0]], cc[be[:, 1]]
    on_face = np.zeros(be.shape[0], dtype=bool)
    for ax in (0, 2):                                                        # the slab is flat in k1: it meets the k0 and k2 faces
        for end in (0, w.shape[ax] - 2):
            on_face |= (a[:, ax] == end) & (b[:, ax] == end)
    assert on_face.all()
    capped = _mesh("slab reaching the border", True)[2]
    assert capped.is_closed() and capped.triangles.shape[0] > sm.triangles.shape[0] - 1


def test_smallest_grids():
    one = np.zeros((2, 2, 2), dtype=np.int64)
    one[0, 0, 0] = FULL
    out = model.extract(one, ORIGIN, SPACING, ISO, False)
    assert out["vertices"].shape == (1, 3) and out["triangles"].shape == (0, 3)
    u = (out["vertices"][0].astype(np.float64) - np.asarray([float(F32(o)) for o in ORIGIN])) / np.asarray([float(F32(s)) for s in SPACING])
    assert np.allclose(u, 1.0 / 6.0, atol=1e-5)                              # three crossings at t = 1/2: the mean is (1/2, 0, 0) / 3 ... per axis 1/6
    assert model.extract(one, ORIGIN, SPACING, ISO, True)["vertices"].shape == (0, 3)
    three = np.zeros((3, 3, 3), dtype=np.int64)
    three[1, 1, 1] = FULL
    out = model.extract(three, ORIGIN, SPACING, ISO, True)
    assert out["vertices"].shape == (8, 3) and out["triangles"].shape == (12, 3)
    sm = mesh.SurfaceMesh(out["vertices"], out["normals"], out["triangles"], time=0, iso=ISO, origin=ORIGIN, spacing=SPACING, shape=(3, 3, 3))
    assert sm.is_closed() and sm.volume() > 0
    assert model.extract(np.zeros((4, 3, 5), dtype=np.int64), ORIGIN, SPACING, ISO, True)["vertices"].shape == (0, 3)
    assert model.extract(np.full((4, 3, 5), FULL, dtype=np.int64), ORIGIN, SPACING, ISO, False)["triangles"].shape == (0, 3)


# ---- SurfaceMesh ---------------------------------------------------------------------------------------------------------------
def read_ply(path):
    """A minimal reader of what `write_ply` writes: (vertices, normals, triangles, comments)."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    comments = [s[len("comment "):] for s in lines if s.startswith("comment ")]
    rest = [s for s in lines[2:] if not s.startswith("comment ")]
    V = int(rest[0].split()[2])
    assert rest[0].startswith("element vertex ") and rest[1:7] == [f"property float {p}" for p in ("x", "y", "z", "nx", "ny", "nz")]
    T = int(rest[7].split()[2])
    assert rest[7].startswith("element face ") and rest[8:] == ["property list uchar int vertex_indices"]
    rows = np.frombuffer(body[:V * 24], dtype="<f4").reshape(V, 6)
    faces = np.frombuffer(body[V * 24:], dtype=np.dtype([("k", "u1"), ("i", "<i4", 3)]))
    assert len(body) == V * 24 + T * 13 and faces.shape == (T,) and (faces["k"] == 3).all()
    return rows[:, :3], rows[:, 3:], faces["i"], comments


def test_write_ply_round_trip(tmp_path):
    w, out, sm = _mesh("two balls touching", True)
    path = tmp_path / "surface.ply"
    sm.write_ply(path, comments=("frame 3",))
    v, n, t, comments = read_ply(path)
    assert np.array_equal(v, sm.vertices) and np.array_equal(n, sm.normals) and np.array_equal(t, sm.triangles)
    assert "frame 3" in comments and "time 0.5" in comments
    empty = mesh.SurfaceMesh(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), time=0, iso=ISO, origin=ORIGIN, spacing=SPACING, shape=(2, 2, 2))
    empty.write_ply(path)
    v, n, t, _ = read_ply(path)
    assert v.shape == (0, 3) and t.shape == (0, 3) and empty.volume() == 0 and empty.area() == 0 and empty.is_closed()


def test_volume_area_of_a_tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=F32)
    t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)   # outward
    sm = mesh.SurfaceMesh(v, np.zeros((4, 3)), t, time=0, iso=ISO, origin=ORIGIN, spacing=SPACING, shape=(2, 2, 2))
    assert sm.is_closed() and abs(sm.volume() - 1 / 6) < 1e-15 and abs(sm.area() - (1.5 + np.sqrt(3) / 2)) < 1e-12
    flipped = mesh.SurfaceMesh(v, np.zeros((4, 3)), t[:, ::-1], time=0, iso=ISO, origin=ORIGIN, spacing=SPACING, shape=(2, 2, 2))
    assert flipped.is_closed() and flipped.volume() < 0
    torn = mesh.SurfaceMesh(v, np.zeros((4, 3)), t[:3], time=0, iso=ISO, origin=ORIGIN, spacing=SPACING, shape=(2, 2, 2))
    assert not torn.is_closed() and sorted(map(tuple, torn.boundary_edges().tolist())) == [(1, 3), (2, 1), (3, 2)]


# ---- arguments and the driver's key ------------------------------------------------------------------------------------------------
def test_argument_checks():
    assert mesh.mesh_args() == {"iso": float(F32(0.4)), "cap": True}
    assert mesh.mesh_args(4.0, False) == {"iso": 4.0, "cap": False}
    for bad in (0.0, -0.1, float("nan"), float("inf"), 4.5, 1e-50, "0.4", None, True):
        with pytest.raises(ValueError, match="iso"):
            mesh.mesh_args(bad)
    with pytest.raises(ValueError, match="cap"):
        mesh.mesh_args(0.4, 1)
    ga = mesh.grid_args(0.05, (0.1, 0.1, 0.1), (2, 7, 9), particle_diameter=0.02, domain_size=(1, 1, 1))
    assert ga["shape"] == (2, 7, 9)
    assert min(mesh.grid_args(particle_diameter=0.02, domain_size=(1.0, 1.2, 0.8))["shape"]) >= 2
    for shape in ((1, 7, 9), (4, 1, 4), (4, 4, 1)):
        with pytest.raises(ValueError, match="at least 2"):
            mesh.grid_args(0.05, None, shape, particle_diameter=0.02, domain_size=(1, 1, 1))
    with pytest.raises(ValueError, match="at least 1"):
        mesh.grid_args(0.05, None, (4, 0, 4), particle_diameter=0.02, domain_size=(1, 1, 1))


def _config(**keys):
    sd = scenes.fluid_only(counts=(3, 3, 3))
    sd["Configuration"].update(keys)
    return SimConfig(config=sd)


def test_driver_scene_key():
    assert mesh.mesh_config(_config()) is None
    assert mesh.mesh_config(_config(exportMesh={})) == {"spacing": None, "origin": None, "shape": None, "iso": 0.4, "cap": True, "objects": None}
    kw = mesh.mesh_config(_config(exportMesh={"spacing": 0.04, "origin": [0.1, 0.1, 0.1], "shape": [5, 5, 5], "iso": 0.3, "cap": False, "objects": [0]}))
    assert kw == {"spacing": 0.04, "origin": [0.1, 0.1, 0.1], "shape": [5, 5, 5], "iso": 0.3, "cap": False, "objects": [0]}
    for bad, msg in (({"spacing": -1}, "positive"), ({"cell": 0.1}, "unknown key"), ({"fields": ["velocity"]}, "unknown key"), ({"iso": 0}, "iso"),
                     ({"iso": "half"}, "iso"), ({"cap": "yes"}, "cap"), ({"shape": [1, 4, 4]}, "at least 2"), ({"shape": [4, 4]}, "three"),
                     ({"objects": []}, "empty")):
        with pytest.raises(ValueError, match=f'"exportMesh".*{msg}'):
            mesh.mesh_config(_config(exportMesh=bad))
    with pytest.raises(ValueError, match="must be an object"):
        mesh.mesh_config(_config(exportMesh=[1]))
