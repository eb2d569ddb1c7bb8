"""The surface mesh on the device (include/sph_hip.h, section "Surface mesh"; csrc/sph_mesh.hip) against the numpy model of
tests/mesh_model.py, run on the context's OWN downloaded weight plane (sph_sample_grid_download).

Counts and triangles are integers: array_equal.  Vertices are exact too: only + - x / in IEEE f64 and f32, nothing contracted,
in a fixed order -- a difference there is a bug, not a tolerance.  Normals may differ by ONE f32 ulp per component: they pass
through an f64 sqrt whose last bit may differ between the two sides, and a relative f64 error of a few 2^-52 moves the f32
rounding by one step at most.

Internal sizes the shapes straddle (csrc/sph_mesh.hip): a workgroup takes MTPB = 256 consecutive linear nodes, a wave 64; the scan
of the block counts takes MESH_SCAN_CHUNK = 1024 blocks per trip.  (7, 5, 9) = 315 nodes: two blocks, the second with 59 nodes
(less than a wave); (33, 17, 65) = 36,465 nodes: 143 blocks, rows of 65 that never line up with a wave; (65, 3, 2) = 390 nodes: one
cell layer along two axes; (96, 64, 48) = 294,912 nodes: 1,152 blocks, two trips of the scan with a carried total.
"""
import copy
import ctypes as C
import json

import numpy as np
import pytest

from sph_taichi_amd import _lib, mesh
from tests import mesh_model as model
from tests import scenes
from tests.test_mesh_host import read_ply

pytestmark = pytest.mark.gpu

F32 = np.float32
CROWDED = (12, 8, 10)          # 1,920 particles, 16 per cell: fill about 1.6 inside
ptr = lambda a: a.ctypes.data_as(C.c_void_p)


def _weight(ps, shape):
    nodes = int(np.prod(shape))
    w = np.empty(nodes, dtype=np.int64)
    ps._call("sph_sample_grid_download", ptr(w), None, None, nodes)
    return w.reshape(shape)


def _ordered(a):
    """f32 -> integers that ascend with the value, one step per ulp."""
    i = a.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _same(sm, want, tag):
    V, T = want["vertices"].shape[0], want["triangles"].shape[0]
    print(f"{tag}: V = {sm.vertices.shape[0]} (model {V}), T = {sm.triangles.shape[0]} (model {T})")
    assert sm.vertices.shape == (V, 3) and sm.normals.shape == (V, 3) and sm.triangles.shape == (T, 3), tag
    assert np.array_equal(sm.triangles, want["triangles"]), (tag, "triangles")
    assert not np.isnan(sm.vertices).any() and not np.isnan(sm.normals).any(), tag
    diff = sm.vertices != want["vertices"]
    assert not diff.any(), (tag, "vertices", int(diff.sum()), float(np.abs(sm.vertices - want["vertices"]).max()))
    ulps = np.abs(_ordered(sm.normals) - _ordered(want["normals"]))
    print(f"{tag}: normals differ by at most {int(ulps.max()) if ulps.size else 0} ulp in {int((ulps > 0).sum())} components")
    assert (ulps <= 1).all(), (tag, "normals", int(ulps.max()))


def _check(ps, tag, iso=0.4, cap=True, material="fluid", objects=None, **grid):
    """ps.surface_mesh against the model on the weight plane it was cut from; returns the mesh."""
    sm = ps.surface_mesh(iso=iso, cap=cap, material=material, objects=objects, **grid)
    want = model.extract(_weight(ps, sm.shape), sm.origin, sm.spacing, iso, cap)
    _same(sm, want, (tag, grid, iso, cap))
    assert sm.time == ps.time and sm.iso == float(F32(iso))
    return sm


def _bytes(sm):
    return sm.vertices.tobytes() + sm.normals.tobytes() + sm.triangles.tobytes()


@pytest.fixture(scope="module")
def crowded():
    ps, solver = scenes.make_ps(scenes.crowded_fluid(counts=CROWDED))
    solver.initialize()
    solver.step(5)
    yield ps
    ps.close()


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def test_mixed_scene_against_the_model():
    """Fluid + static block + dynamic block after step(7), the whole domain at spacing d."""
    ps, solver = scenes.make_ps(scenes.fluid_with_rigid_blocks())
    solver.initialize()
    solver.step(7)
    capped = _check(ps, "capped")
    assert capped.shape == tuple(int(np.ceil(ps.domain_size[a] / float(F32(ps.particle_diameter)))) + 1 for a in range(3))
    assert capped.vertices.shape[0] > 500 and capped.is_closed() and capped.volume() > 0      # closed: on the device result itself
    t = capped.triangles
    assert ((t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])).all()
    uncapped = _check(ps, "uncapped", cap=False)
    assert _bytes(uncapped) == _bytes(capped)                                  # the fluid is nowhere near the domain's border
    assert _bytes(_check(ps, "object 0", objects=[0])) == _bytes(capped)     # object 0 is all the fluid there is
    anym = _check(ps, "material any", material=None)
    assert anym.is_closed() and anym.volume() > capped.volume()               # the solids join the surface
    low = _check(ps, "iso 0.25", iso=0.25)
    high = _check(ps, "iso 0.6", iso=0.6)
    assert low.is_closed() and high.is_closed() and low.volume() > capped.volume() > high.volume() > 0
    ps.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_smallest_grids():
    """27 particles: the fill is 0.46 at their centre and about 0.05 three spacings away, so iso = 0.2 separates the two."""
    ps, solver = scenes.make_ps(scenes.fluid_only(counts=(3, 3, 3)))
    solver.initialize()
    centre = tuple(float(v) for v in ps.x.to_numpy().mean(axis=0))
    one = _check(ps, "2 x 2 x 2, node 0 at the centre", iso=0.2, cap=False, origin=centre, spacing=0.06, shape=(2, 2, 2))
    assert one.vertices.shape == (1, 3) and one.triangles.shape == (0, 3)     # one cell, one vertex
    none = _check(ps, "2 x 2 x 2 capped", iso=0.2, origin=centre, spacing=0.06, shape=(2, 2, 2))
    assert none.vertices.shape == (0, 3) and none.triangles.shape == (0, 3)   # all 8 nodes are border nodes
    eight = _check(ps, "3 x 3 x 3 capped", iso=0.2, origin=tuple(c - 0.06 for c in centre), spacing=0.06, shape=(3, 3, 3))
    assert eight.vertices.shape == (8, 3) and eight.triangles.shape == (12, 3) and eight.is_closed() and eight.volume() > 0
    for cap in (True, False):
        out = _check(ps, "outside the fluid", cap=cap, origin=(0.6, 0.7, 0.5), shape=(5, 4, 3))
        assert out.vertices.shape == (0, 3) and out.triangles.shape == (0, 3)   # and the downloads of size 0 succeeded
    ps.close()
    ps, solver = scenes.make_ps(scenes.fluid_only())                           # 10 x 12 x 8 particles from 0.1
    solver.initialize()
    inside = dict(origin=(0.15, 0.15, 0.14), shape=(4, 5, 3))
    full = _check(ps, "inside the fluid", cap=False, **inside)
    assert full.vertices.shape == (0, 3) and full.triangles.shape == (0, 3)
    box = _check(ps, "inside the fluid, capped", **inside)
    assert box.is_closed() and box.volume() > 0 and box.vertices.shape[0] == 3 * 4 * 2   # every cell touches the 2 x 3 x 1 inner nodes
    ps.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_shapes_that_break_tiling_and_the_scan(crowded):
    ps = crowded
    x = ps.x.to_numpy()
    lo, hi = x.min(axis=0).astype(np.float64), x.max(axis=0).astype(np.float64)
    mid = (lo + hi) / 2
    for cap in (True, False):
        a = _check(ps, "(7, 5, 9)", cap=cap, origin=tuple(float(v) - 0.03 for v in lo), shape=(7, 5, 9))
        b = _check(ps, "(33, 17, 65)", cap=cap, spacing=(0.0125, 0.02, 0.0125), origin=tuple(float(v) - 0.05 for v in lo), shape=(33, 17, 65))
        c = _check(ps, "(65, 3, 2)", cap=cap, spacing=0.0125, origin=(float(lo[0]) - 0.05, float(mid[1]) - 0.01, float(mid[2]) - 0.01), shape=(65, 3, 2))
        d = _check(ps, "(96, 64, 48)", cap=cap, spacing=0.0125, shape=(96, 64, 48))
        assert a.vertices.shape[0] > 0 and b.vertices.shape[0] > 1000 and d.vertices.shape[0] > 1000
        assert b.is_closed() and d.is_closed()                                # the fluid lies inside both grids
        assert a.is_closed() == cap                                           # the fluid leaves this one
        assert (c.vertices.shape[0] > 0) == (not cap)                         # capped: every node of a (65, 3, 2) grid is a border node
        assert c.triangles.shape[0] % 2 == 0 and (not cap or c.triangles.shape[0] == 0)   # (only edges along k2 at k1 = 1 have four cells round them)


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_buffers_and_state(crowded):
    ps = crowded
    x = ps.x.to_numpy()
    lo = x.min(axis=0).astype(np.float64)
    big = dict(spacing=0.02, origin=tuple(float(v) - 0.05 for v in lo), shape=(20, 14, 18))
    small = dict(origin=tuple(float(v) - 0.03 for v in lo), shape=(7, 5, 9))
    first = _check(ps, "large", **big)
    little = _check(ps, "then small", **small)
    larger = _check(ps, "then larger: regrow", spacing=(0.0125, 0.02, 0.0125), origin=tuple(float(v) - 0.05 for v in lo), shape=(33, 17, 65))
    assert little.vertices.shape[0] < first.vertices.shape[0] < larger.vertices.shape[0]
    again = _check(ps, "large again", **big)
    assert _bytes(again) == _bytes(first)
    # the same extract twice on one sampled grid
    twice = mesh.extract_raw(ps, float(F32(0.4)), True)
    assert b"".join(a.tobytes() for a in twice) == _bytes(again)
    # a refused extract leaves the mesh downloadable
    bad = _lib.SphMeshSpec()
    bad.iso, bad.cap = 0.0, 1
    for iso in (0.0, -1.0, float("nan"), float("inf"), 4.5):
        bad.iso = iso
        with pytest.raises(_lib.SphError, match=r"rc=-1.*iso"):
            ps._call("sph_mesh_extract", C.byref(bad))
    with pytest.raises(_lib.SphError, match=r"rc=-1.*NULL"):
        ps._call("sph_mesh_extract", None)
    nv, nt = C.c_int64(), C.c_int64()
    ps._call("sph_mesh_counts", C.byref(nv), C.byref(nt))
    V, T = again.vertices.shape[0], again.triangles.shape[0]
    assert (nv.value, nt.value) == (V, T)
    pos, nrm, tri = np.zeros((V, 3), F32), np.zeros((V, 3), F32), np.zeros((T, 3), np.int32)
    down = lambda v, t: ps._call("sph_mesh_download", ptr(pos), ptr(nrm), ptr(tri), v, t)
    down(V, T)
    assert pos.tobytes() + nrm.tobytes() + tri.tobytes() == _bytes(again)
    # a download with wrong sizes
    for v, t in ((V - 1, T), (V, T + 2), (0, 0)):
        with pytest.raises(_lib.SphError, match=r"rc=-1.*the last extract made"):
            down(v, t)
    # sph_sample_grid after the extract: another grid, even a slice, changes nothing of the mesh
    ps.sample_grid(fields=("velocity",), origin=(0.0, 0.0, float(lo[2]) + 0.05), shape=(40, 30, 1))
    pos[:] = 0; nrm[:] = 0; tri[:] = 0
    down(V, T)
    assert pos.tobytes() + nrm.tobytes() + tri.tobytes() == _bytes(again)
    ps._call("sph_mesh_download", None, None, ptr(tri), V, T)                 # any pointer may be NULL
    # ... but an extract on that slice is refused (n[a] < 2), and the mesh is still there
    ok = _lib.SphMeshSpec()
    ok.iso, ok.cap = 0.4, 1
    with pytest.raises(_lib.SphError, match=r"rc=-1.*at least 2"):
        ps._call("sph_mesh_extract", C.byref(ok))
    down(V, T)
    assert pos.tobytes() + nrm.tobytes() + tri.tobytes() == _bytes(again)
    with pytest.raises(ValueError, match="at least 2"):
        ps.surface_mesh(shape=(40, 30, 1))
    # a fresh context: nothing sampled, nothing extracted
    fresh, solver = scenes.make_ps(scenes.fluid_only(counts=(3, 3, 3)))
    solver.initialize()
    with pytest.raises(_lib.SphError, match=r"rc=-4.*no grid has been sampled"):
        fresh._call("sph_mesh_extract", C.byref(ok))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*no mesh has been extracted"):
        fresh._call("sph_mesh_counts", C.byref(nv), C.byref(nt))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*no mesh has been extracted"):
        fresh._call("sph_mesh_download", None, None, None, 0, 0)
    fresh.close()


def test_slab_rank_is_refused():
    from sph_taichi_amd import ParticleSystem
    from sph_taichi_amd.config_builder import SimConfig
    sd = scenes.fluid_only(counts=(4, 4, 4))
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.surface_mesh()
    ok = _lib.SphMeshSpec()
    ok.iso, ok.cap = 0.4, 1
    with pytest.raises(_lib.SphError, match=r"rc=-4.*single-domain"):
        slab._call("sph_mesh_extract", C.byref(ok))
    slab.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_read_only():
    sd = scenes.fluid_with_rigid_blocks()
    a, solver_a = scenes.make_ps(sd)
    solver_a.initialize()
    for k in range(10):
        solver_a.step(1)
        assert a.surface_mesh(cap=bool(k % 2)).vertices.shape[0] > 0
    b, solver_b = scenes.make_ps(sd)
    solver_b.initialize()
    solver_b.step(10)
    for name in ("x", "v", "density"):
        assert scenes.ps_by_pid(a, name).tobytes() == scenes.ps_by_pid(b, name).tobytes(), f"{name} differs after meshing between the steps"
    assert a.time == b.time
    a.close(); b.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_run_simulation_writes_meshes(tmp_path, monkeypatch):
    """27 particles in free fall, timeStepSize 0.016 so that every frame is an output interval: 2 frames, 2 meshes."""
    from sph_taichi_amd import run_simulation
    sd = scenes.fluid_only(counts=(3, 3, 3), start=(0.3, 0.3, 0.3))
    sd["Configuration"]["timeStepSize"] = 0.016
    spec = {"spacing": 0.02, "origin": [0.2, 0.1, 0.2], "shape": [12, 16, 12], "iso": 0.2, "cap": True, "objects": [0]}
    sd["Configuration"]["exportMesh"] = spec
    scene_file = tmp_path / "mesh_scene.json"
    scene_file.write_text(json.dumps(sd))
    monkeypatch.chdir(tmp_path)                                               # the meshes go to {scene}_output/ under the working directory
    run_simulation.main(["--scene_file", str(scene_file), "--frames", "2"])
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    for k in range(2):
        solver.step(1)
        sm = ps.surface_mesh(spacing=0.02, origin=(0.2, 0.1, 0.2), shape=(12, 16, 12), iso=0.2, objects=[0])
        v, n, t, comments = read_ply(tmp_path / "mesh_scene_output" / f"surface_{k:06}.ply")
        assert v.shape[0] > 0 and t.shape[0] > 0 and f"frame {k}" in comments
        assert np.array_equal(v, sm.vertices) and np.array_equal(n, sm.normals) and np.array_equal(t, sm.triangles)
    assert sorted(p.name for p in (tmp_path / "mesh_scene_output").iterdir()) == ["surface_000000.ply", "surface_000001.ply"]
    ps.close()
