"""Field sampling on the device (include/sph_hip.h, section "Field sampling"; csrc/sph_sample.hip) against the numpy model of
tests/sample_model.py on the context's OWN downloaded x, v, m_V, density, pressure, material and object_id.

Every comparison with the model is exact (array_equal on the raw i64 planes): the pair term is a fixed sequence of f32
operations with a correctly rounded square root, the terms are llrint of exact f64 products, the sums are integers -- nothing
rounds differently on the two sides, so there is no tolerance to choose.  The model is brute force over (position, particle)
pairs: a footprint that is too small on the device shows as a difference.
"""
import copy
import ctypes as C
import json

import numpy as np
import pytest

from sph_taichi_amd import ParticleSystem, _lib, sample
from sph_taichi_amd.config_builder import SimConfig
from tests import sample_model as model
from tests import scenes

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = ("velocity", "density", "pressure")
STATE = ("x", "v", "acceleration", "m_V", "m", "density", "pressure", "material", "color", "is_dynamic", "object_id", "grid_ids")
RAW = ("count", "weight", "sums")
CROWDED = (12, 8, 10)          # 1,920 particles at 16 per cell: eight blocks of the walk, and a model that stays quick


def _download(ps):
    return {f: getattr(ps, f).to_numpy() for f in ("x", "v", "m_V", "density", "pressure", "material", "object_id")}


def _want(ps, f, positions, fields, material, objects):
    sel = sample.select_args(fields=fields, material=material, objects=objects)
    chosen = model.select(f["material"], f["object_id"], sel["material"], sel["objects"])
    return model.sample(positions, f["x"], f["m_V"], model.values_of(sel["planes"], f["v"], f["density"], f["pressure"]), chosen,
                        model.inv_h(ps.support_radius), F32(ps._params.k_w))


def _same(got, want, tag):
    for k in RAW:
        g, w = getattr(got, k).reshape(want[k].shape), want[k]
        assert g.dtype == w.dtype == np.int64, (tag, k)
        assert np.array_equal(g, w), (tag, k, int((g != w).sum()), int(np.abs(g - w).max()))


def _check_grid(ps, f=None, tag="", fields=ALL, material="fluid", objects=None, **kw):
    """ps.sample_grid against the model on the fields as they are now; returns the grid."""
    grid = ps.sample_grid(fields=fields, material=material, objects=objects, **kw)
    f = f if f is not None else _download(ps)
    pos = model.node_positions(grid.origin, grid.spacing, grid.shape)
    _same(grid, _want(ps, f, pos, fields, material, objects), (tag, kw))
    assert grid.time == ps.time
    return grid


def _check_points(ps, points, f=None, tag="", fields=ALL, material="fluid", objects=None):
    pr = ps.sample_points(points, fields=fields, material=material, objects=objects)
    f = f if f is not None else _download(ps)
    _same(pr, _want(ps, f, pr.points, fields, material, objects), tag)
    return pr


def _bytes(s):
    return b"".join(getattr(s, k).tobytes() for k in RAW)


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def test_mixed_scene_against_the_model():
    """Fluid + static block + dynamic block after step(7): N ragged against 64 and 256; the whole domain at spacing d, all five
    planes; fluid only, each single object, and material any (the solids then contribute with their boundary volumes)."""
    ps, solver = scenes.make_ps(scenes.fluid_with_rigid_blocks())
    solver.initialize()
    solver.step(7)
    n = ps.particle_max_num
    assert n % 64 != 0 and n % 256 != 0 and n > 256, n
    f = _download(ps)
    fluid = _check_grid(ps, f, "fluid")
    assert fluid.shape == tuple(int(np.ceil(ps.domain_size[a] / float(F32(ps.particle_diameter)))) + 1 for a in range(3))
    assert fluid.planes == model.PLANES and fluid.count.max() > 20 and (fluid.count == 0).any()
    # the other selections over the part of the domain that holds the three objects (the model is brute force)
    box = dict(origin=(0.02, 0.0, 0.02), shape=(20, 22, 18))
    near = _check_grid(ps, f, "fluid, the objects' box", **box)
    assert _bytes(_check_grid(ps, f, "object 0", objects=[0], **box)) == _bytes(near)        # object 0 is all the fluid there is
    anym = _check_grid(ps, f, "material any", material=None, **box)
    assert (anym.count >= near.count).all() and anym.count.sum() > near.count.sum()
    for rigid in (1, 2):
        solid = _check_grid(ps, f, "a rigid object, any material", material=None, objects=[rigid], **box)
        assert solid.count.any() and (f["m_V"][f["object_id"] == rigid] != F32(ps.m_V0)).any()  # boundary volumes, not m_V0
        empty = _check_grid(ps, f, "a rigid object as fluid", objects=[rigid], **box)
        assert not empty.count.any() and not empty.weight.any() and not empty.sums.any()
    ps.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_less_than_one_wave():
    ps, solver = scenes.make_ps(scenes.fluid_only(counts=(3, 3, 3)))
    solver.initialize()
    f = _download(ps)
    centre = tuple(float(v) for v in f["x"].mean(axis=0))
    one = _check_grid(ps, f, "1 x 1 x 1", origin=centre, shape=(1, 1, 1))
    assert one.count.tolist() == [[[27]]]
    sl = _check_grid(ps, f, "a slice", origin=(centre[0], 0.0, 0.0), shape=(1, 16, 16))
    assert 0 < np.count_nonzero(sl.count) < 256
    out = _check_grid(ps, f, "outside the fluid", origin=(0.6, 0.7, 0.5), shape=(5, 4, 3))
    assert not out.count.any() and not out.weight.any() and not out.sums.any()
    ps.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_shapes_that_break_the_combining_stage():
    """One state (16 particles per cell after 5 steps), many grids; see the tags."""
    ps, solver = scenes.make_ps(scenes.crowded_fluid(counts=CROWDED))
    solver.initialize()
    solver.step(5)
    f = _download(ps)
    d, h = float(F32(ps.particle_diameter)), float(F32(ps.support_radius))
    lo, hi = f["x"].min(axis=0).astype(np.float64), f["x"].max(axis=0).astype(np.float64)
    mid = tuple(float(v) for v in (lo + hi) / 2)
    one = _check_grid(ps, f, "one node in the middle: every nearby particle hits one address", origin=mid, shape=(1, 1, 1))
    assert one.count[0, 0, 0] > 40                                              # about 67: twice the rest density inside h
    eighth = float(F32(ps.support_radius) / F32(8))
    fine = _check_grid(ps, f, "spacing h / 8 over a box of 2 h: footprints of 17^3 nodes", spacing=eighth,
                       origin=tuple(m - h for m in mid), shape=(17, 17, 17))
    assert fine.count.min() > 30
    with pytest.raises(_lib.SphError, match=r"rc=-1.*eighth of the support radius"):
        ps.sample_grid(spacing=float(np.nextafter(F32(eighth), F32(0))), origin=mid, shape=(2, 2, 2))
    with pytest.raises(_lib.SphError, match=r"rc=-1.*eighth of the support radius"):
        ps.sample_grid(spacing=(d, d, float(np.nextafter(F32(eighth), F32(0)))), origin=mid, shape=(2, 2, 1))    # a slice still gives a spacing
    coarse = _check_grid(ps, f, "spacing 3 h: most particles touch no node", spacing=3 * h)
    assert 0 < np.count_nonzero(coarse.count) < coarse.count.size
    part = _check_grid(ps, f, "the middle of the block only", origin=tuple(float(v) + 0.06 for v in lo), shape=(5, 3, 4))
    assert part.count.min() > 20                                                # fluid on every side of the grid
    _check_grid(ps, f, "a negative origin", spacing=2 * d, origin=(-0.33, -0.17, -0.05), shape=(24, 14, 12))
    _check_grid(ps, f, "anisotropic spacing", spacing=(d, 2 * d, d / 2), origin=tuple(float(v) - 0.05 for v in lo), shape=(16, 6, 24))
    for axis in range(3):
        shape = [16, 12, 14]
        shape[axis] = 1
        origin = [float(v) - 0.03 for v in lo]
        origin[axis] = mid[axis]
        sl = _check_grid(ps, f, f"a slice along axis {axis}", origin=tuple(origin), shape=tuple(shape))
        assert sl.count.any() and (sl.count == 0).any()
    ps.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_order_independence():
    """x, v and m_V permuted (not sorted) and uploaded: the grid equals the model, and two different permutations give the same
    bytes.  A few values are replaced: velocities of +-2^25 (clamp to +-2^24), -0.0, one NaN position (contributes nowhere),
    one NaN m_V (weight 0, but it counts).  A grid at spacing h / 8 over the whole block gives the same bytes in cell order and
    permuted."""
    ps, solver = scenes.make_ps(scenes.crowded_fluid(counts=CROWDED))
    solver.initialize()
    solver.step(5)
    x, v, m_V = ps.x.to_numpy(), ps.v.to_numpy(), ps.m_V.to_numpy()
    n = x.shape[0]
    v[3] = (2.0 ** 25, -2.0 ** 25, -0.0)
    v[n // 2] = (-0.0, 2.0 ** 25, 1.0)
    x[7] = (np.nan, x[7, 1], x[7, 2])
    m_V[n - 5] = np.nan
    near_nan_mv = x[n - 5].astype(np.float64)
    rng = np.random.default_rng(17)
    lo = np.nanmin(x, axis=0)
    eighth = float(F32(ps.support_radius) / F32(8))
    whole = dict(fields=("velocity",), spacing=eighth, origin=tuple(float(c) - 0.04 for c in lo), shape=(64, 48, 56))
    for field, a in (("x", x), ("v", v), ("m_V", m_V)):
        getattr(ps, field).from_numpy(a)                                     # the replaced values, still in cell order
    in_order = _bytes(ps.sample_grid(**whole))
    seen = []
    for k in range(2):
        perm = rng.permutation(n)
        ps.x.from_numpy(x[perm])
        ps.v.from_numpy(v[perm])
        ps.m_V.from_numpy(m_V[perm])
        f = _download(ps)
        assert np.array_equal(f["x"], x[perm], equal_nan=True) and np.array_equal(f["m_V"], m_V[perm], equal_nan=True)
        grid = _check_grid(ps, f, f"permutation {k}", fields=("velocity",), origin=tuple(float(c) - 0.04 for c in lo), shape=(18, 14, 16))
        again = ps.sample_grid(fields=("velocity",), origin=tuple(float(c) - 0.04 for c in lo), shape=(18, 14, 16))
        assert _bytes(grid) == _bytes(again), "two calls on one state differ"
        pr = _check_points(ps, [list(near_nan_mv), [0.2, 0.2, 0.2]], f, f"permutation {k}, points", fields=("velocity",))
        assert _bytes(ps.sample_grid(**whole)) == in_order, "the fine grid depends on the particle order"
        seen.append((_bytes(grid), _bytes(pr)))
    assert seen[0] == seen[1], "the result depends on the particle order"
    # the particle with the NaN volume counts at its own position, with weight 0: against the same state with that volume restored
    ps.m_V.from_numpy(np.where(np.isnan(m_V), F32(ps.m_V0), m_V)[perm])
    with_mv = ps.sample_points([list(near_nan_mv)], fields=())
    w_self = int(np.rint(float(F32(F32(ps.m_V0) * F32(ps._params.k_w))) * 2.0 ** 30))
    assert with_mv.count[0] == pr.count[0] and with_mv.weight[0] == pr.weight[0] + w_self
    ps.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_points():
    ps, solver = scenes.make_ps(scenes.crowded_fluid(counts=CROWDED))
    solver.initialize()
    solver.step(5)
    f = _download(ps)
    lo, hi = f["x"].min(axis=0).astype(np.float64), f["x"].max(axis=0).astype(np.float64)
    rng = np.random.default_rng(3)
    for m in (1, 65, 1024):
        pts = rng.uniform(lo - 0.1, hi + 0.1, size=(m, 3))
        pr = _check_points(ps, pts, f, f"m = {m}")
        assert pr.count.shape == (m,) and pr.sums.shape == (5, m)
    assert pr.count.any() and (pr.count == 0).any()
    j = int(np.argmin(np.abs(f["x"] - (lo + hi) / 2).sum(axis=1)))
    pts = np.array([f["x"][j], [0.9, 1.1, 0.7], f["x"][j], [0.9, 0.05, 0.7]], dtype=np.float64)
    pr = _check_points(ps, pts, f, "special points")
    assert pr.count[1] == pr.count[3] == 0 and pr.weight[1] == pr.weight[3] == 0 and not pr.sums[:, [1, 3]].any()    # outside the fluid
    assert np.isnan(pr.velocity[1]).all() and np.isnan(pr.pressure[3])
    assert pr.count[0] == pr.count[2] and pr.weight[0] == pr.weight[2] and np.array_equal(pr.sums[:, 0], pr.sums[:, 2])   # the same point twice
    # a point equal to a particle's position: q == 0, W == k_w for that pair
    only = ps.sample_points([f["x"][j]], fields=(), objects=None)
    rest = np.delete(np.arange(f["x"].shape[0]), j)
    others = model.sample(f["x"][j][None, :], f["x"][rest], f["m_V"][rest], [], np.ones(rest.size, bool), model.inv_h(ps.support_radius), F32(ps._params.k_w))
    assert only.weight[0] - others["weight"][0] == int(np.rint(float(F32(f["m_V"][j] * F32(ps._params.k_w))) * 2.0 ** 30))
    assert only.count[0] == others["count"][0] + 1
    # the nodes of a small grid passed as points: the two kernels give the same raw values
    grid = ps.sample_grid(fields=ALL, spacing=0.03, origin=tuple(float(c) - 0.05 for c in lo), shape=(9, 8, 10))
    pr = ps.sample_points(grid.positions.reshape(-1, 3), fields=ALL)
    assert np.array_equal(pr.points, grid.positions.reshape(-1, 3))
    for k in RAW:
        assert np.array_equal(getattr(pr, k), getattr(grid, k).reshape(getattr(pr, k).shape)), k
    assert grid.count.any() and (grid.count == 0).any()
    ps.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["uniform_fluid", "mixed"])
def test_read_only(scene):
    sd = scenes.fluid_only() if scene == "uniform_fluid" else scenes.fluid_with_rigid_blocks()
    a, solver_a = scenes.make_ps(sd)
    solver_a.initialize()
    solver_a.step(3)
    g = a.sample_grid(fields=ALL)
    p = a.sample_points([[0.2, 0.2, 0.2], [0.15, 0.3, 0.15]], fields=("pressure", "density"), material=None)
    assert g.count.any() and p.count.any()
    solver_a.step(3)
    b, solver_b = scenes.make_ps(sd)
    solver_b.initialize()
    solver_b.step(6)
    for name in STATE:
        assert np.array_equal(scenes.ps_by_pid(a, name), scenes.ps_by_pid(b, name)), f"{name} differs after sampling between the steps"
    assert a.time == b.time
    a.close(); b.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_derived_views():
    """Uniform v = (0, -1, 0) before any step: the interpolated velocity is that velocity within count / weight (each llrint
    errs by at most 1/2, in the numerator and in the denominator) wherever weight > 0, NaN elsewhere."""
    ps, solver = scenes.make_ps(scenes.fluid_only())
    grid = ps.sample_grid(origin=(0.0, 0.0, 0.0), shape=(20, 22, 18))
    has = grid.weight > 0
    assert has.any() and not has.all() and grid.fields == ("velocity",) and grid.time == 0.0
    bound = grid.count[has] / grid.weight[has]
    v = grid.velocity
    assert (np.abs(v[..., 1][has] + 1.0) <= bound).all() and (np.abs(v[..., 0][has]) <= bound).all() and (np.abs(v[..., 2][has]) <= bound).all()
    assert np.isnan(v[~has]).all()
    assert ((grid.fill >= 0) & (grid.fill <= 4 * grid.count)).all()
    assert 0.7 < grid.fill.max() < 0.81                                            # m_V0 = 0.8 d^3: a full rest neighbourhood sums to 0.8
    assert grid.wet().any() and np.array_equal(grid.wet(0.25), grid.fill >= 0.25)
    ps.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def _grid(n=(4, 4, 4), origin=(0.1, 0.1, 0.1), spacing=(0.02, 0.02, 0.02), inv_h=25.0, fields=7, material=1, n_objects=0):
    g = _lib.SphSampleGrid()
    g.n = (C.c_int32 * 3)(*n)
    g.origin, g.spacing = (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing)
    g.inv_h, g.fields = inv_h, fields
    g.select.material, g.select.n_objects = material, n_objects
    return g


def test_refusals():
    sd = scenes.fluid_only(counts=(4, 4, 4))
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    assert float(F32(1) / F32(ps.support_radius)) == 25.0
    w, cnt = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    down = lambda nodes: ps._call("sph_sample_grid_download", ptr(w), ptr(cnt), None, nodes)
    pdown = lambda m: ps._call("sph_sample_points_download", ptr(w), ptr(cnt), None, m)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been sampled"):
        down(64)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been sampled"):
        pdown(1)
    inf, nan = float("inf"), float("nan")
    bad_grids = ((dict(n=(0, 4, 4)), "at least 1"), (dict(n=(4, 4, -1)), "at least 1"), (dict(n=(1 << 12, 1 << 12, 2)), "SPH_SAMPLE_MAX_NODES"),
                 (dict(origin=(nan, 0, 0)), "origin"), (dict(origin=(0, inf, 0)), "origin"), (dict(spacing=(0.02, 0.0, 0.02)), "spacing"),
                 (dict(spacing=(0.02, 0.02, -0.02)), "spacing"), (dict(spacing=(nan, 0.02, 0.02)), "spacing"), (dict(spacing=(inf, 0.02, 0.02)), "spacing"),
                 (dict(spacing=(0.02, 0.0049, 0.02)), "eighth"), (dict(n=(1, 4, 4), spacing=(0.0049, 0.02, 0.02)), "eighth"),
                 (dict(inv_h=0.0), "inv_h"), (dict(inv_h=-25.0), "inv_h"), (dict(inv_h=nan), "inv_h"), (dict(inv_h=inf), "inv_h"),
                 (dict(inv_h=0.125), "eighth"), (dict(fields=32), "unknown bits"), (dict(fields=-1), "unknown bits"),
                 (dict(material=-2), "material"), (dict(material=256), "material"), (dict(n_objects=-1), "n_objects"), (dict(n_objects=33), "n_objects"))
    for bad, msg in bad_grids:
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*{msg}"):
            ps._call("sph_sample_grid", C.byref(_grid(**bad)))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been sampled"):
        down(64)                                                            # a refused call leaves nothing to download
    sel = _grid().select
    pts = np.array([[0.13, 0.13, 0.13], [0.5, 0.5, 0.5]], dtype=F32)
    call_points = lambda p, m, fields=7, s=sel, inv_h=25.0: ps._call("sph_sample_points", ptr(p), m, fields, C.byref(s), inv_h)
    big = np.zeros((1025, 3), dtype=F32)
    for args, msg in (((pts, 0), "SPH_SAMPLE_MAX_POINTS"), ((big, 1025), "SPH_SAMPLE_MAX_POINTS"), ((np.array([[0, nan, 0]], dtype=F32), 1), "not finite"),
                      ((np.array([[inf, 0, 0]], dtype=F32), 1), "not finite"), ((pts, 2, 64), "unknown bits"), ((pts, 2, 7, _grid(material=300).select), "material"),
                      ((pts, 2, 7, _grid(n_objects=40).select), "n_objects"), ((pts, 2, 7, sel, 0.0), "inv_h"), ((pts, 2, 7, sel, nan), "inv_h")):
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*{msg}"):
            call_points(*args)
    ps._call("sph_sample_grid", C.byref(_grid()))
    for bad in (63, 65, 0):
        with pytest.raises(_lib.SphError, match=r"rc=-1.*nodes"):
            down(bad)
    down(64)
    good = (w.copy(), cnt.copy())
    assert cnt.min() > 0 and w.min() > 0
    with pytest.raises(_lib.SphError, match=r"rc=-1"):
        ps._call("sph_sample_grid", C.byref(_grid(n=(8, 8, 0))))
    w[:] = 0; cnt[:] = 0
    down(64)                                                                # after a failed call the last good result is still there
    assert np.array_equal(w, good[0]) and np.array_equal(cnt, good[1])
    call_points(pts, 2)
    with pytest.raises(_lib.SphError, match=r"rc=-1.*took 2 points"):
        pdown(3)
    with pytest.raises(_lib.SphError, match=r"rc=-1"):
        call_points(big, 1025)
    pdown(2)
    assert cnt[0] > 0 and cnt[1] == 0 and w[0] > 0 and w[1] == 0
    ps.close()
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.sample_grid()
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.sample_points([[0.1, 0.1, 0.1]])
    with pytest.raises(_lib.SphError, match=r"rc=-4.*single-domain"):
        slab._call("sph_sample_grid", C.byref(_grid()))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*single-domain"):
        slab._call("sph_sample_points", ptr(pts), 2, 7, C.byref(sel), 25.0)
    slab.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_run_simulation_grids_and_probes(tmp_path, monkeypatch):
    """27 particles in free fall, timeStepSize 0.016 so that every frame is an output interval (the lattice at rest spacing
    exerts no pressure, so the large step is harmless): 3 frames, 3 volumes, 3 lines."""
    from sph_taichi_amd import run_simulation
    sd = scenes.fluid_only(counts=(3, 3, 3), start=(0.3, 0.3, 0.3))
    sd["Configuration"]["timeStepSize"] = 0.016
    points = [[0.32, 0.32, 0.32], [0.9, 0.7, 0.5]]                           # in the block at the start, never wet
    grid_spec = {"spacing": 0.04, "origin": [0.2, 0.1, 0.32], "shape": [6, 8, 1], "fields": ["velocity", "pressure"], "objects": [0]}
    sd["Configuration"]["sampleGrid"] = grid_spec
    sd["Configuration"]["probes"] = {"points": points, "fields": ["velocity", "density"]}
    scene_file = tmp_path / "sample_scene.json"
    scene_file.write_text(json.dumps(sd))
    out = tmp_path / "probes.jsonl"
    monkeypatch.chdir(tmp_path)                                               # the volumes go to {scene}_output/ under the working directory
    run_simulation.main(["--scene_file", str(scene_file), "--frames", "3", "--probes", str(out)])
    lines = [json.loads(s) for s in out.read_text().splitlines()]
    assert [row["frame"] for row in lines] == [0, 1, 2]
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    for k, row in enumerate(lines):
        solver.step(1)
        pr = ps.sample_points(points, fields=("velocity", "density"))
        assert row["time"] == pr.time and row["probes"] == json.loads(json.dumps(pr.rows()))
        assert row["probes"][1]["count"] == 0 and row["probes"][1]["velocity"] == [None, None, None]
        grid = ps.sample_grid(spacing=0.04, origin=(0.2, 0.1, 0.32), shape=(6, 8, 1), fields=("velocity", "pressure"), objects=[0])
        want = tmp_path / "want.vtk"
        grid.write_vtk(want)
        got = tmp_path / "sample_scene_output" / f"grid_{k:06}.vtk"
        assert got.read_bytes() == want.read_bytes() and b"DIMENSIONS 6 8 1" in got.read_bytes()[:200]
    assert lines[0]["probes"][0]["count"] > 0 and lines[0]["probes"][0]["velocity"][1] < 0
    assert sorted(p.name for p in (tmp_path / "sample_scene_output").iterdir()) == ["grid_000000.vtk", "grid_000001.vtk", "grid_000002.vtk"]
    ps.close()
