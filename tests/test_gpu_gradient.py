"""Sampled gradients on the device (include/sph_hip.h, "Field sampling: gradients"; csrc/sph_sample.hip) against the numpy model of
tests/gradient_model.py on the context's OWN downloaded x, v, m_V, density, pressure, material and object_id.

Every comparison of raw planes with the model is exact (array_equal on int64): the gradient term is a fixed sequence of f32
operations with a correctly rounded square root and division, the terms are llrint of exact f64 products, the sums are integers.
There is no tolerance anywhere in this file.  The model is brute force over (position, particle) pairs: it knows nothing of
footprints, lanes or LDS chunks.
"""
import copy
import ctypes as C
import json

import numpy as np
import pytest

from sph_taichi_amd import ParticleSystem, _lib, mesh, sample
from sph_taichi_amd.config_builder import SimConfig
from tests import gradient_model as gm
from tests import sample_model as model
from tests import scenes

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = ("velocity", "density", "pressure")
STATE = ("x", "v", "density", "pressure")
BASE = ("count", "weight", "sums")
RAW = BASE + ("grad_fill", "grad_sums")
CROWDED = (12, 8, 10)          # 1,920 particles at 16 per cell: eight blocks of the walk, and a model that stays quick


def _download(ps):
    return {f: getattr(ps, f).to_numpy() for f in ("x", "v", "m_V", "density", "pressure", "material", "object_id")}


def _want(ps, f, positions, fields, gradients, material, objects):
    sel = sample.select_args(fields=fields, material=material, objects=objects)
    gr = sample.gradient_args(gradients, sel["fields"])
    chosen = model.select(f["material"], f["object_id"], sel["material"], sel["objects"])
    return gm.sample(positions, f["x"], f["m_V"], model.values_of(sel["planes"], f["v"], f["density"], f["pressure"]),
                     gm.grad_indices(sel["planes"], gr["planes"]), chosen, model.inv_h(ps.support_radius), F32(ps._params.k_w))


def _same(got, want, tag, keys=RAW):
    for k in keys:
        g, w = getattr(got, k), want[k]
        assert g.dtype == w.dtype == np.int64, (tag, k)
        g = g.reshape(w.shape)
        assert np.array_equal(g, w), (tag, k, int((g != w).sum()), int(np.abs(g - w).max()))


def _bytes(s, keys=RAW):
    return b"".join(getattr(s, k).tobytes() for k in keys)


def _check_grid(ps, f, tag, fields=ALL, gradients=ALL, material="fluid", objects=None, **kw):
    """ps.sample_grid with gradients against the model on the fields `f`; the base planes against the plain call; returns the grid."""
    grid = ps.sample_grid(fields=fields, material=material, objects=objects, gradients=gradients, **kw)
    pos = model.node_positions(grid.origin, grid.spacing, grid.shape)
    _same(grid, _want(ps, f, pos, fields, gradients, material, objects), (tag, kw))
    plain = ps.sample_grid(fields=fields, material=material, objects=objects, **kw)
    assert plain.grad_fill is None and _bytes(plain, BASE) == _bytes(grid, BASE), (tag, "the base planes of a gradient call differ from the plain call")
    assert grid.grad_fill.shape == (3,) + grid.shape and grid.grad_sums.shape[:2] == (len(grid.grad_planes), 3) and grid.time == ps.time
    return grid


def _check_points(ps, points, f, tag, fields=ALL, gradients=ALL, material="fluid", objects=None):
    pr = ps.sample_points(points, fields=fields, material=material, objects=objects, gradients=gradients)
    _same(pr, _want(ps, f, pr.points, fields, gradients, material, objects), tag)
    return pr


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def test_mixed_scene_against_the_model():
    """Fluid + static block + dynamic block, before the first sort (creation order) and after step(7) (cell order; N ragged
    against 64 and 256): all five gradient bits, the velocity bit alone, the fill gradient alone; fluid, solid, any material and
    an object list."""
    ps, solver = scenes.make_ps(scenes.fluid_with_rigid_blocks())
    box = dict(origin=(0.02, 0.0, 0.02), shape=(20, 22, 18))
    small = dict(origin=(0.08, 0.04, 0.08), shape=(9, 12, 8))
    f = _download(ps)
    first = _check_grid(ps, f, "before the first sort", fields=("velocity",), gradients=("velocity",), **small)
    assert first.count.any() and first.grad_fill.any()
    solver.initialize()
    solver.step(7)
    n = ps.particle_max_num
    assert n % 64 != 0 and n % 256 != 0 and n > 256, n
    f = _download(ps)
    full = _check_grid(ps, f, "all five bits", **box)
    assert full.grad_planes == model.PLANES and full.gradients == ALL and full.grad_sums.shape == (5, 3) + full.shape
    assert full.count.max() > 20 and (full.count == 0).any() and all(full.grad_sums[k].any() for k in range(5))
    vel = _check_grid(ps, f, "the velocity bit alone, beside density and pressure sums", gradients=("velocity",), **small)
    assert vel.grad_planes == ("vx", "vy", "vz") and vel.planes == model.PLANES
    only = _check_grid(ps, f, "velocity alone", fields=("velocity",), gradients=("velocity",), **small)
    assert np.array_equal(only.grad_sums, vel.grad_sums) and np.array_equal(only.grad_fill, vel.grad_fill)
    fill = _check_grid(ps, f, "the fill gradient alone", fields=(), gradients=("fill",), **small)
    assert fill.grad_sums.shape == (0, 3) + fill.shape and np.array_equal(fill.grad_fill, vel.grad_fill)
    pgrad = _check_grid(ps, f, "pressure only: a bit that is not the first plane", fields=("density", "pressure"), gradients=("pressure",), **small)
    assert pgrad.grad_planes == ("pressure",)
    solid = _check_grid(ps, f, "solid", material="solid", **small)
    anym = _check_grid(ps, f, "material any", material=None, **small)
    assert solid.count.any() and (anym.count == solid.count + vel.count).all()
    objs = _check_grid(ps, f, "an object list, any material", material=None, objects=[2, 1], **small)
    assert np.array_equal(objs.grad_fill, solid.grad_fill) and objs.grad_fill.any()              # objects 1 and 2 are all the solids there are
    # the views: the normal on the fluid's upper face points up; the gradient views are finite exactly where something contributed
    has = full.weight != 0
    assert np.isfinite(full.velocity_gradient[has]).all() and np.isnan(full.vorticity[~has]).all() and np.isnan(full.pressure_gradient[~has]).all()
    assert np.isfinite(full.q_criterion[has]).all() and np.isfinite(full.divergence[has]).all() and np.isfinite(full.density_gradient[has]).all()
    ps.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_less_than_one_wave_and_the_exact_branches():
    """27 particles.  1 x 1 x 1, a slice, nothing in reach.  Then two particles are moved to coordinates made of a = f32(0.02)
    (inv_h is exactly 25): a node ON a particle (r == 0: counts, weighs, adds nothing to any gradient sum), a node at q == 0.5
    and a node at q == 1 (contributes, with D = -0)."""
    ps, solver = scenes.make_ps(scenes.fluid_only(counts=(3, 3, 3)))
    solver.initialize()
    f = _download(ps)
    centre = tuple(float(v) for v in f["x"].mean(axis=0))
    one = _check_grid(ps, f, "1 x 1 x 1", origin=centre, shape=(1, 1, 1))
    assert one.count.tolist() == [[[27]]]
    off = _check_grid(ps, f, "1 x 1 x 1 off the centre", origin=(centre[0] + 0.013, centre[1] - 0.007, centre[2] + 0.004), shape=(1, 1, 1))
    assert off.grad_fill.all()
    sl = _check_grid(ps, f, "a slice", origin=(centre[0], 0.0, 0.0), shape=(1, 16, 16))
    assert 0 < np.count_nonzero(sl.count) < 256
    out = _check_grid(ps, f, "outside the fluid", origin=(0.6, 0.7, 0.5), shape=(5, 4, 3))
    assert not out.count.any() and not out.grad_fill.any() and not out.grad_sums.any()
    assert float(model.inv_h(ps.support_radius)) == 25.0
    a = F32(0.02)
    x, v = f["x"].copy(), f["v"].copy()
    x[0], x[1] = (a, 0.5, 0.5), (F32(2) * a, 0.75, 0.5)
    v[0], v[1] = (1.5, -2.0, 0.25), (-0.5, 3.0, 1.0)
    ps.x.from_numpy(x)
    ps.v.from_numpy(v)
    f = _download(ps)
    assert np.array_equal(f["x"], x)
    q = lambda dx: F32(np.sqrt(F32(F32(dx) * F32(dx)))) * F32(25)
    assert q(F32(2) * a - a) == F32(0.5) and q(F32(4) * a - F32(2) * a) == F32(1) and F32(a + a) == F32(2) * a
    g0 = _check_grid(ps, f, "nodes at r == 0 and q == 0.5", fields=("velocity",), gradients=("velocity",), spacing=float(a),
                     origin=(float(a), 0.5, 0.5), shape=(2, 1, 1))
    assert g0.count.reshape(-1).tolist() == [1, 1] and g0.weight.all()
    assert not g0.grad_fill[:, 0].any() and not g0.grad_sums[:, :, 0].any() and g0.sums[:, 0].all()       # r == 0
    assert g0.grad_fill[0, 1, 0, 0] < 0 and not g0.grad_fill[1:, 1].any() and g0.grad_sums[:, 0, 1, 0, 0].all()   # q == 0.5, e = (1, 0, 0)
    g1 = _check_grid(ps, f, "nodes at r == 0 and q == 1", fields=("velocity",), gradients=("velocity",), spacing=float(F32(2) * a),
                     origin=(float(F32(2) * a), 0.75, 0.5), shape=(2, 1, 1))
    assert g1.count.reshape(-1).tolist() == [1, 1] and g1.weight.reshape(-1)[0] > 0 and g1.weight.reshape(-1)[1] == 0
    assert not g1.grad_fill.any() and not g1.grad_sums.any()
    pr = _check_points(ps, [x[0], [float(F32(2) * a), 0.5, 0.5], [float(F32(4) * a), 0.75, 0.5], x[1]], f, "the same as points")
    assert pr.count.tolist() == [1, 1, 1, 1] and not pr.grad_fill[:, [0, 2, 3]].any() and pr.grad_fill[0, 1] == g0.grad_fill[0, 1, 0, 0]
    ps.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_shapes_that_can_break_the_grid_kernel():
    """One state (16 particles per cell after 5 steps; 1,920 is no multiple of 256), several grids; see the tags."""
    ps, solver = scenes.make_ps(scenes.crowded_fluid(counts=CROWDED))
    solver.initialize()
    solver.step(5)
    f = _download(ps)
    assert f["x"].shape[0] % 256 != 0
    h = float(F32(ps.support_radius))
    lo, hi = f["x"].min(axis=0).astype(np.float64), f["x"].max(axis=0).astype(np.float64)
    mid = tuple(float(v) for v in (lo + hi) / 2)
    one = _check_grid(ps, f, "one node in the middle: every nearby particle hits one address on 25 planes", origin=mid, shape=(1, 1, 1))
    assert one.count[0, 0, 0] > 40
    eighth = float(F32(ps.support_radius) / F32(8))
    fine = _check_grid(ps, f, "spacing h / 8 over a box of 2 h: footprints of 17^3 nodes", gradients=("velocity",), spacing=eighth,
                       origin=tuple(m - h for m in mid), shape=(17, 17, 17))
    assert fine.count.min() > 30
    part = _check_grid(ps, f, "the middle of the block only: every footprint is clipped, on every side", origin=tuple(float(v) + 0.06 for v in lo), shape=(5, 3, 4))
    assert part.count.min() > 20
    j = int(np.argmin(np.abs(f["x"] - (lo + hi) / 2).sum(axis=1)))
    on = _check_grid(ps, f, "a node on a particle, among many others", origin=tuple(float(c) for c in f["x"][j]), shape=(1, 1, 1))
    assert on.count[0, 0, 0] > 40
    _check_grid(ps, f, "anisotropic spacing, a negative origin", fields=("velocity",), gradients=("velocity",),
                spacing=(0.04, 0.02, 0.03), origin=(-0.33, -0.17, -0.05), shape=(24, 14, 12))
    ps.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_points_across_the_chunk_boundary():
    """25 channels cut the points into chunks of 164: m = 1, 164, 165 (a chunk of one point behind a full one) and 1024 (seven
    chunks).  m = 513 without gradients beside them: the plain call still cuts at 512."""
    ps, solver = scenes.make_ps(scenes.crowded_fluid(counts=CROWDED))
    solver.initialize()
    solver.step(5)
    f = _download(ps)
    lo, hi = f["x"].min(axis=0).astype(np.float64), f["x"].max(axis=0).astype(np.float64)
    rng = np.random.default_rng(3)
    pts = rng.uniform(lo - 0.05, hi + 0.05, size=(1024, 3))
    pts[163], pts[164], pts[1023] = f["x"][5], f["x"][700], f["x"][1900]       # a particle's own position on both sides of the boundary
    full = None
    for m in (1, 164, 165, 1024):
        pr = _check_points(ps, pts[:m], f, f"m = {m}")
        assert pr.grad_fill.shape == (3, m) and pr.grad_sums.shape == (5, 3, m)
        full = pr
    assert full.count.any() and (full.count == 0).any() and full.grad_fill.any()
    for m in (164, 165):                                                        # the chunking does not show in the result
        pr = ps.sample_points(pts[:m], fields=ALL, gradients=ALL)
        for k in RAW:
            assert np.array_equal(getattr(pr, k), getattr(full, k)[..., :m]), (m, k)
    some = _check_points(ps, pts[:700], f, "twelve channels: chunks of 322", fields=("velocity", "density"), gradients=("density",))
    assert some.grad_planes == ("density",)
    fillonly = _check_points(ps, pts[:600], f, "five channels: the 512 cap", fields=(), gradients=("fill",))
    assert np.array_equal(fillonly.grad_fill, full.grad_fill[:, :600])
    plain = ps.sample_points(pts[:513], fields=ALL)
    want = _want(ps, f, plain.points, ALL, (), "fluid", None)
    _same(plain, want, "m = 513, plain", BASE)
    assert plain.grad_fill is None and _bytes(plain, BASE) == b"".join(getattr(full, k)[..., :513].tobytes() for k in BASE)
    # the nodes of a small grid passed as points: the two kernels give the same raw values
    grid = ps.sample_grid(fields=ALL, gradients=ALL, spacing=0.03, origin=tuple(float(c) - 0.05 for c in lo), shape=(9, 8, 10))
    pr = ps.sample_points(grid.positions.reshape(-1, 3), fields=ALL, gradients=ALL)
    for k in RAW:
        assert np.array_equal(getattr(pr, k), getattr(grid, k).reshape(getattr(pr, k).shape)), k
    ps.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def _grid(n=(4, 4, 4), origin=(0.1, 0.1, 0.1), spacing=(0.02, 0.02, 0.02), inv_h=25.0, fields=7, material=1, n_objects=0):
    g = _lib.SphSampleGrid()
    g.n = (C.c_int32 * 3)(*n)
    g.origin, g.spacing = (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing)
    g.inv_h, g.fields = inv_h, fields
    g.select.material, g.select.n_objects = material, n_objects
    return g


def test_state_and_refusals():
    sd = scenes.fluid_only(counts=(4, 4, 4))
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    assert float(F32(1) / F32(ps.support_radius)) == 25.0
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    gr = np.zeros((12, 64), dtype=np.int64)
    w, cnt = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.int64)
    gdown = lambda nodes, a=gr: ps._call("sph_sample_grid_gradients_download", ptr(a), nodes)
    pdown = lambda m, a=gr: ps._call("sph_sample_points_gradients_download", ptr(a), m)
    ggrid = lambda g, mask: ps._call("sph_sample_grid_gradients", C.byref(g), mask)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been sampled"):
        gdown(64)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been sampled"):
        pdown(1)
    ps._call("sph_sample_grid", C.byref(_grid()))                          # a plain sample carries no gradients
    with pytest.raises(_lib.SphError, match=r"rc=-4.*without gradients"):
        gdown(64)
    sel = _grid().select
    pts = np.array([[0.13, 0.13, 0.13], [0.5, 0.5, 0.5]], dtype=F32)
    ps._call("sph_sample_points", ptr(pts), 2, 7, C.byref(sel), 25.0)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*without gradients"):
        pdown(2)
    for mask, msg in ((32, "unknown bits"), (-1, "unknown bits"), (8, "not in fields"), (7 | 16, "not in fields")):
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*gradients.*{msg}"):
            ggrid(_grid(), mask)
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*gradients.*{msg}"):
            ps._call("sph_sample_points_gradients", ptr(pts), 2, 7, mask, C.byref(sel), 25.0)
    inf, nan = float("inf"), float("nan")
    for bad, msg in ((dict(n=(0, 4, 4)), "at least 1"), (dict(n=(1 << 12, 1 << 12, 2)), "SPH_SAMPLE_MAX_NODES"), (dict(origin=(nan, 0, 0)), "origin"),
                     (dict(spacing=(0.02, 0.0, 0.02)), "spacing"), (dict(spacing=(0.02, 0.0049, 0.02)), "eighth"), (dict(inv_h=0.0), "inv_h"),
                     (dict(inv_h=inf), "inv_h"), (dict(fields=32 | 7), "unknown bits"), (dict(material=256), "material"), (dict(n_objects=33), "n_objects")):
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*sph_sample_grid_gradients.*{msg}"):
            ggrid(_grid(**bad), 7)
    big = np.zeros((1025, 3), dtype=F32)
    for args, msg in (((pts, 0, 7, 7), "SPH_SAMPLE_MAX_POINTS"), ((big, 1025, 7, 7), "SPH_SAMPLE_MAX_POINTS"), ((np.array([[0, nan, 0]], dtype=F32), 1, 7, 7), "not finite"),
                      ((pts, 2, 64, 0), "unknown bits")):
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*sph_sample_points_gradients.*{msg}"):
            ps._call("sph_sample_points_gradients", ptr(args[0]), args[1], args[2], args[3], C.byref(sel), 25.0)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*without gradients"):
        gdown(64)                                                           # the refused calls changed nothing
    ggrid(_grid(), 7)
    for bad in (63, 65, 0):
        with pytest.raises(_lib.SphError, match=r"rc=-1.*nodes"):
            gdown(bad)
    gdown(64)
    ps._call("sph_sample_grid_download", ptr(w), ptr(cnt), None, 64)
    good = gr.copy()
    assert cnt.min() > 0 and gr[:3].any() and gr[3:].any()
    for bad_call in (lambda: ggrid(_grid(n=(8, 8, 0)), 7), lambda: ggrid(_grid(), 8), lambda: ps._call("sph_sample_grid", C.byref(_grid(n=(8, 8, 0))))):
        with pytest.raises(_lib.SphError, match=r"rc=-1"):
            bad_call()
    gr[:] = 0
    gdown(64)                                                               # after refused calls the last good result is still there
    assert np.array_equal(gr, good)
    ggrid(_grid(fields=0), 0)                                               # the fill gradient alone: three planes
    three = np.zeros((3, 64), dtype=np.int64)
    gdown(64, three)
    assert np.array_equal(three, good[:3])
    # a larger grid after a smaller one reallocates: 25 planes of 10 x 9 x 8 nodes behind 3 planes of 64
    larger = ps.sample_grid(fields=ALL, gradients=ALL, origin=(0.06, 0.06, 0.06), shape=(10, 9, 8))
    f = _download(ps)
    _same(larger, _want(ps, f, model.node_positions(larger.origin, larger.spacing, larger.shape), ALL, ALL, "fluid", None), "a larger grid")
    ggrid(_grid(), 7)                                                       # and a smaller one again, in the larger buffer
    gr[:] = 0
    gdown(64)
    assert np.array_equal(gr, good)
    # points
    ps._call("sph_sample_points_gradients", ptr(pts), 2, 7, 7, C.byref(sel), 25.0)
    pg = np.zeros((12, 2), dtype=np.int64)
    with pytest.raises(_lib.SphError, match=r"rc=-1.*took 2 points"):
        pdown(3, pg)
    with pytest.raises(_lib.SphError, match=r"rc=-1"):
        ps._call("sph_sample_points_gradients", ptr(big), 1025, 7, 7, C.byref(sel), 25.0)
    pdown(2, pg)
    assert pg[:, 0].any() and not pg[:, 1].any()
    ps._call("sph_sample_points_download", ptr(w), ptr(cnt), None, 2)
    assert cnt[0] > 0 and cnt[1] == 0
    ps.close()
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.sample_grid(gradients=("velocity",))
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.sample_points([[0.1, 0.1, 0.1]], gradients=("fill",))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*single-domain"):
        slab._call("sph_sample_grid_gradients", C.byref(_grid()), 7)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*single-domain"):
        slab._call("sph_sample_points_gradients", ptr(pts), 2, 7, 7, C.byref(sel), 25.0)
    slab.close()


def test_python_argument_errors():
    ps, solver = scenes.make_ps(scenes.fluid_only(counts=(3, 3, 3)))
    for bad, msg in ((dict(gradients="velocity"), "not one string"), (dict(gradients=("speed",)), "unknown gradient"),
                     (dict(gradients=("velocity", "velocity")), "twice"), (dict(gradients=("pressure",)), "name it in fields")):
        with pytest.raises(ValueError, match=msg):
            ps.sample_grid(**bad)
        with pytest.raises(ValueError, match=msg):
            ps.sample_points([[0.1, 0.1, 0.1]], **bad)
    plain = ps.sample_grid(gradients=())
    assert plain.grad_fill is None
    with pytest.raises(ValueError, match="was not sampled"):
        plain.vorticity
    g = ps.sample_grid(gradients=("fill",))
    assert g.grad_fill.any() and g.gradients == ()
    with pytest.raises(ValueError, match="gradient of vx was not sampled"):
        g.vorticity
    assert np.isfinite(g.fill_gradient[g.weight != 0]).all() and np.isnan(g.fill_gradient[g.weight == 0]).all()
    ps.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["uniform_fluid", "mixed"])
def test_read_only(scene):
    sd = scenes.fluid_only() if scene == "uniform_fluid" else scenes.fluid_with_rigid_blocks()
    a, solver_a = scenes.make_ps(sd)
    solver_a.initialize()
    solver_a.step(3)
    g = a.sample_grid(fields=ALL, gradients=ALL)
    p = a.sample_points([[0.2, 0.2, 0.2], [0.15, 0.3, 0.15]], fields=("pressure", "density"), gradients=("pressure", "density"), material=None)
    assert g.grad_sums.any() and p.grad_fill.any()
    solver_a.step(3)
    b, solver_b = scenes.make_ps(sd)
    solver_b.initialize()
    solver_b.step(6)
    for name in STATE:
        assert np.array_equal(scenes.ps_by_pid(a, name), scenes.ps_by_pid(b, name)), f"{name} differs after gradient sampling between the steps"
    assert a.time == b.time
    a.close(); b.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_mesh_reads_the_same_weight_plane():
    ps, solver = scenes.make_ps(scenes.fluid_only())
    solver.initialize()
    solver.step(3)
    geom = dict(origin=(0.04, 0.02, 0.04), shape=(16, 18, 14))
    ps.sample_grid(fields=ALL, **geom)
    plain = mesh.extract_raw(ps, 0.4, True)
    ps.sample_grid(fields=ALL, gradients=ALL, **geom)
    grad = mesh.extract_raw(ps, 0.4, True)                                   # cut from the weight plane of a gradient-carrying grid
    assert plain[0].shape[0] > 100 and plain[2].shape[0] > 100
    for a, b in zip(plain, grad):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    ps.sample_grid(fields=("velocity",), gradients=("velocity",), **geom)
    after = ps.surface_mesh(**geom)                                           # samples again (plain) behind a gradient-carrying grid
    assert np.array_equal(after.vertices, plain[0]) and np.array_equal(after.triangles, plain[2])
    ps.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_run_simulation_writes_the_gradient_fields(tmp_path, monkeypatch):
    """27 particles in free fall, timeStepSize 0.016 so that every frame is an output interval: 2 frames, 2 volumes, 2 lines."""
    from sph_taichi_amd import run_simulation
    sd = scenes.fluid_only(counts=(3, 3, 3), start=(0.3, 0.3, 0.3))
    sd["Configuration"]["timeStepSize"] = 0.016
    points = [[0.32, 0.32, 0.32], [0.9, 0.7, 0.5]]                           # in the block at the start, never wet
    grid_kw = dict(spacing=0.04, origin=(0.2, 0.1, 0.32), shape=(6, 8, 1), fields=("velocity", "pressure"), gradients=("velocity",))
    sd["Configuration"]["sampleGrid"] = {"spacing": 0.04, "origin": [0.2, 0.1, 0.32], "shape": [6, 8, 1], "fields": ["velocity", "pressure"],
                                         "gradients": ["velocity"]}
    sd["Configuration"]["probes"] = {"points": points, "fields": ["velocity", "density"], "gradients": ["density", "velocity"]}
    scene_file = tmp_path / "gradient_scene.json"
    scene_file.write_text(json.dumps(sd))
    out = tmp_path / "probes.jsonl"
    monkeypatch.chdir(tmp_path)
    run_simulation.main(["--scene_file", str(scene_file), "--frames", "2", "--probes", str(out)])
    lines = [json.loads(s) for s in out.read_text().splitlines()]
    assert [row["frame"] for row in lines] == [0, 1]
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    for k, row in enumerate(lines):
        solver.step(1)
        pr = ps.sample_points(points, fields=("velocity", "density"), gradients=("velocity", "density"))
        assert row["time"] == pr.time and row["probes"] == json.loads(json.dumps(pr.rows()))
        assert list(row["probes"][0])[5:] == ["fill_gradient", "vorticity", "divergence", "q_criterion", "density_gradient"]
        assert row["probes"][1]["vorticity"] == [None, None, None] and row["probes"][0]["vorticity"] == [float(c) for c in pr.vorticity[0]]
        grid = ps.sample_grid(**grid_kw)
        want = tmp_path / "want.vtk"
        grid.write_vtk(want)
        got = (tmp_path / "gradient_scene_output" / f"grid_{k:06}.vtk").read_bytes()
        assert got == want.read_bytes()
        for label in (b"VECTORS fill_gradient float\n", b"VECTORS vorticity float\n", b"SCALARS divergence float 1\n", b"SCALARS q_criterion float 1\n"):
            assert got.count(label) == 1
        assert b"pressure_gradient" not in got
        vort = np.frombuffer(got[got.index(b"VECTORS vorticity float\n") + 24:][:48 * 3 * 4], dtype=">f4").reshape(1, 8, 6, 3)
        assert np.array_equal(vort, np.transpose(grid.vorticity, (2, 1, 0, 3)).astype(F32), equal_nan=True) and np.isfinite(vort).any()
    ps.close()
