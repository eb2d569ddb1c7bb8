"""Passive tracers on the device (include/sph_hip.h, section "Passive tracers"; csrc/sph_tracers.hip) against the numpy model of
tests/tracer_model.py evaluated on the context's OWN state downloaded before the step.

Every comparison with the model is exact (array_equal on the downloaded arrays): the pair term is a fixed sequence of f32
operations with a correctly rounded square root, the terms are llrint of exact f64 products, the sums are integers, the mean is
one f64 division rounded to f32, the advance one f32 multiply and one f32 add -- nothing rounds differently on the two sides.  The
sort of the step only permutes the records, and integer sums do not depend on their order, so the pre-step download in whatever
order serves.  The only tolerance in this file is the derived bound of the last test.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from sph_taichi_amd import ParticleSystem, _lib
from sph_taichi_amd.config_builder import SimConfig
from tests import scenes
from tests import tracer_model as model

pytestmark = pytest.mark.gpu

F32 = np.float32
KEYS = ("x", "u", "weight", "count", "wet_steps", "dry_steps")
DTYPES = {"x": np.float32, "u": np.float32, "weight": np.int64, "count": np.int32, "wet_steps": np.int32, "dry_steps": np.int32}
CROWDED = (12, 8, 10)          # 1,920 particles at 16 per cell


def _particles(ps):
    return {f: getattr(ps, f).to_numpy() for f in ("x", "v", "m_V", "material", "object_id")}


def _model(ps, state, f, min_fill=0.2, material=1, objects=()):
    return model.advance(state, f["x"], f["v"], f["m_V"], f["material"], f["object_id"],
                         model.params_of(ps, min_fill=min_fill, material=material, objects=objects))


def _same(got, want, tag=""):
    for k in KEYS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype == DTYPES[k], (tag, k, g.dtype, w.dtype)
        assert g.shape == w.shape and np.array_equal(g, w), (tag, k, int((g != w).sum()))


def _bytes(state):
    return b"".join(np.ascontiguousarray(state[k]).tobytes() for k in KEYS)


def _mixed_points(ps, f, m=203, seed=5):
    """On fluid particles; on exact multiples of the cell size; at padding and wall_hi; in the air; inside the static block; in the
    first and last reachable cell layers; the rest anywhere about the fluid."""
    rng = np.random.default_rng(seed)
    gs, pad = F32(ps._params.grid_size), F32(ps._params.padding)
    whi = np.array([ps._params.wall_hi[a] for a in range(3)], dtype=F32)
    fluid = f["x"][f["material"] == 1]
    lo, hi = fluid.min(axis=0), fluid.max(axis=0)
    on_particles = fluid[rng.choice(fluid.shape[0], 60, replace=False)]
    k = np.stack(np.meshgrid(np.arange(3, 7), np.arange(3, 7), np.arange(3, 6), indexing="ij"), axis=-1).reshape(-1, 3)
    on_cells = (k.astype(F32) * gs).astype(F32)                                       # 48 cell corners in and about the fluid
    corners = np.array([[(pad, whi[0])[i], (pad, whi[1])[j], (pad, whi[2])[l]] for i in (0, 1) for j in (0, 1) for l in (0, 1)], dtype=F32)
    air = rng.uniform([0.1, 0.8, 0.1], [0.9, 1.1, 0.7], size=(20, 3)).astype(F32)
    block = rng.uniform([0.1, 0.065, 0.1], [0.34, 0.095, 0.3], size=(20, 3)).astype(F32)
    layers = rng.uniform(0.0, 1.0, size=(20, 3)).astype(F32) * (whi - pad) + pad
    layers[:10, 0] = pad + rng.uniform(0, 0.03, 10).astype(F32)                     # the first reachable layer of x ...
    layers[10:, 0] = np.minimum(whi[0], whi[0] - rng.uniform(0, 0.03, 10).astype(F32))   # ... and the last, whose +x neighbours do not exist
    layers[5:15, 2] = np.minimum(whi[2], whi[2] - rng.uniform(0, 0.03, 10).astype(F32))
    rest = rng.uniform(lo - 0.03, hi + 0.03, size=(m - 60 - 48 - 8 - 60, 3)).astype(F32)
    pts = np.concatenate([on_particles, on_cells, corners, air, block, layers, rest]).astype(F32)
    assert pts.shape == (m, 3)
    return np.minimum(np.maximum(pts, pad), whi)


def _mixed(steps=7, dfsph=False):
    sd = scenes.fluid_with_rigid_blocks()
    ps, solver = scenes.make_ps(scenes.as_dfsph(sd) if dfsph else sd)
    solver.initialize()
    if steps:
        solver.step(steps)
    return ps, solver


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def test_one_step_against_the_model():
    ps, solver = _mixed()
    f = _particles(ps)
    pts = _mixed_points(ps, f)
    assert pts.shape[0] == 203 and pts.shape[0] % 4 and pts.shape[0] % 16 and pts.shape[0] % 64
    tr = ps.set_tracers(pts)
    assert tr is ps.tracers and tr.info().m == 203 and tr.info().advances == 0
    first = tr.state()
    assert np.array_equal(first["x"], pts) and not first["u"].any() and not first["weight"].any() and not first["wet_steps"].any()
    solver.step(1)
    got = tr.state()
    want = _model(ps, model.fresh(pts), f)
    _same(got, want, "mixed")
    assert tr.info().advances == 1
    wet = got["wet_steps"] == 1
    assert 50 < wet.sum() < 190 and (got["dry_steps"] == 1).sum() == 203 - wet.sum()          # some wet, some dry
    assert (got["count"] > 20).sum() > 40 and (got["count"] == 0).sum() >= 20                # whole neighbourhoods, and the air
    assert np.array_equal(got["x"][~wet], pts[~wet]) and (got["x"][wet] != pts[wet]).any()
    # the single accessors agree with the whole state
    assert np.array_equal(tr.positions(), got["x"]) and np.array_equal(tr.velocities(), got["u"]) and np.array_equal(tr.weight(), got["weight"])
    assert np.array_equal(tr.wet_steps(), got["wet_steps"]) and np.array_equal(tr.dry_steps(), got["dry_steps"]) and np.array_equal(tr.count(), got["count"])
    ps.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_many_steps_chained_model_and_history():
    a, sa = _mixed()
    b, sb = _mixed()
    pts = _mixed_points(a, _particles(a), seed=6)
    ta = a.set_tracers(pts)
    tb = b.set_tracers(pts, record_every=1, record_capacity=5)
    want, frames = model.fresh(pts), []
    for k in range(5):
        want = _model(a, want, _particles(a))
        sa.step(1)
        _same(ta.state(), want, k)
        frames.append(want["x"])
    sb.step(5)
    assert _bytes(tb.state()) == _bytes(ta.state())
    paths = tb.paths()
    assert paths.dtype == np.float32 and paths.shape == (5, 203, 3) and np.array_equal(paths, np.stack(frames))
    i = tb.info()
    assert (i.advances, i.frames, i.dropped) == (5, 5, 0)
    a.close(); b.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_observer_only():
    a, sa = _mixed(steps=0)
    b, sb = _mixed(steps=0)
    b.set_tracers(_mixed_points(b, _particles(b)), record_every=2, record_capacity=10)
    for _ in range(4):
        sa.step(5); sb.step(5)
    for name in ("x", "v", "density", "pressure", "acceleration"):
        assert getattr(a, name).to_numpy().tobytes() == getattr(b, name).to_numpy().tobytes(), name
    for opt in (_lib.OPT_SORT_FAST_COUNT, _lib.OPT_SORT_GENERAL_COUNT):
        assert a.get_option(opt) == b.get_option(opt), opt
    assert a.get_option(_lib.OPT_SORT_FAST_COUNT) > 0 and b.tracers.info().advances == 20
    a.close(); b.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_crowded_cells():
    """16 particles per cell: a run of three cells holds about 48 records, three trips of the 16 lanes with ragged tails."""
    ps, solver = scenes.make_ps(scenes.crowded_fluid(counts=CROWDED))
    solver.initialize()
    solver.step(2)
    f = _particles(ps)
    rng = np.random.default_rng(8)
    lo, hi = f["x"].min(axis=0), f["x"].max(axis=0)
    pts = np.concatenate([f["x"][rng.choice(f["x"].shape[0], 30, replace=False)],
                          rng.uniform(lo - 0.03, hi + 0.03, size=(37, 3)).astype(F32)]).astype(F32)
    occupancy = np.bincount(np.ravel_multi_index(model.particle_cells(f["x"], ps._params.grid_size, model.params_of(ps)["grid_num"]).T,
                                                 model.params_of(ps)["grid_num"]))
    assert occupancy.max() >= 16
    tr = ps.set_tracers(pts)
    solver.step(1)
    got = tr.state()
    _same(got, _model(ps, model.fresh(pts), f), "crowded")
    assert got["count"].max() > 48 and (got["wet_steps"] == 1).sum() >= 30
    ps.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_selection():
    """Three contexts in the same state, one per material selection (their counts must add up), then the object lists on one of
    them in later steps."""
    counts, keep = {}, None
    for tag, material, mm in (("fluid", "fluid", 1), ("solid", "solid", 0), ("any", None, -1)):
        ps, solver = _mixed()
        f = _particles(ps)
        pts = _mixed_points(ps, f, seed=9)
        pts[-8:] = f["x"][f["object_id"] == 2][:8]          # some on the dynamic block, which hangs above the fluid
        tr = ps.set_tracers(pts, material=material)
        solver.step(1)
        got = tr.state()
        _same(got, _model(ps, model.fresh(pts), f, material=mm), tag)
        counts[tag] = got["count"]
        if tag == "any":
            keep = (ps, solver, pts)
        else:
            ps.close()
    assert counts["solid"].any() and counts["fluid"].any() and np.array_equal(counts["fluid"] + counts["solid"], counts["any"])
    ps, solver, pts = keep
    for tag, objects in (("static block", [1]), ("fluid and dynamic block", [0, 2]), ("dynamic block", 2)):
        f = _particles(ps)
        tr = ps.set_tracers(pts, material=None, objects=objects)
        solver.step(1)
        got = tr.state()
        _same(got, _model(ps, model.fresh(pts), f, material=-1, objects=tuple(np.atleast_1d(objects))), tag)
        assert got["count"].any(), tag
    ps.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_walls():
    ps, solver = scenes.make_ps(scenes.fluid_only(counts=(10, 12, 8), start=(0.76, 0.1, 0.1)))
    solver.initialize()
    v = ps.v.to_numpy()
    v[:] = (50.0, 0.0, 0.0)
    ps.v.from_numpy(v)
    f = _particles(ps)
    whi = F32(ps._params.wall_hi[0])
    near = f["x"][f["x"][:, 0] > 0.93][:21].copy()
    near[:, 0] = F32(0.95)
    tr = ps.set_tracers(near)
    solver.step(1)
    got = tr.state()
    _same(got, _model(ps, model.fresh(near), f), "walls")
    assert (got["wet_steps"] == 1).all() and (got["x"][:, 0] == whi).all() and np.array_equal(got["x"][:, 1:], near[:, 1:])
    ps.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_history_bookkeeping():
    a, sa = _mixed()
    b, sb = _mixed()
    pts = _mixed_points(a, _particles(a), seed=11)
    ta = a.set_tracers(pts, record_every=3, record_capacity=4)
    tb = b.set_tracers(pts)
    t0, dt = a.time, float(F32(sa.dt[None]))
    sa.step(20)
    i = ta.info()
    assert (i.m, i.advances, i.frames, i.dropped) == (203, 20, 4, 2)
    twin, t, times = [], t0, []
    for k in range(4):
        sb.step(3)
        twin.append(tb.positions())
        for _ in range(3):
            t += dt
        times.append(t)
    assert np.array_equal(ta.paths(), np.stack(twin))
    assert ta.times == times and tb.times == [] and len(ta.times) == 4
    with pytest.raises(_lib.SphError, match=r"rc=-1"):
        a._call("sph_tracers_history_download", None, 3, 203)
    a.close(); b.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_dfsph():
    ps, solver = _mixed(steps=2, dfsph=True)
    pts = _mixed_points(ps, _particles(ps), seed=12)
    tr = ps.set_tracers(pts)
    want = model.fresh(pts)
    for k in range(2):
        want = _model(ps, want, _particles(ps))
        solver.step(1)
        _same(tr.state(), want, k)
    assert tr.info().advances == 2 and (want["wet_steps"] == 2).sum() > 50
    ps.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_order_independence_replace_and_clear():
    a, sa = _mixed()
    b, sb = _mixed()
    pts = _mixed_points(a, _particles(a), seed=13)
    perm = np.random.default_rng(14).permutation(pts.shape[0])
    ta, tb = a.set_tracers(pts), b.set_tracers(pts[perm])
    sa.step(3); sb.step(3)
    sa_, sb_ = ta.state(), tb.state()
    for k in KEYS:
        assert np.array_equal(sa_[k][perm], sb_[k]), k
    # replacing the set zeroes its counters
    tb2 = b.set_tracers(pts[:50], record_every=1, record_capacity=2)
    s = tb2.state()
    assert tb2.info().advances == 0 and tb2.info().m == 50 and not s["wet_steps"].any() and not s["dry_steps"].any() and not s["weight"].any()
    sb.step(1)
    assert tb2.info().advances == 1 and tb2.info().frames == 1
    # clearing it: the steps advance nothing
    b.clear_tracers()
    before = b.tracers.info()
    sb.step(2)
    after = b.tracers.info()
    assert (before.m, before.advances) == (0, 0) == (after.m, after.advances) and after.frames == 0
    assert b.tracers.positions().shape == (0, 3)
    a.close(); b.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    sd = scenes.fluid_with_rigid_blocks()
    fresh, _ = scenes.make_ps(sd)
    buf = np.zeros((4, 3), np.float32)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_tracers_set first"):
        fresh._call("sph_tracers_download", buf.ctypes.data_as(C.c_void_p), None, None, None, None, None, 4)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_tracers_set first"):
        fresh._call("sph_tracers_history_download", None, 0, 4)
    assert fresh.tracers is None
    fresh.close()

    ps, solver = _mixed()
    pts = _mixed_points(ps, _particles(ps), seed=15)
    tr = ps.set_tracers(pts, record_every=1, record_capacity=3)
    solver.step(2)
    good = _bytes(tr.state())
    params = _lib.SphTracerParams()
    params.min_fill, params.select.material = 0.2, 1
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(rc, *args, p=params):
        with pytest.raises(_lib.SphError, match=rf"rc={rc}"):
            ps._call("sph_tracers_set", *args, C.byref(p))
        assert ps.tracers is tr and _bytes(tr.state()) == good and tr.info().advances == 2 and tr.info().frames == 2

    refused(-1, ptr(pts), _lib.TRACERS_MAX + 1)                       # m too large (checked before a single point is read)
    refused(-1, ptr(pts), -1)
    bad = pts.copy(); bad[7, 1] = np.nan
    refused(-1, ptr(bad), 203)
    bad = pts.copy(); bad[200, 0] = np.inf
    refused(-1, ptr(bad), 203)
    bad = pts.copy(); bad[5, 2] = np.nextafter(F32(ps._params.padding), F32(0))      # one ulp outside the domain
    refused(-1, ptr(bad), 203)
    bad = pts.copy(); bad[5, 0] = np.nextafter(F32(ps._params.wall_hi[0]), F32(2))
    refused(-1, ptr(bad), 203)
    for mf in (0.0, -0.2, 4.5, float("nan"), float("inf")):
        p = _lib.SphTracerParams(); p.min_fill, p.select.material = mf, 1
        refused(-1, ptr(pts), 203, p=p)
    for every, cap in ((-1, 0), (0, -1), (1, (1 << 31) // (12 * 203) + 1)):
        p = _lib.SphTracerParams(); p.min_fill, p.record_every, p.record_capacity, p.select.material = 0.2, every, cap, 1
        refused(-1, ptr(pts), 203, p=p)
    p = _lib.SphTracerParams(); p.min_fill, p.select.material = 0.2, 256
    refused(-1, ptr(pts), 203, p=p)
    p = _lib.SphTracerParams(); p.min_fill, p.select.material, p.select.n_objects = 0.2, 1, 33
    refused(-1, ptr(pts), 203, p=p)
    with pytest.raises(ValueError):
        ps.set_tracers(pts, min_fill=0.0)
    with pytest.raises(ValueError):
        ps.set_tracers(np.full((3, 3), np.nan))
    with pytest.raises(_lib.SphError, match=r"rc=-1.*outside"):
        ps.set_tracers([[0.5, 0.5, 5.0]])
    assert ps.tracers is tr
    out = np.zeros((300, 3), np.float32)
    for m in (202, 204, 0):
        with pytest.raises(_lib.SphError, match=r"rc=-1.*holds 203"):
            ps._call("sph_tracers_download", ptr(out), None, None, None, None, None, m)
    with pytest.raises(_lib.SphError, match=r"rc=-1"):
        ps._call("sph_tracers_history_download", ptr(out), 1, 203)
    assert _bytes(tr.state()) == good
    solver.step(1)                      # ... and the last good set goes on being advanced
    assert tr.info().advances == 3 and tr.info().frames == 3 and _bytes(tr.state()) != good
    ps.close()

    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=4096))
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.set_tracers(pts)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*single-domain"):
        slab._call("sph_tracers_set", ptr(pts), 203, C.byref(params))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*single-domain"):
        slab._call("sph_tracers_download", ptr(out), None, None, None, None, None, 203)
    slab.close()


# ---- 11 -----------------------------------------------------------------------------------------------------------------
def test_uniform_flow_within_the_derived_bound():
    """A block in uniform motion V without gravity; tracers on interior particles.  Every particle carries V, so the mean is V up
    to the llrints: each of at most 2^9 terms rounds by at most half a unit of 2^-30 in the weight and in the sum, and the weight is
    at least min_fill * 2^30, so |u - V| <= 2^9 (1 + |V|) / (0.2 * 2^30) per component."""
    V = np.array([0.75, -1.25, 0.4], dtype=F32)
    sd = scenes.fluid_only(counts=(10, 12, 8), start=(0.3, 0.3, 0.3), velocity=tuple(float(c) for c in V))
    sd["Configuration"]["gravitation"] = [0.0, 0.0, 0.0]
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    x = ps.x.to_numpy()
    lo, hi = x.min(axis=0), x.max(axis=0)
    interior = x[((x > lo + 0.05) & (x < hi - 0.05)).all(axis=1)]
    assert interior.shape[0] >= 40
    tr = ps.set_tracers(interior)
    solver.step(1)
    got = tr.state()
    assert (got["wet_steps"] == 1).all() and (got["count"] >= 27).all() and (got["count"] <= 512).all()
    bound = 2.0 ** 9 * (1.0 + np.abs(V).astype(np.float64)) / (0.2 * 2.0 ** 30)
    err = np.abs(got["u"].astype(np.float64) - V.astype(np.float64)).max(axis=0)
    print("max |u - V| per component:", err, "bound:", bound)
    assert (err <= bound).all(), (err, bound)
    dt = F32(ps._params.dt)
    assert np.array_equal(got["x"], (interior + dt * got["u"]).astype(F32))
    ps.close()


# ---- 12 -----------------------------------------------------------------------------------------------------------------
def test_run_simulation_writes_pathlines(tmp_path, monkeypatch):
    """27 particles in free fall, timeStepSize 0.016 so that every frame is an output interval: 3 frames, 3 files that grow by a
    frame each, and the final pathlines equal to a twin run's."""
    import json
    from sph_taichi_amd import run_simulation, tracers
    sd = scenes.fluid_only(counts=(3, 3, 3), start=(0.3, 0.3, 0.3))
    sd["Configuration"]["timeStepSize"] = 0.016
    sd["Configuration"]["tracers"] = {"lattice": {"start": [0.31, 0.31, 0.31], "end": [0.33, 0.31, 0.33], "spacing": 0.02}, "recordEvery": 1}
    scene_file = tmp_path / "tracer_scene.json"
    scene_file.write_text(json.dumps(sd))
    final = tmp_path / "final.vtk"
    monkeypatch.chdir(tmp_path)
    run_simulation.main(["--scene_file", str(scene_file), "--frames", "3", "--tracers", str(final)])
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    pts = tracers.lattice([0.31, 0.31, 0.31], [0.33, 0.31, 0.33], 0.02)
    assert pts.shape == (4, 3)
    tr = ps.set_tracers(pts, record_every=1, record_capacity=3)
    for k in range(3):
        solver.step(1)
        got, t = tracers.read_vtk(str(tmp_path / "tracer_scene_output" / f"tracers_{k:06}.vtk"))
        assert got.shape == (k + 1, 4, 3) and np.array_equal(got, tr.paths()) and np.array_equal(t, np.asarray(tr.times))
    got, t = tracers.read_vtk(str(final))
    assert np.array_equal(got, tr.paths()) and len(t) == 3 and (tr.wet_steps() == 3).all() and (got[2, :, 1] < got[0, :, 1]).all()
    ps.close()
