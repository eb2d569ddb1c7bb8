"""Fluid loads on the device (include/sph_hip.h, section "Fluid loads"; csrc/sph_loads.hip) against the brute-force numpy model of
tests/loads_model.py evaluated on the context's OWN state downloaded at the sample point.

Every comparison with the model is exact (array_equal on all nine i64 per object): the pair geometry is the same f32 sequence on both
sides, the coefficient and the components are IEEE f64 multiplies, divides and subtracts on both sides, llrint and np.rint both round
to nearest even, and every sum is an integer sum whatever the order.  The one tolerance in this file is the momentum balance of
`test_momentum_balance_on_the_device`, whose bound is 3 x the residual measured on the GPU (profiles/loads_parity.json).

A stand-alone sample is taken stage by stage (`_stages`): the sort, the density and equation-of-state entries of the path under test,
`ps.loads.sample()`.  The geometry tests upload density and pressure
fields of their own instead: the sample uses whatever the particle record holds."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

from sph_taichi_amd import _lib, loads
from tests import loads_model as model
from tests import loads_scenes
from tests import scenes

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUBE_OBJ = os.path.join(ROOT, "tests", "golden", "cube_0p1.obj")
CUBE_ANCHOR = (0.36, 0.20, 0.36)                   # the cube's top edge towards the side fluid: both fluid blocks are drawn to it
STATE = ("x", "m_V", "m", "density", "pressure", "material", "object_id")


def _open(sd, factor=0.9, seed=0, toward=None, fused=1, squeeze=True):
    cfg, sc = scenes.build(sd)
    if squeeze:
        loads_scenes.squeeze(sc, factor, seed=seed, toward=toward)
    ps, solver = scenes.make_ps(sd, sc.arrays, fused=fused)
    solver.initialize()
    return ps, solver


def _state(ps):
    return {f: getattr(ps, f).to_numpy() for f in STATE}


def _stages(ps, solver, fused=1):
    """One step's kernels up to the sample point, through the stage entries.  The fused step has ONE density-and-EOS phase (moving
    boundary volume, density sweep with the equation of state in its finish), which is an entry of its own; the unfused step's
    are the per-kernel entries.  The two density sweeps agree to rounding only (tests/test_gpu_parity.py), so each path's twin
    takes that path's own."""
    ps.initialize_particle_system()
    if fused:
        ps._call("sph_slab_density")
        return
    solver.compute_moving_boundary_volume()
    solver.compute_densities()
    solver.compute_pressure_forces()


def _model(ps, f, objects, about):
    return model.sample(f["x"], f["m_V"], f["material"], f["object_id"], f["m"], f["density"], f["pressure"], list(objects), about,
                        F32(ps._params.support_radius), F32(ps._params.density_0), F32(ps._params.k_dw))


def _same(got, want, tag=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype == np.int64 and got.shape == want.shape, tag
    assert np.array_equal(got, want), (tag, got.tolist(), want.tolist())


def _random_fields(ps, seed, p_max=5.0e4):
    """Density in [1000, 1400] and pressure in [0, p_max] of the sample's own making, then the sort (which carries them along)."""
    rng = np.random.default_rng(seed)
    n = ps.density.to_numpy().shape[0]
    ps.density.from_numpy(rng.uniform(1000.0, 1400.0, size=n).astype(F32))
    ps.pressure.from_numpy(rng.uniform(0.0, p_max, size=n).astype(F32))
    ps.initialize_particle_system()


# ---- 1: one stand-alone sample against the model ----------------------------------------------------------------------------
def test_one_step_against_the_model():
    """Fluid on and beside a static cube (object 1), a slab that is NOT selected (object 2, wet all the same) and a selected block
    that no fluid reaches (object 3): its row is all zero."""
    ps, solver = _open(loads_scenes.cube_scene(), toward=CUBE_ANCHOR)
    about = (0.36, 0.16, 0.36)
    ld = ps.set_loads(objects=[1, 3], about=about, every=1, capacity=4)
    assert ld is ps.loads and ld.info().samples == 0 and ld.history().raw.shape == (0, 2, 9)
    _stages(ps, solver)
    f = _state(ps)
    assert (f["material"] == 0).sum() == 371 and (f["material"] == 1).sum() == 480
    ld.sample()
    h = ld.history()
    want = _model(ps, f, [1, 3], about)
    _same(h.raw[0], want, "cube")
    assert h.samples == 1 and h.times[0] == ps.time and ld.info().steps_seen == 0
    assert want[0, 6] > 500 and 36 < want[0, 7] < 216 and want[0, 8] == 0 and not want[1].any()
    assert _model(ps, f, [2], about)[0, 6] > 100                     # the slab is wet too: it is left out because it is not selected
    assert h.force()[0, 0, 1] < 0 and h.force()[0, 0, 0] < 0          # pressed down by the fluid on top, towards -x by the fluid beside
    ld.sample()                                                       # a second sample of the same state: the next row, the same numbers
    h2 = ld.history()
    _same(h2.raw[1], want, "second row")
    _same(h2.raw[0], want, "first row untouched")
    # the same state about another point: the force is the same, the torque is the transported one up to its own rounding
    other = ps.set_loads(objects=[3, 1], about=(0.1, 0.9, 0.2), capacity=1)
    other.sample()
    h3 = other.history()
    _same(h3.raw[0], _model(ps, f, [3, 1], (0.1, 0.9, 0.2)), "other point, other order")
    assert np.array_equal(h3.raw[0, 1, 0:3], want[0, 0:3])
    # each target's arm x_j - c is one f32 subtraction (half an ulp of a length below 1.2, the domain: 2^-24 * 0.6 per component, for
    # either point, two products per torque component), each target's torque term rounds once to 2^-25 N m
    norm = model.pair_magnitude(f["x"], f["m_V"], f["material"], f["object_id"], f["m"], f["density"], f["pressure"], [1],
                                F32(ps._params.support_radius), F32(ps._params.density_0), F32(ps._params.k_dw))
    tol = 2 * 2 * (0.6 * 2.0 ** -24) * norm + 2 * int(want[0, 7]) * 2.0 ** -25
    assert np.abs(h3.torque()[0, 1] - h.torque(about=(0.1, 0.9, 0.2))[0, 0]).max() <= tol
    ps.close()


# ---- 2: the hook's sample against the stand-alone one -------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "unfused"])
def test_in_step_equals_stand_alone(fused):
    a, sa = _open(loads_scenes.cube_scene(), toward=CUBE_ANCHOR, fused=fused)
    b, sb = _open(loads_scenes.cube_scene(), toward=CUBE_ANCHOR, fused=fused)
    la, lb = a.set_loads(objects=[1, 2, 3], about=(0.5, 0.1, 0.4)), b.set_loads(objects=[1, 2, 3], about=(0.5, 0.1, 0.4))
    t0 = a.time
    sa.step(1)
    _stages(b, sb, fused)
    lb.sample()
    ha, hb = la.history(), lb.history()
    assert ha.samples == hb.samples == 1 and ha.raw[0, 0, 6] > 500 and ha.raw[0, 1, 6] > 100 and not ha.raw[0, 2].any()
    assert ha.raw.tobytes() == hb.raw.tobytes(), (ha.raw.tolist(), hb.raw.tolist())
    assert ha.times[0] == t0 == hb.times[0] and la.info().steps_seen == 1 and lb.info().steps_seen == 0
    _same(hb.raw[0], _model(b, _state(b), [1, 2, 3], (0.5, 0.1, 0.4)), "twin")
    a.close(); b.close()


# ---- 3: the clipped walk, ragged target counts, mixed waves -------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [None, "1"], ids=["whole-grid", "one-block"])
def test_geometry_edge_cases(blocks, monkeypatch):
    """Targets in the first and the last cell layer of every axis (the 27 cells are clipped on three sides at once); 57 targets, no
    multiple of 4 or 16; three objects whose counts 27, 18 and 12 cannot all fill whole waves of four rows, so some wave holds two
    objects and takes the per-row atomics.  With the gather's grid cut to one block (16 rows) the waves take four trips."""
    if blocks is None:
        monkeypatch.delenv("SPH_LOADS_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("SPH_LOADS_BLOCKS", blocks)
    ps, solver = _open(loads_scenes.corner_scene(), factor=1.0, seed=3)
    _random_fields(ps, seed=4)
    f = _state(ps)
    solid = f["material"] == 0
    assert [int((solid & (f["object_id"] == o)).sum()) for o in (1, 2, 3)] == [27, 18, 12] and solid.sum() % 4 == 1 and solid.sum() % 16 == 9
    n = np.asarray(ps.grid_num)
    cells = np.clip((f["x"][solid] / F32(ps._params.grid_size)).astype(np.int64), 0, n - 1)
    for axis in range(3):
        assert (cells[:, axis] == 0).any() and (cells[:, axis] == n[axis] - 1).any(), axis
    about = (0.5, 0.6, 0.4)
    ld = ps.set_loads(objects=[2, 3, 1], about=about)
    ld.sample()
    want = _model(ps, f, [2, 3, 1], about)
    _same(ld.history().raw[0], want, blocks)
    assert (want[:, 6] > 20).all() and (want[:, 7] > 3).all() and not want[:, 8].any()
    ps.close()


# ---- 4: crowded cells ---------------------------------------------------------------------------------------------------------
def test_crowded_cells():
    """512 fluid particles drawn into a 0.04 cube above the slab: cells with more than 16 and more than 64 fluid records, so a row's
    run takes up to 32 trips; one fluid particle sits exactly on a target (r = 0: refused by r > 1e-5)."""
    sd = loads_scenes.block_on_slab(fluid_counts=(8, 8, 8))
    cfg, sc = scenes.build(sd)
    loads_scenes.squeeze(sc, 0.25, seed=6, amplitude=0.02)
    a = sc.arrays
    top = np.nonzero((a["material"] == 0) & (a["x"][:, 1] > 0.07))[0]
    a["x"][np.nonzero(a["material"] == 1)[0][0]] = a["x"][top[top.size // 2]]
    a["x_0"] = a["x"].copy()
    ps, solver = scenes.make_ps(sd, a)
    solver.initialize()
    _random_fields(ps, seed=7, p_max=50.0)
    f = _state(ps)
    fluid = f["material"] == 1
    n = np.asarray(ps.grid_num)
    cell = np.clip((f["x"][fluid] / F32(ps._params.grid_size)).astype(np.int64), 0, n - 1)
    occupancy = np.bincount(np.ravel_multi_index(cell.T, n))
    assert occupancy.max() > 64 and ((occupancy > 16) & (occupancy <= 64)).any()
    ld = ps.set_loads(objects=[1], about=(0.2, 0.1, 0.2))
    ld.sample()
    want = _model(ps, f, [1], (0.2, 0.1, 0.2))
    _same(ld.history().raw[0], want, "crowded")
    assert want[0, 6] > 1000 and want[0, 8] == 0
    d = f["x"][fluid][:, None, :] - f["x"][~fluid][None, :, :]
    assert (np.sqrt((d.astype(np.float64) ** 2).sum(axis=-1)) == 0).sum() == 1
    ps.close()


# ---- 5: every, capacity, dropped, reset, replace, clear -----------------------------------------------------------------------
def test_bookkeeping_over_twelve_steps():
    ps, solver = _open(loads_scenes.block_on_slab(), seed=2)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_loads_sample.*no load set"):
        ps._call("sph_loads_sample")
    assert ps.loads is None
    ld = ps.set_loads(objects=[1], every=3, capacity=3)
    times = []
    for k in range(12):
        times.append(ps.time)
        solver.step(1)
    i = ld.info()
    assert (i.n_objects, i.every, i.samples, i.dropped, i.steps_seen) == (1, 3, 3, 1, 12)          # steps 0 3 6 kept, step 9 dropped
    h = ld.history()
    assert h.raw.shape == (3, 1, 9) and np.array_equal(h.times, np.array(times)[[0, 3, 6]]) and (h.raw[:, 0, 6] > 0).all()
    assert len({r.tobytes() for r in h.raw}) == 3 and h.impulse().shape == (1, 3) and h.impulse()[0, 1] < 0
    ld.sample()                                                        # a stand-alone sample of a full history is dropped alike
    assert (ld.info().samples, ld.info().dropped) == (3, 2) and ld.history().raw.tobytes() == h.raw.tobytes()
    ld.reset()
    i = ld.info()
    assert (i.samples, i.dropped, i.steps_seen, i.every, i.n_objects) == (0, 0, 0, 3, 1) and ld.history().raw.shape == (0, 1, 9)
    solver.step(4)                                                     # steps 0 and 3 of the new count
    assert ld.info().samples == 2 and ld.info().steps_seen == 4 and (ld.history().raw[:, 0, 6] > 0).all()
    big = ps.set_loads(objects=[1, 0], every=1, capacity=64)           # replaced by a larger set: zeroed, the fluid's own object has no solids
    assert big.info().samples == 0
    solver.step(2)
    hb = big.history()
    assert hb.raw.shape == (2, 2, 9) and (hb.raw[:, 0, 6] > 0).all() and not hb.raw[:, 1].any()
    ps.clear_loads()
    assert ps.loads is None and big.info().samples == 0
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_loads_download.*no load set"):
        ps._call("sph_loads_download", None, None, 0, 2)
    solver.step(1)
    ps.close()


# ---- 6: the momentum balance, on the device --------------------------------------------------------------------------------
def test_momentum_balance_on_the_device():
    """After sph_step(1): sum_i m_i (a_i - g) over the fluid plus the sampled load of that step vanishes (one uniform fluid mass: the
    fluid-fluid pairs cancel), normalised by the sum over the fluid-solid pairs of |f|.  The force sweep works in f32 with hardware
    reciprocals, the load in f64.  MEASURED on the MI355X: 3.3e-08 (profiles/loads_parity.json); the bound is 3 x that figure."""
    parity = json.load(open(os.path.join(ROOT, "profiles", "loads_parity.json")))
    ps, solver = _open(loads_scenes.block_on_slab(), seed=1)
    ld = ps.set_loads(objects=[1])
    x0 = scenes.ps_by_pid(ps, "x")
    solver.step(1)
    f = {k: scenes.ps_by_pid(ps, k) for k in STATE}
    f["x"] = x0                                                        # the sample saw x(t_k); density and pressure are this step's
    acc = scenes.ps_by_pid(ps, "acceleration")
    fluid = f["material"] == 1
    F = ld.force()[0, 0]
    g = np.array([float(v) for v in ps._params.g])
    fluid_side = (f["m"][fluid].astype(np.float64)[:, None] * (acc[fluid].astype(np.float64) - g)).sum(axis=0)
    norm = model.pair_magnitude(f["x"], f["m_V"], f["material"], f["object_id"], f["m"], f["density"], f["pressure"], [1],
                                F32(ps._params.support_radius), F32(ps._params.density_0), F32(ps._params.k_dw))
    residual = float(np.abs(fluid_side + F).max() / norm)
    print(f"load {F}, fluid side {fluid_side}, sum over pairs of |f| {norm:.6e}, residual {residual:.3e}")
    assert norm > 1.0 and F[1] < 0 and ld.saturated()[0, 0] == 0
    measured = parity["momentum_balance"]["measured_residual"]
    assert parity["momentum_balance"]["bound"] <= 3 * measured
    scenes.bound("loads_parity", "momentum_balance", residual, parity["momentum_balance"]["bound"])
    ps.close()


# ---- 7: the step is untouched -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["fluid_and_solids", "pure_fluid"])
def test_the_step_is_untouched(scene):
    """Positions and velocities after 20 steps with a set armed equal those of a run without, bit for bit.  On the pure-fluid scene the
    lean sort is excluded while the set is armed (the sample reads the particle record): other kernels, the same bits."""
    if scene == "fluid_and_solids":
        sd, kw, objects = loads_scenes.cube_scene(), dict(toward=CUBE_ANCHOR, factor=0.97), [1, 2]
    else:
        sd, kw, objects = scenes.fluid_only(counts=(12, 12, 10), velocity=(0.3, -1.0, 0.2)), dict(squeeze=False), [0]
    runs = []
    for armed in (False, True):
        ps, solver = _open(copy.deepcopy(sd), **kw)
        if armed:
            ps.set_loads(objects=objects, every=2)
        solver.step(7)
        solver.step(1)
        solver.step(12)
        if armed:
            raw = ps.loads.history().raw
            assert ps.loads.info().samples == 10 and raw.shape == (10, len(objects), 9)
            assert raw[:, :, 6].any() if scene == "fluid_and_solids" else not raw.any()
        runs.append({n: getattr(ps, n).to_numpy().copy() for n in ("x", "v", "pid", "density", "pressure")})
        ps.close()
    off, on = runs
    for n in off:
        assert off[n].tobytes() == on[n].tobytes(), n


# ---- 8: a kinematic and a dynamic body ------------------------------------------------------------------------------------------
def test_kinematic_and_dynamic_bodies_after_five_steps():
    """A dynamic RigidBody dropped into the fluid and a kinematic one swept through it: the hook's sample of the fifth step equals a
    stand-alone sample of a twin after four steps, and both equal the model on the twin's state."""
    body = lambda oid, tr, dyn, rho, vel=(0.0, 0.0, 0.0): {
        "objectId": oid, "geometryFile": CUBE_OBJ, "translation": list(tr), "rotationAxis": [0, 0, 1], "rotationAngle": 0, "scale": [1, 1, 1],
        "velocity": list(vel), "density": rho, "color": [200, 180, 90], "isDynamic": dyn}
    sd = scenes.fluid_only(counts=(10, 10, 8), start=(0.1, 0.1, 0.1), velocity=(0.0, -1.0, 0.0))
    sd["RigidBodies"] = [body(1, (0.14, 0.30, 0.12), True, 600.0, (0.0, -2.0, 0.0)), body(2, (0.295, 0.14, 0.12), False, 1000.0)]
    about = (0.2, 0.2, 0.2)
    ctxs = []
    for _ in range(2):
        ps, solver = _open(copy.deepcopy(sd), factor=0.97, seed=5)
        ps.set_body_motion(2, linearVelocity=[-1.0, 0.3, 0.1], angularVelocity=[0.4, -0.3, 3.0])
        ctxs.append((ps, solver))
    (a, sa), (b, sb) = ctxs
    la = a.set_loads(objects=[1, 2], about=about, every=1, capacity=8)
    sa.step(5)
    sb.step(4)
    lb = b.set_loads(objects=[1, 2], about=about, every=1, capacity=8)
    _stages(b, sb)
    f = _state(b)
    lb.sample()
    ha, hb = la.history(), lb.history()
    assert ha.samples == 5 and hb.samples == 1
    want = _model(b, f, [1, 2], about)
    _same(hb.raw[0], want, "twin against the model")
    _same(ha.raw[4], want, "the hook's fifth sample")
    assert (want[:, 6] > 20).all() and want[:, 0:3].any(axis=1).all()   # both bodies are wet and loaded
    assert b.is_dynamic.to_numpy()[f["object_id"] == 1].all() and not b.is_dynamic.to_numpy()[f["object_id"] == 2].any()
    a.close(); b.close()


# ---- 9: refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    ps, solver = _open(loads_scenes.cube_scene(), toward=CUBE_ANCHOR)
    good = ps.set_loads(objects=[1], about=(0.3, 0.1, 0.3), capacity=4)
    solver.step(1)
    kept = good.history().raw.tobytes()
    base = loads.set_args(objects=[1, 2], capacity=4)

    def params(**kw):
        p = loads.load_params(base)
        for k, v in kw.items():
            if k == "ids":
                for j, oid in enumerate(v):
                    p.object_ids[j] = oid
            elif k == "about":
                p.about = (C.c_float * 3)(*v)
            else:
                setattr(p, k, v)
        return p
    for kw, word in ((dict(ids=[1, 9]), r"object id 9 is outside \[0, n_objects = \d+\)"), (dict(ids=[-1, 2]), "object id -1"),
                     (dict(ids=[2, 2]), "duplicate object id 2"), (dict(n_objects=0), "n_objects"), (dict(n_objects=33), "n_objects"),
                     (dict(about=(0.0, float("nan"), 0.0)), "about"), (dict(about=(float("inf"), 0.0, 0.0)), "about"), (dict(every=0), "every"),
                     (dict(capacity=0), "capacity"), (dict(capacity=1 << 30), "capacity")):
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*sph_loads_set.*{word}"):
            ps._call("sph_loads_set", C.byref(params(**kw)))
        assert good.info().samples == 1 and good.history().raw.tobytes() == kept, kw             # a refused set changes nothing
    for samples, n_objects in ((2, 1), (1, 2), (0, 1)):
        with pytest.raises(_lib.SphError, match=r"rc=-1.*sph_loads_download.*the set holds 1 samples of 1 objects"):
            ps._call("sph_loads_download", None, None, samples, n_objects)
    solver.step(1)
    assert good.info().samples == 2                                                               # the last good set goes on being sampled
    ps.close()
    # a sample on a context that has not been sorted
    cfg, sc = scenes.build(loads_scenes.block_on_slab())
    fresh, _ = scenes.make_ps(loads_scenes.block_on_slab(), sc.arrays)
    fresh.set_loads(objects=[1])
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_loads_sample.*needs the neighbour structure"):
        fresh.loads.sample()
    fresh.close()
    # DFSPH steps refuse to run with a set, and run again once it is cleared
    df, dsolver = scenes.make_ps(scenes.as_dfsph(loads_scenes.block_on_slab()))
    dsolver.initialize()
    df.set_loads(objects=[1])
    t = df.time
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_dfsph_step.*load set is registered"):
        dsolver.step(1)
    assert df.time == t and df.loads.info().steps_seen == 0
    df.clear_loads()
    dsolver.step(1)
    df.close()


def test_slab_rank_is_refused():
    from sph_taichi_amd import ParticleSystem
    from sph_taichi_amd.config_builder import SimConfig
    sd = scenes.fluid_only(counts=(4, 4, 4))
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.set_loads(objects=[0])
    p = loads.load_params(loads.set_args(objects=[0]))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_loads_set.*single-domain"):
        slab._call("sph_loads_set", C.byref(p))
    for name, args in (("sph_loads_sample", ()), ("sph_loads_download", (None, None, 0, 1)), ("sph_loads_reset", ())):
        with pytest.raises(_lib.SphError, match=rf"rc=-4.*{name}.*single-domain"):
            slab._call(name, *args)
    slab.close()


# ---- 10: saturation -----------------------------------------------------------------------------------------------------------
def test_saturation_is_counted_and_equals_the_model():
    ps, solver = _open(loads_scenes.cube_scene(), toward=CUBE_ANCHOR)
    _stages(ps, solver)
    f = _state(ps)
    cube = (f["material"] == 0) & (f["object_id"] == 1)
    fluid = np.nonzero(f["material"] == 1)[0]
    d = np.sqrt(((f["x"][fluid][:, None, :].astype(np.float64) - f["x"][cube][None, :, :]) ** 2).sum(axis=-1)).min(axis=1)
    near = fluid[np.argsort(d)[:2]]
    p = f["pressure"].copy()
    p[near[0]], p[near[1]] = F32(1.0e30), F32(np.inf)                  # one far over the clamp, one whose terms are infinite or NaN
    ps.pressure.from_numpy(p)
    ps.initialize_particle_system()
    f = _state(ps)
    ld = ps.set_loads(objects=[1, 2], about=(0.36, 0.16, 0.36))
    ld.sample()
    want = _model(ps, f, [1, 2], (0.36, 0.16, 0.36))
    _same(ld.history().raw[0], want, "saturated")
    assert want[0, 8] > 0 and ld.saturated()[0, 0] == want[0, 8] and np.abs(want[0, 0:3]).max() >= 1 << 40
    ps.close()


# ---- 11: run_simulation -------------------------------------------------------------------------------------------------------
def test_run_simulation_writes_the_series(tmp_path, monkeypatch, capsys):
    sd = loads_scenes.block_on_slab(fluid_counts=(4, 4, 4), slab_counts=(6, 2, 6))
    sd["Configuration"]["timeStepSize"] = 0.016                        # every frame is an output interval
    sd["Configuration"]["loads"] = {"objects": [1], "about": [0.2, 0.1, 0.2], "every": 2, "capacity": 16}
    scene_file = tmp_path / "loads_scene.json"
    scene_file.write_text(json.dumps(sd))
    final = tmp_path / "final.csv"
    monkeypatch.chdir(tmp_path)
    from sph_taichi_amd import run_simulation
    run_simulation.main(["--scene_file", str(scene_file), "--frames", "5", "--loads", str(final)])
    report = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert report["loads"] == {"objects": [1], "every": 2, "samples": 3, "dropped": 0, "steps_seen": 5}
    for path in (final, tmp_path / "loads_scene_output" / "loads.csv"):
        back = loads.read_csv(str(path))
        assert back["time"].shape == (3,) and back["about"] == tuple(float(F32(v)) for v in (0.2, 0.1, 0.2))
        assert np.array_equal(back["object"], [1, 1, 1]) and back["force"].shape == (3, 3) and back["time"][0] == 0.0
    with pytest.raises(ValueError, match="--loads needs"):
        sd["Configuration"].pop("loads")
        scene_file.write_text(json.dumps(sd))
        run_simulation.main(["--scene_file", str(scene_file), "--frames", "1", "--loads", str(final)])
