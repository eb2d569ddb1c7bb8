"""Flow diagnostics on the device (include/sph_hip.h, last section; csrc/sph_diag.hip) and the CFL-governed time step.

The model is numpy in f64 on the context's OWN downloaded fields, taken right after the reduction.  Tolerances are derived:
  * counts, lo / hi and the density / pressure extrema are EXACT (integers; minima and maxima of f32 values);
  * v2_max, a2_max: relative 4 * 2^-53 -- the three squares of f32 components are exact in f64, only the two additions
    round (or one, where the compiler contracts a product into an fma);
  * every f64 sum: absolute 4 * N * 2^-53 * sum |term| with N the row's particle count -- the bound for adding N terms in
    any order, times a factor for the roundings inside the terms (m x is exact in f64, 1/2 m |v|^2 is not).
"""
import copy
import math
import os
import types

import numpy as np
import pytest

from sph_taichi_amd import ParticleSystem, _lib, motion, timestep
from sph_taichi_amd.config_builder import SimConfig
from tests import scenes

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUBE = os.path.join(ROOT, "tests", "golden", "cube_0p1.obj")
FIELDS = ("x", "v", "acceleration", "m_V", "m", "density", "pressure", "material", "color", "is_dynamic", "object_id",
          "grid_ids")
MODEL_FIELDS = ("x", "v", "acceleration", "m", "density", "pressure", "material", "is_dynamic", "object_id")


def _download(ps):
    return {f: getattr(ps, f).to_numpy() for f in MODEL_FIELDS}


def _model_row(f, mask):
    """What one row must hold, from the downloaded fields restricted to `mask`, plus sum |term| of every sum."""
    x32, rho, p = f["x"][mask], f["density"][mask], f["pressure"][mask]
    x, v, a = x32.astype(np.float64), f["v"][mask].astype(np.float64), f["acceleration"][mask].astype(np.float64)
    m = f["m"][mask].astype(np.float64)
    fluid = f["material"][mask] == 1
    moving = fluid | (f["is_dynamic"][mask] != 0)
    n = int(mask.sum())
    v2 = (v * v).sum(axis=1)
    a2 = (a * a).sum(axis=1)
    kin = 0.5 * m * v2
    r = {"count": n, "fluid_count": int(fluid.sum()), "moving_count": int(moving.sum()),
         "mass": m.sum(), "mx": (m[:, None] * x).sum(axis=0), "momentum": (m[:, None] * v).sum(axis=0), "kinetic": kin.sum(),
         "v2_max": v2.max() if n else 0.0, "a2_max": a2[moving].max() if moving.any() else 0.0,
         "density_min": rho[fluid].min() if fluid.any() else 0.0, "density_max": rho[fluid].max() if fluid.any() else 0.0,
         "pressure_min": p[fluid].min() if fluid.any() else 0.0, "pressure_max": p[fluid].max() if fluid.any() else 0.0,
         "lo": x32.min(axis=0) if n else np.zeros(3), "hi": x32.max(axis=0) if n else np.zeros(3)}
    mag = {"mass": np.abs(m).sum(), "mx": np.abs(m[:, None] * x).sum(axis=0), "momentum": np.abs(m[:, None] * v).sum(axis=0),
           "kinetic": np.abs(kin).sum()}
    return r, mag


def _check_row(name, row, want, mag):
    worst = 0.0
    for k in ("count", "fluid_count", "moving_count"):
        assert getattr(row, k) == want[k], (name, k, getattr(row, k), want[k])
    for k in ("density_min", "density_max", "pressure_min", "pressure_max"):
        assert getattr(row, k) == float(want[k]), (name, k, getattr(row, k), float(want[k]))
    for k in ("lo", "hi"):
        assert np.array_equal(np.asarray(getattr(row, k), dtype=np.float32), np.asarray(want[k], dtype=np.float32)), (name, k)
    for k in ("v2_max", "a2_max"):
        got, ref = getattr(row, k), float(want[k])
        err, tol = abs(got - ref), 4 * U * abs(ref)
        worst = max(worst, err / tol if tol else (0.0 if err == 0.0 else math.inf))
        assert err <= tol, (name, k, got, ref)
    n = max(want["count"], 1)
    for k in ("mass", "mx", "momentum", "kinetic"):
        got, ref = np.atleast_1d(np.asarray(getattr(row, k), dtype=np.float64)), np.atleast_1d(want[k])
        tol = 4 * n * U * np.atleast_1d(mag[k])
        err = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
        worst = max(worst, float(ratio.max()))
        assert np.all(err <= tol), (name, k, got, ref, tol)
    return worst


def _check_against_numpy(ps, diag, tag):
    """Every object row and the total against the numpy model on the fields as they are now."""
    f = _download(ps)
    n_objects = int(ps._params.n_objects)
    assert len(diag.objects) == n_objects and diag.time == ps.time
    worst = 0.0
    for k in range(n_objects):
        want, mag = _model_row(f, f["object_id"] == k)
        worst = max(worst, _check_row(f"{tag}: object {k}", diag.objects[k], want, mag))
    want, mag = _model_row(f, np.ones(f["object_id"].shape[0], dtype=bool))
    worst = max(worst, _check_row(f"{tag}: total", diag.total, want, mag))
    in_range = (f["object_id"] >= 0) & (f["object_id"] < n_objects)
    assert diag.total.count == f["object_id"].shape[0]
    assert sum(r.count for r in diag.objects) == int(in_range.sum())
    print(f"{tag}: N = {diag.total.count}, {n_objects} objects, counts {[r.count for r in diag.objects]}; "
          f"worst error / bound over the f64 members = {worst:.3f}")
    return f


def _check_derived(diag, g):
    t = diag.total
    assert t.v_max == math.sqrt(t.v2_max) and t.a_max == math.sqrt(t.a2_max)
    assert t.center_of_mass == tuple(c / t.mass for c in t.mx)
    assert t.potential == -sum(gc * c for gc, c in zip(g, t.mx)) and t.energy == t.kinetic + t.potential
    d = diag.as_dict()
    assert d["total"]["count"] == t.count and len(d["objects"]) == len(diag.objects) and d["time"] == diag.time


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def test_reduction_against_numpy_mixed_scene():
    """Fluid + static block + dynamic block (three object ids) after step(7): the fused path, so the fluid's density and
    pressure sit in the lean record when diagnostics() is called -- before any download could have folded them back."""
    sd = scenes.fluid_with_rigid_blocks()
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    solver.step(7)
    diag = ps.diagnostics()
    n = ps.particle_max_num
    assert n % 64 != 0 and n % 256 != 0 and n > 256, n            # a ragged tail, more than one block
    f = _check_against_numpy(ps, diag, "mixed scene, step 7")
    assert int(ps._params.n_objects) == 3 and all(r.count > 0 for r in diag.objects)
    assert diag.total.count == sum(r.count for r in diag.objects) == n
    assert diag.objects[0].fluid_count == diag.objects[0].count and diag.objects[1].moving_count == 0
    assert diag.objects[2].moving_count == diag.objects[2].count and diag.objects[2].fluid_count == 0
    assert diag.objects[1].density_max == 0.0 and diag.objects[1].a2_max == 0.0      # no fluid / nothing moving: zeros
    assert diag.total.pressure_max > 0.0 and diag.total.a2_max > 0.0 and f["density"].max() > 0
    _check_derived(diag, sd["Configuration"]["gravitation"])
    ps.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_less_than_one_wave():
    """27 particles right after initialize(): one partly filled wave; the acceleration is still all zero."""
    sd = scenes.fluid_only(counts=(3, 3, 3))
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    diag = ps.diagnostics()
    assert diag.total.count == 27 == diag.objects[0].count and diag.total.a2_max == 0.0
    assert diag.total.v2_max == 1.0 and diag.total.momentum[1] < 0.0
    _check_against_numpy(ps, diag, "27 particles")
    ps.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def _smallest_block_above(threshold):
    s = int(round(threshold ** (1.0 / 3.0)))
    best = None
    for a in range(s - 2, s + 3):
        for b in range(a, s + 3):
            for c in range(b, s + 3):
                if a * b * c > threshold and (best is None or a * b * c < best[0]):
                    best = (a * b * c, (a, b, c))
    return best[1]


def test_more_than_one_pass_of_the_grid():
    """N just above SPH_DIAG_BLOCKS * SPH_DIAG_THREADS: some lanes take a second particle, most do not, and the last
    wave of the second pass is ragged."""
    per_pass = _lib.DIAG_BLOCKS * _lib.DIAG_THREADS
    counts = _smallest_block_above(per_pass)
    n = counts[0] * counts[1] * counts[2]
    assert per_pass < n < 1.05 * per_pass and n % 64 != 0, (counts, n)
    end = [math.ceil((0.1 + c * 0.02 + 0.1) * 10) / 10 for c in counts]
    sd = scenes.fluid_only(counts=counts, domain_end=end)
    ps, solver = scenes.make_ps(sd)
    assert ps.particle_max_num == n
    solver.initialize()
    solver.step(2)
    diag = ps.diagnostics()
    _check_against_numpy(ps, diag, f"{counts} block")
    ps.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def _raw_bytes(ps):
    from sph_taichi_amd import diagnostics
    return bytes(diagnostics.download_rows(ps))


def _all_fields(ps):
    return {f: scenes.ps_by_pid(ps, f) for f in FIELDS}


def test_repeatable_and_side_effect_free():
    sd = scenes.fluid_with_rigid_blocks()
    a, solver_a = scenes.make_ps(sd)
    solver_a.initialize()
    solver_a.step(5)
    first, second = _raw_bytes(a), _raw_bytes(a)          # the first call folds density / pressure back, the second finds them
    assert first == second and len(first) == 4 * 144
    d = a.diagnostics()
    assert d.total.count == a.particle_max_num
    solver_a.step(5)
    b, solver_b = scenes.make_ps(sd)
    solver_b.initialize()
    solver_b.step(10)
    fa, fb = _all_fields(a), _all_fields(b)
    for f in FIELDS:
        assert np.array_equal(fa[f], fb[f]), f"{f} differs after diagnostics between the steps"
    assert a.time == b.time
    a.close(); b.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_reduction_against_numpy_dfsph():
    sd = scenes.as_dfsph(scenes.fluid_with_rigid_blocks())
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    solver.step(3)
    diag = ps.diagnostics()
    _check_against_numpy(ps, diag, "DFSPH mixed scene, step 3")
    assert diag.total.a2_max > 0.0 and diag.objects[0].density_max > 0.0      # (DFSPH does not clamp the density at rho0)
    ps.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    sd = scenes.fluid_only(counts=(4, 4, 4))
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    n_rows = int(ps._params.n_objects) + 1
    rows = (_lib.SphDiagRow * (n_rows + 1))()
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been reduced"):
        ps._call("sph_diag_download", rows, n_rows)
    ps._call("sph_diag_reduce")
    for bad in (n_rows - 1, n_rows + 1):
        with pytest.raises(_lib.SphError, match=r"rc=-1.*n_objects \+ 1"):
            ps._call("sph_diag_download", rows, bad)
    ps._call("sph_diag_download", rows, n_rows)
    assert rows[n_rows - 1].count == 64
    ps.close()
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.diagnostics()
    slab.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
ADAPTIVE = {"cflVelocity": 0.01}


def _numpy_total(ps):
    f = _download(ps)
    v, a = f["v"].astype(np.float64), f["acceleration"].astype(np.float64)
    fluid = f["material"] == 1
    moving = fluid | (f["is_dynamic"] != 0)
    return types.SimpleNamespace(v_max=math.sqrt((v * v).sum(axis=1).max()),
                                 a_max=math.sqrt((a * a).sum(axis=1)[moving].max()) if moving.any() else 0.0,
                                 density_max=float(f["density"][fluid].max()) if fluid.any() else 0.0)


def test_adaptive_run_equals_the_run_with_dt_set_by_hand():
    """cflVelocity = 0.01 makes dt_v = 0.01 * 0.02 / |v| = 2e-4 at the start, below timeStepSize = 4e-4, and smaller after
    every block as the free fall adds about g dt per step to max |v|."""
    sd = scenes.fluid_only()
    sd["Configuration"]["adaptiveTimeStep"] = dict(ADAPTIVE)
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    controller = ps.build_time_step_controller(solver)
    assert isinstance(controller, timestep.TimeStepController)
    dt_used = [float(np.float32(solver.dt[None]))]          # block k runs at dt_used[k]
    t = 0.0
    for k in range(6):
        solver.step(5)
        for _ in range(5):
            t += dt_used[k]                                  # the library's additions: f64 += (f64) f32 dt, once per step
        dt, diag = controller.update()
        want = timestep.cfl_dt(_numpy_total(ps), diameter=ps.particle_diameter, dt_prev=dt_used[k], cfg=controller.cfg,
                               sound_speed=controller.sound_speed)
        assert dt == want == float(np.float32(dt)) == solver.dt[None], (k, dt, want)
        assert diag.time == ps.time == t, (k, diag.time, t)
        dt_used.append(dt)
    print("adaptive dt per block:", dt_used)
    assert len(set(dt_used)) >= 3, dt_used                   # the controller acted, and kept acting
    assert all(b < a for a, b in zip(dt_used[1:-1], dt_used[2:])), "max |v| grows in free fall: dt_v must shrink"
    assert controller.updates == 6 and controller.dt_max_used == dt_used[0] and controller.dt_min_used == min(dt_used)
    assert controller.cfg["minTimeStepSize"] < min(dt_used), "the lower clamp must not be what is tested here"
    # the same sequence set by hand, no controller, no diagnostics
    ps2, solver2 = scenes.make_ps(scenes.fluid_only())
    solver2.initialize()
    assert ps2.build_time_step_controller(solver2) is None
    for k in range(6):
        solver2.dt[None] = dt_used[k]
        solver2.step(5)
    assert ps2.time == ps.time == t
    fa, fb = _all_fields(ps), _all_fields(ps2)
    for f in FIELDS:
        assert np.array_equal(fa[f], fb[f]), f
    ps.close(); ps2.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
BODY = 1
SWEEP = {"linearVelocity": [-1.0, 0.3, 0.1], "angularVelocity": [0.4, -0.3, 3.0],
         "oscillation": {"amplitude": [0.0, 0.004, 0.002], "frequency": 40.0, "phase": 0.3}}
EPS = 2.0 ** -24


def kin_scene(motion_spec, translation=(0.30, 0.14, 0.12)):
    """The scene of tests/test_gpu_kinematic.py: the fluid block falling at 1 m/s with the voxelised 0.1 m cube, a kinematic
    body, one particle spacing to its +x side."""
    sd = scenes.fluid_only(counts=(10, 10, 8), start=(0.1, 0.1, 0.1), velocity=(0.0, -1.0, 0.0))
    sd["RigidBodies"] = [{"objectId": BODY, "geometryFile": CUBE, "translation": list(translation), "rotationAxis": [0, 0, 1],
                          "rotationAngle": 0, "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "density": 1000.0,
                          "color": [200, 180, 90], "isDynamic": False, "motion": copy.deepcopy(motion_spec)}]
    return sd


def test_variable_dt_reaches_the_pose_clock():
    """A kinematic body under the adaptive step: after 4 blocks of 5 steps at changing dt the body stands at the closed form
    of ps.time, within the rounding bound of the pose test of tests/test_gpu_kinematic.py:
        |x - x_ref| <= 16 * 2^-24 * (|origin|_inf + |x_0 - pivot|_1),  |v - v_ref| <= 16 * 2^-24 * (|u|_inf + |w| |x_0 - pivot|_1)."""
    sd = kin_scene(SWEEP)
    sd["Configuration"]["adaptiveTimeStep"] = dict(ADAPTIVE)
    cfg, sc = scenes.build(sd)
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    controller = ps.build_time_step_controller(solver)
    dt_used = [float(np.float32(solver.dt[None]))]
    t = 0.0
    for k in range(4):
        solver.step(5)
        for _ in range(5):
            t += dt_used[k]
        dt_used.append(controller.update()[0])
    assert ps.time == t and len(set(dt_used[:4])) >= 3 and t < 20 * dt_used[0], (dt_used, t)
    body = sc.arrays["object_id"] == BODY
    m = sc.motions[BODY]
    x0 = sc.arrays["x_0"][body].astype(np.float64)
    R, c, u, w = motion.pose(m, t)
    X, V = motion.apply_pose(R, c, u, w, m.pivot, x0)
    q1 = np.abs(x0 - m.pivot).sum(axis=1, keepdims=True)
    x, v = scenes.ps_by_pid(ps, "x")[body].astype(np.float64), scenes.ps_by_pid(ps, "v")[body].astype(np.float64)
    ex = np.abs(x - X) / (16 * EPS * (np.abs(c).max() + q1))
    ev = np.abs(v - V) / (16 * EPS * (np.abs(u).max() + np.linalg.norm(w) * q1))
    print(f"pose at t = {t:.6e} (dt per block {dt_used[:4]}): worst |x err| / bound = {ex.max():.3f}, |v err| / bound = {ev.max():.3f}")
    assert ex.max() <= 1.0 and ev.max() <= 1.0
    # the pose of the fixed-dt clock is somewhere else: the variable dt did reach the clock
    X_fixed, _ = motion.apply_pose(*motion.pose(m, 20 * dt_used[0]), m.pivot, x0)
    assert np.abs(X_fixed - X).max() > 100 * 16 * EPS
    # and the body's diagnostics row is the body
    row = ps.diagnostics().objects[BODY]
    assert row.count == int(body.sum()) and row.fluid_count == 0 and row.moving_count == 0
    assert np.array_equal(np.asarray(row.lo, np.float32), scenes.ps_by_pid(ps, "x")[body].min(axis=0))
    ps.close()
