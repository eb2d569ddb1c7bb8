"""Kinematic rigid bodies on the device (include/sph_hip.h, last section): the pose kernel against the closed form, the step
with a prescribed body against the unmodified CPU oracle driven one step at a time (its body rows overwritten with the
closed form after every step), and the no-op / reproducibility / restart / refusal properties.

Scene: domain (1.0, 1.2, 0.8), r = 0.01, a 10 x 10 x 8 fluid block and the 0.1 m cube of tests/golden voxelised to 216
particles -- more than a wave, not a multiple of the 256-thread block, spread over several cells (h = 0.04)."""
import copy
import math
import os

import numpy as np
import pytest

from sph_taichi_amd import _lib, motion
from tests import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUBE = os.path.join(ROOT, "tests", "golden", "cube_0p1.obj")
EPS = 2.0 ** -24
BODY = 1
FIELDS = ("x", "v", "acceleration", "m_V", "m", "density", "pressure", "material", "color", "is_dynamic", "object_id",
          "grid_ids")


def _body(oid, translation, dynamic=False, density=1000.0, velocity=(0.0, 0.0, 0.0), **kw):
    b = {"objectId": oid, "geometryFile": CUBE, "translation": list(translation), "rotationAxis": [0, 0, 1],
         "rotationAngle": 0, "scale": [1, 1, 1], "velocity": list(velocity), "density": density,
         "color": [200, 180, 90], "isDynamic": dynamic}
    b.update(kw)
    return b


def kin_scene(motion_spec=None, dt=None, translation=(0.30, 0.14, 0.12)):
    """The fluid block (x 0.10..0.28) falling at 1 m/s with the cube one particle spacing to its +x side."""
    sd = scenes.fluid_only(counts=(10, 10, 8), start=(0.1, 0.1, 0.1), velocity=(0.0, -1.0, 0.0))
    sd["RigidBodies"] = [_body(BODY, translation)]
    if motion_spec is not None:
        sd["RigidBodies"][0]["motion"] = copy.deepcopy(motion_spec)
    if dt is not None:
        sd["Configuration"]["timeStepSize"] = dt
    return sd


SWEEP = {"linearVelocity": [-1.0, 0.3, 0.1], "angularVelocity": [0.4, -0.3, 3.0],
         "oscillation": {"amplitude": [0.0, 0.004, 0.002], "frequency": 40.0, "phase": 0.3}}


def _check_shape(sc):
    n = int((sc.arrays["object_id"] == BODY).sum())
    assert n > 64 and n % 256 != 0, n                       # several waves, a ragged tail
    x = sc.arrays["x"][sc.arrays["object_id"] == BODY]
    cells = np.unique(np.floor(x / np.float32(sc.geom.grid_size)).astype(np.int64), axis=0)
    assert len(cells) >= 8, "the body must spread over several cells (the sort then scatters its particles)"
    return n


def _closed_form(m, t, x0):
    """numpy f64: (x, v) of rest positions x0 at time t."""
    R, c, u, w = motion.pose(m, t)
    return motion.apply_pose(R, c, u, w, m.pivot, x0)


def _dt32(sd):
    return float(np.float32(sd["Configuration"]["timeStepSize"]))     # the dt the library holds (SphParams.dt is f32)


def _drive_oracle(o, sc, motions, n, dt32, per_step=None):
    """n x (oracle.step(1); overwrite the kinematic bodies' rows with the f32-rounded closed form of the step's end time).
    The clock makes the library's additions: t += (f64) dt32."""
    x0 = sc.arrays["x_0"].astype(np.float64)               # by persistent id (the creation order)
    t = 0.0
    for _ in range(n):
        o.step(1)
        t += dt32
        for oid, m in motions.items():
            rows = np.nonzero(o["object_id"] == oid)[0]
            X, V = _closed_form(m, t, x0[o["pid"][rows]])
            o["x"][rows] = X.astype(np.float32)
            o["v"][rows] = V.astype(np.float32)
        if per_step is not None:
            per_step()
    return t


def _fluid(sc):
    return sc.arrays["material"] == 1


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def test_closed_form():
    """x, v of the body after step(20) against numpy f64 pose(20 dt) applied to x_0, per coordinate:
        |x - x_ref| <= 16 * 2^-24 * (|origin|_inf + |x_0 - pivot|_1)
        |v - v_ref| <= 16 * 2^-24 * (|u|_inf + |w| * |x_0 - pivot|_1)
    A rounding-analysis bound, not a measurement: the pose entries are rounded to f32 (half an ulp each: 2^-25 (|origin| +
    |q|_1)), q = x_0 - pivot is one rounding, r = R q three products and two sums (fused here: fewer roundings), x = origin + r
    one more: about 5 * 2^-24 of the bracket in the worst case, hence 16 with a margin of about 3.  The cross product adds
    two products and a sum on top of r's error, scaled by |w|.  dt = 2^-12 is a binary fraction, so the library's clock
    (f64 sums of the f32 dt) is exactly 20 dt."""
    dt = 2.0 ** -12
    sd = kin_scene(SWEEP, dt=dt)
    cfg, sc = scenes.build(sd)
    n_body = _check_shape(sc)
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    before = {f: scenes.ps_by_pid(ps, f) for f in ("m", "m_V", "material", "is_dynamic", "object_id", "color")}
    assert ps.time == 0.0
    solver.step(20)
    assert ps.time == 20 * dt                                # exact: see above
    body = sc.arrays["object_id"] == BODY
    m = sc.motions[BODY]
    x0 = sc.arrays["x_0"][body].astype(np.float64)
    X, V = _closed_form(m, 20 * dt, x0)
    R, c, u, w = motion.pose(m, 20 * dt)
    q1 = np.abs(x0 - m.pivot).sum(axis=1, keepdims=True)
    x, v = scenes.ps_by_pid(ps, "x")[body].astype(np.float64), scenes.ps_by_pid(ps, "v")[body].astype(np.float64)
    ex = np.abs(x - X) / (16 * EPS * (np.abs(c).max() + q1))
    ev = np.abs(v - V) / (16 * EPS * (np.abs(u).max() + np.linalg.norm(w) * q1))
    print(f"closed form, {n_body} particles: worst |x err| / bound = {ex.max():.3f}, worst |v err| / bound = {ev.max():.3f}")
    scenes.bound("kinematic", "closed_form:x/bound", float(ex.max()), 1.0)
    scenes.bound("kinematic", "closed_form:v/bound", float(ev.max()), 1.0)
    assert np.abs(X - x0).max() > 0.004 and np.abs(V).max() > 1.0, "the motion does not test anything"
    for f, a in before.items():                              # nothing but x and v of the body is written
        assert np.array_equal(scenes.ps_by_pid(ps, f)[body], a[body]), f
    assert np.array_equal(np.sort(ps.pid.to_numpy()), np.arange(sc.particle_max_num))
    ps.close()


# ---- 2, 3 ---------------------------------------------------------------------------------------------------------------
def test_parity_with_the_oracle_wcsph():
    """15 steps of the body sweeping into the fluid: fluid positions by pid within the project's parity bound (rel L2 <= 1e-4)
    of the oracle's, cell ids of the last step bit-equal."""
    sd = kin_scene(SWEEP)
    cfg, sc = scenes.build(sd)
    _check_shape(sc)
    o = scenes.make_oracle(cfg, sc)
    ps, solver = scenes.make_ps(sd)
    o.initialize(); solver.initialize()
    n = 15
    t = _drive_oracle(o, sc, sc.motions, n, _dt32(sd))
    solver.step(n)
    assert abs(ps.time - t) <= 1e-15
    fl = _fluid(sc)
    x, x_ref = scenes.ps_by_pid(ps, "x"), o.by_pid("x")
    err = scenes.rel_l2(x[fl], x_ref[fl])
    print(f"WCSPH with a kinematic body, {n} steps: fluid rel_l2(x) = {err:.3e}")
    scenes.bound("kinematic", "wcsph:fluid_rel_l2_x", err, 1e-4)
    assert np.array_equal(scenes.ps_by_pid(ps, "grid_ids"), o.by_pid("grid_ids")), "cell ids of the last step differ"
    # the body matters: the same steps without the motion leave the fluid elsewhere
    ps0, solver0 = scenes.make_ps(kin_scene(None))
    solver0.initialize(); solver0.step(n)
    assert scenes.rel_l2(scenes.ps_by_pid(ps0, "x")[fl], x_ref[fl]) > 10 * max(err, 1e-9), "the fluid never felt the moving body"
    ps0.close(); ps.close()


def test_parity_with_the_oracle_dfsph():
    """The same under DFSPH for 8 steps, stepping both sides one step at a time: both solvers' iteration counts equal the
    oracle's in every step (DFSPH reads the prescribed solid velocities wherever its kernels read v_j of solids)."""
    spec = dict(SWEEP, linearVelocity=[-0.5, 0.15, 0.05])
    sd = scenes.as_dfsph(kin_scene(spec))
    cfg, sc = scenes.build(sd)
    o = scenes.make_oracle(cfg, sc)
    ps, solver = scenes.make_ps(sd)
    o.initialize(); solver.initialize()
    its_ref, its = [], []
    n = 8
    _drive_oracle(o, sc, sc.motions, n, _dt32(sd), per_step=lambda: its_ref.append((o.s.last_iterations_v, o.s.last_iterations)))
    for _ in range(n):
        solver.step(1)
        st = solver.stats()
        its.append((st["iterations_v"], st["iterations"]))
    print(f"DFSPH iterations (divergence, pressure) per step: oracle {its_ref}, device {its}")
    fl = _fluid(sc)
    err = scenes.rel_l2(scenes.ps_by_pid(ps, "x")[fl], o.by_pid("x")[fl])
    print(f"DFSPH with a kinematic body, {n} steps: fluid rel_l2(x) = {err:.3e}")
    scenes.bound("kinematic", "dfsph:fluid_rel_l2_x", err, 1e-4)
    assert its == its_ref
    assert np.array_equal(scenes.ps_by_pid(ps, "grid_ids"), o.by_pid("grid_ids"))
    ps.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_coexistence_with_a_dynamic_body_and_a_static_block():
    """One kinematic body, one dynamic (shape-matched) body and a static block in one scene: the general sweep path with the
    dynamic list.  10 steps against the oracle at the same bounds; the static block does not move by a bit; the dynamic body
    stays within the rigid parity bound of test_gpu_parity.py (rel L2 <= 5e-5 over its particles)."""
    sd = scenes.fluid_only(counts=(14, 8, 12), start=(0.1, 0.1, 0.1), velocity=(0.0, -1.0, 0.0))
    spec = {"linearVelocity": [-2.0, 0.0, 0.2], "angularVelocity": [0.0, 1.5, 2.0]}
    sd["RigidBodies"] = [_body(1, (0.14, 0.26, 0.14), dynamic=True, density=600.0, velocity=(0.0, -2.0, 0.0)),
                         _body(2, (0.42, 0.12, 0.14), motion=spec)]
    start = (0.08, 0.05, 0.08)
    sd["RigidBlocks"] = [{"objectId": 3, "start": list(start), "end": scenes.lattice_end(start, (16, 2, 14)),
                          "translation": [0.0, 0.0, 0.0], "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "density": 1000.0,
                          "color": [255, 255, 255], "isDynamic": False}]
    cfg, sc = scenes.build(sd)
    assert sorted(sc.dynamic_rigid_ids) == [1] and list(sc.motions) == [2]
    o = scenes.make_oracle(cfg, sc, rigid_sums_f64=True)
    ps, solver = scenes.make_ps(sd)
    o.initialize(); solver.initialize()
    x_start = scenes.ps_by_pid(ps, "x")
    n = 10
    _drive_oracle(o, sc, sc.motions, n, _dt32(sd))
    solver.step(n)
    oid = sc.arrays["object_id"]
    x, x_ref = scenes.ps_by_pid(ps, "x"), o.by_pid("x")
    err = scenes.rel_l2(x[oid == 0], x_ref[oid == 0])
    err_dyn = scenes.rel_l2(x[oid == 1], x_ref[oid == 1])
    print(f"coexistence, {n} steps: fluid rel_l2(x) = {err:.3e}, dynamic body rel_l2(x) = {err_dyn:.3e}")
    scenes.bound("kinematic", "coexistence:fluid_rel_l2_x", err, 1e-4)
    scenes.bound("kinematic", "coexistence:dynamic_body_rel_l2_x", err_dyn, 5e-5)
    assert np.array_equal(x[oid == 3], x_start[oid == 3]), "the static block moved"
    assert np.array_equal(scenes.ps_by_pid(ps, "grid_ids"), o.by_pid("grid_ids"))
    X, _ = _closed_form(sc.motions[2], ps.time, sc.arrays["x_0"][oid == 2].astype(np.float64))
    assert np.abs(x[oid == 2] - X).max() <= 1e-6 and np.abs(X - x_start[oid == 2]).max() > 5e-3
    ps.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def _all_fields(ps):
    return {f: scenes.ps_by_pid(ps, f) for f in FIELDS}


def test_zero_motion_is_a_no_op():
    """An all-zero motion writes x = pivot + (x_0 - pivot) and v = 0 + 0.  The body lies inside [pivot / 2, 2 pivot] in every
    coordinate (asserted), so x_0 - pivot is exact (Sterbenz) and the sum gives x_0 back bit for bit: every field equals the
    run without a registration, and so does a run whose registration was cleared again."""
    sd = kin_scene(None)
    cfg, sc = scenes.build(sd)
    rest = sc.arrays["x_0"][sc.arrays["object_id"] == BODY].astype(np.float64)
    pivot = rest.mean(axis=0)
    assert np.all(rest >= pivot / 2) and np.all(rest <= 2 * pivot)
    runs = []
    for mode in ("plain", "zero", "cleared"):
        ps, solver = scenes.make_ps(sd)
        solver.initialize()
        if mode != "plain":
            ps.set_body_motion(BODY)                         # every key at its default: all zeros
        if mode == "cleared":
            ps.clear_body_motion(BODY)
        solver.step(10)
        runs.append(_all_fields(ps))
        ps.close()
    for f in FIELDS:
        assert np.array_equal(runs[0][f], runs[1][f]), f"zero motion changed {f}"
        assert np.array_equal(runs[0][f], runs[2][f]), f"a cleared motion changed {f}"


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_reproducible_and_independent_of_how_the_steps_are_split():
    sd = kin_scene(SWEEP)
    dt = _dt32(sd)
    runs = []
    for split in ((12,), (5, 7), (12,)):
        ps, solver = scenes.make_ps(sd)
        solver.initialize()
        for k in split:
            solver.step(k)
        runs.append(_all_fields(ps))
        t = 0.0
        for _ in range(12):
            t += dt
        assert ps.time == t
        ps.close()
    for f in FIELDS:
        assert np.array_equal(runs[0][f], runs[1][f]), f"step(12) and step(5); step(7) differ in {f}"
        assert np.array_equal(runs[0][f], runs[2][f]), f"two runs differ in {f}"
    # the clock follows a dt changed between two calls
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    solver.step(5)
    solver.dt[None] = 2.0 ** -13
    solver.step(7)
    t = 0.0
    for k in range(12):
        t += dt if k < 5 else 2.0 ** -13
    assert ps.time == t
    body = scenes.build(sd)[1].arrays["object_id"] == BODY
    cfg, sc = scenes.build(sd)
    X, _ = _closed_form(sc.motions[BODY], t, sc.arrays["x_0"][body].astype(np.float64))
    assert np.abs(scenes.ps_by_pid(ps, "x")[body] - X).max() <= 1e-6
    ps.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_restart_continues_the_motion_exactly(tmp_path):
    sd = kin_scene(SWEEP)
    ps, solver = scenes.make_ps(sd)
    solver.initialize(); solver.step(3)
    ck = str(tmp_path / "state.npz")
    ps.save_state(ck)
    t3 = ps.time
    solver.step(3)
    end, t6 = _all_fields(ps), ps.time
    ps.close()
    ps2, solver2 = scenes.make_ps(sd)
    solver2.initialize()
    ps2.load_state(ck)
    assert ps2.time == t3 and t3 > 0.0
    solver2.step(3)
    assert ps2.time == t6
    got = _all_fields(ps2)
    for f in FIELDS:
        assert np.array_equal(got[f], end[f]), f"the restarted run differs in {f}"
    ps2.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_stand_alone_pose_and_the_sweep_after_it():
    """set_body_pose with a quarter turn about z places the body as numpy says; the neighbour structure and a stand-alone
    compute_densities after it (the reference's order: positions changed, so initialize_particle_system() first) give the
    oracle's densities for those positions -- no list or partition of the steps before survives the pose."""
    sd = kin_scene(None)
    cfg, sc = scenes.build(sd)
    o = scenes.make_oracle(cfg, sc)
    ps, solver = scenes.make_ps(sd)
    o.initialize(); solver.initialize()
    o.step(3); solver.step(3)                                # lists, partition and staging records of a step are in place
    body = sc.arrays["object_id"] == BODY
    x0 = sc.arrays["x_0"][body].astype(np.float64)
    pivot = x0.mean(axis=0).astype(np.float32).astype(np.float64)
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    origin = pivot + np.array([-0.01, 0.01, 0.0])           # towards the fluid: the body's neighbourhoods change
    lin, ang = np.array([0.5, 0.0, -0.25]), np.array([0.0, 0.0, 2.0])
    ps.set_body_pose(BODY, R, origin, lin_vel=lin, ang_vel=ang)
    X, V = motion.apply_pose(R, origin.astype(np.float32).astype(np.float64), lin, ang, pivot, x0)
    x, v = scenes.ps_by_pid(ps, "x"), scenes.ps_by_pid(ps, "v")
    q1 = np.abs(x0 - pivot).sum(axis=1, keepdims=True)
    assert np.all(np.abs(x[body] - X) <= 16 * EPS * (np.abs(origin).max() + q1))
    assert np.all(np.abs(v[body] - V) <= 16 * EPS * (np.abs(lin).max() + np.linalg.norm(ang) * q1))
    # a quarter turn: (qx, qy, qz) -> (-qy, qx, qz)
    assert np.allclose(x[body] - origin, np.stack([-(x0 - pivot)[:, 1], (x0 - pivot)[:, 0], (x0 - pivot)[:, 2]], axis=1), atol=1e-6)
    rows = np.nonzero(o["object_id"] == BODY)[0]
    o["x"][rows] = x[o["pid"][rows]]
    o["v"][rows] = v[o["pid"][rows]]
    o.initialize_particle_system(); o.compute_densities()
    ps.initialize_particle_system(); solver.compute_densities()
    fl = _fluid(sc)
    rho, rho_ref = scenes.ps_by_pid(ps, "density"), o.by_pid("density")
    err = float(np.abs(rho[fl] - rho_ref[fl]).max() / np.abs(rho_ref[fl]).max())
    print(f"densities after a stand-alone pose: max err / max ref = {err:.3e}")
    scenes.bound("kinematic", "stand_alone:density", err, 3e-6)      # the density tolerance of test_gpu_parity.py (F_TOL)
    ps.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def _motion_struct(oid, **kw):
    s = motion.to_struct(oid, motion.parse_motion({"pivot": [0.37, 0.19, 0.17]}))
    for k, val in kw.items():
        setattr(s, k, val)
    return s


def test_refusals():
    import ctypes as C
    sd = scenes.fluid_only(counts=(10, 10, 8), start=(0.1, 0.1, 0.1), velocity=(0.0, -1.0, 0.0))
    sd["RigidBodies"] = [_body(1, (0.32, 0.14, 0.12)), _body(2, (0.5, 0.3, 0.3), dynamic=True, density=800.0)]
    cfg, sc = scenes.build(sd)
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    solver.step(2)
    lib, ctx = ps._lib, ps._ctx
    INVALID = -1

    def kin_set(structs, n=None):
        arr = (_lib.SphKinematicMotion * max(len(structs), 1))(*structs)
        return lib.sph_kinematic_set(ctx, arr, len(structs) if n is None else n)

    x_before = scenes.ps_by_pid(ps, "x")
    assert kin_set([_motion_struct(2)]) == INVALID and b"dynamic" in lib.sph_last_error(ctx)     # a dynamic body
    with pytest.raises(ValueError, match="isDynamic"):
        ps.set_body_motion(2, linearVelocity=[1, 0, 0])
    assert kin_set([_motion_struct(0)]) == INVALID                                                 # the fluid
    assert kin_set([_motion_struct(7)]) == INVALID and kin_set([_motion_struct(-1)]) == INVALID    # unknown ids
    assert kin_set([_motion_struct(1)] * 9) == INVALID                                             # nine objects
    assert kin_set([_motion_struct(1), _motion_struct(1)]) == INVALID                              # one id twice
    assert kin_set([_motion_struct(1, osc_phase=float("nan"))]) == INVALID                         # NaN fields
    assert kin_set([_motion_struct(1, lin_vel=(C.c_double * 3)(0.0, float("inf"), 0.0))]) == INVALID
    assert kin_set([_motion_struct(1, start_time=2.0, end_time=1.0)]) == INVALID
    pivot = sc.arrays["x_0"][sc.arrays["object_id"] == 1].astype(np.float64).mean(axis=0)
    with pytest.raises(_lib.SphError, match="orthonormal"):
        ps.set_body_pose(1, np.eye(3) * 1.01, pivot)
    with pytest.raises(_lib.SphError, match="orthonormal"):
        ps.set_body_pose(1, [[1, 0.01, 0], [0, 1, 0], [0, 0, 1]], pivot)
    with pytest.raises(_lib.SphError, match="reflection"):
        ps.set_body_pose(1, np.diag([1.0, 1.0, -1.0]), pivot)
    with pytest.raises(_lib.SphError, match="non-finite"):
        ps.set_body_pose(1, np.eye(3), [float("nan"), 0.2, 0.2])
    with pytest.raises(_lib.SphError, match="dynamic"):
        ps.set_body_pose(2, np.eye(3), [0.5, 0.3, 0.3])
    with pytest.raises(_lib.SphError, match="leave"):
        ps.set_body_pose(1, np.eye(3), [0.05, 0.19, 0.17])                                         # into the wall padding
    assert np.array_equal(scenes.ps_by_pid(ps, "x"), x_before), "a refused call moved something"

    # containment: the body's low x face is 0.32 - 0.04 = 0.28 from the padding plane; at -30 m/s it gets there in
    # 0.28 / (30 * 0.0004) = 23.3 steps, so a call of 30 steps enqueues 23 and refuses the rest
    t0 = ps.time
    ps.set_body_motion(1, linearVelocity=[-30.0, 0.0, 0.0], startTime=t0)
    dyn, n_dyn = solver._dynamic_ids()
    rc = lib.sph_step(ctx, 30, dyn, n_dyn)
    msg = lib.sph_last_error(ctx).decode()
    assert rc == INVALID and "object 1" in msg and "step 23" in msg, msg
    assert abs(ps.time - (t0 + 23 * _dt32(sd))) <= 1e-12
    x = scenes.ps_by_pid(ps, "x")
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(scenes.ps_by_pid(ps, "v")))
    g = sc.geom
    assert np.all(x >= np.float32(g.padding)) and np.all(x <= np.asarray(g.domain_size, dtype=np.float64) - g.padding + 1e-6)
    with pytest.raises(_lib.SphError, match="object 1"):
        solver.step(1)                                       # still refused: nothing is enqueued, the clock stands
    assert abs(ps.time - (t0 + 23 * _dt32(sd))) <= 1e-12
    ps.clear_body_motion(1)
    solver.step(2)                                           # a valid step works again
    x2 = scenes.ps_by_pid(ps, "x")
    body = sc.arrays["object_id"] == 1
    assert np.abs(x2[body] - x[body]).max() <= 1e-6 and np.all(np.isfinite(x2))      # frozen where the last enqueued step left it ...
    assert not scenes.ps_by_pid(ps, "v")[body].any()                                  # ... and at rest
    ps.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_frames_follow_the_motion():
    from sph_taichi_amd.render import Camera
    sd = kin_scene(None)
    cfg, sc = scenes.build(sd)
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    pivot = sc.arrays["x_0"][sc.arrays["object_id"] == BODY].astype(np.float64).mean(axis=0)
    cam = Camera(eye=(float(pivot[0]), float(pivot[1]), 1.5), lookat=(float(pivot[0]), float(pivot[1]), 0.0), draw_box=False)
    img0 = ps.render(camera=cam, size=(64, 64))
    d0 = ps.render_depth()
    ps.set_body_pose(BODY, np.eye(3), pivot + np.array([0.0, 0.0, 0.2]))     # 0.2 towards the camera
    img1 = ps.render(camera=cam, size=(64, 64))
    d1 = ps.render_depth()
    assert not np.array_equal(img0, img1)
    c0, c1 = float(d0[32, 32]), float(d1[32, 32])
    assert math.isfinite(c0) and math.isfinite(c1)
    # the image centre shows the body's front face, 0.2 nearer; the pixel's ray meets a sphere of the front layer somewhere on its
    # near half, whose depth spans one particle radius, and not at the same spot in both frames (perspective)
    assert abs((c0 - c1) - 0.2) <= ps.particle_radius, (c0, c1)
    ps.close()
