"""GPU parity AWAY from the one parameter point of scenes.BASE_CFG (tests/param_points.py lists the points).

Per kernel the criterion is an f64 reference of the same operation (oracle/brute.py, dtype=float64): with
    E_hip = max |hip - f64| / max |f64|,    E_ref = max |oracle_f32 - f64| / max |f64|
a stage passes when E_hip <= 3 * E_ref + 4 * eps_f32.  Both sides are f32 evaluations of the same formulas on identical
f32 inputs; summation order, fma contraction and reciprocal forms move the error by a small factor, and the factor 3 (the
project's standing margin) is applied to the REFERENCE's own error, never to a number read off the GPU.  Trajectories are
held to the oracle at the north star (1e-4 relative L2 on x) on scenes that tests/test_params_host.py has shown to be
deterministic to 3e-5 under the reference alone."""
import numpy as np
import pytest

import param_points as pp
import scenes
from oracle.brute import Brute

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
FIELDS = ("m_V", "density", "pressure", "acceleration", "v", "x")
STAGES = ("compute_moving_boundary_volume", "compute_densities", "compute_non_pressure_forces", "compute_pressure_forces",
          "advect", "enforce_boundary_3D")


def _err(got, ref64):
    return float(np.abs(np.asarray(got, np.float64) - ref64).max()) / max(float(np.abs(ref64).max()), 1e-300)


def _hold(key, hip, ora, ref64):
    """The 3 x E_ref rule.  The pair goes to the evidence file ($SPH_TEST_EVIDENCE_DIR/param_parity.json, kept as
    profiles/param_parity_errors.json) as one entry: measured = E_hip, bound = 3 E_ref + 4 eps_f32, so E_ref = (bound - 4 eps_f32) / 3."""
    e_hip, e_ref = _err(hip, ref64), _err(ora, ref64)
    if e_hip == 0.0 and e_ref == 0.0:      # a field the stage does not touch
        return
    print(f"{key}: E_hip {e_hip:.3e} E_ref {e_ref:.3e}")
    scenes.bound("param_parity", key, e_hip, 3.0 * e_ref + 4.0 * EPS)


_REF = {}      # point -> the oracle / f64 brute-force pipeline of the kernel scene, run once and left unchanged


def _reference(name):
    """Stage by stage: the f32 state every side starts the stage from (the oracle's), the oracle's f32 result and the f64 one.
    Everything is in the oracle's order after its first sort, which is the HIP side's order too (asserted by the caller)."""
    if name in _REF:
        return _REF[name]
    sd, cfg, sc = pp.build_coupled(name)
    prm = pp.params(cfg, sc, name)
    o = pp.make_oracle(cfg, sc, name)
    o.update_grid_id()
    ids = {"grid_ids_hash": o["grid_ids"].copy()}
    o.prefix_sum()
    ids["grid_particles_num"] = o["grid_particles_num"].copy()
    o.counting_sort()
    ids["grid_ids"], ids["pid"] = o["grid_ids"].copy(), o["pid"].copy()
    start = {k: o[k].copy() for k in sc.arrays if k != "pid"}
    o = pp.make_oracle(cfg, sc, name)
    o.initialize()
    assert np.array_equal(o["pid"], ids["pid"])
    b = Brute(prm, start, dtype=np.float64)
    b.boundary_volume(False); b.boundary_volume(True)
    out = {"sd": sd, "cfg": cfg, "sc": sc, "ids": ids, "m_V_init": (o["m_V"].copy(), b.a["m_V"].copy()), "stages": []}
    for stage in STAGES:
        state = {f: o[f].copy() for f in FIELDS}
        for f in FIELDS:
            b.set(f, state[f])
        if stage == "compute_moving_boundary_volume":
            o.compute_moving_boundary_volume(); b.boundary_volume(True)
        elif stage == "enforce_boundary_3D":
            o.enforce_boundary_3D(1); b.enforce_boundary_3D(1)
        else:
            getattr(o, stage)(); getattr(b, stage)()
        out["stages"].append((stage, state, {f: o[f].copy() for f in FIELDS}, {f: b.a[f].copy() for f in FIELDS}))
    # One step carries nobody to a wall, so padding and wall_hi (folded from the radius) would go uncompared: the wall pass once
    # more, from the same state with 14 fluid particles put beyond faces, edges and a corner, moving outwards.
    state = {f: o[f].copy() for f in FIELDS}
    g = sc.geom
    lo, hi = g.padding - 0.3 * g.particle_diameter, np.asarray(g.domain_size) - g.padding + 0.3 * g.particle_diameter
    idx = np.nonzero(o["material"] == 1)[0][:14]
    for k, i in enumerate(idx):
        for ax in range(3):
            side = (k // 3 ** ax) % 3          # 0 inside, 1 below the low face, 2 above the high face
            if k == 13:
                side = 1 + ax % 2
            if side:
                state["x"][i, ax] = lo if side == 1 else hi[ax]
                state["v"][i, ax] = -1.5 - 0.1 * k if side == 1 else 1.5 + 0.1 * k
    for f in FIELDS:
        o[f][:] = state[f]
        b.set(f, state[f])
    o.enforce_boundary_3D(1); b.enforce_boundary_3D(1)
    assert not np.array_equal(o["x"], state["x"]) and not np.array_equal(o["v"], state["v"])
    out["stages"].append(("enforce_boundary_3D walls", state, {f: o[f].copy() for f in FIELDS}, {f: b.a[f].copy() for f in FIELDS}))
    _REF[name] = out
    return out


def _upload(ps, state):
    """The stage's f32 start state.  x is uploaded only where it differs: until the advect it is bit for bit what the sort
    left, and the neighbour structure of the step describes exactly those positions."""
    for f in FIELDS:
        if f == "x" and np.array_equal(ps.x.to_numpy(), state[f]):
            continue
        getattr(ps, f).from_numpy(state[f])


@pytest.mark.parametrize("impl", [1, 0])
@pytest.mark.parametrize("name", pp.NAMES)
def test_kernel_by_kernel(name, impl):
    ref = _reference(name)
    sc, ids = ref["sc"], ref["ids"]
    ps, solver = pp.make_ps(ref["sd"], sc.arrays, name, gather_impl=impl)
    if name in pp.RADIUS_POINTS:          # the folded grid constants: hash, histogram scan and stable order, bit for bit
        ps.update_grid_id()
        assert np.array_equal(ps.grid_ids.to_numpy(), ids["grid_ids_hash"])
        ps.prefix_sum()
        assert np.array_equal(ps.grid_particles_num.to_numpy(), ids["grid_particles_num"])
        ps.counting_sort()
        assert np.array_equal(ps.grid_ids.to_numpy(), ids["grid_ids"]) and np.array_equal(ps.pid.to_numpy(), ids["pid"])
    solver.initialize()
    assert np.array_equal(ps.pid.to_numpy(), ids["pid"])
    _hold(f"{name} impl={impl} initialize:m_V", ps.m_V.to_numpy(), *ref["m_V_init"])
    for stage, state, ora, f64 in ref["stages"]:
        _upload(ps, state)
        if stage.startswith("enforce_boundary_3D"):
            solver.enforce_boundary_3D(1)
        else:
            getattr(solver, stage)()
        for f in FIELDS:
            _hold(f"{name} impl={impl} {stage}:{f}", getattr(ps, f).to_numpy(), ora[f], f64[f])
    ps.close()


@pytest.mark.parametrize("name", pp.EXP_POINTS)
def test_fused_eos_against_stand_alone_eos(name):
    """The Tait pressure of the fused density + EOS sweep (one step() call, SPH_OPT_FUSED_STEP 1: sph_tait_pow<true>) and of
    the stand-alone compute_densities + compute_pressure_forces (k_eos: sph_tait_pow<false>).  Integer exponents up to 32
    take the multiply loop in both; every other exponent takes exp2(e * log2 x) on the hardware transcendentals in the
    fused sweep and powf in the stand-alone kernel.  Each is judged ON THE SAME STATE: the f32 density the HIP run itself
    holds goes through the f64 EOS and through the oracle's f32 EOS, so the density sweep's own error (amplified by
    stiffness * exponent) is on no side and what is left is the power alone."""
    ref = _reference(name)
    sd, cfg, sc = ref["sd"], ref["cfg"], ref["sc"]
    o = pp.make_oracle(cfg, sc, name)
    o.initialize()
    b = Brute(pp.params(cfg, sc, name), {k: o[k].copy() for k in sc.arrays if k != "pid"}, dtype=np.float64)
    order = o["pid"].copy()
    got = {}
    ps, solver = pp.make_ps(sd, sc.arrays, name, fused=0)
    solver.initialize()
    assert np.array_equal(ps.pid.to_numpy(), order)
    solver.compute_moving_boundary_volume(); solver.compute_densities(); solver.compute_pressure_forces()
    got["stand-alone"] = (ps.density.to_numpy(), ps.pressure.to_numpy())
    ps.close()
    ps, solver = pp.make_ps(sd, sc.arrays, name, fused=1)
    solver.initialize()
    solver.step(1)
    got["fused"] = (scenes.ps_by_pid(ps, "density")[order], scenes.ps_by_pid(ps, "pressure")[order])   # the oracle's order
    ps.close()
    fluid = o["material"] == 1
    rho0 = np.float32(cfg.get_cfg("density0"))
    for form, (rho, p) in got.items():
        assert (rho[fluid] >= rho0).all() and (rho[fluid] / rho0).max() >= 1.005, "the density after the EOS is the clamped one"
        b.set("density", rho); b.eos()
        o["density"][:] = rho
        o.compute_pressure_forces()
        assert b.a["pressure"].max() > 0
        _hold(f"{name} {form} EOS:pressure", p, o["pressure"], b.a["pressure"])
    # the two densities are the same sum in the same order: the two forms were compared on (all but) the same numbers
    assert np.abs(got["fused"][0] - got["stand-alone"][0]).max() <= 4 * EPS * float(rho0) * 1.3


def _variants(name):
    v = [(1, 1, 0), (0, 0, 0)]          # (gather_impl, fused, brick_shape)
    return v + [(1, 1, 1)] if name in pp.RADIUS_POINTS else v


_TRAJ = {}


def _traj_reference(name):
    if name not in _TRAJ:
        sd, cfg, sc = pp.build_traj(name)
        o = pp.make_oracle(cfg, sc, name)
        o.initialize()
        o.step(pp.traj_steps(name))
        _TRAJ[name] = (sd, sc, o.by_pid("x"), o.by_pid("v"))
    return _TRAJ[name]


@pytest.mark.parametrize("name,impl,fused,shape", [(n,) + v for n in pp.NAMES for v in _variants(n)])
def test_trajectory(name, impl, fused, shape):
    sd, sc, x_ref, v_ref = _traj_reference(name)
    ps, solver = pp.make_ps(sd, sc.arrays, name, gather_impl=impl, fused=fused, brick_shape=shape)
    solver.initialize()
    n = pp.traj_steps(name)
    solver.step(n)
    ex = scenes.rel_l2(scenes.ps_by_pid(ps, "x"), x_ref)
    ev = scenes.rel_l2(scenes.ps_by_pid(ps, "v"), v_ref)
    print(f"{name} impl={impl} fused={fused} shape={shape}: x {ex:.3e} v {ev:.3e}")
    assert ex <= 1e-4, f"rel L2 position error after {n} steps = {ex:.3e}"
    assert ev <= 2e-3, f"rel L2 velocity error after {n} steps = {ev:.3e}"
    assert np.all(np.diff(ps.grid_ids.to_numpy()) >= 0)
    ps.close()


@pytest.mark.parametrize("name", pp.BODY_POINTS)
def test_shape_matched_bodies(name, tmp_path):
    """Two voxelised cubes of side 10 r dropping into a fluid block, at the other radii and mass scales: rigid_fx_exp
    (sph_api.hip::refresh_dyn) comes from the dynamic-particle count, m_V0 * rho_max and the domain extent.  An overflowing
    or too coarse fixed-point scale shows as a body leaving the oracle's path; the sums stay exact integers, so two runs,
    and the batched and the body-by-body solve, agree bit for bit."""
    from sph_taichi_amd import _lib
    sd, cfg, sc = pp.build_bodies(name, str(tmp_path / "cube.obj"))
    a = sc.arrays
    o = pp.make_oracle(cfg, sc, name, rigid_sums_f64=True)
    o.initialize()
    runs = []
    for batch in (1, 1, 0):
        ps, solver = pp.make_ps(sd, a, name)
        ps.set_option(_lib.OPT_RIGID_BATCH, batch)
        solver.initialize()
        if not runs:
            assert np.array_equal(ps.pid.to_numpy(), o["pid"])
            R = solver.solve_constraints(1)
            assert np.allclose(R, o.solve_constraints(1), rtol=0.0, atol=2e-6)
        else:
            solver.solve_constraints(1)
        solver.step(20)
        runs.append((scenes.ps_by_pid(ps, "x"), scenes.ps_by_pid(ps, "v")))
        if len(runs) == 1:
            R_end = solver.solve_constraints(1)      # the rotation the body has taken in the fluid
        ps.close()
    o.step(20)
    # ... against the oracle's: R is the polar factor of A = sum m (x - cm) q^T, so positions that differ by dx move it by
    # about dx / (rms distance from the centre) -- the 2e-6 of the rest pose plus twice that for the positions as they are
    body = a["object_id"] == 1
    dx = float(np.abs(runs[0][0][body].astype(np.float64) - o.by_pid("x")[body]).max())
    q = a["x_0"][body].astype(np.float64)
    r_rms = float(np.sqrt(((q - q.mean(axis=0)) ** 2).sum(axis=1).mean()))
    R_ref = o.solve_constraints(1)
    assert np.abs(R_ref - np.eye(3)).max() > 1e-4, "body 1 has not turned: the comparison says nothing about the sums"
    assert np.allclose(R_end, R_ref, rtol=0.0, atol=2e-6 + 2.0 * dx / r_rms), (np.abs(R_end - R_ref).max(), dx / r_rms)
    rigid = (a["material"] == 0) & (a["is_dynamic"] == 1)
    err = scenes.rel_l2(runs[0][0][rigid], o.by_pid("x")[rigid])
    print(f"{name}: rigid x {err:.3e}  all x {scenes.rel_l2(runs[0][0], o.by_pid('x')):.3e}")
    assert err <= 1e-4
    assert scenes.rel_l2(runs[0][0], o.by_pid("x")) <= 1e-4
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "two runs differ"
    assert np.array_equal(runs[0][0], runs[2][0]) and np.array_equal(runs[0][1], runs[2][1]), "batched != body by body"


def test_attributes_changed_between_two_step_calls():
    """viscosity, surface_tension, g, exponent and stiffness are plain solver attributes that _push() sends before every
    step() call: changed after five steps, the next five follow the oracle that got the same change at the same step."""
    sd, cfg, sc = pp.build_traj(None)
    o = pp.make_oracle(cfg, sc)
    o.initialize(); o.step(5)
    o.set_solver_attrs(**pp.IN_FLIGHT)
    o.step(5)
    res = {}
    for change in (True, False):
        ps, solver = pp.make_ps(sd, sc.arrays)
        solver.initialize()
        solver.step(5)
        if change:
            for k, v in pp.IN_FLIGHT.items():
                setattr(solver, k, np.array(v) if k == "g" else v)
        solver.step(5)
        res[change] = scenes.ps_by_pid(ps, "x")
        ps.close()
    err = scenes.rel_l2(res[True], o.by_pid("x"))
    print(f"in flight: x {err:.3e}; against the unchanged run {scenes.rel_l2(res[True], res[False]):.3e}")
    assert err <= 1e-4
    assert scenes.rel_l2(res[True], res[False]) > 1e-4, "the second block equals a run without the change: the push never arrived"


# ---- DFSPH (simulationMethod 4) at r_large, r_small, rho_heavy, g_oblique, visc_hi ------------------------------------------
def _fluid_hold(key, fluid, hip, ora, ref64):
    _hold(key, hip[fluid], ora[fluid], ref64[fluid])


@pytest.mark.parametrize("impl", [1, 0])
@pytest.mark.parametrize("name", pp.DFSPH_POINTS)
def test_dfsph_kernel_by_kernel(name, impl):
    """The stage list of test_gpu_parity.test_dfsph_kernel_by_kernel one step into the point's scene.  Both sides start from
    the oracle's f32 state (uploaded before the sort, so every cached structure is built from it): the density, factor and
    density-change sweeps then run on identical inputs and are held to Brute(float64) by the 3 x E_ref rule, as is the
    density advection after its inputs (v, density) are uploaded again; the solver loops and the stages between follow the
    oracle within DF_TOL."""
    from test_gpu_parity import DF_TOL
    sd, cfg, sc = pp.build_dfsph(name)
    o = pp.make_oracle(cfg, sc, name)
    ps, solver = pp.make_ps(sd, sc.arrays, name, gather_impl=impl)
    o.initialize(); solver.initialize()
    o.step(1); solver.step(1)
    assert np.array_equal(ps.pid.to_numpy(), o["pid"])
    for f in ("x", "v", "m_V", "density", "acceleration"):
        getattr(ps, f).from_numpy(o[f])
    o.initialize_particle_system(); ps.initialize_particle_system()
    assert np.array_equal(ps.pid.to_numpy(), o["pid"]) and np.array_equal(ps.grid_ids.to_numpy(), o["grid_ids"])
    o.compute_moving_boundary_volume(); solver.compute_moving_boundary_volume()
    ps.m_V.from_numpy(o["m_V"])
    b = Brute(pp.params(cfg, sc, name), {k: o[k].copy() for k in sc.arrays if k != "pid"}, dtype=np.float64)
    fluid = o["material"] == 1
    key = f"dfsph {name} impl={impl} "
    o.compute_densities(); solver.compute_densities(); b.compute_densities()
    _hold(key + "compute_densities:density", ps.density.to_numpy(), o["density"], b.a["density"])
    o.compute_DFSPH_factor(); solver.compute_DFSPH_factor()
    _fluid_hold(key + "compute_DFSPH_factor:dfsph_factor", fluid, ps.dfsph_factor.to_numpy(), o["dfsph_factor"], b.dfsph_factor())
    o.compute_density_change(); solver.compute_density_change()
    ref = b.dfsph_density_change()
    assert (ref[fluid] > 0).any() and (ref[fluid] == 0).any(), "both sides of the neighbour-count switch must occur"
    _fluid_hold(key + "compute_density_change:density_adv", fluid, ps.density_adv.to_numpy(), o["density_adv"], ref)

    def follow(stage, fields):
        for f in fields:
            got, want = getattr(ps, f).to_numpy(), o[f]
            if f in ("dfsph_factor", "density_adv"):
                got, want = got[fluid], want[fluid]
            err = float(np.abs(got.astype(np.float64) - want).max()) / max(float(np.abs(want).max()), 1e-30)
            scenes.bound("param_parity", key + f"{stage}:{f} (vs oracle)", err, DF_TOL[f])

    r = o.divergence_solve(); solver.divergence_solve()
    follow("divergence_solve", ("v", "density_adv", "dfsph_factor"))
    assert solver.stats()["iterations_v"] == r
    o.compute_non_pressure_forces(); solver.compute_non_pressure_forces()
    follow("compute_non_pressure_forces", ("acceleration",))
    o.predict_velocity(); solver.predict_velocity()
    follow("predict_velocity", ("v",))
    ps.v.from_numpy(o["v"]); ps.density.from_numpy(o["density"])
    b.set("v", o["v"]); b.set("density", o["density"])
    o.compute_density_adv(); solver.compute_density_adv()
    _fluid_hold(key + "compute_density_adv:density_adv", fluid, ps.density_adv.to_numpy(), o["density_adv"], b.dfsph_density_adv())
    r = o.pressure_solve(); solver.pressure_solve()
    follow("pressure_solve", ("v", "density_adv", "acceleration"))
    assert solver.stats()["iterations"] == r
    o.dfsph_advect(); solver.advect()
    follow("dfsph_advect", ("x", "v"))
    ps.close()


@pytest.mark.parametrize("impl", [1, 0])
@pytest.mark.parametrize("name", pp.DFSPH_POINTS)
def test_dfsph_trajectory(name, impl):
    sd, cfg, sc = pp.build_dfsph(name)
    o = pp.make_oracle(cfg, sc, name)
    ps, solver = pp.make_ps(sd, sc.arrays, name, gather_impl=impl)
    o.initialize(); solver.initialize()
    n = pp.dfsph_steps(name)
    its = []
    for _ in range(n):
        o.step(1)
        its.append((o.s.last_iterations_v, o.s.last_iterations))
    solver.step(n)
    err = scenes.rel_l2(scenes.ps_by_pid(ps, "x"), o.by_pid("x"))
    print(f"dfsph {name} impl={impl}: x {err:.3e} iterations {its}")
    assert err <= 1e-4, f"rel L2 position error after {n} DFSPH steps = {err:.3e}"
    st = solver.stats()
    assert st["steps"] == n
    assert abs(st["total_iterations_v"] - sum(a + 1 for a, _ in its)) <= 1
    assert abs(st["total_iterations"] - sum(b + 1 for _, b in its)) <= 1
    assert sum(a for a, _ in its) > 0, "the divergence solver never iterated: the scene does not test it"
    ps.close()
