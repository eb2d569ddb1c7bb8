"""CPU preconditions of tests/test_gpu_params.py: at every parameter point of tests/param_points.py the references agree with
each other, the scenes have work for every kernel, and the f32 reference alone is deterministic enough over the
trajectory scenes for the 1e-4 bound of the GPU tests to mean something."""
import numpy as np
import pytest

import param_points as pp
import scenes
from oracle.brute import Brute

FIELDS = ["m_V", "density", "pressure", "acceleration", "v", "x"]
NOISE_CAP = 3e-5      # relative L2 on x of the perturbed oracle against the unperturbed one: a third of the GPU tests' 1e-4


def test_points_are_the_listed_departures_from_the_base_point():
    base = scenes.BASE_CFG
    changed = {n: {k for k, v in pp.point_cfg(n).items() if v != base[k]} for n in pp.NAMES}
    assert changed["r_large"] == {"particleRadius"} and changed["r_small"] == {"particleRadius", "domainEnd"}
    assert changed["exp_7p5"] == {"exponent"} and changed["stiff_hi"] == {"stiffness", "timeStepSize"}
    assert changed["visc_0"] == set() and pp.attrs("visc_0") == {"viscosity": 0.0}
    for n in pp.EXP_POINTS:
        c = pp.point_cfg(n)
        assert c["stiffness"] * c["exponent"] <= 3.5e5 or n == "exp_7p5", n
    for n, dims in (("r_large", (10, 12, 8)), ("r_small", (19, 16, 13))):
        _, _, sc = pp.build_coupled(n)
        assert tuple(int(v) for v in sc.geom.grid_num) == dims, n


@pytest.mark.parametrize("name", pp.NAMES)
def test_kernel_scene_references_agree_and_have_work(name):
    """(a) the C oracle against Brute(float32), kernel by kernel, as tightly as test_oracle_vs_brute.py asks at the default
    point; (b) compressed fluid inside the support of the static slab and of the dynamic block; Brute(float64) sits within
    the same distance of both (it is the same operation)."""
    sd, cfg, sc = pp.build_coupled(name)
    a = sc.arrays
    n = a["x"].shape[0]
    assert n <= 1500
    g = sc.geom
    assert (a["x"] < np.asarray(g.domain_size) - g.grid_size).all() and (a["x"] > g.padding).all(), "a cell inside every face"
    prm = pp.params(cfg, sc, name)
    o = pp.make_oracle(cfg, sc, name)
    b = Brute(prm, a)
    b64 = Brute(prm, a, dtype=np.float64)
    o.initialize()
    for bb in (b, b64):
        bb.boundary_volume(False); bb.boundary_volume(True)
    assert np.allclose(o.by_pid("m_V"), b.a["m_V"], rtol=2e-5)
    assert np.allclose(b64.a["m_V"], b.a["m_V"], rtol=2e-5)
    rho0 = float(cfg.get_cfg("density0"))
    for stage in ("compute_densities", "compute_non_pressure_forces", "compute_pressure_forces", "advect"):
        getattr(o, stage)(); getattr(b, stage)(); getattr(b64, stage)()
        for f in FIELDS:
            ref, got = b.a[f], o.by_pid(f)
            assert np.abs(got - ref).max() <= 2e-4 * max(np.abs(ref).max(), 1e-30), (stage, f)
            assert np.abs(b64.a[f] - ref).max() <= 2e-4 * max(np.abs(ref).max(), 1e-30), (stage, f, "f64")
        if stage == "compute_densities":
            fluid = a["material"] == 1
            dense = fluid & (b.a["density"] > rho0)
            assert dense.any(), "no fluid above density0: the pressure would be zero"
            if name in pp.EXP_POINTS:
                assert (b.a["density"][fluid] / np.float32(rho0)).max() >= 1.005
            x = a["x"].astype(np.float64)
            for solid in ((a["material"] == 0) & (a["is_dynamic"] == 0), (a["material"] == 0) & (a["is_dynamic"] == 1)):
                dist = np.linalg.norm(x[dense][:, None, :] - x[solid][None, :, :], axis=2)
                assert (dist < 0.98 * g.support_radius).any(), "no compressed fluid inside a solid's support"
        if stage == "compute_non_pressure_forces":
            # the viscous term has work: the same sweep without viscosity differs by more than g -- unless the point switches it off
            b0 = Brute(dict(prm, viscosity=0.0), a, dtype=np.float64)
            for f in ("m_V", "density"):
                b0.a[f] = b64.a[f].copy()
            b0.compute_non_pressure_forces()
            visc = float(np.abs(b64.a["acceleration"] - b0.a["acceleration"]).max())
            assert (visc == 0.0) if prm.get("viscosity", 0.01) == 0.0 else (visc > 9.81), f"viscous acceleration {visc:.3e}"
    dyn = (a["material"] == 0) & (a["is_dynamic"] == 1)
    grav = np.asarray(cfg.get_cfg("gravitation"), np.float32)
    assert np.abs(b.a["acceleration"][dyn] - grav).max() > 1e-3 * max(1.0, float(np.abs(grav).max())), \
        "scene must exercise the two-way coupling scatter"
    assert b.a["pressure"].max() > 0


def _noise(build, name, steps, **okw):
    sd, cfg, sc = build()
    assert sc.arrays["x"].shape[0] <= 2500 and steps <= 20
    out = {}
    for perturb in (0, 1, 3) if pp.integer_exponent(name) else (0, 1):
        o = pp.make_oracle(cfg, sc, name, perturb=perturb, **okw)
        o.initialize()
        o.step(steps)
        out[perturb] = o.by_pid("x")
        assert np.isfinite(out[perturb]).all()
    for perturb in out:
        if perturb:
            err = scenes.rel_l2(out[perturb], out[0])
            assert err <= NOISE_CAP, f"{name}: perturb={perturb}: the reference alone moves by {err:.2e} over {steps} steps"


@pytest.mark.parametrize("name", pp.NAMES)
def test_trajectory_scene_is_tame(name):
    """(c) reversed neighbour traversal (and, for integer exponents, the Tait power by multiplication) against the oracle as
    it stands: a scene on which ulp-level changes of the reference grow past 3e-5 cannot hold a kernel to 1e-4."""
    _noise(lambda: pp.build_traj(name), name, pp.traj_steps(name))


@pytest.mark.parametrize("name", pp.BODY_POINTS)
def test_body_scene_is_tame(name, tmp_path):
    build = lambda: pp.build_bodies(name, str(tmp_path / "cube.obj"))
    _noise(build, name, 20, rigid_sums_f64=True)
    sd, cfg, sc = build()
    assert sorted(sc.dynamic_rigid_ids) == [1, 2]
    o = pp.make_oracle(cfg, sc, name, rigid_sums_f64=True)
    o.initialize(); o.step(20)
    v = o.by_pid("v")
    dt, gy = cfg.get_cfg("timeStepSize"), cfg.get_cfg("gravitation")[1]
    vy = [float(v[sc.arrays["object_id"] == i, 1].mean()) for i in (1, 2)]
    assert max(abs(w - (-2.0 + gy * 20 * dt)) for w in vy) > 0.02, "no body felt the fluid"


@pytest.mark.parametrize("name", pp.DFSPH_POINTS)
def test_dfsph_scene_is_tame_and_both_solvers_iterate(name):
    sd, cfg, sc = pp.build_dfsph(name)
    assert cfg.get_cfg("timeStepSize") == pytest.approx(2e-3 * cfg.get_cfg("particleRadius") / 0.01)
    n = pp.dfsph_steps(name)
    out, its = {}, []
    for perturb in (0, 1):
        o = pp.make_oracle(cfg, sc, name, perturb=perturb)
        o.initialize()
        for _ in range(n):
            o.step(1)
            if perturb == 0:
                its.append((o.s.last_iterations_v, o.s.last_iterations))
        out[perturb] = o.by_pid("x")
    assert scenes.rel_l2(out[1], out[0]) <= NOISE_CAP
    assert sum(a for a, _ in its) > 0 and sum(b for _, b in its) > 0, its


@pytest.mark.parametrize("name", pp.DFSPH_POINTS)
def test_dfsph_sweeps_of_the_references_agree(name):
    """The state the GPU test judges the DFSPH sweeps on (one step in): oracle against Brute in f32 and f64, as tightly as
    test_oracle_vs_brute.py asks at the default point; both sides of the 20-neighbour switch occur."""
    sd, cfg, sc = pp.build_dfsph(name)
    o = pp.make_oracle(cfg, sc, name)
    o.initialize(); o.step(1)
    o.initialize_particle_system(); o.compute_moving_boundary_volume(); o.compute_densities()
    state = {k: o[k].copy() for k in sc.arrays if k != "pid"}
    fluid = state["material"] == 1
    prm = pp.params(cfg, sc, name)
    o.compute_DFSPH_factor()
    fac = o["dfsph_factor"].copy()
    o.compute_density_change()
    chg = o["density_adv"].copy()
    o.compute_density_adv()
    adv = o["density_adv"].copy()
    for dtype in (np.float32, np.float64):
        b = Brute(prm, state, dtype=dtype)
        ref = b.dfsph_factor()
        assert np.abs(fac - ref)[fluid].max() <= 2e-4 * np.abs(ref).max()
        ref = b.dfsph_density_change()
        assert (ref[fluid] > 0).any() and (ref[fluid] == 0).any()
        assert np.abs(chg - ref)[fluid].max() <= 3e-4 * np.abs(ref).max()
        ref = b.dfsph_density_adv()
        assert np.abs(adv - ref)[fluid].max() <= 2e-5


def test_in_flight_scene_is_tame_and_the_change_matters():
    name = None      # the base point
    sd, cfg, sc = pp.build_traj(name)
    res = {}
    for key, perturb, change in (("ref", 0, True), ("perturbed", 1, True), ("unchanged", 0, False)):
        o = pp.make_oracle(cfg, sc, name, perturb=perturb)
        o.initialize(); o.step(5)
        if change:
            o.set_solver_attrs(**pp.IN_FLIGHT)
        o.step(5)
        res[key] = o.by_pid("x")
    assert scenes.rel_l2(res["perturbed"], res["ref"]) <= NOISE_CAP
    assert scenes.rel_l2(res["unchanged"], res["ref"]) > 1e-4, "the change of attributes must move the second block of steps"


def test_brute_f64_is_f64_throughout():
    sd, cfg, sc = pp.build_coupled("exp_7p5")
    b = Brute(pp.params(cfg, sc, "exp_7p5"), sc.arrays, dtype=np.float64)
    assert b.a["x"].dtype == np.float64 and np.array_equal(b.a["x"], sc.arrays["x"].astype(np.float64))
    b.boundary_volume(False); b.boundary_volume(True); b.step()
    for f in FIELDS:
        assert b.a[f].dtype == np.float64, f
    for f in (b.dfsph_factor(), b.dfsph_density_change(), b.dfsph_density_adv()):
        assert f.dtype == np.float64
    # the kernel constants are the f64 fold, not an f32 rounded on the way
    assert b._w(np.zeros(1))[0] == 8 / np.pi / (4.0 * 0.01) ** 3
    with pytest.raises(ValueError):
        Brute(pp.params(cfg, sc), sc.arrays, dtype=np.float16)
