"""Particle features on the device (include/sph_hip.h, section "Particle features"; csrc/sph_features.hip) against the brute-force
numpy model of tests/features_model.py evaluated on the context's OWN state downloaded at the sample point.

Every comparison with the model is exact (the 64-byte rows, byte for byte): the pair geometry and the kernel polynomial are the same
f32 sequence on both sides, the terms are IEEE f64 multiplies, divides and subtracts on both sides, llrint and np.rint both round to
nearest even, every sum is an integer sum whatever the order, and every float of a row is one conversion of an integer.

A stand-alone sample is taken stage by stage (`_stages`): the sort, the density and equation-of-state entry of the fused path,
`ps.features.sample()`.  The geometry tests upload density fields of their own instead: the sample uses whatever the record holds."""
import copy
import ctypes as C
import json

import numpy as np
import pytest

import fieldcolour_model as fm
from sph_taichi_amd import _lib, features, render
from tests import features_model as model
from tests import loads_scenes
from tests import scenes

pytestmark = pytest.mark.gpu

F32 = np.float32
CUBE_ANCHOR = (0.36, 0.20, 0.36)


def _open(sd, factor=0.9, seed=0, toward=None, squeeze=True, arrays=None):
    cfg, sc = scenes.build(sd)
    if squeeze:
        loads_scenes.squeeze(sc, factor, seed=seed, toward=toward)
    a = sc.arrays
    if arrays is not None:
        arrays(a)
        a["x_0"] = a["x"].copy()
    ps, solver = scenes.make_ps(sd, a)
    solver.initialize()
    return ps, solver


def _stages(ps):
    """One fused step's kernels up to the sample point: the sort, then the density-and-EOS phase."""
    ps.initialize_particle_system()
    ps._call("sph_slab_density")


def _random_density(ps, seed):
    rng = np.random.default_rng(seed)
    n = ps.density.to_numpy().shape[0]
    ps.density.from_numpy(rng.uniform(900.0, 1400.0, size=n).astype(F32))
    ps.initialize_particle_system()


def _model(ps, ft, st=None):
    st = model.state_of_ps(ps) if st is None else st
    return model.sample(st, model.params_of_ps(ps), material=ft.material, objects=ft.objects, min_neighbours=ft.min_neighbours,
                        normal_min=ft.normal_min, n_rows=ft.info().rows)


def _same(got, want, tag=""):
    assert got.dtype == want.dtype == features.ROW_DTYPE and got.shape == want.shape, tag
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])
        raise AssertionError((tag, bad.size, bad[:5].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist()))


def _by_pid(ps, values):
    out = np.zeros((ps.features.info().rows,) + values.shape[1:], dtype=values.dtype)
    out[ps.pid.to_numpy()] = values
    return out


# ---- 1: fluid beside a static solid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [None, "1"], ids=["whole-grid", "one-block"])
def test_fluid_beside_a_static_solid(blocks, monkeypatch):
    """Jittered fluid on and beside a static cube: solid candidates through m_V, fluid ones through m / rho of the step's own density,
    both counts.  With the gather's grid cut to one block (16 rows) the waves take thirty trips over the 480 targets."""
    if blocks is None:
        monkeypatch.delenv("SPH_FEATURES_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("SPH_FEATURES_BLOCKS", blocks)
    ps, solver = _open(loads_scenes.cube_scene(), toward=CUBE_ANCHOR)
    assert ps.features is None
    ft = ps.set_features(every=1, normal_min=0.35)
    assert ft is ps.features and ft.info().samples == 0 and ft.step == -1 and not ft.rows().tobytes().strip(b"\0")
    _stages(ps)
    st = model.state_of_ps(ps)
    ft.sample()
    rows, want = ft.rows(), _model(ps, ft, st)
    _same(rows, want, "cube")
    fluid = _by_pid(ps, st["material"]) == 1
    assert fluid.sum() == 480 and np.array_equal(ft.valid(), fluid) and not rows[~fluid].tobytes().strip(b"\0")
    assert (rows["n_solid"][fluid] > 0).sum() > 50 and (rows["n_fluid"][fluid] >= 5).all() and not ft.saturated().any()
    assert 0 < ft.surface().sum() < 480 and rows["vorticity"][fluid].any() and np.array_equal(ft.positions()[fluid], _by_pid(ps, st["x"])[fluid])
    i = ft.info()
    assert (i.samples, i.steps_seen, i.step, i.time) == (1, 0, 0, ps.time)
    n = ft.normal()
    length = np.sqrt((n.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length[fluid] - 1).max() < 1e-6 and not n[~fluid].any()
    w = rows["vorticity"][fluid].astype(np.float64)
    assert ft.enstrophy() == pytest.approx(0.5 * ps.m_V0 * (w * w).sum(), rel=1e-12)
    # every material as targets: the solids' rows through their own volume, and a second sample replaces the first
    both = ps.set_features(every=1, material=None, objects=[0, 1])
    both.sample()
    want2 = _model(ps, both, st)
    _same(both.rows(), want2, "fluid and cube")
    obj = _by_pid(ps, st["object_id"])
    assert np.array_equal(both.valid(), obj <= 1) and (want2["n_fluid"][obj == 1] > 0).any()
    ps.close()


# ---- 2, 3, 4: clamped cell layers, a crowded cell, an isolated particle ------------------------------------------------------------
def test_border_cells_a_crowded_cell_and_an_isolated_particle():
    """The corner scene: particles in the first and the last cell layer of every axis (the 27 cells are clipped on three sides at once,
    most solids lie outside the padding).  Eighty fluid particles are drawn into one cell (more than one wave's worth of candidates),
    one is put on top of another (r = 0: refused by r > 1e-5), one far from everybody (no pair: fill = V W(0), surface)."""
    def move(a):
        fluid = np.flatnonzero(a["material"] == 1)
        rng = np.random.default_rng(9)
        a["x"][fluid[:80]] = (np.array([0.10, 0.05, 0.05]) + rng.uniform(0.001, 0.018, size=(80, 3))).astype(F32)
        a["x"][fluid[80]] = a["x"][fluid[0]]
        a["x"][fluid[81]] = np.array([0.5, 0.6, 0.4], dtype=F32)
        a["v"][fluid] = rng.normal(size=(fluid.size, 3)).astype(F32)
    ps, solver = _open(loads_scenes.corner_scene(), factor=1.0, seed=3, arrays=move)
    _random_density(ps, seed=4)
    st = model.state_of_ps(ps)
    n = np.asarray(ps.grid_num)
    cells = model.cell_coords(st["x"], ps._params.grid_size, n)
    for axis in range(3):
        assert (cells[:, axis] == 0).any() and (cells[:, axis] == n[axis] - 1).any(), axis
    assert np.bincount(np.ravel_multi_index(cells[st["material"] == 1].T, n)).max() > 64
    ft = ps.set_features(every=1, material=None)
    ft.sample()
    rows, want = ft.rows(), _model(ps, ft, st)
    _same(rows, want, "corner")
    assert ft.valid().all() and (rows["n_fluid"] > 64).any() and (rows["n_solid"] > 0).any()
    alone = np.flatnonzero((rows["n_fluid"] + rows["n_solid"]) == 0)
    assert alone.size == 1 and rows["flags"][alone[0]] == 3 and not rows["normal"][alone[0]].any() and not rows["vorticity"][alone[0]].any()
    k = np.flatnonzero(st["pid"] == alone[0])[0]
    vol = float(st["m"][k]) / float(st["density"][k])
    assert rows["fill"][alone[0]] == F32(np.rint(vol * float(F32(ps._params.k_w)) * 2.0 ** 30) / 2.0 ** 30)
    d = st["x"][:, None, :].astype(np.float64) - st["x"][None, :, :]
    assert ((d * d).sum(axis=-1) == 0).sum() == st["x"].shape[0] + 2          # one coincident pair beside the diagonal
    ps.close()


# ---- 5: two fluid objects, one selected --------------------------------------------------------------------------------------------
def test_two_fluid_objects_one_selected():
    sd = scenes.fluid_only(counts=(6, 6, 6), start=(0.1, 0.1, 0.1), velocity=(0.5, -1.0, 0.0))
    second = (0.1 + 6 * 0.02, 0.1, 0.1)
    sd["FluidBlocks"].append(scenes._block(1, second, scenes.lattice_end(second, (5, 6, 6)), (-0.5, 0.3, 0.2)))
    ps, solver = _open(sd, factor=0.95, seed=5)
    ft = ps.set_features(every=1, objects=[1])
    _stages(ps)
    st = model.state_of_ps(ps)
    ft.sample()
    rows = ft.rows()
    _same(rows, _model(ps, ft, st), "one of two")
    obj = _by_pid(ps, st["object_id"])
    assert np.array_equal(ft.valid(), obj == 1) and (obj == 1).sum() == 180 and not rows[obj != 1].tobytes().strip(b"\0")
    only = model.sample({k: v[st["object_id"] == 1] for k, v in st.items()}, model.params_of_ps(ps), n_rows=rows.shape[0])
    assert (rows["n_fluid"][obj == 1] > only["n_fluid"][obj == 1]).any()       # the other object is a candidate
    ps.close()


# ---- 6: a non-finite velocity --------------------------------------------------------------------------------------------------------
def test_a_non_finite_velocity_saturates_its_neighbourhood_only():
    ps, solver = _open(scenes.fluid_only(counts=(8, 8, 8), velocity=(0.2, -0.4, 0.1)), factor=0.97, seed=6)
    ft = ps.set_features(every=1)
    _stages(ps)
    ft.sample()
    clean = ft.rows()
    assert not ft.saturated().any()
    st = model.state_of_ps(ps)
    k = int(np.argmin(((st["x"].astype(np.float64) - st["x"].astype(np.float64).mean(axis=0)) ** 2).sum(axis=1)))
    pid_k = int(st["pid"][k])
    v = st["v"].copy()
    v[k] = (np.nan, np.inf, 1.0)
    ps.v.from_numpy(v)
    ps.initialize_particle_system()                                           # (the sort reads positions only)
    st = model.state_of_ps(ps)
    ft.sample()
    rows = ft.rows()
    _same(rows, _model(ps, ft, st), "non-finite")
    sat = ft.saturated()
    near = np.zeros(rows.shape[0], bool)
    k = int(np.flatnonzero(st["pid"] == pid_k)[0])
    d = st["x"].astype(np.float64) - st["x"][k].astype(np.float64)
    near[st["pid"][np.sqrt((d * d).sum(axis=1)) < 0.9 * float(ps._params.support_radius)]] = True
    assert sat[st["pid"][k]] and sat[near].all() and 10 < sat.sum() < 120
    assert clean[~sat].tobytes() == rows[~sat].tobytes()                      # nothing else changes
    for name in ("x", "normal", "fill", "n_fluid", "n_solid"):                # ... and of the saturated rows only what the velocity enters
        assert np.array_equal(clean[name], rows[name]), name
    ps.close()


# ---- 7, 8: the hook, and the run untouched ------------------------------------------------------------------------------------------
def _dam(counts=(10, 14, 8)):
    return scenes.fluid_only(counts=counts, start=(0.06, 0.06, 0.06), velocity=(0.0, 0.0, 0.0))


def test_in_step_hook_after_thirty_steps():
    """every = 7 over 30 steps: steps 0, 7, 14, 21 and 28 are sampled, the latest is step 28 at t_28.  A twin makes 28 steps, then the
    stages of the 29th up to the sample point and a stand-alone sample: the same rows, and the model's on the twin's state."""
    a, sa = _open(_dam(), squeeze=False)
    b, sb = _open(_dam(), squeeze=False)
    fa = a.set_features(every=7)
    sa.step(13)
    sa.step(17)
    sb.step(28)
    t28 = b.time
    fb = b.set_features(every=7)
    _stages(b)
    st = model.state_of_ps(b)
    fb.sample()
    ia, ib = fa.info(), fb.info()
    assert (ia.samples, ia.steps_seen, ia.step, ia.time) == (5, 30, 28, t28) and (ib.samples, ib.steps_seen, ib.step, ib.time) == (1, 0, 0, t28)
    assert (fa.step, fa.time, fa.samples) == (28, t28, 5)
    ra, rb = fa.rows(), fb.rows()
    _same(ra, rb, "hook against stand-alone")
    _same(rb, _model(b, fb, st), "twin against the model")
    assert not np.array_equal(st["pid"], np.arange(st["pid"].shape[0]))         # many sorts later the records are not in id order
    assert np.array_equal(ra["x"][st["pid"]], st["x"]) and ra["vorticity"].any() and 0 < fa.surface().sum() < ra.shape[0]
    a.close(); b.close()


@pytest.mark.parametrize("scene", ["pure_fluid", "fluid_and_solids"])
def test_the_step_is_untouched(scene):
    """Positions and velocities after 30 steps with a set armed equal those of a run without, bit for bit; after clear_features the run
    goes on identically.  On the pure-fluid scene the lean sort is excluded while the set is armed: other kernels, the same bits."""
    if scene == "pure_fluid":
        sd, kw = scenes.fluid_only(counts=(12, 12, 10), velocity=(0.3, -1.0, 0.2)), dict(squeeze=False)
    else:
        sd, kw = loads_scenes.cube_scene(), dict(toward=CUBE_ANCHOR, factor=0.97)
    runs = []
    for armed in (False, True):
        ps, solver = _open(copy.deepcopy(sd), **kw)
        if armed:
            ps.set_features(every=7)
        solver.step(9)
        solver.step(1)
        solver.step(20)
        mid = {n: getattr(ps, n).to_numpy().copy() for n in ("x", "v", "pid", "density", "pressure")}
        if armed:
            assert ps.features.info().samples == 5 and ps.features.valid().sum() == (ps.material.to_numpy() == 1).sum()
            ps.clear_features()
            assert ps.features is None
        solver.step(10)
        runs.append((mid, {n: getattr(ps, n).to_numpy().copy() for n in ("x", "v", "pid", "density", "pressure")}))
        ps.close()
    for off, on in zip(*runs):
        for n in off:
            assert off[n].tobytes() == on[n].tobytes(), n


# ---- 9: refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ps, solver = _open(loads_scenes.block_on_slab(), seed=2)
    for name, args in (("sph_features_sample", ()), ("sph_features_download", (None, 0)), ("sph_features_paint", (0, 0.0, 1.0, None))):
        with pytest.raises(_lib.SphError, match=rf"rc=-4.*{name}.*no feature set"):
            ps._call(name, *args)
    good = ps.set_features(every=1)
    solver.step(1)
    kept = good.rows().tobytes()
    base = features.set_args()
    for kw, word in ((dict(every=0), "every"), (dict(min_neighbours=-1), "min_neighbours"), (dict(normal_min=float("nan")), "normal_min"),
                     (dict(normal_min=-1.0), "normal_min"), (dict(material=300), "material"), (dict(n_objects=33), "n_objects")):
        p = features.feature_params(base)
        for k, v in kw.items():
            setattr(p.select if k in ("material", "n_objects") else p, k, v)
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*sph_features_set.*{word}"):
            ps._call("sph_features_set", C.byref(p))
        assert good.info().samples == 1 and good.rows().tobytes() == kept      # a refused set changes nothing
    with pytest.raises(_lib.SphError, match=r"rc=-1.*sph_features_download.*the set holds"):
        ps._call("sph_features_download", None, good.info().rows + 1)
    ps.close()
    cfg, sc = scenes.build(loads_scenes.block_on_slab())
    fresh, _ = scenes.make_ps(loads_scenes.block_on_slab(), sc.arrays)
    fresh.set_features()
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_features_sample.*needs the neighbour structure"):
        fresh.features.sample()
    fresh.close()
    df, dsolver = scenes.make_ps(scenes.as_dfsph(loads_scenes.block_on_slab()))
    dsolver.initialize()
    df.set_features()
    t = df.time
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_dfsph_step.*feature set is registered"):
        dsolver.step(1)
    assert df.time == t and df.features.info().steps_seen == 0
    df.clear_features()
    dsolver.step(1)
    df.close()


def test_slab_rank_is_refused():
    from sph_taichi_amd import ParticleSystem
    from sph_taichi_amd.config_builder import SimConfig
    sd = scenes.fluid_only(counts=(4, 4, 4))
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.set_features()
    p = features.feature_params(features.set_args())
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_features_set.*single-domain"):
        slab._call("sph_features_set", C.byref(p))
    for name, args in (("sph_features_sample", ()), ("sph_features_download", (None, 0)), ("sph_features_paint", (0, 0.0, 1.0, None))):
        with pytest.raises(_lib.SphError, match=rf"rc=-4.*{name}.*single-domain"):
            slab._call(name, *args)
    i = _lib.SphFeatureInfo()
    slab._call("sph_features_info", C.byref(i))
    assert (i.every, i.rows, i.step) == (0, 0, -1)
    slab.close()


# ---- 10: paint ------------------------------------------------------------------------------------------------------------------------
def test_paint():
    ps, solver = _open(loads_scenes.cube_scene(), toward=CUBE_ANCHOR)
    ft = ps.set_features(every=1)
    solver.step(3)
    rows = ft.rows()
    valid = ft.valid()
    before = scenes.ps_by_pid(ps, "color")
    n = before.shape[0]
    assert 0 < valid[:n].sum() < n
    assert ft.paint("vorticity", range=(0.0, 30.0), colormap="coolwarm") == (0.0, 30.0)
    want = before.copy()
    idx = fm.index(features.paint_values(rows[:n], "vorticity"), 0.0, 30.0)
    want[valid[:n]] = render.colormap("coolwarm").astype(np.int32)[idx[valid[:n]]]
    got = scenes.ps_by_pid(ps, "color")
    assert np.array_equal(got, want) and np.unique(idx[valid[:n]]).size > 3 and np.array_equal(got[~valid[:n]], before[~valid[:n]])
    rng = ft.paint("surface", range=(0.0, 1.0), colormap="grey")
    idx = fm.index(features.paint_values(rows[:n], "surface"), *rng)
    assert set(np.unique(idx[valid[:n]])) == {0, 255}
    want[valid[:n]] = render.colormap("grey").astype(np.int32)[idx[valid[:n]]]
    assert np.array_equal(scenes.ps_by_pid(ps, "color"), want)
    auto = ft.paint("neighbours")                                              # the valid rows' own range, the default table
    count = (rows["n_fluid"] + rows["n_solid"])[valid]
    assert auto == (float(count.min()), float(count.max()))
    lut = render.colormap("heat").astype(np.int32)
    for args in ((5, 0.0, 1.0, lut), (-1, 0.0, 1.0, lut), (0, 1.0, 1.0, lut), (0, 0.0, float("nan"), lut), (0, 0.0, 1e-45, lut), (0, 0.0, 1.0, lut + 1)):
        with pytest.raises(_lib.SphError, match=r"rc=-1.*sph_features_paint"):
            ps._call("sph_features_paint", args[0], args[1], args[2], np.ascontiguousarray(args[3]).ctypes.data_as(C.c_void_p))
    ps.close()


# ---- 11: two runs, the same bits; the scene key ------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    out = []
    for _ in range(2):
        ps, solver = _open(loads_scenes.cube_scene(), toward=CUBE_ANCHOR, factor=0.97)
        ft = ps.set_features(every=3, material=None)
        solver.step(10)
        out.append((ft.rows().tobytes(), ft.step))
        ps.close()
    assert out[0] == out[1] and out[0][1] == 9


def test_run_simulation_writes_surface_files_and_painted_frames(tmp_path, monkeypatch, capsys):
    sd = scenes.fluid_only(counts=(6, 8, 6), start=(0.06, 0.06, 0.06), velocity=(0.0, 0.0, 0.0))
    sd["Configuration"]["timeStepSize"] = 0.016                        # every frame is an output interval
    sd["Configuration"]["exportFrame"] = True
    sd["Configuration"]["features"] = {"every": 2, "objects": [0], "minNeighbours": 24, "export": "surface",
                                       "paint": {"field": "vorticity", "range": [0, 50]}}
    scene_file = tmp_path / "features_scene.json"
    scene_file.write_text(json.dumps(sd))
    extra = tmp_path / "extra"
    monkeypatch.chdir(tmp_path)
    from sph_taichi_amd import run_simulation
    run_simulation.main(["--scene_file", str(scene_file), "--frames", "3", "--features", str(extra), "--image_size", "64", "48"])
    report = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert report["features"]["every"] == 2 and report["features"]["samples"] == 2 and report["features"]["files_written"] == 3
    assert report["frames_written"] == 3
    for d in (tmp_path / "features_scene_output", extra):
        data = features.read_ply(str(d / "features_000002.ply"))
        assert 0 < data.shape[0] <= 6 * 8 * 6 and (data["surface"] == 1).all() and np.all(np.diff(data["id"]) > 0)
    with pytest.raises(ValueError, match="--features needs"):
        sd["Configuration"].pop("features")
        scene_file.write_text(json.dumps(sd))
        run_simulation.main(["--scene_file", str(scene_file), "--frames", "1", "--features", str(extra)])
