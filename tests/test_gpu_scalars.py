"""Carried scalars on the device (include/sph_hip.h, section "Carried scalars"; csrc/sph_scalars.hip) against the brute-force numpy
model of tests/scalars_model.py evaluated on the context's OWN state downloaded at the sample point.

Every comparison with the model is exact (array_equal on every i64 of the store and on both counters): the pair geometry is the same
f32 sequence on both sides, the weights are IEEE f64 operations on both sides, llrint and np.rint both round to nearest even, and
every sum is an integer sum whatever the order.  The one tolerance in this file is the formula test's, 3 x the error the model
measures on the CPU (profiles/scalars_parity.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from sph_taichi_amd import _lib, render
from tests import scalars_model as model
from tests import scenes

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("x", "m_V", "material", "object_id", "pid")
RUN = ("x", "v", "density", "pressure", "acceleration", "pid")


def _state(ps):
    return {f: getattr(ps, f).to_numpy() for f in STATE}


def _expect(ps, st, by_id, sel_material, sel_objects, sources, kappa, every, detail=False):
    """The model's sample of the downloaded state `st` (record order) on the store `by_id` i64 [n_ids, K]: (new store, model output)."""
    role = model.roles(st["material"], st["object_id"], sel_material, sel_objects, sources)
    snap = model.snapshot(by_id[st["pid"]], role, st["object_id"], sources)
    out = model.sample(st["x"], st["m_V"], role, snap, model.coefficients(ps._params.dt, every, kappa), F32(ps._params.support_radius),
                       F32(ps._params.k_dw), detail=detail)
    new = by_id.copy()
    car = role == model.CARRIER
    new[st["pid"][car]] = out[0][car]
    return new, out, role


def _same(got, want, tag=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype == np.int64 and got.shape == want.shape, tag
    assert np.array_equal(got, want), (tag, int((got != want).sum()), got[got != want][:4].tolist(), want[got != want][:4].tolist())


def _fluid_tank(counts=(10, 12, 8), soft=False):
    sd = scenes.fluid_only(counts=counts, velocity=(0.3, -1.0, 0.2))
    if soft:
        sd["Configuration"]["stiffness"] = 50.0
        sd["Configuration"]["exponent"] = 1
    cfg, sc = scenes.build(sd)
    scenes.jitter(sc, 0.1, seed=11)
    return sd, sc


# ---- (a) one stand-alone sample on the mixed scene, with (e)'s overshoot, saturation and range property -----------------------------
@pytest.mark.parametrize("blocks", [None, "3"], ids=["whole-grid", "three-blocks"])
def test_one_sample_on_the_mixed_scene(blocks, monkeypatch):
    """tests/scalars_model.py mixed_scene: two carrier blocks, an unselected sheet between them, a fluid and a solid source, a cell
    of 250 records, carriers in and outside the domain's corner cells, 1,563 carriers (no multiple of 4), K = 3 with diffusivities
    (kappa, 0, 10 kappa), values at +-2^20.  With the diffusion's grid cut to three blocks (48 rows) the waves take 33 trips."""
    if blocks is None:
        monkeypatch.delenv("SPH_SCALARS_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("SPH_SCALARS_BLOCKS", blocks)
    sd, a, values, crowd = model.mixed_scene()
    kappa, planted = model.mixed_kappa(a, values, crowd, F32(0.04), sd["Configuration"]["timeStepSize"])
    values[planted, 2] = -model.VALUE_MAX
    ps, solver = scenes.make_ps(sd, a)
    solver.initialize()
    kap = (kappa, F32(0), F32(10) * kappa)
    sc = ps.set_scalars(channels=("heat", "still", "fast"), diffusivity=kap, values=values, sources=model.MIXED_SOURCES, objects=[0])
    assert sc is ps.scalars and sc.info().samples == 0
    by_id = model.to_raw(values)
    for oid, row in model.MIXED_SOURCES.items():                 # set_scalars shows a source's particles at their prescribed value
        by_id[a["object_id"] == oid] = model.to_raw(row)
    _same(sc.raw(), by_id, "as set")
    ps.initialize_particle_system()
    st = _state(ps)
    sc.sample()
    want, out, role = _expect(ps, st, by_id, 1, [0], model.MIXED_SOURCES, kap, 1, detail=True)
    got = sc.raw()
    _same(got, want, "one sample")
    new, over, sat, pairs, lo, hi, wsum = out
    info = sc.info()
    assert (info.samples, info.steps_seen) == (1, 0) and info.overshoot == over.tolist() == [0, 0, 250] and info.saturated == sat.tolist() == [0, 0, 1]
    assert abs(got[planted, 2]) == 1 << 52 and np.array_equal(got[:, 1], by_id[:, 1]) and (got[:, 0] != by_id[:, 0]).sum() > 1400
    # below the stability limit (channel 0) every new value lies within its contributing snapshot values, half a unit per llrint
    car = role == model.CARRIER
    assert (wsum[car, 0] <= 1 << 32).all()
    margin = pairs[car] + 1
    assert (new[car, 0] >= lo[car, 0] - margin).all() and (new[car, 0] <= hi[car, 0] + margin).all()
    # a second sample goes on from the first
    sc.sample()
    want2, out2, _ = _expect(ps, st, want, 1, [0], model.MIXED_SOURCES, kap, 1)
    _same(sc.raw(), want2, "second sample")
    info = sc.info()
    assert info.overshoot == (over + out2[1]).tolist() and info.saturated == (sat + out2[2]).tolist() and info.samples == 2
    assert np.array_equal(sc.values(), want2.astype(np.float64) / model.ONE)
    ps.close()


# ---- (b) the hook: in-step samples against the model on the x(t_k) of a twin -------------------------------------------------------
@pytest.mark.parametrize("dfsph", [False, True], ids=["wcsph", "dfsph"])
@pytest.mark.parametrize("every", [1, 2])
def test_in_step_samples(every, dfsph):
    sd = scenes.fluid_with_rigid_blocks()
    if dfsph:
        sd = scenes.as_dfsph(sd)
    cfg, scn = scenes.build(sd)
    scenes.jitter(scn, 0.1, seed=4)
    a, sa = scenes.make_ps(sd, scn.arrays)
    b, sb = scenes.make_ps(sd, scn.arrays)
    sa.initialize(); sb.initialize()
    n = a.particle_max_num
    rng = np.random.default_rng(8)
    values = rng.uniform(0.0, 100.0, size=(n, 2))
    sources = {1: (350.0, -1.0)}
    kap = (F32(2e-3), F32(5e-4))
    sc = a.set_scalars(channels=("heat", "dye"), diffusivity=kap, values=values, sources=sources, every=every)
    by_id = sc.raw()
    sa.step(5)
    want, samples = by_id, 0
    for k in range(5):
        if k % every == 0:
            want, out, _ = _expect(b, _state(b), want, 1, [], sources, kap, every)     # x(t_k): the twin before its step k
            assert not out[1].any() and not out[2].any()
            samples += 1
        sb.step(1)
    _same(sc.raw(), want, f"every {every}")
    info = sc.info()
    assert (info.samples, info.steps_seen, info.every) == (samples, 5, every) and (want != by_id).sum() > n
    for f in ("x", "v"):                                                # the twin never held a set: the run is the same run
        assert np.array_equal(scenes.ps_by_pid(a, f), scenes.ps_by_pid(b, f)), f
    a.close(); b.close()


# ---- (c) the run is untouched ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solids", [False, True], ids=["pure-fluid", "with-solids"])
def test_the_run_is_untouched(solids):
    if solids:
        sd = scenes.fluid_with_rigid_blocks()
        cfg, scn = scenes.build(sd)
        scenes.jitter(scn, 0.1, seed=4)
    else:
        sd, scn = _fluid_tank(soft=True)
    frames, counts = [], []
    for with_set in (False, True):
        ps, solver = scenes.make_ps(sd, scn.arrays)
        ps.set_option(_lib.OPT_SORT_FAST, 1)
        ps.set_option(_lib.OPT_SORT_LEAN, 1)
        solver.initialize()
        if with_set:
            ps.set_scalars(channels=("a", "b"), diffusivity=(1e-3, 1e-4), values=np.random.default_rng(3).uniform(0, 1, (ps.particle_max_num, 2)),
                           sources={1: (1.0, 0.0)} if solids else None)
        solver.step(7); solver.step(13)
        counts.append((ps.get_option(_lib.OPT_SORT_FAST_COUNT), ps.get_option(_lib.OPT_SORT_GENERAL_COUNT)))
        if with_set:
            assert ps.scalars.info().samples == 20 and (ps.scalars.raw() != 0).any()
        frames.append({f: getattr(ps, f).to_numpy().copy() for f in RUN})
        ps.close()
    assert counts[0] == counts[1] and sum(counts[0]) == 21 and (solids or counts[0] == (20, 1)), counts
    for f in RUN:
        assert frames[0][f].tobytes() == frames[1][f].tobytes(), f


# ---- (d) conservation --------------------------------------------------------------------------------------------------------------
def test_conservation_over_fifty_steps():
    """One fluid of equal volumes, no sources: the integer sum of every channel is its start to the last bit; kappa = 0 leaves every
    word as it was."""
    sd, scn = _fluid_tank()
    ps, solver = scenes.make_ps(sd, scn.arrays)
    solver.initialize()
    assert len(np.unique(ps.m_V.to_numpy().view(np.uint32))) == 1
    n = ps.particle_max_num
    values = np.zeros((n, 3))
    values[:, 0] = np.where(scn.arrays["x"][:, 0] < 0.2, 1.0, 0.0)          # dye in one half
    values[:, 1] = np.random.default_rng(5).uniform(-1e3, 1e3, n)
    values[:, 2] = values[:, 1]
    sc = ps.set_scalars(channels=("dye", "noise", "still"), diffusivity=(2e-3, 5e-3, 0.0), values=values)
    start = sc.raw()
    totals = [sc.total(k) for k in range(3)]
    assert totals == start.sum(axis=0).tolist()
    solver.step(50)
    end = sc.raw()
    info = sc.info()
    assert info.samples == 50 and info.overshoot == [0, 0, 0] and info.saturated == [0, 0, 0]
    assert [sc.total("dye"), sc.total("noise"), sc.total(2)] == totals
    assert np.array_equal(end[:, 2], start[:, 2]) and (end[:, 0] != start[:, 0]).sum() > 100 and (end[:, 1] != start[:, 1]).all()
    lo, hi = sc.range("dye")
    assert 0.0 <= lo < hi <= 1.0
    ps.close()


# ---- (f) paint -----------------------------------------------------------------------------------------------------------------------
def test_paint():
    sd = scenes.fluid_with_rigid_blocks()
    cfg, scn = scenes.build(sd)
    ps, solver = scenes.make_ps(sd, scn.arrays)
    solver.initialize()
    n = ps.particle_max_num
    values = np.random.default_rng(6).uniform(-5.0, 45.0, size=(n, 2))
    sc = ps.set_scalars(channels=("heat", "dye"), diffusivity=(1e-3, 0), values=values, sources={1: (40.0, 0.0)})
    before = scenes.ps_by_pid(ps, "color")
    obj = np.zeros(n, np.int64)
    obj[ps.pid.to_numpy()] = ps.object_id.to_numpy()
    mat = np.zeros(n, np.int64)
    mat[ps.pid.to_numpy()] = ps.material.to_numpy()
    part = (mat == 1) | (obj == 1)                                       # fluid carriers and the static slab; the dynamic cube takes no part
    assert part.sum() < n and (obj == 2).sum() > 0
    assert sc.paint("heat", range=(0.0, 40.0), colormap="coolwarm") == (0.0, 40.0)
    raw = sc.raw()
    want = before.copy()
    want[part] = render.colormap("coolwarm").astype(np.int32)[model.paint_index(raw[part, 0], 0.0, 40.0)]
    got = scenes.ps_by_pid(ps, "color")
    assert np.array_equal(got, want) and (got[part] != before[part]).any() and np.array_equal(got[~part], before[~part])
    idx = model.paint_index(raw[part, 0], 0.0, 40.0)
    assert idx.min() == 0 and idx.max() == 255 and (idx[obj[part] == 1] == 255).all()
    rng = sc.paint(1)                                                    # the carriers' own range, the default table
    assert rng == sc.range(1)
    want[part] = render.colormap("heat").astype(np.int32)[model.paint_index(raw[part, 1], *rng)]
    assert np.array_equal(scenes.ps_by_pid(ps, "color"), want)
    lut = render.colormap("heat").astype(np.int32)
    for args, code in (((2, 0.0, 1.0, lut), -1), ((-1, 0.0, 1.0, lut), -1), ((0, 1.0, 1.0, lut), -1), ((0, 0.0, float("nan"), lut), -1),
                       ((0, 0.0, 1e-45, lut), -1), ((0, 0.0, 1.0, lut + 1), -1)):
        with pytest.raises(_lib.SphError, match=rf"rc={code}.*sph_scalars_paint"):
            ps._call("sph_scalars_paint", args[0], args[1], args[2], np.ascontiguousarray(args[3]).ctypes.data_as(C.c_void_p))
    with pytest.raises(_lib.SphError, match=r"rc=-1.*table is NULL"):
        ps._call("sph_scalars_paint", 0, 0.0, 1.0, None)
    assert np.array_equal(scenes.ps_by_pid(ps, "color"), want)            # a refused paint paints nothing
    ps.close()


# ---- (g) replace, clear, every across calls, refusals ----------------------------------------------------------------------------------
def test_bookkeeping_and_refusals():
    sd, scn = _fluid_tank(counts=(8, 8, 8))
    ps, solver = scenes.make_ps(sd, scn.arrays)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_scalars_sample.*no scalar set"):
        ps._call("sph_scalars_sample")
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_scalars_download.*no scalar set"):
        ps._call("sph_scalars_download", None, None, 1)
    i = _lib.SphScalarInfo()
    ps._call("sph_scalars_info", C.byref(i))
    assert (i.K, i.ids, i.samples) == (0, 0, 0) and ps.scalars is None
    n = ps.particle_max_num
    values = np.random.default_rng(9).uniform(0, 10, (n, 1))
    sc = ps.set_scalars(diffusivity=(2e-3,), values=values, every=3)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*sph_scalars_sample.*neighbour structure"):
        sc.sample()
    solver.initialize()
    by_id = sc.raw()
    _same(by_id, model.to_raw(values), "as set")
    # every = 3 across calls of 2, 2, 3 steps: steps 0, 3 and 6 are sampled
    twin, stw = scenes.make_ps(sd, scn.arrays)
    stw.initialize()
    want = by_id
    for call in (2, 2, 3):
        solver.step(call)
    for k in range(7):
        if k % 3 == 0:
            want, _, _ = _expect(twin, _state(twin), want, 1, [], {}, (F32(2e-3),), 3)
        stw.step(1)
    _same(sc.raw(), want, "every 3 over three calls")
    assert (sc.info().samples, sc.info().steps_seen) == (3, 7)
    # every refusal leaves the set as it is and sampling
    good = _lib.SphScalarParams()
    good.K, good.every, good.kappa[0] = 1, 1, 1e-3
    good.select.material = 1
    ok = np.zeros((n, 1))

    def bad(**kw):
        p = _lib.SphScalarParams.from_buffer_copy(good)
        for k, v in kw.items():
            if k == "kappa":
                p.kappa[0] = v
            elif k == "material":
                p.select.material = v
            elif k == "sel_objects":
                p.select.n_objects = v
            elif k == "source":
                p.n_sources, p.source_object[0], p.source_object[1], p.source_value[0][0] = v
            else:
                setattr(p, k, v)
        return p
    cases = [(bad(K=5), ok, n), (bad(K=-1), ok, n), (bad(every=0), ok, n), (bad(n_sources=9), ok, n), (bad(n_sources=-1), ok, n),
             (bad(kappa=-1e-3), ok, n), (bad(kappa=float("nan")), ok, n), (bad(kappa=float("inf")), ok, n), (bad(material=256), ok, n),
             (bad(sel_objects=33), ok, n), (bad(source=(1, 99, 0, 0.0)), ok, n), (bad(source=(2, 0, 0, 0.0)), ok, n),
             (bad(source=(1, 0, 0, float("inf"))), ok, n), (bad(source=(1, 0, 0, 2.0 ** 20 + 1)), ok, n), (bad(), ok, n + 1), (bad(), ok, 0),
             (bad(), np.full((n, 1), np.nan), n), (bad(), np.full((n, 1), 2.0 ** 20 + 0.5), n)]
    for p, vals, ids in cases:
        with pytest.raises(_lib.SphError, match=r"rc=-1.*sph_scalars_set"):
            ps._call("sph_scalars_set", vals.ctypes.data_as(C.c_void_p), ids, C.byref(p))
    with pytest.raises(_lib.SphError, match=r"rc=-1.*sph_scalars_download.*n_ids"):
        ps._call("sph_scalars_download", None, None, n - 1)
    _same(sc.raw(), want, "after the refusals")
    assert (sc.info().samples, sc.info().steps_seen, sc.info().every) == (3, 7, 3)
    solver.step(3)                                                       # steps 7, 8, 9: step 9 is sampled
    stw.step(2)
    want, _, _ = _expect(twin, _state(twin), want, 1, [], {}, (F32(2e-3),), 3)
    _same(sc.raw(), want, "the last good set goes on sampling")
    # replace: new values, counters from zero; NULL values are zeros; clear: nothing is sampled any more
    sc2 = ps.set_scalars(channels=("a", "b"), diffusivity=(1e-3, 1e-3))
    assert ps.scalars is sc2 and not sc2.raw().any() and sc2.raw().shape == (n, 2) and (sc2.info().samples, sc2.info().steps_seen) == (0, 0)
    solver.step(2)
    assert sc2.info().samples == 2 and not sc2.raw().any()
    ps.clear_scalars()
    assert ps.scalars is None
    solver.step(2)
    ps._call("sph_scalars_info", C.byref(i))
    assert (i.K, i.samples, i.steps_seen) == (0, 0, 0)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*no scalar set"):
        sc2.raw()
    ps.close(); twin.close()


def test_save_round_trip(tmp_path):
    sd, scn = _fluid_tank(counts=(6, 6, 6))
    ps, solver = scenes.make_ps(sd, scn.arrays)
    solver.initialize()
    sc = ps.set_scalars(values={0: (3.25,)}, diffusivity=(1e-3,))
    solver.step(3)
    path = str(tmp_path / "scalars.npz")
    sc.save(path)
    z = np.load(path)
    assert np.array_equal(z["raw"], sc.raw()) and np.array_equal(z["ids"], np.arange(ps.particle_max_num)) and list(z["channels"]) == ["dye"]
    again = ps.set_scalars(values=z["values"], diffusivity=(1e-3,))          # values() plus set_scalars restores a run
    assert np.array_equal(again.raw(), z["raw"])
    ps.close()


# ---- (h) the formula, independently of the kernel: the one toleranced test ---------------------------------------------------------
def test_cosine_mode_decays_at_the_analytic_rate():
    """A resting lattice block at rest density, C = cos(pi x / L) along its long axis, ten stand-alone samples with a = dt * 50 * kappa:
    the device equals the model word for word, and the decay rate of the mode over the block's core is the analytic
    kappa (pi / L)^2 within 3 x the error the model measures on the CPU (0.0180: profiles/scalars_parity.json)."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "scalars_parity.json")))
    x, mode, L, core = model.lattice()
    sd = scenes.fluid_only(counts=model.MODE_COUNTS, start=(0.1, 0.1, 0.1), velocity=(0.0, 0.0, 0.0))
    cfg, scn = scenes.build(sd)
    a = scn.arrays
    assert a["x"].shape == x.shape and sd["Configuration"]["timeStepSize"] == model.MODE_DT
    a["x"] = x.copy(); a["x_0"] = x.copy()
    ps, solver = scenes.make_ps(sd, a)
    solver.initialize()
    assert len(np.unique(ps.m_V.to_numpy())) == 1 and F32(ps._params.support_radius) == F32(2 * model.MODE_D)
    sc = ps.set_scalars(channels=("mode",), diffusivity=(model.MODE_KAPPA,), values=mode[:, None], every=model.MODE_EVERY)
    ps.initialize_particle_system()
    for _ in range(model.MODE_SAMPLES):
        sc.sample()
    got = sc.raw()[:, 0]
    err_model, want, coef = model.mode_decay(m_V=scenes.ps_by_pid(ps, "m_V"), k_dw_=F32(ps._params.k_dw))   # the context's own constants
    assert coef == model.coefficients(ps._params.dt, model.MODE_EVERY, [F32(model.MODE_KAPPA)])
    _same(got, want, "ten samples")
    err = model.mode_rate_error(got, mode, core, L, model.MODE_SAMPLES * float(F32(model.MODE_DT)) * model.MODE_EVERY)
    print(f"decay-rate error: device {err:.6f}, model {err_model:.6f}, bound {rec['bound']:.6f}")
    assert err <= rec["bound"] and rec["bound"] == pytest.approx(3 * rec["rate_error_measured"])
    assert sc.info().overshoot == [0] and sc.info().saturated == [0]
    ps.close()
