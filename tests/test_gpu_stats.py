"""Running flow statistics on the device (include/sph_hip.h, section "Running flow statistics"; csrc/sph_stats.hip) against the
numpy model of tests/stats_model.py evaluated on the context's OWN state downloaded at each sample.

Every comparison with the model is exact (array_equal on all eleven i64 planes): the scatter's sums are integers whatever the
particle order, the i64 -> f64 conversions and the f64 divisions are correctly rounded on both sides, the scalings are by powers of
two and llrint / np.rint both round to nearest even.  The only tolerances in this file are the derived bounds of the last test.

Step 0 of a registered set is always sampled by the hook (steps_seen % every == 0 at steps_seen == 0), so the stand-alone context of
`test_in_step_samples_equal_stand_alone_samples` takes its samples by hand before steps 3, 6 and 9 and lets the hook take step 0's;
that the hook's sample of step 0 equals a stand-alone sample of the same state is asserted there with a third context.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from sph_taichi_amd import _lib, mesh, stats
from tests import sample_model
from tests import scenes
from tests import stats_model as model

pytestmark = pytest.mark.gpu

F32 = np.float32
PLANES = ("n_wet", "sum_w", "sum_u", "sum_uu")
BLOCK = (10, 12, 8)                                              # 960 fluid particles from (0.1, 0.1, 0.1), spacing 0.02
ODD = dict(origin=(0.13, 0.21, 0.12), spacing=(0.03, 0.025, 0.02), shape=(7, 5, 9))     # 315 nodes: no multiple of 2, 64 or 256


def _open(sd=None, dfsph=False, velocity=(0.0, -1.0, 0.0)):
    sd = sd if sd is not None else scenes.fluid_only(counts=BLOCK, velocity=velocity)
    ps, solver = scenes.make_ps(scenes.as_dfsph(sd) if dfsph else sd)
    solver.initialize()
    return ps, solver


def _particles(ps):
    return {f: getattr(ps, f).to_numpy() for f in ("x", "v", "m_V", "material", "object_id")}


def _model_sample(acc, ps, st, f=None, material=1, objects=()):
    f = f if f is not None else _particles(ps)
    pos = sample_model.node_positions(st.origin, st.spacing, st.shape)
    sel = sample_model.select(f["material"], f["object_id"], material, objects)
    return model.sample(acc, pos, f["x"], f["v"], f["m_V"], sel, sample_model.inv_h(ps.support_radius), F32(ps._params.k_w), st.wet_min)


def _same(got, want, tag=""):
    for k in PLANES:
        g, w = getattr(got, k).reshape(want[k].shape), want[k]
        assert g.dtype == w.dtype == np.int64, (tag, k)
        assert np.array_equal(g, w), (tag, k, int((g != w).sum()), int(np.abs(g - w).max()))
    assert got.samples == want["samples"], tag


def _bytes(acc):
    return b"".join(getattr(acc, k).tobytes() for k in PLANES)


# ---- 1: bit parity of one stand-alone sample ------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [ODD,
                                  dict(origin=(0.05, 0.2, 0.04), spacing=0.02, shape=(12, 1, 11)),                  # a slice
                                  dict(origin=(0.02, 0.02, 0.02), spacing=(0.03, 0.035, 0.03), shape=(11, 11, 9)),  # sticks out on every side
                                  dict(origin=(0.2, 0.2, 0.18), spacing=0.02, shape=(1, 1, 1)),
                                  dict(origin=(0.1, 0.1, 0.1), spacing=0.02, shape=(8, 8, 4))],                     # even: the 16-byte instance
                         ids=["odd-volume", "slice", "sticks-out", "one-node", "even-volume"])
def test_one_sample_against_the_model(grid):
    ps, solver = _open()
    rng = np.random.default_rng(2)
    v = ps.v.to_numpy()
    ps.v.from_numpy((v + rng.normal(scale=0.5, size=v.shape)).astype(F32))          # every particle its own velocity
    st = ps.set_statistics(every=5, **grid)
    assert st is ps.statistics and st.info().samples == 0 and st.info().shape == tuple(grid["shape"])
    zero = st.accumulators()
    assert not any(getattr(zero, k).any() for k in PLANES)
    st.sample()
    got = st.accumulators()
    want = _model_sample(model.fresh(st.nodes), ps, st)
    _same(got, want, grid)
    i = st.info()
    assert (i.samples, i.dropped, i.steps_seen, i.every) == (1, 0, 0, 5) and i.t_first == i.t_last == ps.time == st.times[0]
    n_wet = want["n_wet"]
    if st.nodes > 1:
        assert n_wet.any()
    if grid["shape"] == (11, 11, 9):
        assert (n_wet == 0).sum() > 100 and n_wet.sum() > 100                         # never-wet nodes and wet ones
        assert np.isnan(got.mean_velocity()[n_wet.reshape(st.shape) == 0]).all()
    st.sample()                                                                         # the fold left the scratch clear
    _same(st.accumulators(), _model_sample(want, ps, st), "second sample")
    ps.close()


# ---- 2: a node that is wet in some samples and dry in others -------------------------------------------------------------------
def test_intermittent_node():
    ps, solver = _open(velocity=(0.0, -5.0, 0.0))
    st = ps.set_statistics(origin=(0.15, 0.30, 0.15), spacing=(0.02, 0.005, 0.02), shape=(5, 11, 3), every=1000, wet=0.4)    # across the top face
    want = model.fresh(st.nodes)
    for k in range(6):
        f = _particles(ps)
        want = _model_sample(want, ps, st, f)
        st.sample()
        _same(st.accumulators(), want, k)
        solver.step(1)
        if k == 0:          # the hook takes step 0 of a registered set whatever `every` is: the state of the first hand sample once more
            want = _model_sample(want, ps, st, f)
    got = st.accumulators()
    _same(got, want, "end")
    assert st.info().samples == 7 and st.info().steps_seen == 6
    assert ((got.n_wet > 0) & (got.n_wet < 7)).any() and (got.n_wet == 7).any() and (got.n_wet == 0).any()
    inter = got.intermittency()
    assert ((inter > 0) & (inter < 1)).any()
    ps.close()


# ---- 3: in-step samples against stand-alone samples ----------------------------------------------------------------------------
def test_in_step_samples_equal_stand_alone_samples():
    a, sa = _open()
    b, sb = _open()
    c, sc = _open()
    ta, tb, tc = a.set_statistics(every=3, **ODD), b.set_statistics(every=1000, **ODD), c.set_statistics(every=1000, **ODD)
    tc.sample()
    first = tc.accumulators()
    assert tc.info().steps_seen == 0
    sa.step(7)
    sa.step(5)
    for k in range(12):
        if k in (3, 6, 9):
            tb.sample()
        sb.step(1)
        if k == 0:
            assert _bytes(tb.accumulators()) == _bytes(first) and first.n_wet.any()      # the hook's sample of step 0 = a stand-alone one
    ia, ib = ta.info(), tb.info()
    assert (ia.samples, ia.steps_seen, ia.dropped) == (4, 12, 0) and (ib.samples, ib.steps_seen) == (4, 12)
    ga, gb = ta.accumulators(), tb.accumulators()
    assert _bytes(ga) == _bytes(gb) and _bytes(ga) != _bytes(first)
    dt = float(F32(a._params.dt))
    assert ia.t_first == 0.0 and abs(ia.t_last - 9 * dt) < 1e-12 and ib.t_last == ia.t_last
    assert a.x.to_numpy().tobytes() == b.x.to_numpy().tobytes()
    for p in (a, b, c):
        p.close()


# ---- 4: the run is untouched ---------------------------------------------------------------------------------------------------
def test_the_run_is_untouched():
    sd = scenes.fluid_only(counts=(12, 12, 10), velocity=(0.3, -1.0, 0.2))
    runs = []
    for with_stats in (False, True):
        ps, solver = _open(copy.deepcopy(sd))
        assert ps.get_option(_lib.OPT_SORT_LEAN) == 1 and ps.get_option(_lib.OPT_SORT_FAST) == 1       # the defaults
        grid = ps.sample_grid(spacing=0.02, origin=(0.08, 0.08, 0.08), shape=(14, 14, 12), fields=("velocity", "density"))
        cut = mesh.extract_raw(ps, 0.4, True)
        if with_stats:
            ps.set_statistics(every=2, **ODD)
        solver.step(5)
        solver.step(1)
        solver.step(6)
        if with_stats:
            assert ps.statistics.info().samples == 6 and ps.statistics.accumulators().n_wet.any()
        # the last sample_grid of before the run: still downloadable, unchanged, and the mesh can still be cut from it
        nodes = grid.weight.size
        weight, count, sums = np.empty(nodes, np.int64), np.empty(nodes, np.int64), np.empty((4, nodes), np.int64)
        ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)
        ps._call("sph_sample_grid_download", ptr(weight), ptr(count), ptr(sums), nodes)
        assert np.array_equal(weight, grid.weight.reshape(-1)) and np.array_equal(count, grid.count.reshape(-1))
        assert np.array_equal(sums, grid.sums.reshape(4, -1)) and weight.any()
        again = mesh.extract_raw(ps, 0.4, True)
        assert all(np.array_equal(p, q) for p, q in zip(cut, again)) and cut[2].shape[0] > 0
        assert ps.surface_mesh(spacing=0.02).vertices.shape[0] > 0
        counts = (ps.get_option(_lib.OPT_SORT_FAST_COUNT), ps.get_option(_lib.OPT_SORT_GENERAL_COUNT), ps.get_option(_lib.OPT_SORT_LEAN))
        runs.append(({n: getattr(ps, n).to_numpy().copy() for n in ("x", "v", "pid", "density", "pressure")}, counts))
        ps.close()
    (off, c_off), (on, c_on) = runs
    for n in off:
        assert off[n].tobytes() == on[n].tobytes(), n
    assert c_on == c_off and c_on[0] == 12 and c_on[2] == 1               # every step's sort the fast one, with and without; lean as requested


# ---- 5: capacity ---------------------------------------------------------------------------------------------------------------
def test_capacity():
    a, sa = _open()
    b, sb = _open()
    ta, tb = a.set_statistics(every=1, capacity=2, **ODD), b.set_statistics(every=1, **ODD)
    sa.step(4)
    sb.step(2)
    i = ta.info()
    assert (i.samples, i.dropped, i.steps_seen) == (2, 2, 4) and tb.info().samples == 2
    assert _bytes(ta.accumulators()) == _bytes(tb.accumulators()) and ta.accumulators().n_wet.max() == 2
    ta.sample()                                                            # a stand-alone sample of a full set is dropped alike
    assert (ta.info().samples, ta.info().dropped) == (2, 3) and _bytes(ta.accumulators()) == _bytes(tb.accumulators())
    a.close(); b.close()


# ---- 6: replace, reset, refusals -----------------------------------------------------------------------------------------------
def test_replace_reset_and_refusals():
    ps, solver = _open()
    with pytest.raises(_lib.SphError, match=r"sph_stats_sample.*no statistics set"):
        ps._call("sph_stats_sample")
    with pytest.raises(_lib.SphError, match=r"sph_stats_download.*no statistics set"):
        ps._call("sph_stats_download", None, None, None, None, 1)
    assert ps.statistics is None
    st = ps.set_statistics(every=1, **ODD)
    solver.step(2)
    good = st.accumulators()
    assert good.samples == 2 and good.n_wet.any()
    # refused sets: the old sums stay downloadable and unchanged, the message names the entry
    a = stats.set_args(every=1, particle_diameter=ps.particle_diameter, domain_size=ps.domain_size, **ODD)
    def params(**kw):
        p = stats.stats_params(ps, a)
        for k, v in kw.items():
            if k == "spacing":
                p.grid.spacing = (C.c_float * 3)(*v)
            elif k == "fields":
                p.grid.fields = v
            else:
                setattr(p, k, v)
        return p
    for kw, word in ((dict(every=0), "every"), (dict(spacing=(0.03, -0.02, 0.02)), "spacing"), (dict(spacing=(0.03, 0.001, 0.02)), "eighth"),
                     (dict(fields=1 | 2 | 4 | 8), "fields"), (dict(fields=1), "fields"), (dict(capacity=0), "capacity"),
                     (dict(capacity=(1 << 19) + 1), "capacity"), (dict(wet_min=-1), "wet_min")):
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*sph_stats_set.*{word}"):
            ps._call("sph_stats_set", C.byref(params(**kw)))
        assert _bytes(st.accumulators()) == _bytes(good) and st.info().samples == 2, kw
    with pytest.raises(_lib.SphError, match=r"rc=-1.*sph_stats_download.*nodes"):
        ps._call("sph_stats_download", None, None, None, None, st.nodes + 1)
    solver.step(1)                                                         # ... and the last good set goes on being sampled
    assert st.info().samples == 3 and _bytes(st.accumulators()) != _bytes(good)
    ps._call("sph_stats_set", C.byref(params(fields=0)))                    # fields 0 means the velocity too
    assert st.info().samples == 0 and not st.accumulators().n_wet.any()
    # reset keeps the set
    solver.step(1)
    assert st.info().samples == 1
    st.reset()
    i = st.info()
    assert (i.samples, i.dropped, i.steps_seen, i.shape, i.every) == (0, 0, 0, ODD["shape"], 1)
    zero = st.accumulators()
    assert not any(getattr(zero, k).any() for k in PLANES)
    st.sample()
    _same(st.accumulators(), _model_sample(model.fresh(st.nodes), ps, st), "after reset")
    # another, larger grid: the planes are allocated again and start from zero
    big = ps.set_statistics(origin=(0.05, 0.05, 0.05), spacing=0.02, shape=(16, 17, 13), every=1)
    assert big.info().samples == 0 and big.nodes == 16 * 17 * 13 and not big.accumulators().sum_w.any()
    big.sample()
    _same(big.accumulators(), _model_sample(model.fresh(big.nodes), ps, big), "larger grid")
    small = ps.set_statistics(every=1, **ODD)                               # and a smaller one in the same allocation
    small.sample()
    _same(small.accumulators(), _model_sample(model.fresh(small.nodes), ps, small), "smaller grid")
    ps.clear_statistics()
    assert ps.statistics is None
    with pytest.raises(_lib.SphError, match=r"sph_stats_download.*no statistics set"):
        ps._call("sph_stats_download", None, None, None, None, small.nodes)
    solver.step(1)
    ps.close()


# ---- 7: DFSPH ------------------------------------------------------------------------------------------------------------------
def test_dfsph_steps_are_sampled():
    ps, solver = _open(scenes.fluid_with_rigid_blocks(), dfsph=True)
    st = ps.set_statistics(origin=(0.1, 0.08, 0.1), spacing=0.025, shape=(9, 11, 7), every=1, wet=0.3)
    want = model.fresh(st.nodes)
    for k in range(3):
        want = _model_sample(want, ps, st)
        solver.step(1)
        _same(st.accumulators(), want, k)
    assert st.info().samples == 3 and st.info().steps_seen == 3 and want["n_wet"].max() == 3
    # the selection: solids of object 1 instead of the fluid
    solid = ps.set_statistics(origin=(0.1, 0.04, 0.1), spacing=0.025, shape=(9, 5, 7), every=1, wet=0.05, material="solid", objects=[1])
    f = _particles(ps)
    solver.step(1)
    _same(solid.accumulators(), _model_sample(model.fresh(solid.nodes), ps, solid, f=f, material=0, objects=(1,)), "solids")
    assert solid.accumulators().n_wet.any()
    ps.close()


# ---- 8: the Python surface -----------------------------------------------------------------------------------------------------
def test_python_surface_on_a_rigidly_moving_block(tmp_path):
    ps, solver = _open()
    v0 = np.array([0.75, -1.5, 0.25])
    ps.v.from_numpy(np.tile(v0.astype(F32), (ps.v.to_numpy().shape[0], 1)))
    st = ps.set_statistics(origin=(0.05, 0.05, 0.05), spacing=0.03, shape=(9, 11, 8), every=1)
    for _ in range(3):
        st.sample()
    acc = st.accumulators()
    wet = acc.n_wet > 0
    assert wet.sum() > 50 and (~wet).sum() > 50 and (acc.n_wet[wet] == 3).all()
    u = st.mean_velocity()
    # one Shepard ratio carries a relative error of about 2^-30 per term: 1e-6 relative is far above it
    rel = np.abs(u[wet] - v0).max() / np.linalg.norm(v0)
    r = st.reynolds_stress()
    worst = np.abs(r[wet]).max()
    print(f"mean velocity: max relative error {rel:.3e}; |R| max {worst:.3e} against the bound {1e-9 * (v0 ** 2).sum() + 2.0 ** -24:.3e}")
    assert rel <= 1e-6
    # |R| <= 1e-9 |v0|^2 + 2^-24: the product term rounds to 2^-25, the means to 2^-33 each, and every sample holds the same u
    assert worst <= 1e-9 * (v0 ** 2).sum() + 2.0 ** -24
    assert np.isnan(u[~wet]).all() and np.isnan(r[~wet]).all() and np.isnan(st.tke()[~wet]).all()
    assert np.array_equal(st.intermittency(), wet.astype(np.float64)) and np.allclose(st.rms_velocity()[wet], 0.0, atol=2.0 ** -11)
    inside = acc.n_wet.reshape(st.shape)[3:5, 4:6, 3:5]
    assert (inside == 3).all() and np.allclose(st.mean_fill()[3:5, 4:6, 3:5], 0.8, atol=0.05)
    path = str(tmp_path / "statistics.vtk")
    st.write_vtk(path)
    back = stats.read_vtk(path)
    assert back["shape"] == st.shape and np.array_equal(back["arrays"]["mean_velocity"], u.astype(F32), equal_nan=True)
    ps.close()
