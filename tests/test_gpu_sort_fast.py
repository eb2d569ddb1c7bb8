"""SPH_OPT_SORT_FAST: the sort at the head of a step ranks the particles that stay in their cell from the previous order
(sph_sort.hip, rule in tests/sort_rank_model.py).  It must leave exactly the general sort's order: with the option on and
off, pid, x, v, density and pressure are compared bit for bit after EVERY step, in the current order (so a wrong rank shows
as a wrong pid at once, not only as a different sum a step later).  Which path ran is read from the context's counters
(SPH_OPT_SORT_FAST_COUNT / SPH_OPT_SORT_GENERAL_COUNT)."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

FIELDS = ("pid", "grid_ids", "x", "v", "density", "pressure")
TPB = 256   # the scatter's workgroup


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _counts(ps):
    from sph_taichi_amd import _lib
    return ps.get_option(_lib.OPT_SORT_FAST_COUNT), ps.get_option(_lib.OPT_SORT_GENERAL_COUNT)


def _trajectory(sd, arrays, fast, steps, events=None):
    """Fields in the current order after every step, the (fast, general) sort counts after every step, the stats after the
    last one.  events: {step index: f(ps)} called before that step."""
    from sph_taichi_amd import _lib
    ps, solver = scenes.make_ps(sd, arrays)
    ps.set_option(_lib.OPT_SORT_FAST, fast)
    assert ps.get_option(_lib.OPT_SORT_FAST) == fast      # the requested value
    solver.initialize()
    frames, counts, occ = [], [_counts(ps)], []
    for it in range(steps):
        if events and it in events:
            events[it](ps)
        solver.step(1)
        frames.append({n: getattr(ps, n).to_numpy().copy() for n in FIELDS})
        counts.append(_counts(ps))
        st = _lib.SphStats()
        ps._call("sph_get_stats", st)
        occ.append(int(st.max_cell_occupancy))
    ps.close()
    return frames, counts, occ


def _assert_same(on, off, what):
    assert len(on) == len(off)
    for it, (a, b) in enumerate(zip(on, off)):
        for n in FIELDS:
            assert np.array_equal(_bits(a[n]), _bits(b[n])), \
                f"{what}: {n} differs after step {it + 1} in {int((_bits(a[n]) != _bits(b[n])).sum())} words"


def _movers(frames):
    """per step, the signed cell-id change of every particle that changed cell (by persistent id)"""
    out = []
    for a, b in zip(frames[:-1], frames[1:]):
        ka = np.empty_like(a["grid_ids"]); ka[a["pid"]] = a["grid_ids"]
        kb = np.empty_like(b["grid_ids"]); kb[b["pid"]] = b["grid_ids"]
        d = kb.astype(np.int64) - ka
        out.append(d[d != 0])
    return out


def _all_fast_after_first(counts):
    f0, g0 = counts[0]
    assert f0 == 0 and g0 >= 1                       # initialize(): the general sort
    return all(c == (f0 + k, g0) for k, c in enumerate(counts))


def _straddles(keys):
    """some cell's segment begins before a workgroup boundary of the scatter and goes on behind it"""
    b = np.arange(TPB, len(keys), TPB)
    return bool(np.any(keys[b - 1] == keys[b]))


def test_falling_block_movers_in_one_direction():
    sd = scenes.fluid_only(counts=(13, 17, 11), start=(0.1, 0.3, 0.1), velocity=(0.0, -3.0, 0.0))
    cfg, sc = scenes.build(sd)
    scenes.jitter(sc, 0.1, seed=3)
    n = sc.arrays["x"].shape[0]
    assert n == 13 * 17 * 11 and n % TPB != 0
    on, c_on, _ = _trajectory(sd, sc.arrays, 1, 40)
    off, c_off, _ = _trajectory(sd, sc.arrays, 0, 40)
    _assert_same(on, off, "falling block")
    assert _all_fast_after_first(c_on)
    assert all(c[0] == 0 for c in c_off) and c_off[-1][1] == c_off[0][1] + 40
    mv = np.concatenate(_movers(on))
    assert len(mv) > 200 and (mv < 0).sum() > 10 * (mv > 0).sum()      # many movers, nearly all downwards
    assert all(_straddles(f["grid_ids"]) for f in on)                   # segments across workgroup boundaries, every step


def test_sloshing_block_movers_in_both_directions():
    sd = scenes.fluid_only(counts=(15, 9, 13), start=(0.2, 0.1, 0.2), velocity=(0.0, 0.0, 0.0))
    cfg, sc = scenes.build(sd)
    scenes.jitter(sc, 0.1, seed=4)
    v = sc.arrays["v"]
    layer = (np.arange(v.shape[0]) // 13) % 2                            # alternate z rows stream against each other in x and z
    v[:, 0] = np.where(layer == 0, 2.0, -2.0)
    v[:, 2] = np.where(layer == 0, -1.5, 1.5)
    n = v.shape[0]
    assert n % TPB != 0
    on, c_on, _ = _trajectory(sd, sc.arrays, 1, 40)
    off, _, _ = _trajectory(sd, sc.arrays, 0, 40)
    _assert_same(on, off, "sloshing block")
    assert _all_fast_after_first(c_on)
    mv = np.concatenate(_movers(on))
    assert (mv > 0).sum() > 100 and (mv < 0).sum() > 100
    per_step = [((m > 0).any() and (m < 0).any()) for m in _movers(on)]
    assert sum(per_step) > 10                                            # both directions inside one sort


def test_pile_up_with_a_cell_of_more_than_64_members():
    """343 particles inside ONE cell next to a small block, under a soft linear equation of state: the cell's segment is longer
    than a workgroup of the scatter plus a wave, so some workgroup boundary lies more than 64 records behind its start -- the
    stretch the whole wave counts."""
    sd = scenes.fluid_only(counts=(9, 8, 7), start=(0.1, 0.1, 0.1), velocity=(0.0, -0.5, 0.0))
    sd["Configuration"]["stiffness"] = 50.0
    sd["Configuration"]["exponent"] = 1
    cfg, sc = scenes.build(sd)
    scenes.jitter(sc, 0.1, seed=5)
    x = sc.arrays["x"]
    i, j, k = np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij")
    x[:343] = (np.array([0.482, 0.482, 0.482]) + 0.005 * np.stack([i, j, k], -1).reshape(-1, 3)).astype(np.float32)
    sc.arrays["x_0"] = x.copy()
    g = np.float32(sc.geom.grid_size)
    assert len(np.unique(np.floor(x[:343] / g), axis=0)) == 1
    on, c_on, occ = _trajectory(sd, sc.arrays, 1, 30)
    off, _, _ = _trajectory(sd, sc.arrays, 0, 30)
    _assert_same(on, off, "pile-up")
    assert _all_fast_after_first(c_on)
    assert all(np.isfinite(f["x"]).all() for f in on)
    crowded_steps = [it for it, o in enumerate(occ) if o > 64]
    assert len(crowded_steps) >= 3, occ                                  # (sph_get_stats: the fullest cell of the step's sort)
    # and in at least one FAST sort a crowded segment starts more than a wave before a workgroup boundary inside it
    far = 0
    for it in crowded_steps:
        keys = on[it]["grid_ids"]       # the order this step's sort left = the old order of the next step's fast sort
        b = np.arange(TPB, len(keys), TPB)
        start = np.searchsorted(keys, keys[b], side="left")
        far += int(np.any((keys[b - 1] == keys[b]) & (b - start > 64))) if it + 1 < len(on) else 0
    assert far >= 2


def test_fallbacks_take_the_general_sort_once_and_rearm():
    from sph_taichi_amd import _lib
    sd = scenes.fluid_only(counts=(11, 13, 9), start=(0.1, 0.2, 0.1), velocity=(0.5, -2.0, 0.3))
    cfg, sc = scenes.build(sd)
    scenes.jitter(sc, 0.1, seed=6)

    def upload_x(ps):
        x = ps.x.to_numpy()
        x[:, 0] += np.float32(0.011)                   # a shift of a quarter cell: many particles change cell at once
        ps.x.from_numpy(x)

    def insert(ps):                                    # the records of the set are (re)seated from the host
        n = ps.count()
        ps._call("sph_set_particle_count", n)
        ps.x.from_numpy(ps.x.to_numpy())

    def stand_alone_sort(ps):
        ps._call("sph_sort")

    def by_pid_on(ps):
        ps.set_option(_lib.OPT_SORT_BY_PID, 1)

    def by_pid_off(ps):
        ps.set_option(_lib.OPT_SORT_BY_PID, 0)

    events = {5: upload_x, 10: insert, 15: stand_alone_sort, 20: by_pid_on, 23: by_pid_off}
    on, c_on, _ = _trajectory(sd, sc.arrays, 1, 30, events)
    off, c_off, _ = _trajectory(sd, sc.arrays, 0, 30, events)
    _assert_same(on, off, "fallbacks")
    assert all(c[0] == 0 for c in c_off)
    # counts[k] = after k steps; the step with index k is the transition counts[k] -> counts[k + 1]
    path = []
    for k in range(30):
        df, dg = c_on[k + 1][0] - c_on[k][0], c_on[k + 1][1] - c_on[k][1]
        path.append((df, dg))
    want = {k: (1, 0) for k in range(30)}
    want[5] = (0, 1)            # after the upload
    want[10] = (0, 1)           # after the insert
    want[15] = (1, 1)           # sph_sort itself is a general sort; the step's own sort behind it is armed again
    for k in (20, 21, 22):
        want[k] = (0, 1)        # sort_by_pid on
    assert path == [want[k] for k in range(30)], path
