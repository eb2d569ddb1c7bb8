"""SPH_OPT_SORT_LEAN: on the pure-fluid uniform step the fast scatter moves the persistent id alone, through an array of its own,
and the (m, density, pressure, id) record is written back when somebody asks (sph_sort.hip, sph_derived.h).  Nothing a caller
can read may differ from the run that moves the record in every sort: two contexts, the option 0 and 1, are compared bit for bit
after every call, in the current order -- a lost or misplaced id shows as a wrong pid at once.

The scene is a tank of 12,000 fluid particles (47 workgroups of the scatter) under a soft linear equation of state, streaming
obliquely, with 343 of them packed into one cell: cells' segments cross workgroup boundaries, a few hundred particles change
cell in every step, and the crowded cell takes the path the whole wave ranks."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

FIELDS = ("x", "v", "density", "pressure", "pid", "m", "grid_ids", "grid_particles_num")
CALLS = (1,) * 10 + (3,) * 5 + (7,)
TPB = 256   # the scatter's workgroup


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _tank(rigid=False):
    sd = scenes.fluid_only(counts=(24, 25, 20), start=(0.1, 0.1, 0.1), velocity=(0.5, -2.0, 0.3))
    sd["Configuration"]["stiffness"] = 50.0
    sd["Configuration"]["exponent"] = 1
    if rigid:   # one static slab beside the fluid
        s0 = (0.7, 0.1, 0.1)
        sd["RigidBlocks"] = [scenes._block(1, s0, scenes.lattice_end(s0, (3, 4, 5)), isDynamic=False, color=(255, 255, 255))]
    cfg, sc = scenes.build(sd)
    scenes.jitter(sc, 0.1, seed=11)
    x = sc.arrays["x"]
    i, j, k = np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij")
    x[:343] = (np.array([0.482, 0.482, 0.482]) + 0.005 * np.stack([i, j, k], -1).reshape(-1, 3)).astype(np.float32)
    sc.arrays["x_0"] = x.copy()
    assert len(np.unique(np.floor(x[:343] / np.float32(sc.geom.grid_size)), axis=0)) == 1
    return sd, sc


@pytest.fixture(scope="module")
def tank():
    sd, sc = _tank()
    assert sc.arrays["x"].shape[0] == 12000 and 12000 % TPB != 0
    return sd, sc


def _open(sd, sc, lean, options=()):
    from sph_taichi_amd import _lib
    ps, solver = scenes.make_ps(sd, sc.arrays)
    ps.set_option(_lib.OPT_SORT_LEAN, lean)
    assert ps.get_option(_lib.OPT_SORT_LEAN) == lean      # the requested value
    for opt, value in options:
        ps.set_option(opt, value)
    solver.initialize()
    return ps, solver


def _frame(ps, fields=FIELDS):
    return {n: getattr(ps, n).to_numpy().copy() for n in fields}


def _counts(ps):
    from sph_taichi_amd import _lib
    return ps.get_option(_lib.OPT_SORT_FAST_COUNT), ps.get_option(_lib.OPT_SORT_GENERAL_COUNT)


def _same(a, b, what):
    assert a.keys() == b.keys()
    for n in a:
        assert a[n].shape == b[n].shape and np.array_equal(_bits(a[n]), _bits(b[n])), \
            f"{what}: {n} differs in {int((_bits(a[n]) != _bits(b[n])).sum())} words"


def _pair(sd, sc, calls, events=None, options=(), fields=FIELDS):
    """The same calls on a context with the option off and one with it on; every field compared after every call.  events:
    {call index: f(ps)} run before that call.  Returns the lean context's frames and both contexts' sort counts."""
    runs = []
    for lean in (0, 1):
        ps, solver = _open(sd, sc, lean, options)
        frames = []
        for k, n in enumerate(calls):
            if events and k in events:
                events[k](ps)
            solver.step(n)
            frames.append(_frame(ps, fields))
        runs.append((frames, _counts(ps)))
        ps.close()
    (off, c_off), (on, c_on) = runs
    for k, (a, b) in enumerate(zip(off, on)):
        _same(a, b, f"call {k} (step({calls[k]}))")
    return on, c_off, c_on


def test_ab_identity(tank):
    sd, sc = tank
    on, c_off, c_on = _pair(sd, sc, CALLS)
    steps = sum(CALLS)
    assert c_on == c_off == (steps, 1)                       # initialize() is the general sort, every step's the fast one: in both
    # the scene does what it is for
    straddle, crowded, movers = 0, 0, []
    for a, b in zip(on[:-1], on[1:]):
        keys = a["grid_ids"]
        edge = np.arange(TPB, len(keys), TPB)
        straddle += bool(np.any(keys[edge - 1] == keys[edge]))
        occ = np.diff(a["grid_particles_num"], prepend=0)
        crowded += int(occ.max() > 64)
        ka = np.empty_like(a["grid_ids"]); ka[a["pid"]] = a["grid_ids"]
        kb = np.empty_like(b["grid_ids"]); kb[b["pid"]] = b["grid_ids"]
        movers.append(int((ka != kb).sum()))
    assert straddle == len(on) - 1 and crowded >= 3, (straddle, crowded)
    assert min(movers[:9]) >= 24, movers                      # dozens of particles change cell in every single step
    for f in on:
        assert np.array_equal(np.sort(f["pid"]), np.arange(12000)) and np.isfinite(f["x"]).all()
        assert len(np.unique(_bits(f["m"]))) == 1


def test_pid_read_through_a_download_after_a_lean_sort(tank):
    sd, sc = tank
    got = []
    for lean in (0, 1):
        ps, solver = _open(sd, sc, lean)
        solver.step(2)
        solver.step(9)                                        # (the second call's last sort finds the ids apart)
        got.append((ps.pid.to_numpy().copy(), ps.x.to_numpy().copy()))
        ps.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    assert not np.array_equal(got[1][0], np.arange(12000))    # (the order really has changed since the upload)


def test_pid_read_through_the_particle_export_after_a_lean_sort(tank):
    sd, sc = tank
    rows = []
    for lean in (0, 1):
        ps, solver = _open(sd, sc, lean)
        solver.step(2)
        solver.step(9)
        e = ps.export_particles(fields=("velocity", "mass", "id"), every=3, phase=1)
        rows.append(e.data.copy())
        again = ps.export_particles(fields=("density", "pressure", "id"))     # ... and the fold's other half behind it
        rows.append(again.data.copy())
        ps.close()
    assert rows[0].shape[0] == 4000 and np.array_equal(rows[0]["id"], np.arange(1, 12000, 3))
    assert rows[0].tobytes() == rows[2].tobytes() and rows[1].tobytes() == rows[3].tobytes()


def test_a_static_solid_from_the_start_keeps_the_general_scatter():
    sd, sc = _tank(rigid=True)
    assert (sc.arrays["material"] == 0).sum() == 60
    on, c_off, c_on = _pair(sd, sc, (1, 1, 4, 1))
    assert c_on == c_off and c_on[0] >= 1                    # (the fast sort itself stays eligible beside a static solid)
    assert np.array_equal(np.sort(on[-1]["pid"]), np.arange(12060))


def test_a_solid_arriving_in_a_running_context(tank):
    """200 particles of the running (lean) context are declared static solids from the host: the record comes back whole --
    ids, masses -- before the upload touches it, and the steps behind it move it again."""
    sd, sc = tank

    def freeze(ps):
        pid = ps.pid.to_numpy()
        for name in ("material", "is_dynamic"):
            a = getattr(ps, name).to_numpy()
            a[(pid >= 3000) & (pid < 3200)] = 0
            getattr(ps, name).from_numpy(a)
        v = ps.v.to_numpy()
        v[(pid >= 3000) & (pid < 3200)] = 0.0
        ps.v.from_numpy(v)

    fields = FIELDS + ("material", "m_V")
    on, c_off, c_on = _pair(sd, sc, (3, 2, 1, 4, 1), events={2: freeze}, fields=fields)
    assert c_on == c_off
    last = on[-1]
    assert np.array_equal(np.sort(last["pid"]), np.arange(12000))
    assert np.array_equal(np.sort(last["pid"][last["material"] == 0]), np.arange(3000, 3200))


def test_an_upload_of_m_between_two_step_calls_is_honoured(tank):
    sd, sc = tank

    def lighter(ps):
        m = ps.m.to_numpy()
        ps.m.from_numpy((m * np.float32(0.75)).astype(np.float32))

    def one_heavier(ps):                                      # no longer one mass: the uniform-fluid step is off after this
        m = ps.m.to_numpy()
        m[ps.pid.to_numpy() == 77] *= np.float32(1.5)
        ps.m.from_numpy(m)

    on, c_off, c_on = _pair(sd, sc, (3, 2, 2, 1, 2), events={1: lighter, 3: one_heavier})
    assert c_on == c_off
    m0 = np.float32(on[0]["m"][0])
    assert np.all(on[0]["m"] == m0) and np.all(on[1]["m"] == np.float32(m0 * np.float32(0.75))) and np.all(on[2]["m"] == on[1]["m"])
    heavy = on[-1]["m"] != on[1]["m"][0]
    assert heavy.sum() == 1 and on[-1]["pid"][heavy][0] == 77


@pytest.mark.parametrize("option", ["sort_by_pid", "drop_outside"])
def test_sort_by_pid_and_drop_outside_keep_their_path(tank, option):
    from sph_taichi_amd import _lib
    sd, sc = tank
    opt = {"sort_by_pid": _lib.OPT_SORT_BY_PID, "drop_outside": _lib.OPT_SLAB_DROP_OUTSIDE}[option]
    on, c_off, c_on = _pair(sd, sc, (2, 1, 3), options=((opt, 1),))
    assert c_on == c_off == (0, 7)                            # neither may take the fast sort, so neither scatter is the lean one
    # ... and switched on and off again in a run that was lean before
    events = {1: lambda ps: ps.set_option(opt, 1), 3: lambda ps: ps.set_option(opt, 0)}
    on, c_off, c_on = _pair(sd, sc, (3, 2, 1, 3, 1), events=events)
    assert c_on == c_off and c_on[1] >= 1 + 3


def test_with_tracers_in_the_step(tank):
    """The in-step consumer the step loop has for a pure fluid: a registered tracer set advances behind every sort."""
    sd, sc = tank
    rng = np.random.default_rng(3)
    x = sc.arrays["x"]
    pts = np.concatenate([x[rng.choice(x.shape[0], 40, replace=False)],
                          rng.uniform(x.min(axis=0) - 0.03, x.max(axis=0) + 0.03, size=(23, 3)).astype(np.float32)]).astype(np.float32)
    states, frames = [], []
    for lean, with_tracers in ((0, False), (0, True), (1, True)):
        ps, solver = _open(sd, sc, lean)
        tr = ps.set_tracers(pts) if with_tracers else None
        out = []
        for n in (1, 4, 1, 6):
            solver.step(n)
            out.append(_frame(ps))
        frames.append(out)
        if tr is not None:
            s = tr.state()
            states.append(b"".join(np.ascontiguousarray(s[k]).tobytes() for k in sorted(s)))
            assert tr.info().advances == 12
        ps.close()
    for k in range(4):
        _same(frames[0][k], frames[1][k], f"tracers on / off, call {k}")
        _same(frames[1][k], frames[2][k], f"tracers on, lean off / on, call {k}")
    assert states[0] == states[1]
