"""The pure-fluid instance of the one-gather force sweep (k_gather_brick<GM_FORCE_FUSED_U, ..., FORCE_BF | DEEP | PURE_INTERNAL>):
a context without any solid particle runs the branch-free pair term WITHOUT its solid-neighbour path (compare on the record's
sign word, accept test, dependent aux load, 64-bit atomics, the self test that only that path read).  The fluid term is the same
expression tree on the same operand values, so every field must be BIT-identical to the general instance
(SPH_OPT_PURE_FLUID_INSTANCE 0, the A/B switch that turns the density sweep's and the force sweep's instance off together),
and a context that holds -- or receives -- a solid particle must run the general instance.

sph_get_option(SPH_OPT_PURE_FLUID_INSTANCE) reports the REQUESTED value (0 / 1 / 2), not which instance the launcher took:
selection is therefore checked through the results -- the pure instance evaluates a solid neighbour's record (4th word = -m_V)
with the fluid formula, so a wrong selection cannot reproduce the general instance's bits -- together with
SPH_OPT_UNIFORM_FLUID_STATE == 1 (the one-gather sweep, whose two instances are compared, is what runs)."""
import copy

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

FIELDS = ("x", "v", "density", "pressure", "acceleration")
STEPS = 25


def _bits(a):
    """== on the bit patterns: no tolerance, and a NaN or a signed zero cannot hide a difference."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _run(sd, arrays, pure, steps=STEPS, midway=None):
    """One trajectory from the given upload with SPH_OPT_PURE_FLUID_INSTANCE = pure; midway(ps) is called after the first
    half of the steps.  Returns the fields by persistent id, the list statistics of the last step and the uniform-fluid state."""
    from sph_taichi_amd import _lib
    ps, solver = scenes.make_ps(sd, arrays)
    assert ps.get_option(_lib.OPT_PURE_FLUID_INSTANCE) == 1      # the default
    ps.set_option(_lib.OPT_PURE_FLUID_INSTANCE, pure)
    assert ps.get_option(_lib.OPT_PURE_FLUID_INSTANCE) == pure
    assert ps.get_option(_lib.OPT_KERNEL_VARIANT) == _lib.VAR_DEFAULT   # the force loop the pure instance exists for
    solver.initialize()
    if midway is None:
        solver.step(steps)
    else:
        solver.step(steps // 2)
        midway(ps)
        solver.step(steps - steps // 2)
    st = _lib.SphStats()
    ps._call("sph_get_stats", st)
    out = {n: scenes.ps_by_pid(ps, n) for n in FIELDS}
    state = ps.get_option(_lib.OPT_UNIFORM_FLUID_STATE)
    ps.close()
    return out, st, state


def _assert_identical(a, b, what):
    for n in FIELDS:
        assert np.isfinite(a[n]).all(), f"{what}: {n} is not finite"
        assert np.array_equal(_bits(a[n]), _bits(b[n])), \
            f"{what}: {n} differs between the pure-fluid and the general instance in {int((_bits(a[n]) != _bits(b[n])).sum())} words"


def test_pure_force_instance_is_bit_identical_in_a_small_tank():
    """20 x 20 x 20 particles in a tank little larger than the block, thrown into the corner: floor and two walls are reached
    within the first steps, cells fill unevenly (1 .. 20 and more particles per cell) as the block is compressed against them."""
    sd = scenes.fluid_only(counts=(20, 20, 20), start=(0.045, 0.045, 0.045), velocity=(-1.0, -1.5, -1.0), domain_end=(0.56, 0.6, 0.56))
    cfg, sc = scenes.build(sd)
    scenes.jitter(sc, 0.1, seed=21)
    on, st, state = _run(sd, sc.arrays, 1)
    off, _, state_off = _run(sd, sc.arrays, 0)
    assert state == 1 and state_off == 1
    assert st.targets == 8000
    _assert_identical(on, off, "small tank")
    # the scene does what it is for: the block has met the floor and both walls
    pad = np.float32(sc.geom.padding)
    assert all((on["x"][:, a] <= pad * np.float32(1.0001)).any() for a in range(3))


def _ragged(velocity=(0.3, -0.2, 0.1)):
    # a lattice whose nodes sit on cell faces: run lengths 1 .. 27 per cell (the benchmark's initial state)
    sd = scenes.fluid_only(counts=(18, 14, 16), start=(0.04, 0.04, 0.04), velocity=velocity)
    cfg, sc = scenes.build(sd)
    return sd, sc


def test_pure_force_instance_with_a_target_in_flat_cell_0():
    """The reference's max(0, idx-1) quirk: flat cell 0's own range is never visited, so a target that lives there never
    meets itself in its list -- the one case in which the self test of the general instance mattered, and only on the solid
    path.  The fluid term needs no such test (r = 0 multiplies finite coefficients by 0)."""
    sd, sc = _ragged()
    x = sc.arrays["x"]
    x[0] = (0.03, 0.03, 0.03)            # inside flat cell 0 ((0.04)^3 at the domain's origin), 0.017 from the lattice's corner node
    sc.arrays["x_0"] = x.copy()
    g = sc.geom
    assert (np.floor(x[0] / np.float32(g.grid_size)) == 0).all()
    on, _, state = _run(sd, sc.arrays, 1)
    off, _, _ = _run(sd, sc.arrays, 0)
    assert state == 1
    _assert_identical(on, off, "flat cell 0")
    one_on, _, _ = _run(sd, sc.arrays, 1, steps=1)     # ... and after the one step in which that cell is certainly occupied
    one_off, _, _ = _run(sd, sc.arrays, 0, steps=1)
    _assert_identical(one_on, one_off, "flat cell 0, first step")
    assert np.abs(one_on["acceleration"][0]).max() > 0.0


def test_pure_force_instance_beside_the_exact_fallback():
    """216 particles packed at 0.66 d (3.5 x the lattice's number density) away from the block: their lists outgrow the 95-entry
    cap, so those targets take the per-target exact cell walk (the general pair term) inside the same launch in which every
    other target runs the pure instance's list loop."""
    sd, sc = _ragged(velocity=(0.2, -0.3, 0.1))
    sd["Configuration"]["stiffness"] = 200.0            # keeps the packed cluster's expansion gentle
    cfg, sc = scenes.build(sd)
    x = sc.arrays["x"]
    i, j, k = np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij")
    x[:216] = (np.array([0.5, 0.5, 0.3]) + 0.0132 * np.stack([i, j, k], -1).reshape(-1, 3)).astype(np.float32)
    sc.arrays["x_0"] = x.copy()
    one_on, st, state = _run(sd, sc.arrays, 1, steps=1)
    assert state == 1
    # (a CPU count of the packed lattice: 32 of its particles have more than 95 others within h)
    assert 0 < st.list_overflow_targets < 216 and st.lds_overflow_targets == 0, (st.list_overflow_targets, st.lds_overflow_targets)
    one_off, _, _ = _run(sd, sc.arrays, 0, steps=1)
    _assert_identical(one_on, one_off, "list overflow, first step")
    on, _, _ = _run(sd, sc.arrays, 1)
    off, _, _ = _run(sd, sc.arrays, 0)
    _assert_identical(on, off, "list overflow")


def test_a_scene_with_one_static_solid_runs_the_general_instance():
    """One static solid particle next to the fluid: the uniform-fluid step still runs (one-gather force sweep), but never its
    pure-fluid instances -- the results are those of the A/B switch's general path, bit for bit, and the fluid feels the solid."""
    from sph_taichi_amd import _lib
    sd = scenes.fluid_only(counts=(12, 10, 12), start=(0.1, 0.1, 0.1), velocity=(0.4, -0.6, 0.2))
    solid = (0.1 + 5 * 0.02, 0.1 - 0.02, 0.1 + 5 * 0.02)       # one lattice spacing under the block's floor layer
    sd["RigidBlocks"] = [scenes._block(1, solid, scenes.lattice_end(solid, (1, 1, 1)), isDynamic=False, color=(255, 255, 255))]
    cfg, sc = scenes.build(sd)
    assert int((sc.arrays["material"] == 0).sum()) == 1
    on, st, state = _run(sd, sc.arrays, 1)
    off, _, state_off = _run(sd, sc.arrays, 0)
    assert state == 1 and state_off == 1
    assert st.targets == 12 * 10 * 12
    _assert_identical(on, off, "one static solid")
    # the solid is really felt: the same fluid without it moves differently
    sd0 = copy.deepcopy(sd)
    del sd0["RigidBlocks"]
    cfg0, sc0 = scenes.build(sd0)
    alone, _, _ = _run(sd0, sc0.arrays, 1)
    fluid = sc.arrays["material"] == 1
    assert not np.array_equal(on["x"][fluid], alone["x"])


def test_a_solid_that_arrives_in_a_running_context_drops_the_instance():
    """A pure-fluid context runs the instance for 12 steps; then one particle in the middle of the block becomes a static solid
    (material / is_dynamic uploaded, as an insert does).  The upload asks for a new device-side check, which no longer finds the
    context solid-free: from the next step on the general instance runs -- a pure instance kept by mistake would evaluate the new
    solid's record with the fluid formula and leave other bits than the A/B switch's general path."""
    from sph_taichi_amd import _lib
    sd = scenes.fluid_only(counts=(12, 10, 12), start=(0.1, 0.1, 0.1), velocity=(0.4, -0.6, 0.2))
    cfg, sc = scenes.build(sd)
    victim = (5 * 10 + 4) * 12 + 6        # persistent id of an interior lattice node

    def solidify(ps):
        at = int(np.nonzero(ps.pid.to_numpy() == victim)[0][0])
        for name in ("material", "is_dynamic"):
            a = getattr(ps, name).to_numpy()
            a[at] = 0
            getattr(ps, name).from_numpy(a)
        assert ps.get_option(_lib.OPT_UNIFORM_FLUID_STATE) == -1     # undecided until the next step's check

    on, st, state = _run(sd, sc.arrays, 1, midway=solidify)
    off, _, state_off = _run(sd, sc.arrays, 0, midway=solidify)
    assert state == 1 and state_off == 1
    assert st.targets == 12 * 10 * 12 - 1
    _assert_identical(on, off, "solid inserted mid-run")
    untouched, _, _ = _run(sd, sc.arrays, 1)
    assert not np.array_equal(on["x"], untouched["x"])
