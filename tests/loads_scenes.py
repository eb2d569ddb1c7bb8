"""Scenes of the fluid-load tests (tests/test_loads_host.py, tests/test_gpu_loads.py): domain (1.0, 1.2, 0.8), diameter 0.02,
fluid blocks of at most 12^3 and at most 600 solid particles.  A lattice at rest spacing has a density at or below density0 next to a
boundary, which the equation of state clamps to zero pressure -- and zero load; `squeeze` therefore draws the fluid's lattice together
(about 1.37 x density0 at factor 0.9) and jitters it, which also takes the positions off the cell boundaries."""
import copy

import numpy as np

from tests import scenes

F32 = np.float32


def block_on_slab(fluid_counts=(6, 6, 6), slab_counts=(8, 2, 8)):
    """One fluid block resting on one static slab (object 1): a few hundred particles."""
    slab_start = (0.10, 0.06, 0.10)
    fluid_start = (0.12, 0.06 + slab_counts[1] * 0.02, 0.12)
    return {"Configuration": copy.deepcopy(scenes.BASE_CFG),
            "FluidBlocks": [scenes._block(0, fluid_start, scenes.lattice_end(fluid_start, fluid_counts), (0.0, -0.5, 0.0))],
            "RigidBlocks": [scenes._block(1, slab_start, scenes.lattice_end(slab_start, slab_counts), isDynamic=False, color=(255, 255, 255))]}


def cube_scene():
    """Fluid ON (6 x 5 x 6) and BESIDE (5 x 10 x 6) a static cube of 6^3 (object 1, selected), a static slab under the side fluid
    (object 2, not selected) and a small static block far from any fluid (object 3, selected and dry): 371 solid, 480 fluid particles."""
    cube = (0.30, 0.10, 0.30)
    top = (0.30, 0.10 + 6 * 0.02, 0.30)
    side = (0.30 + 6 * 0.02, 0.10, 0.30)
    slab = (0.40, 0.06, 0.28)
    far = (0.70, 0.80, 0.50)
    rigid = lambda oid, start, counts: scenes._block(oid, start, scenes.lattice_end(start, counts), isDynamic=False, color=(255, 255, 255))
    return {"Configuration": copy.deepcopy(scenes.BASE_CFG),
            "FluidBlocks": [scenes._block(0, top, scenes.lattice_end(top, (6, 5, 6)), (0.0, -0.5, 0.0)),
                            scenes._block(0, side, scenes.lattice_end(side, (5, 10, 6)), (-0.3, -0.5, 0.0))],
            "RigidBlocks": [rigid(1, cube, (6, 6, 6)), rigid(2, slab, (8, 2, 8)), rigid(3, far, (3, 3, 3))]}


def corner_scene():
    """Targets in the first and the last cell layer of every axis: two solid objects interleaved cell by cell in the low corner (so a
    wave of four targets holds both), one in the high corner, each with fluid beside it.  27 + 18 + 12 = 57 solid particles, most of
    them outside the padding (nothing is advected in the test that uses this scene)."""
    lo_a, lo_b = (0.005, 0.005, 0.005), (0.005, 0.065, 0.005)
    hi = (0.945, 1.145, 0.745)
    rigid = lambda oid, start, counts: scenes._block(oid, start, scenes.lattice_end(start, counts), isDynamic=False, color=(255, 255, 255))
    f_lo, f_hi = (0.065, 0.005, 0.005), (0.865, 1.105, 0.705)
    return {"Configuration": copy.deepcopy(scenes.BASE_CFG),
            "FluidBlocks": [scenes._block(0, f_lo, scenes.lattice_end(f_lo, (4, 6, 4)), (0.0, 0.0, 0.0)),
                            scenes._block(0, f_hi, scenes.lattice_end(f_hi, (4, 4, 4)), (0.0, 0.0, 0.0))],
            "RigidBlocks": [rigid(1, lo_a, (3, 3, 3)), rigid(2, lo_b, (3, 2, 3)), rigid(3, hi, (3, 2, 2))]}


def squeeze(sc, factor=0.9, seed=0, amplitude=0.1, toward=None):
    """The fluid of a built scene drawn together by `factor` about `toward` (default: the fluid's lowest corner) and jittered by
    +- amplitude * diameter; x_0 follows.  In place; returns the scene."""
    a = sc.arrays
    fluid = a["material"] == 1
    x = a["x"].astype(np.float64)
    anchor = x[fluid].min(axis=0) if toward is None else np.asarray(toward, dtype=np.float64)
    rng = np.random.default_rng(seed)
    d = sc.geom.particle_diameter
    x[fluid] = anchor + (x[fluid] - anchor) * factor + rng.uniform(-amplitude * d, amplitude * d, size=(int(fluid.sum()), 3))
    a["x"] = x.astype(F32)
    a["x_0"] = a["x"].copy()
    return sc
