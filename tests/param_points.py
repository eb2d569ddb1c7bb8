"""Parameter points away from scenes.BASE_CFG and the radius-scaled scenes the parity tests run at them.

A point changes only what its entry lists against BASE_CFG ("all_off" combines six of them).  `cfg` overrides the scene's
Configuration, `fluid_rho` / `body_rho` the densities of the fluid blocks and of the dynamic body, `attrs` are SOLVER
ATTRIBUTES (sph_base.py:15, WCSPH.py:15: not in the scene file) set on the solver object after build_solver() and handed
to the oracle and the brute force in `params`.

Every scene is laid out in units of the particle diameter d = 2 r, starts at least one cell (2 d) inside the high faces of
the grid (the reference's neighbour lookup aliases there, and the gridless brute force cannot follow it), and is jittered.
The fluid lattice is squeezed towards its foot (spacing q d, q < 1): a d-spaced lattice holds 0.8 rho0, so without the
squeeze the clamp max(rho, rho0) would leave the pressure zero and the equation of state untested.
"""
from __future__ import annotations

import copy

import numpy as np

import scenes

R_LARGE = {"particleRadius": 0.025, "domainEnd": [1.0, 1.2, 0.8]}        # 10 x 12 x 8 cells
R_SMALL = {"particleRadius": 0.004, "domainEnd": [0.30, 0.25, 0.20]}     # 19 x 16 x 13 cells: a multiple of no brick shape
G_OBLIQUE = [3.0, -7.0, 5.0]

POINTS = {
    "r_large": dict(cfg=R_LARGE),
    "r_small": dict(cfg=R_SMALL),
    "rho_heavy": dict(cfg={"density0": 13600}, fluid_rho=13600.0, body_rho=20000.0),
    "rho_light": dict(cfg={"density0": 1.2}, fluid_rho=1.2, body_rho=0.5),
    # integer exponents (the multiply loop of sph_tait_pow covers 1..32): stiffness * exponent <= 3.5e5, the default point's
    "exp_1": dict(cfg={"exponent": 1}),
    "exp_2": dict(cfg={"exponent": 2}),
    "exp_32": dict(cfg={"exponent": 32, "stiffness": 10000}),
    "exp_33": dict(cfg={"exponent": 33, "stiffness": 10000}),            # the first integer that leaves the loop
    "exp_1p5": dict(cfg={"exponent": 1.5}),
    "exp_7p5": dict(cfg={"exponent": 7.5, "stiffness": 50000}),
    "stiff_lo": dict(cfg={"stiffness": 500}),
    "stiff_hi": dict(cfg={"stiffness": 5e6, "timeStepSize": 4e-5}),
    "g_oblique": dict(cfg={"gravitation": G_OBLIQUE}),
    "g_zero": dict(cfg={"gravitation": [0.0, 0.0, 0.0]}),
    "visc_0": dict(attrs={"viscosity": 0.0}),
    "visc_hi": dict(attrs={"viscosity": 0.5}),
    "st_0": dict(attrs={"surface_tension": 0.0}),
    "st_hi": dict(attrs={"surface_tension": 1.0}),
    "dt_small": dict(cfg={"timeStepSize": 1e-5}),
    "dt_large": dict(cfg={"timeStepSize": 2e-3, "stiffness": 500}),
    "all_off": dict(cfg=dict(R_LARGE, density0=13600, exponent=1.5, gravitation=G_OBLIQUE), fluid_rho=13600.0,
                    body_rho=20000.0, attrs={"viscosity": 0.5, "surface_tension": 1.0}),
}
NAMES = list(POINTS)
EXP_POINTS = [n for n in NAMES if n.startswith("exp_")]
RADIUS_POINTS = ["r_large", "r_small"]
BODY_POINTS = ["r_large", "r_small", "rho_heavy", "rho_light", "all_off"]
DFSPH_POINTS = ["r_large", "r_small", "rho_heavy", "g_oblique", "visc_hi"]

SQUEEZE = 0.92          # fluid lattice spacing in d: 0.8 / 0.92^3 = 1.03 rho0 in the bulk, up to 1.23 rho0 with the jitter
TRAJ_STEPS = 20
# What a point's TRAJECTORY scenes change so that the f32 reference ALONE stays deterministic to 3e-5 over the run
# (tests/test_params_host.py holds every scene to that on the CPU; the kernel-by-kernel scene keeps the point as listed):
#   exp_32 / exp_33  1.23^32 = 800: a gentler squeeze (1.07 rho0 at the most)
#   rho_light        stiffness 5e4 at density 1.2 is a sound speed of 540 m/s, 30 x what the time step resolves: stiffness 60
#                    keeps stiffness * exponent / density0 at the default point's 350
#   visc_hi          the explicit viscosity term is unstable at nu = 0.5, h = 0.04, dt = 4e-4 (speeds grow 7 x a step): 3 steps
TRAJ = {"exp_32": dict(squeeze=0.97), "exp_33": dict(squeeze=0.97), "rho_light": dict(cfg={"stiffness": 60}),
        "visc_hi": dict(steps=3)}


# the attributes test_gpu_params changes between two step() calls
IN_FLIGHT = dict(viscosity=0.5, surface_tension=0.0, g=G_OBLIQUE, exponent=1.5, stiffness=500)


def traj_steps(name):
    return TRAJ.get(name, {}).get("steps", TRAJ_STEPS)


def point_cfg(name):
    cfg = copy.deepcopy(scenes.BASE_CFG)
    cfg.update(copy.deepcopy(POINTS.get(name, {}).get("cfg", {})))
    return cfg


def attrs(name):
    return dict(POINTS.get(name, {}).get("attrs", {}))


def integer_exponent(name):
    e = float(point_cfg(name)["exponent"])
    return e == int(e)


def _at(units, d):
    return [u * d for u in units]


def _block(oid, start_u, counts, d, **kw):
    start = _at(start_u, d)
    return scenes._block(oid, start, scenes.lattice_end(start, counts, d), **kw)


def coupled(name, fluid_velocity=(0.2, -0.5, 0.1), body_velocity=(0.0, -2.0, 0.0), traj=False):
    """scenes.fluid_with_rigid_blocks in units of d: 504 fluid particles on a static slab of 240, a dynamic block of 48
    1.4 d above the fluid (inside its support from the first step; at 1 d the few-neighbour m_V of the block doubles the
    density under it and the run turns violent).  15 x 19 x 13 d at the most: inside the high
    padding of every point's grid."""
    p = POINTS.get(name, {})      # name None is the base point: BASE_CFG, default attributes
    cfg = point_cfg(name)
    if traj:
        cfg.update(TRAJ.get(name, {}).get("cfg", {}))
    d = 2 * cfg["particleRadius"]
    rho_f, rho_b = p.get("fluid_rho", 1000.0), p.get("body_rho", 800.0)
    return {
        "Configuration": cfg,
        "FluidBlocks": [_block(0, (5, 5.5, 4.5), (8, 9, 7), d, velocity=fluid_velocity, density=rho_f)],
        "RigidBlocks": [
            _block(1, (3, 3, 3), (12, 2, 10), d, density=rho_f, isDynamic=False, color=(255, 255, 255)),
            _block(2, (7, 14.9, 6), (4, 4, 3), d, velocity=body_velocity, density=rho_b, isDynamic=True,
                   color=(255, 100, 50)),
        ],
    }


def _squeeze(sc, foot_y_u, layers, q=SQUEEZE):
    """Fluid spacing q d about the centre of the block's foot; dynamic solids follow the surface down."""
    a = sc.arrays
    d = sc.geom.particle_diameter
    fl = a["material"] == 1
    x = a["x"].astype(np.float64)
    c = x[fl].mean(axis=0)
    c[1] = foot_y_u * d
    x[fl] = c + (x[fl] - c) * q
    dyn = (a["material"] == 0) & (a["is_dynamic"] == 1)
    x[dyn, 1] -= (1.0 - q) * layers * d
    a["x"] = x.astype(np.float32)
    a["x_0"] = a["x"].copy()


def build_coupled(name, seed=2, amplitude=0.2, traj=False, **kw):
    """(scene dict, cfg, scene) of the coupled scene at a point: squeezed, jittered.  traj: with the point's TRAJ changes."""
    sd = coupled(name, traj=traj, **kw)
    cfg, sc = scenes.build(sd)
    _squeeze(sc, 5.5, 8, TRAJ.get(name, {}).get("squeeze", SQUEEZE) if traj else SQUEEZE)
    scenes.jitter(sc, amplitude, seed=seed)
    _stir(sc, seed)
    return sd, cfg, sc


def _stir(sc, seed):
    """A shear (1 m/s over four layers) and a seeded scatter (0.2 m/s) on the fluid's velocity: with one velocity for the whole
    block every v_i - v_j is zero and the viscous term, 10 nu and visc_eps with it, would never be evaluated."""
    a = sc.arrays
    fl = a["material"] == 1
    d = sc.geom.particle_diameter
    y = a["x"][fl, 1].astype(np.float64)
    v = a["v"][fl].astype(np.float64)
    v[:, 0] += (y - y.mean()) / (4 * d)
    v += np.random.default_rng(seed + 100).normal(0.0, 0.2, size=v.shape)
    a["v"][fl] = v.astype(np.float32)


def build_traj(name):
    return build_coupled(name, seed=4, amplitude=0.1, traj=True)


def bodies(name, obj_path):
    """scenes.fluid_with_rigid_bodies in units of d: two voxelised cubes of side 10 r, one turned by 30 degrees, dropping into
    a fluid block of 648 particles."""
    p = POINTS.get(name, {})      # name None is the base point: BASE_CFG, default attributes
    cfg = point_cfg(name)
    # a 20-step run like the trajectories: the Configuration changes of TRAJ apply (rho_light: stiffness 60); its squeeze
    # and step count do not -- this block is not squeezed and every point is tame over 20 steps (test_params_host.py)
    cfg.update(TRAJ.get(name, {}).get("cfg", {}))
    d = 2 * cfg["particleRadius"]
    rho_f, rho_b = p.get("fluid_rho", 1000.0), p.get("body_rho", 800.0)
    scenes.write_cube_obj(obj_path, (0.0, 0.0, 0.0), 5 * d)
    body = lambda oid, tr, ang, rho, vel: {
        "objectId": oid, "geometryFile": obj_path, "translation": _at(tr, d), "rotationAxis": [0, 0, 1],
        "rotationAngle": ang, "scale": [1, 1, 1], "velocity": list(vel), "density": rho, "color": [255, 255, 255],
        "isDynamic": True}
    return {"Configuration": cfg,
            "FluidBlocks": [_block(0, (3, 3, 3), (12, 6, 9), d, velocity=(0.0, -0.5, 0.0), density=rho_f)],
            "RigidBodies": [body(1, (3.5, 9.2, 4), 0, 0.75 * rho_b, (0.0, -2.0, 0.0)),
                            body(2, (11.5, 9.6, 5), 30, 3.0 * rho_b, (0.0, -2.0, 0.0))]}


def build_bodies(name, obj_path, seed=6):
    sd = bodies(name, obj_path)
    cfg, sc = scenes.build(sd)
    # (fluid only: the bodies keep their voxel lattice, x_0 is their rest shape)
    a = sc.arrays
    rng = np.random.default_rng(seed)
    fl = a["material"] == 1
    d = sc.geom.particle_diameter
    a["x"][fl] += rng.uniform(-0.1 * d, 0.1 * d, size=(int(fl.sum()), 3)).astype(np.float32)
    a["x_0"] = a["x"].copy()
    return sd, cfg, sc


DFSPH_STEPS = 10
# (visc_hi: the explicit viscosity term at nu = 0.5 and the DFSPH step of 2e-3 leaves the 3e-5 cap at the third step)
DFSPH_TRAJ_STEPS = {"visc_hi": 2}


def dfsph_steps(name):
    return DFSPH_TRAJ_STEPS.get(name, DFSPH_STEPS)


def build_dfsph(name):
    """The point's trajectory scene under DFSPHSolver; timeStepSize scales with the radius (2e-3 at r = 0.01)."""
    sd, _, sc0 = build_traj(name)
    sd = scenes.as_dfsph(sd, dt=2e-3 * sd["Configuration"]["particleRadius"] / 0.01)
    cfg, sc = scenes.build(sd)
    sc.arrays = sc0.arrays       # squeezed, jittered, stirred
    return sd, cfg, sc


def params(cfg, sc, name=None, extra=None):
    """scenes.solver_params plus the point's solver attributes (Oracle and Brute read them from `params`)."""
    out = scenes.solver_params(cfg, sc)
    if name is not None:
        out.update(attrs(name))
    out.update(extra or {})
    return out


def make_oracle(cfg, sc, name=None, perturb=0, rigid_sums_f64=False, extra=None, arrays=None):
    from oracle.oracle import Oracle
    return Oracle(params(cfg, sc, name, extra), sc.arrays if arrays is None else arrays, n_objects=max(sc.n_objects, 1),
                  rigid_body_ids=sorted(sc.object_id_rigid_body), dynamic_ids=sorted(sc.dynamic_rigid_ids),
                  rigid_sums_f64=rigid_sums_f64, perturb=perturb)


def make_ps(sd, arrays, name=None, **kw):
    """scenes.make_ps, then the point's solver attributes set on the solver object (pushed by initialize() / step())."""
    ps, solver = scenes.make_ps(sd, arrays, **kw)
    for k, v in (attrs(name) if name else {}).items():
        setattr(solver, k, v)
    return ps, solver
