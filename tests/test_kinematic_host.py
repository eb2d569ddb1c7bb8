"""Kinematic rigid bodies, host side (no GPU): sph_taichi_amd/motion.py against an independent numpy evaluation of the
motion model, the validation rules, the scene-file path, and the header / binding / library exports of the four entry points."""
import copy
import ctypes
import math
import os
import re

import numpy as np
import pytest

from sph_taichi_amd import _lib, motion
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIN_SYMBOLS = ["sph_kinematic_set", "sph_kinematic_apply", "sph_get_time", "sph_set_time"]


def _ref_pose(V, W, P, A, f, phi, t0, t1, t):
    """The model of the issue, written out independently of motion.py (axis-angle through the matrix exponential's closed
    form applied to a vector, not through a matrix): returns a function x_0 -> (x, v)."""
    V, W, P, A = (np.asarray(a, dtype=np.float64) for a in (V, W, P, A))
    tau = min(max(t, t0), t1) - t0
    d = V * tau + A * (math.sin(2 * math.pi * f * tau + phi) - math.sin(phi))
    dd = V + A * 2 * math.pi * f * math.cos(2 * math.pi * f * tau + phi)
    wn = np.linalg.norm(W)

    def at(x0):
        q = np.asarray(x0, dtype=np.float64) - P
        if wn > 0:
            k, th = W / wn, wn * tau
            r = q * math.cos(th) + np.cross(k, q) * math.sin(th) + k * np.dot(k, q) * (1 - math.cos(th))
        else:
            r = q
        x = P + d + r
        v = dd + np.cross(W, x - P - d) if t0 <= t <= t1 else np.zeros(3)
        return x, v
    return at


def _check(spec, pivot, t, points, tol=1e-14):
    m = motion.parse_motion(dict(spec, pivot=pivot))
    R, c, u, w = motion.pose(m, t)
    osc = spec.get("oscillation", {})
    ref = _ref_pose(spec.get("linearVelocity", (0, 0, 0)), spec.get("angularVelocity", (0, 0, 0)), m.pivot,
                    osc.get("amplitude", (0, 0, 0)), osc.get("frequency", 0.0), osc.get("phase", 0.0),
                    spec.get("startTime", 0.0), spec.get("endTime", math.inf), t)
    X, Vv = motion.apply_pose(R, c, u, w, m.pivot, np.asarray(points, dtype=np.float64))
    for p, x, v in zip(points, X, Vv):
        xr, vr = ref(p)
        assert np.abs(x - xr).max() <= tol and np.abs(v - vr).max() <= tol * 10, (p, x, xr, v, vr)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1) <= 1e-15
    return R, c, u, w


def test_pose_quarter_turn_about_z():
    R, c, u, w = _check({"angularVelocity": [0, 0, math.pi / 2]}, [0.25, 0.5, 0.125], 1.0, [(1, 0, 0), (0.3, 0.7, 0.2)])
    pivot = np.array([0.25, 0.5, 0.125])
    x = c + R @ (np.array([1.0, 0.0, 0.0]) - pivot)
    # (1,0,0) - pivot = (0.75, -0.5, -0.125) turns into (0.5, 0.75, -0.125)
    assert np.allclose(x, pivot + np.array([0.5, 0.75, -0.125]), atol=1e-15)
    assert np.array_equal(c, pivot) and np.array_equal(u, np.zeros(3)) and np.array_equal(w, [0, 0, math.pi / 2])


def test_pose_translation_only():
    R, c, u, w = _check({"linearVelocity": [0.5, -0.25, 2.0]}, [0.5, 0.5, 0.5], 0.75, [(0.1, 0.2, 0.3)])
    assert np.array_equal(R, np.eye(3)) and np.array_equal(c, np.array([0.5, 0.5, 0.5]) + 0.75 * np.array([0.5, -0.25, 2.0]))
    assert np.array_equal(u, [0.5, -0.25, 2.0]) and np.array_equal(w, np.zeros(3))


def test_pose_oscillation_at_quarter_period():
    f = 2.5
    spec = {"oscillation": {"amplitude": [0.1, 0.0, -0.05], "frequency": f}}
    R, c, u, w = _check(spec, [0.5, 0.5, 0.5], 1 / (4 * f), [(0.4, 0.6, 0.5)])
    assert np.allclose(c, [0.6, 0.5, 0.45], atol=1e-16) and np.abs(u).max() <= 1e-15 * 2 * math.pi * f      # the turning point
    # with a phase: d(0) = 0 whatever the phase, and the velocity there is A 2 pi f cos(phi)
    spec["oscillation"]["phase"] = 0.7
    R, c, u, w = _check(spec, [0.5, 0.5, 0.5], 0.0, [(0.4, 0.6, 0.5)])
    assert np.array_equal(c, [0.5, 0.5, 0.5]) and np.allclose(u, np.array([0.1, 0, -0.05]) * 2 * math.pi * f * math.cos(0.7), rtol=1e-15)
    _check(dict(spec, linearVelocity=[0.1, 0.2, 0.3], angularVelocity=[1.0, -2.0, 0.5]), [0.5, 0.5, 0.5], 0.3731, [(0.4, 0.6, 0.5)])


def test_pose_is_clamped_outside_the_interval_with_zero_velocity():
    spec = {"linearVelocity": [1.0, 0.0, 0.0], "angularVelocity": [0.0, 2.0, 0.0], "startTime": 0.5, "endTime": 1.5}
    pts = [(0.4, 0.6, 0.5), (0.9, 0.1, 0.2)]
    R0, c0, u0, w0 = _check(spec, [0.5, 0.5, 0.5], 0.25, pts)            # before: the rest pose, at rest
    assert np.array_equal(R0, np.eye(3)) and np.array_equal(c0, [0.5, 0.5, 0.5]) and not u0.any() and not w0.any()
    R1, c1, u1, w1 = _check(spec, [0.5, 0.5, 0.5], 9.0, pts)             # after: the pose of endTime, at rest
    Re, ce, ue, we = _check(spec, [0.5, 0.5, 0.5], 1.5, pts)
    assert np.array_equal(R1, Re) and np.array_equal(c1, ce) and not u1.any() and not w1.any()
    assert np.array_equal(ue, [1.0, 0.0, 0.0]) and np.array_equal(we, [0.0, 2.0, 0.0])       # the ends belong to the interval
    assert np.allclose(ce, [1.5, 0.5, 0.5])


def test_default_pivot_is_the_f64_mean_of_the_rest_positions_held_in_f32():
    rest = np.random.default_rng(3).uniform(0.2, 0.4, size=(217, 3)).astype(np.float32)
    m = motion.parse_motion({"linearVelocity": [1, 0, 0]}, rest_positions=rest)
    mean = rest.astype(np.float64).mean(axis=0)
    assert np.array_equal(m.pivot, mean.astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError, match="pivot"):
        motion.pose(motion.parse_motion({}), 0.0)
    assert m.end_time == math.inf and m.start_time == 0.0 and m.frequency == 0.0 and not m.amplitude.any()


@pytest.mark.parametrize("spec,dyn,what", [
    ({"linearVelocity": [1, 0, 0]}, True, "isDynamic"),
    ({"linearVelocity": [1, float("nan"), 0]}, False, "finite"),
    ({"angularVelocity": [float("inf"), 0, 0]}, False, "finite"),
    ({"pivot": [0, 0, float("nan")]}, False, "finite"),
    ({"oscillation": {"amplitude": [0, 0, 1], "frequency": float("nan")}}, False, "finite"),
    ({"oscillation": {"phase": float("inf")}}, False, "finite"),
    ({"startTime": float("inf")}, False, "finite"),
    ({"endTime": float("nan")}, False, "finite"),
    ({"endTime": -float("inf")}, False, "finite"),
    ({"startTime": 2.0, "endTime": 1.0}, False, "endTime"),
    ({"velocity": [1, 0, 0]}, False, "unknown"),
    ({"oscillation": {"amplitude": [0, 0, 1], "period": 2.0}}, False, "unknown"),
    ({"linearVelocity": [1, 0]}, False, "three"),
])
def test_validation_raises(spec, dyn, what):
    with pytest.raises(ValueError, match=what):
        motion.parse_motion(spec, is_dynamic=dyn)


def test_scene_file_motion_is_parsed_and_checked():
    sd = scenes.fluid_with_rigid_blocks()
    sd["RigidBlocks"][0]["motion"] = {"linearVelocity": [0.0, 0.0, 0.25], "endTime": 2.0}
    cfg, sc = scenes.build(sd)
    assert list(sc.motions) == [1] and sc.motions[1].end_time == 2.0
    rest = sc.arrays["x_0"][sc.arrays["object_id"] == 1].astype(np.float64)
    assert np.array_equal(sc.motions[1].pivot, rest.mean(axis=0).astype(np.float32).astype(np.float64))
    assert scenes.build(scenes.fluid_with_rigid_blocks())[1].motions == {}
    bad = copy.deepcopy(sd)
    bad["RigidBlocks"][1]["motion"] = {"linearVelocity": [0.0, 0.0, 0.25]}         # the dynamic block
    with pytest.raises(ValueError, match="isDynamic"):
        scenes.build(bad)
    bad = copy.deepcopy(sd)
    bad["RigidBlocks"][0]["motion"]["speed"] = 3
    with pytest.raises(ValueError, match="unknown"):
        scenes.build(bad)


def test_slab_solver_refuses_a_scene_with_a_motion():
    from sph_taichi_amd import distributed
    sd = scenes.fluid_with_rigid_blocks()
    sd["RigidBlocks"][0]["motion"] = {"linearVelocity": [0.0, 0.0, 0.25]}
    with pytest.raises(NotImplementedError, match="single-domain"):
        distributed.SlabSolver(sd, rank=0, world=2)


def test_header_binding_and_library_carry_the_kinematic_abi():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6       # additive: the version stays
    assert re.search(r"#define SPH_MAX_KINEMATIC 8\b", header) and _lib.MAX_KINEMATIC == 8 == motion.MAX_KINEMATIC
    declared = set(re.findall(r"\b(sph_[a-z0-9_A-Z]+)\s*\(", header))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in KIN_SYMBOLS:
        assert name in declared and name in bound, name
    assert {n for n in declared if n.startswith("sph_kinematic")} == {"sph_kinematic_set", "sph_kinematic_apply"}
    # struct layouts: i32 + 3 f32, then 13 f64 / i32 + 21 f32
    assert ctypes.sizeof(_lib.SphKinematicMotion) == 16 + 13 * 8 and _lib.SphKinematicMotion.lin_vel.offset == 16
    assert _lib.SphKinematicMotion.end_time.offset == 16 + 12 * 8
    assert ctypes.sizeof(_lib.SphBodyPose) == 4 * 22 and _lib.SphBodyPose.origin.offset == 4 * 13
    lib = _lib.load()                                    # builds with the compiler if needed; no device call
    assert lib.sph_abi_version() == 6
    for name in KIN_SYMBOLS:
        assert hasattr(lib, name), name
    s = motion.to_struct(3, motion.parse_motion({"linearVelocity": [1, 2, 3], "pivot": [0.1, 0.2, 0.3], "endTime": 4.0}))
    assert s.object_id == 3 and list(s.lin_vel) == [1.0, 2.0, 3.0] and s.end_time == 4.0 and s.start_time == 0.0
    assert list(s.pivot) == [float(np.float32(v)) for v in (0.1, 0.2, 0.3)]
