"""Kinematic rigid bodies: the motion a scene file (or `ParticleSystem.set_body_motion`) prescribes for a NON-dynamic
solid object -- a piston, a flap, a stirrer, a gate.  The reference has no counterpart: its solids are frozen
(`isDynamic: false`) or shape-matched (`isDynamic: true`).

    "motion": {"linearVelocity": [vx, vy, vz], "angularVelocity": [wx, wy, wz], "pivot": [px, py, pz],
               "oscillation": {"amplitude": [ax, ay, az], "frequency": f, "phase": phi},
               "startTime": t0, "endTime": t1}

Every key is optional: velocities, amplitude, frequency and phase default to zero, `pivot` to the f64 mean of the
object's rest positions, `startTime` to 0 and `endTime` to +inf.  With tau = clamp(t, t0, t1) - t0:

    d(tau) = V tau + A (sin(2 pi f tau + phi) - sin(phi))
    R(tau) = rotation about w / |w| by |w| tau            (Rodrigues; the identity when w = 0)
    x(t)   = pivot + d + R (x_0 - pivot)
    v(t)   = d'(tau) + w x (x - pivot - d)                (v = 0 for t outside [t0, t1])

This module is host-only (NumPy, f64): parsing / validation and `pose`, the same formula the library evaluates per
step (csrc/sph_api.hip: kin_pose) before it rounds the pose to f32 for the kernel.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

MAX_KINEMATIC = 8                # SPH_MAX_KINEMATIC
_KEYS = {"linearVelocity", "angularVelocity", "pivot", "oscillation", "startTime", "endTime"}
_OSC_KEYS = {"amplitude", "frequency", "phase"}


@dataclass
class Motion:
    linear_velocity: np.ndarray = field(default_factory=lambda: np.zeros(3))
    angular_velocity: np.ndarray = field(default_factory=lambda: np.zeros(3))
    pivot: np.ndarray | None = None          # None: not resolved yet (the mean of the object's rest positions)
    amplitude: np.ndarray = field(default_factory=lambda: np.zeros(3))
    frequency: float = 0.0
    phase: float = 0.0
    start_time: float = 0.0
    end_time: float = math.inf

    def with_pivot(self, rest_positions) -> "Motion":
        """The default pivot: the f64 mean of the object's rest positions.  The pivot is held in f32 (it is a
        position, and the C ABI carries it as one), so `pose` and the library subtract the same number."""
        if self.pivot is None:
            self.pivot = _f32_point(np.asarray(rest_positions, dtype=np.float64).reshape(-1, 3).mean(axis=0))
        return self


def _f32_point(p) -> np.ndarray:
    return np.asarray(p, dtype=np.float32).astype(np.float64)


def _vec3(spec, key, what):
    v = np.asarray(spec, dtype=np.float64)
    if v.shape != (3,):
        raise ValueError(f"motion: {what} '{key}' must have three components")
    if not np.all(np.isfinite(v)):
        raise ValueError(f"motion: {what} '{key}' is not finite")
    return v


def _scalar(spec, key, allow_inf=False):
    try:
        v = float(spec)
    except (TypeError, ValueError):
        raise ValueError(f"motion: '{key}' must be a number") from None
    if math.isnan(v) or (math.isinf(v) and not (allow_inf and v > 0)):
        raise ValueError(f"motion: '{key}' is not finite")
    return v


def parse_motion(spec: dict, is_dynamic=False, rest_positions=None) -> Motion:
    """Validate a scene file's "motion" entry (or the keyword form of `set_body_motion`).  ValueError: a motion on a
    dynamic object, an unknown key, a non-finite number (`endTime` may be +inf), `endTime < startTime`."""
    if is_dynamic:
        raise ValueError("motion: only a non-dynamic solid can be kinematic (isDynamic is true: the body is shape-matched)")
    if not isinstance(spec, dict):
        raise ValueError("motion: expected an object with the keys " + ", ".join(sorted(_KEYS)))
    unknown = set(spec) - _KEYS
    if unknown:
        raise ValueError(f"motion: unknown key(s) {sorted(unknown)}; known: {sorted(_KEYS)}")
    m = Motion()
    if "linearVelocity" in spec:
        m.linear_velocity = _vec3(spec["linearVelocity"], "linearVelocity", "vector")
    if "angularVelocity" in spec:
        m.angular_velocity = _vec3(spec["angularVelocity"], "angularVelocity", "vector")
    if spec.get("pivot") is not None:
        m.pivot = _f32_point(_vec3(spec["pivot"], "pivot", "point"))
    osc = spec.get("oscillation")
    if osc is not None:
        if not isinstance(osc, dict):
            raise ValueError("motion: 'oscillation' must be an object with the keys amplitude, frequency, phase")
        unknown = set(osc) - _OSC_KEYS
        if unknown:
            raise ValueError(f"motion: unknown oscillation key(s) {sorted(unknown)}; known: {sorted(_OSC_KEYS)}")
        if "amplitude" in osc:
            m.amplitude = _vec3(osc["amplitude"], "amplitude", "vector")
        m.frequency = _scalar(osc.get("frequency", 0.0), "frequency")
        m.phase = _scalar(osc.get("phase", 0.0), "phase")
    m.start_time = _scalar(spec.get("startTime", 0.0), "startTime")
    m.end_time = _scalar(spec.get("endTime", math.inf), "endTime", allow_inf=True)
    if m.end_time < m.start_time:
        raise ValueError(f"motion: endTime {m.end_time} < startTime {m.start_time}")
    if rest_positions is not None:
        m.with_pivot(rest_positions)
    return m


def rotation(axis_angle) -> np.ndarray:
    """Rodrigues: the rotation about a / |a| by |a| (f64 [3, 3]); the identity for a = 0."""
    a = np.asarray(axis_angle, dtype=np.float64)
    th = float(np.linalg.norm(a))
    if th == 0.0:
        return np.eye(3)
    k = a / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def pose(motion: Motion, t: float):
    """(R[3, 3], c[3], u[3], w[3]) at time t, in f64: x = c + R (x_0 - pivot), v = u + w x (x - c); c = pivot + d, u = d'."""
    if motion.pivot is None:
        raise ValueError("motion: the pivot is not resolved (Motion.with_pivot(rest positions))")
    t = float(t)
    tau = min(max(t, motion.start_time), motion.end_time) - motion.start_time
    active = motion.start_time <= t <= motion.end_time
    arg = 2.0 * math.pi * motion.frequency * tau + motion.phase
    d = motion.linear_velocity * tau + motion.amplitude * (math.sin(arg) - math.sin(motion.phase))
    wn = float(np.linalg.norm(motion.angular_velocity))
    R = rotation(motion.angular_velocity / wn * (wn * tau)) if wn > 0.0 else np.eye(3)
    if active:
        u = motion.linear_velocity + motion.amplitude * (2.0 * math.pi * motion.frequency * math.cos(arg))
        w = motion.angular_velocity.copy()
    else:
        u, w = np.zeros(3), np.zeros(3)
    return R, motion.pivot + d, u, w


def apply_pose(R, c, u, w, pivot, x_0):
    """Positions and velocities (f64 [n, 3] each) of rest positions x_0 under a pose."""
    r = (np.asarray(x_0, dtype=np.float64) - np.asarray(pivot, dtype=np.float64)) @ np.asarray(R, dtype=np.float64).T
    return np.asarray(c, dtype=np.float64) + r, np.asarray(u, dtype=np.float64) + np.cross(np.asarray(w, dtype=np.float64), r)


def to_struct(object_id: int, motion: Motion):
    """`struct SphKinematicMotion` (include/sph_hip.h) of a motion with its pivot resolved."""
    import ctypes as C
    from . import _lib
    if motion.pivot is None:
        raise ValueError("motion: the pivot is not resolved (Motion.with_pivot(rest positions))")
    s = _lib.SphKinematicMotion()
    s.object_id = int(object_id)
    s.pivot = (C.c_float * 3)(*[float(v) for v in motion.pivot])
    s.lin_vel = (C.c_double * 3)(*[float(v) for v in motion.linear_velocity])
    s.ang_vel = (C.c_double * 3)(*[float(v) for v in motion.angular_velocity])
    s.osc_amplitude = (C.c_double * 3)(*[float(v) for v in motion.amplitude])
    s.osc_frequency, s.osc_phase = float(motion.frequency), float(motion.phase)
    s.start_time, s.end_time = float(motion.start_time), float(motion.end_time)
    return s
