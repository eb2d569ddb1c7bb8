"""A CFL-governed time step from the device diagnostics (pure host code; nothing here imports the GPU library).

The three criteria of the reference's older engine (legacy/engine/sph_solver.py:738-759: velocity, acceleration, speed of
sound), with this solver's own equation of state and the particle diameter d as the length:

    dt_v = cflVelocity     * d / v_max                               (ignored when v_max == 0)
    dt_f = cflAcceleration * sqrt(d / a_max)                         (ignored when a_max == 0)
    dt_a = cflSound * d / (c0 * sqrt((rho_max / rho0) ** (exponent - 1)))     (WCSPH only)
    c0   = sqrt(stiffness * exponent / density0)                     (Tait EOS, WCSPH.py:76: c^2 = dp / drho)
    dt   = clamp(min(dt_v, dt_f, dt_a, maxGrowth * dt_prev), minTimeStepSize, maxTimeStepSize)    rounded to f32

The scene file switches it on with an "adaptiveTimeStep": {...} object in its Configuration (may be empty).  The defaults
are POLICY, not measurements: the CFL numbers are the customary ones of the SPH literature, and maxTimeStepSize defaults
to the scene's timeStepSize so that, unless told otherwise, the controller only ever shrinks the hand-tuned step
(minTimeStepSize = timeStepSize / 16 bounds how far).  dt changes BETWEEN `solver.step(n)` calls, never inside one.
"""
from __future__ import annotations

import math

import numpy as np

DEFAULTS = {"cflVelocity": 0.4, "cflAcceleration": 0.25, "cflSound": 0.4, "maxGrowth": 1.1}
KEYS = tuple(DEFAULTS) + ("maxTimeStepSize", "minTimeStepSize")


def resolve_config(adaptive: dict, scene_configuration: dict) -> dict:
    """The "adaptiveTimeStep" object with every default filled in, plus the EOS constants dt_a needs (density0, exponent)."""
    unknown = sorted(set(adaptive) - set(KEYS))
    if unknown:
        raise ValueError(f"adaptiveTimeStep: unknown keys {unknown} (known: {list(KEYS)})")
    dt0 = float(scene_configuration.get("timeStepSize") or 1e-4)
    cfg = {k: float(adaptive.get(k, v)) for k, v in DEFAULTS.items()}
    cfg["maxTimeStepSize"] = float(adaptive.get("maxTimeStepSize", dt0))
    cfg["minTimeStepSize"] = float(adaptive.get("minTimeStepSize", dt0 / 16.0))
    cfg["density0"] = float(scene_configuration.get("density0") or 1000.0)
    cfg["exponent"] = float(scene_configuration.get("exponent") or 7.0)
    for k in KEYS:
        if not (cfg[k] > 0.0 and math.isfinite(cfg[k])):
            raise ValueError(f"adaptiveTimeStep: {k} must be positive and finite, got {cfg[k]}")
    if cfg["minTimeStepSize"] > cfg["maxTimeStepSize"]:
        raise ValueError("adaptiveTimeStep: minTimeStepSize > maxTimeStepSize")
    return cfg


def tait_sound_speed(stiffness: float, exponent: float, density0: float) -> float:
    """c0 of p = stiffness ((rho / rho0)^exponent - 1)  (WCSPH.py:76)."""
    return math.sqrt(float(stiffness) * float(exponent) / float(density0))


def cfl_dt(diag_total, *, diameter, dt_prev, cfg, sound_speed=None) -> float:
    """The next dt from the total row of a `Diagnostics` (anything with v_max, a_max, density_max), the particle diameter,
    the dt in force and a config from `resolve_config`.  `sound_speed` = c0 for WCSPH, None for DFSPH (no dt_a).  The
    result is an f32 value: the library holds dt as f32."""
    d = float(diameter)
    cand = [float(cfg["maxGrowth"]) * float(dt_prev)]
    if diag_total.v_max > 0.0:
        cand.append(cfg["cflVelocity"] * d / diag_total.v_max)
    if diag_total.a_max > 0.0:
        cand.append(cfg["cflAcceleration"] * math.sqrt(d / diag_total.a_max))
    if sound_speed is not None and diag_total.density_max > 0.0:
        ratio = diag_total.density_max / cfg["density0"]
        cand.append(cfg["cflSound"] * d / (float(sound_speed) * math.sqrt(ratio ** (cfg["exponent"] - 1.0))))
    dt = min(max(min(cand), cfg["minTimeStepSize"]), cfg["maxTimeStepSize"])
    return float(np.float32(dt))


class TimeStepController:
    """`update()` between two `solver.step(n)` calls: reduce the diagnostics, apply `cfl_dt`, set `solver.dt[None]`."""

    def __init__(self, ps, solver, cfg: dict | None = None):
        self.ps, self.solver = ps, solver
        self.cfg = resolve_config(dict(cfg or {}), ps.cfg.config["Configuration"])
        self.sound_speed = None
        if ps.cfg.get_cfg("simulationMethod") == 0:      # WCSPH: the Tait EOS of the solver as it stands now
            self.sound_speed = tait_sound_speed(solver.stiffness, solver.exponent, solver.density_0)
            self.cfg["density0"], self.cfg["exponent"] = float(solver.density_0), float(solver.exponent)
        self.dt_min_used = self.dt_max_used = float(np.float32(solver.dt[None]))    # the steps before the first update
        self.updates = 0

    def update(self):
        diag = self.ps.diagnostics()
        dt = cfl_dt(diag.total, diameter=self.ps.particle_diameter, dt_prev=self.solver.dt[None], cfg=self.cfg,
                    sound_speed=self.sound_speed)
        self.solver.dt[None] = dt
        self.dt_min_used = min(self.dt_min_used, dt)
        self.dt_max_used = max(self.dt_max_used, dt)
        self.updates += 1
        return dt, diag


def build_controller(ps, solver):
    """None unless the scene's Configuration holds an "adaptiveTimeStep" object."""
    adaptive = ps.cfg.get_cfg("adaptiveTimeStep")
    if adaptive is None:
        return None
    if not isinstance(adaptive, dict):
        raise ValueError("adaptiveTimeStep must be an object (it may be empty)")
    return TimeStepController(ps, solver, adaptive)
