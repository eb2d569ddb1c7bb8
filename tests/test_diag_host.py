"""Host side of the flow diagnostics and the CFL-governed time step (no GPU): the C ABI additions and their ctypes mirror,
`timestep.cfl_dt` against hand-computed values, the scene-file switch, and what importing the two modules pulls in."""
import ctypes
import math
import os
import re
import subprocess
import sys
import types

import numpy as np

from sph_taichi_amd import _lib, build
from sph_taichi_amd.config_builder import SimConfig
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()


def f32(x):
    return float(np.float32(x))


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_two_calls_and_the_row():
    assert re.search(r"int32_t\s+sph_diag_reduce\s*\(\s*SphContext\s*\*\s*\w+\s*\)\s*;", HEADER)
    assert re.search(r"int32_t\s+sph_diag_download\s*\(\s*SphContext\s*\*\s*\w+\s*,\s*SphDiagRow\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", HEADER)
    assert re.search(r"typedef\s+struct\s+SphDiagRow\s*\{", HEADER) and re.search(r"\}\s*SphDiagRow\s*;", HEADER)
    assert re.search(r"#define\s+SPH_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6      # additive: the version stays


def test_binding_has_the_two_calls():
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert bound["sph_diag_reduce"] == (ctypes.c_int32, [ctypes.c_void_p])
    res, args = bound["sph_diag_download"]
    assert res is ctypes.c_int32 and args == [ctypes.c_void_p, ctypes.POINTER(_lib.SphDiagRow), ctypes.c_int32]


def test_row_layout():
    """Size from the member list of the issue (3 i64, 10 f64, 10 f32) and every offset from a hand-written table."""
    assert ctypes.sizeof(_lib.SphDiagRow) == 3 * 8 + (1 + 3 + 3 + 1 + 1 + 1) * 8 + (4 + 3 + 3) * 4 == 144
    table = {"count": 0, "fluid_count": 8, "moving_count": 16, "mass": 24, "mx": 32, "momentum": 56, "kinetic": 80,
             "v2_max": 88, "a2_max": 96, "density_min": 104, "density_max": 108, "pressure_min": 112, "pressure_max": 116,
             "lo": 120, "hi": 132}
    assert [n for n, _ in _lib.SphDiagRow._fields_] == list(table)
    for name, off in table.items():
        assert getattr(_lib.SphDiagRow, name).offset == off, name
    # the header's struct lists the same members in the same order
    body = re.search(r"typedef\s+struct\s+SphDiagRow\s*\{(.*?)\}\s*SphDiagRow\s*;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", part.strip().split()[-1]) for part in decl.split(",")]
    assert names == list(table)


def test_launch_constants_mirror_the_header():
    for macro, value in (("SPH_DIAG_BLOCKS", _lib.DIAG_BLOCKS), ("SPH_DIAG_THREADS", _lib.DIAG_THREADS),
                         ("SPH_DIAG_MAX_OBJECTS", _lib.DIAG_MAX_OBJECTS)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", HEADER).group(1)) == value
    assert _lib.DIAG_MAX_OBJECTS >= 64 and _lib.DIAG_THREADS % 64 == 0
    # the per-block row tables (one per wave, n_objects + 1 rows) fit the 64 KiB of LDS a launch may ask for
    assert (_lib.DIAG_THREADS // 64) * (_lib.DIAG_MAX_OBJECTS + 1) * ctypes.sizeof(_lib.SphDiagRow) <= 65536


def test_source_is_built():
    assert "sph_diag.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "sph_diag.hip"))


# ---- cfl_dt ---------------------------------------------------------------------------------------------------------------
def _total(v_max=0.0, a_max=0.0, density_max=1000.0):
    return types.SimpleNamespace(v_max=v_max, a_max=a_max, density_max=density_max)


def _cfg(**over):
    from sph_taichi_amd import timestep
    conf = {"timeStepSize": 4e-4, "density0": 1000, "exponent": 7, "stiffness": 50000}
    return timestep.resolve_config(over, conf)


D = 0.02
C0 = math.sqrt(50000.0 * 7.0 / 1000.0)          # 18.708...


def test_cfl_velocity_binds():
    from sph_taichi_amd.timestep import cfl_dt
    # dt_v = 0.4 * 0.02 / 40 = 2e-4; dt_f = 0.25 sqrt(0.02 / 10) = 1.118e-2; dt_a = 0.4 * 0.02 / c0 = 4.28e-4; growth 4.4e-4
    got = cfl_dt(_total(40.0, 10.0), diameter=D, dt_prev=4e-4, cfg=_cfg(), sound_speed=C0)
    assert got == f32(0.4 * 0.02 / 40.0) and abs(got - 2e-4) <= 2e-4 * 2.0 ** -24


def test_cfl_acceleration_binds():
    from sph_taichi_amd.timestep import cfl_dt
    # dt_f = 0.25 sqrt(0.02 / 20000) = 2.5e-4; dt_v = 0.4 * 0.02 / 1 = 8e-3
    got = cfl_dt(_total(1.0, 20000.0), diameter=D, dt_prev=4e-4, cfg=_cfg(), sound_speed=C0)
    assert got == f32(0.25 * math.sqrt(0.02 / 20000.0)) and abs(got - 2.5e-4) <= 2.5e-4 * 2.0 ** -24


def test_cfl_sound_binds_and_dfsph_has_none():
    from sph_taichi_amd.timestep import cfl_dt
    # rho_max / rho0 = 1.1: c = c0 sqrt(1.1^6) = c0 * 1.331; dt_a = 0.4 * 0.02 / (18.708 * 1.331) = 3.2128e-4
    cfg = _cfg(maxTimeStepSize=1.0, maxGrowth=100.0)
    got = cfl_dt(_total(0.0, 0.0, 1100.0), diameter=D, dt_prev=4e-4, cfg=cfg, sound_speed=C0)
    assert got == f32(0.4 * 0.02 / (C0 * math.sqrt(1.1 ** 6))) and abs(got - 3.2128e-4) < 1e-8     # (the hand value has five digits)
    # DFSPH: no speed of sound, v_max == 0 and a_max == 0 ignored: only the growth limit is left
    got = cfl_dt(_total(0.0, 0.0, 1100.0), diameter=D, dt_prev=4e-4, cfg=cfg, sound_speed=None)
    assert got == f32(100.0 * 4e-4)


def test_zero_velocity_and_acceleration_are_ignored():
    from sph_taichi_amd.timestep import cfl_dt
    cfg = _cfg(maxTimeStepSize=1.0, maxGrowth=2.0)
    assert cfl_dt(_total(0.0, 0.0), diameter=D, dt_prev=1e-4, cfg=cfg) == f32(2e-4)                  # growth alone
    assert cfl_dt(_total(0.0, 20000.0), diameter=D, dt_prev=4e-4, cfg=cfg) == f32(2.5e-4)            # dt_f alone
    assert cfl_dt(_total(40.0, 0.0), diameter=D, dt_prev=4e-4, cfg=cfg) == f32(2e-4)                 # dt_v alone


def test_growth_limit_and_clamps():
    from sph_taichi_amd.timestep import cfl_dt
    # growth: 1.1 * 1e-4 below every criterion and below the maximum
    assert cfl_dt(_total(1.0, 1.0), diameter=D, dt_prev=1e-4, cfg=_cfg(), sound_speed=C0) == f32(1.1 * 1e-4)
    # upper clamp: calm flow, large previous dt -> the scene's timeStepSize (the default maximum)
    assert cfl_dt(_total(1e-3, 1e-3), diameter=D, dt_prev=1.0, cfg=_cfg(), sound_speed=None) == f32(4e-4)
    # lower clamp: dt_v = 0.4 * 0.02 / 1e4 = 8e-7 < timeStepSize / 16 = 2.5e-5
    assert cfl_dt(_total(1e4, 0.0), diameter=D, dt_prev=4e-4, cfg=_cfg(), sound_speed=C0) == f32(4e-4 / 16)
    assert cfl_dt(_total(1e4, 0.0), diameter=D, dt_prev=4e-4, cfg=_cfg(minTimeStepSize=1e-5), sound_speed=C0) == f32(1e-5)


def test_result_is_an_f32_value():
    from sph_taichi_amd.timestep import cfl_dt
    got = cfl_dt(_total(0.1, 7.0), diameter=D, dt_prev=4e-4, cfg=_cfg(maxTimeStepSize=1.0, maxGrowth=100.0), sound_speed=None)
    assert isinstance(got, float) and got == f32(got) and got == f32(0.25 * math.sqrt(0.02 / 7.0))
    assert got != 0.25 * math.sqrt(0.02 / 7.0)              # the f64 value is not representable: it WAS rounded


# ---- the scene-file switch ------------------------------------------------------------------------------------------------
def _fake(scene_dict):
    cfg = SimConfig(config=scene_dict)
    ps = types.SimpleNamespace(cfg=cfg, particle_diameter=0.02)
    c = scene_dict["Configuration"]
    solver = types.SimpleNamespace(dt={None: c["timeStepSize"]}, stiffness=c["stiffness"], exponent=c["exponent"],
                                   density_0=c["density0"])
    return ps, solver


def test_controller_is_built_only_when_the_scene_asks():
    from sph_taichi_amd import timestep
    from sph_taichi_amd.particle_system import ParticleSystem
    sd = scenes.fluid_only()
    ps, solver = _fake(sd)
    assert ParticleSystem.build_time_step_controller(ps, solver) is None        # key absent: the run is what it was
    sd["Configuration"]["adaptiveTimeStep"] = {}
    ps, solver = _fake(sd)
    c = ParticleSystem.build_time_step_controller(ps, solver)
    assert isinstance(c, timestep.TimeStepController) and c.updates == 0
    want = {"cflVelocity": 0.4, "cflAcceleration": 0.25, "cflSound": 0.4, "maxGrowth": 1.1,
            "maxTimeStepSize": 0.0004, "minTimeStepSize": 0.0004 / 16}
    assert {k: c.cfg[k] for k in want} == want
    assert c.cfg["maxTimeStepSize"] == sd["Configuration"]["timeStepSize"]
    assert c.sound_speed == C0                                                   # WCSPH: the Tait EOS of the scene
    sd["Configuration"]["adaptiveTimeStep"] = {"cflVelocity": 0.01, "minTimeStepSize": 1e-6}
    c = ParticleSystem.build_time_step_controller(*_fake(sd))
    assert c.cfg["cflVelocity"] == 0.01 and c.cfg["minTimeStepSize"] == 1e-6 and c.cfg["cflSound"] == 0.4
    d4 = scenes.as_dfsph(sd)
    assert ParticleSystem.build_time_step_controller(*_fake(d4)).sound_speed is None   # DFSPH: no dt_a
    sd["Configuration"]["adaptiveTimeStep"] = {"cflVelocty": 0.01}
    try:
        ParticleSystem.build_time_step_controller(*_fake(sd))
    except ValueError as e:
        assert "cflVelocty" in str(e)
    else:
        raise AssertionError("a misspelt key must not be ignored")


def test_diag_row_derived_members():
    from sph_taichi_amd.diagnostics import DiagRow, Diagnostics
    raw = _lib.SphDiagRow()
    raw.count, raw.fluid_count, raw.moving_count, raw.mass = 2, 2, 2, 4.0
    raw.mx[:] = [2.0, 8.0, -4.0]
    raw.momentum[:] = [1.0, 0.0, 0.0]
    raw.kinetic, raw.v2_max, raw.a2_max = 3.0, 9.0, 16.0
    row = DiagRow(raw, g=(0.0, -10.0, 0.0))
    assert row.v_max == 3.0 and row.a_max == 4.0 and row.center_of_mass == (0.5, 2.0, -1.0)
    assert row.potential == 80.0 and row.energy == 83.0
    import json
    d = json.loads(json.dumps(Diagnostics(0.5, [row], row).as_dict()))
    assert d["time"] == 0.5 and d["total"]["energy"] == 83.0 and d["objects"][0]["mx"] == [2.0, 8.0, -4.0]
    assert DiagRow(_lib.SphDiagRow()).center_of_mass is None


def test_modules_import_without_the_library_or_the_oracle():
    code = ("import sys\n"
            "import sph_taichi_amd.timestep, sph_taichi_amd.diagnostics\n"
            "from sph_taichi_amd import _lib\n"
            "assert _lib._LIB is None, 'the library was loaded at import'\n"
            "bad = [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.') or m == 'torch']\n"
            "assert not bad, bad\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for mod in ("timestep.py", "diagnostics.py"):
        src = open(os.path.join(ROOT, "sph_taichi_amd", mod)).read()
        assert not re.search(r"^(from|import)\s+\S*(_lib|oracle|torch)", src, re.M), mod   # nothing of the GPU at module level
