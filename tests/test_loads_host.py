"""Host side of the fluid loads (no GPU): the C ABI additions with their ctypes mirror against a host program compiled with the
header, the argument and scene-key checks, the CSV round trip, the torque transport and the impulse, and THE FORMULA against the CPU
oracle, independent of the kernel: the load the numpy model (tests/loads_model.py) computes is minus the momentum the oracle's
accelerations give the fluid beyond gravity."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sph_taichi_amd import _lib, build, loads
from sph_taichi_amd.config_builder import SimConfig
from tests import loads_model as model
from tests import loads_scenes
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
ENTRIES = ("sph_loads_set", "sph_loads_sample", "sph_loads_info", "sph_loads_download", "sph_loads_reset")


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    decls = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"int32_t\s+{name}\s*\(\s*SphContext\s*\*", decls), name
    assert re.search(r"#define\s+SPH_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    assert HEADER.index("Fluid loads (") > HEADER.index("Running flow statistics (")                       # the last section
    section = HEADER[HEADER.index("Fluid loads ("):]
    for word in ("m_i * rho0 * m_V_j", "q <= 1.0f and r > 1e-5f", "65536.0", "llrint(c_a * 2^24)", "2^40", "2^22", "no float or double atomic",
                 "steps_seen % every == 0", "dropped", "sph_dfsph_step with a registered set returns SPH_E_STATE", "not part of a checkpoint",
                 "SPH_OPT_SORT_LEAN is not\n * taken", "Fx Fy Fz Tx Ty Tz pairs wet saturated"):
        assert word in section, word


def test_binding():
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = {"sph_loads_set": [vp, ctypes.POINTER(_lib.SphLoadParams)], "sph_loads_sample": [vp],
            "sph_loads_info": [vp, ctypes.POINTER(_lib.SphLoadInfo)], "sph_loads_download": [vp, vp, vp, i64, i32], "sph_loads_reset": [vp]}
    for name, args in want.items():
        assert bound[name] == (i32, args), name
    assert "sph_loads.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "sph_loads.hip"))
    assert (_lib.LOADS_MAX_OBJECTS, _lib.LOADS_ROW_WORDS, _lib.LOADS_SCALE_LOG2) == (loads.MAX_OBJECTS, loads.ROW_WORDS, loads.SCALE_LOG2) == (32, 9, 24)


def test_struct_layouts_against_the_host_compiler(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "loads_abi_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "loads_abi_driver.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = {line.split()[0]: line.split()[1:] for line in out.splitlines()}
    pairs = lambda words: {words[k]: int(words[k + 1]) for k in range(1, len(words), 2)}
    P, I = _lib.SphLoadParams, _lib.SphLoadInfo
    assert int(rows["SphLoadParams"][0]) == ctypes.sizeof(P) == 152
    assert pairs(rows["SphLoadParams"]) == {k: getattr(P, k).offset for k in ("object_ids", "n_objects", "about", "every", "capacity")}
    assert int(rows["SphLoadInfo"][0]) == ctypes.sizeof(I) == 32
    assert pairs(rows["SphLoadInfo"]) == {k: getattr(I, k).offset for k in ("n_objects", "every", "samples", "dropped", "steps_seen")}
    assert [int(rows[k][0]) for k in ("SPH_LOADS_MAX_OBJECTS", "SPH_LOADS_ROW_WORDS", "SPH_LOADS_SCALE_LOG2", "SPH_ABI_VERSION")] == [32, 9, 24, 6]


# ---- arguments and the scene key ------------------------------------------------------------------------------------------
def test_argument_checks():
    assert loads.set_args() == {"objects": [1], "about": (0.0, 0.0, 0.0), "every": 1, "capacity": 4096}
    a = loads.set_args(objects=[3, 1], about=[0.5, 0.25, np.float32(0.1)], every=4, capacity=10)
    assert a["objects"] == [3, 1] and a["about"] == (0.5, 0.25, float(np.float32(0.1))) and (a["every"], a["capacity"]) == (4, 10)
    assert loads.set_args(objects=2)["objects"] == [2]
    for kw in ({"objects": None}, {"objects": []}, {"objects": [1, 1]}, {"objects": [-1]}, {"objects": list(range(33))}, {"objects": [1.5]},
               {"about": [0, 0]}, {"about": [0, float("nan"), 0]}, {"about": [0, 0, float("inf")]}, {"about": "x"}, {"about": [1e39, 0, 0]},
               {"every": 0}, {"every": 1.5}, {"every": True}, {"capacity": 0}, {"capacity": -3}, {"capacity": 2.0},
               {"objects": list(range(32)), "capacity": 1 << 20}):
        with pytest.raises(ValueError):
            loads.set_args(**kw)
    p = loads.load_params(a)
    assert list(p.object_ids)[:3] == [3, 1, 0] and p.n_objects == 2 and list(p.about) == [0.5, 0.25, np.float32(0.1)] and (p.every, p.capacity) == (4, 10)


def _config(**keys):
    sd = scenes.fluid_only(counts=(3, 3, 3))
    sd["Configuration"].update(keys)
    return SimConfig(config=sd)


def test_scene_key_and_command_line_flag():
    assert loads.loads_config(_config()) is None
    assert loads.loads_config(_config(loads={"objects": [1]})) == {"objects": [1], "about": (0.0, 0.0, 0.0), "every": 1, "capacity": 4096}
    kw = loads.loads_config(_config(loads={"objects": [2, 1], "about": [0.5, 0.1, 0.4], "every": 5, "capacity": 100}))
    assert kw == {"objects": [2, 1], "about": [0.5, 0.1, 0.4], "every": 5, "capacity": 100} and loads.set_args(**kw)["objects"] == [2, 1]
    for bad in ([1], {}, {"object": [1]}, {"objects": [1], "point": [0, 0, 0]}, {"objects": []}, {"objects": [1, 1]}, {"objects": [1], "every": 0},
                {"objects": [1], "capacity": "many"}, {"objects": [1], "about": [0, 0]}):
        with pytest.raises(ValueError, match="loads"):
            loads.loads_config(_config(loads=bad))
    from sph_taichi_amd import run_simulation
    args = run_simulation.build_parser().parse_args(["--scene_file", "x.json", "--loads", "out.csv"])
    assert args.loads == "out.csv"


def test_slab_rank_is_refused():
    class Slab:
        slab = {"x_lo": 0}

        def _call(self, *a):
            raise AssertionError("the library must not be reached")
    with pytest.raises(NotImplementedError, match="single-domain contexts only"):
        loads.set_loads(Slab())
    with pytest.raises(NotImplementedError, match="single-domain"):
        loads.clear_loads(Slab())
    with pytest.raises(ValueError):                                   # the arguments are checked first, as for the other observers
        loads.set_loads(Slab(), every=0)


# ---- the history's views ----------------------------------------------------------------------------------------------------
def _history(samples=5, objects=(1, 4), about=(0.5, 0.25, 0.125), seed=3):
    rng = np.random.default_rng(seed)
    rows = rng.integers(-(1 << 30), 1 << 30, size=(samples, len(objects), 9), dtype=np.int64)
    rows[..., 6:] = rng.integers(0, 1000, size=(samples, len(objects), 3))
    times = np.cumsum(rng.uniform(1e-4, 5e-4, size=samples))
    return loads.LoadHistory(rows, times, objects, about)


def test_views_and_csv_round_trip(tmp_path):
    h = _history()
    assert h.samples == 5 and h.force().shape == h.torque().shape == (5, 2, 3) and h.force().dtype == np.float64
    assert np.array_equal(h.force() * 2.0 ** 24, h.raw[..., 0:3]) and np.array_equal(h.torque() * 2.0 ** 24, h.raw[..., 3:6])
    assert np.array_equal(h.pairs(), h.raw[..., 6]) and np.array_equal(h.wet_particles(), h.raw[..., 7]) and np.array_equal(h.saturated(), h.raw[..., 8])
    rows = h.rows()
    assert len(rows) == 10 and rows[3]["object"] == 4 and rows[3]["time"] == h.times[1] and rows[3]["force"] == list(h.force()[1, 1])
    path = str(tmp_path / "loads.csv")
    h.write_csv(path)
    back = loads.read_csv(path)
    assert back["about"] == h.about and open(path).readlines()[1].strip() == ",".join(loads.CSV_HEADER)
    assert np.array_equal(back["time"], np.repeat(h.times, 2)) and np.array_equal(back["object"], np.tile([1, 4], 5))
    assert np.array_equal(back["force"], h.force().reshape(-1, 3)) and np.array_equal(back["torque"], h.torque().reshape(-1, 3))   # repr reads back exactly
    for k, col in (("pairs", 6), ("wet_particles", 7), ("saturated", 8)):
        assert np.array_equal(back[k], h.raw[..., col].reshape(-1))
    empty = loads.LoadHistory(np.zeros((0, 2, 9), np.int64), np.zeros(0), (1, 4), (0, 0, 0))
    empty.write_csv(path)
    assert loads.read_csv(path)["time"].size == 0 and empty.force().shape == (0, 2, 3) and not empty.impulse().any()
    with pytest.raises(ValueError):
        loads.LoadHistory(np.zeros((2, 1, 9), np.int64), np.zeros(3), (1,), (0, 0, 0))


def test_torque_transport_identity():
    """Point forces F_k at x_k: the torque about c' computed directly equals the torque about c transported by T - (c' - c) x F."""
    rng = np.random.default_rng(5)
    x, F = rng.uniform(0, 1, size=(40, 3)), rng.normal(size=(40, 3))
    c, c2 = np.array([0.5, 0.25, 0.125]), np.array([-0.3, 0.9, 0.4])
    T, T2 = np.cross(x - c, F).sum(axis=0), np.cross(x - c2, F).sum(axis=0)
    assert np.abs(loads.transport_torque(T, F.sum(axis=0), c, c2) - T2).max() <= 1e-13
    h = _history()
    assert np.array_equal(h.torque(about=h.about), h.torque())
    moved = h.torque(about=(0.0, 1.0, 0.5))
    want = h.torque() - np.cross(np.broadcast_to(np.array([0.0, 1.0, 0.5]) - np.array(h.about), h.force().shape), h.force())
    assert np.array_equal(moved, want) and not np.array_equal(moved, h.torque())


def test_impulse_is_the_trapezoid():
    rows = np.zeros((4, 1, 9), np.int64)
    rows[:, 0, 0] = np.array([0, 2, 2, 6]) << 24                      # Fx = 0, 2, 2, 6 N
    rows[:, 0, 1] = np.array([1, 1, 1, 1]) << 24
    h = loads.LoadHistory(rows, [0.0, 1.0, 3.0, 4.0], (1,), (0, 0, 0))
    assert np.array_equal(h.impulse(), [[1.0 + 4.0 + 4.0, 4.0, 0.0]])
    assert not loads.LoadHistory(rows[:1], [0.0], (1,), (0, 0, 0)).impulse().any()


# ---- the formula against the CPU oracle -------------------------------------------------------------------------------------
def test_load_is_minus_the_fluids_momentum_change_in_the_oracle():
    """One fluid of ONE particle mass on one static slab.  The oracle's kernels of one step up to its accelerations (sort, boundary
    volume, density, non-pressure and pressure forces; x is still the x they were computed at).  With one uniform fluid mass the
    fluid-fluid pressure, viscosity and surface-tension pairs cancel pairwise and the reference has no boundary viscosity, so
        sum_i m_i (a_i - g) + sum_objects F_model = 0
    up to the oracle's f32 rounding.  The residual is normalised by the sum over the fluid-solid pairs of |f|.
    MEASURED here against the oracle: 8.6e-08 (the oracle's build rounds every f32 operation once, on any machine); the bound is 3 x that (README: every test bound is <= 3 x the error measured)."""
    sd = loads_scenes.block_on_slab()
    cfg, sc = scenes.build(sd)
    loads_scenes.squeeze(sc, 0.9, seed=1)
    o = scenes.make_oracle(cfg, sc)
    o.initialize()
    o.initialize_particle_system()
    o.compute_moving_boundary_volume()
    o.compute_densities()
    o.compute_non_pressure_forces()
    o.compute_pressure_forces()
    f = {k: o[k].copy() for k in ("x", "m_V", "m", "density", "pressure", "material", "object_id", "acceleration")}
    fluid = f["material"] == 1
    assert fluid.sum() == 216 and (~fluid).sum() == 128 and np.unique(f["m"][fluid]).size == 1
    par = scenes.solver_params(cfg, sc)
    h, rho0 = sc.geom.support_radius, par["density_0"]
    rows = model.sample(f["x"], f["m_V"], f["material"], f["object_id"], f["m"], f["density"], f["pressure"], [1], (0.0, 0.0, 0.0), h, rho0)
    F = rows[0, 0:3].astype(np.float64) / 2.0 ** 24
    g = np.asarray(par["g"], dtype=np.float64)
    fluid_side = (f["m"][fluid].astype(np.float64)[:, None] * (f["acceleration"][fluid].astype(np.float64) - g)).sum(axis=0)
    norm = model.pair_magnitude(f["x"], f["m_V"], f["material"], f["object_id"], f["m"], f["density"], f["pressure"], [1], h, rho0)
    residual = float(np.abs(fluid_side + F).max() / norm)
    print(f"load {F}, fluid side {fluid_side}, sum over pairs of |f| {norm:.6e}, residual {residual:.3e}; pairs {rows[0, 6]}, wet {rows[0, 7]}")
    assert rows[0, 6] > 100 and rows[0, 7] >= 36 and rows[0, 8] == 0 and norm > 1.0
    assert F[1] < 0 and abs(F[1]) > 0.5 * norm                        # the fluid presses the slab DOWN, and mostly straight down
    assert residual <= 3 * 8.6e-08
