"""Host side of the running flow statistics (no GPU): the geometry and default parsing against `sample_grid`'s, the `wet`
conversion, the derived fields from accumulators made by the numpy model (tests/stats_model.py), the VTK file read back, the
"statistics" scene key, the slab-rank refusal, and the C ABI additions with their ctypes mirror against a host program compiled with
the header."""
import ctypes
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from sph_taichi_amd import _lib, build, sample, stats
from sph_taichi_amd.config_builder import SimConfig
from tests import scenes
from tests import stats_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
GEOM = dict(particle_diameter=0.02, domain_size=(1.0, 1.2, 0.8))


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    decls = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("sph_stats_set", "sph_stats_sample", "sph_stats_info", "sph_stats_download", "sph_stats_reset"):
        assert re.search(rf"int32_t\s+{name}\s*\(\s*SphContext\s*\*", decls), name
    assert re.search(r"#define\s+SPH_STATS_MAX_SAMPLES\s+\(1\s*<<\s*19\)", HEADER)
    assert _lib.STATS_MAX_SAMPLES == stats.MAX_SAMPLES == 1 << 19
    section = HEADER[HEADER.index("Running flow statistics ("):]
    assert HEADER.index("Running flow statistics (") > HEADER.index("Passive tracers (")                  # the last section
    for word in ("steps_seen % every == 0", "wet_min", "weight > 0", "1024.0", "2^32", "2^24", "xx xy xz yy yz zz", "2^42", "2^44",
                 "dropped", "no atomics", "bit-identical", "frees nothing", "not part of a\n * checkpoint", "changes nothing",
                 "Density and\n * pressure statistics are out of scope"):
        assert word in section, word


def test_binding():
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = {"sph_stats_set": [vp, ctypes.POINTER(_lib.SphStatsParams)], "sph_stats_sample": [vp],
            "sph_stats_info": [vp, ctypes.POINTER(_lib.SphStatsInfo)], "sph_stats_download": [vp, vp, vp, vp, vp, i64],
            "sph_stats_reset": [vp]}
    for name, args in want.items():
        assert bound[name] == (i32, args), name
    assert "sph_stats.hip" in build.SOURCES


def test_struct_layouts_against_the_host_compiler(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "stats_abi_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "stats_abi_driver.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = {line.split()[0]: line.split()[1:] for line in out.splitlines()}
    pairs = lambda words: {words[k]: int(words[k + 1]) for k in range(1, len(words), 2)}
    assert int(rows["SphSampleGrid"][0]) == ctypes.sizeof(_lib.SphSampleGrid)
    P, I = _lib.SphStatsParams, _lib.SphStatsInfo
    assert int(rows["SphStatsParams"][0]) == ctypes.sizeof(P)
    assert pairs(rows["SphStatsParams"]) == {"every": P.every.offset, "capacity": P.capacity.offset, "wet_min": P.wet_min.offset}
    assert int(rows["SphStatsInfo"][0]) == ctypes.sizeof(I) == 64
    assert pairs(rows["SphStatsInfo"]) == {k: getattr(I, k).offset for k in ("n", "every", "samples", "dropped", "steps_seen", "t_first", "t_last")}
    assert int(rows["SPH_STATS_MAX_SAMPLES"][0]) == 1 << 19


# ---- arguments --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"spacing": 0.05}, {"spacing": [0.05, 0.02, 0.1], "origin": [0.1, 0.0, 0.2]},
                                {"shape": (7, 5, 9), "origin": 0.1}, {"shape": (1, 30, 20), "origin": [0.5, 0.0, 0.0], "spacing": 0.04}])
def test_geometry_is_sample_grids(kw):
    want = sample.grid_args(kw.get("spacing"), kw.get("origin"), kw.get("shape"), **GEOM)
    got = stats.set_args(**kw, **GEOM)
    assert {k: got[k] for k in ("spacing", "origin", "shape")} == want
    assert got["material"] == 1 and got["objects"] == [] and got["every"] == 10 and got["capacity"] == 1 << 19
    assert got["wet_min"] == int(np.rint(np.float64(0.4) * 2 ** 30))


def test_argument_checks():
    assert stats.set_args(material=None, objects=[2, 3], every=1, capacity=5, **GEOM)["material"] == -1
    assert stats.set_args(objects=2, **GEOM)["objects"] == [2]
    for kw in ({"every": 0}, {"every": -3}, {"every": 2.5}, {"every": True}, {"capacity": 0}, {"capacity": (1 << 19) + 1}, {"capacity": 1.5},
               {"wet": -0.1}, {"wet": float("nan")}, {"wet": "x"}, {"wet": 4.5}, {"spacing": 0.0}, {"spacing": [0.1, 0.1]},
               {"shape": (0, 4, 4)}, {"shape": (4, 4)}, {"shape": (4096, 4096, 2)}, {"origin": float("inf")}, {"material": "gas"},
               {"objects": []}, {"objects": list(range(33))}):
        with pytest.raises(ValueError):
            stats.set_args(**kw, **GEOM)


def test_wet_conversion():
    assert stats.wet_min_of(0.4) == int(np.rint(np.float64(0.4) * 2 ** 30)) == 429496730 == model.wet_min(0.4)
    assert stats.wet_min_of(0) == 0 and stats.wet_min_of(1) == 1 << 30 and stats.wet_min_of(4.0) == 1 << 32
    assert stats.wet_min_of(np.float32(0.2)) == int(np.rint(np.float64(np.float32(0.2)) * 2 ** 30))


# ---- the derived fields, from accumulators the model made -------------------------------------------------------------------
SHAPE = (2, 3, 2)
NODES = 12
W = int(0.8 * 2 ** 30)


def _acc(m):
    return stats.Accumulators(m["n_wet"], m["sum_w"], m["sum_u"], m["sum_uu"], samples=m["samples"], shape=SHAPE, origin=(0.1, 0.2, 0.3),
                              spacing=0.05, times=(0.0, 0.004))


def test_constant_velocity_has_no_stress():
    v0 = np.array([1.25, -0.7, 3.0])
    m = model.fresh(NODES)
    for _ in range(37):
        m = model.fold_velocity(m, v0, W)
    a = _acc(m)
    assert (a.n_wet == 37).all() and np.array_equal(a.intermittency(), np.ones(SHAPE)) and np.allclose(a.mean_fill(), 0.8, atol=1e-9)
    assert a.mean_velocity().shape == SHAPE + (3,) and np.abs(a.mean_velocity() - v0).max() <= 2.0 ** -30 * 4
    r = a.reynolds_stress()
    assert r.shape == SHAPE + (3, 3) and np.array_equal(r, np.swapaxes(r, -1, -2))
    # per term: the product rounds to 2^-25, each mean to 2^-33 (times |v0| <= 4 in the product of the means)
    assert np.abs(r).max() <= 2.0 ** -25 + 2 * 4 * 2.0 ** -33 + 1e-15
    assert np.abs(a.tke()).max() <= 1.5 * (2.0 ** -25 + 2 * 4 * 2.0 ** -33) + 1e-15 and a.rms_velocity().max() <= 2.0 ** -11


def test_alternating_velocity_gives_v0_squared():
    v0 = np.array([0.5, -2.0, 1.5])
    m = model.fresh(NODES)
    for k in range(40):
        m = model.fold_velocity(m, v0 if k % 2 == 0 else -v0, W)
    a = _acc(m)
    assert np.abs(a.mean_velocity()).max() <= 2.0 ** -30
    r = a.reynolds_stress()
    want = np.outer(v0, v0)
    assert np.abs(r - want).max() <= 2.0 ** -24                       # <u_a u_b> = v0_a v0_b in every sample, the means vanish
    assert np.allclose(a.rms_velocity(), np.abs(v0), atol=1e-6) and np.allclose(a.tke(), 0.5 * (v0 ** 2).sum(), atol=1e-6)


def test_a_never_wet_node_is_nan_without_a_warning():
    weight = np.full(NODES, W, dtype=np.int64)
    weight[5] = 0                                                     # never wet: weight 0
    weight[7] = model.wet_min(0.4) - 1                                # never wet: below the threshold
    m = model.fresh(NODES)
    for k in range(3):
        m = model.fold_velocity(m, [1.0, 2.0, 3.0], weight, model.wet_min(0.4))
    assert m["n_wet"][5] == 0 and m["n_wet"][7] == 0 and m["sum_w"][7] == 0 and not m["sum_uu"][:, 7].any()
    a = _acc(m)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fields = [a.intermittency(), a.mean_fill(), a.mean_velocity(), a.reynolds_stress(), a.rms_velocity(), a.tke()]
        arrays = a.vtk_arrays()
        empty = _acc(model.fresh(NODES))
        assert np.isnan(empty.intermittency()).all() and np.isnan(empty.tke()).all()
    dry = np.zeros(NODES, bool)
    dry[[5, 7]] = True
    dry = dry.reshape(SHAPE)
    assert np.array_equal(fields[0], np.where(dry, 0.0, 1.0))
    for f in fields[1:]:
        nan = np.isnan(f.reshape(SHAPE + (-1,))).all(axis=-1)
        assert np.array_equal(nan, dry)
    assert len(arrays) == 11


def test_the_clamp_and_the_zero_weight_lane():
    m = model.fold(model.fresh(2), [0, 1 << 20], [[5, 1 << 40], [0, -(1 << 41)], [0, 1 << 20]], 0)
    assert m["n_wet"].tolist() == [0, 1] and m["sum_u"][:, 0].tolist() == [0, 0, 0]
    assert m["sum_u"][:, 1].tolist() == [1024 << 32, -(1024 << 32), 1 << 32]
    assert m["sum_uu"][:, 1].tolist() == [1 << 44, -(1 << 44), 1 << 34, 1 << 44, -(1 << 34), 1 << 24]


# ---- the VTK file -----------------------------------------------------------------------------------------------------------
def test_vtk_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    m = model.fresh(NODES)
    for k in range(6):
        weight = np.where(rng.uniform(size=NODES) < 0.7, W, 0)
        m = model.fold_velocity(m, rng.normal(size=(NODES, 3)), weight)
    a = _acc(m)
    path = str(tmp_path / "statistics.vtk")
    a.write_vtk(path)
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"POINT_DATA")].decode("ascii").split("\n")
    assert head[0] == "# vtk DataFile Version 3.0" and "6 samples" in head[1] and head[2:4] == ["BINARY", "DATASET STRUCTURED_POINTS"]
    assert head[4] == "DIMENSIONS 2 3 2" and head[5].startswith("ORIGIN 0.1") and head[6].startswith("SPACING 0.05")
    back = stats.read_vtk(path)
    assert back["shape"] == SHAPE and np.allclose(back["origin"], (0.1, 0.2, 0.3)) and np.allclose(back["spacing"], 0.05)
    names = ["intermittency", "mean_fill", "mean_velocity", "rms_velocity", "tke"] + [f"reynolds_{n}" for n in ("xx", "xy", "xz", "yy", "yz", "zz")]
    assert list(back["arrays"]) == names
    r = a.reynolds_stress()
    want = {"intermittency": a.intermittency(), "mean_fill": a.mean_fill(), "mean_velocity": a.mean_velocity(), "rms_velocity": a.rms_velocity(),
            "tke": a.tke(), "reynolds_xy": r[..., 0, 1], "reynolds_zz": r[..., 2, 2]}
    for name, w in want.items():
        assert np.array_equal(back["arrays"][name], w.astype(np.float32), equal_nan=True), name


# ---- the scene key ----------------------------------------------------------------------------------------------------------
def _config(**keys):
    sd = scenes.fluid_only(counts=(3, 3, 3))
    sd["Configuration"].update(keys)
    return SimConfig(config=sd)


def test_scene_key():
    assert stats.statistics_config(_config()) is None
    kw = stats.statistics_config(_config(statistics={}))
    assert kw == {"spacing": None, "origin": None, "shape": None, "objects": None, "every": 10, "capacity": None, "wet": 0.4}
    kw = stats.statistics_config(_config(statistics={"spacing": 0.04, "shape": [1, 20, 10], "origin": [0.5, 0, 0], "every": 1, "capacity": 100,
                                                      "wet": 0.2, "objects": [0]}))
    assert kw["spacing"] == 0.04 and kw["shape"] == [1, 20, 10] and kw["every"] == 1 and kw["capacity"] == 100 and kw["wet"] == 0.2
    assert stats.set_args(**kw, **GEOM)["shape"] == (1, 20, 10)
    for bad in ([1, 2], {"spacings": 0.1}, {"every": 0}, {"every": "often"}, {"capacity": 0}, {"wet": -1}, {"spacing": -0.1}, {"shape": [1, 2]},
                {"objects": []}, {"fields": ["velocity"]}):
        with pytest.raises(ValueError, match="statistics"):
            stats.statistics_config(_config(statistics=bad))


def test_command_line_flag():
    from sph_taichi_amd import run_simulation
    args = run_simulation.build_parser().parse_args(["--scene_file", "x.json", "--statistics", "out.vtk"])
    assert args.statistics == "out.vtk"


# ---- slab ranks -------------------------------------------------------------------------------------------------------------
def test_slab_rank_is_refused():
    class Slab:
        slab = {"x_lo": 0}
        particle_diameter, domain_size, support_radius = 0.02, (1.0, 1.2, 0.8), 0.04

        def _call(self, *a):
            raise AssertionError("the library must not be reached")
    with pytest.raises(NotImplementedError, match="single-domain contexts only: a slab rank's ghost records would be counted twice"):
        stats.set_statistics(Slab())
    with pytest.raises(NotImplementedError, match="single-domain"):
        stats.clear_statistics(Slab())
    with pytest.raises(ValueError):                                   # the arguments are checked first, as for the other observers
        stats.set_statistics(Slab(), every=0)
