"""Host side of the column maps (no GPU): the C ABI additions and their ctypes mirror, the numpy model against a map computed
by hand, the derived views of `ColumnMap`, and the driver's flags and scene key."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from sph_taichi_amd import _lib, build, columns
from sph_taichi_amd.config_builder import SimConfig
from tests import columns_model as model
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_section():
    assert re.search(r"int32_t\s+sph_columns_reduce\s*\(\s*SphContext\s*\*\s*\w*\s*,\s*const\s+SphColumnParams\s*\*\s*\w*\s*\)\s*;", HEADER)
    assert re.search(r"int32_t\s+sph_columns_download\s*\(\s*SphContext\s*\*", HEADER)
    for name in ("SphColumnParams", "SphColumnTotals"):
        assert re.search(rf"typedef\s+struct\s+{name}\s*\{{", HEADER) and re.search(rf"\}}\s*{name}\s*;", HEADER)
    assert re.search(r"#define\s+SPH_COLUMNS_MAX\s+\(1\s*<<\s*20\)", HEADER) and _lib.COLUMNS_MAX == 1 << 20 == columns.COLUMNS_MAX
    assert re.search(r"#define\s+SPH_COLUMNS_V_SCALE_LOG2\s+20\b", HEADER) and _lib.COLUMNS_V_SCALE_LOG2 == 20 == columns.V_SCALE_LOG2
    assert re.search(r"#define\s+SPH_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6      # additive: the version stays
    assert HEADER.index("sph_columns_reduce") > HEADER.index("sph_diag_download")               # behind the diagnostics


def test_struct_layouts():
    """SphColumnParams: i32, 2 i32, 2 f32, 2 f32, i32 = 32 bytes; SphColumnTotals: 3 i64 = 24 bytes."""
    assert ctypes.sizeof(_lib.SphColumnParams) == 4 + 8 + 8 + 8 + 4 == 32
    table = {"axis": 0, "n": 4, "origin": 12, "inv_cell": 20, "object_id": 28}
    assert [n for n, _ in _lib.SphColumnParams._fields_] == list(table)
    for name, off in table.items():
        assert getattr(_lib.SphColumnParams, name).offset == off, name
    assert ctypes.sizeof(_lib.SphColumnTotals) == 24
    assert [(n, getattr(_lib.SphColumnTotals, n).offset) for n, _ in _lib.SphColumnTotals._fields_] == \
        [("selected", 0), ("binned", 8), ("outside", 16)]


def test_binding_and_build_list():
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert bound["sph_columns_reduce"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(_lib.SphColumnParams)])
    res, args = bound["sph_columns_download"]
    assert res is ctypes.c_int32 and len(args) == 7 and args[5] is ctypes.c_int32
    assert args[6] == ctypes.POINTER(_lib.SphColumnTotals)
    assert "sph_columns.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "sph_columns.hip"))


# ---- the model against a map computed by hand -------------------------------------------------------------------------------
S = 2.0 ** -20
HAND_X = np.array([[-0.5, 0.2, 0.1],       # column (0, 0)
                   [-0.25, 0.7, 0.3],      # column (0, 0): a negative horizontal coordinate above the negative origin
                   [0.5, -0.3, 0.75],      # column (1, 1): a negative coordinate along the axis
                   [1.5, 0.4, 0.6],        # column (2, 1): velocities that clamp
                   [2.5, 0.1, 0.1],        # k0 = 3: outside
                   [0.5, 0.5, 0.25],       # solid
                   [0.5, 0.9, 0.25]],      # column (1, 0), object 2
                  dtype=np.float32)
HAND_V = np.array([[1.0, 0.0, 0.0], [-0.5 * S, 1.5 * S, 2.0], [0.0, -1.0, 0.0], [70000.0, -70000.0, 0.25], [9.0, 9.0, 9.0],
                   [5.0, 5.0, 5.0], [0.0, 0.5, 0.0]], dtype=np.float32)
HAND_MATERIAL = np.array([1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
HAND_OBJECT = np.array([0, 0, 0, 0, 0, 1, 2], dtype=np.int32)
HAND = dict(axis=1, origin=np.array([-1.0, 0.0], np.float32), inv=model.inv_cell([1.0, 0.5]), shape=(3, 2))


def test_model_against_hand_computed_map():
    assert np.array_equal(HAND["inv"], np.array([1.0, 2.0], np.float32))
    m = model.column_map(HAND_X, HAND_V, HAND_MATERIAL, HAND_OBJECT, HAND["axis"], HAND["origin"], HAND["inv"], HAND["shape"])
    assert (m["selected"], m["binned"], m["outside"]) == (6, 5, 1)
    assert m["count"].tolist() == [[2, 0], [1, 1], [0, 1]]
    one = 1 << 20
    # ties to even: rint(-0.5) = -0 and rint(1.5) = 2; the clamp: +-65536 * 2^20 = +-2^36
    assert m["sum_v"][0].tolist() == [[one + 0, 0], [0, 0], [0, 1 << 36]]
    assert m["sum_v"][1].tolist() == [[2, 0], [one // 2, -one], [0, -(1 << 36)]]
    assert m["sum_v"][2].tolist() == [[2 * one, 0], [0, 0], [0, one // 4]]
    f = lambda v: float(np.float32(v))
    assert m["top"].tolist() == [[f(0.7), 0.0], [f(0.9), f(-0.3)], [0.0, f(0.4)]]
    assert m["bottom"].tolist() == [[f(0.2), 0.0], [f(0.9), f(-0.3)], [0.0, f(0.4)]]
    # one object only: the particle of object 2 leaves, its column empties
    m0 = model.column_map(HAND_X, HAND_V, HAND_MATERIAL, HAND_OBJECT, HAND["axis"], HAND["origin"], HAND["inv"], HAND["shape"],
                          select_object=0)
    assert (m0["selected"], m0["binned"], m0["outside"]) == (5, 4, 1) and m0["count"].tolist() == [[2, 0], [0, 1], [0, 1]]
    assert m0["top"][1, 0] == 0.0 and m0["sum_v"][1][1, 0] == 0
    # the solid's object holds no fluid: nothing selected
    m1 = model.column_map(HAND_X, HAND_V, HAND_MATERIAL, HAND_OBJECT, HAND["axis"], HAND["origin"], HAND["inv"], HAND["shape"],
                          select_object=1)
    assert m1["selected"] == 0 and not m1["count"].any() and not m1["top"].any()
    # the other axes: axis 0 spans (y, z), axis 2 spans (x, y)
    m2 = model.column_map(HAND_X, HAND_V, HAND_MATERIAL, HAND_OBJECT, 2, np.array([-1.0, -1.0], np.float32),
                          model.inv_cell(1.0), (4, 2))
    assert m2["count"].tolist() == [[0, 2], [1, 1], [0, 1], [0, 1]] and m2["outside"] == 0
    assert m2["top"][0, 1] == np.float32(0.3) and m2["bottom"][0, 1] == np.float32(0.1)


# ---- ColumnMap ------------------------------------------------------------------------------------------------------------------
def _hand_map(**over):
    m = model.column_map(HAND_X, HAND_V, HAND_MATERIAL, HAND_OBJECT, HAND["axis"], HAND["origin"], HAND["inv"], HAND["shape"])
    kw = dict(selected=m["selected"], binned=m["binned"], outside=m["outside"], time=0.25, axis=1, cell=(1.0, 0.5),
              origin=(-1.0, 0.0), particle_diameter=0.5)
    kw.update(over)
    return columns.ColumnMap(m["count"], m["sum_v"], m["top"], m["bottom"], **kw), m


def test_column_map_views():
    cm, m = _hand_map()
    assert cm.shape == (3, 2) and cm.axes == (0, 2) and cm.time == 0.25 and cm.cell == (1.0, 0.5) and cm.origin == (-1.0, 0.0)
    assert (cm.selected, cm.binned, cm.outside) == (6, 5, 1)
    # depth = count * d^3 / (cell_0 * cell_1) = count * 0.125 / 0.5
    assert np.array_equal(cm.depth, m["count"] * 0.25)
    # surface = top + radius, NaN where empty
    assert np.isnan(cm.surface[0, 1]) and np.isnan(cm.surface[2, 0])
    assert cm.surface[0, 0] == float(np.float32(0.7)) + 0.25 and cm.surface[1, 1] == float(np.float32(-0.3)) + 0.25
    # velocity = sum_v / 2^20 / count in f64, NaN where empty
    v = cm.velocity
    assert v.shape == (3, 2, 3) and v.dtype == np.float64 and np.isnan(v[0, 1]).all() and np.isnan(v[2, 0]).all()
    assert v[0, 0].tolist() == [0.5, 2 * S / 2, 1.0] and v[1, 1].tolist() == [0.0, -1.0, 0.0]
    assert v[2, 1].tolist() == [65536.0, -65536.0, 0.25]
    d = json.loads(json.dumps(cm.as_dict()))
    assert d["count"] == m["count"].tolist() and d["surface"][0][1] is None and d["wet_extent"] == [[-1.0, 2.0], [0.0, 1.0]]
    assert d["time"] == 0.25 and d["axis"] == 1 and d["selected"] == 6 and d["sum_v"][0][2][1] == 1 << 36


def test_wet_extent_dry_and_wet():
    cm, _ = _hand_map()
    assert cm.wet_extent() == ((-1.0, 2.0), (0.0, 1.0))
    assert cm.wet_extent(min_count=2) == ((-1.0, 0.0), (0.0, 0.5))           # only column (0, 0) holds two
    assert cm.wet_extent(min_count=3) is None
    dry = columns.ColumnMap(np.zeros((3, 2), np.int64), np.zeros((3, 3, 2), np.int64), np.zeros((3, 2), np.float32),
                            np.zeros((3, 2), np.float32), selected=0, binned=0, outside=0, time=0.0, axis=1, cell=0.5, origin=0.0,
                            particle_diameter=0.02)
    assert dry.wet_extent() is None and np.isnan(dry.surface).all() and np.isnan(dry.velocity).all() and not dry.depth.any()
    assert dry.cell == (0.5, 0.5) and dry.origin == (0.0, 0.0)


def test_column_of_on_cell_edges_against_the_model():
    """Points on, just below and just above every cell edge of a map whose cell (0.04) is not a power of two."""
    cell, origin, shape = (0.04, 0.04), (0.0, -0.1), (25, 20)
    cm = columns.ColumnMap(np.zeros(shape, np.int64), np.zeros((3,) + shape, np.int64), np.zeros(shape, np.float32),
                           np.zeros(shape, np.float32), selected=0, binned=0, outside=0, time=0.0, axis=1, cell=cell, origin=origin,
                           particle_diameter=0.02)
    inv = model.inv_cell(cell)
    assert np.array_equal(np.asarray(cm.inv_cell, np.float32), inv) and inv.dtype == np.float32
    edges0 = (np.float32(origin[0]) + np.arange(-1, shape[0] + 2) * np.float32(0.04)).astype(np.float32)
    edges1 = (np.float32(origin[1]) + np.arange(-1, shape[1] + 2) * np.float32(0.04)).astype(np.float32)
    pts = []
    for e0 in edges0:
        for e1 in edges1:
            for a in (np.nextafter(e0, np.float32(-9)), e0, np.nextafter(e0, np.float32(9))):
                for b in (np.nextafter(e1, np.float32(-9)), e1, np.nextafter(e1, np.float32(9))):
                    pts.append((a, b))
    pts = np.array(pts, dtype=np.float32)
    got, want = cm.column_of(pts), model.index(pts, np.asarray(origin, np.float32), inv, shape)
    assert np.array_equal(got, want) and (want == -1).any() and (want >= 0).any() and want.max() == shape[0] * shape[1] - 1
    assert cm.column_of([[np.nan, 0.0]]).tolist() == [-1] and cm.column_of([[1e30, 0.0]]).tolist() == [-1]
    g = cm.gauge([[0.5, 0.5], [99.0, 0.0]])
    assert g["column"].tolist() == [12 * 20 + 15, -1] and g["depth"][0] == 0.0 and np.isnan(g["depth"][1])
    assert np.isnan(g["surface"]).all() and np.isnan(g["velocity"]).all()


def test_gauge_reads_the_columns():
    cm, _ = _hand_map()
    g = cm.gauge([[-0.9, 0.2], [1.5, 0.75], [0.0, 0.99], [-1.5, 0.2]])
    assert g["column"].tolist() == [0, 5, 3, -1]
    assert g["depth"][:3].tolist() == [0.5, 0.25, 0.25] and np.isnan(g["depth"][3])
    assert g["velocity"][1].tolist() == [65536.0, -65536.0, 0.25] and np.isnan(g["velocity"][3]).all()
    rows = json.loads(json.dumps(columns.gauge_rows(cm, [[-0.9, 0.2], [-1.5, 0.2]])))
    assert rows[0]["column"] == 0 and rows[0]["depth"] == 0.5 and rows[1] == {"point": [-1.5, 0.2], "column": -1, "depth": None,
                                                                             "surface": None, "velocity": [None, None, None]}


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_parser_has_the_two_flags():
    from sph_taichi_amd.run_simulation import build_parser
    a = build_parser().parse_args([])
    assert a.gauges == "" and a.heightmap_dir == "" and a.diagnostics == ""
    a = build_parser().parse_args(["--gauges", "g.jsonl", "--heightmap_dir", "hm"])
    assert a.gauges == "g.jsonl" and a.heightmap_dir == "hm"


def test_scene_gauges_key_and_its_defaults():
    sd = scenes.fluid_only()
    assert columns.gauges_config(SimConfig(config=sd)) == {"axis": 1, "cell": None, "points": []}
    sd["Configuration"]["gauges"] = {"axis": 2, "cell": 0.05, "points": [[0.1, 0.2], [0.3, 0.4]]}
    assert columns.gauges_config(SimConfig(config=sd)) == {"axis": 2, "cell": 0.05, "points": [[0.1, 0.2], [0.3, 0.4]]}
    sd["Configuration"]["gauges"] = {"points": [[0.5, 0.5]]}
    assert columns.gauges_config(SimConfig(config=sd)) == {"axis": 1, "cell": None, "points": [[0.5, 0.5]]}
    for bad in ({"axes": 1}, {"axis": 3}, {"cell": 0.0}, {"points": [[1.0, 2.0, 3.0]]}):
        sd["Configuration"]["gauges"] = bad
        with pytest.raises(ValueError):
            columns.gauges_config(SimConfig(config=sd))


def test_heightmap_image():
    cm, _ = _hand_map()
    img = columns.heightmap_image(cm, 2.0)
    assert img.shape == (3, 2, 3) and img.dtype == np.uint8 and (img[..., 0] == img[..., 1]).all() and (img[..., 0] == img[..., 2]).all()
    assert img[0, 1, 0] == 0 and img[1, 1, 0] == 0                         # empty; a surface below zero clips
    assert img[0, 0, 0] == int(np.rint((float(np.float32(0.7)) + 0.25) / 2.0 * 255.0))


def test_module_imports_without_the_library():
    code = ("import sys\n"
            "import sph_taichi_amd.columns\n"
            "from sph_taichi_amd import _lib\n"
            "assert _lib._LIB is None, 'the library was loaded at import'\n"
            "assert 'torch' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
