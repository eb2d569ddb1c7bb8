"""Host side of the particle export (no GPU): the C ABI additions and their ctypes mirror, the numpy model on hand-made arrays,
the binary PLY writer against the reader of tests/export_model.py, the scene key and the argument checking of `export_particles`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from sph_taichi_amd import _lib, build, export
from sph_taichi_amd.config_builder import SimConfig
from tests import export_model as model
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_section():
    assert re.search(r"int32_t\s+sph_export_select\s*\(\s*SphContext\s*\*\s*\w*\s*,\s*const\s+SphExportParams\s*\*\s*\w*\s*\)\s*;", HEADER)
    assert re.search(r"int32_t\s+sph_export_info\s*\(\s*SphContext\s*\*\s*\w*\s*,\s*SphExportInfo\s*\*\s*\w*\s*\)\s*;", HEADER)
    assert re.search(r"int32_t\s+sph_export_download\s*\(\s*SphContext\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*,\s*size_t\s+\w*\s*\)\s*;", HEADER)
    for name in ("SphExportParams", "SphExportInfo"):
        assert re.search(rf"typedef\s+struct\s+{name}\s*\{{", HEADER) and re.search(rf"\}}\s*{name}\s*;", HEADER)
    bits = {"X": 1, "V": 2, "DENSITY": 4, "PRESSURE": 8, "MASS": 16, "ID": 32, "OBJECT": 64}
    for name, bit in bits.items():
        assert re.search(rf"#define\s+SPH_EXPORT_{name}\s+{bit}\b", HEADER), name
        assert getattr(_lib, f"EXPORT_{name}") == bit
    assert re.search(r"#define\s+SPH_EXPORT_MAX_OBJECTS\s+32\b", HEADER) and _lib.EXPORT_MAX_OBJECTS == 32 == export.MAX_OBJECTS
    assert export.EXPORT_X == 1 and export.FIELD_BITS == {"velocity": 2, "density": 4, "pressure": 8, "mass": 16, "id": 32, "object": 64}
    assert re.search(r"#define\s+SPH_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6      # additive: the version stays
    assert HEADER.index("sph_export_select") > HEADER.index("sph_columns_download")             # behind the column maps


def _header_struct_fields(name):
    """(c type, field name, array length) of every member of `typedef struct name { ... } name;` in the header."""
    body = re.search(rf"typedef\s+struct\s+{name}\s*\{{(.*?)\}}\s*{name}\s*;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(SPH_\w+)\s+(\d+)\b", HEADER)}
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for item in rest.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", item)
            length = m.group(2)
            out.append((ctype, m.group(1), 1 if length is None else int(consts.get(length, length))))
    return out


C_SIZE = {"int32_t": 4, "int64_t": 8, "float": 4}


def _natural_layout(fields):
    """offsets and size of a C struct of these members under natural alignment"""
    off, offsets, align = 0, {}, 1
    for ctype, name, length in fields:
        a = C_SIZE[ctype]
        off = (off + a - 1) // a * a
        offsets[name] = off
        off += a * length
        align = max(align, a)
    return offsets, (off + align - 1) // align * align


@pytest.mark.parametrize("name", ["SphExportParams", "SphExportInfo"])
def test_struct_layouts_follow_the_header(name):
    fields = _header_struct_fields(name)
    mirror = getattr(_lib, name)
    assert [n for n, _ in mirror._fields_] == [n for _, n, _ in fields]
    offsets, size = _natural_layout(fields)
    assert ctypes.sizeof(mirror) == size
    for n, off in offsets.items():
        assert getattr(mirror, n).offset == off, n
    # the sizes written out: 3 + 32 + 3 i32 and 6 f32; 2 i64 and 2 i32
    assert size == {"SphExportParams": 4 * (3 + 32 + 3 + 6), "SphExportInfo": 24}[name]


def test_binding_and_build_list():
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert bound["sph_export_select"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(_lib.SphExportParams)])
    assert bound["sph_export_info"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(_lib.SphExportInfo)])
    assert bound["sph_export_download"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t])
    assert "sph_export.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "sph_export.hip"))


# ---- the model on hand-made arrays ------------------------------------------------------------------------------------------
NAN = np.float32("nan")
HAND = dict(
    x=np.array([[0.5, 0.5, 0.5], [1.0, 0.25, 0.75], [0.0, 0.0, 0.0], [NAN, 0.5, 0.5], [0.25, 1.0, 0.5], [0.75, 0.75, 0.75],
                [0.5, 0.5, 1.5]], dtype=np.float32),
    v=np.arange(21, dtype=np.float32).reshape(7, 3),
    density=np.array([1000, 1001, 1002, 1003, 1004, 1005, 1006], dtype=np.float32),
    pressure=np.array([0, -1, 2, -3, 4, -5, 6], dtype=np.float32),
    m=np.array([8, 8, 8, 8, 6, 6, 6], dtype=np.float32) * np.float32(1e-3),
    material=np.array([1, 1, 1, 1, 0, 0, 1], dtype=np.int32),
    object_id=np.array([0, 0, 0, 0, 1, 2, 3], dtype=np.int32),
    pid=np.array([5, 2, 9, 0, 7, 3, 4], dtype=np.int32))


def test_model_order_and_columns():
    m = model.export_rows(**HAND, fields=model.ALL_FIELDS)
    assert (m["selected"], m["rows"], m["duplicate_ids"]) == (7, 7, 0)
    d = m["data"]
    assert d.dtype.names == ("x", "y", "z", "vx", "vy", "vz", "density", "pressure", "mass", "id", "object") and d.dtype.itemsize == 44
    assert d["id"].tolist() == [0, 2, 3, 4, 5, 7, 9]                        # ascending persistent id
    order = [3, 1, 5, 6, 0, 4, 2]                                         # the records that carry those ids
    assert d["object"].tolist() == HAND["object_id"][order].tolist() and d["density"].tolist() == HAND["density"][order].tolist()
    assert d["vx"].tolist() == HAND["v"][order, 0].tolist() and d["mass"].tobytes() == HAND["m"][order].tobytes()
    assert np.isnan(d["x"][0]) and d["y"][0] == 0.5
    only_x = model.export_rows(**HAND)["data"]
    assert only_x.dtype.names == ("x", "y", "z") and only_x.tobytes() == HAND["x"][order].tobytes()
    some = model.export_rows(**HAND, fields=("object", "pressure"))["data"]    # the row order is the header's, not the caller's
    assert some.dtype.names == ("x", "y", "z", "pressure", "object")


def test_model_selection():
    ids = lambda **kw: model.export_rows(**HAND, fields=("id",), **kw)["data"]["id"].tolist()
    assert ids(select_material=1) == [0, 2, 4, 5, 9] and ids(select_material=0) == [3, 7]
    assert ids(objects=[0]) == [0, 2, 5, 9] and ids(objects=[2, 1]) == [3, 7] and ids(objects=[17]) == []
    assert ids(every=3, phase=0) == [0, 3, 9] and ids(every=3, phase=1) == [4, 7] and ids(every=3, phase=2) == [2, 5]
    assert ids(every=1) == [0, 2, 3, 4, 5, 7, 9]
    # box edges are inclusive; the NaN position (id 0) is outside every box
    assert ids(box=([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])) == [2, 3, 5, 7, 9]
    assert ids(box=([0.5, 0.25, 0.5], [1.0, 0.5, 0.75])) == [2, 5]
    assert ids(box=([0.5, 0.5, 0.5], [0.5, 0.5, 0.5])) == [5]
    big = np.finfo(np.float32).max
    assert ids(box=([-big] * 3, [big] * 3)) == [2, 3, 4, 5, 7, 9]
    assert ids(box=([0.0, 0.0, 0.0], [1.0, 1.0, 1.0]), select_material=1, every=2, phase=1) == [5, 9]
    # the box is compared in f32: a bound that rounds onto the coordinate keeps it
    assert ids(box=([0.0, 0.0, 0.0], [0.75 + 1e-12, 0.75, 0.75]), objects=[2]) == [3]


def test_model_empty_selection_and_duplicates():
    m = model.export_rows(**HAND, fields=("velocity", "id"), objects=[9])
    assert (m["selected"], m["rows"], m["duplicate_ids"]) == (0, 0, 0)
    assert m["data"].shape == (0,) and m["data"].dtype == model.row_dtype(("velocity", "id")) and m["data"].tobytes() == b""
    dup = dict(HAND, pid=np.array([5, 2, 9, 0, 7, 2, 4], dtype=np.int32))
    m = model.export_rows(**dup)
    assert (m["selected"], m["rows"], m["duplicate_ids"]) == (7, 6, 1) and m["data"] is None
    assert model.export_rows(**dup, select_material=1)["duplicate_ids"] == 0          # the second holder of id 2 is a solid


# ---- write_ply ----------------------------------------------------------------------------------------------------------------
SUBSETS = [(), ("id",), ("id", "object"), ("velocity",), ("velocity", "id"), ("velocity", "density", "object"),        # 3 .. 11 words
           ("velocity", "density", "pressure", "mass"), ("velocity", "density", "pressure", "mass", "id"), model.ALL_FIELDS]


@pytest.mark.parametrize("fields", SUBSETS, ids=[str(3 + sum(3 if f == "velocity" else 1 for f in s)) + "_words" for s in SUBSETS])
def test_write_ply_round_trip(tmp_path, fields):
    assert export.row_dtype(fields) == model.row_dtype(fields)
    data = model.export_rows(**HAND, fields=fields)["data"]
    path = tmp_path / "p.ply"
    export.write_ply(str(path), data, comments=("frame 3",))
    got, comments, body = model.read_ply(path)
    assert body == data.tobytes() and got.dtype == data.dtype and got.tobytes() == data.tobytes()
    assert comments == ["created by sph_taichi_amd", "frame 3"]
    # through ParticleExport, and an empty selection
    ex = export.ParticleExport(data, 7, fields, 0.125)
    assert (ex.count, ex.selected, ex.fields, ex.time) == (7, 7, tuple(fields), 0.125)
    ex.write_ply(str(path))
    got, comments, body = model.read_ply(path)
    assert body == data.tobytes() and comments[-1] == "time 0.125"
    export.write_ply(str(path), data[:0])
    got, _, body = model.read_ply(path)
    assert got.shape == (0,) and body == b"" and got.dtype == data.dtype


def test_write_ply_refuses_what_it_cannot_describe(tmp_path):
    p = str(tmp_path / "q.ply")
    for bad in (np.zeros(3, np.float32), np.zeros((2, 2), dtype=[("x", "<f4")]), np.zeros(2, dtype=[("x", "<f8")]),
                np.zeros(2, dtype=np.dtype({"names": ["x", "y"], "formats": ["<f4", "<f4"], "offsets": [0, 8], "itemsize": 12}))):
        with pytest.raises(ValueError):
            export.write_ply(p, bad)
    with pytest.raises(ValueError):
        export.write_ply(p, np.zeros(1, dtype=[("x", "<f4")]), comments=("two\nlines",))


# ---- the scene key --------------------------------------------------------------------------------------------------------------
def test_export_config_defaults_and_bad_keys():
    sd = scenes.fluid_only()
    assert export.export_config(SimConfig(config=sd)) is None
    sd["Configuration"]["exportParticles"] = {}
    assert export.export_config(SimConfig(config=sd)) == {"objects": None, "material": None, "fields": (), "box": None, "every": 1, "phase": 0}
    sd["Configuration"]["exportParticles"] = {"objects": [0, 2], "material": "fluid", "fields": ["id", "velocity"], "every": 4, "phase": 3,
                                              "box": [[0, 0, 0], [1, 0.5, 1]]}
    assert export.export_config(SimConfig(config=sd)) == {"objects": [0, 2], "material": 1, "fields": ("velocity", "id"), "every": 4, "phase": 3,
                                                          "box": ((0.0, 0.0, 0.0), (1.0, 0.5, 1.0))}
    for bad in ({"object": [0]}, {"fields": ["colour"]}, {"fields": "velocity"}, {"every": 0}, {"every": 2, "phase": 2}, {"objects": []},
                {"box": [[0, 0, 0], [1, 1]]}, {"box": [[1, 0, 0], [0, 1, 1]]}, {"material": "gas"}, [0]):
        sd["Configuration"]["exportParticles"] = bad
        with pytest.raises(ValueError, match="exportParticles"):
            export.export_config(SimConfig(config=sd))


# ---- argument checking, without a context ----------------------------------------------------------------------------------------
def test_select_args_normalises():
    a = export.select_args()
    assert a == {"fields": ("velocity",), "mask": 1 | 2, "material": -1, "objects": [], "box": None, "every": 1, "phase": 0}
    a = export.select_args(objects=3, material="solid", fields=("object", "mass", "density"), box=([0, 0, 0], [1, 2, 3]), every=5, phase=4)
    assert a["fields"] == ("density", "mass", "object") and a["mask"] == 1 | 4 | 16 | 64 and a["material"] == 0 and a["objects"] == [3]
    assert a["box"] == ((0.0, 0.0, 0.0), (1.0, 2.0, 3.0)) and (a["every"], a["phase"]) == (5, 4)
    assert export.select_args(material=1, objects=np.array([1, 2], np.int32))["objects"] == [1, 2]
    assert export.select_args(box=([0.1] * 3, [0.1] * 3))["box"][0] == (float(np.float32(0.1)),) * 3       # the bounds the kernel sees
    p = export.make_params(a)
    assert (p.fields, p.material, p.n_objects, p.object_ids[0], p.pid_stride, p.pid_phase, p.use_box) == (85, 0, 1, 3, 5, 4, 1)
    assert list(p.box_hi) == [1.0, 2.0, 3.0]


@pytest.mark.parametrize("bad", [
    dict(fields=("colour",)), dict(fields="velocity"), dict(fields=("id", "id")), dict(fields=("position",)),
    dict(material="gas"), dict(material=256), dict(material=-1), dict(material=1.5),
    dict(objects=[]), dict(objects=[-1]), dict(objects=list(range(33))), dict(objects=[0.5]), dict(objects=["0"]),
    dict(every=0), dict(every=-2), dict(every=1.0), dict(every=2 ** 31), dict(phase=1), dict(every=3, phase=3), dict(every=3, phase=-1),
    dict(every=True),
    dict(box=[0, 1]), dict(box=([0, 0], [1, 1])), dict(box=([0, 0, 0], [1, 1, float("nan")])), dict(box=([0, 0, 0], [1, float("inf"), 1])),
    dict(box=([0, 0, 0], [1e39, 1, 1])), dict(box=([0, 0.5, 0], [1, 0.25, 1])), dict(box="everything"),
], ids=lambda d: ",".join(f"{k}={v!r}"[:40] for k, v in d.items()))
def test_select_args_value_errors(bad):
    with pytest.raises(ValueError):
        export.select_args(**bad)


def test_export_particles_checks_its_arguments_before_any_device_call():
    """`export` validates first: a stand-in without a context shows no call was made."""
    class NoDevice:
        slab = None

        def _call(self, *a):
            raise AssertionError("a device call was made")
    for bad in (dict(fields=("colour",)), dict(every=0), dict(box=([1, 0, 0], [0, 1, 1])), dict(objects=[])):
        with pytest.raises(ValueError):
            export.export(NoDevice(), **bad)


def test_module_imports_without_the_library():
    code = ("import sys\n"
            "import sph_taichi_amd.export\n"
            "from sph_taichi_amd import _lib\n"
            "assert _lib._LIB is None, 'the library was loaded at import'\n"
            "assert 'torch' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
