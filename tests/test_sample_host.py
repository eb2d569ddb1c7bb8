"""Host side of the field sampling (no GPU): the C ABI additions and their ctypes mirror, the numpy model against sums computed
by hand, the derived views of `FieldGrid` / `FieldProbes`, the VTK writer, and the driver's scene keys."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from sph_taichi_amd import _lib, build, sample
from sph_taichi_amd.config_builder import SimConfig
from tests import sample_model as model
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
F32 = np.float32
ENTRIES = ("sph_sample_grid", "sph_sample_grid_download", "sph_sample_points", "sph_sample_points_download")


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_section():
    assert re.search(r"int32_t\s+sph_sample_grid\s*\(\s*SphContext\s*\*\s*\w*\s*,\s*const\s+SphSampleGrid\s*\*\s*\w*\s*\)\s*;", HEADER)
    for name in ENTRIES:
        assert re.search(rf"int32_t\s+{name}\s*\(\s*SphContext\s*\*", HEADER), name
    for name in ("SphSampleGrid", "SphSampleSelect"):
        assert re.search(rf"typedef\s+struct\s+{name}\s*\{{", HEADER) and re.search(rf"\}}\s*{name}\s*;", HEADER)
    assert re.search(r"#define\s+SPH_SAMPLE_MAX_NODES\s+\(1\s*<<\s*24\)", HEADER) and _lib.SAMPLE_MAX_NODES == 1 << 24 == sample.MAX_NODES
    assert re.search(r"#define\s+SPH_SAMPLE_MAX_POINTS\s+1024\b", HEADER) and _lib.SAMPLE_MAX_POINTS == 1024 == sample.MAX_POINTS
    assert re.search(r"#define\s+SPH_SAMPLE_SCALE_LOG2\s+30\b", HEADER) and _lib.SAMPLE_SCALE_LOG2 == 30 == sample.SCALE_LOG2
    for k, name in enumerate(("VX", "VY", "VZ", "DENSITY", "PRESSURE")):
        assert re.search(rf"#define\s+SPH_SAMPLE_{name}\s+{1 << k}\b", HEADER) and getattr(_lib, f"SAMPLE_{name}") == 1 << k
    assert [sample.PLANE_BITS[p] for p in model.PLANES] == [1, 2, 4, 8, 16]
    assert re.search(r"#define\s+SPH_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6      # additive: the version stays
    assert HEADER.index("sph_sample_grid") > HEADER.index("sph_export_download")
    section = HEADER[HEADER.index("Field sampling"):]
    for word in ("2^54", "2^9", "one dt behind", "SPH_E_STATE", "support_radius / 8", "acceleration is not read"):
        assert word in section, word


def test_struct_layouts():
    assert ctypes.sizeof(_lib.SphSampleSelect) == 4 + 4 + 32 * 4 == 136
    assert [(n, getattr(_lib.SphSampleSelect, n).offset) for n, _ in _lib.SphSampleSelect._fields_] == \
        [("material", 0), ("n_objects", 4), ("object_ids", 8)]
    table = {"n": 0, "origin": 12, "spacing": 24, "inv_h": 36, "fields": 40, "select": 44}
    assert [n for n, _ in _lib.SphSampleGrid._fields_] == list(table)
    for name, off in table.items():
        assert getattr(_lib.SphSampleGrid, name).offset == off, name
    assert ctypes.sizeof(_lib.SphSampleGrid) == 44 + 136


def test_binding_and_build_list():
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ENTRIES:
        assert name in bound and bound[name][0] is ctypes.c_int32, name
    assert bound["sph_sample_grid"][1] == [ctypes.c_void_p, ctypes.POINTER(_lib.SphSampleGrid)]
    assert bound["sph_sample_grid_download"][1] == [ctypes.c_void_p] * 4 + [ctypes.c_int64]
    assert bound["sph_sample_points"][1] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.POINTER(_lib.SphSampleSelect), ctypes.c_float]
    assert bound["sph_sample_points_download"][1] == [ctypes.c_void_p] * 4 + [ctypes.c_int32]
    assert "sph_sample.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "sph_sample.hip"))


# ---- the model against sums computed by hand --------------------------------------------------------------------------------
# A lattice whose every coordinate is exact in f32: d = 2^-5, h = 4 d = 2^-3, so inv_h = 8, r^2 = n d^2 and q = sqrt_f32(n) / 4 exactly.
D = 2.0 ** -5
H = 4 * D
KW = model.k_w(H)
MV = F32(0.8 * D ** 3)


def _scalar_w(n2):
    """w of a lattice offset with i^2 + j^2 + k^2 = n2, written out as scalar f32 steps (independent of the model's arrays)."""
    q = F32(np.sqrt(F32(n2))) * F32(0.25)
    if not q <= F32(1):
        return None
    if q <= F32(0.5):
        q2 = F32(q * q)
        q3 = F32(q2 * q)
        W = F32(KW * F32(F32(F32(F32(6) * q3) - F32(F32(6) * q2)) + F32(1)))
    else:
        t = F32(F32(1) - q)
        W = F32(F32(KW * F32(2)) * F32(F32(t * t) * t))
    return min(max(F32(MV * W), F32(0)), F32(4))


def _lattice(n):
    k = np.arange(n, dtype=np.float64) * D
    return np.stack([a.reshape(-1) for a in np.meshgrid(k, k, k, indexing="ij")], axis=1).astype(F32)


def test_rest_lattice_fill_equals_the_hand_sum():
    x = _lattice(11)
    n = x.shape[0]
    centre = np.array([[5 * D, 5 * D, 5 * D]], dtype=F32)                 # four spacings from every face: a full neighbourhood
    got = model.sample(centre, x, np.full(n, MV), [], np.ones(n, bool), model.inv_h(H), KW)
    want_w = want_c = 0
    for i in range(-4, 5):
        for j in range(-4, 5):
            for k in range(-4, 5):
                w = _scalar_w(i * i + j * j + k * k)
                if w is not None:
                    want_c += 1
                    want_w += int(np.rint(float(w) * 2.0 ** 30))
    assert want_c == 257                                                   # lattice points with i^2 + j^2 + k^2 <= 16
    assert got["count"].tolist() == [want_c] and got["weight"].tolist() == [want_w]
    fill = want_w / 2.0 ** 30
    assert abs(fill - 0.8) < 1e-3, fill                                    # m_V0 = 0.8 d^3: the Shepard sum of a rest lattice is 0.8


def test_uniform_velocity_comes_back_within_the_rounding_bound():
    x = _lattice(7)
    n = x.shape[0]
    v = np.tile(np.array([0.3, -1.7, 2.0 ** -9], dtype=F32), (n, 1))
    origin, spacing, shape = (-0.14, -0.13, -0.15), (0.033, 0.037, 0.041), (12, 11, 10)
    pos = model.node_positions(origin, spacing, shape)
    got = model.sample(pos, x, np.full(n, MV), model.values_of(("vx", "vy", "vz"), v, None, None), np.ones(n, bool), model.inv_h(H), KW)
    grid = sample.FieldGrid(got["weight"], got["count"], got["sums"], ("vx", "vy", "vz"), time=0.25, origin=origin, spacing=spacing, shape=shape)
    assert np.array_equal(grid.positions.reshape(-1, 3), pos)
    has = grid.weight > 0
    assert has.any() and not has.all()
    # each llrint errs by at most 1/2, in the numerator (count terms) and the denominator alike: |sum / weight - v| <= count (|v| + 1) / (2 weight)
    bound = grid.count[has] / grid.weight[has]
    for a in range(3):
        err = np.abs(grid.velocity[..., a][has] - float(v[0, a]))
        assert (err <= bound * max(abs(float(v[0, a])), 1.0)).all(), (a, err.max(), bound.max())
    assert np.isnan(grid.velocity[~has]).all()
    assert ((grid.fill >= 0) & (grid.fill <= 4 * grid.count)).all()
    assert np.array_equal(grid.wet(0.5), grid.fill >= 0.5) and grid.time == 0.25 and grid.fields == ("velocity",)
    with pytest.raises(ValueError, match="pressure was not sampled"):
        grid.pressure


def test_the_three_branches_of_q():
    x = np.array([[0.5, 0.5, 0.5]], dtype=F32)
    pts = np.array([[0.5, 0.5, 0.5],                      # q == 0: W = k_w
                    [0.5 + H / 2, 0.5, 0.5],              # q == 0.5: the inner branch, k_w / 4
                    [0.5, 0.5 - H, 0.5],                  # q == 1: contributes, with W = 0
                    [0.5, 0.5, np.nextafter(F32(0.5 + H), F32(1))]], dtype=F32)   # just outside
    got = model.sample(pts, x, np.array([MV]), [np.array([3.0], dtype=F32)], np.ones(1, bool), model.inv_h(H), KW)
    w0 = int(np.rint(float(F32(MV * KW)) * 2.0 ** 30))
    wh = int(np.rint(float(F32(MV * F32(KW * F32(0.25)))) * 2.0 ** 30))
    assert got["count"].tolist() == [1, 1, 1, 0]
    assert got["weight"].tolist() == [w0, wh, 0, 0] and w0 > wh > 0
    assert got["sums"][0].tolist() == [int(np.rint(float(F32(MV * KW)) * 3.0 * 2.0 ** 30)), int(np.rint(float(F32(MV * F32(KW * F32(0.25)))) * 3.0 * 2.0 ** 30)), 0, 0]
    # a NaN position contributes nowhere, a NaN volume counts with weight 0, a velocity beyond 2^24 clamps
    x2 = np.array([[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, 0.5, 0.5]], dtype=F32)
    got = model.sample(pts[:1], x2, np.array([MV, MV, np.nan], dtype=F32), [np.array([2.0 ** 25, 1.0, 1.0], dtype=F32)], np.ones(3, bool),
                       model.inv_h(H), KW)
    assert got["count"].tolist() == [2] and got["weight"].tolist() == [w0]
    assert got["sums"][0].tolist() == [int(np.rint(float(F32(MV * KW)) * 2.0 ** 24 * 2.0 ** 30))]


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_defaults_and_argument_errors():
    ga = sample.grid_args(particle_diameter=0.02, domain_size=(1.0, 1.2, 0.8))
    assert ga["spacing"] == (float(F32(0.02)),) * 3 and ga["origin"] == (0.0, 0.0, 0.0)
    assert all(ga["origin"][a] + (ga["shape"][a] - 1) * ga["spacing"][a] >= size for a, size in enumerate((1.0, 1.2, 0.8)))
    assert all(ga["origin"][a] + (ga["shape"][a] - 2) * ga["spacing"][a] < size for a, size in enumerate((1.0, 1.2, 0.8)))
    ga = sample.grid_args(0.05, (0.1, -0.2, 0.3), (1, 7, 9), particle_diameter=0.02, domain_size=(1, 1, 1))
    assert ga["shape"] == (1, 7, 9) and ga["spacing"] == (float(F32(0.05)),) * 3 and ga["origin"][1] == float(F32(-0.2))
    for bad, msg in ((dict(spacing=0.0), "positive"), (dict(spacing=(0.1, -1, 0.1)), "positive"), (dict(spacing=(1, 2)), "one per axis"),
                     (dict(spacing=float("nan")), "finite"), (dict(origin=(0, float("inf"), 0)), "finite"), (dict(shape=(4, 4)), "three"),
                     (dict(shape=(4, 0, 4)), "at least 1"), (dict(shape=(4, 2.5, 4)), "integer"), (dict(shape=(1 << 10, 1 << 10, 17)), "at most")):
        with pytest.raises(ValueError, match=msg):
            sample.grid_args(**{"spacing": None, "origin": None, "shape": None, **bad}, particle_diameter=0.02, domain_size=(1, 1, 1))
    sel = sample.select_args()
    assert sel == {"fields": ("velocity",), "planes": ("vx", "vy", "vz"), "mask": 7, "material": 1, "objects": []}
    sel = sample.select_args(fields=("pressure", "velocity", "density"), material=None, objects=[2, 0])
    assert sel["planes"] == model.PLANES and sel["mask"] == 31 and sel["material"] == -1 and sel["objects"] == [2, 0]
    assert sample.select_args(fields=(), material="solid", objects=3) == {"fields": (), "planes": (), "mask": 0, "material": 0, "objects": [3]}
    for bad, msg in ((dict(fields="velocity"), "not one string"), (dict(fields=("speed",)), "unknown field"), (dict(fields=("density", "density")), "twice"),
                     (dict(material="gas"), "material"), (dict(material=256), "material id"), (dict(objects=[]), "empty"),
                     (dict(objects=list(range(33))), "at most 32"), (dict(objects=[-1]), "negative"), (dict(objects=[1.5]), "integer")):
        with pytest.raises(ValueError, match=msg):
            sample.select_args(**bad)
    assert sample.points_arg([0.1, 0.2, 0.3]).shape == (1, 3) and sample.points_arg(np.zeros((1024, 3))).dtype == F32
    for bad, msg in (([], "triples"), ([[1, 2]], "triples"), (np.zeros((1025, 3)), "1024"), ([[0, float("nan"), 0]], "finite"), ([[1e39, 0, 0]], "finite")):
        with pytest.raises(ValueError, match=msg):
            sample.points_arg(bad)
    assert sample.inv_h_f32(0.08) == float(F32(1) / F32(0.08))


def test_probe_rows():
    pr = sample.FieldProbes([[0.5, 0.25, 0.125], [9, 9, 9]], [1 << 29, 0], [3, 0], [[1 << 28, 0], [-(1 << 29), 0], [0, 0], [5 << 29, 0]],
                            ("vx", "vy", "vz", "pressure"), time=1.5)
    assert pr.fields == ("velocity", "pressure") and pr.fill.tolist() == [0.5, 0.0]
    assert pr.rows() == [{"point": [0.5, 0.25, 0.125], "count": 3, "fill": 0.5, "velocity": [0.5, -1.0, 0.0], "pressure": 5.0},
                         {"point": [9.0, 9.0, 9.0], "count": 0, "fill": 0.0, "velocity": [None, None, None], "pressure": None}]


def test_write_vtk_round_trip(tmp_path):
    shape = (2, 3, 4)
    rng = np.random.default_rng(5)
    weight = rng.integers(0, 1 << 30, size=shape)
    weight[0, 1, 2] = 0
    sums = rng.integers(-(1 << 31), 1 << 31, size=(4,) + shape)
    grid = sample.FieldGrid(weight, (weight > 0) * 7, sums, ("vx", "vy", "vz", "pressure"), time=0.5, origin=(0.1, -0.2, 0.3),
                            spacing=(0.02, 0.04, 0.01), shape=shape)
    path = tmp_path / "grid.vtk"
    grid.write_vtk(path)
    raw = path.read_bytes()
    head = raw.split(b"POINT_DATA 24\n")[0].decode("ascii").splitlines()
    assert head[0] == "# vtk DataFile Version 3.0" and "0.5" in head[1] and head[2:4] == ["BINARY", "DATASET STRUCTURED_POINTS"]
    assert head[4] == "DIMENSIONS 2 3 4"
    assert [float(v) for v in head[5].split()[1:]] == [float(F32(0.1)), float(F32(-0.2)), float(F32(0.3))] and head[5].startswith("ORIGIN ")
    assert [float(v) for v in head[6].split()[1:]] == [float(F32(0.02)), float(F32(0.04)), float(F32(0.01))] and head[6].startswith("SPACING ")
    rest = raw.split(b"POINT_DATA 24\n")[1]

    def take(label, comps):
        nonlocal rest
        assert rest.startswith(label), (label, rest[:40])
        body = rest[len(label):len(label) + 24 * comps * 4]
        assert rest[len(label) + len(body):][:1] == b"\n"
        rest = rest[len(label) + len(body) + 1:]
        return np.frombuffer(body, dtype=">f4").reshape((4, 3, 2) + ((comps,) if comps > 1 else ()))   # z slowest, x fastest

    fill = take(b"SCALARS fill float 1\nLOOKUP_TABLE default\n", 1)
    vel = take(b"VECTORS velocity float\n", 3)
    prs = take(b"SCALARS pressure float 1\nLOOKUP_TABLE default\n", 1)
    assert rest == b""
    assert np.array_equal(fill, grid.fill.astype(F32).transpose(2, 1, 0))
    assert np.array_equal(vel, grid.velocity.astype(F32).transpose(2, 1, 0, 3), equal_nan=True)
    assert np.array_equal(prs, grid.pressure.astype(F32).transpose(2, 1, 0), equal_nan=True)
    assert np.isnan(prs[2, 1, 0]) and np.isnan(vel[2, 1, 0]).all() and fill[2, 1, 0] == 0 and not np.isnan(prs).all()


def _config(**keys):
    sd = scenes.fluid_only(counts=(3, 3, 3))
    sd["Configuration"].update(keys)
    return SimConfig(config=sd)


def test_driver_scene_keys():
    assert sample.sample_grid_config(_config()) is None and sample.probes_config(_config()) is None
    assert sample.sample_grid_config(_config(sampleGrid={})) == {"spacing": None, "origin": None, "shape": None, "fields": ("velocity",), "objects": None}
    kw = sample.sample_grid_config(_config(sampleGrid={"spacing": 0.04, "origin": [0.1, 0.1, 0.1], "shape": [1, 5, 5], "fields": ["velocity", "pressure"],
                                                       "objects": [0]}))
    assert kw == {"spacing": 0.04, "origin": [0.1, 0.1, 0.1], "shape": [1, 5, 5], "fields": ("velocity", "pressure"), "objects": [0]}
    for bad, msg in (({"spacing": -1}, "positive"), ({"cell": 0.1}, "unknown key"), ({"fields": "velocity"}, "list of names"), ({"fields": ["speed"]}, "unknown field"),
                     ({"shape": [0, 1, 1]}, "at least 1"), ({"objects": []}, "empty")):
        with pytest.raises(ValueError, match=f'"sampleGrid".*{msg}'):
            sample.sample_grid_config(_config(sampleGrid=bad))
    with pytest.raises(ValueError, match="must be an object"):
        sample.sample_grid_config(_config(sampleGrid=[1]))
    kw = sample.probes_config(_config(probes={"points": [[0.5, 0.25, 0.125]], "fields": ["pressure"]}))
    assert kw == {"points": [[0.5, 0.25, 0.125]], "fields": ("pressure",)}
    assert sample.probes_config(_config(probes={"points": [[0.5, 0.25, 0.125]]}))["fields"] == ("velocity",)
    for bad, msg in (({}, "points is missing"), ({"points": [[1, 2]]}, "triples"), ({"points": [[0, 0, 0]], "field": []}, "unknown key"),
                     ({"points": [[0, 0, 0]], "fields": ["mass"]}, "unknown field")):
        with pytest.raises(ValueError, match=f'"probes".*{msg}'):
            sample.probes_config(_config(probes=bad))
    from sph_taichi_amd import run_simulation
    assert run_simulation.build_parser().parse_args(["--probes", "p.jsonl"]).probes == "p.jsonl"
    assert run_simulation.build_parser().parse_args([]).probes == ""
