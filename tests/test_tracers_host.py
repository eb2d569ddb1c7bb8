"""Host side of the passive tracers (no GPU): the numpy model (tests/tracer_model.py) against cases worked out by hand, the
argument checks of `set_tracers`, the "tracers" scene key, the `lattice` helper, the VTK writer read back, and the C ABI additions
with their ctypes mirror."""
import ctypes
import os
import re

import numpy as np
import pytest

from sph_taichi_amd import _lib, build, tracers
from sph_taichi_amd.config_builder import SimConfig
from tests import scenes
from tests import tracer_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
F32 = np.float32
TWO30 = 2.0 ** 30
H = F32(0.04)                                  # support radius = cell size of the hand cases
K_W = F32((8 / np.pi) / float(H) ** 3)


def _params(**kw):
    P = {"grid_size": H, "grid_num": (25, 25, 25), "inv_h": F32(1) / H, "k_w": K_W, "dt": F32(0.001), "padding": F32(0.04),
         "wall_hi": np.array([0.96, 0.96, 0.96], dtype=F32), "min_fill": F32(0.2), "material": 1, "objects": ()}
    P.update(kw)
    return P


def _one(tx, x, v=(1.0, -2.0, 0.5), m_V=None, P=None):
    x = np.asarray(x, dtype=F32).reshape(-1, 3)
    n = x.shape[0]
    m_V = np.full(n, F32(0.8) * F32(0.02) ** 3, dtype=F32) if m_V is None else np.asarray(m_V, dtype=F32)
    vel = np.tile(np.asarray(v, dtype=F32), (n, 1))
    return model.advance(model.fresh(tx), x, vel, m_V, np.ones(n, np.int32), np.zeros(n, np.int32), P or _params())


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    decls = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("sph_tracers_set", "sph_tracers_info", "sph_tracers_download", "sph_tracers_history_download"):
        assert re.search(rf"int32_t\s+{name}\s*\(\s*SphContext\s*\*", decls), name
    assert re.search(r"#define\s+SPH_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6          # additive: the version stays
    assert re.search(r"#define\s+SPH_TRACERS_MAX\s+\(1\s*<<\s*22\)", HEADER) and _lib.TRACERS_MAX == tracers.MAX_TRACERS == 1 << 22
    section = HEADER[HEADER.index("Passive tracers ("):]
    assert HEADER.index("Passive tracers (") > HEADER.index("Surface mesh (")                           # the last section
    for word in ("neighbour_ms", "forward-Euler", "27 cells", "q <= 1.0f", "min_weight", "NOT contracted", "record_every", "dropped",
                 "bit-identical", "frees nothing", "not part of a checkpoint", "A refused call changes nothing"):
        assert word in section, word


def test_binding_and_layouts():
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = {"sph_tracers_set": [vp, vp, i32, ctypes.POINTER(_lib.SphTracerParams)],
            "sph_tracers_info": [vp, ctypes.POINTER(_lib.SphTracerInfo)],
            "sph_tracers_download": [vp, vp, vp, vp, vp, vp, vp, i32],
            "sph_tracers_history_download": [vp, vp, i64, i32]}
    for name, args in want.items():
        assert bound[name] == (i32, args), name
    assert ctypes.sizeof(_lib.SphTracerParams) == 12 + ctypes.sizeof(_lib.SphSampleSelect) == 12 + 8 + 4 * 32
    assert ctypes.sizeof(_lib.SphTracerInfo) == 32 and _lib.SphTracerInfo.advances.offset == 8
    assert "sph_tracers.hip" in build.SOURCES and any(h.endswith("sph_sample_pair.h") for h in build.HEADERS)


# ---- the model against hand-computed cases ----------------------------------------------------------------------------------
def test_one_particle_at_r_zero():
    """W(0) = k_w, w = m_V k_w; the mean of one particle is its velocity up to the rounding of the two llrints."""
    p = [0.5, 0.5, 0.5]
    m_V = F32(0.8) * F32(0.02) ** 3
    w = m_V * (K_W * ((F32(6) * F32(0) - F32(6) * F32(0)) + F32(1)))
    # min_fill below the single particle's weight (about 0.255): wet
    out = _one([p], [p], P=_params(min_fill=F32(0.2)))
    wt = int(np.rint(float(w) * TWO30))
    assert out["count"][0] == 1 and out["weight"][0] == wt
    sums = [int(np.rint((float(w) * a) * TWO30)) for a in (1.0, -2.0, 0.5)]
    u = np.array([F32(s / wt) for s in sums], dtype=F32)
    assert np.array_equal(out["u"][0], u) and np.allclose(u, [1.0, -2.0, 0.5], atol=1e-6)
    assert np.array_equal(out["x"][0], (np.asarray(p, F32) + F32(0.001) * u).astype(F32))
    assert out["wet_steps"][0] == 1 and out["dry_steps"][0] == 0
    # the same particle under a threshold above its weight: dry, nothing moves
    dry = _one([p], [p], P=_params(min_fill=F32(0.3)))
    assert dry["count"][0] == 1 and dry["weight"][0] == wt and not dry["u"].any()
    assert np.array_equal(dry["x"][0], np.asarray(p, F32)) and dry["wet_steps"][0] == 0 and dry["dry_steps"][0] == 1


def test_q_just_inside_and_just_outside_one():
    """A particle along x at a distance whose q is the last f32 at or below 1, and the next one above: in and out."""
    p = np.array([0.5, 0.5, 0.5], dtype=F32)
    inv_h = F32(1) / H
    d = F32(H)
    while (F32(p[0] + d) - p[0]) * inv_h > F32(1):        # the largest offset whose f32 difference still has q <= 1
        d = np.nextafter(d, F32(0))
    x_in = F32(p[0] + d)
    x_out = x_in
    while (x_out - p[0]) * inv_h <= F32(1):
        x_out = np.nextafter(x_out, F32(1))
    assert model.tracer_cells([x_out, p[1], p[2]], H)[0] - model.tracer_cells(p, H)[0] <= 1          # both in the 27 cells
    inside = _one([p], [[x_in, p[1], p[2]]], P=_params(min_fill=F32(1e-9)))
    outside = _one([p], [[x_out, p[1], p[2]]], P=_params(min_fill=F32(1e-9)))
    assert inside["count"][0] == 1 and outside["count"][0] == 0 and outside["weight"][0] == 0
    assert inside["weight"][0] >= 0          # W(1) rounds to (almost) nothing: counted, weighing next to nothing
    assert outside["dry_steps"][0] == 1 and not outside["u"].any()


def test_a_tracer_two_cells_away_is_dry_and_cells_gate_the_pairs():
    p = [0.5, 0.5, 0.5]
    far = _one([p], [[0.5 + 2.5 * float(H), 0.5, 0.5]])
    assert far["count"][0] == 0 and far["weight"][0] == 0 and far["dry_steps"][0] == 1 and np.array_equal(far["x"][0], np.asarray(p, F32))
    # "in the 27 cells AND q <= 1": a pair with q <= 1 whose cells are two apart does not exist at h == cell size, so widen h
    P = _params(inv_h=F32(1) / (F32(3) * H), k_w=F32((8 / np.pi) / (3 * float(H)) ** 3), min_fill=F32(1e-9))
    two_cells = _one([p], [[0.5 + 2.2 * float(H), 0.5, 0.5]], P=P)
    one_cell = _one([p], [[0.5 + 1.2 * float(H), 0.5, 0.5]], P=P)
    assert two_cells["count"][0] == 0 and one_cell["count"][0] == 1
    # selection: a solid particle is nobody to a fluid tracer set
    n = 1
    out = model.advance(model.fresh([p]), np.asarray([p], F32), np.ones((n, 3), F32), np.full(n, 1e-5, F32), np.zeros(n, np.int32),
                        np.zeros(n, np.int32), _params())
    assert out["count"][0] == 0
    # no particles at all: dry
    none = model.advance(model.fresh([p]), np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, F32), np.zeros(0, np.int32),
                         np.zeros(0, np.int32), _params())
    assert none["dry_steps"][0] == 1 and none["count"][0] == 0


def test_walls_clamp_the_advance():
    p = [0.9599, 0.5, 0.0401]
    out = _one([p], [p], v=(50.0, 0.0, -50.0), P=_params(min_fill=F32(0.2)))
    assert out["x"][0, 0] == F32(0.96) and out["x"][0, 2] == F32(0.04) and out["x"][0, 1] == F32(0.5)


def test_min_weight():
    assert model.min_weight(0.2) == int(np.rint(float(F32(0.2)) * TWO30)) and model.min_weight(1e-12) == 1


# ---- Python argument checking ---------------------------------------------------------------------------------------------
def test_set_args():
    a = tracers.set_args([[0.1, 0.2, 0.3]])
    assert a["points"].dtype == np.float32 and a["points"].shape == (1, 3) and a["material"] == 1 and a["objects"] == []
    assert a["min_fill"] == float(F32(0.2)) and a["record_every"] == 0 and a["record_capacity"] == 0
    assert tracers.set_args([0.1, 0.2, 0.3], material=None, objects=[2, 3])["material"] == -1
    assert tracers.set_args([[0.1, 0.2, 0.3]], material="solid", objects=2)["objects"] == [2]
    for bad in ([], [[0.1, 0.2]], "abc", [[np.nan, 0, 0]], [[1e39, 0, 0]], np.zeros((2, 2, 3))):
        with pytest.raises(ValueError):
            tracers.set_args(bad)
    for kw in ({"min_fill": 0.0}, {"min_fill": -1.0}, {"min_fill": 4.5}, {"min_fill": float("nan")}, {"min_fill": "x"},
               {"record_every": -1}, {"record_capacity": -1}, {"record_every": 1.5}, {"record_every": True},
               {"material": "gas"}, {"material": 256}, {"objects": []}, {"objects": [-1]}, {"objects": list(range(33))},
               {"record_capacity": (1 << 31) // 12 + 1}):
        with pytest.raises(ValueError):
            tracers.set_args([[0.1, 0.2, 0.3]], **kw)
    assert tracers.set_args([[0.1, 0.2, 0.3]], min_fill=4.0, record_every=3, record_capacity=(1 << 31) // 12)["record_every"] == 3


def test_history_capacity():
    assert tracers.history_capacity(100, 1000, 0) == 0
    assert tracers.history_capacity(100, 1000, 3) == 333
    assert tracers.history_capacity(1 << 22, 1000, 1) == (1 << 31) // (12 << 22) == 42


# ---- the lattice helper -----------------------------------------------------------------------------------------------------
def test_lattice():
    p = tracers.lattice([0.1, 0.2, 0.3], [0.3, 0.2, 0.35], 0.1)
    assert p.dtype == np.float32 and p.shape == (3, 3)
    assert np.array_equal(p, np.array([[0.1, 0.2, 0.3], [0.2, 0.2, 0.3], [0.1 + 2 * 0.1, 0.2, 0.3]], dtype=np.float32))
    q = tracers.lattice(0.0, 1.0, [0.5, 1.0, 0.25])
    assert q.shape == (3 * 2 * 5, 3) and np.array_equal(q[:6, 2], np.array([0, 0.25, 0.5, 0.75, 1.0, 0], np.float32))    # x slowest
    assert np.array_equal(q[-1], np.array([1, 1, 1], np.float32))
    for bad in (([0, 0, 0], [1, 1, 1], 0.0), ([0, 0, 0], [1, 1, -1], 0.1), ([0, 0], [1, 1, 1], 0.1), ([0, 0, 0], [1, 1, 1], 1e-4)):
        with pytest.raises(ValueError):
            tracers.lattice(*bad)


# ---- the scene key ----------------------------------------------------------------------------------------------------------
def _config(**keys):
    sd = scenes.fluid_only(counts=(3, 3, 3))
    sd["Configuration"].update(keys)
    return SimConfig(config=sd)


def test_scene_key():
    assert tracers.tracers_config(_config()) is None
    kw = tracers.tracers_config(_config(tracers={"points": [[0.3, 0.3, 0.3], [0.4, 0.3, 0.3]]}))
    assert kw["points"].shape == (2, 3) and kw["record_every"] == 1 and kw["min_fill"] == float(F32(0.2)) and kw["objects"] is None
    kw = tracers.tracers_config(_config(tracers={"lattice": {"start": [0.3, 0.3, 0.3], "end": [0.34, 0.3, 0.3], "spacing": 0.02},
                                                 "recordEvery": 5, "minFill": 0.4, "objects": [0]}))
    assert kw["points"].shape == (3, 3) and kw["record_every"] == 5 and kw["min_fill"] == float(F32(0.4)) and kw["objects"] == [0]
    for bad in ([1, 2], {}, {"points": [[0, 0, 0]], "lattice": {}}, {"point": [[0, 0, 0]]}, {"points": [[0, 0]]},
                {"lattice": {"start": [0, 0, 0], "end": [1, 1, 1]}}, {"points": [[0.3, 0.3, 0.3]], "recordEvery": -1},
                {"points": [[0.3, 0.3, 0.3]], "minFill": 0}):
        with pytest.raises(ValueError, match="tracers"):
            tracers.tracers_config(_config(tracers=bad))


# ---- the VTK writer, read back ----------------------------------------------------------------------------------------------
def test_vtk_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    paths = rng.uniform(0.1, 0.9, size=(4, 5, 3)).astype(np.float32)
    times = [0.001, 0.002, 0.0035, 0.1]
    path = str(tmp_path / "paths.vtk")
    tracers.write_vtk(path, paths, times)
    text = open(path).read()
    assert text.startswith("# vtk DataFile Version 3.0\n") and "\nASCII\nDATASET POLYDATA\nPOINTS 20 float\n" in text
    assert "\nLINES 5 25\n4 0 1 2 3\n4 4 5 6 7\n" in text and "\nPOINT_DATA 20\nSCALARS time double 1\nLOOKUP_TABLE default\n" in text
    got, t = tracers.read_vtk(path)
    assert got.dtype == np.float32 and np.array_equal(got, paths) and np.array_equal(t, np.asarray(times))
    with pytest.raises(ValueError):
        tracers.write_vtk(path, paths, times[:3])
    with pytest.raises(ValueError):
        tracers.write_vtk(path, paths[0], times)
