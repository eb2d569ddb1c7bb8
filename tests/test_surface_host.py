"""Surface frames, host side (no GPU): header / binding of the surface symbols, properties of the NumPy model
(tests/surface_model.py) on analytic inputs, and run_simulation's frameStyle option."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import render_model
import surface_model
from sph_taichi_amd import _lib, render, run_simulation
from test_render_host import AXIS_CAM, RENDER_SYMBOLS, _FakePS, _scene_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE_SYMBOLS = ["sph_surface_set_params", "sph_surface_frame", "sph_surface_download", "sph_surface_download_depth",
                   "sph_surface_download_thickness"]


def _style(radius=0.1, **over):
    return render.resolve_style(render.SurfaceStyle(**over), radius, (50, 100, 200))


# ---- header / binding -------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_surface_abi():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6
    declared = set(re.findall(r"\b(sph_[a-z0-9_A-Z]+)\s*\(", header))
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    for name in SURFACE_SYMBOLS:
        assert name in declared and name in bound, name
    assert {n for n in declared if n.startswith("sph_surface")} == set(SURFACE_SYMBOLS) | {"sph_surface_frame_timed"}
    assert {n for n in declared if n.startswith("sph_render")} == set(RENDER_SYMBOLS)      # the sphere frame's ABI is untouched
    assert declared == set(bound)                                                           # every declaration is bound
    # struct layout, read off the header: every member is 4 bytes wide
    body = re.search(r"typedef struct SphSurfaceParams \{(.*?)\} SphSurfaceParams;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    offset, layout = 0, {}
    for ctype, decl in re.findall(r"\b(int32_t|float)\s+([^;]+);", body):
        for item in decl.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            layout[m.group(1)] = (offset, ctype, int(m.group(2) or 1))
            offset += 4 * int(m.group(2) or 1)
    assert ctypes.sizeof(_lib.SphSurfaceParams) == offset == 56
    assert [n for n, _ in _lib.SphSurfaceParams._fields_] == list(layout)
    for name, (off, ctype, count) in layout.items():
        field = getattr(_lib.SphSurfaceParams, name)
        assert field.offset == off and field.size == 4 * count, name
    assert layout["iterations"][1] == "int32_t" and all(v[1] == "float" for k, v in layout.items() if k != "iterations")
    assert re.search(r"#define SPH_SURFACE_MAX_FILTER_R 16\b", header) and _lib.SURFACE_MAX_FILTER_R == 16
    assert re.search(r"#define SPH_SURFACE_PASSES 6\b", header) and _lib.SURFACE_PASSES == len(_lib.SURFACE_PASS_NAMES) == 6
    assert "sph_surface.hip" in __import__("sph_taichi_amd.build", fromlist=["SOURCES"]).SOURCES
    lib = _lib.load()                                    # builds with the compiler if needed; no device call
    assert lib.sph_abi_version() == 6
    for name in SURFACE_SYMBOLS + ["sph_surface_frame_timed"]:
        assert hasattr(lib, name), name


def test_surface_style_defaults_and_struct():
    s = render.resolve_style(None, 0.01, (50, 100, 200))
    assert s.iterations == 3 and s.filter_radius == pytest.approx(0.03) and s.depth_range == pytest.approx(0.04)
    assert s.fluid_color == pytest.approx((50 / 255, 100 / 255, 200 / 255))
    mine = render.SurfaceStyle(iterations=1, filter_radius=0.5, fluid_color=(0.1, 0.2, 0.3))
    r = render.resolve_style(mine, 0.01, (0, 0, 0))
    assert (r.iterations, r.filter_radius, r.fluid_color) == (1, 0.5, (0.1, 0.2, 0.3)) and r.depth_range == pytest.approx(0.04)
    assert mine.depth_range is None                       # the caller's object is not written
    p = render.surface_params(r)
    assert p.iterations == 1 and p.filter_radius == 0.5 and list(p.fluid_color) == [np.float32(v) for v in (0.1, 0.2, 0.3)]
    assert list(p.absorb) == [18.0, 6.0, 2.0] and p.f0 == np.float32(0.02)
    c = render.surface_style_from_config({"iterations": 5, "filterRadius": 0.05, "absorb": [1, 2, 3], "fluidColor": [0, 0.5, 1]})
    assert c.iterations == 5 and c.filter_radius == 0.05 and c.absorb == (1, 2, 3) and c.fluid_color == (0, 0.5, 1)
    assert render.surface_style_from_config(None) == render.SurfaceStyle()
    with pytest.raises(ValueError, match="unknown key"):
        render.surface_style_from_config({"radius": 1})


# ---- model properties ----------------------------------------------------------------------------------------------------
def test_model_lone_particle_matches_the_sphere_frame():
    """One fluid particle: the unsmoothed fluid depth and its coverage are the sphere frame's depth and coverage."""
    x = np.array([[0.03, -0.02, -2.0]], np.float32)
    col, oid = np.array([[200, 100, 50]]), np.array([0])
    _, depth, win = render_model.render(x, col, oid, AXIS_CAM, (128, 96), 0.1, (1, 1, 1))
    for dtype in (np.float32, np.float64):
        out = surface_model.surface(x, col, oid, np.array([1]), AXIS_CAM, (128, 96), 0.1, (1, 1, 1), _style(), dtype=dtype)
        _, d, w = render_model.render(x, col, oid, AXIS_CAM, (128, 96), 0.1, (1, 1, 1), dtype=dtype)
        assert np.array_equal(np.isfinite(out["z0"]), w == 0) and (w == 0).sum() > 40
        assert np.array_equal(out["z0"], d)
        assert np.array_equal(out["shown"], w == 0) and np.all(np.isinf(out["zo"]))
        assert np.all(out["thickness"][w != 0] == 0) and np.all(out["thickness"][w == 0] > 0)
        assert out["thickness"].max() <= 2 * 0.1 * 1.01                 # at most the sphere's diameter
        assert np.all(out["img"][w != 0] == 0) and out["img"][w == 0].max() > 0
    assert np.array_equal(win == 0, np.isfinite(depth))


def test_model_iterations_zero_is_the_raw_minimum():
    rng = np.random.default_rng(2)
    x = rng.uniform([-0.5, -0.5, -3.0], [0.5, 0.5, -2.0], size=(60, 3)).astype(np.float32)
    col, oid, mat = np.full((60, 3), 99), np.zeros(60, int), np.ones(60, int)
    out = surface_model.surface(x, col, oid, mat, AXIS_CAM, (96, 80), 0.08, (1, 1, 1), _style(0.08, iterations=0))
    _, depth, _ = render_model.render(x, col, oid, AXIS_CAM, (96, 80), 0.08, (1, 1, 1))
    assert np.array_equal(out["zs"], out["z0"]) and np.array_equal(out["z0"], depth) and np.array_equal(out["depth"], depth)
    three = surface_model.surface(x, col, oid, mat, AXIS_CAM, (96, 80), 0.08, (1, 1, 1), _style(0.08, iterations=3))
    assert np.array_equal(np.isfinite(three["zs"]), np.isfinite(out["z0"])) and not np.array_equal(three["zs"], out["z0"])
    assert np.array_equal(three["ts"], out["ts"])                       # the thickness filter reads the raw depth only
    # order independence of the model itself
    perm = rng.permutation(60)
    again = surface_model.surface(x[perm], col, oid, mat, AXIS_CAM, (96, 80), 0.08, (1, 1, 1), _style(0.08, iterations=3))
    for k in ("img", "depth", "thickness"):
        assert np.array_equal(three[k], again[k]), k


def test_model_smoothing_flattens_a_flat_layer():
    """One lattice layer facing the camera: every raw depth lies between the spheres' front plane and their centre plane; the
    smoothed depth, an average of them, stays strictly nearer to the front plane."""
    D, radius = 2.0, 0.05
    g = (np.arange(9) - 4) * (2 * radius)
    gx, gy = np.meshgrid(g, g)
    x = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -D)], axis=1).astype(np.float32)
    n = x.shape[0]
    out = surface_model.surface(x, np.full((n, 3), 80), np.zeros(n, int), np.ones(n, int), AXIS_CAM, (128, 128), radius, (1, 1, 1),
                                _style(radius))
    has = np.isfinite(out["z0"])
    plane = D - radius
    raw = np.abs(out["z0"][has] - plane).max()
    smooth = np.abs(out["zs"][has] - plane).max()
    assert has.sum() > 1000 and out["R"].max() > 3
    assert 0.5 * radius < raw <= radius * 1.001 and smooth < 0.8 * raw
    assert np.abs(out["zs"][has] - plane).mean() < np.abs(out["z0"][has] - plane).mean()


def test_model_solid_in_front_hides_the_fluid():
    x = np.array([[0.0, 0.0, -2.0], [0.0, 0.0, -1.5]], np.float32)        # fluid behind, solid in front, on the axis
    col, oid, mat = np.array([[0, 0, 255], [255, 255, 255]]), np.array([0, 1]), np.array([1, 0])
    out = surface_model.surface(x, col, oid, mat, AXIS_CAM, (96, 96), 0.1, (1, 1, 1), _style())
    oimg, odepth, owin = render_model.render(x[1:], col[1:], oid[1:], AXIS_CAM, (96, 96), 0.1, (1, 1, 1))
    solid = owin == 0
    assert solid.sum() > 80 and np.isfinite(out["z0"][solid]).sum() > 50          # the fluid is there, behind the solid
    assert not out["shown"][solid].any() and np.all(out["thickness"][solid] == 0) and np.all(out["S"][solid] == 0)
    assert np.array_equal(out["img"][solid], oimg[solid]) and np.array_equal(out["depth"][solid], odepth[solid])
    # the other way round the fluid is composited over the solid: with absorb = 0 the solid shows through
    x2 = np.array([[0.0, 0.0, -1.5], [0.0, 0.0, -2.0]], np.float32)
    clear = _style(absorb=(0.0, 0.0, 0.0), specular=0.0, f0=0.0)
    out2 = surface_model.surface(x2, col, oid, mat, AXIS_CAM, (96, 96), 0.1, (1, 1, 1), clear)
    oimg2, _, owin2 = render_model.render(x2[1:], col[1:], oid[1:], AXIS_CAM, (96, 96), 0.1, (1, 1, 1))
    both = out2["shown"] & (owin2 == 0)
    assert both.sum() > 50 and np.all(out2["thickness"][both] > 0)
    centre = both & (np.hypot(*np.meshgrid(np.arange(96) - 47.5, np.arange(96) - 47.5)) < 3)    # facing the eye: Fresnel ~ 0
    assert centre.sum() >= 4 and np.abs(out2["img"][centre].astype(int) - oimg2[centre].astype(int)).max() <= 1
    # hiding the solid object shows the fluid that was behind it
    out3 = surface_model.surface(x, col, oid, mat, AXIS_CAM, (96, 96), 0.1, (1, 1, 1), _style(), invisible=[1])
    assert out3["shown"][48, 48] and out3["thickness"][48, 48] > 0


# ---- run_simulation ------------------------------------------------------------------------------------------------------
def test_parser_accepts_frame_style():
    a = run_simulation.build_parser().parse_args(["--frame_style", "surface"])
    assert a.frame_style == "surface" and run_simulation.build_parser().parse_args([]).frame_style is None
    with pytest.raises(SystemExit):
        run_simulation.build_parser().parse_args(["--frame_style", "mesh"])


def _run(tmp_path, monkeypatch, cfg, argv):
    seen = []

    class PS(_FakePS):
        def render(self, camera=None, invisible_objects=(), size=(1024, 1024)):      # exactly today's signature
            seen.append(("render", tuple(camera.eye), list(invisible_objects), tuple(size), None))
            return np.zeros((size[1], size[0], 3), np.uint8)

        def render_surface(self, camera=None, invisible_objects=(), size=(1024, 1024), style=None):
            seen.append(("render_surface", tuple(camera.eye), list(invisible_objects), tuple(size), style))
            return np.full((size[1], size[0], 3), 7, np.uint8)

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(run_simulation, "ParticleSystem", PS)
    path = _scene_file(tmp_path, exportFrame=True, invisibleObjects=[3], timeStepSize=0.0004, **cfg)
    run_simulation.main(["--scene_file", path, "--frames", "41", "--image_size", "48", "32", "--camera", "1", "2", "3", "0", "0.5", "0"] + argv)
    assert sorted(os.listdir(tmp_path / "tiny_output_img")) == ["000000.png", "000040.png"]
    return seen


def test_frame_style_surface_reaches_render_surface(tmp_path, monkeypatch, capsys):
    seen = _run(tmp_path, monkeypatch, dict(frameStyle="surface", surfaceStyle={"iterations": 2, "absorb": [1, 2, 3]}), [])
    want = render.SurfaceStyle(iterations=2, absorb=(1, 2, 3))
    assert seen == [("render_surface", (1.0, 2.0, 3.0), [3], (48, 32), want)] * 2
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["frames_written"] == 2
    # the command line chooses it too, with the default style; and it overrides the scene file
    seen = _run(tmp_path, monkeypatch, {}, ["--frame_style", "surface"])
    assert seen == [("render_surface", (1.0, 2.0, 3.0), [3], (48, 32), render.SurfaceStyle())] * 2
    seen = _run(tmp_path, monkeypatch, dict(frameStyle="surface"), ["--frame_style", "spheres"])
    assert [s[0] for s in seen] == ["render", "render"]
    with pytest.raises(ValueError, match="frameStyle"):
        _run(tmp_path, monkeypatch, dict(frameStyle="mesh"), [])


def test_default_frame_style_calls_render_as_before(tmp_path, monkeypatch):
    for cfg in ({}, dict(frameStyle="spheres"), dict(surfaceStyle={"iterations": 1})):
        seen = _run(tmp_path, monkeypatch, cfg, [])
        assert seen == [("render", (1.0, 2.0, 3.0), [3], (48, 32), None)] * 2      # (a fourth keyword would have raised TypeError)
