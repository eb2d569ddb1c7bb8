"""Frame export, host side (no GPU): the PNG writer, the camera and its view basis, the NumPy model of the renderer on
analytic inputs, run_simulation's options, and the header / binding of the five render symbols."""
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest

import render_model
import scenes
from sph_taichi_amd import _lib, render, run_simulation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def decode_png(path):
    """8-bit RGB, non-interlaced, filter 0 on every row: what write_png promises.  Checks signature, chunk CRCs, IHDR."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        chunks.append((tag, data))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, flt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT")), dtype=np.uint8)
    rows = rows.reshape(h, 1 + 3 * w)
    assert np.all(rows[:, 0] == 0)
    return rows[:, 1:].reshape(h, w, 3)


@pytest.mark.parametrize("shape", [(1, 1), (7, 13), (64, 64), (33, 2)])
def test_write_png_roundtrip(tmp_path, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    a = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    render.write_png(path, a)
    assert np.array_equal(decode_png(path), a)
    render.write_png(path, a[:, ::-1])                 # a non-contiguous view
    assert np.array_equal(decode_png(path), a[:, ::-1])
    with pytest.raises(ValueError):
        render.write_png(path, a.astype(np.float32))


def test_camera_defaults_are_the_reference_window():
    """run_simulation.py:37-45, 90, 93 of the reference: 1024 x 1024 window, camera.position(5.5, 2.5, 4.0), up(0, 1, 0),
    lookat(-1, 0, 0), fov(70), point light (2, 2, 2), line colour (0.99, 0.68, 0.28), background (0, 0, 0)."""
    c = render.Camera()
    assert tuple(c.eye) == (5.5, 2.5, 4.0) and tuple(c.lookat) == (-1.0, 0.0, 0.0) and tuple(c.up) == (0.0, 1.0, 0.0)
    assert c.fov_y_deg == 70.0 and tuple(c.light) == (2.0, 2.0, 2.0) and tuple(c.box_color) == (0.99, 0.68, 0.28)
    assert tuple(c.background) == (0, 0, 0) and c.draw_box
    args = run_simulation.build_parser().parse_args([])
    assert args.image_size == [1024, 1024] and args.camera is None


@pytest.mark.parametrize("cam", [render.Camera(), render.Camera(eye=(0.3, 0.9, -2.0), lookat=(0.5, 0.2, 0.4), up=(0.1, 1.0, 0.0))])
def test_view_basis_is_orthonormal_and_looks_at_lookat(cam):
    r, u, f, focal = render.view_basis(cam, 1024)
    assert all(v.dtype == np.float32 for v in (r, u, f)) and focal.dtype == np.float32
    M = np.stack([r, u, -f]).astype(np.float64)                   # rows: right, up, -forward (view space looks down -z)
    assert np.allclose(M @ M.T, np.eye(3), atol=3e-7)
    assert np.linalg.det(M) > 0.999                               # right-handed
    v = M @ (np.array(cam.lookat, dtype=np.float64) - np.array(cam.eye, dtype=np.float64))
    assert abs(v[0]) < 1e-5 and abs(v[1]) < 1e-5 and v[2] < 0      # lookat lies on the -z axis
    assert np.dot(u.astype(np.float64), np.array(cam.up)) > 0
    assert np.isclose(float(focal), 512.0 / np.tan(np.deg2rad(cam.fov_y_deg) / 2), rtol=1e-6)


def test_view_basis_rejects_degenerate_cameras():
    with pytest.raises(ValueError):
        render.view_basis(render.Camera(eye=(1, 2, 3), lookat=(1, 2, 3)), 64)
    with pytest.raises(ValueError):
        render.view_basis(render.Camera(eye=(0, 0, 0), lookat=(0, 2, 0), up=(0, 1, 0)), 64)
    with pytest.raises(ValueError):
        render.view_basis(render.Camera(fov_y_deg=0.0), 64)


AXIS_CAM = render.Camera(eye=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov_y_deg=60.0, draw_box=False,
                         light=(0.5, 1.0, 1.0))


def test_model_single_particle_covers_its_disc():
    """One particle on the optical axis at distance D: exactly the pixels whose centre is within focal * radius / D of the
    image centre (numbers chosen so that no pixel centre is within 1e-3 px of the rim)."""
    W = H = 128
    D, radius = 2.0, 0.1
    img, depth, win = render_model.render(np.array([[0.0, 0.0, -D]], np.float32), np.array([[200, 100, 50]]), np.array([0]),
                                          AXIS_CAM, (W, H), radius, (1, 1, 1))
    focal = (H / 2) / np.tan(np.deg2rad(60.0) / 2)
    R = focal * radius / D
    jj, ii = np.mgrid[0:H, 0:W]
    dist = np.hypot(ii + 0.5 - W / 2, jj + 0.5 - H / 2)
    assert np.min(np.abs(dist - R)) > 1e-3
    assert np.array_equal(win == 0, dist < R) and (dist < R).sum() > 80
    assert np.all(np.isinf(depth[win != 0])) and np.all(img[win != 0] == 0)
    # the nearest surface point is the one on the axis (no pixel centre is exactly there: the four around it)
    assert abs(depth.min() - (D - radius)) < 2e-3 and np.all(depth[win == 0] < D)
    assert img[win == 0].max() > 0


def test_model_nearer_particle_wins_whatever_the_order():
    x = np.array([[0.0, 0.0, -2.0], [0.0, 0.0, -3.0]], np.float32)
    col = np.array([[255, 0, 0], [0, 0, 255]])
    a = render_model.render(x, col, np.array([0, 1]), AXIS_CAM, (64, 64), 0.1, (1, 1, 1))
    b = render_model.render(x[::-1], col[::-1], np.array([1, 0]), AXIS_CAM, (64, 64), 0.1, (1, 1, 1))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    centre = a[0][32, 32]
    assert centre[0] > 0 and centre[2] == 0                          # the red one, which is nearer
    assert np.all(a[2][a[2] >= 0] == 0) and np.all(b[2][b[2] >= 0] == 1)   # the far one is entirely hidden
    # hiding the near object shows the far one
    c = render_model.render(x, col, np.array([0, 1]), AXIS_CAM, (64, 64), 0.1, (1, 1, 1), invisible=[0])
    assert c[0][32, 32][2] > 0 and c[0][32, 32][0] == 0


def test_model_is_order_independent_and_culls():
    rng = np.random.default_rng(5)
    n = 400
    x = rng.uniform([-0.6, -0.6, -3.0], [0.6, 0.6, 1.0], size=(n, 3)).astype(np.float32)   # some behind the camera
    col = rng.integers(0, 256, size=(n, 3))
    oid = rng.integers(0, 3, size=n)
    cam = render.Camera(eye=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, -1.0), fov_y_deg=60.0, near_plane=0.2, draw_box=True)
    a = render_model.render(x, col, oid, cam, (96, 80), 0.05, (0.5, 0.5, 0.5))
    perm = rng.permutation(n)
    b = render_model.render(x[perm], col[perm], oid[perm], cam, (96, 80), 0.05, (0.5, 0.5, 0.5))
    assert a[0].shape == (80, 96, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(perm[b[2][b[2] >= 0]], a[2][a[2] >= 0])
    shown = np.unique(a[2][a[2] >= 0])
    assert len(shown) > 20 and np.all(-x[shown, 2] >= 0.2)           # nothing inside the near plane or behind the eye
    # a particle at the eye, and one far outside the view, change nothing
    x2 = np.concatenate([x, np.array([[0, 0, 0], [50.0, 0, -1.0], [np.inf, 0, -1], [np.nan, 0, 0]], np.float32)])
    c = render_model.render(x2, np.concatenate([col, np.full((4, 3), 255)]), np.concatenate([oid, [0] * 4]), cam, (96, 80),
                            0.05, (0.5, 0.5, 0.5))
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_model_box_only():
    cam = render.Camera()
    img, depth, win = render_model.render(np.zeros((0, 3), np.float32), np.zeros((0, 3), int), np.zeros(0, int), cam,
                                          (128, 128), 0.01, (5.0, 3.0, 2.0))
    assert set(np.unique(win)) == {-2, -1} and 100 < (win == -2).sum() < 128 * 128 // 8
    assert np.all(img[win == -2] == (252, 173, 71)) and np.all(img[win == -1] == 0)     # round(255 * (0.99, 0.68, 0.28))
    assert np.all(np.isfinite(depth[win == -2])) and np.all(np.isinf(depth[win == -1]))


# ---- run_simulation ---------------------------------------------------------------------------------------------------
def test_parser_accepts_the_frame_options():
    a = run_simulation.build_parser().parse_args(["--scene_file", "x.json", "--image_size", "320", "200", "--camera", "1", "2", "3",
                                                  "0.5", "0.25", "0"])
    assert a.image_size == [320, 200] and a.camera == [1.0, 2.0, 3.0, 0.5, 0.25, 0.0]
    with pytest.raises(SystemExit):
        run_simulation.build_parser().parse_args(["--image_size", "320"])


class _FakeSolver:
    def __init__(self, ps):
        self.ps = ps

    def initialize(self):
        pass

    def step(self, n=1):
        self.ps.steps += n


class _FakePS:
    """A ParticleSystem whose library binding raises on every render symbol (and does nothing otherwise); `render` is the
    real method, so a frame request reaches the binding."""
    from sph_taichi_amd.particle_system import ParticleSystem as _PS
    render = _PS.render
    calls = []

    def __init__(self, config, **kw):
        self.particle_max_num, self.steps = 8, 0
        self.particle_radius, self.domain_end = 0.01, np.array([1.0, 1.2, 0.8])

    def _call(self, name, *args):
        _FakePS.calls.append(name)
        if name.startswith("sph_render"):
            raise RuntimeError(f"render symbol {name} called")

    def build_solver(self):
        return _FakeSolver(self)

    def sync(self):
        pass

    def close(self):
        pass


def _scene_file(tmp_path, **cfg):
    sd = scenes.fluid_only(counts=(2, 2, 2))
    sd["Configuration"].update(cfg)
    p = tmp_path / "tiny.json"
    p.write_text(json.dumps(sd))
    return str(p)


def test_export_frame_false_calls_no_render_symbol(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(run_simulation, "ParticleSystem", _FakePS)
    _FakePS.calls = []
    run_simulation.main(["--scene_file", _scene_file(tmp_path), "--frames", "45"])
    assert not any(n.startswith("sph_render") for n in _FakePS.calls)
    assert not os.path.exists(tmp_path / "tiny_output_img")
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["steps"] == 45 and "frames_written" not in report and "render_ms_per_frame" not in report
    # ... and with exportFrame true the first frame goes to the binding (which raises here), after the directory was made
    with pytest.raises(RuntimeError, match="render symbol sph_render_set_params called"):
        run_simulation.main(["--scene_file", _scene_file(tmp_path, exportFrame=True), "--frames", "45"])
    assert os.path.isdir(tmp_path / "tiny_output_img")


def test_export_frame_names_and_interval(tmp_path, monkeypatch, capsys):
    """One PNG when cnt % int(0.016 / timeStepSize) == 0, named {cnt:06}.png under {scene}_output_img (run_simulation.py:23,
    27-28, 96-98 of the reference); invisibleObjects, --image_size and --camera reach the render call."""
    seen = []

    class PS(_FakePS):
        def render(self, camera=None, invisible_objects=(), size=(1024, 1024)):
            seen.append((tuple(camera.eye), tuple(camera.lookat), list(invisible_objects), tuple(size)))
            img = np.zeros((size[1], size[0], 3), np.uint8)
            img[: 1 + len(seen)] = 200
            return img

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(run_simulation, "ParticleSystem", PS)
    path = _scene_file(tmp_path, exportFrame=True, invisibleObjects=[3], timeStepSize=0.0004, numberOfStepsPerRenderUpdate=2)
    run_simulation.main(["--scene_file", path, "--frames", "81", "--image_size", "48", "32", "--camera", "1", "2", "3", "0", "0.5", "0"])
    assert sorted(os.listdir(tmp_path / "tiny_output_img")) == ["000000.png", "000040.png", "000080.png"]
    assert seen == [((1.0, 2.0, 3.0), (0.0, 0.5, 0.0), [3], (48, 32))] * 3
    img = decode_png(str(tmp_path / "tiny_output_img" / "000040.png"))
    assert img.shape == (32, 48, 3) and np.all(img[:3] == 200) and np.all(img[3:] == 0)
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["frames_written"] == 3 and report["render_ms_per_frame"] >= 0 and report["steps"] == 162


# ---- header / binding -------------------------------------------------------------------------------------------------
RENDER_SYMBOLS = ["sph_render_set_params", "sph_render_set_invisible", "sph_render_frame", "sph_render_download",
                  "sph_render_download_depth"]


def test_header_and_binding_carry_the_render_abi():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6
    declared = set(re.findall(r"\b(sph_[a-z0-9_A-Z]+)\s*\(", header))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in RENDER_SYMBOLS:
        assert name in declared and name in bound, name
    assert {n for n in declared if n.startswith("sph_render")} == set(RENDER_SYMBOLS)
    # struct layout: 2 i32, 3 x 3 f32, 3 f32, 3 f32, 1 f32, 4 u8, 2 x 3 f32
    import ctypes
    assert ctypes.sizeof(_lib.SphRenderParams) == 4 * (2 + 9 + 3 + 3 + 1 + 1 + 6)
    assert _lib.SphRenderParams.background.offset == 4 * 18 and _lib.SphRenderParams.box_end.offset == 4 * 19
    lib = _lib.load()                                    # builds with the compiler if needed; no device call
    assert lib.sph_abi_version() == 6
    for name in RENDER_SYMBOLS:
        assert hasattr(lib, name), name
    assert "sph_render.hip" in __import__("sph_taichi_amd.build", fromlist=["SOURCES"]).SOURCES


def test_render_params_struct_from_camera():
    p = render.render_params(render.Camera(), (640, 480), 0.01, (5.0, 3.0, 2.0))
    assert (p.width, p.height) == (640, 480) and list(p.eye) == [5.5, 2.5, 4.0] and list(p.lookat) == [-1.0, 0.0, 0.0]
    assert p.fov_y_deg == 70.0 and p.radius == np.float32(0.01) and list(p.box_end) == [5.0, 3.0, 2.0]
    assert list(p.background) == [0, 0, 0] and p.draw_box == 1 and np.allclose(list(p.box_color), [0.99, 0.68, 0.28])
