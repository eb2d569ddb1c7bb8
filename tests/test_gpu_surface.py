"""Surface frames on the GPU: the device passes (csrc/sph_surface.hip) against the NumPy model of their specification
(tests/surface_model.py), the perturbation condition, order independence, that a frame only reads, semantics, errors, and
run_simulation end to end.

Parity figures (recording run on an MI355X, profiles/surface_parity.json; fluid pixels shown 412 / 6,998 / 91 / 27,195 / 25 on
the five cases, fluid sprite radii 0.76-0.86 px from the far camera at 256 x 256 and 4.5-14.7 px from the close one, filter
radii 1 / 8-16 / 2 / 16 / 1-2): on every case the device image, depth and thickness equal the float32 model BIT FOR BIT -- 0 pixels
of different coverage, 0 differing depth values, 0 differing thickness values, 0 differing channel values.  Nothing rounds
differently, so the bounds below are 0 (3 x 0).  The same file holds the float32-against-float64 figures of the MODEL on the same
states (the perturbation condition): 0 pixels of different coverage, at most 1 pixel (of 27,195) more than one channel level
apart, relative depth differences up to 4e-6 -- inside the cap of 0.1 % / 1 % of the fluid pixels."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import scenes
import surface_model
from sph_taichi_amd import _lib, render
from test_gpu_render import CLOSE, FAR

pytestmark = pytest.mark.gpu

# scene, view, camera, size, filter radius in particle radii (None: the default of 3)
CASES = [("fluid_block", "far", FAR, (256, 256), 1.0), ("fluid_block", "close", CLOSE, (250, 130), None),
         ("coupled", "far", FAR, (250, 130), None), ("coupled", "close", CLOSE, (256, 256), None),
         ("coupled", "close", CLOSE, (8, 8), None)]
# GPU against the float32 model, per case: 3 x the recording run's figure (profiles/surface_parity.json), which is 0 everywhere
BOUND_COVERAGE = BOUND_DEPTH_VALUES = BOUND_THICKNESS_VALUES = BOUND_CHANNEL_PIXELS = BOUND_CHANNEL_LEVELS = 0
_RECORD = {}


def _scene(name):
    return scenes.fluid_only() if name == "fluid_block" else scenes.fluid_with_rigid_blocks()


def _style(ps, filter_radii=None, **over):
    if filter_radii is not None:
        over["filter_radius"] = filter_radii * ps.particle_radius
    return render.SurfaceStyle(**over)


def _model(ps, cam, size, style=None, invisible=(), dtype=np.float32, keep=None):
    x, col, oid, mat = ps.x.to_numpy(), ps.color.to_numpy(), ps.object_id.to_numpy(), ps.material.to_numpy()
    if keep is not None:
        x, col, oid, mat = x[keep], col[keep], oid[keep], mat[keep]
    resolved = render.resolve_style(style, ps.particle_radius, ps._first_fluid_colour())
    return surface_model.surface(x, col, oid, mat, cam, size, ps.particle_radius, ps.domain_end, resolved, invisible, dtype)


def _frame(ps, cam, size, style=None, invisible=()):
    img = ps.render_surface(cam, invisible_objects=invisible, size=size, style=style)
    return img, ps.render_surface_depth(), ps.render_surface_thickness()


def _same(got, m):
    return np.array_equal(got[0], m["img"]) and np.array_equal(got[1], m["depth"]) and np.array_equal(got[2], m["thickness"])


def _compare(img, depth, thick, shown, m):
    """`shown`: where the first picture shows fluid."""
    both = shown & m["shown"]
    d64, t64 = m["depth"].astype(np.float64), m["thickness"].astype(np.float64)
    rel = np.abs(depth[both].astype(np.float64) - d64[both]) / d64[both]
    chan = np.abs(img.astype(int) - m["img"].astype(int)).max(axis=-1)
    return {"fluid_pixels": int(m["shown"].sum()), "coverage_differs": int((shown != m["shown"]).sum()),
            "depth_values_differ": int((depth.astype(np.float64) != d64).sum()),
            "thickness_values_differ": int((thick.astype(np.float64) != t64).sum()),
            "max_rel_depth_diff": float(rel.max()) if both.any() else 0.0,
            "max_abs_thickness_diff": float(np.abs(thick[both].astype(np.float64) - t64[both]).max()) if both.any() else 0.0,
            "channel_pixels_differ": int((chan > 0).sum()), "pixels_more_than_one_level": int((chan[both] > 1).sum()),
            "max_channel_diff": int(chan.max())}


@pytest.mark.parametrize("scene,view,cam,size,filter_radii", CASES)
def test_model_parity(scene, view, cam, size, filter_radii):
    ps, solver = scenes.make_ps(_scene(scene))
    solver.initialize()
    solver.step(5)
    style = _style(ps, filter_radii)
    img, depth, thick = _frame(ps, cam, size, style)
    assert img.shape == (size[1], size[0], 3) and img.dtype == np.uint8 and depth.shape == thick.shape == (size[1], size[0])
    m = _model(ps, cam, size, style)
    # (the device shows fluid where its depth lies in front of the opaque layer, whose depth test_gpu_render pins bit for bit)
    got = _compare(img, depth, thick, np.isfinite(depth) & (depth < m["zo"]), m)
    # the perturbation condition on the same state: the model in float32 against the model in float64
    d = _model(ps, cam, size, style, dtype=np.float64)
    pert = _compare(m["img"], m["depth"], m["thickness"], m["shown"], d)
    fluid_R = m["R"][m["R"] > 0]
    _RECORD[f"{scene} / {view} {size[0]}x{size[1]}"] = {
        "camera": {"eye": list(cam.eye), "lookat": list(cam.lookat), "near_plane": cam.near_plane},
        "particles": int(ps.particle_max_num), "fluid_sprite_radius_px": list(m["sprite_radius_px"]),
        "filter_radius_px": [int(fluid_R.min()), int(fluid_R.max())], "gpu_vs_model_f32": got, "model_f32_vs_model_f64": pert}
    out = scenes.evidence_path("surface_parity.json")
    if out:
        json.dump(_RECORD, open(out, "w"), indent=1, sort_keys=True)
    print(scene, view, size, got, pert)
    nf = got["fluid_pixels"]
    assert nf > (20 if size == (8, 8) else 80) and np.all(m["thickness"][~m["shown"]] == 0)
    if size == (256, 256) and view == "far":
        assert m["sprite_radius_px"][1] < 1.0 and fluid_R.max() == 1                # sprites below a pixel, filter radius 1
    if size == (256, 256) and view == "close":
        assert m["sprite_radius_px"][1] > 10.0                                       # the wave-per-particle path is in the picture
        assert fluid_R.max() == surface_model.MAX_FILTER_R                           # ... and the filter radius at its clamp
    if size == (250, 130) and view == "close":
        assert fluid_R.min() < fluid_R.max()                                         # a radius that varies over the picture
    # the perturbation stays inside the cap (else the camera is wrong for this check, not the cap)
    assert pert["coverage_differs"] <= 1e-3 * nf and pert["pixels_more_than_one_level"] <= 1e-2 * nf
    if os.environ.get("SPH_TEST_RECORD_ONLY") != "1":
        assert got["coverage_differs"] <= BOUND_COVERAGE and got["depth_values_differ"] <= BOUND_DEPTH_VALUES
        assert got["thickness_values_differ"] <= BOUND_THICKNESS_VALUES
        assert got["channel_pixels_differ"] <= BOUND_CHANNEL_PIXELS and got["max_channel_diff"] <= BOUND_CHANNEL_LEVELS
    ps.close()


def test_no_fluid_in_the_picture_is_the_sphere_frame():
    ps, solver = scenes.make_ps(scenes.fluid_with_rigid_blocks())
    solver.initialize()
    solver.step(5)
    for cam, size in ((FAR, (250, 130)), (CLOSE, (256, 256))):
        img, depth, thick = _frame(ps, cam, size, invisible=[0])
        assert np.array_equal(img, ps.render(cam, invisible_objects=[0], size=size)) and np.array_equal(depth, ps.render_depth())
        assert np.all(thick == 0) and np.isfinite(depth).sum() > 200
    ps.close()


def test_the_two_styles_keep_their_own_results():
    """The two styles run the same splat kernels with their own planes, counters and sizes: a frame of one style leaves the
    other's last image and planes downloadable and unchanged, and changes nothing in what the other renders next.  FAR at
    64 x 48 uses the lane-per-sprite path only, CLOSE at 250 x 130 both paths (sprite radii on both sides of the threshold)."""
    import render_model
    ps, solver = scenes.make_ps(scenes.fluid_with_rigid_blocks())
    solver.initialize()
    solver.step(5)
    small, large = (64, 48), (250, 130)
    spheres, sphere_depth = ps.render(FAR, size=small), ps.render_depth()
    surface = _frame(ps, CLOSE, large)
    assert sphere_depth.shape == (48, 64) and surface[1].shape == (130, 250)
    assert np.array_equal(ps.render_depth().view(np.uint32), sphere_depth.view(np.uint32))      # the sphere frame's, not the surface's
    assert np.array_equal(ps.render(FAR, size=small), spheres) and np.array_equal(ps.render_depth().view(np.uint32), sphere_depth.view(np.uint32))
    again = (ps.render_surface_depth(), ps.render_surface_thickness())
    buf = np.empty((130, 250, 3), np.uint8)
    ps._call("sph_surface_download", buf.ctypes.data_as(C.c_void_p), buf.nbytes)
    assert np.array_equal(buf, surface[0])
    assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(again, surface[1:]))
    # both against their models, bound 0
    m = _model(ps, CLOSE, large)
    assert _same(surface, m) and m["shown"].sum() > 80
    x, col, oid = ps.x.to_numpy(), ps.color.to_numpy(), ps.object_id.to_numpy()
    mimg, mdepth, _ = render_model.render(x, col, oid, FAR, small, ps.particle_radius, ps.domain_end, (), np.float32)
    assert np.array_equal(spheres, mimg) and np.array_equal(sphere_depth, mdepth.astype(np.float32)) and np.isfinite(mdepth).sum() > 80
    radii = [s[5] for s in (render_model.sprite(render_model.Setup(CLOSE, large, ps.particle_radius, ps.domain_end), p) for p in x) if s]
    assert min(radii) < 4.0 < max(radii)                      # SPH_RENDER_SMALL_R: both splat paths were in the surface frame
    ps.close()


def test_order_independence_and_reproducibility():
    sd = scenes.fluid_with_rigid_blocks()
    cfg, sc = scenes.build(sd)
    scenes.jitter(sc, 0.2, seed=3)
    perm = np.random.default_rng(11).permutation(sc.arrays["x"].shape[0])
    shuffled = {k: v[perm].copy() for k, v in sc.arrays.items() if k != "pid"}
    out = []
    for arrays in (sc.arrays, shuffled):
        ps, solver = scenes.make_ps(sd, arrays)
        solver.initialize()                                # sorts; positions are the uploaded ones
        for cam, size in ((FAR, (250, 130)), (CLOSE, (256, 256))):
            a = _frame(ps, cam, size)
            b = _frame(ps, cam, size)                      # the same context twice
            assert all(np.array_equal(p, q) for p, q in zip(a, b))
            out.append(a)
        ps.close()
    assert (out[0][2] > 0).sum() > 50 and (out[1][2] > 0).sum() > 500
    for k in (0, 1):
        assert all(np.array_equal(p, q) for p, q in zip(out[k], out[k + 2]))


def test_surface_frames_only_read():
    sd = scenes.fluid_with_rigid_blocks()
    runs = []
    for with_frames in (False, True):
        ps, solver = scenes.make_ps(sd)
        solver.initialize()
        for _ in range(8):
            solver.step(1)
            if with_frames:
                ps.render_surface(FAR, size=(128, 128))
                ps.render_surface(CLOSE, size=(200, 100), invisible_objects=[1])
        st = _lib.SphStats()
        ps._call("sph_get_stats", C.byref(st))
        fields = {f: getattr(ps, f).to_numpy() for f in ps._STATE_FIELDS}
        fields["grid_ids"] = ps.grid_ids.to_numpy()
        runs.append((fields, bytes(st)))
        ps.close()
    for f in runs[0][0]:
        assert np.array_equal(runs[0][0][f], runs[1][0][f]), f
    assert runs[0][1] == runs[1][1]


def test_semantics():
    sd = scenes.fluid_with_rigid_blocks()
    cfg, sc = scenes.build(sd)
    arrays = {k: v.copy() for k, v in sc.arrays.items()}
    cam = render.Camera(eye=(0.5, 0.5, 0.7), lookat=(0.2, 0.2, 0.2), near_plane=0.1)
    f = np.array(cam.lookat) - np.array(cam.eye)
    f /= np.linalg.norm(f)
    eye = np.array(cam.eye)
    # particles 0..4 of the fluid: at the eye, just inside the near plane, just outside it, behind the camera, far off screen
    assert np.all(arrays["material"][:5] == 1)
    arrays["x"][0] = eye
    arrays["x"][1] = eye + 0.099 * f
    arrays["x"][2] = eye + 0.101 * f
    arrays["x"][3] = eye - 0.3 * f
    arrays["x"][4] = eye + 0.2 * f + np.array([30.0, 0.0, 0.0])
    ps, solver = scenes.make_ps(sd, arrays)
    size = (192, 160)
    got = _frame(ps, cam, size)
    assert _same(got, _model(ps, cam, size))
    drawn = np.ones(arrays["x"].shape[0], bool)
    drawn[[0, 1, 3, 4]] = False                          # the picture without the four culled particles is the same picture
    assert _same(got, _model(ps, cam, size, keep=drawn))
    drawn[2] = False                                      # ... but the one just outside the near plane is in it
    assert not np.array_equal(got[2], _model(ps, cam, size, keep=drawn)["thickness"])
    # iterations = 0: the raw surface
    raw = _style(ps, iterations=0)
    got0 = _frame(ps, cam, size, raw)
    m0 = _model(ps, cam, size, raw)
    assert _same(got0, m0) and np.array_equal(got0[1][m0["shown"]], m0["z0"][m0["shown"]]) and not np.array_equal(got0[1], got[1])
    # from below, the fluid lies BEHIND the static slab (object 1): there it gives neither colour nor thickness
    below = render.Camera(eye=(0.22, -0.6, 0.2), lookat=(0.22, 0.2, 0.2), up=(0.0, 0.0, 1.0))
    gb = _frame(ps, below, size)
    mb = _model(ps, below, size)
    hidden = np.isfinite(mb["z0"]) & (mb["zo"] < mb["z0"]) & ~mb["shown"]
    solids = ps.render(below, invisible_objects=[0], size=size)
    assert _same(gb, mb) and hidden.sum() > 300
    assert np.all(gb[2][hidden] == 0) and np.array_equal(gb[0][hidden], solids[hidden]) and np.array_equal(gb[1][hidden], mb["zo"][hidden])
    # from above it lies IN FRONT of the slab and is composited over it; without absorption the slab shows through
    above = render.Camera(eye=(0.22, 1.0, 0.21), lookat=(0.22, 0.0, 0.2), up=(0.0, 0.0, 1.0))
    clear = _style(ps, absorb=(0.0, 0.0, 0.0))
    ga, gc = _frame(ps, above, size), _frame(ps, above, size, clear)
    ma, mc = _model(ps, above, size), _model(ps, above, size, clear)
    assert _same(ga, ma) and _same(gc, mc)
    solids = ps.render(above, invisible_objects=[0], size=size).astype(int)
    over = ma["shown"] & np.isfinite(ma["zo"])                                                   # fluid shown over the slab
    assert over.sum() > 300 and np.all(ga[2][over] > 0) and np.array_equal(ga[2], gc[2])
    assert np.abs(gc[0].astype(int) - solids)[over].mean() < 0.5 * np.abs(ga[0].astype(int) - solids)[over].mean()
    ps.close()


def _sp(ps, **over):
    style = render.resolve_style(None, ps.particle_radius, (50, 100, 200))
    sp = render.surface_params(style)
    for k, v in over.items():
        setattr(sp, k, (C.c_float * 3)(*v) if isinstance(v, tuple) else v)
    return ps._lib.sph_surface_set_params(ps._ctx, C.byref(sp))


def test_errors():
    from sph_taichi_amd import ParticleSystem
    from sph_taichi_amd.config_builder import SimConfig
    sd = scenes.fluid_only()
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    E_INVALID, E_STATE = -1, -4
    lib, ctx = ps._lib, ps._ctx
    buf = np.zeros(64 * 48 * 3, np.uint8)
    plane = np.zeros(64 * 48, np.float32)
    assert lib.sph_surface_frame(ctx) == E_STATE                                 # nothing set yet
    assert _sp(ps) == 0
    assert lib.sph_surface_frame(ctx) == E_STATE                                 # the style alone: still no camera
    assert lib.sph_surface_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == E_STATE     # no frame yet
    assert lib.sph_surface_download_depth(ctx, plane.ctypes.data_as(C.c_void_p), plane.nbytes) == E_STATE
    rp = render.render_params(FAR, (64, 48), ps.particle_radius, ps.domain_end)
    assert lib.sph_render_set_params(ctx, C.byref(rp)) == 0
    nan, inf = float("nan"), float("inf")
    bad = [dict(iterations=-1), dict(iterations=9), dict(filter_radius=0.0), dict(filter_radius=-1.0), dict(filter_radius=nan),
           dict(filter_radius=inf), dict(depth_range=0.0), dict(depth_range=-0.5), dict(depth_range=nan), dict(depth_range=inf),
           dict(fluid_color=(0.5, 1.5, 0.5)), dict(fluid_color=(-0.1, 0.5, 0.5)), dict(fluid_color=(0.5, 0.5, nan)),
           dict(absorb=(-1.0, 0.0, 0.0)), dict(absorb=(0.0, inf, 0.0)), dict(absorb=(0.0, 0.0, nan)),
           dict(sky=(2.0, 0.0, 0.0)), dict(sky=(0.0, -1.0, 0.0)), dict(sky=(0.0, 0.0, nan)),
           dict(f0=-0.1), dict(f0=1.1), dict(f0=nan), dict(specular=-1.0), dict(specular=nan), dict(specular=inf)]
    for over in bad:
        assert _sp(ps, **over) == E_INVALID, over
        assert b"sph_surface_set_params" in lib.sph_last_error(ctx)
    assert lib.sph_surface_set_params(ctx, None) == E_INVALID
    # the last good parameters are still in force: the context renders ...
    assert lib.sph_surface_frame(ctx) == 0
    assert lib.sph_surface_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 1) == E_INVALID
    assert lib.sph_surface_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes + 1) == E_INVALID
    assert lib.sph_surface_download_depth(ctx, plane.ctypes.data_as(C.c_void_p), plane.nbytes + 4) == E_INVALID
    assert lib.sph_surface_download_thickness(ctx, plane.ctypes.data_as(C.c_void_p), plane.nbytes - 4) == E_INVALID
    assert lib.sph_surface_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
    assert lib.sph_surface_download_thickness(ctx, plane.ctypes.data_as(C.c_void_p), plane.nbytes) == 0
    m = _model(ps, FAR, (64, 48))
    assert np.array_equal(buf.reshape(48, 64, 3), m["img"]) and np.array_equal(plane.reshape(48, 64), m["thickness"])
    ms = (C.c_float * _lib.SURFACE_PASSES)()
    assert lib.sph_surface_frame_timed(ctx, ms, _lib.SURFACE_PASSES - 1) == E_INVALID
    assert lib.sph_surface_frame_timed(ctx, ms, _lib.SURFACE_PASSES) == 0 and all(v >= 0 for v in ms)
    with pytest.raises(_lib.SphError, match="rc=-1"):
        ps.render_surface(FAR, size=(64, 48), style=render.SurfaceStyle(iterations=12))
    # ... and steps
    solver.step(3)
    assert _same(_frame(ps, FAR, (96, 96)), _model(ps, FAR, (96, 96)))
    assert np.array_equal(ps.render(FAR, size=(96, 96)), ps.render(FAR, size=(96, 96)))
    ps.close()
    # a slab rank: compositing across GPUs is not built
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    assert _sp(slab) == E_STATE and slab._lib.sph_surface_frame(slab._ctx) == E_STATE
    with pytest.raises(_lib.SphError, match="rc=-4"):
        slab.render_surface()
    assert slab.count() == 960
    slab.close()


def test_run_simulation_writes_surface_frames(tmp_path, monkeypatch, capsys):
    from test_render_host import decode_png
    from sph_taichi_amd import run_simulation
    names = ("000000.png", "000040.png")
    frames = {}
    for style in ("surface", "spheres"):
        sd = scenes.fluid_with_rigid_blocks()
        sd["Configuration"].update(exportFrame=True, frameStyle=style, surfaceStyle={"iterations": 2})
        d = tmp_path / style / "data" / "scenes"
        d.mkdir(parents=True)
        (d / "coupled.json").write_text(json.dumps(sd))
        monkeypatch.chdir(tmp_path / style)
        run_simulation.main(["--scene_file", str(d / "coupled.json"), "--frames", "80", "--image_size", "160", "120",
                             "--camera", "1.7", "1.1", "1.6", "0.25", "0.2", "0.2"])
        assert sorted(os.listdir(tmp_path / style / "coupled_output_img")) == list(names)
        frames[style] = [decode_png(str(tmp_path / style / "coupled_output_img" / n)) for n in names]
        report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert report["frames_written"] == 2 and report["render_ms_per_frame"] > 0 and report["steps"] == 80
    for img in frames["surface"]:
        assert img.shape == (120, 160, 3) and len(np.unique(img.reshape(-1, 3), axis=0)) > 20
    assert not np.array_equal(frames["surface"][0], frames["surface"][1])           # the block fell in between
    for k in (0, 1):
        assert not np.array_equal(frames["surface"][k], frames["spheres"][k])
