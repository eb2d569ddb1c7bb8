"""Frame export on the GPU: the device renderer (csrc/sph_render.hip) against the NumPy model of its specification
(tests/render_model.py), order independence, that a frame only reads, semantics, errors, and run_simulation end to end.

Parity figures (recording run on an MI355X, profiles/render_parity.json; covered pixels 1,617 / 27,402 / 1,740 / 33,557, sprite
radii 0.75-0.87 px from the far camera and 3.5-13.8 px from the close one): on all four scene / camera cases the device image
and depth equal the float32 model BIT FOR BIT -- 0 pixels of different coverage, 0 differing depth values, 0 differing channel
values.  Nothing rounds differently, so the bounds below are 0 (3 x 0).  The same file holds the float32-against-float64
figures of the MODEL on the same states (the perturbation check): 0 pixels of different coverage or winner, at most 1 channel
level on 0-4 pixels, relative depth differences up to 4e-6 -- inside the cap of 0.1 % of the covered
pixels / 1 channel level)."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import render_model
import scenes
from sph_taichi_amd import _lib, render

pytestmark = pytest.mark.gpu

FAR = render.Camera(eye=(1.7, 1.1, 1.6), lookat=(0.25, 0.2, 0.2))
CLOSE = render.Camera(eye=(0.37, 0.33, 0.36), lookat=(0.2, 0.2, 0.2), near_plane=0.02)      # sprites tens of pixels wide
CASES = [("fluid_block", "far", FAR, (256, 256)), ("fluid_block", "close", CLOSE, (256, 256)),
         ("coupled", "far", FAR, (256, 256)), ("coupled", "close", CLOSE, (320, 240))]
_RECORD = {}


def _scene(name):
    return scenes.fluid_only() if name == "fluid_block" else scenes.fluid_with_rigid_blocks()


def _state(ps):
    return ps.x.to_numpy(), ps.color.to_numpy(), ps.object_id.to_numpy()


def _model(ps, cam, size, invisible=(), dtype=np.float32):
    x, col, oid = _state(ps)
    return render_model.render(x, col, oid, cam, size, ps.particle_radius, ps.domain_end, invisible, dtype)


def _compare(img, depth, mimg, mdepth):
    cov, mcov = np.isfinite(depth), np.isfinite(mdepth)
    both = cov & mcov
    rel = np.zeros(depth.shape)
    rel[both] = np.abs(depth[both].astype(np.float64) - mdepth[both]) / mdepth[both]
    chan = np.abs(img.astype(int) - mimg.astype(int))
    return {"covered_pixels": int(mcov.sum()), "coverage_differs": int((cov != mcov).sum()),
            "winner_differs": int((rel > 1e-4).sum()),            # another surface in front: a depth step, not a rounding
            "depth_values_differ": int((depth[both] != mdepth[both].astype(np.float32)).sum()),
            "max_rel_depth_diff": float(rel.max()), "channel_pixels_differ": int((chan.max(axis=-1) > 0).sum()),
            "max_channel_diff": int(chan.max())}


def _dump_record():
    out = scenes.evidence_path("render_parity.json")
    if out:
        json.dump(_RECORD, open(out, "w"), indent=1, sort_keys=True)


@pytest.mark.parametrize("scene,view,cam,size", CASES)
def test_model_parity(scene, view, cam, size):
    ps, solver = scenes.make_ps(_scene(scene))
    solver.initialize()
    solver.step(5)
    img = ps.render(cam, size=size)
    depth = ps.render_depth()
    assert img.shape == (size[1], size[0], 3) and img.dtype == np.uint8 and depth.shape == (size[1], size[0])
    mimg, mdepth, mwin = _model(ps, cam, size)
    got = _compare(img, depth, mimg, mdepth)
    # the perturbation check on the same state: the model in float64 against the model in float32
    dimg, ddepth, dwin = _model(ps, cam, size, dtype=np.float64)
    pert = _compare(mimg, mdepth, dimg, ddepth)
    pert["winner_differs"] = int((mwin != dwin).sum())
    # (where the two precisions show DIFFERENT particles the colours differ by whatever the two surfaces differ by: the
    # channel figure of the perturbation check is taken over the pixels that show the same particle)
    same = mwin == dwin
    pert["max_channel_diff_same_winner"] = int(np.abs(mimg.astype(int) - dimg.astype(int))[same].max())
    x = _state(ps)[0]
    radii = [s[5] for s in (render_model.sprite(render_model.Setup(cam, size, ps.particle_radius, ps.domain_end), p) for p in x) if s]
    _RECORD[f"{scene} / {view} {size[0]}x{size[1]}"] = {
        "camera": {"eye": list(cam.eye), "lookat": list(cam.lookat), "near_plane": cam.near_plane},
        "particles": int(x.shape[0]), "sprite_radius_px": [float(min(radii)), float(max(radii))],
        "gpu_vs_model_f32": got, "model_f32_vs_model_f64": pert}
    _dump_record()
    print(scene, view, got, pert)
    ncov = got["covered_pixels"]
    assert ncov > 500 and len(np.unique(img.reshape(-1, 3), axis=0)) > 20
    if view == "close":
        assert max(radii) > 10.0                          # the wave-per-particle path is in the picture
    # the perturbation stays inside the cap (else the camera is wrong for this check, not the cap)
    assert pert["coverage_differs"] + pert["winner_differs"] <= 1e-3 * ncov and pert["max_channel_diff_same_winner"] <= 1
    # GPU against the float32 model: measured 0 everywhere -> bounds 0 (3 x 0); the cap of 0.1 % / 1 level holds a fortiori
    assert got["coverage_differs"] == 0 and got["winner_differs"] == 0
    assert got["depth_values_differ"] == 0 and got["max_rel_depth_diff"] == 0.0
    assert got["channel_pixels_differ"] == 0 and got["max_channel_diff"] == 0
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
        for cam, size in ((FAR, (256, 256)), (CLOSE, (320, 240))):
            a, da = ps.render(cam, size=size), ps.render_depth()
            b, db = ps.render(cam, size=size), ps.render_depth()      # the same context twice
            assert np.array_equal(a, b) and np.array_equal(da, db)
            out.append((a, da))
        ps.close()
    assert np.isfinite(out[0][1]).sum() > 500 and np.isfinite(out[1][1]).sum() > 500
    for k in (0, 1):
        assert np.array_equal(out[k][0], out[k + 2][0]) and np.array_equal(out[k][1], out[k + 2][1])


def test_rendering_only_reads():
    sd = scenes.fluid_with_rigid_blocks()
    runs = []
    for with_frames in (False, True):
        ps, solver = scenes.make_ps(sd)
        solver.initialize()
        for _ in range(8):
            solver.step(1)
            if with_frames:
                ps.render(FAR, size=(128, 128))
                ps.render(CLOSE, size=(200, 100), invisible_objects=[1])
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
    # particles 0..5 of the fluid: at the eye, just inside the near plane, just outside it, behind the camera, far off screen
    arrays["x"][0] = eye
    arrays["x"][1] = eye + 0.099 * f
    arrays["x"][2] = eye + 0.101 * f
    arrays["x"][3] = eye - 0.3 * f
    arrays["x"][4] = eye + 0.2 * f + np.array([30.0, 0.0, 0.0])
    ps, solver = scenes.make_ps(sd, arrays)
    size = (192, 160)
    for invisible in ((), [1], [0, 2], [0, 1, 2]):
        img, depth = ps.render(cam, invisible_objects=invisible, size=size), None
        depth = ps.render_depth()
        mimg, mdepth, mwin = _model(ps, cam, size, invisible)
        assert np.array_equal(img, mimg) and np.array_equal(depth, mdepth), invisible
        shown = set(np.unique(mwin[mwin >= 0]))
        assert not shown & {0, 1, 3, 4}, shown                  # culled: at the eye, inside the near plane, behind, off screen
        if not invisible:
            assert 2 in shown                                   # just outside the near plane: drawn, by the wave-per-particle path (R = 11 px)
            oid = ps.object_id.to_numpy()
            assert set(oid[sorted(shown)]) == {0, 1, 2}
    # every object hidden: background + box, and nothing else
    box = mwin == -2
    assert box.sum() > 50 and np.all(img[box] == (252, 173, 71)) and np.all(img[~box] == 0) and np.all(np.isinf(depth[~box]))
    nobox = copy.copy(cam)
    nobox.draw_box = False
    nobox.background = (10, 20, 30)
    img = ps.render(nobox, invisible_objects=[0, 1, 2], size=size)
    assert np.all(img == (10, 20, 30)) and np.all(np.isinf(ps.render_depth()))
    img = ps.render(nobox, size=size)
    mimg, mdepth, mwin = _model(ps, nobox, size)
    assert np.array_equal(img, mimg) and not (mwin == -2).any() and np.all(img[mwin == -1] == (10, 20, 30))
    # looking away from everything: background only
    away = render.Camera(eye=(0.5, 0.5, 2.0), lookat=(0.5, 0.5, 5.0))
    assert np.all(ps.render(away, size=(64, 48)) == 0)
    ps.close()


def _rc(ps, **over):
    rp = render.render_params(over.pop("camera", render.Camera()), over.pop("size", (64, 64)), over.pop("radius", 0.01), (1, 1, 1))
    for k, v in over.items():
        setattr(rp, k, v)
    return ps._lib.sph_render_set_params(ps._ctx, C.byref(rp))


def test_errors():
    from sph_taichi_amd import ParticleSystem
    from sph_taichi_amd.config_builder import SimConfig
    sd = scenes.fluid_only()
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    E_INVALID, E_STATE = -1, -4
    assert ps._lib.sph_render_frame(ps._ctx) == E_STATE                     # no parameters yet
    buf = np.zeros(64 * 64 * 3, np.uint8)
    assert ps._lib.sph_render_download(ps._ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == E_STATE
    assert _rc(ps) == 0
    bad = [dict(size=(0, 64)), dict(size=(64, 0)), dict(size=(64, 20000)),
           dict(camera=render.Camera(eye=(1, 2, 3), lookat=(1, 2, 3))),
           dict(camera=render.Camera(eye=(0, 0, 0), lookat=(0, 3, 0), up=(0, 1, 0))),
           dict(camera=render.Camera(up=(0, 0, 0))),
           dict(radius=0.0), dict(radius=-1.0), dict(camera=render.Camera(fov_y_deg=0.0)), dict(camera=render.Camera(fov_y_deg=-5.0)),
           dict(camera=render.Camera(fov_y_deg=180.0)), dict(camera=render.Camera(near_plane=0.0)),
           dict(camera=render.Camera(ambient=1.5)), dict(camera=render.Camera(eye=(float("nan"), 0, 0)))]
    for over in bad:
        assert _rc(ps, **copy.deepcopy(over)) == E_INVALID, over
        assert b"sph_render_set_params" in ps._lib.sph_last_error(ps._ctx)
    ids = (C.c_int32 * 40)()
    assert ps._lib.sph_render_set_invisible(ps._ctx, ids, 33) == E_INVALID
    assert ps._lib.sph_render_set_invisible(ps._ctx, ids, -1) == E_INVALID
    with pytest.raises(_lib.SphError, match="rc=-1"):
        ps.render(render.Camera(eye=(1, 1, 1), lookat=(1, 1, 1)))
    # the last good parameters are still in force, the context renders and steps
    assert ps._lib.sph_render_frame(ps._ctx) == 0
    assert ps._lib.sph_render_download(ps._ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 1) == E_INVALID
    assert ps._lib.sph_render_download(ps._ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
    solver.step(3)
    img = ps.render(FAR, size=(96, 96))
    assert np.array_equal(img, _model(ps, FAR, (96, 96))[0])
    ps.close()
    # a slab rank: compositing across GPUs is not built
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    assert _rc(slab) == E_STATE and slab._lib.sph_render_frame(slab._ctx) == E_STATE
    assert slab._lib.sph_render_set_invisible(slab._ctx, ids, 1) == E_STATE
    with pytest.raises(_lib.SphError, match="rc=-4"):
        slab.render()
    assert slab.count() == 960
    slab.close()


def test_run_simulation_writes_frames(tmp_path, monkeypatch, capsys):
    from test_render_host import decode_png
    from sph_taichi_amd import run_simulation
    sd = scenes.fluid_with_rigid_blocks()
    sd["Configuration"].update(exportFrame=True, invisibleObjects=[1])
    d = tmp_path / "data" / "scenes"
    d.mkdir(parents=True)
    (d / "coupled.json").write_text(json.dumps(sd))
    monkeypatch.chdir(tmp_path)
    run_simulation.main(["--scene_file", str(d / "coupled.json"), "--frames", "80", "--image_size", "160", "120",
                         "--camera", "1.7", "1.1", "1.6", "0.25", "0.2", "0.2"])
    assert sorted(os.listdir(tmp_path / "coupled_output_img")) == ["000000.png", "000040.png"]
    frames = [decode_png(str(tmp_path / "coupled_output_img" / n)) for n in ("000000.png", "000040.png")]
    for img in frames:
        assert img.shape == (120, 160, 3) and len(np.unique(img.reshape(-1, 3), axis=0)) > 20
        assert not np.any(np.all(img == (255, 255, 255), axis=-1))          # the white slab (object 1) is invisible
    assert not np.array_equal(frames[0], frames[1])                         # the block fell in between
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["frames_written"] == 2 and report["render_ms_per_frame"] > 0 and report["steps"] == 80
