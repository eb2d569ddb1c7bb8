"""Field colouring of the frames on the GPU: the coloured sphere frame and surface frame against the NumPy model of their
specification (tests/fieldcolour_model.py), the range reduction against NumPy, selection semantics, order independence, that
nothing else moves, refusals, and run_simulation end to end.

Bounds: the sphere frame's are those of test_gpu_render.test_model_parity (0 differing pixels in coverage, depth and channels: the
fragment arithmetic is the same function with another colour).  The surface frame's are 3 x the recording run's figures on an
MI355X (profiles/fieldcolour_parity.json), which are 0 on all five cases for image, depth, thickness and index plane: the new pass
uses + - x / only, with contraction off."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import fieldcolour_model as fm
import scenes
from sph_taichi_amd import _lib, render
from sph_taichi_amd.render import FieldColour
from test_gpu_render import CLOSE, FAR

pytestmark = pytest.mark.gpu

RANGES = {"speed": (0.4, 1.6), "vx": (-0.05, 0.05), "vy": (-1.2, -0.4), "vz": (-0.05, 0.05), "density": (995.0, 1030.0),
          "pressure": (0.0, 1500.0), "x": (0.1, 0.32), "y": (0.05, 0.35), "z": (0.1, 0.3)}
SPHERE_CASES = [(f, ("fluid_block", "coupled")[k & 1], FAR, ((256, 256), (320, 240))[(k >> 1) & 1]) for k, f in enumerate(render.FIELDS)] + \
               [("speed", "fluid_block", CLOSE, (256, 256)), ("pressure", "coupled", CLOSE, (320, 240))]
# scene, view, camera, size, filter radius in particle radii: the five kinds of case of profiles/surface_parity.json
SURFACE_CASES = [("fluid_block", "far", FAR, (256, 256), 1.0), ("fluid_block", "close", CLOSE, (250, 130), None),
                 ("coupled", "far", FAR, (250, 130), None), ("coupled", "close", CLOSE, (256, 256), None),
                 ("coupled", "close", CLOSE, (8, 8), None)]
BOUND_COVERAGE = BOUND_DEPTH_VALUES = BOUND_THICKNESS_VALUES = BOUND_CHANNEL_PIXELS = BOUND_CHANNEL_LEVELS = BOUND_INDEX_VALUES = 0
_RECORD = {}
_PS = {}


@pytest.fixture(scope="module")
def stepped():
    """name -> (ps, solver, state) of the two scenes after 5 steps, made once."""
    def get(name):
        if name not in _PS:
            ps, solver = scenes.make_ps(scenes.fluid_only() if name == "fluid_block" else scenes.fluid_with_rigid_blocks())
            solver.initialize()
            solver.step(5)
            _PS[name] = (ps, solver, fm.state(ps))
        return _PS[name]
    yield get
    for ps, _, _ in _PS.values():
        ps.close()
    _PS.clear()


@pytest.mark.parametrize("field,scene,cam,size", SPHERE_CASES)
def test_sphere_frame_against_the_model(stepped, field, scene, cam, size):
    ps, _, st = stepped(scene)
    colour = FieldColour(field, range=RANGES[field], colormap="rainbow", material=None if field == "density" else "fluid", axis_origin=0.01)
    img, depth = ps.render(cam, size=size, colour=colour), ps.render_depth()
    assert ps.frame_colour_range == tuple(float(np.float32(v)) for v in RANGES[field])
    mimg, mdepth, mwin = fm.render(ps, colour, RANGES[field], cam, size, st=st)
    cov, mcov = np.isfinite(depth), np.isfinite(mdepth)
    chan = np.abs(img.astype(int) - mimg.astype(int))
    got = {"covered_pixels": int(mcov.sum()), "coverage_differs": int((cov != mcov).sum()),
           "depth_values_differ": int((depth != mdepth.astype(np.float32)).sum()),
           "channel_pixels_differ": int((chan.max(axis=-1) > 0).sum()), "max_channel_diff": int(chan.max())}
    print(field, scene, size, got)
    assert got["covered_pixels"] > 500
    assert got["coverage_differs"] == 0 and got["depth_values_differ"] == 0
    assert got["channel_pixels_differ"] == 0 and got["max_channel_diff"] == 0
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 20
    plain = ps.render(cam, size=size)
    assert not np.array_equal(img, plain) and np.array_equal(depth, ps.render_depth())
    if cam is CLOSE:
        radii = [s[5] for s in (fm.render_model.sprite(fm.render_model.Setup(cam, size, ps.particle_radius, ps.domain_end), p) for p in st["x"]) if s]
        assert max(radii) > 10.0                              # the wave-per-sprite path is in the picture


def _check_range(ps, field, material, objects, invisible, st=None):
    st = st if st is not None else fm.state(ps)
    got = ps.field_range(field, material=material, objects=objects, invisible_objects=invisible)
    want = fm.field_range(st, FieldColour(field, material=material, objects=objects), invisible)
    assert np.array_equal(np.array(got[:2], np.float32), np.array(want[:2], np.float32)) and got[2:] == want[2:], (field, material, objects, got, want)
    return got


def test_field_range(stepped):
    ps, _, st = stepped("coupled")
    for field in render.FIELDS:
        lo, hi, n, bad = _check_range(ps, field, "fluid", None, (), st)
        assert n == 800 and bad == 0 and lo <= hi
        _check_range(ps, field, None, None, (1,), st)
        _check_range(ps, field, "solid", [2], (), st)
    assert _check_range(ps, "speed", "fluid", [1], (), st) == (float("inf"), float("-inf"), 0, 0)      # an empty selection
    assert _check_range(ps, "speed", "fluid", None, (0,), st)[2] == 0                                   # ... and a hidden one
    # a NaN and an inf velocity written in: they come back in non_finite and stay out of the extrema
    ps2, solver2 = scenes.make_ps(scenes.fluid_only(counts=(3, 3, 3)))
    solver2.initialize()
    assert ps2.count() == 27
    for field in render.FIELDS:
        _check_range(ps2, field, "fluid", None, ())
    v = ps2.v.to_numpy()
    v[5, 0] = np.nan
    v[11, 1] = np.inf
    v[3] = (0.25, -3.0, 0.5)
    ps2.v.from_numpy(v)
    assert _check_range(ps2, "speed", "fluid", None, ())[2:] == (25, 2)
    assert _check_range(ps2, "vx", "fluid", None, ())[2:] == (26, 1) and _check_range(ps2, "vy", None, None, ())[:2] == (-3.0, -1.0)
    assert _check_range(ps2, "vz", "fluid", None, ())[2:] == (27, 0)
    ps2.close()


def test_field_range_over_several_tiles_with_a_ragged_tail():
    ps, solver = scenes.make_ps(scenes.fluid_only(counts=(42, 48, 35), start=(0.05, 0.05, 0.05)))
    solver.initialize()
    assert ps.count() == 70560                                # 276 tiles of 256 over at most 256 blocks: two tiles per block, 160 records in the last
    st = fm.state(ps)
    for field in render.FIELDS:
        assert _check_range(ps, field, "fluid", None, (), st)[2] == 70560
    ps.close()


def test_auto_range_is_the_reduced_range(stepped):
    ps, _, st = stepped("coupled")
    for style in ("spheres", "surface"):
        frame = (lambda **k: ps.render(FAR, size=(250, 130), **k)) if style == "spheres" else (lambda **k: ps.render_surface(FAR, size=(250, 130), **k))
        auto = frame(colour=FieldColour("speed"))
        lo, hi, n, _ = ps.field_range("speed")
        assert ps.frame_colour_range == (lo, hi) and n == 800 and lo < hi
        assert np.array_equal(auto, frame(colour=FieldColour("speed", range=(lo, hi))))
        assert not np.array_equal(auto, frame(colour=FieldColour("speed", range=(lo, 2 * hi))))
        # an empty selection and a degenerate range still make a frame
        frame(colour=FieldColour("speed", objects=[9]))
        assert ps.frame_colour_range == (0.0, 1.0)
        frame(colour=FieldColour("vx", material="solid", objects=[1]))           # the static slab: every vx is 0
        assert ps.frame_colour_range == (0.0, 1.0) and ps.field_range("vx", "solid", [1])[:3] == (0.0, 0.0, 336)


def test_selection_semantics(stepped):
    ps, _, st = stepped("coupled")
    size = (256, 256)
    plain = ps.render(FAR, size=size)
    oid = st["object_id"]
    for colour, chosen in ((FieldColour("speed", range=RANGES["speed"], material="fluid"), oid == 0),
                           (FieldColour("y", range=RANGES["y"], material=None, objects=[2]), oid == 2),
                           (FieldColour("y", range=RANGES["y"], material="solid"), oid != 0)):
        img = ps.render(FAR, size=size, colour=colour)
        mimg, _, mwin = fm.render(ps, colour, colour.range, FAR, size, st=st)
        assert np.array_equal(img, mimg)
        shows_chosen = (mwin >= 0) & chosen[np.maximum(mwin, 0)]
        assert shows_chosen.sum() > 20 and (~shows_chosen & (mwin >= 0)).sum() > 20       # (the falling cube covers some 50 pixels)
        assert np.array_equal(img[~shows_chosen], plain[~shows_chosen])         # the others, box and background: today's bytes
        assert not np.array_equal(img[shows_chosen], plain[shows_chosen])
    colour = FieldColour("speed", range=RANGES["speed"], material=None)
    hidden = ps.render(FAR, invisible_objects=[0], size=size, colour=colour)
    mimg, _, mwin = fm.render(ps, colour, colour.range, FAR, size, invisible=[0], st=st)
    assert np.array_equal(hidden, mimg) and not np.any(oid[mwin[mwin >= 0]] == 0) and (mwin >= 0).sum() > 50


def _surface_compare(got, shown, m):
    """`shown`: where the first picture shows fluid."""
    img, depth, thick, index = got
    chan = np.abs(img.astype(int) - m["img"].astype(int)).max(axis=-1)
    both = shown & m["shown"]
    return {"fluid_pixels": int(m["shown"].sum()), "coverage_differs": int((shown != m["shown"]).sum()),
            "depth_values_differ": int((depth.astype(np.float64) != m["depth"].astype(np.float64)).sum()),
            "thickness_values_differ": int((thick.astype(np.float64) != m["thickness"].astype(np.float64)).sum()),
            "index_values_differ": int((index != m["index"]).sum()), "indexed_pixels": int((m["index"] >= 0).sum()),
            "channel_pixels_differ": int((chan > 0).sum()), "pixels_more_than_one_level": int((chan[both] > 1).sum()),
            "max_channel_diff": int(chan.max())}


@pytest.mark.parametrize("scene,view,cam,size,filter_radii", SURFACE_CASES)
def test_surface_frame_against_the_model(stepped, scene, view, cam, size, filter_radii):
    ps, _, st = stepped(scene)
    style = render.SurfaceStyle(**({"filter_radius": filter_radii * ps.particle_radius} if filter_radii is not None else {}))
    resolved = render.resolve_style(style, ps.particle_radius, ps._first_fluid_colour())
    colour = FieldColour("y", range=RANGES["y"], colormap="rainbow", material=None if scene == "coupled" else "fluid")
    got = (ps.render_surface(cam, size=size, style=style, colour=colour), ps.render_surface_depth(), ps.render_surface_thickness(),
           ps.render_surface_field_index())
    m = fm.surface(ps, colour, colour.range, cam, size, resolved, st=st)
    # (the device shows fluid where its depth lies in front of the opaque layer, whose depth test_gpu_render pins bit for bit)
    figures = _surface_compare(got, np.isfinite(got[1]) & (got[1] < m["zo"]), m)
    # the perturbation condition on the same state: the model in float32 against the model in float64
    d = fm.surface(ps, colour, colour.range, cam, size, resolved, dtype=np.float64, st=st)
    pert = _surface_compare((m["img"], m["depth"], m["thickness"], m["index"]), m["shown"], d)
    pert["index_more_than_one_level"] = int((np.abs(m["index"] - d["index"]) > 1).sum())
    _RECORD[f"{scene} / {view} {size[0]}x{size[1]}"] = {"field": colour.field, "range": list(colour.range), "gpu_vs_model_f32": figures,
                                                        "model_f32_vs_model_f64": pert}
    out = scenes.evidence_path("fieldcolour_parity.json")
    if out:
        json.dump(_RECORD, open(out, "w"), indent=1, sort_keys=True)
    print(scene, view, size, figures, pert)
    nf = figures["fluid_pixels"]
    assert nf > (20 if size == (8, 8) else 80) and figures["indexed_pixels"] >= nf
    plain = ps.render_surface(cam, size=size, style=style)
    assert not np.array_equal(got[0], plain) and np.array_equal(got[1], ps.render_surface_depth())
    with pytest.raises(_lib.SphError, match="rc=-4"):
        ps.render_surface_field_index()                       # the uncoloured frame has no index plane
    # the caps of test_gpu_surface (else the case is wrong for the check, not the cap)
    assert pert["coverage_differs"] <= 1e-3 * nf and pert["pixels_more_than_one_level"] <= 1e-2 * nf
    if os.environ.get("SPH_TEST_RECORD_ONLY") != "1":
        assert figures["coverage_differs"] <= BOUND_COVERAGE and figures["depth_values_differ"] <= BOUND_DEPTH_VALUES
        assert figures["thickness_values_differ"] <= BOUND_THICKNESS_VALUES and figures["index_values_differ"] <= BOUND_INDEX_VALUES
        assert figures["channel_pixels_differ"] <= BOUND_CHANNEL_PIXELS and figures["max_channel_diff"] <= BOUND_CHANNEL_LEVELS


def test_order_independence_and_reproducibility():
    sd = scenes.fluid_with_rigid_blocks()
    cfg, sc = scenes.build(sd)
    scenes.jitter(sc, 0.2, seed=3)
    rng = np.random.default_rng(4)
    sc.arrays["v"] = sc.arrays["v"] + rng.normal(0.0, 0.3, sc.arrays["v"].shape).astype(np.float32)
    perm = np.random.default_rng(11).permutation(sc.arrays["x"].shape[0])
    shuffled = {k: v[perm].copy() for k, v in sc.arrays.items() if k != "pid"}
    colour = FieldColour("speed", material=None)              # auto range
    out = []
    for arrays in (sc.arrays, shuffled):
        ps, solver = scenes.make_ps(sd, arrays)
        solver.initialize()                                # sorts; positions and velocities are the uploaded ones
        for cam, size in ((FAR, (250, 130)), (CLOSE, (256, 256))):
            a = (ps.render(cam, size=size, colour=colour), ps.frame_colour_range, ps.render_surface(cam, size=size, colour=colour),
                 ps.render_surface_field_index())
            b = (ps.render(cam, size=size, colour=colour), ps.frame_colour_range, ps.render_surface(cam, size=size, colour=colour),
                 ps.render_surface_field_index())
            assert all(np.array_equal(p, q) for p, q in zip(a, b))
            out.append(a)
        ps.close()
    assert (out[0][3] >= 0).sum() > 50 and len(np.unique(out[1][3])) > 20
    for k in (0, 1):
        assert all(np.array_equal(p, q) for p, q in zip(out[k], out[k + 2]))


@pytest.mark.parametrize("method", ["wcsph", "dfsph"])
def test_nothing_else_moves(method):
    sd = scenes.fluid_with_rigid_blocks()
    sd = scenes.as_dfsph(sd) if method == "dfsph" else sd
    runs = []
    for with_frames in (False, True):
        ps, solver = scenes.make_ps(sd)
        solver.initialize()
        solver.step(5)
        if with_frames:
            before = (ps.render(FAR, size=(128, 96)), ps.render_surface(CLOSE, size=(128, 96)))
            for field in ("pressure", "speed", "density"):
                colour = FieldColour(field, material=None)
                ps.render(FAR, size=(128, 96), colour=colour)
                ps.render_surface(CLOSE, size=(128, 96), colour=colour)
            after = (ps.render(FAR, size=(128, 96)), ps.render_surface(CLOSE, size=(128, 96)))      # switched off again
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        solver.step(5)
        st = _lib.SphStats()
        ps._call("sph_get_stats", C.byref(st))
        fields = {f: getattr(ps, f).to_numpy() for f in ps._STATE_FIELDS}
        fields["grid_ids"] = ps.grid_ids.to_numpy()
        runs.append((fields, bytes(st)))
        ps.close()
    for f in runs[0][0]:
        assert np.array_equal(runs[0][0][f], runs[1][0][f]), f
    assert runs[0][1] == runs[1][1]


def test_refusals():
    from sph_taichi_amd import ParticleSystem
    from sph_taichi_amd.config_builder import SimConfig
    sd = scenes.fluid_only()
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    E_INVALID, E_STATE = -1, -4
    lib, ctx = ps._lib, ps._ctx
    lut = FieldColour("speed").lut()
    lutp = lut.ctypes.data_as(C.c_void_p)

    def fp(**over):
        p = render.field_colour_params(FieldColour("speed"), (0.0, 1.0))
        for k, v in over.items():
            setattr(p, k, v)
        return p
    out = _lib.SphFieldRange()
    nan, inf = float("nan"), float("inf")
    for over in (dict(field=9), dict(field=-1), dict(material=-2), dict(material=256), dict(n_objects=-1), dict(n_objects=33), dict(axis_origin=nan)):
        assert lib.sph_frame_set_colour(ctx, C.byref(fp(**over)), lutp) == E_INVALID, over
        assert b"sph_frame_set_colour" in lib.sph_last_error(ctx)
        assert lib.sph_field_range(ctx, C.byref(fp(**over)), C.byref(out)) == E_INVALID, over
    for over in (dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0), dict(lo=nan), dict(hi=nan), dict(hi=inf), dict(lo=-inf), dict(lo=-3e38, hi=3e38),
                 dict(lo=0.0, hi=1e-45)):
        assert lib.sph_frame_set_colour(ctx, C.byref(fp(**over)), lutp) == E_INVALID, over
    bad = lut.copy()
    bad[17, 1] = 256
    assert lib.sph_frame_set_colour(ctx, C.byref(fp()), bad.ctypes.data_as(C.c_void_p)) == E_INVALID
    assert lib.sph_frame_set_colour(ctx, C.byref(fp()), None) == E_INVALID and lib.sph_frame_set_colour(ctx, None, lutp) == E_INVALID
    assert lib.sph_field_range(ctx, None, C.byref(out)) == E_INVALID and lib.sph_field_range(ctx, C.byref(fp()), None) == E_INVALID
    for shape in ((255, 3), (256, 4)):
        with pytest.raises(ValueError, match="colormap"):
            ps.render(FAR, size=(64, 48), colour=FieldColour("speed", colormap=np.zeros(shape, np.uint8)))
    with pytest.raises(TypeError):
        ps.render(FAR, size=(64, 48), colour="speed")
    # nothing of that switched a colouring on; a good one works, and null switches it off
    plain = ps.render(FAR, size=(64, 48))
    assert lib.sph_render_frame(ctx) == 0
    buf = np.empty_like(plain)
    assert lib.sph_render_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0 and np.array_equal(buf, plain)
    assert lib.sph_frame_set_colour(ctx, C.byref(fp(lo=0.5, hi=1.5)), lutp) == 0 and lib.sph_render_frame(ctx) == 0
    assert lib.sph_render_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0 and not np.array_equal(buf, plain)
    assert lib.sph_frame_set_colour(ctx, None, None) == 0 and lib.sph_render_frame(ctx) == 0
    assert lib.sph_render_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0 and np.array_equal(buf, plain)
    idx = np.empty((48, 64), np.int32)
    assert lib.sph_frame_download_field_index(ctx, idx.ctypes.data_as(C.c_void_p), idx.nbytes) == E_STATE
    ps.render_surface(FAR, size=(64, 48), colour=FieldColour("speed"))
    assert lib.sph_frame_download_field_index(ctx, idx.ctypes.data_as(C.c_void_p), idx.nbytes - 4) == E_INVALID
    assert lib.sph_frame_download_field_index(ctx, idx.ctypes.data_as(C.c_void_p), idx.nbytes) == 0 and idx.max() >= 0
    ps.close()
    # a slab rank
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    assert slab._lib.sph_frame_set_colour(slab._ctx, C.byref(fp()), lutp) == E_STATE
    assert slab._lib.sph_field_range(slab._ctx, C.byref(fp()), C.byref(out)) == E_STATE
    assert b"slab rank" in slab._lib.sph_last_error(slab._ctx)
    with pytest.raises(_lib.SphError, match="rc=-4"):
        slab.field_range("speed")
    with pytest.raises(_lib.SphError, match="rc=-4"):
        slab.render(colour=FieldColour("speed"))
    assert slab.count() == 960
    slab.close()


def test_run_simulation_writes_coloured_frames(tmp_path, monkeypatch, capsys):
    from test_fieldcolour_host import png_text
    from test_render_host import decode_png
    from sph_taichi_amd import run_simulation
    names = ("000000.png", "000040.png")
    frames = {}
    for key, extra in (("fixed", []), ("auto", ["--frame_colour", "speed", "--frame_style", "surface"]), ("none", None)):
        sd = scenes.fluid_with_rigid_blocks()
        sd["Configuration"].update(exportFrame=True)
        if key == "fixed":
            sd["Configuration"]["frameColour"] = {"field": "y", "range": [0.05, 0.35], "colormap": "coolwarm"}
        d = tmp_path / key / "data" / "scenes"
        d.mkdir(parents=True)
        (d / "coupled.json").write_text(json.dumps(sd))
        monkeypatch.chdir(tmp_path / key)
        run_simulation.main(["--scene_file", str(d / "coupled.json"), "--frames", "80", "--image_size", "160", "120",
                             "--camera", "1.7", "1.1", "1.6", "0.25", "0.2", "0.2"] + (extra or []))
        paths = [str(tmp_path / key / "coupled_output_img" / n) for n in names]
        frames[key] = [decode_png(p) for p in paths]
        report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert report["frames_written"] == 2
        texts = [png_text(p) for p in paths]
        if key == "none":
            assert "frame_colour_range" not in report and texts == [{}, {}]
        elif key == "fixed":
            assert report["frame_colour_range"] == [float(np.float32(0.05)), float(np.float32(0.35))]
            assert all(t["field"] == "y" and t["colormap"] == "coolwarm" and [float(t["lo"]), float(t["hi"])] == report["frame_colour_range"] for t in texts)
        else:
            assert [float(texts[1]["lo"]), float(texts[1]["hi"])] == report["frame_colour_range"] and texts[1]["field"] == "speed"
            assert float(texts[0]["lo"]) < float(texts[0]["hi"]) and texts[0] != texts[1]          # the range follows the flow
    for k in (0, 1):
        assert not np.array_equal(frames["fixed"][k], frames["none"][k])
        assert len(np.unique(frames["fixed"][k].reshape(-1, 3), axis=0)) > 20
