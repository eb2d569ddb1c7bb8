"""Field colouring of the frames, the parts that need no GPU: the colour tables, render.FieldColour and the scene key, the tEXt
chunks of write_png, and the index arithmetic of tests/fieldcolour_model.py (the model the GPU tests compare the device with) at its
edges and against a float64 evaluation.

Share of particles whose float32 index differs from the float64 one by one level, on the synthetic states of
test_index_f32_against_f64 (10,000 values per field, range = their extremes; recorded by that test's print): 0 of 10,000 on
speed, vx, density, pressure and y.  The cap asserted is 1 %, and never more than one level: only a value within a few
2^-24 relative of one of the 255 rounding boundaries of t * 255 + 0.5 can flip, a share of the order of 1e-4."""
import struct
import zlib

import numpy as np
import pytest

import fieldcolour_model as fm
from sph_taichi_amd import render
from sph_taichi_amd.render import FieldColour


def test_colormaps():
    for name in ("heat", "coolwarm", "grey", "rainbow"):
        lut = render.colormap(name)
        assert lut.shape == (256, 3) and lut.dtype == np.uint8
        pts = render._COLORMAPS[name]
        assert tuple(lut[0]) == pts[0][1:] and tuple(lut[255]) == pts[-1][1:]
        assert len(np.unique(lut, axis=0)) > 200
    grey = render.colormap("grey")
    assert np.array_equal(grey[:, 0], np.arange(256)) and np.all(grey[:, 0] == grey[:, 1]) and np.all(grey[:, 1] == grey[:, 2])
    heat = render.colormap("heat").astype(int)
    assert np.all(np.diff(heat.sum(axis=1)) >= 0)                   # brightness never falls
    # a control point between two entries: linear in float64, rounded half up
    assert tuple(render.colormap("coolwarm")[64]) == tuple(int(np.floor(v + 0.5)) for v in
                                                            np.array([141, 176, 254]) + (np.array([221, 221, 221]) - np.array([141, 176, 254])) * ((64 / 255 - 0.25) / 0.25))
    with pytest.raises(ValueError, match="coolwarm.*grey.*heat.*rainbow"):
        render.colormap("jet")


def test_field_colour_validation():
    c = FieldColour("speed")
    assert c.range is None and c.colormap == "heat" and c.material == "fluid" and c.objects is None and c.axis_origin == 0.0
    assert c.lut().dtype == np.int32 and c.lut().shape == (256, 3) and np.array_equal(c.lut(), render.colormap("heat"))
    for f in render.FIELDS:
        FieldColour(f, range=(-1.0, 2.5), colormap="rainbow", material=None, objects=[0, 2])
    with pytest.raises(ValueError, match="speed, vx, vy, vz, density, pressure, x, y, z"):
        FieldColour("vorticity")
    with pytest.raises(ValueError, match="speed, vx"):
        FieldColour(None)
    for bad in ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0), (1.0,), "ab", (1.0, 1.0 + 1e-12), (0.0, 1e-45),
                (-3e38, 3e38)):
        with pytest.raises(ValueError, match="range"):
            FieldColour("speed", range=bad)
    assert FieldColour("speed", range=[0, 3]).range == (0.0, 3.0)
    custom = np.zeros((256, 3), np.uint8)
    custom[:, 1] = np.arange(256)
    assert np.array_equal(FieldColour("y", colormap=custom).lut(), custom) and FieldColour("y", colormap=custom).colormap_name() == "custom"
    for bad in (np.zeros((255, 3), np.uint8), np.zeros((256, 4), np.uint8), np.zeros((256, 3), np.int32), np.zeros((3, 256), np.uint8), "jet"):
        with pytest.raises(ValueError, match="colormap"):
            FieldColour("speed", colormap=bad)
    for bad in ("water", 1):
        with pytest.raises(ValueError, match="material"):
            FieldColour("speed", material=bad)
    for bad in ([], [-1], [0.5], list(range(33)), [True]):
        with pytest.raises(ValueError, match="objects"):
            FieldColour("speed", objects=bad)
    assert FieldColour("speed", objects=3).objects == [3]
    with pytest.raises(ValueError, match="axis_origin"):
        FieldColour("y", axis_origin=float("nan"))
    p = render.field_colour_params(FieldColour("pressure", material="solid", objects=[4, 1], axis_origin=0.5), (-2.0, 7.0))
    assert (p.field, p.material, p.n_objects, p.object_ids[0], p.object_ids[1], p.lo, p.hi, p.axis_origin) == (5, 0, 2, 4, 1, -2.0, 7.0, 0.5)
    assert render.field_colour_params(FieldColour("z", material=None)).material == -1
    assert render.auto_range(1.5, 1.5, 10) == (1.5, 2.5) and render.auto_range(float("inf"), float("-inf"), 0) == (0.0, 1.0)
    assert render.auto_range(-1.0, 4.0, 3) == (-1.0, 4.0)


def test_scene_key():
    assert render.field_colour_from_config(None) is None
    c = render.field_colour_from_config({"field": "speed", "range": [0, 3], "colormap": "coolwarm", "material": None, "objects": [0],
                                         "axisOrigin": 0.25})
    assert (c.field, c.range, c.colormap, c.material, c.objects, c.axis_origin) == ("speed", (0.0, 3.0), "coolwarm", None, [0], 0.25)
    assert render.field_colour_from_config("density") == FieldColour("density")
    assert render.field_colour_from_config({"field": "y"}) == FieldColour("y")
    for entry, what in (({"field": "speed", "colour": 1}, "unknown key 'colour'.*axisOrigin.*field"), ({"range": [0, 1]}, "needs a \"field\""),
                        ({"field": "temperature"}, "frameColour: field must be one of speed"), ({"field": "speed", "range": [1, 0]}, "frameColour: range"),
                        ({"field": "speed", "colormap": [[0, 0, 0]]}, "colormap must be one of"), ({"field": "speed", "colormap": "jet"}, "colormap"),
                        (3, "frameColour must be"), ({"field": "speed", "material": "gas"}, "frameColour: material")):
        with pytest.raises(ValueError, match=what):
            render.field_colour_from_config(entry)


def test_run_simulation_refuses_a_bad_key_before_it_builds_anything(tmp_path, monkeypatch):
    import json
    import scenes
    from sph_taichi_amd import particle_system, run_simulation
    sd = scenes.fluid_only()
    sd["Configuration"].update(exportFrame=True, frameColour={"field": "warmth"})
    path = tmp_path / "s.json"
    path.write_text(json.dumps(sd))

    def no_device(*a, **k):
        raise AssertionError("a ParticleSystem was built")
    monkeypatch.setattr(run_simulation, "ParticleSystem", no_device)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="frameColour: field must be one of"):
        run_simulation.main(["--scene_file", str(path), "--frames", "1"])
    with pytest.raises(ValueError, match="frameColour: field must be one of"):
        run_simulation.main(["--scene_file", str(path), "--frames", "1", "--frame_colour", "hue"])
    assert run_simulation.build_parser().parse_args(["--frame_colour", "speed"]).frame_colour == "speed"


def png_chunks(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, pos = [], 8
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        out.append((tag, body))
        pos += 12 + n
    return out


def png_text(path):
    return {b.split(b"\0", 1)[0].decode("latin-1"): b.split(b"\0", 1)[1].decode("latin-1") for t, b in png_chunks(path) if t == b"tEXt"}


def test_write_png_text(tmp_path):
    from test_render_host import decode_png
    img = np.random.default_rng(0).integers(0, 256, (7, 5, 3), dtype=np.uint8)
    a, b, c = (str(tmp_path / n) for n in ("a.png", "b.png", "c.png"))
    render.write_png(a, img)
    render.write_png(b, img, text=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    text = {"field": "speed", "lo": repr(0.0), "hi": repr(2.75), "colormap": "heat"}
    render.write_png(c, img, text=text)
    chunks = png_chunks(c)
    assert [t for t, _ in chunks] == [b"IHDR", b"tEXt", b"tEXt", b"tEXt", b"tEXt", b"IDAT", b"IEND"]
    assert png_text(c) == text and float(png_text(c)["hi"]) == 2.75
    assert np.array_equal(decode_png(c), img) and png_text(a) == {}
    with pytest.raises(ValueError, match="tEXt keyword"):
        render.write_png(c, img, text={"": "x"})
    with pytest.raises(ValueError, match="tEXt keyword"):
        render.write_png(c, img, text={"k" * 80: "x"})


def test_index_edges():
    inf, nan = float("inf"), float("nan")
    for lo, hi in ((0.0, 3.0), (-2.0, 5.0), (-7.5, -1.25), (1e-3, 2e-3)):
        s = np.array([lo, hi, lo - 1.0, hi + 1.0, nan, inf, -inf, 0.5 * (lo + hi)], dtype=np.float32)
        idx = fm.index(s, lo, hi)
        assert list(idx[:7]) == [0, 255, 0, 255, 0, 255, 0] and idx[7] in (127, 128)
        assert idx.min() >= 0 and idx.max() <= 255
    # every level is reached, in order, and the half-way points round up
    s = np.arange(256, dtype=np.float32)
    assert np.array_equal(fm.index(s, 0.0, 255.0), np.arange(256))
    assert list(fm.index(np.array([0.49, 0.5, 1.5, 254.49, 254.5], np.float32), 0.0, 255.0)) == [0, 1, 2, 254, 255]
    # the speed of the block, operation by operation
    st = {"v": np.array([[3.0, 4.0, 12.0], [nan, 0.0, 0.0], [inf, 1.0, 0.0]], np.float32), "x": np.zeros((3, 3), np.float32)}
    sp = fm.field_values(st, "speed")
    assert sp[0] == 13.0 and np.isnan(sp[1]) and np.isinf(sp[2]) and sp.dtype == np.float32
    assert fm.field_values({"v": st["v"], "x": np.array([[0.0, 0.75, 0.0]] * 3, np.float32)}, "y", 0.25)[0] == 0.5


def test_index_f32_against_f64():
    rng = np.random.default_rng(5)
    n = 10000
    st = {"v": rng.normal(0.0, 1.5, (n, 3)).astype(np.float32), "x": rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32),
          "density": rng.uniform(950.0, 1100.0, n).astype(np.float32), "pressure": rng.uniform(0.0, 4000.0, n).astype(np.float32)}
    for field in ("speed", "vx", "density", "pressure", "y"):
        s32, s64 = fm.field_values(st, field, 0.1), fm.field_values(st, field, 0.1, np.float64)
        lo, hi = float(s32.min()), float(s32.max())
        i32, i64 = fm.index(s32, lo, hi), fm.index(s64, lo, hi, np.float64)
        d = np.abs(i32 - i64)
        share = float((d == 1).mean())
        print(f"{field}: {100 * share:.2f} % of {n} indices differ by one level, none by more: {bool(d.max() <= 1)}")
        assert d.max() <= 1 and share <= 0.01
        assert i32.min() == 0 and i32.max() == 255
