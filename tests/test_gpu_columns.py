"""Column maps on the device (include/sph_hip.h, section "Depth-integrated column maps"; csrc/sph_columns.hip) against the
numpy model of tests/columns_model.py on the context's OWN downloaded x, v, material and object_id.

Every comparison is exact (array_equal): the index is one f32 subtract, one f32 multiply and a floor, the velocity terms are
llrint of an exact f64 product, the sums are integers and the extrema are f32 values -- nothing rounds differently on the two
sides, so there is no tolerance to choose.
"""
import copy
import ctypes as C
import json
import struct

import numpy as np
import pytest

from sph_taichi_amd import ParticleSystem, _lib, columns
from sph_taichi_amd.config_builder import SimConfig
from tests import columns_model as model
from tests import scenes

pytestmark = pytest.mark.gpu

FIELDS = ("x", "v", "acceleration", "m_V", "m", "density", "pressure", "material", "color", "is_dynamic", "object_id",
          "grid_ids")
RAW = ("count", "sum_v", "top", "bottom")


def _download(ps):
    return {f: getattr(ps, f).to_numpy() for f in ("x", "v", "material", "object_id")}


def _check(ps, fields=None, tag="", **kw):
    """ps.column_map(**kw) against the model on the fields as they are now; returns the map."""
    cm = ps.column_map(**kw)
    f = fields if fields is not None else _download(ps)
    oid = -1 if kw.get("object_id") is None else int(kw["object_id"])
    want = model.column_map(f["x"], f["v"], f["material"], f["object_id"], cm.axis, np.asarray(cm.origin, np.float32),
                            model.inv_cell(cm.cell), cm.shape, select_object=oid)
    for k in RAW:
        got = getattr(cm, k)
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (tag, k)
        assert np.array_equal(got, want[k]), (tag, kw, k, int((got != want[k]).sum()))
    assert (cm.selected, cm.binned, cm.outside) == (want["selected"], want["binned"], want["outside"]), (tag, kw)
    assert cm.binned + cm.outside == cm.selected and int(cm.count.sum()) == cm.binned and cm.time == ps.time
    return cm


def _bytes(cm):
    return b"".join(getattr(cm, k).tobytes() for k in RAW) + struct.pack("<3q", cm.selected, cm.binned, cm.outside)


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def test_mixed_scene_against_the_model():
    """Fluid + static block + dynamic block after step(7): N ragged against 64 and 256, solids that must not be binned."""
    sd = scenes.fluid_with_rigid_blocks()
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    solver.step(7)
    n = ps.particle_max_num
    assert n % 64 != 0 and n % 256 != 0 and n > 256, n
    f = _download(ps)
    n_fluid = int((f["material"] == 1).sum())
    for axis in (0, 1, 2):
        cm = _check(ps, f, "mixed", axis=axis)
        assert cm.selected == n_fluid == ps.fluid_particle_num and cm.binned > 0 and cm.axis == axis
        assert cm.shape == tuple(int(np.ceil(ps.domain_size[j] / ps.support_radius)) for j in cm.axes)
        one = _check(ps, f, "mixed, object 0", axis=axis, object_id=0)
        assert _bytes(one) == _bytes(cm)                                   # object 0 is all the fluid there is
        for rigid in (1, 2):
            empty = _check(ps, f, "mixed, a rigid object", axis=axis, object_id=rigid)
            assert empty.selected == empty.binned == empty.outside == 0 and empty.wet_extent() is None
            assert not empty.count.any() and not empty.sum_v.any() and not empty.top.any() and not empty.bottom.any()
    ps.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_less_than_one_wave():
    sd = scenes.fluid_only(counts=(3, 3, 3))
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    cm = _check(ps, tag="27 particles")
    assert cm.count.sum() == 27 and cm.selected == 27 and cm.outside == 0
    v = cm.velocity
    assert (v[..., 1][cm.wet] == -1.0).all() and np.isnan(v[..., 1][~cm.wet]).all() and cm.wet.any() and not cm.wet.all()
    ps.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_shapes_that_break_the_combining_stage():
    """One state (16 particles per cell after 5 steps), four maps: every particle in ONE column (runs far longer than a wave,
    one table slot); cells of half a particle spacing (runs of one, more columns than table slots); a map over the middle of
    the block only (particles outside on every side); a map shifted by a negative origin."""
    ps, solver = scenes.make_ps(scenes.crowded_fluid())
    solver.initialize()
    solver.step(5)
    f = _download(ps)
    n = f["x"].shape[0]
    d = ps.particle_diameter
    one = _check(ps, f, "1 x 1", cell=(1.0, 0.8), shape=(1, 1))
    assert one.count.tolist() == [[n]] and one.outside == 0
    assert one.top[0, 0] == f["x"][:, 1].max() and one.bottom[0, 0] == f["x"][:, 1].min()
    fine = _check(ps, f, "cell = d / 2", cell=d / 2)
    assert fine.outside == 0 and int(fine.wet.sum()) > 512                  # more wet columns than the block table has slots
    lo, hi = f["x"].min(axis=0), f["x"].max(axis=0)
    mid = _check(ps, f, "the middle", cell=d, origin=(float(lo[0]) + 0.1, float(lo[2]) + 0.1), shape=(9, 7))
    assert 0 < mid.outside < n and mid.binned > 0
    assert mid.wet[0].any() and mid.wet[-1].any() and mid.wet[:, 0].any() and mid.wet[:, -1].any()      # the map's edges are in the fluid
    neg = _check(ps, f, "negative origin", origin=(-0.33, -0.17))
    assert neg.outside == 0 and neg.origin == (-0.33, -0.17)
    for axis in (0, 2):
        _check(ps, f, "the middle, other axes", axis=axis, cell=d, origin=(float(lo[1 if axis == 0 else 0]) + 0.05, 0.15), shape=(5, 6))
    ps.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_order_independence():
    """x and v permuted (not sorted) and uploaded: the map equals the model, and two different permutations give the same
    bytes.  A few velocities are replaced: +-7e4 (clamps to +-65536), -0.0, +-3 * 2^-21 (ties: +-1.5 -> +-2)."""
    ps, solver = scenes.make_ps(scenes.crowded_fluid())
    solver.initialize()
    solver.step(5)
    x, v = ps.x.to_numpy(), ps.v.to_numpy()
    n = x.shape[0]
    v[3] = (7e4, -7e4, -0.0)
    v[n // 2] = (3 * 2.0 ** -21, -3 * 2.0 ** -21, 7e4)
    v[n - 1] = (-0.0, 2.0 ** -21, -2.0 ** -21)                # ties: +-0.5 -> 0
    rng = np.random.default_rng(11)
    maps = []
    for k in range(2):
        perm = rng.permutation(n)
        ps.x.from_numpy(x[perm])
        ps.v.from_numpy(v[perm])
        f = _download(ps)
        assert np.array_equal(f["x"], x[perm]) and np.array_equal(f["v"], v[perm]) and (f["material"] == 1).all()
        cm = _check(ps, f, f"permutation {k}", cell=ps.particle_diameter)
        again = ps.column_map(cell=ps.particle_diameter)
        assert _bytes(cm) == _bytes(again), "two calls on one state differ"
        coarse = _check(ps, f, f"permutation {k}, default map")
        maps.append((_bytes(cm), _bytes(coarse)))
    assert maps[0] == maps[1], "the map depends on the particle order"
    ps.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def _all_fields(ps):
    return {f: scenes.ps_by_pid(ps, f) for f in FIELDS}


@pytest.mark.parametrize("dfsph", [False, True], ids=["wcsph", "dfsph"])
def test_side_effect_free(dfsph):
    sd = scenes.fluid_with_rigid_blocks()
    if dfsph:
        sd = scenes.as_dfsph(sd)
    a, solver_a = scenes.make_ps(sd)
    solver_a.initialize()
    solver_a.step(5)
    for axis in (0, 1, 2):
        cm = a.column_map(axis=axis)
        assert cm.selected == a.fluid_particle_num
    solver_a.step(5)
    b, solver_b = scenes.make_ps(sd)
    solver_b.initialize()
    solver_b.step(10)
    fa, fb = _all_fields(a), _all_fields(b)
    for f in FIELDS:
        assert np.array_equal(fa[f], fb[f]), f"{f} differs after column maps between the steps"
    assert a.time == b.time
    a.close(); b.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_physics_lattice_and_fall():
    counts, start = (10, 12, 8), (0.1, 0.1, 0.1)
    ps, solver = scenes.make_ps(scenes.fluid_only(counts=counts, start=start))
    d, r = ps.particle_diameter, ps.particle_radius
    n = counts[0] * counts[1] * counts[2]
    cm = _check(ps, tag="rest lattice", cell=d, origin=(start[0] - d / 2, start[2] - d / 2), shape=(counts[0], counts[2]))
    assert cm.wet.all() and (cm.count == counts[1]).all() and cm.outside == 0 and cm.selected == n
    # depth = 12 d^3 / d^2: two f64 roundings in the factor, one in the product
    assert np.all(np.abs(cm.depth - counts[1] * d) <= 4 * 2.0 ** -53 * counts[1] * d)
    # surface - bottom + radius = (top - bottom) + d = 12 d; top and bottom are f32 lattice coordinates near 0.32 and 0.1:
    # half an ulp of each (2^-25 * 0.5, 2^-25 * 0.125) and the scene's own f32 lattice arithmetic, within 4 ulp of 0.5
    span = cm.surface - cm.bottom.astype(np.float64) + r
    assert np.all(np.abs(span - counts[1] * d) <= 4 * 2.0 ** -24 * 0.5), np.abs(span - counts[1] * d).max()
    assert cm.wet_extent() == ((cm.origin[0], cm.origin[0] + counts[0] * d), (cm.origin[1], cm.origin[1] + counts[2] * d))
    solver.initialize()
    solver.step(200)
    cm = _check(ps, tag="after the fall")
    assert cm.binned + cm.outside == n == ps.fluid_particle_num and cm.outside == 0
    row = ps.diagnostics().objects[0]
    ext = cm.wet_extent()
    # The first wet column holds the lowest particle, the last the highest.  A column edge in f32 index arithmetic sits within
    # 2^-23 relative of origin + k * cell (one rounding of inv_cell, one of the product; origin = 0 here): eps covers it
    # with the domain's largest extent as the magnitude.
    eps = 2.0 ** -23 * 1.2
    for j, a in enumerate(cm.axes):
        assert ext[j][0] - eps <= row.lo[a] < ext[j][0] + cm.cell[j] + eps, (a, ext[j], row.lo[a])
        assert ext[j][1] - cm.cell[j] - eps <= row.hi[a] <= ext[j][1] + eps, (a, ext[j], row.hi[a])
    assert cm.bottom[cm.wet].min() == np.float32(row.lo[1]) and cm.top[cm.wet].max() == np.float32(row.hi[1])
    ps.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def _params(axis=1, n=(4, 4), origin=(0.0, 0.0), inv_cell=(12.5, 12.5), object_id=-1):
    p = _lib.SphColumnParams()
    p.axis, p.object_id = axis, object_id
    p.n = (C.c_int32 * 2)(*n)
    p.origin = (C.c_float * 2)(*origin)
    p.inv_cell = (C.c_float * 2)(*inv_cell)
    return p


def test_refusals():
    sd = scenes.fluid_only(counts=(4, 4, 4))
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    count = np.zeros(64, dtype=np.int64)
    totals = _lib.SphColumnTotals()
    down = lambda nc: ps._call("sph_columns_download", count.ctypes.data_as(C.c_void_p), None, None, None, nc, C.byref(totals))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been reduced"):
        down(16)
    for bad, msg in ((dict(axis=3), "axis"), (dict(axis=-1), "axis"), (dict(n=(0, 4)), "at least 1"), (dict(n=(4, -2)), "at least 1"),
                     (dict(n=(1 << 11, (1 << 9) + 1)), "SPH_COLUMNS_MAX"), (dict(inv_cell=(0.0, 12.5)), "inv_cell"),
                     (dict(inv_cell=(25.0, float("nan"))), "inv_cell"), (dict(inv_cell=(float("inf"), 25.0)), "inv_cell"),
                     (dict(inv_cell=(-1.0, 25.0)), "inv_cell"), (dict(origin=(float("nan"), 0.0)), "origin")):
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*{msg}"):
            ps._call("sph_columns_reduce", C.byref(_params(**bad)))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been reduced"):
        down(16)                                                            # a refused reduce leaves nothing to download
    ps._call("sph_columns_reduce", C.byref(_params()))
    for bad in (15, 17, 0):
        with pytest.raises(_lib.SphError, match=r"rc=-1.*n_columns"):
            down(bad)
    down(16)
    assert count[:16].sum() == 64 == totals.selected == totals.binned and totals.outside == 0 and not count[16:].any()
    ps._call("sph_columns_reduce", C.byref(_params(n=(8, 8))))              # another size: the planes are allocated again
    with pytest.raises(_lib.SphError, match=r"rc=-1.*n_columns"):
        down(16)
    down(64)
    assert count.sum() == 64
    ps.close()
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.column_map()
    with pytest.raises(_lib.SphError, match=r"rc=-4.*single-domain"):
        slab._call("sph_columns_reduce", C.byref(_params()))
    slab.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def _png_size(path):
    with open(path, "rb") as fh:
        head = fh.read(33)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR"
    w, h, depth, colour = struct.unpack(">IIBB", head[16:26])
    assert depth == 8
    return w, h


def test_run_simulation_gauges_and_heightmaps(tmp_path):
    """27 particles in free fall, timeStepSize 0.016 so that every frame is an output interval (the lattice at rest spacing
    exerts no pressure, so the large step is harmless): 3 frames, 3 lines, 3 images."""
    from sph_taichi_amd import run_simulation
    sd = scenes.fluid_only(counts=(3, 3, 3), start=(0.3, 0.3, 0.3))
    sd["Configuration"]["timeStepSize"] = 0.016
    points = [[0.33, 0.33], [0.9, 0.7], [5.0, 5.0]]                        # wet, dry, outside the map
    sd["Configuration"]["gauges"] = {"axis": 1, "cell": 0.04, "points": points}
    scene_file = tmp_path / "gauge_scene.json"
    scene_file.write_text(json.dumps(sd))
    out, hm = tmp_path / "gauges.jsonl", tmp_path / "heightmaps"
    run_simulation.main(["--scene_file", str(scene_file), "--frames", "3", "--gauges", str(out), "--heightmap_dir", str(hm)])
    lines = [json.loads(s) for s in out.read_text().splitlines()]
    assert [row["frame"] for row in lines] == [0, 1, 2]
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    for k, row in enumerate(lines):
        solver.step(1)
        cm = ps.column_map(axis=1, cell=0.04)
        assert row["time"] == cm.time and row["selected"] == 27 == cm.selected and row["outside"] == cm.outside == 0
        assert row["wet_extent"] == [list(e) for e in cm.wet_extent()]
        assert row["gauges"] == json.loads(json.dumps(columns.gauge_rows(cm, points)))
        assert row["gauges"][0]["depth"] > 0 and row["gauges"][1]["depth"] == 0.0 and row["gauges"][2]["column"] == -1
        assert row["gauges"][1]["surface"] is None and row["gauges"][2]["depth"] is None
        assert _png_size(hm / f"{k:06}.png") == (cm.shape[1], cm.shape[0])
    assert sorted(p.name for p in hm.iterdir()) == ["000000.png", "000001.png", "000002.png"]
    assert lines[2]["gauges"][0]["surface"] < lines[0]["gauges"][0]["surface"]      # it falls
    ps.close()
