"""Particle export on the device (include/sph_hip.h, section "Particle export"; csrc/sph_export.hip) against the numpy model of
tests/export_model.py on the context's OWN downloaded x, v, density, pressure, m, material, object_id and pid.

Every comparison is exact (the bytes of the rows): the kernels select, rank and copy -- nothing is computed on a value, so there
is no tolerance to choose.
"""
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from sph_taichi_amd import ParticleSystem, _lib, build, export
from sph_taichi_amd.config_builder import SimConfig
from tests import export_model as model
from tests import scenes

pytestmark = pytest.mark.gpu

ALL = model.ALL_FIELDS
DOWNLOADS = ("x", "v", "density", "pressure", "m", "material", "object_id", "pid")
STATE = ("x", "v", "acceleration", "m_V", "m", "density", "pressure", "material", "color", "is_dynamic", "object_id", "grid_ids")
EXPORT_TILE = int(re.search(r"#define\s+SPH_EXPORT_TILE\s+(\d+)", open(os.path.join(build.CSRC, "sph_export.hip")).read()).group(1))


def _download(ps):
    return {f: getattr(ps, f).to_numpy() for f in DOWNLOADS}


def _model(f, fields=("velocity",), objects=None, material=None, box=None, every=1, phase=0):
    a = export.select_args(objects=objects, material=material, fields=fields, box=box, every=every, phase=phase)
    return model.export_rows(*[f[k] for k in DOWNLOADS], fields=a["fields"], objects=a["objects"] or None,
                             select_material=None if a["material"] < 0 else a["material"], box=a["box"], every=every, phase=phase)


def _check(ps, f=None, tag="", **kw):
    """ps.export_particles(**kw) against the model on the fields as they are now; returns the export."""
    ex = ps.export_particles(**kw)
    want = _model(f if f is not None else _download(ps), **kw)
    assert want["duplicate_ids"] == 0, tag
    assert ex.data.dtype == want["data"].dtype and ex.data.shape == want["data"].shape, (tag, kw, ex.data.shape, want["data"].shape)
    assert ex.data.tobytes() == want["data"].tobytes(), (tag, kw)
    assert (ex.count, ex.selected) == (want["rows"], want["selected"]) and ex.time == ps.time, (tag, kw)
    return ex


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def test_mixed_scene_against_the_model():
    """Fluid + static block + dynamic block after step(7) (a fused step: density / pressure still in its lean record): N ragged
    against 64 and 256."""
    ps, solver = scenes.make_ps(scenes.fluid_with_rigid_blocks())
    solver.initialize()
    solver.step(7)
    n = ps.particle_max_num
    assert n == 1200 and n % 64 != 0 and n % 256 != 0
    everything = ps.export_particles(fields=ALL)            # first: the export itself has to materialise density / pressure
    f = _download(ps)
    assert everything.data.tobytes() == _model(f, fields=ALL)["data"].tobytes()
    assert everything.count == n == everything.selected and everything.fields == ALL
    assert everything.data["id"].tolist() == list(range(n)) and everything.data.dtype.itemsize == 44
    assert _check(ps, f, "default fields").data.dtype.names == ("x", "y", "z", "vx", "vy", "vz")
    counts = {}
    for oid in (0, 1, 2):
        ex = _check(ps, f, f"object {oid}", objects=[oid], fields=ALL)
        assert (ex.data["object"] == oid).all() and ex.count > 0
        counts[oid] = ex.count
    assert sum(counts.values()) == n
    fluid = _check(ps, f, "fluid", material="fluid", fields=ALL)
    solid = _check(ps, f, "solid", material="solid", fields=("object", "mass"))
    assert fluid.count == counts[0] == ps.fluid_particle_num and solid.count == counts[1] + counts[2]
    assert set(solid.data["object"].tolist()) == {1, 2}
    two = _check(ps, f, "two objects", objects=[2, 0], fields=("id", "object"))
    assert two.count == counts[0] + counts[2] and (np.diff(two.data["id"]) > 0).all()
    none = _check(ps, f, "no such object", objects=[7], fields=("velocity", "pressure"))
    assert none.count == 0 == none.selected and none.data.shape == (0,) and none.data.dtype == export.row_dtype(("velocity", "pressure"))
    ps.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_less_than_one_wave():
    ps, solver = scenes.make_ps(scenes.fluid_only(counts=(3, 3, 3)))
    solver.initialize()
    ex = _check(ps, tag="27 particles", fields=ALL)
    assert ex.count == 27 and (ex.data["vy"] == -1.0).all()
    assert _check(ps, tag="27 particles, every third", fields=("id",), every=3, phase=2).data["id"].tolist() == list(range(2, 27, 3))
    ps.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_across_tiles_and_scan_trips():
    """More than 64 tiles of the id table: the offsets kernel (one wave, 64 tile counts per trip) makes a second trip.  Every third
    id leaves the tiles with unequal counts; a box over one corner of the block leaves most tiles empty."""
    counts, start = (42, 42, 40), (0.1, 0.1, 0.1)
    ps, solver = scenes.make_ps(scenes.fluid_only(counts=counts, start=start, domain_end=(1.2, 1.2, 1.2)))
    solver.initialize()
    n = ps.particle_max_num
    n_tiles = -(-n // EXPORT_TILE)
    assert n == 42 * 42 * 40 and n > 64 * EXPORT_TILE and n % EXPORT_TILE != 0 and n_tiles > 64
    f = _download(ps)
    per_tile = lambda ex: np.bincount(ex.data["id"] // EXPORT_TILE, minlength=n_tiles)
    _check(ps, f, "every particle", fields=ALL)
    third = _check(ps, f, "every third id", fields=("id", "velocity"), every=3, phase=1)
    assert third.count == len(range(1, n, 3)) and len(set(per_tile(third).tolist())) > 1 and per_tile(third)[65:].all()
    corner = ([0.0, 0.0, 0.0], [0.1 + 9.5 * 0.02, 0.1 + 9.5 * 0.02, 0.1 + 9.5 * 0.02])
    boxed = _check(ps, f, "a corner", fields=("id",), box=corner)
    assert boxed.count == 1000 and (per_tile(boxed) == 0).any() and (per_tile(boxed) > 0).sum() > 1
    both = _check(ps, f, "a corner, every third id", fields=ALL, box=corner, every=3, phase=1)
    assert 0 < both.count < boxed.count
    far = ([0.5, 0.5, 0.5], [2.0, 2.0, 2.0])                         # the opposite corner: the first tiles are the empty ones
    last = _check(ps, f, "the far corner", fields=("id",), box=far, every=3, phase=1)
    assert per_tile(last)[0] == 0 and per_tile(last)[-1] > 0
    ps.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def _upload_state(ps, state):
    ps.pid.from_numpy(state["pid"])                  # first: x_0 / color are keyed by the persistent id (as load_state does)
    for name in ps._STATE_FIELDS:
        if name != "pid":
            getattr(ps, name).from_numpy(state[name])


def test_order_independence():
    ps, solver = scenes.make_ps(scenes.crowded_fluid())
    solver.initialize()
    solver.step(5)
    before = _check(ps, tag="sorted order", fields=ALL).data.tobytes()
    state = {name: getattr(ps, name).to_numpy() for name in ps._STATE_FIELDS}
    n = state["pid"].shape[0]
    rng = np.random.default_rng(23)
    for k in range(2):
        perm = rng.permutation(n)
        _upload_state(ps, {name: a[perm] for name, a in state.items()})
        assert np.array_equal(ps.pid.to_numpy(), state["pid"][perm]) and np.array_equal(ps.x.to_numpy(), state["x"][perm])
        after = _check(ps, tag=f"permutation {k}", fields=ALL).data.tobytes()
        assert after == before, f"permutation {k}: the rows depend on the particle order"
        assert ps.export_particles(fields=ALL).data.tobytes() == before, "two calls on one state differ"
    ps.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_ids_that_are_not_creation_indices():
    ps, solver = scenes.make_ps(scenes.fluid_only())
    solver.initialize()
    solver.step(2)
    pid, x_0, color = ps.pid.to_numpy(), ps.x_0.to_numpy(), ps.color.to_numpy()
    n = pid.shape[0]
    relabel = np.random.default_rng(5).permutation(n).astype(np.int32)
    ps.pid.from_numpy(relabel[pid])
    ps.x_0.from_numpy(x_0)
    ps.color.from_numpy(color)
    f = _download(ps)
    assert np.array_equal(f["pid"], relabel[pid]) and not np.array_equal(f["pid"], pid)
    ex = _check(ps, f, "relabelled", fields=ALL)
    assert ex.data["id"].tolist() == list(range(n))
    holder = np.empty(n, dtype=np.int64)
    holder[relabel[pid]] = np.arange(n)                      # row r shows the record that now carries id r
    assert np.array_equal(ex.data["x"], f["x"][holder, 0])
    _check(ps, f, "relabelled, decimated", fields=("id",), every=7, phase=3)
    ps.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_duplicate_id_is_reported_and_refused():
    ps, solver = scenes.make_ps(scenes.fluid_only())
    solver.initialize()
    pid = ps.pid.to_numpy()
    n = pid.shape[0]
    twice = pid.copy()
    twice[n // 2] = twice[3]
    ps.pid.from_numpy(twice)
    args = export.select_args(fields=("id",))
    info = export.select_info(ps, export.make_params(args))
    assert (info.selected, info.rows, info.duplicate_ids, info.row_bytes) == (n, n - 1, 1, 16)
    assert _model(_download(ps), fields=("id",))["duplicate_ids"] == 1
    rows = np.empty(n - 1, dtype=export.row_dtype(("id",)))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*duplicate_ids = 1"):
        ps._call("sph_export_download", rows.ctypes.data_as(C.c_void_p), rows.nbytes)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*not unique"):
        ps.export_particles(fields=("id",))
    # a selection that leaves one of the two holders out is in order
    here = [float(v) for v in ps.x.to_numpy()[3]]
    lone = ps.export_particles(fields=("id",), box=(here, here))
    assert lone.count == lone.selected == 1 and lone.data["id"][0] == twice[3]
    ps.pid.from_numpy(pid)
    ex = _check(ps, tag="ids restored", fields=ALL)
    assert ex.count == n
    ps.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_does_not_disturb_the_run():
    sd = scenes.fluid_with_rigid_blocks()
    a, solver_a = scenes.make_ps(sd)
    b, solver_b = scenes.make_ps(sd)
    solver_a.initialize()
    solver_b.initialize()
    for k in range(4):
        solver_a.step(3)
        solver_b.step(3)
        ex = a.export_particles(fields=() if k % 2 == 0 else ALL)       # the second kind folds density / pressure back first
        assert ex.count == a.particle_max_num
    for name in STATE:
        fa, fb = scenes.ps_by_pid(a, name), scenes.ps_by_pid(b, name)
        assert fa.tobytes() == fb.tobytes(), f"{name} differs after exports between the steps"
    assert np.array_equal(a.pid.to_numpy(), b.pid.to_numpy()) and a.time == b.time
    a.close(); b.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_stable_vertices():
    ps, solver = scenes.make_ps(scenes.fluid_with_rigid_blocks())
    solver.initialize()
    solver.step(2)
    first = ps.export_particles(objects=[0], fields=("id",))
    solver.step(5)
    second = ps.export_particles(objects=[0], fields=("id",))
    assert first.count == second.count == ps.fluid_particle_num
    assert np.array_equal(first.data["id"], second.data["id"])
    assert not np.array_equal(first.data["y"], second.data["y"]) and second.time > first.time
    ps.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_dfsph():
    ps, solver = scenes.make_ps(scenes.as_dfsph(scenes.fluid_with_rigid_blocks()))
    solver.initialize()
    solver.step(2)
    f = _download(ps)
    assert _check(ps, f, "dfsph", fields=ALL).count == 1200
    _check(ps, f, "dfsph, fluid in a box", material="fluid", fields=("density", "pressure", "id"), box=([0.1, 0.1, 0.1], [0.25, 0.3, 0.2]))
    ps.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def _params(fields=1, material=-1, objects=(), n_objects=None, stride=1, phase=0, box=None):
    p = _lib.SphExportParams()
    p.fields, p.material, p.pid_stride, p.pid_phase = fields, material, stride, phase
    p.n_objects = len(objects) if n_objects is None else n_objects
    for k, oid in enumerate(objects):
        p.object_ids[k] = oid
    if box is not None:
        p.use_box = 1
        p.box_lo, p.box_hi = (C.c_float * 3)(*box[0]), (C.c_float * 3)(*box[1])
    return p


def test_refusals():
    sd = scenes.fluid_only(counts=(4, 4, 4))
    ps, solver = scenes.make_ps(sd)
    solver.initialize()
    rows = np.zeros(64, dtype=export.row_dtype(()))
    info = _lib.SphExportInfo()
    down = lambda nbytes: ps._call("sph_export_download", rows.ctypes.data_as(C.c_void_p), nbytes)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been selected"):
        down(rows.nbytes)
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been selected"):
        ps._call("sph_export_info", C.byref(info))
    nan, inf = float("nan"), float("inf")
    for bad, msg in ((dict(fields=0), "SPH_EXPORT_X"), (dict(fields=2 | 32), "SPH_EXPORT_X"), (dict(fields=1 | 128), "unknown bits"),
                     (dict(fields=-1), "unknown bits"), (dict(n_objects=33), "n_objects"), (dict(n_objects=-1), "n_objects"),
                     (dict(stride=0), "pid_stride"), (dict(stride=-3), "pid_stride"), (dict(stride=4, phase=4), "pid_phase"),
                     (dict(stride=4, phase=-1), "pid_phase"), (dict(box=([0.5, 0.0, 0.0], [0.25, 1.0, 1.0])), "box_lo"),
                     (dict(box=([0.0, 0.0, 0.0], [1.0, nan, 1.0])), "finite"), (dict(box=([0.0, 0.0, -inf], [1.0, 1.0, 1.0])), "finite")):
        with pytest.raises(_lib.SphError, match=rf"rc=-1.*{msg}"):
            ps._call("sph_export_select", C.byref(_params(**bad)))
    with pytest.raises(_lib.SphError, match=r"rc=-4.*nothing has been selected"):
        down(rows.nbytes)                                                   # a refused select leaves nothing to download
    ps._call("sph_export_select", C.byref(_params()))
    ps._call("sph_export_info", C.byref(info))
    assert (info.selected, info.rows, info.row_bytes, info.duplicate_ids) == (64, 64, 12, 0)
    for bad in (rows.nbytes - 4, rows.nbytes + 12, 0):
        with pytest.raises(_lib.SphError, match=r"rc=-1.*bytes"):
            down(bad)
    down(rows.nbytes)
    assert rows.tobytes() == _model(_download(ps), fields=())["data"].tobytes()
    ps._call("sph_export_select", C.byref(_params(objects=(5,))))          # nothing selected: zero bytes, no buffer needed
    ps._call("sph_export_download", None, 0)
    with pytest.raises(_lib.SphError, match=r"rc=-1.*pid_stride"):
        ps._call("sph_export_select", C.byref(_params(stride=0)))
    _check(ps, tag="after the refusals", fields=ALL, every=2, phase=1)      # rows of another size: the buffer grows
    ps.close()
    nx = int(scenes.build(sd)[1].geom.grid_num[0])
    slab = ParticleSystem(SimConfig(config=copy.deepcopy(sd)), slab=dict(x_lo=0, x_hi=nx, halo=1, capacity=2048))
    with pytest.raises(NotImplementedError, match="single-domain"):
        slab.export_particles()
    with pytest.raises(_lib.SphError, match=r"rc=-4.*single-domain"):
        slab._call("sph_export_select", C.byref(_params()))
    slab.close()


# ---- 11 -----------------------------------------------------------------------------------------------------------------
def _run(monkeypatch, capsys, tmp_path, name, sd, frames=3):
    from sph_taichi_amd import run_simulation
    scene_file = tmp_path / f"{name}.json"
    scene_file.write_text(json.dumps(sd))
    monkeypatch.chdir(tmp_path)
    capsys.readouterr()
    run_simulation.main(["--scene_file", str(scene_file), "--frames", str(frames), "--dump_npz", str(tmp_path / f"{name}.npz")])
    report = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")][-1]
    return report, np.load(tmp_path / f"{name}.npz")


def test_run_simulation_export_particles(tmp_path, monkeypatch, capsys):
    """27 particles in free fall, timeStepSize 0.016 so that every frame is an output interval (the lattice at rest spacing exerts
    no pressure, so the large step is harmless): 3 frames, 3 files."""
    sd = scenes.fluid_only(counts=(3, 3, 3), start=(0.3, 0.3, 0.3))
    sd["Configuration"]["timeStepSize"] = 0.016
    with_key = copy.deepcopy(sd)
    with_key["Configuration"]["exportParticles"] = {"fields": ["velocity", "id"]}
    report, state = _run(monkeypatch, capsys, tmp_path, "drop", with_key)
    out = tmp_path / "drop_output"
    assert sorted(p.name for p in out.iterdir()) == [f"particles_{k:06}.ply" for k in range(3)]
    assert report["particle_files_written"] == 3 and report["export_ms_per_file"] > 0
    files = [model.read_ply(out / f"particles_{k:06}.ply") for k in range(3)]
    for k, (data, comments, _) in enumerate(files):
        assert data.dtype == export.row_dtype(("velocity", "id")) and data.shape == (27,)
        assert data["id"].tolist() == list(range(27)) and f"frame {k}" in comments
    assert (files[2][0]["y"] < files[0][0]["y"]).all() and (files[2][0]["vy"] < files[0][0]["vy"]).all()      # it falls
    # the last file is the state the run ended in
    by_pid = np.empty_like(state["x"])
    by_pid[state["pid"]] = state["x"]
    assert np.array_equal(files[2][0]["x"], by_pid[:, 0]) and np.array_equal(files[2][0]["z"], by_pid[:, 2])
    plain, state_plain = _run(monkeypatch, capsys, tmp_path, "plain", sd)
    assert "particle_files_written" not in plain and "export_ms_per_file" not in plain
    assert not (tmp_path / "plain_output").exists()
    assert sorted(state.files) == sorted(state_plain.files)
    for name in state.files:
        assert state[name].tobytes() == state_plain[name].tobytes(), f"{name} differs between the run with exports and the run without"
