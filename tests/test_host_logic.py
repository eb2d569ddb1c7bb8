"""CPU-side checks: scene ingestion, config semantics, and that libsph_hip.so
loads and exports every symbol include/sph_hip.h declares (no compute calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

import scenes
from sph_taichi_amd import _lib, scene as scene_mod
from sph_taichi_amd.config_builder import SimConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_simconfig_semantics(tmp_path):
    import json
    p = tmp_path / "s.json"
    p.write_text(json.dumps(scenes.fluid_only()))
    cfg = SimConfig(scene_file_path=str(p))
    assert cfg.get_cfg("particleRadius") == 0.01
    assert cfg.get_cfg("noSuchKey") is None                      # config_builder.py:15-18
    with pytest.raises(AssertionError):
        cfg.get_cfg("noSuchKey", enforce_exist=True)            # config_builder.py:12-13
    assert cfg.get_rigid_bodies() == [] and cfg.get_rigid_blocks() == []
    assert len(cfg.get_fluid_blocks()) == 1


def test_scene_counts_match_reference_formulas():
    # dragon fluid block 55*140*55, armadillo block 246*73*96; grid (125,75,50)
    d = 0.02
    assert scene_mod.compute_cube_particle_num([0.1, 0.1, 0.5], [1.2, 2.9, 1.6], d) == 55 * 140 * 55
    assert scene_mod.compute_cube_particle_num([0.04, 0.04, 0.04], [4.96, 1.50, 1.96], d) == 246 * 73 * 96
    cfg, sc = scenes.build(scenes.fluid_only(counts=(3, 4, 5), domain_end=(5.0, 3.0, 2.0)))
    assert list(sc.geom.grid_num) == [125, 75, 50]
    a = sc.arrays
    assert a["x"].shape == (60, 3) and a["x"].dtype == np.float32
    # z fastest lattice (particle_system.py:478-483)
    assert np.allclose(a["x"][1] - a["x"][0], [0, 0, 0.02], atol=1e-7)
    assert np.all(a["m_V"] == np.float32(0.8 * d ** 3)) and np.allclose(a["m"], 6.4e-3, rtol=1e-6)
    assert np.all(a["material"] == 1) and np.all(a["is_dynamic"] == 1) and np.array_equal(a["x"], a["x_0"])


def test_rigid_blocks_and_bookkeeping():
    cfg, sc = scenes.build(scenes.fluid_with_rigid_blocks())
    assert sc.particle_max_num == sc.fluid_particle_num + sc.solid_particle_num == 1200
    assert sc.num_rigid_bodies == 2 and sc.n_objects == 3
    assert sc.object_id_rigid_body == set()          # blocks are not shape-matched (particle_system.py:171-188)
    a = sc.arrays
    assert set(np.unique(a["object_id"])) == {0, 1, 2}
    assert np.all(a["is_dynamic"][a["object_id"] == 1] == 0) and np.all(a["is_dynamic"][a["object_id"] == 2] == 1)
    assert np.all(a["density"][a["object_id"] == 2] == 800.0)


def test_voxelizer_cube(tmp_path):
    from sph_taichi_amd import voxelizer
    obj = tmp_path / "cube.obj"
    v = [(x, y, z) for x in (0, 0.1) for y in (0, 0.1) for z in (0, 0.1)]
    f = [(1, 2, 4), (1, 4, 3), (5, 8, 6), (5, 7, 8), (1, 6, 2), (1, 5, 6), (3, 4, 8), (3, 8, 7), (1, 3, 7), (1, 7, 5),
         (2, 6, 8), (2, 8, 4)]
    obj.write_text("".join(f"v {a} {b} {c}\n" for a, b, c in v) + "".join(f"f {a} {b} {c}\n" for a, b, c in f))
    body = {"geometryFile": str(obj), "scale": [1, 1, 1], "translation": [0.5, 0.5, 0.5], "rotationAxis": [0, 1, 0],
            "rotationAngle": 0}
    pts, mesh = voxelizer.load_rigid_body(body, 0.02)
    assert pts.shape == (216, 3)                                  # 6^3 lattice points incl. the filled interior
    assert np.allclose(pts.min(axis=0), 0.5) and np.allclose(pts.max(axis=0), 0.6)
    assert np.allclose(np.round(pts / 0.02) * 0.02, pts)          # centres on the world lattice k*d
    body["rotationAngle"] = 90
    pts90, _ = voxelizer.load_rigid_body(body, 0.02)
    assert pts90.shape[0] == 216


def test_library_exports_every_header_symbol():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    declared = set(re.findall(r"\b(sph_[a-z0-9_A-Z]+)\s*\(", header))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    assert declared == bound, f"binding/header mismatch: {declared ^ bound}"
    lib = _lib.load()                                             # builds with hipcc if needed; dlopen
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.sph_abi_version() == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.SphParams) == 4 * (2 + 3 + 3 + 2 + 10 + 3 + 3 + 1 + 3 + 4)


def test_product_fails_loudly_without_gpu():
    lib = _lib.load()
    if lib.sph_device_count() > 0:
        pytest.skip("a GPU is visible here")
    from sph_taichi_amd import ParticleSystem
    with pytest.raises(_lib.SphError, match="no HIP device"):
        ParticleSystem(SimConfig(config=scenes.fluid_only(counts=(2, 2, 2))))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "sph_taichi_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, fn)).read()
                assert "oracle" not in src.lower().replace("# oracle", ""), f"{fn} mentions the oracle"


def test_exporters_and_mesh_roundtrip(tmp_path):
    """run_simulation.py:96-113 counterparts: ASCII PLY series file and the OBJ export of a rigid body's mesh."""
    from sph_taichi_amd.run_simulation import write_ply_ascii
    from sph_taichi_amd import voxelizer
    pos = np.random.default_rng(0).uniform(0, 1, size=(17, 3)).astype(np.float32)
    ply = str(tmp_path / "p.ply")
    write_ply_ascii(ply, pos)
    lines = open(ply).read().splitlines()
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0" and "element vertex 17" in lines
    body = np.loadtxt(lines[lines.index("end_header") + 1:], dtype=np.float32)
    assert body.shape == (17, 3) and np.allclose(body, pos, atol=1e-6)
    obj = str(tmp_path / "cube.obj")
    scenes.write_cube_obj(obj, (0.1, 0.2, 0.3), 0.5)
    m = voxelizer.load_mesh(obj)
    assert m.vertices.shape == (8, 3) and m.faces.shape == (12, 3)
    open(str(tmp_path / "again.obj"), "w").write(m.export(file_type="obj"))
    m2 = voxelizer.load_mesh(str(tmp_path / "again.obj"))
    assert np.allclose(m2.vertices, m.vertices) and np.array_equal(m2.faces, m.faces)


def test_reference_scene_files_parse_with_expected_counts():
    """Every scene JSON of the reference parses; fluid particle counts follow particle_system.py:450-456.  The scene
    files are stored unchanged under tests/golden/reference_data/scenes/."""
    import glob
    from sph_taichi_amd.config_builder import SimConfig
    from sph_taichi_amd import scene as scene_mod
    expect = {"dragon_bath.json": 423500, "armadillo_bath_dynamic.json": 1723968}
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data", "scenes", "*.json")))
    assert len(files) == 7
    for f in files:
        cfg = SimConfig(scene_file_path=f)
        assert cfg.get_cfg("simulationMethod") in (0, 4) and cfg.get_cfg("missing-key") is None
        g = scene_mod.Geometry(cfg)
        n = sum(scene_mod.compute_cube_particle_num(np.array(b["start"]) + np.array(b["translation"]),
                                                    np.array(b["end"]) + np.array(b["translation"]), g.particle_diameter)
                for b in cfg.get_fluid_blocks())
        if os.path.basename(f) in expect:
            assert n == expect[os.path.basename(f)], (f, n)


def test_layer_histogram_counts_bodies_and_cuts_balance(tmp_path):
    """scene.x_layer_histogram / slab_cuts with RigidBodies: the histogram equals the per-layer particle counts of the
    built scene, and the cut planes split the particles evenly while respecting the minimum slab width."""
    sd = scenes.fluid_with_rigid_bodies(str(tmp_path / "cube.obj"))
    cfg, sc = scenes.build(sd)
    hist = scene_mod.x_layer_histogram(SimConfig(config=sd))
    nx = int(sc.geom.grid_num[0])
    layers = scene_mod.x_layer_of(sc.arrays["x"][:, 0], sc.geom.grid_size, nx)
    assert np.array_equal(hist, np.bincount(layers, minlength=nx))
    for world, width in ((2, 3), (3, 4)):
        cuts = scene_mod.slab_cuts(hist, world, min_width=width)
        assert cuts[0] == 0 and cuts[-1] == nx and all(b - a >= width for a, b in zip(cuts, cuts[1:]))
    with pytest.raises(ValueError):
        scene_mod.slab_cuts(hist, 9, min_width=4)            # 9 slabs of >= 4 layers do not fit 25 layers


def test_library_build_stamp_tracks_contents_not_times():
    """build.stale() compares a content hash (a snapshot copied to another box keeps contents, not mtimes)."""
    from sph_taichi_amd import build
    build.build()                                            # make sure library + stamp exist
    assert not build.stale()
    src = os.path.join(build.CSRC, build.SOURCES[0])
    os.utime(src, None)                                      # newer mtime, same bytes
    assert not build.stale()
    stamp = open(build.STAMP).read()
    try:
        open(build.STAMP, "w").write("0" * 64 + "\n")       # a different fingerprint => stale
        assert build.stale()
    finally:
        open(build.STAMP, "w").write(stamp)
    assert not build.stale()


def test_usable_cpus_honours_affinity_and_cgroup_quota(tmp_path, monkeypatch):
    """oracle.usable_cpus(): what the CPU baseline and the deep parity cases size their OpenMP teams with.  The GPU
    boxes report 256 CPUs and grant 16 through cpu.max; 128 threads there run the oracle 3.6 x slower than 16."""
    import builtins
    import os
    from oracle import oracle as orc
    n = orc.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1) and orc.max_threads() == n
    real_open = builtins.open

    def fake_open(path, *a, **k):
        if path == "/sys/fs/cgroup/cpu.max":
            p = tmp_path / "cpu.max"
            p.write_text("250000 100000\n")
            return real_open(p, *a, **k)
        return real_open(path, *a, **k)

    monkeypatch.setattr(builtins, "open", fake_open)
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(64)), raising=False)
    assert orc.usable_cpus() == 3          # ceil(2.5)


def test_pmc_file_is_quoted_only_for_its_own_kernel_fingerprint():
    """bench.py's counter-derived figures come from profiles/pmc_traffic.json, which must carry the fingerprint of
    the kernel sources it was measured on (VERDICT r01 'weak' #4); the committed file matches the committed sources."""
    import json
    import os
    from sph_taichi_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pm = json.load(open(os.path.join(root, "profiles", "pmc_traffic.json")))
    assert "kernel_fingerprint" in pm and len(pm["kernel_fingerprint"]) == 64
    if pm["kernel_fingerprint"] != build._fingerprint():
        # a kernel edit without a new PMC pass: bench.py then reports traffic / VALU figures as null (checked below)
        import pytest
        import bench  # noqa: F401  (importable without a GPU)
        pytest.skip("profiles/pmc_traffic.json is older than the kernel sources: bench.py quotes no counter figures "
                    "until tools/gpu_pmc.sh + tools/refresh_pmc.py are re-run on the GPU box")
    k = pm["kernels"]["k_gather_brick<GM_DENSITY_EOS>"]
    assert k["valu_wave_insts"] > 0 and k["fetch_kb"] > 0 and k["write_kb"] > 0


def test_restart_state_is_cut_like_the_scene():
    """A restart (`state` = positions / velocities by persistent id, e.g. gather_by_pid of an earlier slab run): every
    slab keeps the particles whose RESTART position lies in its layers, with the scene file's identity (object, material,
    mass, x_0 = rest position); the slabs partition the scene; the cut-planning histogram counts the restart positions."""
    import copy
    from sph_taichi_amd import scene as S
    from sph_taichi_amd.config_builder import SimConfig
    sd = scenes.fluid_with_rigid_blocks()
    full = S.build_scene(SimConfig(config=copy.deepcopy(sd)))
    n = full.particle_max_num
    rng = np.random.default_rng(0)
    x = full.arrays["x"] + rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    v = rng.normal(size=(n, 3)).astype(np.float32)
    g = full.geom
    nx = int(g.grid_num[0])
    seen = []
    for lo, hi in ((0, 10), (10, 18), (18, nx)):
        f = lambda xs, lo=lo, hi=hi: (S.x_layer_of(xs, g.grid_size, nx) >= lo) & (S.x_layer_of(xs, g.grid_size, nx) < hi)
        sc = S.build_scene(SimConfig(config=copy.deepcopy(sd)), x_filter=f, state={"x": x, "v": v})
        pid = sc.arrays["pid"]
        assert np.array_equal(sc.arrays["x"], x[pid]) and np.array_equal(sc.arrays["v"], v[pid])
        assert np.array_equal(sc.arrays["x_0"], full.arrays["x_0"][pid])
        for k in ("object_id", "material", "is_dynamic", "m", "density", "color"):
            assert np.array_equal(sc.arrays[k], full.arrays[k][pid]), k
        seen.append(pid)
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(n))
    hist = S.x_layer_histogram(SimConfig(config=copy.deepcopy(sd)), state={"x": x, "v": v})
    assert hist.sum() == n and np.array_equal(hist, np.bincount(S.x_layer_of(x[:, 0], g.grid_size, nx), minlength=nx))
    whole = S.build_scene(SimConfig(config=copy.deepcopy(sd)), state={"x": x, "v": v})
    assert np.array_equal(whole.arrays["x"], x) and np.array_equal(whole.arrays["x_0"], full.arrays["x_0"])
    with pytest.raises(ValueError, match="restart state"):
        S.build_scene(SimConfig(config=copy.deepcopy(sd)), state={"x": x[:-1], "v": v[:-1]})
