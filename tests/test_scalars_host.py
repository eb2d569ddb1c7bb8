"""Host side of the carried scalars (no GPU): the numpy model (tests/scalars_model.py) against a plain Python double loop, its exact
conservation and antisymmetry on an equal-volume set, the C ABI additions with their ctypes mirror against a host program compiled
with the header (under the address and undefined-behaviour sanitizers where the host compiler has them), the argument and scene-key
checks, the paint index against the field colouring's arithmetic, the caps of the GPU test's mixed scene, and the formula test's
measured error against its record."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sph_taichi_amd import _lib, build, scalars
from sph_taichi_amd.config_builder import SimConfig
from tests import fieldcolour_model
from tests import scalars_model as model
from tests import scenes

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
ENTRIES = ("sph_scalars_set", "sph_scalars_sample", "sph_scalars_info", "sph_scalars_download", "sph_scalars_paint")


def _cloud(n=60, seed=1, equal=False):
    """n particles in a 0.1 cube (h = 0.04: a dozen neighbours each), two coincident (r = 0 is refused), three roles."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.1, 0.2, size=(n, 3)).astype(F32)
    x[7] = x[3]
    m_V = np.full(n, F32(6.4e-6)) if equal else rng.uniform(4e-6, 9e-6, n).astype(F32)
    role = np.full(n, model.CARRIER) if equal else rng.choice([model.NONE, model.CARRIER, model.CARRIER, model.SOURCE], n)
    snap = model.to_raw(rng.uniform(-50.0, 50.0, size=(n, 2)))
    return x, m_V, role, snap


# ---- the model ------------------------------------------------------------------------------------------------------------
def test_model_equals_a_plain_double_loop():
    x, m_V, role, snap = _cloud()
    snap[5, 0], snap[9, 0] = 1 << 52, -(1 << 52)
    for a in ([2.0e-6, 0.0], [3.0e-3, 4.0e-4]):              # below the stability limit, and far beyond it (overshoot, saturation)
        got = model.sample(x, m_V, role, snap, a, F32(0.04))
        want = model.sample_loop(x, m_V, role, snap, a, F32(0.04))
        for g, w in zip(got, want):
            assert g.dtype == np.int64 and np.array_equal(g, w)
    assert np.array_equal(got[0][role != model.CARRIER], snap[role != model.CARRIER])                 # only carriers change
    assert got[1].any() and got[2].any() and (got[0] != snap).any()
    calm = model.sample(x, m_V, role, snap, [2.0e-6, 0.0], F32(0.04))
    assert not calm[1].any() and np.array_equal(calm[0][:, 1], snap[:, 1]) and (calm[0][:, 0] != snap[:, 0]).any()


def test_equal_volumes_conserve_the_sum_to_the_last_bit():
    x, m_V, role, snap = _cloud(equal=True)
    a = [3.0e-6, 1.0e-6]
    C = snap
    for _ in range(5):
        C, over, sat = model.sample(x, m_V, role, C, a, F32(0.04))
        assert not over.any() and not sat.any()
        assert np.array_equal(C.sum(axis=0), snap.sum(axis=0))
    assert (C != snap).any()
    # antisymmetry, pair by pair: term_ij = -term_ji
    accept, w = model.pair_weights(x, x, m_V, a, F32(0.04), model.k_dw(F32(0.04)))
    assert np.array_equal(accept, accept.T) and accept.sum() > 300 and not accept[3, 7]
    diff = (snap[None, :, 0] - snap[:, None, 0]).astype(np.float64)
    term = np.where(accept, np.rint(diff * w[0]).astype(np.int64), 0)
    assert np.array_equal(term, -term.T) and term.any()
    # ... and not with unequal volumes: conservation is a property of bit-equal m_V
    x2, m_V2, _, _ = _cloud(equal=False)
    C2 = model.sample(x, m_V2, role, snap, a, F32(0.04))[0]
    assert not np.array_equal(C2.sum(axis=0), snap.sum(axis=0))


def test_roles_and_snapshot():
    material = np.array([1, 1, 0, 1, 0, 1])
    obj = np.array([0, 2, 1, 4, 3, 0])
    role = model.roles(material, obj, 1, [0, 4], {1: (5.0,), 4: (7.0,)})
    assert role.tolist() == [model.CARRIER, model.NONE, model.SOURCE, model.SOURCE, model.NONE, model.CARRIER]    # a source wins over the selection
    assert model.roles(material, obj, -1, [], {}).tolist() == [model.CARRIER] * 6
    snap = model.snapshot(np.arange(6, dtype=np.int64)[:, None], role, obj, {1: (5.0,), 4: (7.0,)})
    assert snap[:, 0].tolist() == [0, 1, 5 << 32, 7 << 32, 4, 5]
    assert model.coefficients(F32(4e-4), 3, [F32(1e-3)]) == [(float(F32(4e-4)) * 3.0) * float(F32(1e-3))]


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    decls = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"int32_t\s+{name}\s*\(\s*SphContext\s*\*", decls), name
    assert re.search(r"#define\s+SPH_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    assert HEADER.index("Carried scalars (") > HEADER.index("Fluid loads (")                       # the last section
    section = HEADER[HEADER.index("Carried scalars ("):]
    for word in ("lap  = ((2.0 * (k_dw * g)) * r) / (h * (r * r + (0.01 * h) * h))", "q <= 1.0f and r > 1e-5f", "llrint(w_k * 2^32)", "-2^52, 2^52",
                 "steps_seen % every == 0", "overshoot[k]", "saturated[k]", "not part of a\n * checkpoint", "bit-equal m_V", "SNAPSHOT",
                 "idx = int(t * 255 + 0.5)", "keeps its\n * lean and fast sorts"):
        assert word in section, word


def test_binding():
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    want = {"sph_scalars_set": [vp, vp, i64, ctypes.POINTER(_lib.SphScalarParams)], "sph_scalars_sample": [vp],
            "sph_scalars_info": [vp, ctypes.POINTER(_lib.SphScalarInfo)], "sph_scalars_download": [vp, vp, vp, i64],
            "sph_scalars_paint": [vp, i32, f32, f32, vp]}
    for name, args in want.items():
        assert bound[name] == (i32, args), name
    assert "sph_scalars.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "sph_scalars.hip"))
    assert (_lib.SCALARS_MAX_CHANNELS, _lib.SCALARS_MAX_SOURCES, _lib.SCALARS_SCALE_LOG2) == (scalars.MAX_CHANNELS, scalars.MAX_SOURCES, scalars.SCALE_LOG2) == (4, 8, 32)


def test_struct_layouts_against_the_host_compiler(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "scalars_abi_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "scalars_abi_driver.cpp")]
    # The program is small and stands alone: a host compiler without the sanitizers' runtimes is an error of the machine, not a reason
    # to run unchecked.  SPH_TEST_NO_SANITIZERS=1 says so explicitly, and the test's output names the build that ran.
    sanitized = os.environ.get("SPH_TEST_NO_SANITIZERS") != "1"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    subprocess.run(cmd + flags, check=True)
    print("scalars_abi_driver built " + ("with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers (SPH_TEST_NO_SANITIZERS=1)"))
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = {line.split()[0]: line.split()[1:] for line in out.splitlines()}
    pairs = lambda words: {words[k]: int(words[k + 1]) for k in range(1, len(words), 2)}
    P, I = _lib.SphScalarParams, _lib.SphScalarInfo
    assert int(rows["SphScalarParams"][0]) == ctypes.sizeof(P) == 456
    assert pairs(rows["SphScalarParams"]) == {k: getattr(P, k).offset for k in ("K", "kappa", "every", "select", "n_sources", "source_object", "source_value")}
    assert int(rows["SphScalarInfo"][0]) == ctypes.sizeof(I) == 96
    assert pairs(rows["SphScalarInfo"]) == {k: getattr(I, k).offset for k in ("K", "every", "ids", "samples", "steps_seen", "overshoot", "saturated")}
    assert [int(rows[k][0]) for k in ("SPH_SCALARS_MAX_CHANNELS", "SPH_SCALARS_MAX_SOURCES", "SPH_SCALARS_SCALE_LOG2", "SPH_ABI_VERSION")] == [4, 8, 32, 6]
    assert rows["checksum"] == ["1328.0"]
    # the library's own parameter checks (csrc/sph_scalars_check.h), run by the driver: verdict and the word the message must hold
    verdicts = {}
    for line in out.splitlines():
        w = line.split(" ", 3)
        if w[0] in ("set", "paint"):
            verdicts[(w[0], w[1])] = (int(w[2]), w[3] if len(w) > 3 else "")
    want = {("set", "good"): None, ("set", "good_null_values"): None, ("set", "good_at_the_limit"): None, ("set", "K_5"): "K = 5", ("set", "K_negative"): "K = -1",
            ("set", "K_huge"): "K = ", ("set", "every_0"): "every", ("set", "n_sources_9"): "n_sources = 9", ("set", "n_sources_huge"): "n_sources",
            ("set", "n_sources_negative"): "n_sources = -1", ("set", "kappa_negative"): "kappa[1]", ("set", "kappa_nan"): "kappa[0]", ("set", "kappa_inf"): "kappa[0]",
            ("set", "kappa_beyond_K_is_not_read"): None, ("set", "source_outside"): "source object 3", ("set", "source_negative"): "source object -1",
            ("set", "source_twice"): "named twice", ("set", "source_beyond_n_is_not_read"): None, ("set", "source_value_inf"): "source_value[1][0]",
            ("set", "source_value_large"): "source_value[0][1]", ("set", "material_256"): "material = 256", ("set", "select_33"): "n_objects = 33",
            ("set", "select_negative"): "n_objects = -1", ("set", "n_ids_0"): "n_ids = 0", ("set", "n_ids_negative"): "n_ids = -4",
            ("set", "n_ids_above_cold"): "n_ids = 9", ("set", "value_nan_last"): "values[7][1]", ("set", "value_large_first"): "values[0][0]",
            ("paint", "good"): None, ("paint", "channel_2"): "channel = 2", ("paint", "channel_negative"): "channel = -1", ("paint", "lo_equals_hi"): "smaller",
            ("paint", "hi_nan"): "finite", ("paint", "lo_inf"): "finite", ("paint", "too_narrow"): "too narrow", ("paint", "too_wide"): "too narrow or too wide",
            ("paint", "null_table"): "NULL", ("paint", "entry_256_last"): "outside [0, 255]", ("paint", "entry_negative_first"): "outside [0, 255]"}
    assert verdicts.keys() == want.keys()
    for key, word in want.items():
        rc, msg = verdicts[key]
        assert (rc, msg) == (0, "") if word is None else (rc == -1 and word in msg and msg.startswith("sph_scalars_" + key[0])), (key, rc, msg)


# ---- arguments and the scene key ------------------------------------------------------------------------------------------
def test_argument_checks():
    a = scalars.set_args()
    assert a == {"channels": ["dye"], "diffusivity": (float(F32(1e-4)),), "values": None, "sources": {}, "every": 1, "material": 1, "objects": []}
    a = scalars.set_args(channels=("heat", "dye"), diffusivity=(1e-3, 0), values={0: (20, 0), "2": [30.5, 1]}, sources={1: (350, 0)}, every=10,
                         material=None, objects=[0, 2])
    assert a["values"] == {0: (20.0, 0.0), 2: (30.5, 1.0)} and a["sources"] == {1: (350.0, 0.0)} and a["material"] == -1 and a["objects"] == [0, 2]
    assert scalars.set_args(values=np.arange(5.0))["values"].shape == (5, 1)
    assert scalars.set_args(channels="t", values=[[2.0 ** 20], [-2.0 ** 20]])["values"].shape == (2, 1)
    p = scalars.scalar_params(a)
    assert p.K == 2 and list(p.kappa) == [F32(1e-3), 0, 0, 0] and p.every == 10 and p.select.material == -1 and p.select.n_objects == 2
    assert p.n_sources == 1 and p.source_object[0] == 1 and list(p.source_value[0]) == [350.0, 0.0, 0.0, 0.0]
    for kw in ({"channels": ()}, {"channels": ("a", "b", "c", "d", "e")}, {"channels": ("a", "a"), "diffusivity": (0, 0)}, {"channels": (1,)},
               {"channels": ("",)}, {"channels": 3}, {"diffusivity": (1e-4, 1e-4)}, {"diffusivity": (-1e-4,)}, {"diffusivity": (float("nan"),)},
               {"diffusivity": (1e39,)}, {"diffusivity": "x"}, {"every": 0}, {"every": 1.5}, {"every": True}, {"material": "gas"},
               {"objects": []}, {"objects": [-1]}, {"objects": list(range(33))}, {"sources": [1]}, {"sources": {1: (1, 2)}},
               {"sources": {1: (float("inf"),)}}, {"sources": {1: (2.0 ** 20 + 1,)}}, {"sources": {-1: (0,)}}, {"sources": {"a": (0,)}},
               {"sources": {1: (0,), "1": (0,)}}, {"sources": {k: (0,) for k in range(9)}}, {"values": {0: (1, 2)}}, {"values": {0: (float("nan"),)}},
               {"values": np.zeros((3, 2))}, {"values": np.zeros((0, 1))}, {"values": [[2.0 ** 21]]}, {"values": [[float("nan")]]}, {"values": "x"}):
        with pytest.raises(ValueError):
            scalars.set_args(**kw)
    # the host expansion of {object id: row}: values first, then the sources' rows over their objects
    init = scalars.expand({0: (1.0, 2.0), 2: (3.0, 4.0)}, {1: (9.0, 8.0)}, np.array([0, 1, 2, 0, 5]), 2)
    assert init.tolist() == [[1.0, 2.0], [9.0, 8.0], [3.0, 4.0], [1.0, 2.0], [0.0, 0.0]]
    with pytest.raises(ValueError, match="rows"):
        scalars.expand(np.zeros((4, 2)), {}, np.zeros(5, int), 2)
    for kw in ({"channel": 2}, {"channel": "x"}, {"channel": 0.5}, {"range": (1, 1)}, {"range": (0, float("nan"))}, {"colormap": "nope"},
               {"colormap": np.zeros((256, 3), np.int32)}, {"tint": 1}):
        with pytest.raises(ValueError):
            scalars.check_paint(kw, ["a", "b"])
    assert scalars.check_paint({"channel": "b", "range": [0, 2]}, ["a", "b"])["channel"] == 1


def _config(**keys):
    sd = scenes.fluid_only(counts=(3, 3, 3))
    sd["Configuration"].update(keys)
    return SimConfig(config=sd)


def test_scene_key_and_command_line_flag():
    assert scalars.scalars_config(_config()) is None
    kw, paint = scalars.scalars_config(_config(scalars={}))
    assert paint is None and scalars.set_args(**kw) == scalars.set_args()
    kw, paint = scalars.scalars_config(_config(scalars={"channels": ["heat"], "diffusivity": [1e-3], "values": {"0": [20]}, "sources": {"1": [350]},
                                                        "every": 10, "paint": {"channel": "heat", "range": [20, 350], "colormap": "coolwarm"}}))
    assert scalars.set_args(**kw)["sources"] == {1: (350.0,)} and paint["channel"] == 0 and paint["range"] == (20.0, 350.0) and paint["lut"].shape == (256, 3)
    for bad in ([1], {"channel": ["a"]}, {"every": 0}, {"values": [[1.0]]}, {"sources": {"1": [1, 2]}}, {"paint": {"channel": 3}}, {"paint": [0]},
                {"paint": {"range": [1, 0]}}, {"diffusivity": [-1]}):
        with pytest.raises(ValueError, match="scalars"):
            scalars.scalars_config(_config(scalars=bad))
    from sph_taichi_amd import run_simulation
    args = run_simulation.build_parser().parse_args(["--scene_file", "x.json", "--scalars", "out"])
    assert args.scalars == "out"


def test_slab_rank_is_refused():
    class Slab:
        slab = {"x_lo": 0}

        def _call(self, *a):
            raise AssertionError("the library must not be reached")
    with pytest.raises(NotImplementedError, match="single-domain contexts only"):
        scalars.set_scalars(Slab())
    with pytest.raises(NotImplementedError, match="single-domain"):
        scalars.clear_scalars(Slab())
    with pytest.raises(ValueError):                                   # the arguments are checked first, as for the other observers
        scalars.set_scalars(Slab(), every=0)


# ---- the paint index ------------------------------------------------------------------------------------------------------
def test_paint_index_is_the_field_colourings():
    rng = np.random.default_rng(2)
    raw = np.concatenate([model.to_raw(rng.uniform(-3.0, 12.0, 2000)), [0, 1 << 52, -(1 << 52), 5 << 32, (10 << 32) - 1, (10 << 32) + 1]]).astype(np.int64)
    s = (raw.astype(np.float64) / model.ONE).astype(F32)
    for lo, hi in ((0.0, 10.0), (-1.5, 0.25), (5.0, 5.0 + 1e-3)):
        idx = model.paint_index(raw, lo, hi)
        assert np.array_equal(idx, fieldcolour_model.index(s, lo, hi)) and idx.min() == 0 and idx.max() == 255


# ---- the mixed scene of the GPU test stays inside its own caps ----------------------------------------------------------------
def test_mixed_scene_caps():
    sd, a, values, crowd = model.mixed_scene()
    h, dt = F32(0.04), sd["Configuration"]["timeStepSize"]
    role = model.roles(a["material"], a["object_id"], 1, [0], model.MIXED_SOURCES)
    n_car = int((role == model.CARRIER).sum())
    assert n_car % 4 and n_car % 16 and n_car > 1500 and (role == model.SOURCE).sum() > 500 and (role == model.NONE).sum() == 108
    kappa, planted = model.mixed_kappa(a, values, crowd, h, dt)
    values[planted, 2] = -model.VALUE_MAX
    snap = model.snapshot(model.to_raw(values), role, a["object_id"], model.MIXED_SOURCES)
    new, over, sat, pairs, lo, hi, wsum = model.sample(a["x"], a["m_V"], role, snap, model.coefficients(dt, 1, [kappa, 0.0, F32(10) * kappa]), h, detail=True)
    assert over.tolist() == [0, 0, 250] and sat.tolist() == [0, 0, 1]            # overshoot in the channel meant to, saturation of the planted value
    assert abs(new[planted, 2]) == 1 << 52 and np.array_equal(new[:, 1], snap[:, 1])
    n = np.array([25, 30, 20])
    cells = np.clip((a["x"] / F32(0.04)).astype(np.int64), 0, n - 1)
    occ = np.bincount(np.ravel_multi_index(cells.T, n), minlength=n.prod())
    assert occ.max() == 250 and occ[0] >= 4 and occ[-1] >= 4                       # the crowded cell, both corner cells
    assert (a["x"] < 0).any() and (a["x"] > np.array([1.0, 1.2, 0.8], F32)).any()  # outside the domain, clamped into border cells
    assert pairs[crowd].max() > 200 and pairs[role == model.CARRIER].min() >= 0


# ---- the formula, on the CPU ------------------------------------------------------------------------------------------------
def test_mode_decay_matches_its_record():
    rec = json.load(open(os.path.join(ROOT, "profiles", "scalars_parity.json")))
    err, _, _ = model.mode_decay()
    assert err == pytest.approx(rec["rate_error_measured"], rel=1e-9) and rec["bound"] == pytest.approx(3 * rec["rate_error_measured"])
    assert err < 0.10 and err <= rec["bound"]
