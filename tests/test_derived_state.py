"""The validity rules of the context's derived device buffers (csrc/sph_derived.h), executed on the CPU: the header is
host-only, so tests/derived_state_driver.cpp is compiled against it with the host C++ compiler and runs event sequences
in the order the launch code issues them.  Plus two source-level checks: the header is the only owner of the fields, and
the API entries that must drop everything do report the event."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sph_taichi_amd", "csrc")
FIELDS = ("lists_valid|bricks_valid|bricks_key|brec_valid|brec_key|stg_kind|k_kind|gcnt_written|df_bpart_valid|aux_stale|"
          "brick_count_zero")
SCENARIOS = [
    "wcsph_fused_step",      # sort (list built), density writes lists + records, force reader gets lists, records, one gather
    "dfsph_step",            # one writer, many readers, k_kind 0 -> 1 -> 0 -> 2
    "advect_after_density",  # readers get "no lists", stats still report the lengths
    "slab_order",            # writer over [lo, hi), readers over sub-ranges: subset, lists yes, records no
    "foreign_rebuild",       # writer under K, non-list sweep rebuilds under K' > K, reader under K: subset, no lists, no records
    "everything_dropped",    # option changes and the scan's error flag
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("derived") / "derived_state_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "derived_state_driver.cpp")], check=True)
    return exe


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_derived_state_rules(driver, scenario):
    r = subprocess.run([driver, scenario], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("PASS"), r.stdout + r.stderr


def test_derived_state_has_one_owner():
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name == "sph_derived.h":
            continue
        with open(os.path.join(CSRC, name)) as fh:
            for no, line in enumerate(fh, 1):
                if re.search(FIELDS, line) or "memcmp(key" in line:
                    hits.append(f"{name}:{no}: {line.strip()}")
    assert not hits, "\n".join(hits)
    with open(os.path.join(CSRC, "sph_derived.h")) as fh:
        assert "#include" not in fh.read()          # host only: nothing of HIP, nothing at all


def test_api_entries_that_drop_everything_say_so():
    with open(os.path.join(CSRC, "sph_api.hip")) as fh:
        src = fh.read()
    body = src[src.index("int32_t sph_set_option("):]
    body = body[:body.index("unknown option")]
    cases = re.split(r"\n\s*case ", body)
    for opt in ("SPH_OPT_BRICK_SHAPE", "SPH_OPT_KERNEL_VARIANT", "SPH_OPT_EXACT_MATH", "SPH_OPT_BRICK_RECORDS",
                "SPH_OPT_PURE_FLUID_INSTANCE"):
        mine = [c for c in cases if c.startswith(opt + ":")]
        assert len(mine) == 1 and "sph_invalidate_lists(c)" in mine[0], opt
    flags = src[src.index("int sph_check_device_flags("):]
    assert "sph_invalidate_lists(c)" in flags[:flags.index("\n}\n")]
    with open(os.path.join(CSRC, "sph_internal.h")) as fh:
        assert re.search(r"sph_invalidate_lists\(SphContext\* c\) \{ sphd_invalidate\(c->dv\); \}", fh.read())
