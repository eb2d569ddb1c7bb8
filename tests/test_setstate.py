"""What the host knows about the particle set and the stage of the sort pipeline (csrc/sph_setstate.h), executed on the
CPU: the header is host-only, so tests/setstate_driver.cpp is compiled against it with the host C++ compiler and runs event
sequences in the order the API entry points issue them.  Plus a source-level check: the header is the only owner of the
fields."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sph_taichi_amd", "csrc")
# nine of the ten names are looked for as words wherever they stand, comments included; `sorted` is an English word the
# kernels' comments use for the record order ("cell-sorted"), so it is looked for as what only a field can be: a member access
FIELDS = (r"\b(have_keys|have_prefix|n_dyn_host|obj_info_valid|uniform_state|m_uniform|pure_fluid|pure_fluid_n|acc_partial)\b"
          r"|(->|\.)\s*sorted\b")
SCENARIOS = [
    "stand_alone_sort",                  # hash -> scan -> scatter, each refused out of order
    "step_then_truncate_append_same_n",  # the pure verdict is gone although N is restored; the dynamic count unless vouched
    "append_vouched",                    # opt_uniform 1: the uniform verdict survives, the pure one does not
    "select_range",                      # drops the order, keeps the object info
    "count_set",                         # the mirror image
    "upload_table",                      # each uploadable field -> exactly its consequences
    "window_change",
    "device_error",
    "slab_forces_fused",                 # acceleration incomplete until a full force pass, a step or an upload of it
    "uniform_check",                     # N = 0, mixed masses, uniform with solids, pure; the four options
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("setstate") / "setstate_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "setstate_driver.cpp")], check=True)
    return exe


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_setstate_rules(driver, scenario):
    r = subprocess.run([driver, scenario], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("PASS"), r.stdout + r.stderr


def test_setstate_has_one_owner():
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name == "sph_setstate.h":
            continue
        with open(os.path.join(CSRC, name)) as fh:
            for no, line in enumerate(fh, 1):
                if re.search(FIELDS, line):
                    hits.append(f"{name}:{no}: {line.strip()}")
    assert not hits, "\n".join(hits)
    with open(os.path.join(CSRC, "sph_setstate.h")) as fh:
        assert "#include" not in fh.read()          # host only: nothing of HIP, nothing at all
