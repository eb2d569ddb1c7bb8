"""Where the persistent id lives (csrc/sph_derived.h: the lean scatter of SPH_OPT_SORT_LEAN moves it through an array of its
own and leaves aux behind until somebody asks), executed on the CPU: the header is host-only, so tests/sort_lean_driver.cpp is
compiled against it and sph_setstate.h with the host C++ compiler and runs the call orders of the launch code on plain arrays.
Plus the source-level check that the header is the only owner of the new field."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sph_taichi_amd", "csrc")
SCENARIOS = [
    "enter",                  # general sort, verdict, lean sorts: ids from aux.w once, then from the pid array; one fold on demand
    "fold",                   # the fold writes the whole record once; the conditions that keep the scatter general
    "re_enter",               # fold, lean again through aux.w; a stand-alone sort in between
    "set_change_while_lean",  # truncate / new count / the switch turned off while the ids live apart
    "upload_while_lean",      # an upload of m is honoured; the uniform check folds before it forgets the mass
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sort_lean") / "sort_lean_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "sort_lean_driver.cpp")], check=True)
    return exe


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_pid_location_rules(driver, scenario):
    r = subprocess.run([driver, scenario], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("PASS"), r.stdout + r.stderr


def test_pid_location_has_one_owner():
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name == "sph_derived.h":
            continue
        with open(os.path.join(CSRC, name)) as fh:
            for no, line in enumerate(fh, 1):
                if re.search(r"\bpid_apart\b", line):
                    hits.append(f"{name}:{no}: {line.strip()}")
    assert not hits, "\n".join(hits)
    with open(os.path.join(CSRC, "sph_derived.h")) as fh:
        src = fh.read()
    assert "#include" not in src and re.search(r"\bbool pid_apart;", src)


def test_every_scatter_that_moves_aux_asks_for_the_fold_first():
    """sphk_sort_scatter is the one launcher of all four scatters: unless the scatter is the lean one it asks for the ids
    back before it builds its view; and the fold's demand function is the header's question, nothing of its own."""
    with open(os.path.join(CSRC, "sph_sort.hip")) as fh:
        src = fh.read()
    body = src[src.index("int sphk_sort_scatter("):]
    assert body.index("if (!lean) { int rc0 = sph_ensure_pid(c);") < body.index("DevView d = sph_view(c);")
    with open(os.path.join(CSRC, "sph_internal.h")) as fh:
        assert "static inline int sph_ensure_pid(SphContext* c) { return sphd_pid_apart(c->dv) ? sph_ensure_aux(c) : 0; }" in fh.read()
