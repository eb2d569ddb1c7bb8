"""Host side of the particle selection (no GPU, no library): one table of `material` / `objects` inputs through every parser that
takes them, the one struct filler into the three ctypes structs, and the three limits of include/sph_hip.h against the one here."""
import os
import re

import numpy as np
import pytest

from sph_taichi_amd import _lib, export, render, sample, selection, tracers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()

# (material, objects) and the (mat, ids) they mean
VALID = [
    ((None, None), (-1, [])), (("fluid", None), (1, [])), (("solid", None), (0, [])),
    ((0, None), (0, [])), ((255, None), (255, [])), ((np.int32(7), None), (7, [])),
    (("fluid", 3), (1, [3])), ((None, [2, 0]), (-1, [2, 0])), (("fluid", list(range(32))), (1, list(range(32)))),
    (("fluid", np.int64(5)), (1, [5])), ((None, np.array([1, 2], np.int32)), (-1, [1, 2])), (("solid", (4, 4)), (0, [4, 4])),
]
INVALID = [
    (256, None), (-1, None), ("gas", None), (True, None), (1.5, None), ([1], None),
    ("fluid", []), ("fluid", list(range(33))), ("fluid", [-1]), ("fluid", [1.5]), ("fluid", True), ("fluid", [True]),
    (None, np.True_), (None, 1.5), (None, ["0"]),
]


def _sample(**kw):
    a = sample.select_args(fields=(), **kw)
    return a["material"], a["objects"]


def _export(**kw):
    a = export.select_args(**kw)
    return a["material"], a["objects"]


def _tracers(**kw):
    a = tracers.set_args([0.5, 0.5, 0.5], **kw)
    return a["material"], a["objects"]


def _colour(**kw):
    p = render.field_colour_params(render.FieldColour("speed", **kw))
    return p.material, list(p.object_ids[:p.n_objects])


PARSERS = {"sample": _sample, "export": _export, "tracers": _tracers, "FieldColour": _colour}


@pytest.mark.parametrize("given, want", VALID, ids=[repr(g) for g, _ in VALID])
def test_every_parser_means_the_same(given, want):
    material, objects = given
    assert selection.parse(material, objects) == want
    for name, parse in PARSERS.items():
        if name == "FieldColour" and isinstance(material, (int, np.integer)):
            with pytest.raises(ValueError, match="material"):         # the documented exception: names only
                parse(material=material, objects=objects)
            continue
        mat, ids = parse(material=material, objects=objects)
        assert (mat, ids) == want and type(mat) is int and all(type(i) is int for i in ids), name


@pytest.mark.parametrize("given", INVALID, ids=[repr(g) for g in INVALID])
def test_every_parser_refuses_the_same(given):
    material, objects = given
    word = "object" if objects is not None else "material"
    for parse in list(PARSERS.values()) + [lambda material, objects: selection.parse(material, objects)]:
        with pytest.raises(ValueError, match=word):
            parse(material=material, objects=objects)


def test_field_colour_takes_material_names_only():
    assert selection.parse("solid", None, material_ids=False) == (0, [])
    for bad in (0, 1, np.int32(1)):
        with pytest.raises(ValueError, match="material"):
            selection.parse(bad, None, material_ids=False)


def test_fill_writes_the_same_selection_into_the_three_structs():
    for mat, ids in ((-1, []), (1, [3]), (0, [9, 2, 9]), (255, list(range(100, 132)))):
        seen = []
        for struct in (_lib.SphSampleSelect(), _lib.SphExportParams(), _lib.SphFieldColour()):
            selection.fill(struct, 0, list(range(200, 232)))       # what an earlier use left behind
            assert selection.fill(struct, mat, ids) is struct
            seen.append((struct.material, struct.n_objects, list(struct.object_ids)))
        assert seen[0] == seen[1] == seen[2] == (mat, len(ids), ids + [0] * (32 - len(ids)))
    # the callers' fillers are this one
    assert bytes(sample.make_select({"material": 1, "objects": [5]})) == bytes(selection.fill(_lib.SphSampleSelect(), 1, [5]))
    p = export.make_params(export.select_args(objects=[5], material="fluid"))
    assert (p.material, p.n_objects, list(p.object_ids)) == (1, 1, [5] + [0] * 31)


def test_the_three_limits_of_the_header_are_this_one():
    for name in ("SPH_EXPORT_MAX_OBJECTS", "SPH_FIELD_MAX_OBJECTS", "SPH_SAMPLE_MAX_OBJECTS"):
        m = re.search(rf"#define\s+{name}\s+(\d+)\b", HEADER)
        assert m and int(m.group(1)) == selection.MAX_OBJECTS, name
    assert selection.MAX_OBJECTS == _lib.EXPORT_MAX_OBJECTS == _lib.FIELD_MAX_OBJECTS == _lib.SAMPLE_MAX_OBJECTS
    assert export.MAX_OBJECTS == sample.MAX_OBJECTS == selection.MAX_OBJECTS
    for struct in (_lib.SphSampleSelect, _lib.SphExportParams, _lib.SphFieldColour):
        assert len(struct().object_ids) == selection.MAX_OBJECTS


def test_config_object():
    class Cfg:
        def __init__(self, **kw):
            self.kw = kw

        def get_cfg(self, key):
            return self.kw.get(key)
    assert selection.config_object(Cfg(), "probes", ("points",)) is None
    assert selection.config_object(Cfg(probes={"points": 1}), "probes", ("points",)) == {"points": 1}
    assert selection.config_object({"a": 1}, "thing", ("a", "b")) == {"a": 1} and selection.config_object(None, "thing", ()) is None
    with pytest.raises(ValueError, match='"probes" must be an object'):
        selection.config_object(Cfg(probes=[1]), "probes", ("points",))
    with pytest.raises(ValueError, match=r'"probes": unknown key\(s\) \[\'a\', \'b\'\]'):
        selection.config_object(Cfg(probes={"b": 1, "a": 2, "points": 3}), "probes", ("points",))
