"""The particle selection every observer takes -- `material=` and `objects=` of `export_particles`, `sample_grid`,
`sample_points`, `surface_mesh`, `set_tracers` and `FieldColour` -- parsed once, and the preamble of the scene keys that carry
one.  The library's side is `SphSel` in csrc/sph_observe.h.  Nothing here touches the GPU.
"""
from __future__ import annotations

import numpy as np

MATERIALS = {"solid": 0, "fluid": 1}           # particle_system.py:30-31 of the reference
MAX_OBJECTS = 32                               # SPH_EXPORT_ / SPH_FIELD_ / SPH_SAMPLE_MAX_OBJECTS (checked where `fill` meets a struct)


def integer(value, name) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, not {value!r}")
    return int(value)


def parse(material, objects, *, material_ids=True):
    """(mat, ids) of `material` -- a name of MATERIALS, None (any: -1) or, with `material_ids`, an id in [0, 255] -- and
    `objects` -- None (all: []), one object id or up to MAX_OBJECTS of them.  ValueError otherwise."""
    if material is None:
        mat = -1
    elif isinstance(material, str) or not material_ids:
        if not isinstance(material, str) or material not in MATERIALS:
            raise ValueError(f"material must be one of {list(MATERIALS)}{', a material id' if material_ids else ''} or None (any), not {material!r}")
        mat = MATERIALS[material]
    else:
        mat = integer(material, "material")
        if not 0 <= mat <= 255:
            raise ValueError("a material id is in [0, 255]")
    if objects is None:
        return mat, []
    if isinstance(objects, (int, np.integer, bool, np.bool_)):
        objects = [objects]
    try:
        objects = list(objects)
    except TypeError:
        raise ValueError(f"objects must be an object id, a list of them or None, not {objects!r}") from None
    ids = [integer(o, "an object id in objects") for o in objects]
    if not ids:
        raise ValueError("objects is empty: pass None for every object")
    if len(ids) > MAX_OBJECTS:
        raise ValueError(f"at most {MAX_OBJECTS} objects can be selected at once")
    if min(ids) < 0:
        raise ValueError("an object id in objects is not negative")
    return mat, ids


def fill(struct, mat, ids):
    """The selection into a SphExportParams, SphFieldColour or SphSampleSelect -- a fresh one, or one this function filled
    before: the ids behind the new ones are zero then, as in a fresh struct.  Returns the struct."""
    dst, before = struct.object_ids, struct.n_objects
    assert len(dst) == MAX_OBJECTS
    struct.material, struct.n_objects = mat, len(ids)
    for k, oid in enumerate(ids):
        dst[k] = oid
    for k in range(len(ids), before):
        dst[k] = 0
    return struct


def config_object(config_or_entry, key, allowed_keys):
    """The scene's object under `key` -- looked up in a Configuration, or the entry itself where the caller holds it -- or None
    when it is absent.  ValueError unless it is an object whose keys are among `allowed_keys`."""
    spec = config_or_entry.get_cfg(key) if hasattr(config_or_entry, "get_cfg") else config_or_entry
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError(f'"{key}" must be an object')
    unknown = set(spec) - set(allowed_keys)
    if unknown:
        raise ValueError(f'"{key}": unknown key(s) {sorted(unknown)}')
    return spec
