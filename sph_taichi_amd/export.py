"""Particle export: what `ParticleSystem.export_particles()` returns and the binary PLY it writes (include/sph_hip.h, section
"Particle export"; csrc/sph_export.hip).

The device selects the particles (objects, material, a box, a decimation by persistent id), orders them BY PERSISTENT ID and
packs the chosen fields into the byte rows of a binary PLY vertex body; only those rows cross to the host, and vertex k of one
file is the same particle as vertex k of the next.  Nothing in this module touches the GPU when it is imported: the library is
reached through the ParticleSystem handed to `export`.
"""
from __future__ import annotations

import numpy as np

from . import selection
from .selection import MATERIALS, MAX_OBJECTS   # noqa: F401  (part of this module's surface)

# optional fields in ROW ORDER: name -> (bit of SphExportParams.fields, columns of the structured array)
FIELD_BITS = {"velocity": 2, "density": 4, "pressure": 8, "mass": 16, "id": 32, "object": 64}
FIELD_COLUMNS = {"velocity": (("vx", "<f4"), ("vy", "<f4"), ("vz", "<f4")), "density": (("density", "<f4"),),
                 "pressure": (("pressure", "<f4"),), "mass": (("mass", "<f4"),), "id": (("id", "<i4"),), "object": (("object", "<i4"),)}
EXPORT_X = 1
CONFIG_KEYS = ("objects", "material", "fields", "box", "every", "phase")


def row_dtype(fields) -> np.dtype:
    """The structured dtype of one row: x y z, then the columns of `fields` in row order (packed, little endian)."""
    cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    for name in FIELD_BITS:
        if name in fields:
            cols.extend(FIELD_COLUMNS[name])
    return np.dtype(cols)


def select_args(objects=None, material=None, fields=("velocity",), box=None, every=1, phase=0) -> dict:
    """The arguments of `export_particles` checked and normalised, without a context: {"fields": names in row order, "mask",
    "material": -1 or the id, "objects": list, "box": None or (lo, hi) as f32 triples, "every", "phase"}.  ValueError otherwise."""
    if isinstance(fields, str):
        raise ValueError("fields must be a sequence of names, not one string")
    fields = list(fields)
    unknown = [f for f in fields if f not in FIELD_BITS]
    if unknown:
        raise ValueError(f"unknown field(s) {unknown}: choose from {list(FIELD_BITS)} (the position is always exported)")
    if len(set(fields)) != len(fields):
        raise ValueError("a field is named twice")
    names = tuple(n for n in FIELD_BITS if n in fields)
    mask = EXPORT_X
    for n in names:
        mask |= FIELD_BITS[n]
    mat, ids = selection.parse(material, objects)
    every, phase = selection.integer(every, "every"), selection.integer(phase, "phase")
    if every < 1 or every > 2 ** 31 - 1:
        raise ValueError("every must be at least 1")
    if not 0 <= phase < every:
        raise ValueError("phase must be in [0, every)")
    if box is not None:
        try:
            b = np.asarray(box, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError("box must be [[lo_x, lo_y, lo_z], [hi_x, hi_y, hi_z]]") from e
        if b.shape != (2, 3):
            raise ValueError("box must be [[lo_x, lo_y, lo_z], [hi_x, hi_y, hi_z]]")
        with np.errstate(over="ignore"):
            b = b.astype(np.float32)
        if not np.isfinite(b).all():
            raise ValueError("box must be finite (as f32)")
        if (b[0] > b[1]).any():
            raise ValueError("box: lo must not exceed hi")
        box = (tuple(float(v) for v in b[0]), tuple(float(v) for v in b[1]))
    return {"fields": names, "mask": mask, "material": mat, "objects": ids, "box": box, "every": every, "phase": phase}


def export_config(config):
    """The scene's "exportParticles" object: {"objects": [0], "material": "fluid", "fields": [...], "box": [[lo], [hi]],
    "every": 1, "phase": 0}, every key optional ({} = every particle, positions only).  Returns the checked keyword arguments
    of `export_particles`, or None when the key is absent.  A misspelt key or a bad value raises ValueError."""
    spec = selection.config_object(config, "exportParticles", CONFIG_KEYS)
    if spec is None:
        return None
    kw = {"objects": spec.get("objects"), "material": spec.get("material"), "fields": tuple(spec.get("fields", ())),
          "box": spec.get("box"), "every": spec.get("every", 1), "phase": spec.get("phase", 0)}
    try:
        a = select_args(**kw)
    except ValueError as e:
        raise ValueError(f'"exportParticles": {e}') from e
    return {"objects": a["objects"] or None, "material": None if a["material"] < 0 else a["material"], "fields": a["fields"],
            "box": a["box"], "every": a["every"], "phase": a["phase"]}


def ply_header(dtype: np.dtype, count: int, comments=()) -> bytes:
    lines = ["ply", "format binary_little_endian 1.0", "comment created by sph_taichi_amd"]
    for c in comments:
        if "\n" in str(c) or "\r" in str(c):
            raise ValueError("a PLY comment is one line")
        lines.append(f"comment {c}")
    lines.append(f"element vertex {int(count)}")
    for name in dtype.names:
        kind = dtype[name]
        if kind == np.dtype("<f4"):
            lines.append(f"property float {name}")
        elif kind == np.dtype("<i4"):
            lines.append(f"property int {name}")
        else:
            raise ValueError(f"field {name}: only little-endian f32 and i32 columns can be written, not {kind}")
    lines.append("end_header")
    return ("\n".join(lines) + "\n").encode("ascii")


def write_ply(path, data, comments=()):
    """`data` (a structured array of packed little-endian f32 / i32 columns) as a binary PLY vertex list: a header with one
    `property float|int <name>` per column in row order, then `data.tobytes()` unchanged."""
    data = np.asarray(data)
    if data.dtype.names is None or data.ndim != 1:
        raise ValueError("write_ply takes a one-dimensional structured array")
    if data.dtype.itemsize != 4 * len(data.dtype.names):
        raise ValueError("write_ply takes packed rows (no padding between the columns)")
    head = ply_header(data.dtype, data.shape[0], comments)
    with open(path, "wb") as fh:
        fh.write(head)
        fh.write(data.tobytes())


class ParticleExport:
    """One export: `data` (structured array over the downloaded rows: x y z, then whichever of vx vy vz density pressure mass
    id object were asked for), `count` rows in ascending persistent id, `selected` records, `fields`, `time`."""

    def __init__(self, data, selected, fields, time):
        self.data = data
        self.count = int(data.shape[0])
        self.selected = int(selected)
        self.fields = tuple(fields)
        self.time = float(time)

    def write_ply(self, path, comments=()):
        write_ply(path, self.data, tuple(comments) + (f"time {self.time!r}",))


def make_params(args: dict):
    """SphExportParams of checked arguments (`select_args`)."""
    import ctypes as C
    from . import _lib
    p = _lib.SphExportParams()
    p.fields = args["mask"]
    selection.fill(p, args["material"], args["objects"])
    p.pid_stride, p.pid_phase = args["every"], args["phase"]
    p.use_box = 0 if args["box"] is None else 1
    if args["box"] is not None:
        p.box_lo, p.box_hi = (C.c_float * 3)(*args["box"][0]), (C.c_float * 3)(*args["box"][1])
    return p


def select_info(ps, params):
    """sph_export_select + sph_export_info: the SphExportInfo of the selection (synchronises)."""
    import ctypes as C
    from . import _lib
    ps._call("sph_export_select", C.byref(params))
    info = _lib.SphExportInfo()
    ps._call("sph_export_info", C.byref(info))
    return info


def download_rows(ps, info, dtype) -> np.ndarray:
    """sph_export_download into a fresh structured array (raises SphError if the ids were not unique)."""
    import ctypes as C
    assert dtype.itemsize == info.row_bytes, (dtype.itemsize, info.row_bytes)
    data = np.empty(int(info.rows), dtype=dtype)
    ps._call("sph_export_download", data.ctypes.data_as(C.c_void_p), data.nbytes)
    return data


def export(ps, objects=None, material=None, fields=("velocity",), box=None, every=1, phase=0) -> ParticleExport:
    args = select_args(objects=objects, material=material, fields=fields, box=box, every=every, phase=phase)
    if ps.slab is not None:
        raise NotImplementedError("particles are exported from single-domain contexts only: a slab rank's ghost records would "
                                  "be exported twice (the ranks' owned ranges would have to be selected and gathered)")
    info = select_info(ps, make_params(args))
    data = download_rows(ps, info, row_dtype(args["fields"]))
    return ParticleExport(data, info.selected, args["fields"], ps.time)
