"""numpy model of the particle export (include/sph_hip.h, section "Particle export"): a boolean mask, an argsort of the persistent
id and a column stack.  Nothing is computed on a value; the box is compared in f32 (a NaN is outside).  `read_ply` is the reader the tests
parse the written files with: it knows nothing of the writer."""
import numpy as np

# row order of the optional fields and the structured columns they become
ROW_ORDER = ("velocity", "density", "pressure", "mass", "id", "object")
ALL_FIELDS = ROW_ORDER


def row_dtype(fields):
    cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    for name in ROW_ORDER:
        if name in fields:
            cols += [("vx", "<f4"), ("vy", "<f4"), ("vz", "<f4")] if name == "velocity" else \
                [(name, "<i4" if name in ("id", "object") else "<f4")]
    return np.dtype(cols)


def select_mask(x, material, object_id, pid, *, objects=None, select_material=None, box=None, every=1, phase=0):
    """Which records the selection keeps.  `objects`: list of ids or None (all); `select_material`: an id or None (any)."""
    n = pid.shape[0]
    keep = np.ones(n, dtype=bool)
    if select_material is not None:
        keep &= material == np.int32(select_material)
    if objects is not None:
        keep &= np.isin(object_id, np.asarray(list(objects), dtype=np.int32))
    keep &= (pid % np.int32(every)) == np.int32(phase)
    if box is not None:
        lo, hi = np.asarray(box[0], dtype=np.float32), np.asarray(box[1], dtype=np.float32)
        xf = np.asarray(x, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            keep &= ((xf >= lo) & (xf <= hi)).all(axis=1)          # comparisons with a NaN are False
    return keep


def export_rows(x, v, density, pressure, m, material, object_id, pid, *, fields=(), objects=None, select_material=None, box=None,
                every=1, phase=0):
    """{"data": structured rows in ascending persistent id, "selected", "rows", "duplicate_ids"}.  With duplicate ids among the
    selected records no row order is defined: "data" is None then."""
    keep = select_mask(x, material, object_id, pid, objects=objects, select_material=select_material, box=box, every=every,
                       phase=phase)
    idx = np.flatnonzero(keep)
    selected = int(idx.size)
    distinct = int(np.unique(pid[idx]).size)
    out = {"selected": selected, "rows": distinct, "duplicate_ids": selected - distinct, "data": None}
    if distinct != selected:
        return out
    idx = idx[np.argsort(pid[idx], kind="stable")]
    data = np.empty(selected, dtype=row_dtype(fields))
    data["x"], data["y"], data["z"] = x[idx, 0], x[idx, 1], x[idx, 2]
    if "velocity" in fields:
        data["vx"], data["vy"], data["vz"] = v[idx, 0], v[idx, 1], v[idx, 2]
    for name, src in (("density", density), ("pressure", pressure), ("mass", m), ("id", pid), ("object", object_id)):
        if name in fields:
            data[name] = src[idx]
    out["data"] = data
    return out


def read_ply(path):
    """(structured array over the body, comments) of a binary little-endian PLY with one vertex element"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    count, cols, comments = None, [], []
    for line in lines[2:-1]:
        w = line.split()
        if w[0] == "comment":
            comments.append(line[len("comment "):])
        elif w[0] == "element":
            assert w[1] == "vertex" and count is None
            count = int(w[2])
        else:
            assert w[0] == "property" and w[1] in ("float", "int"), line
            cols.append((w[2], "<f4" if w[1] == "float" else "<i4"))
    body = raw[end:]
    data = np.frombuffer(body, dtype=np.dtype(cols))
    assert data.shape[0] == count
    return data, comments, body
