"""numpy model of the column maps (include/sph_hip.h, section "Depth-integrated column maps"): the same operations on the same
operands as csrc/sph_columns.hip, so every comparison with the device is exact.

    index     : np.floor((x - o) * inv) in f32 -- one f32 subtract, one f32 multiply, floor; inside when 0 <= f < n on the float
    velocity  : np.rint(np.fmax(np.fmin(v, L), -L).astype(f64) * 2^20).astype(i64), L = 65536 (rint: ties to even, as llrint)
    columns   : np.add.at / np.maximum.at / np.minimum.at
"""
import numpy as np

V_LIMIT = np.float32(65536.0)
V_SCALE = float(1 << 20)
MATERIAL_FLUID = 1


def horizontal(axis):
    return [j for j in range(3) if j != axis]


def inv_cell(cell):
    """f32(1) / f32(cell), per horizontal axis (`cell`: one number or a pair)."""
    c = np.broadcast_to(np.asarray(cell, dtype=np.float64), (2,))
    return np.array([np.float32(1) / np.float32(v) for v in c], dtype=np.float32)


def index(points2, origin, inv, shape):
    """Flat column index k0 * n1 + k1 of points [M, 2]; -1 outside."""
    p = np.asarray(points2, dtype=np.float32).reshape(-1, 2)
    o, inv = np.asarray(origin, dtype=np.float32), np.asarray(inv, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((p - o[None, :]) * inv[None, :])
        assert f.dtype == np.float32
        n = np.asarray(shape, dtype=np.float32)
        inside = ((f >= 0) & (f < n[None, :])).all(axis=1)
    k = np.where(inside[:, None], f, 0).astype(np.int64)
    return np.where(inside, k[:, 0] * int(shape[1]) + k[:, 1], -1)


def velocity_terms(v):
    v = np.asarray(v, dtype=np.float32)
    return np.rint(np.fmax(np.fmin(v, V_LIMIT), -V_LIMIT).astype(np.float64) * V_SCALE).astype(np.int64)


def column_map(x, v, material, object_id, axis, origin, inv, shape, select_object=-1):
    """dict(count [n0, n1] i64, sum_v [3, n0, n1] i64, top, bottom [n0, n1] f32 (0 where empty), selected, binned, outside)."""
    x, v = np.asarray(x, dtype=np.float32), np.asarray(v, dtype=np.float32)
    sel = np.asarray(material) == MATERIAL_FLUID
    if select_object >= 0:
        sel &= np.asarray(object_id) == select_object
    col = index(x[sel][:, horizontal(axis)], origin, inv, shape)
    binned = col >= 0
    nc = int(shape[0]) * int(shape[1])
    count = np.zeros(nc, dtype=np.int64)
    sum_v = np.zeros((3, nc), dtype=np.int64)
    top = np.full(nc, -np.inf, dtype=np.float32)
    bottom = np.full(nc, np.inf, dtype=np.float32)
    c = col[binned]
    np.add.at(count, c, 1)
    terms = velocity_terms(v[sel][binned])
    for a in range(3):
        np.add.at(sum_v[a], c, terms[:, a])
    up = x[sel][binned][:, axis]
    np.maximum.at(top, c, up)
    np.minimum.at(bottom, c, up)
    top[count == 0] = 0.0
    bottom[count == 0] = 0.0
    shape = (int(shape[0]), int(shape[1]))
    return {"count": count.reshape(shape), "sum_v": sum_v.reshape((3,) + shape), "top": top.reshape(shape),
            "bottom": bottom.reshape(shape), "selected": int(sel.sum()), "binned": int(binned.sum()),
            "outside": int((~binned).sum())}
