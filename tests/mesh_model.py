"""A vectorised NumPy model of the surface mesh (include/sph_hip.h, section "Surface mesh"): surface nets on an i64 weight plane.
Written from the header's definition alone; the device result is held to it bit for bit (tests/test_gpu_mesh.py)."""
import numpy as np

F32 = np.float32
SCALE = 2.0 ** 30


def threshold(iso):
    """T = llrint((double)iso * 2^30) of the f32 value of iso (np.rint rounds half to even, as llrint does)."""
    return int(np.rint(float(F32(iso)) * SCALE))


def capped(weight, cap):
    """phi: the weight plane with the grid's outer layer of nodes set to 0 when cap is set."""
    phi = np.array(weight, dtype=np.int64, copy=True)
    assert phi.ndim == 3 and min(phi.shape) >= 2, phi.shape
    if cap:
        for a in range(3):
            idx = [slice(None)] * 3
            for end in (0, -1):
                idx[a] = end
                phi[tuple(idx)] = 0
    return phi


def cell_corners(a):
    """The 8 corner views [n0-1, n1-1, n2-1] of a node array; corner (i0, i1, i2) is entry 4 i0 + 2 i1 + i2."""
    n = a.shape
    return [a[(j >> 2):n[0] - 1 + (j >> 2), ((j >> 1) & 1):n[1] - 1 + ((j >> 1) & 1), (j & 1):n[2] - 1 + (j & 1)] for j in range(8)]


def extract(weight, origin, spacing, iso, cap):
    """{"vertices" f32 [V, 3], "normals" f32 [V, 3], "triangles" i32 [T, 3], "cells" i64 [V] (the cell linear index of every
    vertex), "keys" i64 [T / 2] (3 L + a of every quad)}."""
    phi = capped(weight, cap)
    n = phi.shape
    T = threshold(iso)
    inside = phi >= T
    P = [p.reshape(-1) for p in cell_corners(phi)]
    n_in = sum(p >= T for p in P)
    cells = np.nonzero((n_in > 0) & (n_in < 8))[0].astype(np.int64)          # ascending cell linear index
    V = cells.size
    P = [p[cells] for p in P]
    I = [p >= T for p in P]
    sums = np.zeros((3, V), dtype=np.float64)
    m = np.zeros(V, dtype=np.int64)
    g = np.zeros((3, V), dtype=np.int64)
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for ic in (0, 1):
            for ib in (0, 1):
                lo = ib * (4 >> b) + ic * (4 >> c)
                hi = lo + (4 >> a)
                d = P[hi] - P[lo]
                g[a] += d
                cross = I[lo] != I[hi]
                t = (T - P[lo]).astype(np.float64) / np.where(cross, d, 1).astype(np.float64)
                sums[a] += np.where(cross, t, 0.0)
                sums[b] += np.where(cross, float(ib), 0.0)
                sums[c] += np.where(cross, float(ic), 0.0)
                m += cross
    assert (m > 0).all()
    ccoord = np.stack(np.unravel_index(cells, tuple(k - 1 for k in n)), axis=0)
    pos = np.empty((V, 3), dtype=F32)
    for a in range(3):
        u = (sums[a] / m.astype(np.float64)).astype(F32)
        pos[:, a] = F32(origin[a]) + (ccoord[a].astype(F32) + u) * F32(spacing[a])
    gd = g.astype(np.float64)
    s = (gd[0] * gd[0] + gd[1] * gd[1]) + gd[2] * gd[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = np.where(s == 0, 0.0, -gd / np.sqrt(s)).astype(F32).T
    # faces
    vmap = np.full(tuple(k - 1 for k in n), -1, dtype=np.int64)
    vmap.reshape(-1)[cells] = np.arange(V)
    keys, quads, lo_in = [], [], []
    for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        lo_sl, hi_sl = [slice(None)] * 3, [slice(None)] * 3
        lo_sl[a], hi_sl[a] = slice(0, n[a] - 1), slice(1, n[a])
        cross = np.zeros(n, dtype=bool)
        cross[tuple(lo_sl)] = inside[tuple(lo_sl)] != inside[tuple(hi_sl)]
        region = np.zeros(n, dtype=bool)
        reg = [slice(None)] * 3
        reg[a], reg[b], reg[c] = slice(0, n[a] - 1), slice(1, n[b] - 1), slice(1, n[c] - 1)
        region[tuple(reg)] = True
        k = np.argwhere(cross & region)                                      # [Qa, 3]
        L = (k[:, 0] * n[1] + k[:, 1]) * n[2] + k[:, 2]
        eb, ec = np.eye(3, dtype=np.int64)[b], np.eye(3, dtype=np.int64)[c]
        four = [vmap[tuple((k - off).T)] for off in (eb + ec, ec, 0 * eb, eb)]
        keys.append(3 * L + a)
        quads.append(np.stack(four, axis=1))
        lo_in.append(inside[tuple(k.T)])
    keys, quads, lo_in = np.concatenate(keys), np.concatenate(quads), np.concatenate(lo_in)
    order = np.argsort(keys, kind="stable")
    keys, quads, lo_in = keys[order], quads[order], lo_in[order]
    assert (quads >= 0).all(), "a cell round a crossing edge is not active"
    c0, c1, c2, c3 = quads.T
    first = np.where(lo_in[:, None], np.stack([c0, c1, c2], axis=1), np.stack([c0, c3, c2], axis=1))
    second = np.where(lo_in[:, None], np.stack([c0, c2, c3], axis=1), np.stack([c0, c2, c1], axis=1))
    tri = np.stack([first, second], axis=1).reshape(-1, 3).astype(np.int32)
    return {"vertices": pos, "normals": nrm, "triangles": tri, "cells": cells, "keys": keys.astype(np.int64)}


def cell_counts(weight, iso, cap):
    """(cells with all 8 corners inside, cells not all outside) of the capped field: the volume sandwich in cells."""
    phi = capped(weight, cap)
    T = threshold(iso)
    n_in = sum((p >= T).astype(np.int64) for p in cell_corners(phi))
    return int((n_in == 8).sum()), int((n_in > 0).sum())
