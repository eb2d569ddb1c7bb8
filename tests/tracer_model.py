"""A brute-force numpy model of the tracer contract (include/sph_hip.h, section "Passive tracers"): one advance of a set of tracers
through a particle state.  Cell coordinates of tracer and particles by the f32 divide + truncation (the particles' clamped into the
grid, as the sort hashes them), membership in the tracer's 27 cells, the pair term in f32 operation by operation (np.float32
throughout; np.sqrt on f32 is correctly rounded), the terms as f64 products rounded with np.rint into int64, then the advance.  It
knows nothing of lanes, runs, the cell array or the particle order: every tracer looks at every particle.
"""
import numpy as np

F32 = np.float32
SCALE = float(1 << 30)
LIMIT = F32(2.0 ** 24)


def params_of(ps, min_fill=0.2, material=1, objects=(), dt=None):
    """What the model needs of a ParticleSystem's context parameters (the f32 values the library holds)."""
    p = ps._params
    return {"grid_size": F32(p.grid_size), "grid_num": tuple(int(v) for v in p.grid_num), "inv_h": F32(1) / F32(p.support_radius),
            "k_w": F32(p.k_w), "dt": F32(p.dt if dt is None else dt), "padding": F32(p.padding),
            "wall_hi": np.array([p.wall_hi[a] for a in range(3)], dtype=F32), "min_fill": F32(min_fill),
            "material": -1 if material is None else int(material), "objects": tuple(objects)}


def min_weight(min_fill):
    return max(int(np.rint(float(F32(min_fill)) * SCALE)), 1)


def tracer_cells(p, grid_size):
    """(int)(p_a / grid_size): f32 division, truncation, no clamp."""
    return (np.asarray(p, dtype=F32) / F32(grid_size)).astype(np.int32)


def particle_cells(x, grid_size, grid_num):
    """... and clamped into the grid, as the sort hashes the particles (sph_cell_coord)."""
    c = (np.asarray(x, dtype=F32) / F32(grid_size)).astype(np.int32)
    return np.clip(c, 0, np.asarray(grid_num, dtype=np.int32) - 1)


def pair_weight(p, x, m_V, inv_h, k_w):
    """(contributes [N], w f32 [N]) of position p [3] against particles x [N, 3], m_V [N]: the contract's f32 sequence."""
    inv_h, k_w = F32(inv_h), F32(k_w)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[0] - x[:, 0], p[1] - x[:, 1], p[2] - x[:, 2]
        r2 = (dx * dx + dy * dy) + dz * dz
        r = np.sqrt(r2)
        q = r * inv_h
        assert q.dtype == F32
        inside = q <= F32(1)
        q2 = q * q
        q3 = q2 * q
        inner = k_w * ((F32(6) * q3 - F32(6) * q2) + F32(1))
        t = F32(1) - q
        outer = (k_w * F32(2)) * ((t * t) * t)
        W = np.where(q <= F32(0.5), inner, outer)
        w = np.fmin(np.fmax(m_V * W, F32(0)), F32(4))
        assert w.dtype == F32
    return inside, w


def selected(material, object_id, want_material, objects):
    sel = np.ones(np.asarray(material).shape[0], dtype=bool)
    if want_material is not None and want_material >= 0:
        sel &= np.asarray(material) == want_material
    if len(objects):
        sel &= np.isin(np.asarray(object_id), np.asarray(list(objects)))
    return sel


def gather(tx, x, v, m_V, material, object_id, P):
    """count i32 [m], weight i64 [m], sums i64 [m, 3] of the tracers tx [m, 3] over the particle state."""
    tx = np.asarray(tx, dtype=F32).reshape(-1, 3)
    x, v, m_V = np.asarray(x, dtype=F32).reshape(-1, 3), np.asarray(v, dtype=F32).reshape(-1, 3), np.asarray(m_V, dtype=F32).reshape(-1)
    m = tx.shape[0]
    count, weight, sums = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64), np.zeros((m, 3), dtype=np.int64)
    if x.shape[0] == 0:
        return count, weight, sums
    sel = selected(material, object_id, P["material"], P["objects"])
    pc = particle_cells(x, P["grid_size"], P["grid_num"])
    tc = tracer_cells(tx, P["grid_size"])
    v64 = np.fmax(np.fmin(v, LIMIT), -LIMIT).astype(np.float64)
    for t in range(m):
        in_block = (np.abs(pc - tc[t]) <= 1).all(axis=1)      # (a cell outside the grid holds nobody: pc is inside it)
        inside, w = pair_weight(tx[t], x, m_V, P["inv_h"], P["k_w"])
        c = sel & in_block & inside
        w64 = w[c].astype(np.float64)
        count[t] = int(c.sum())
        weight[t] = np.rint(w64 * SCALE).astype(np.int64).sum()
        sums[t] = np.rint((w64[:, None] * v64[c]) * SCALE).astype(np.int64).sum(axis=0)
    return count, weight, sums


def advance(state, x, v, m_V, material, object_id, P):
    """One advance.  `state`: {"x" f32 [m, 3], "wet_steps", "dry_steps" i32 [m]} (and whatever else: ignored); returns the new
    state {"x", "u", "weight", "count", "wet_steps", "dry_steps"}; the input is left alone."""
    tx = np.array(state["x"], dtype=F32, copy=True).reshape(-1, 3)
    count, weight, sums = gather(tx, x, v, m_V, material, object_id, P)
    wet = weight >= min_weight(P["min_fill"])
    u = np.zeros_like(tx)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (sums.astype(np.float64) / weight.astype(np.float64)[:, None]).astype(F32)
    u[wet] = mean[wet]
    xn = tx + F32(P["dt"]) * u                                # f32 multiply, then f32 add
    assert xn.dtype == F32
    xn = np.fmin(np.fmax(xn, F32(P["padding"])), np.asarray(P["wall_hi"], dtype=F32)[None, :])
    out_x = np.where(wet[:, None], xn, tx).astype(F32)
    return {"x": out_x, "u": u, "weight": weight, "count": count,
            "wet_steps": (np.asarray(state["wet_steps"], dtype=np.int32) + wet).astype(np.int32),
            "dry_steps": (np.asarray(state["dry_steps"], dtype=np.int32) + ~wet).astype(np.int32)}


def fresh(points):
    m = np.asarray(points).reshape(-1, 3).shape[0]
    return {"x": np.asarray(points, dtype=F32).reshape(-1, 3).copy(), "wet_steps": np.zeros(m, np.int32), "dry_steps": np.zeros(m, np.int32)}
