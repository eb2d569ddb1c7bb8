"""Numpy model of the particle features (include/sph_hip.h, section "Particle features"): BRUTE FORCE over all target x candidate
pairs, with the contract's arithmetic term by term -- the pair geometry and the kernel polynomial in f32, the volumes, gradients and
terms in f64 (IEEE multiply, divide, subtract: numpy's are the device's) in the contract's order, the clamps, np.rint (to nearest
even, like llrint) and integer sums -- and the finish that turns the sums into the 64-byte rows.  Candidates are restricted to the
27 cells around the target's (clamped) cell, as the contract restricts them; `cells=False` lifts that for the all-pairs check.

    sums = sample_sums(state, params, ...)      {"fill" [T], "N" [T, 3], "G" [T, 9], "n_fluid", "n_solid", "sat" [T]} i64, + "targets"
    rows = finish(state, sums, params, ...)     features.ROW_DTYPE [n_rows] by persistent id
    rows = sample(state, params, ...)           both

`state`: arrays in any common order: x, v f32 [N, 3]; m_V, m, density f32 [N]; material, object_id, pid int [N].
`params`: {"support_radius", "grid_size", "k_w", "k_dw" f32; "grid_num" int [3]}.
"""
import numpy as np

from sph_taichi_amd import features as ft
from sph_taichi_amd import scene as scene_mod

F32 = np.float32
SCALE = float(1 << 24)
LIMIT = float(1 << 20)
FILL_SCALE = float(1 << 30)
FILL_LIMIT = float(1 << 14)


def params_of(support_radius, grid_size, grid_num):
    """The context's f32 parameters from the geometry, as the Python layer hands them to the library (scene.kernel_constants)."""
    kc = scene_mod.kernel_constants(float(support_radius), 0.0)
    return {"support_radius": F32(support_radius), "grid_size": F32(grid_size), "grid_num": np.asarray(grid_num, dtype=np.int64),
            "k_w": F32(kc["k_w"]), "k_dw": F32(kc["k_dw"])}


def params_of_ps(ps):
    p = ps._params
    return {"support_radius": F32(p.support_radius), "grid_size": F32(p.grid_size), "grid_num": np.array(list(p.grid_num), dtype=np.int64),
            "k_w": F32(p.k_w), "k_dw": F32(p.k_dw)}


def state_of_ps(ps):
    return {"x": ps.x.to_numpy(), "v": ps.v.to_numpy(), "m_V": ps.m_V.to_numpy(), "m": ps.m.to_numpy(), "density": ps.density.to_numpy(),
            "material": ps.material.to_numpy(), "object_id": ps.object_id.to_numpy(), "pid": ps.pid.to_numpy()}


def cell_coords(x, grid_size, grid_num):
    """pos_to_index with the library's clamp: int(p / grid_size) in f32, truncated, clamped to the grid."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.trunc(np.asarray(x, F32) / F32(grid_size)).astype(np.int64)
    return np.clip(c, 0, np.asarray(grid_num, np.int64) - 1)


def selected(state, material=1, objects=()):
    sel = np.ones(np.asarray(state["material"]).shape[0], dtype=bool)
    if material is not None and material >= 0:
        sel &= np.asarray(state["material"]) == material
    if len(objects):
        sel &= np.isin(np.asarray(state["object_id"]), list(objects))
    return sel


def _term(f, limit, scale):
    cl = np.fmin(np.fmax(f, -limit), limit)                                   # a NaN ends at -limit, like fmin(fmax()) on the device
    return np.rint(cl * scale).astype(np.int64), (cl != f)


def volumes(state):
    """f64 [N]: m / rho of a fluid record, the boundary volume of any other."""
    fluid = np.asarray(state["material"]) == 1
    with np.errstate(all="ignore"):
        vf = np.asarray(state["m"], F32).astype(np.float64) / np.asarray(state["density"], F32).astype(np.float64)
    return np.where(fluid, vf, np.asarray(state["m_V"], F32).astype(np.float64))


def sample_sums(state, params, material=1, objects=(), cells=True, chunk=128):
    x, v = np.asarray(state["x"], F32), np.asarray(state["v"], F32)
    fluid = np.asarray(state["material"]) == 1
    vol = volumes(state)
    tgt = np.flatnonzero(selected(state, material, objects))
    h32 = F32(params["support_radius"])
    inv_h = F32(1) / h32
    h, kw, kdw = float(h32), float(F32(params["k_w"])), float(F32(params["k_dw"]))
    cc = cell_coords(x, params["grid_size"], params["grid_num"])
    T = tgt.size
    out = {"targets": tgt, "fill": np.zeros(T, np.int64), "N": np.zeros((T, 3), np.int64), "G": np.zeros((T, 9), np.int64),
           "n_fluid": np.zeros(T, np.int64), "n_solid": np.zeros(T, np.int64), "sat": np.zeros(T, np.int64)}
    for at in range(0, T, chunk):
        i = tgt[at:at + chunk]
        sl = slice(at, at + i.size)
        with np.errstate(all="ignore"):
            d = x[i][:, None, :] - x[None, :, :]                              # f32: d = x_i - x_j
            r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            r = np.sqrt(r2)
            q = r * inv_h
            assert d.dtype == r.dtype == q.dtype == F32
            accept = (q <= F32(1.0)) & (r > F32(1e-5))
            if cells:
                accept &= (np.abs(cc[i][:, None, :] - cc[None, :, :]) <= 1).all(axis=-1)
            q2 = q * q
            q3 = q2 * q
            t = F32(1) - q
            P = np.where(q <= F32(0.5), (F32(6) * q3 - F32(6) * q2) + F32(1), F32(2) * ((t * t) * t))
            assert P.dtype == F32
            q64, r64 = q.astype(np.float64), r.astype(np.float64)
            g = np.where(q <= F32(0.5), q64 * (3.0 * q64 - 2.0), -((1.0 - q64) * (1.0 - q64)))
            coef = (kdw * g) / (r64 * h)
            gW = coef[..., None] * d.astype(np.float64)                       # [I, J, 3]
            vj = vol[None, :]
            fill_t, fill_s = _term(vj * (kw * P.astype(np.float64)), FILL_LIMIT, FILL_SCALE)
            n_t, n_s = _term(vj[..., None] * gW, LIMIT, SCALE)
            dv = v[None, :, :] - v[i][:, None, :]                             # f32: v_j - v_i
            assert dv.dtype == F32
            vdv = vj[..., None] * dv.astype(np.float64)                       # [I, J, a]
            g_t, g_s = _term(vdv[..., :, None] * gW[..., None, :], LIMIT, SCALE)   # [I, J, a, b]
            self_t, self_s = _term(vol[i] * (kw * 1.0), FILL_LIMIT, FILL_SCALE)
        af = accept & fluid[None, :]
        out["fill"][sl] = np.where(accept, fill_t, 0).sum(axis=1) + self_t
        out["N"][sl] = np.where(accept[..., None], n_t, 0).sum(axis=1)
        out["G"][sl] = np.where(af[..., None, None], g_t, 0).sum(axis=1).reshape(i.size, 9)
        out["n_fluid"][sl] = af.sum(axis=1)
        out["n_solid"][sl] = (accept & ~fluid[None, :]).sum(axis=1)
        out["sat"][sl] = (np.where(accept, fill_s, False).sum(axis=1) + np.where(accept[..., None], n_s, False).sum(axis=(1, 2))
                          + np.where(af[..., None, None], g_s, False).sum(axis=(1, 2, 3)) + self_s)
    return out


def finish(state, sums, params, min_neighbours=24, normal_min=0.0, n_rows=None):
    pid = np.asarray(state["pid"]).astype(np.int64)
    n_rows = int(pid.max()) + 1 if n_rows is None else int(n_rows)
    rows = np.zeros(n_rows, dtype=ft.ROW_DTYPE)
    tgt = sums["targets"]
    G, N = sums["G"], sums["N"]
    f = lambda I, scale: (I.astype(np.float64) / scale).astype(F32)
    r = np.zeros(tgt.size, dtype=ft.ROW_DTYPE)
    r["x"] = np.asarray(state["x"], F32)[tgt]
    r["vorticity"] = np.stack([f(G[:, 7] - G[:, 5], SCALE), f(G[:, 2] - G[:, 6], SCALE), f(G[:, 3] - G[:, 1], SCALE)], axis=1)
    r["divergence"] = f((G[:, 0] + G[:, 4]) + G[:, 8], SCALE)
    r["normal"] = f(N, SCALE)
    r["fill"] = f(sums["fill"], FILL_SCALE)
    r["n_fluid"], r["n_solid"] = sums["n_fluid"], sums["n_solid"]
    Nd = N.astype(np.float64) / SCALE
    n2 = (Nd[:, 0] * Nd[:, 0] + Nd[:, 1] * Nd[:, 1]) + Nd[:, 2] * Nd[:, 2]
    h, nm = float(F32(params["support_radius"])), float(F32(normal_min))
    surface = (sums["n_fluid"] + sums["n_solid"]) < int(min_neighbours)
    if F32(normal_min) > 0:
        surface |= (h * h) * n2 > nm * nm
    r["flags"] = ft.VALID | np.where(surface, ft.SURFACE, 0) | np.where(sums["sat"] > 0, ft.SATURATED, 0)
    ok = (pid[tgt] >= 0) & (pid[tgt] < n_rows)
    rows[pid[tgt][ok]] = r[ok]
    return rows


def sample(state, params, material=1, objects=(), min_neighbours=24, normal_min=0.0, n_rows=None, cells=True):
    return finish(state, sample_sums(state, params, material, objects, cells), params, min_neighbours, normal_min, n_rows)


def gradient(sums):
    """f64 [T, 3, 3]: G[a, b] = d v_a / d x_b of the targets, from the integer sums."""
    return sums["G"].astype(np.float64).reshape(-1, 3, 3) / SCALE


def all_pairs_f64(state, params, material=1, objects=()):
    """The same quantities in plain f64 from the f32 state, over ALL pairs with |x_i - x_j| <= h, no cells, no fixed point: what the
    model's integers are checked against.  Returns {"fill" [T], "N" [T, 3], "G" [T, 3, 3], "n" [T]}."""
    x, v = np.asarray(state["x"], F32).astype(np.float64), np.asarray(state["v"], F32).astype(np.float64)
    fluid = np.asarray(state["material"]) == 1
    vol = volumes(state)
    tgt = np.flatnonzero(selected(state, material, objects))
    h = float(F32(params["support_radius"]))
    kw, kdw = float(F32(params["k_w"])), float(F32(params["k_dw"]))
    out = {"fill": np.zeros(tgt.size), "N": np.zeros((tgt.size, 3)), "G": np.zeros((tgt.size, 3, 3)), "n": np.zeros(tgt.size, np.int64)}
    for k, i in enumerate(tgt):
        d = x[i] - x
        r = np.sqrt((d * d).sum(axis=1))
        q = r / h
        near = (q <= 1.0) & (r > 1e-5)
        j = np.flatnonzero(near)
        qj, rj = q[j], r[j]
        W = kw * np.where(qj <= 0.5, 6 * qj ** 3 - 6 * qj ** 2 + 1, 2 * (1 - qj) ** 3)
        dW = kdw * np.where(qj <= 0.5, qj * (3 * qj - 2), -(1 - qj) ** 2) / h
        gW = (dW / rj)[:, None] * d[j]
        out["fill"][k] = vol[i] * kw + (vol[j] * W).sum()
        out["N"][k] = (vol[j][:, None] * gW).sum(axis=0)
        jf = fluid[j]
        out["G"][k] = np.einsum("j,ja,jb->ab", vol[j][jf], (v[j] - v[i])[jf], gW[jf])
        out["n"][k] = j.size
    return out
