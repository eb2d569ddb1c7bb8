"""A numpy model of the field-sampling contract (include/sph_hip.h, section "Field sampling"): the f32 operations of the pair
term one by one (np.float32 throughout, np.sqrt on f32, which is correctly rounded), the terms as f64 products rounded with
np.rint, the sums in int64.  Brute force over (position, particle) pairs, in chunks of positions: it knows nothing of footprints,
tiles or particle order, so a footprint that is too small on the device is a difference from this model.
"""
import numpy as np

F32 = np.float32
SCALE = float(1 << 30)
LIMIT = F32(2.0 ** 24)
PLANES = ("vx", "vy", "vz", "density", "pressure")          # the order of the SPH_SAMPLE_* bits


def k_w(support_radius):
    """The context's folded constant as the Python layer hands it to the library: f32(8 / (pi h^3)) (sph_base.py:28-34)."""
    h = float(support_radius)
    return F32((8 / np.pi) / h ** 3)


def inv_h(support_radius):
    return F32(1) / F32(support_radius)


def node_positions(origin, spacing, shape):
    """f32 [nodes, 3] in node order (k0 * n1 + k1) * n2 + k2: origin_a + f32(k_a) * spacing_a, one multiply, one add."""
    axes = [F32(origin[a]) + np.arange(shape[a]).astype(F32) * F32(spacing[a]) for a in range(3)]
    g = np.meshgrid(*axes, indexing="ij")
    return np.stack([a.reshape(-1) for a in g], axis=1).astype(F32)


def pair_weight(p, x, m_V, inv_h, k_w):
    """(contributes, w) for positions p [P, 1, 3] against particles x [1, N, 3], m_V [1, N]: the contract's f32 sequence."""
    inv_h, k_w = F32(inv_h), F32(k_w)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[..., 0] - x[..., 0], p[..., 1] - x[..., 1], p[..., 2] - x[..., 2]
        r2 = (dx * dx + dy * dy) + dz * dz
        r = np.sqrt(r2)
        q = r * inv_h
        assert q.dtype == F32
        inside = q <= F32(1)                                   # False for a NaN
        q2 = q * q
        q3 = q2 * q
        inner = k_w * ((F32(6) * q3 - F32(6) * q2) + F32(1))
        t = F32(1) - q
        outer = (k_w * F32(2)) * ((t * t) * t)
        W = np.where(q <= F32(0.5), inner, outer)
        w = np.fmin(np.fmax(m_V * W, F32(0)), F32(4))          # fmaxf / fminf: a NaN operand yields the other one
        assert w.dtype == F32
    return inside, w


def select(material, object_id, want_material=1, objects=()):
    sel = np.ones(material.shape[0], dtype=bool)
    if want_material is not None and want_material >= 0:
        sel &= material == want_material
    if len(objects):
        sel &= np.isin(object_id, np.asarray(list(objects)))
    return sel


def sample(positions, x, m_V, values, selected, inv_h, k_w, chunk=512):
    """positions f32 [P, 3]; x f32 [N, 3]; m_V f32 [N]; values: list of f32 [N] (one per requested plane); selected bool [N].
    Returns {"count": i64 [P], "weight": i64 [P], "sums": i64 [F, P]}."""
    positions = np.asarray(positions, dtype=F32).reshape(-1, 3)
    sel = np.asarray(selected, dtype=bool)
    x = np.asarray(x, dtype=F32)[sel]
    m_V = np.asarray(m_V, dtype=F32)[sel]
    with np.errstate(invalid="ignore"):
        vals = [np.fmax(np.fmin(np.asarray(v, dtype=F32)[sel], LIMIT), -LIMIT).astype(np.float64) for v in values]
    P = positions.shape[0]
    count, weight = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    sums = np.zeros((len(vals), P), dtype=np.int64)
    # a particle further than h (with a margin far above every rounding) from the chunk's bounding box cannot contribute: the
    # chunk then meets fewer particles.  This is a property of the pair rule (q <= 1), not of any footprint arithmetic.
    reach = 1.001 / float(inv_h) + 1e-6
    finite = np.isfinite(x).all(axis=1)
    for c0 in range(0, P, chunk):
        p = positions[c0:c0 + chunk]
        lo, hi = p.min(axis=0).astype(np.float64) - reach, p.max(axis=0).astype(np.float64) + reach
        with np.errstate(invalid="ignore"):
            near = finite & (x >= lo).all(axis=1) & (x <= hi).all(axis=1)
        if not near.any():
            continue
        inside, w = pair_weight(p[:, None, :], x[near][None, :, :], m_V[near][None, :], inv_h, k_w)
        w64 = np.where(inside, w, F32(0)).astype(np.float64)
        count[c0:c0 + chunk] = inside.sum(axis=1)
        weight[c0:c0 + chunk] = np.rint(w64 * SCALE).astype(np.int64).sum(axis=1)
        for f, v in enumerate(vals):
            sums[f, c0:c0 + chunk] = np.where(inside, np.rint((w64 * v[near][None, :]) * SCALE), 0.0).astype(np.int64).sum(axis=1)
    return {"count": count, "weight": weight, "sums": sums}


def planes_of(fields):
    """Plane names of user-level fields, in plane order."""
    out = []
    if "velocity" in fields:
        out += ["vx", "vy", "vz"]
    if "density" in fields:
        out.append("density")
    if "pressure" in fields:
        out.append("pressure")
    return tuple(out)


def values_of(planes, v, density, pressure):
    src = {"vx": v[:, 0], "vy": v[:, 1], "vz": v[:, 2], "density": density, "pressure": pressure}
    return [np.asarray(src[p], dtype=F32) for p in planes]
