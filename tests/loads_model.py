"""Numpy model of the fluid loads (include/sph_hip.h, section "Fluid loads"): BRUTE FORCE over all fluid x target pairs, no cells,
with the contract's arithmetic term by term -- the pair geometry in f32, the coefficient and the components in f64 (IEEE multiply,
divide, subtract: numpy's are the device's), the clamps, np.rint (to nearest even, like llrint) and integer sums.  Being cell-free it
also checks the kernel's walk over the 27 cells.  Returns the nine integers per object.
"""
import numpy as np

F32 = np.float32
SCALE = float(1 << 24)
F_LIMIT = 65536.0
T_LIMIT = float(1 << 40)
WORDS = 9


def k_dw(support_radius):
    """The context's folded constant as the Python layer hands it to the library: f32(6 * 8 / (pi h^3)) (sph_base.py:50-57)."""
    return F32(6.0 * (8 / np.pi) / float(support_radius) ** 3)


def pair_terms(xi, xj, m_Vj, m, rho, p, support_radius, rho0, k_dw_):
    """xi [I, 3], m, rho, p [I] of the fluid; xj [J, 3], m_Vj [J] of the targets, all f32.  Returns (accept bool [J, I], terms i64
    [J, I, 3], saturated i64 [J, I]): what each pair adds to F_j."""
    h32 = F32(support_radius)
    inv_h = F32(1) / h32
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = xi[None, :, :] - xj[:, None, :]                                   # f32: d = x_i - x_j
        r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        r = np.sqrt(r2)
        q = r * inv_h
        assert d.dtype == r.dtype == q.dtype == F32
        accept = (q <= F32(1.0)) & (r > F32(1e-5))
        q64, r64 = q.astype(np.float64), r.astype(np.float64)
        g = np.where(q <= F32(0.5), q64 * (3.0 * q64 - 2.0), -((1.0 - q64) * (1.0 - q64)))
        m64, rho64, p64 = (np.asarray(a, dtype=F32).astype(np.float64)[None, :] for a in (m, rho, p))
        rho0_64, kdw64, h64 = float(F32(rho0)), float(F32(k_dw_)), float(h32)
        dp = p64 / (rho64 * rho64) + p64 / (rho0_64 * rho0_64)
        coef = (((m64 * rho0_64) * m_Vj.astype(np.float64)[:, None]) * dp) * ((kdw64 * g) / (r64 * h64))
        f = coef[..., None] * d.astype(np.float64)
        cl = np.fmin(np.fmax(f, -F_LIMIT), F_LIMIT)                           # a NaN ends at -2^16, like fmin(fmax()) on the device
        sat = (cl != f).sum(axis=-1)
        terms = np.rint(cl * SCALE).astype(np.int64)
    terms = np.where(accept[..., None], terms, 0)
    return accept, terms, np.where(accept, sat, 0).astype(np.int64)


def sample(x, m_V, material, object_id, m, rho, p, objects, about, support_radius, rho0, k_dw_=None, chunk=256):
    """The nine integers [len(objects), 9] of one sample of the state (arrays in any common order): x f32 [N, 3]; m_V, m, rho (density),
    p (pressure) f32 [N]; material, object_id int [N]."""
    x = np.asarray(x, dtype=F32)
    m_V = np.asarray(m_V, dtype=F32)
    k_dw_ = k_dw(support_radius) if k_dw_ is None else k_dw_
    fluid = np.asarray(material) == 1
    xi, mi, ri, pi = x[fluid], np.asarray(m, F32)[fluid], np.asarray(rho, F32)[fluid], np.asarray(p, F32)[fluid]
    c = np.asarray(about, dtype=F32)
    out = np.zeros((len(objects), WORDS), dtype=np.int64)
    for slot, oid in enumerate(objects):
        tgt = np.nonzero((np.asarray(material) == 0) & (np.asarray(object_id) == oid))[0]
        for at in range(0, tgt.size, chunk):
            j = tgt[at:at + chunk]
            accept, terms, sat = pair_terms(xi, x[j], m_V[j], mi, ri, pi, support_radius, rho0, k_dw_)
            F = terms.sum(axis=1)                                             # i64 [J, 3]: the integer force of each target
            pairs = accept.sum(axis=1).astype(np.int64)
            a = (x[j] - c[None, :]).astype(np.float64)                        # the subtraction in f32
            Fd = F.astype(np.float64) / SCALE
            T = np.stack([a[:, 1] * Fd[:, 2] - a[:, 2] * Fd[:, 1], a[:, 2] * Fd[:, 0] - a[:, 0] * Fd[:, 2],
                          a[:, 0] * Fd[:, 1] - a[:, 1] * Fd[:, 0]], axis=1)
            ts = T * SCALE
            tc = np.fmin(np.fmax(ts, -T_LIMIT), T_LIMIT)
            out[slot, 0:3] += F.sum(axis=0)
            out[slot, 3:6] += np.rint(tc).astype(np.int64).sum(axis=0)
            out[slot, 6] += pairs.sum()
            out[slot, 7] += (pairs > 0).sum()
            out[slot, 8] += sat.sum() + (tc != ts).sum()
    return out


def pair_magnitude(x, m_V, material, object_id, m, rho, p, objects, support_radius, rho0, k_dw_=None):
    """sum over all contributing pairs of |f| (f64, in N): what a momentum-balance residual is normalised by."""
    x = np.asarray(x, dtype=F32)
    k_dw_ = k_dw(support_radius) if k_dw_ is None else k_dw_
    fluid = np.asarray(material) == 1
    tgt = (np.asarray(material) == 0) & np.isin(np.asarray(object_id), list(objects))
    _, terms, _ = pair_terms(x[fluid], x[tgt], np.asarray(m_V, F32)[tgt], np.asarray(m, F32)[fluid], np.asarray(rho, F32)[fluid],
                             np.asarray(p, F32)[fluid], support_radius, rho0, k_dw_)
    return float(np.sqrt(((terms.astype(np.float64) / SCALE) ** 2).sum(axis=-1)).sum())
