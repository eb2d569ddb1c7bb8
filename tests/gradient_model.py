"""A numpy model of the gradient sums of the field sampling (include/sph_hip.h, "Field sampling: gradients"), beside the model of
the base planes in tests/sample_model.py, whose pair weight it imports: the f32 operations of the gradient term one by one
(np.float32 throughout; np.sqrt and the division on f32 are correctly rounded), the terms as f64 products rounded with np.rint,
the sums in int64.  Brute force over (position, particle) pairs, in chunks of positions: it knows nothing of footprints, tiles,
LDS chunks or particle order.
"""
import numpy as np

from tests import sample_model as model

F32 = model.F32
SCALE = model.SCALE
LIMIT = model.LIMIT


def pair_gradient(p, x, m_V, inv_h, k_w):
    """(contributes, w, g) for positions p [P, 1, 3] against particles x [1, N, 3], m_V [1, N]: `contributes` and `w` are
    sample_model.pair_weight's; g is f32 [P, N, 3], the contract's g_b = u * e_b, computed from the same dx, dy, dz, r, q."""
    inv_h, k_w = F32(inv_h), F32(k_w)
    inside, w = model.pair_weight(p, x, m_V, inv_h, k_w)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = [p[..., b] - x[..., b] for b in range(3)]
        r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        r = np.sqrt(r2)
        q = r * inv_h
        inner = (k_w * F32(6)) * (q * (F32(3) * q - F32(2)))
        t = F32(1) - q
        outer = (k_w * F32(6)) * (-(t * t))
        D = np.where(q <= F32(0.5), inner, outer)
        u = np.fmax(np.fmin(m_V * D, F32(0)), F32(-8))               # fminf / fmaxf: a NaN operand yields the other one
        assert u.dtype == F32 and r.dtype == F32
        pos = r > F32(0)
        g = np.stack([u * np.where(pos, d[b] / np.where(pos, r, F32(1)), F32(0)) for b in range(3)], axis=-1)
        assert g.dtype == F32
    return inside, w, g


def sample(positions, x, m_V, values, grad_of, selected, inv_h, k_w, chunk=512):
    """positions f32 [P, 3]; x f32 [N, 3]; m_V f32 [N]; values: list of f32 [N], one per requested plane; grad_of: indices into
    `values` of the planes whose gradient sums are wanted, in plane order; selected bool [N].
    Returns sample_model.sample's {"count", "weight", "sums"} plus "grad_fill": i64 [3, P] and "grad_sums": i64 [len(grad_of), 3, P]."""
    positions = np.asarray(positions, dtype=F32).reshape(-1, 3)
    base = model.sample(positions, x, m_V, values, selected, inv_h, k_w, chunk=chunk)
    sel = np.asarray(selected, dtype=bool)
    x = np.asarray(x, dtype=F32)[sel]
    m_V = np.asarray(m_V, dtype=F32)[sel]
    with np.errstate(invalid="ignore"):
        vals = [np.fmax(np.fmin(np.asarray(values[f], dtype=F32)[sel], LIMIT), -LIMIT).astype(np.float64) for f in grad_of]
    P = positions.shape[0]
    grad_fill = np.zeros((3, P), dtype=np.int64)
    grad_sums = np.zeros((len(vals), 3, P), dtype=np.int64)
    reach = 1.001 / float(inv_h) + 1e-6                                # as in sample_model.sample: a property of q <= 1
    finite = np.isfinite(x).all(axis=1)
    for c0 in range(0, P, chunk):
        p = positions[c0:c0 + chunk]
        lo, hi = p.min(axis=0).astype(np.float64) - reach, p.max(axis=0).astype(np.float64) + reach
        with np.errstate(invalid="ignore"):
            near = finite & (x >= lo).all(axis=1) & (x <= hi).all(axis=1)
        if not near.any():
            continue
        inside, _, g = pair_gradient(p[:, None, :], x[near][None, :, :], m_V[near][None, :], inv_h, k_w)
        g64 = np.where(inside[..., None], g, F32(0)).astype(np.float64)
        for b in range(3):
            grad_fill[b, c0:c0 + chunk] = np.rint(g64[..., b] * SCALE).astype(np.int64).sum(axis=1)
            for k, v in enumerate(vals):
                grad_sums[k, b, c0:c0 + chunk] = np.where(inside, np.rint((g64[..., b] * v[near][None, :]) * SCALE), 0.0).astype(np.int64).sum(axis=1)
    return dict(base, grad_fill=grad_fill, grad_sums=grad_sums)


def grad_indices(planes, grad_planes):
    """Indices into `planes` of `grad_planes`, which must be in plane order."""
    idx = [planes.index(p) for p in grad_planes]
    assert idx == sorted(idx)
    return idx
