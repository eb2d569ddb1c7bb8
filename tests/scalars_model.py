"""Numpy model of the carried scalars (include/sph_hip.h, section "Carried scalars"): BRUTE FORCE over all carrier x participant
pairs, no cells, with the contract's arithmetic term by term -- the pair geometry in f32, the weights in f64 (IEEE multiply, add,
divide: numpy's are the device's), np.rint (to nearest even, like llrint) and integer sums.  Being cell-free it also checks the
kernel's walk over the 27 cells.  `sample_loop` is the same contract as a plain Python double loop, for the model's own test.
"""
import numpy as np

F32 = np.float32
ONE = float(1 << 32)
LIMIT = 1 << 52
NONE, CARRIER, SOURCE = 0, 1, 2


def k_dw(support_radius):
    """The context's folded constant as the Python layer hands it to the library: f32(6 * 8 / (pi h^3)) (sph_base.py:50-57)."""
    return F32(6.0 * (8 / np.pi) / float(support_radius) ** 3)


def to_raw(values):
    """i64 of f64 values: llrint(value * 2^32)."""
    return np.rint(np.asarray(values, dtype=np.float64) * ONE).astype(np.int64)


def roles(material, object_id, sel_material, sel_objects, sources):
    """int [N]: SOURCE where the object is a source, CARRIER where the record is selected (material -1 / None: any; no objects:
    all) and no source, NONE elsewhere."""
    material, object_id = np.asarray(material), np.asarray(object_id)
    sel = np.ones(material.shape[0], bool)
    if sel_material is not None and sel_material >= 0:
        sel &= material == sel_material
    if sel_objects:
        sel &= np.isin(object_id, list(sel_objects))
    src = np.isin(object_id, list(sources)) if len(sources) else np.zeros(material.shape[0], bool)
    return np.where(src, SOURCE, np.where(sel, CARRIER, NONE))


def coefficients(dt, every, kappa):
    """a_k = ((double)dt * every) * (double)kappa_k with dt and kappa f32."""
    return [(float(F32(dt)) * float(int(every))) * float(F32(k)) for k in kappa]


def snapshot(C, role, object_id, sources):
    """The snapshot in the records' order: C (i64 [N, K], the stored values of the records) with the prescribed raw values on the
    source records.  sources: {object id: row of K f64}."""
    snap = np.array(C, dtype=np.int64, copy=True)
    for oid, row in sources.items():
        snap[(role == SOURCE) & (np.asarray(object_id) == oid)] = to_raw(row)
    return snap


def pair_weights(xi, xj, m_Vj, a, support_radius, k_dw_):
    """xi [I, 3] targets, xj [J, 3], m_Vj [J] candidates, f32.  Returns (accept bool [I, J], w f64 [K, I, J])."""
    h32 = F32(support_radius)
    inv_h = F32(1) / h32
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = xi[:, None, :] - xj[None, :, :]                                   # f32: d = x_i - x_j
        r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        r = np.sqrt(r2)
        q = r * inv_h
        assert d.dtype == r.dtype == q.dtype == F32
        accept = (q <= F32(1.0)) & (r > F32(1e-5))
        q64, r64 = q.astype(np.float64), r.astype(np.float64)
        g = np.where(q <= F32(0.5), q64 * (3.0 * q64 - 2.0), -((1.0 - q64) * (1.0 - q64)))
        h = float(h32)
        kdw = float(F32(k_dw_))
        lap = ((2.0 * (kdw * g)) * r64) / (h * (r64 * r64 + (0.01 * h) * h))
        mV = np.asarray(m_Vj, dtype=F32).astype(np.float64)[None, :]
        w = np.stack([np.fmin(np.fmax((-(ak * mV)) * lap, 0.0), 1.0) for ak in a])      # a NaN gives 0, like fmin(fmax()) on the device
    return accept, w


def sample(x, m_V, role, snap, a, support_radius, k_dw_=None, chunk=128, detail=False):
    """One sample.  x f32 [N, 3], m_V f32 [N], role int [N], snap i64 [N, K] (see `snapshot`), a: K coefficients.  Returns (new i64
    [N, K]: the carriers' rows updated, every other row as in snap; overshoot i64 [K]; saturated i64 [K]) and, with `detail`, also
    (pairs i64 [N], lo, hi i64 [N, K]: min / max over each carrier's own and contributing snapshot values, wsum i64 [N, K])."""
    x = np.asarray(x, dtype=F32)
    m_V = np.asarray(m_V, dtype=F32)
    k_dw_ = k_dw(support_radius) if k_dw_ is None else k_dw_
    K = snap.shape[1]
    part = np.nonzero(role != NONE)[0]
    car = np.nonzero(role == CARRIER)[0]
    new = np.array(snap, dtype=np.int64, copy=True)
    over, sat = np.zeros(K, np.int64), np.zeros(K, np.int64)
    pairs = np.zeros(x.shape[0], np.int64)
    lo, hi = snap.copy(), snap.copy()
    wsum_all = np.zeros_like(snap)
    for at in range(0, car.size, chunk):
        i = car[at:at + chunk]
        accept, w = pair_weights(x[i], x[part], m_V[part], a, support_radius, k_dw_)
        pairs[i] = accept.sum(axis=1)
        for k in range(K):
            diff = (snap[part, k][None, :] - snap[i, k][:, None]).astype(np.float64)      # exact: both within 2^52
            term = np.where(accept, np.rint(diff * w[k]).astype(np.int64), 0)
            wk = np.where(accept, np.rint(w[k] * ONE).astype(np.int64), 0)
            v = snap[i, k] + term.sum(axis=1)
            cl = np.clip(v, -LIMIT, LIMIT)
            new[i, k] = cl
            wsum = wk.sum(axis=1)
            wsum_all[i, k] = wsum
            over[k] += int((wsum > (1 << 32)).sum())
            sat[k] += int((cl != v).sum())
            big = np.iinfo(np.int64).max
            lo[i, k] = np.minimum(snap[i, k], np.where(accept, snap[part, k][None, :], big).min(axis=1, initial=big))
            hi[i, k] = np.maximum(snap[i, k], np.where(accept, snap[part, k][None, :], -big).max(axis=1, initial=-big))
    if detail:
        return new, over, sat, pairs, lo, hi, wsum_all
    return new, over, sat


def sample_loop(x, m_V, role, snap, a, support_radius, k_dw_=None):
    """The same sample as a plain double loop over Python scalars (numpy only for the f32 operations)."""
    import math
    x = np.asarray(x, dtype=F32)
    m_V = np.asarray(m_V, dtype=F32)
    k_dw_ = k_dw(support_radius) if k_dw_ is None else k_dw_
    h32 = F32(support_radius)
    inv_h = F32(1) / h32
    h, kdw = float(h32), float(F32(k_dw_))
    N, K = snap.shape
    new = [[int(v) for v in row] for row in snap]
    over, sat = [0] * K, [0] * K
    for i in range(N):
        if role[i] != CARRIER:
            continue
        s, ws = [0] * K, [0] * K
        for j in range(N):
            if role[j] == NONE:
                continue
            d = x[i] - x[j]
            r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            r = np.sqrt(r2)
            q = r * inv_h
            if not (q <= F32(1.0)) or not (r > F32(1e-5)):
                continue
            q64, r64 = float(q), float(r)
            g = q64 * (3.0 * q64 - 2.0) if q <= F32(0.5) else -((1.0 - q64) * (1.0 - q64))
            lap = ((2.0 * (kdw * g)) * r64) / (h * (r64 * r64 + (0.01 * h) * h))
            for k in range(K):
                w = (-(a[k] * float(m_V[j]))) * lap
                w = min(max(w, 0.0), 1.0) if not math.isnan(w) else 0.0
                s[k] += int(np.rint(float(int(snap[j, k]) - int(snap[i, k])) * w))
                ws[k] += int(np.rint(w * ONE))
        for k in range(K):
            v = int(snap[i, k]) + s[k]
            cl = max(min(v, LIMIT), -LIMIT)
            new[i][k] = cl
            over[k] += ws[k] > (1 << 32)
            sat[k] += cl != v
    return np.array(new, dtype=np.int64), np.array(over, dtype=np.int64), np.array(sat, dtype=np.int64)


def paint_index(raw, lo, hi):
    """The table index of raw i64 values: s = f32(f64(C) * 2^-32), then the field colouring's arithmetic (tests/fieldcolour_model.py)."""
    s = (np.asarray(raw, dtype=np.int64).astype(np.float64) * (1.0 / ONE)).astype(F32)
    with np.errstate(all="ignore"):
        inv = F32(1) / (F32(hi) - F32(lo))
        t = (s - F32(lo)) * inv
        t = np.where(t >= 0, np.minimum(t, F32(1)), F32(0))
        return (t * F32(255) + F32(0.5)).astype(np.int64)


# ---- the lattice of the formula test: a resting block, C = cos(pi x / L) along its long axis ------------------------------------
# Two things a first measurement on a 24 x 6 x 6 lattice at spacing d showed (decay rate 0.71 of the analytic one) and their causes:
#   * the library's fluid volume is m_V0 = 0.8 d^3, so a lattice at spacing d fills 0.8 of space and every volume sum comes out 0.8 x
#     (the header's "Field sampling" says the same of the Shepard sum); a fluid AT REST DENSITY sits at spacing d * 0.8^(1/3);
#   * a particle within h of a free face lacks neighbours, and the neighbours it lacks at (dx != 0, dy != 0) carry part of the second
#     derivative along x: the rate drops there although the mode has no gradient across the block.
# With the lattice at rest density and the amplitude taken over the CORE (three layers or more from the lateral faces, 0.056 > h)
# the rate is 0.982 of the analytic one: the discretisation error of Brookshaw's form at h = 4 r.
MODE_COUNTS, MODE_CORE, MODE_D = (24, 10, 10), 3, 0.02
MODE_KAPPA, MODE_EVERY, MODE_DT, MODE_SAMPLES = 1e-3, 50, 4e-4, 10


def lattice(counts=MODE_COUNTS, d=MODE_D, origin=0.1, core=MODE_CORE):
    """Cell-centred lattice at rest density, x = origin + (i + 1/2) s with s = d * 0.8^(1/3): for the insulated block of length
    L = counts[0] s the mode cos(pi x / L) is the lowest eigenmode of the Laplacian with zero flux at both ends.  Returns (x f32
    [N, 3], mode f64 [N], L, core bool [N])."""
    s = d * 0.8 ** (1.0 / 3.0)
    g = np.stack(np.meshgrid(*[np.arange(c) for c in counts], indexing="ij"), axis=-1).reshape(-1, 3)
    x = ((g + 0.5) * s + origin).astype(F32)
    L = counts[0] * s
    inner = np.all((g[:, 1:] >= core) & (g[:, 1:] < np.array(counts[1:]) - core), axis=1)
    return x, np.cos(np.pi * ((g[:, 0] + 0.5) * s) / L), L, inner


def mode_rate_error(raw, mode, core, L, t, kappa=MODE_KAPPA):
    """|ln(amplitude) / ln(exp(-kappa (pi / L)^2 t)) - 1| with the amplitude of raw i64 [N] projected on the mode over the core."""
    amp = float((np.asarray(raw, np.int64)[core].astype(np.float64) / ONE * mode[core]).sum() / (mode[core] * mode[core]).sum())
    return abs(np.log(amp) / (-kappa * (np.pi / L) ** 2 * t) - 1.0)


def mode_decay(n_samples=MODE_SAMPLES, m_V=None, k_dw_=None):
    """The formula test on the CPU: (relative error of the decay rate, raw i64 [N] after n samples, the coefficient a)."""
    x, mode, L, core = lattice()
    a = coefficients(MODE_DT, MODE_EVERY, [MODE_KAPPA])
    m_V = np.full(x.shape[0], F32(0.8 * MODE_D ** 3), F32) if m_V is None else np.asarray(m_V, F32)   # (the library's m_V0)
    role = np.full(x.shape[0], CARRIER)
    C = to_raw(mode)[:, None]
    for _ in range(n_samples):
        C, over, sat = sample(x, m_V, role, C, a, F32(2 * MODE_D), k_dw_)
        assert not over.any() and not sat.any()
    t = n_samples * float(F32(MODE_DT)) * MODE_EVERY
    return mode_rate_error(C[:, 0], mode, core, L, t), C[:, 0], a


# ---- the mixed scene of the stand-alone GPU test, shared with the host check of its caps -------------------------------------------
MIXED_SOURCES = {1: (350.0, 1.0, -5.0), 4: (0.0, 2.0, 7.0)}     # the static solid block and a fluid object
MIXED_CELL = (0.60, 0.60, 0.40)                                  # low corner of the crowded cell (cells are 0.04 wide)
VALUE_MAX = float(1 << 20)


def mixed_scene(seed=5):
    """Domain (1.0, 1.2, 0.8), d = 0.02: fluid object 0 in two blocks (the carriers) with a one-layer sheet of fluid object 2 (NOT
    selected) between them, fluid object 4 (a source) behind the second block and a static solid block (object 1, a source) under
    the first.  Of the first block's carriers 250 are crowded into ONE cell (runs of 15 trips and a ragged last one), six sit in the
    two corner cells of the domain and six outside it (clamped into border cells).  Returns (scene dict, arrays, values f64
    [N, 3] by particle index = persistent id before the first sort, index of the planted carrier)."""
    import copy
    from tests import scenes
    blk = lambda oid, start, counts, **kw: scenes._block(oid, start, scenes.lattice_end(start, counts), **kw)
    sd = {"Configuration": copy.deepcopy(scenes.BASE_CFG),
          "FluidBlocks": [blk(0, (0.20, 0.14, 0.20), (9, 9, 11)), blk(2, (0.38, 0.14, 0.20), (1, 9, 12)),
                          blk(0, (0.40, 0.14, 0.20), (7, 8, 12)), blk(4, (0.54, 0.14, 0.20), (3, 8, 12))],
          "RigidBlocks": [blk(1, (0.20, 0.10, 0.20), (10, 2, 12), isDynamic=False, color=(255, 255, 255))]}
    cfg, sc = scenes.build(sd)
    scenes.jitter(sc, 0.1, seed=seed)
    a = sc.arrays
    rng = np.random.default_rng(seed + 1)
    car = np.nonzero((a["material"] == 1) & (a["object_id"] == 0))[0]
    x = a["x"]
    crowd = car[:250]
    x[crowd] = (np.array(MIXED_CELL) + rng.uniform(0.002, 0.038, size=(250, 3))).astype(F32)
    x[car[250:256]] = np.array([[0.005, 0.006, 0.007], [0.03, 0.02, 0.01], [-0.01, 0.01, 0.02], [0.01, -0.02, 0.01], [0.02, 0.02, -0.005],
                                [0.035, 0.035, 0.035]], F32)
    x[car[256:262]] = np.array([[0.99, 1.19, 0.79], [0.97, 1.17, 0.78], [1.02, 1.21, 0.81], [1.01, 1.19, 0.79], [0.98, 1.22, 0.77],
                                [0.965, 1.165, 0.765]], F32)
    a["x_0"] = x.copy()
    n = x.shape[0]
    values = np.zeros((n, 3))
    values[:, 0] = 100.0 * x[:, 0].astype(np.float64)
    values[:, 1] = rng.uniform(-1.0, 1.0, n)
    values[:, 2] = rng.uniform(0.0, 10.0, n)
    values[car[700], 0] = VALUE_MAX                  # a value at the limit that diffuses away: no saturation without overshoot
    values[car[701], 0] = -VALUE_MAX
    values[crowd, 2] = VALUE_MAX                     # the crowded cell at +2^20 in the overshooting channel ...
    return sd, a, values, crowd


def mixed_kappa(a, values, crowd, h, dt):
    """(kappa, index of the planted carrier): kappa puts the largest weight sum of ANY carrier at 0.5 in channel 0 (so channels 0
    and 1 cannot overshoot) and 5 in channel 2 (10 kappa); the planted carrier is the crowded one with the largest weight sum."""
    role = roles(a["material"], a["object_id"], 1, [0], MIXED_SOURCES)
    snap = to_raw(values[:, :1])
    w = sample(a["x"], a["m_V"], role, snap, [1.0e-6], h, detail=True)[6][:, 0].astype(np.float64) / ONE / 1.0e-6   # weight sum per unit a
    planted = crowd[np.argmax(w[crowd])]
    return F32(0.5 / (w.max() * float(F32(dt)))), int(planted)
