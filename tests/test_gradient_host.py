"""Host side of the sampled gradients (no GPU): the C ABI additions and their ctypes mirror, the numpy model of the gradient sums
(tests/gradient_model.py) against sums written out by hand, the derived views of `FieldGrid` / `FieldProbes` (consistency with
central differences of the interpolant, accuracy on a linear field, the surface normal), the argument errors, the scene keys and
the VTK writer.

Every bound below that is not exact was MEASURED with the integer model on the CPU and is at most three times the figure
written next to it."""
import ctypes
import os
import re

import numpy as np
import pytest

from sph_taichi_amd import _lib, build, sample
from sph_taichi_amd.config_builder import SimConfig
from tests import gradient_model as gm
from tests import sample_model as model
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
F32 = np.float32
TWO30 = 2.0 ** 30


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    ctx, ws = r"SphContext\s*\*\s*\w*", r"\s*"
    decls = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)                       # the declarations without their comments
    assert re.search(rf"int32_t\s+sph_sample_grid_gradients\s*\({ws}{ctx}{ws},{ws}const\s+SphSampleGrid\s*\*\s*\w*{ws},{ws}int32_t\s+\w+{ws}\)\s*;", decls)
    assert re.search(rf"int32_t\s+sph_sample_grid_gradients_download\s*\({ws}{ctx}{ws},{ws}int64_t\s*\*\s*\w*{ws},{ws}int64_t\s+\w+{ws}\)\s*;", decls)
    assert re.search(rf"int32_t\s+sph_sample_points_gradients\s*\({ws}{ctx}{ws},{ws}const\s+float\s*\*\s*\w*{ws},{ws}int32_t\s+\w+{ws},{ws}int32_t\s+\w+{ws},"
                     rf"{ws}int32_t\s+\w+{ws},{ws}const\s+SphSampleSelect\s*\*\s*\w*{ws},{ws}float\s+\w+{ws}\)\s*;", decls)
    assert re.search(rf"int32_t\s+sph_sample_points_gradients_download\s*\({ws}{ctx}{ws},{ws}int64_t\s*\*\s*\w*{ws},{ws}int32_t\s+\w+{ws}\)\s*;", decls)
    assert re.search(r"#define\s+SPH_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6          # additive: the version stays
    section = HEADER[HEADER.index("Field sampling: gradients"):HEADER.index("Surface mesh (")]
    for word in ("2^55", "2^57", "2^8 - 1", "2^6 - 1", "r == 0", "DIMENSIONLESS", "not in `fields`", "carried no gradients", "cubic_kernel_derivative"):
        assert word in section, word
    assert HEADER.index("Field sampling: gradients") > HEADER.index("sph_sample_points_download")


def test_binding_and_layouts():
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = {"sph_sample_grid_gradients": [vp, ctypes.POINTER(_lib.SphSampleGrid), i32],
            "sph_sample_grid_gradients_download": [vp, vp, i64],
            "sph_sample_points_gradients": [vp, vp, i32, i32, i32, ctypes.POINTER(_lib.SphSampleSelect), ctypes.c_float],
            "sph_sample_points_gradients_download": [vp, vp, i32]}
    for name, args in want.items():
        assert name in bound and bound[name][0] is i32 and bound[name][1] == args, name
    assert ctypes.sizeof(_lib.SphSampleSelect) == 136 and ctypes.sizeof(_lib.SphSampleGrid) == 44 + 136      # unchanged
    assert _lib.SAMPLE_MAX_CHANNELS == 25
    assert "sph_sample.hip" in build.SOURCES


# ---- the model against sums computed by hand --------------------------------------------------------------------------------
# The lattice of test_sample_host.py: d = 2^-5, h = 4 d = 2^-3, every coordinate exact in f32, inv_h = 8.
D = 2.0 ** -5
H = 4 * D
KW = model.k_w(H)
MV = F32(0.8 * D ** 3)


def _lattice(n):
    k = np.arange(n, dtype=np.float64) * D
    return np.stack([a.reshape(-1) for a in np.meshgrid(k, k, k, indexing="ij")], axis=1).astype(F32)


def _scalar_g(p, xj, m_V=MV, inv_h=F32(8), k_w=KW):
    """(g_x, g_y, g_z) of one pair as scalar f32 steps, or None when it does not contribute (independent of the model's arrays)."""
    d = [F32(F32(p[b]) - F32(xj[b])) for b in range(3)]
    r2 = F32(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2]))
    r = F32(np.sqrt(r2))
    q = F32(r * inv_h)
    if not q <= F32(1):
        return None
    k6 = F32(k_w * F32(6))
    if q <= F32(0.5):
        Dq = F32(k6 * F32(q * F32(F32(F32(3) * q) - F32(2))))
    else:
        t = F32(F32(1) - q)
        Dq = F32(k6 * F32(-F32(t * t)))
    u = max(min(F32(m_V * Dq), F32(0)), F32(-8))
    return [F32(u * F32(d[b] / r)) if r > 0 else F32(0) for b in range(3)]


def _hand(p, x, a):
    """count, G [3], S [3] of one position over all particles, one field a [N]: integer sums of the rounded f64 terms."""
    cnt, G, S = 0, [0, 0, 0], [0, 0, 0]
    for j in range(x.shape[0]):
        g = _scalar_g(p, x[j])
        if g is None:
            continue
        cnt += 1
        for b in range(3):
            G[b] += int(np.rint(float(g[b]) * TWO30))
            S[b] += int(np.rint((float(g[b]) * float(a[j])) * TWO30))
    return cnt, G, S


def test_model_equals_the_hand_sums_on_the_rest_lattice():
    x = _lattice(11)
    n = x.shape[0]
    a = (F32(0.5) + x[:, 0] * F32(3) - x[:, 2]).astype(F32)
    centre = np.array([5 * D, 5 * D, 5 * D], dtype=F32)                     # a lattice point: the neighbourhood is symmetric
    offset = np.array([5 * D + D / 4, 5 * D - 3 * D / 8, 5 * D + D / 8], dtype=F32)
    pts = np.stack([centre, offset])
    got = gm.sample(pts, x, np.full(n, MV), [a], [0], np.ones(n, bool), model.inv_h(H), KW)
    assert got["grad_fill"].shape == (3, 2) and got["grad_sums"].shape == (1, 3, 2) and got["grad_fill"].dtype == np.int64
    for k, p in enumerate(pts):
        cnt, G, S = _hand(p, x, a)
        assert got["count"][k] == cnt
        assert got["grad_fill"][:, k].tolist() == G and got["grad_sums"][0, :, k].tolist() == S, k
    assert got["count"][0] == 257 and got["grad_fill"][:, 0].tolist() == [0, 0, 0]          # exactly 0 by symmetry; r == 0 is in it
    assert all(got["grad_fill"][:, 1] != 0) and all(got["grad_sums"][0, [0, 2], 0] != 0)     # (the field does not vary along y)
    # the base planes are sample_model's
    base = model.sample(pts, x, np.full(n, MV), [a], np.ones(n, bool), model.inv_h(H), KW)
    for k in ("count", "weight", "sums"):
        assert np.array_equal(got[k], base[k])


def test_the_three_branches_of_q():
    x = np.array([[0.5, 0.5, 0.5]], dtype=F32)
    pts = np.array([[0.5, 0.5, 0.5],                      # q == 0, r == 0: counts, weighs, no gradient
                    [0.5 + H / 2, 0.5, 0.5],              # q == 0.5: the inner branch, D = -1.5 k_w, e = (1, 0, 0)
                    [0.5, 0.5 - H, 0.5],                  # q == 1: contributes, with D = -0
                    [0.5, 0.5, np.nextafter(F32(0.5 + H), F32(1))]], dtype=F32)   # just outside
    got = gm.sample(pts, x, np.array([MV]), [np.array([3.0], dtype=F32)], [0], np.ones(1, bool), model.inv_h(H), KW)
    assert got["count"].tolist() == [1, 1, 1, 0]
    g_half = F32(MV * F32(F32(KW * F32(6)) * F32(F32(0.5) * F32(F32(F32(3) * F32(0.5)) - F32(2)))))
    assert g_half == F32(MV * F32(F32(KW * F32(6)) * F32(-0.25))) and g_half < 0
    gx = int(np.rint(float(g_half) * TWO30))
    assert got["grad_fill"].tolist() == [[0, gx, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert got["grad_sums"][0].tolist() == [[0, int(np.rint(float(g_half) * 3.0 * TWO30)), 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    # the outer branch away from its zero: q = 0.75 along -z, D = -(6 k_w) / 16, e = (0, 0, -1)
    p = np.array([[0.5, 0.5, 0.5 - 3 * H / 4]], dtype=F32)
    got = gm.sample(p, x, np.array([MV]), [], [], np.ones(1, bool), model.inv_h(H), KW)
    g = F32(F32(MV * F32(F32(KW * F32(6)) * F32(-0.0625))) * F32(-1))
    assert g > 0 and got["grad_fill"][:, 0].tolist() == [0, 0, int(np.rint(float(g) * TWO30))]
    # a NaN volume counts with no gradient; a field beyond 2^24 clamps; the clamp of u at -8
    x3 = np.array([[0.5, 0.5, 0.5]] * 3, dtype=F32)
    got = gm.sample(pts[1:2], x3, np.array([MV, np.nan, 1.0], dtype=F32), [np.array([2.0 ** 25, 1.0, 1.0], dtype=F32)], [0], np.ones(3, bool),
                    model.inv_h(H), KW)
    assert F32(F32(1.0) * F32(F32(KW * F32(6)) * F32(-0.25))) < F32(-8)
    assert got["count"].tolist() == [3] and got["grad_fill"][:, 0].tolist() == [gx - 8 * (1 << 30), 0, 0]
    assert got["grad_sums"][0, :, 0].tolist() == [int(np.rint(float(g_half) * 2.0 ** 24 * TWO30)) - 8 * (1 << 30), 0, 0]


# ---- the derived views ------------------------------------------------------------------------------------------------------
PLANES4 = ("vx", "vy", "vz", "pressure")


def _probes(pts, x, v, prs, h, grad=PLANES4):
    n = x.shape[0]
    got = gm.sample(pts, x, np.full(n, MV), model.values_of(PLANES4, v, None, prs), gm.grad_indices(PLANES4, grad), np.ones(n, bool),
                    model.inv_h(h), model.k_w(h))
    return sample.FieldProbes(pts, got["weight"], got["count"], got["sums"], PLANES4, time=0.0, grad_fill=got["grad_fill"],
                              grad_sums=got["grad_sums"], grad_planes=grad, inv_h=float(model.inv_h(h)))


def test_gradient_is_the_derivative_of_the_interpolant():
    """A jittered lattice with a smooth velocity: velocity_gradient against central differences of the model's OWN velocity at
    p -+ eps per axis, eps = 2^-11 and every p a multiple of 2^-10 (p -+ eps exact in f32).  Measured: max |J - fd| = 2.8e-5 at
    max |J| = 3.1 (what remains is the f32 rounding of the weights divided by 2 eps, and eps^2 times the third derivative)."""
    rng = np.random.default_rng(11)
    x = (_lattice(13).astype(np.float64) + rng.uniform(-0.2, 0.2, (13 ** 3, 3)) * D).astype(F32)
    xd = x.astype(np.float64)
    v = np.stack([np.sin(3 * xd[:, 1]) + xd[:, 2] ** 2, np.cos(2 * xd[:, 0]) * xd[:, 2], xd[:, 0] * xd[:, 1] - np.sin(4 * xd[:, 2])], axis=1).astype(F32)
    prs = (1000 * xd[:, 1]).astype(F32)
    eps = 2.0 ** -11
    base = (np.round(rng.uniform(5 * D, 7 * D, (20, 3)) * 1024) / 1024).astype(F32)
    J = _probes(base, x, v, prs, H).velocity_gradient
    fd = np.zeros_like(J)
    for a in range(3):
        e = np.zeros(3, dtype=F32)
        e[a] = eps
        assert np.array_equal((base + e).astype(np.float64), base.astype(np.float64) + e)
        fd[:, :, a] = (_probes(base + e, x, v, prs, H, grad=()).velocity - _probes(base - e, x, v, prs, H, grad=()).velocity) / (2 * eps)
    err = np.abs(J - fd).max()
    print(f"max |J - fd| = {err:.3e}, max |J| = {np.abs(J).max():.3f}")
    assert np.abs(J).max() > 1.0
    assert err <= 7.5e-5                                                   # measured 2.8e-5


def test_a_linear_field_comes_back():
    """v = A x + b, p = c . x on the rest lattice at h = 2 d, 64 random interior positions (29 to 39 contributors each).  The
    errors are the lattice's discretisation error.  Measured with the integer model, relative to max |A| (max |c|):
    A 3.3 %, c 3.1 %, vorticity 4.9 %, divergence 3.4 %, strain rate 4.5 %; Q 5.9 % of max |A|^2."""
    h = 2 * D
    x = _lattice(11)
    xd = x.astype(np.float64)
    rng = np.random.default_rng(5)
    A, b, c = rng.uniform(-1, 1, (3, 3)), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3) * 100
    v, prs = (xd @ A.T + b).astype(F32), (xd @ c).astype(F32)
    pts = rng.uniform(3 * D, 7 * D, (64, 3)).astype(F32)
    pr = _probes(pts, x, v, prs, h)
    assert pr.count.min() >= 27 and pr.velocity_gradient.shape == (64, 3, 3) and pr.gradients == ("velocity", "pressure")
    top = np.abs(A).max()
    S, O = 0.5 * (A + A.T), 0.5 * (A - A.T)
    figures = {"A": (np.abs(pr.velocity_gradient - A).max() / top, 0.07),                                          # measured 0.033
               "c": (np.abs(pr.pressure_gradient - c).max() / np.abs(c).max(), 0.07),                              # 0.031
               "vorticity": (np.abs(pr.vorticity - np.array([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]])).max() / top, 0.10),   # 0.049
               "divergence": (np.abs(pr.divergence - np.trace(A)).max() / top, 0.07),                              # 0.034
               "strain_rate": (np.abs(pr.strain_rate - np.sqrt((S * S).sum())).max() / top, 0.09),                 # 0.045
               "q_criterion": (np.abs(pr.q_criterion - 0.5 * ((O * O).sum() - (S * S).sum())).max() / top ** 2, 0.12)}   # 0.059
    print({k: round(float(e), 4) for k, (e, _) in figures.items()})
    for name, (err, bound) in figures.items():
        assert err <= bound, (name, err)
    # (component, axis): row c of velocity_gradient is the gradient of v_c
    assert np.array_equal(pr.velocity_gradient[:, 1, :], pr._gradient("vy"))


def test_surface_normal_on_the_top_face():
    """Positions within half a spacing of the top face of the 11^3 block, in the middle of it in x and z, h = 4 d: the normal
    points along +y.  Measured: 1 - n_y <= 2.3e-6 (0.12 degrees), |n_x|, |n_z| <= 2.13e-3."""
    x = _lattice(11)
    rng = np.random.default_rng(7)
    top = 10 * D
    pts = np.concatenate([rng.uniform(4 * D, 6 * D, (32, 1)), rng.uniform(top - D / 2, top + D / 2, (32, 1)), rng.uniform(4 * D, 6 * D, (32, 1))], axis=1).astype(F32)
    n = x.shape[0]
    got = gm.sample(pts, x, np.full(n, MV), [], [], np.ones(n, bool), model.inv_h(H), KW)
    pr = sample.FieldProbes(pts, got["weight"], got["count"], got["sums"], (), time=0.0, grad_fill=got["grad_fill"], inv_h=float(model.inv_h(H)))
    nrm, fg = pr.surface_normal, pr.fill_gradient
    print(f"n_y min {nrm[:, 1].min():.7f}, max |n_x|, |n_z| {np.abs(nrm[:, [0, 2]]).max():.2e}")
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12) and (fg[:, 1] < 0).all()      # the fill falls upwards
    assert np.array_equal(fg, np.moveaxis(got["grad_fill"], 0, -1) * (float(model.inv_h(H)) / TWO30))
    assert nrm[:, 1].min() >= 1 - 6.9e-6 and np.abs(nrm[:, [0, 2]]).max() <= 6.3e-3
    assert pr.gradients == () and pr.grad_sums.shape == (0, 3, 32)
    with pytest.raises(ValueError, match="gradient of vx was not sampled"):
        pr.velocity_gradient
    with pytest.raises(ValueError, match="gradient of pressure was not sampled"):
        pr.pressure_gradient


def test_uniform_field_has_no_gradient_beyond_the_rounding():
    """Uniform v = a on the lattice of the existing uniform-velocity test: S_b = a G_b up to the llrints.  Each llrint errs by at
    most 1/2, so |S_b - a G_b| <= count (1 + |a|) / 2, and the interpolant itself errs by at most count (|a| + 1) / (2 weight):
    |gradient| <= inv_h (count / weight) max(|a|, 1) (1 + |G_b| / weight).  NaN where weight == 0."""
    x = _lattice(7)
    n = x.shape[0]
    v = np.tile(np.array([0.3, -1.7, 2.0 ** -9], dtype=F32), (n, 1))
    origin, spacing, shape = (-0.14, -0.13, -0.15), (0.033, 0.037, 0.041), (12, 11, 10)
    pos = model.node_positions(origin, spacing, shape)
    planes = ("vx", "vy", "vz")
    got = gm.sample(pos, x, np.full(n, MV), model.values_of(planes, v, None, None), [0, 1, 2], np.ones(n, bool), model.inv_h(H), KW)
    grid = sample.FieldGrid(got["weight"], got["count"], got["sums"], planes, time=0.25, origin=origin, spacing=spacing, shape=shape,
                            grad_fill=got["grad_fill"], grad_sums=got["grad_sums"], grad_planes=planes, inv_h=float(model.inv_h(H)))
    assert grid.grad_fill.shape == (3,) + shape and grid.grad_sums.shape == (3, 3) + shape and grid.gradients == ("velocity",)
    has = grid.weight > 0
    assert has.any() and not has.all()
    J = grid.velocity_gradient
    assert J.shape == shape + (3, 3)
    scale = grid.inv_h * grid.count[has] / grid.weight[has]
    for c in range(3):
        for b in range(3):
            bound = scale * max(abs(float(v[0, c])), 1.0) * (1 + np.abs(grid.grad_fill[b][has]) / grid.weight[has])
            assert (np.abs(J[..., c, b][has]) <= bound).all(), (c, b)
    assert np.abs(J[grid.fill > 0.1]).max() < 1e-5 < np.abs(grid.fill_gradient[has]).max()       # and the bound is not vacuous where there is fluid
    for view in (J, grid.fill_gradient, grid.surface_normal, grid.vorticity, grid.divergence, grid.strain_rate, grid.q_criterion):
        assert np.isnan(view[~has]).all() and not np.isnan(view[has]).any()
    with pytest.raises(ValueError, match="gradient of pressure was not sampled"):
        grid.pressure_gradient
    with pytest.raises(ValueError, match="gradient of density was not sampled"):
        grid.density_gradient
    plain = sample.FieldGrid(got["weight"], got["count"], got["sums"], planes, time=0.25, origin=origin, spacing=spacing, shape=shape)
    assert plain.grad_fill is None and plain.grad_sums.shape == (0, 3) + shape and plain.gradients == ()
    for name in ("fill_gradient", "surface_normal", "velocity_gradient", "vorticity", "divergence", "strain_rate", "q_criterion"):
        with pytest.raises(ValueError, match="was not sampled"):
            getattr(plain, name)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_gradient_argument_errors():
    assert sample.gradient_args() == {"names": (), "planes": (), "mask": 0, "any": False}
    assert sample.gradient_args(("fill",), ()) == {"names": (), "planes": (), "mask": 0, "any": True}
    assert sample.gradient_args(("pressure", "velocity"), ("velocity", "density", "pressure")) == \
        {"names": ("velocity", "pressure"), "planes": ("vx", "vy", "vz", "pressure"), "mask": 7 | 16, "any": True}
    assert sample.gradient_args(["density", "fill"], ("density",))["mask"] == 8
    for bad, msg in ((dict(gradients="velocity"), "not one string"), (dict(gradients=("speed",)), "unknown gradient"),
                     (dict(gradients=("velocity", "velocity")), "twice"), (dict(gradients=("fill", "fill")), "twice"),
                     (dict(gradients=("pressure",)), "name it in fields"), (dict(gradients=("velocity",), fields=("density",)), "name it in fields")):
        with pytest.raises(ValueError, match=msg):
            sample.gradient_args(**bad)
    with pytest.raises(ValueError, match="needs the sums"):
        sample.FieldProbes([[0, 0, 0]], [1], [1], [[1]], ("vx",), time=0.0, grad_fill=[[0], [0], [0]], grad_sums=[[[0], [0], [0]]], grad_planes=("vy",), inv_h=8.0)
    with pytest.raises(ValueError, match="inv_h"):
        sample.FieldProbes([[0, 0, 0]], [1], [1], [[1]], ("vx",), time=0.0, grad_fill=[[0], [0], [0]])


def _config(**keys):
    sd = scenes.fluid_only(counts=(3, 3, 3))
    sd["Configuration"].update(keys)
    return SimConfig(config=sd)


def test_driver_scene_keys():
    assert "gradients" in sample.GRID_CONFIG_KEYS and "gradients" in sample.PROBES_CONFIG_KEYS
    kw = sample.sample_grid_config(_config(sampleGrid={"fields": ["velocity", "pressure"], "gradients": ["velocity"]}))
    assert kw == {"spacing": None, "origin": None, "shape": None, "fields": ("velocity", "pressure"), "objects": None, "gradients": ("velocity",)}
    assert sample.sample_grid_config(_config(sampleGrid={"gradients": []}))["gradients"] == ()
    assert "gradients" not in sample.sample_grid_config(_config(sampleGrid={}))
    for bad, msg in (({"gradients": "velocity"}, "gradients must be a list of names"), ({"gradients": ["speed"]}, "unknown gradient"),
                     ({"gradients": ["pressure"]}, "name it in fields"), ({"gradients": ["velocity", "velocity"]}, "twice")):
        with pytest.raises(ValueError, match=f'"sampleGrid".*{msg}'):
            sample.sample_grid_config(_config(sampleGrid=bad))
    kw = sample.probes_config(_config(probes={"points": [[0.5, 0.25, 0.125]], "fields": ["pressure"], "gradients": ["pressure", "fill"]}))
    assert kw == {"points": [[0.5, 0.25, 0.125]], "fields": ("pressure",), "gradients": ("pressure", "fill")}
    assert "gradients" not in sample.probes_config(_config(probes={"points": [[0.5, 0.25, 0.125]]}))
    for bad, msg in (({"gradients": "fill"}, "gradients must be a list of names"), ({"gradients": ["density"]}, "name it in fields"),
                     ({"gradients": ["mass"]}, "unknown gradient")):
        with pytest.raises(ValueError, match=f'"probes".*{msg}'):
            sample.probes_config(_config(probes={"points": [[0, 0, 0]], **bad}))


def test_probe_rows_carry_the_gradient_fields():
    # one wet point with S = (2, 0, 0) 2^28 for vx, G = 0 and weight 2^29: d vx / dx = inv_h * 2^29 / 2^29
    z = [0, 0]
    pr = sample.FieldProbes([[0.5, 0.25, 0.125], [9, 9, 9]], [1 << 29, 0], [3, 0], [[1 << 28, 0], z, z, [5 << 29, 0]], ("vx", "vy", "vz", "pressure"), time=1.5,
                            grad_fill=[[-(1 << 30), 0], z, z], grad_sums=[[[0, 0], z, z], [z, z, z], [z, z, z], [z, [1 << 29, 0], z]],
                            grad_planes=("vx", "vy", "vz", "pressure"), inv_h=8.0)
    rows = pr.rows()
    assert list(rows[0]) == ["point", "count", "fill", "velocity", "pressure", "fill_gradient", "vorticity", "divergence", "q_criterion", "pressure_gradient"]
    assert rows[0]["fill_gradient"] == [-8.0, 0.0, 0.0] and rows[0]["velocity"] == [0.5, 0.0, 0.0]
    # grad vx = inv_h (0 - 0.5 * (-2^30)) / 2^29 = 8;  grad p = inv_h ((0, 2^29, 0) - 5 * (-2^30, 0, 0)) / 2^29 = (80, 8, 0)
    assert rows[0]["divergence"] == 8.0 and rows[0]["vorticity"] == [0.0, 0.0, 0.0] and rows[0]["q_criterion"] == -32.0
    assert rows[0]["pressure_gradient"] == [80.0, 8.0, 0.0]
    assert pr.surface_normal[0].tolist() == [1.0, 0.0, 0.0] and pr.strain_rate[0] == 8.0
    assert rows[1]["fill_gradient"] == [None] * 3 and rows[1]["divergence"] is None and rows[1]["pressure_gradient"] == [None] * 3
    plain = sample.FieldProbes([[0.5, 0.25, 0.125]], [1 << 29], [3], [[1 << 28]], ("vx",), time=1.5)
    assert list(plain.rows()[0]) == ["point", "count", "fill"]


# ---- the VTK writer -----------------------------------------------------------------------------------------------------------
def _vtk_bytes_as_before(grid):
    """The file the writer made before gradients existed: its array order (fill, then the fields) rebuilt here."""
    order = lambda a: np.ascontiguousarray(np.transpose(a, (2, 1, 0) + tuple(range(3, a.ndim))))
    arrays = [("fill", 1, order(grid.fill).astype(F32))]
    for name in grid.fields:
        arrays.append((name, 3 if name == "velocity" else 1, order(getattr(grid, name)).astype(F32)))
    n = grid.shape[0] * grid.shape[1] * grid.shape[2]
    head = ["# vtk DataFile Version 3.0", f"sph_taichi_amd field grid, time {grid.time!r}", "BINARY", "DATASET STRUCTURED_POINTS",
            "DIMENSIONS {} {} {}".format(*grid.shape), "ORIGIN {!r} {!r} {!r}".format(*grid.origin),
            "SPACING {!r} {!r} {!r}".format(*grid.spacing), f"POINT_DATA {n}"]
    out = ("\n".join(head) + "\n").encode("ascii")
    for name, comps, a in arrays:
        out += (f"VECTORS {name} float\n" if comps == 3 else f"SCALARS {name} float 1\nLOOKUP_TABLE default\n").encode("ascii")
        out += a.astype(">f4").tobytes() + b"\n"
    return out


def test_write_vtk(tmp_path):
    shape = (2, 3, 4)
    rng = np.random.default_rng(5)
    weight = rng.integers(0, 1 << 30, size=shape)
    weight[0, 1, 2] = 0
    planes = ("vx", "vy", "vz", "density", "pressure")
    sums = rng.integers(-(1 << 31), 1 << 31, size=(5,) + shape)
    geom = dict(time=0.5, origin=(0.1, -0.2, 0.3), spacing=(0.02, 0.04, 0.01), shape=shape)
    plain = sample.FieldGrid(weight, (weight > 0) * 7, sums, planes, **geom)
    plain.write_vtk(tmp_path / "plain.vtk")
    assert (tmp_path / "plain.vtk").read_bytes() == _vtk_bytes_as_before(plain)                  # without gradients: the bytes as they were
    grad = sample.FieldGrid(weight, (weight > 0) * 7, sums, planes, **geom, grad_fill=rng.integers(-(1 << 29), 1 << 29, size=(3,) + shape),
                            grad_sums=rng.integers(-(1 << 31), 1 << 31, size=(5, 3) + shape), grad_planes=planes, inv_h=12.5)
    grad.write_vtk(tmp_path / "grad.vtk")
    raw = (tmp_path / "grad.vtk").read_bytes()
    before = _vtk_bytes_as_before(grad)
    assert raw.startswith(before)                                                                   # appended AFTER today's arrays
    rest = raw[len(before):]
    order = lambda a: np.transpose(a, (2, 1, 0) + tuple(range(3, a.ndim)))
    for name, comps in (("fill_gradient", 3), ("vorticity", 3), ("divergence", 1), ("q_criterion", 1), ("pressure_gradient", 3), ("density_gradient", 3)):
        label = (f"VECTORS {name} float\n" if comps == 3 else f"SCALARS {name} float 1\nLOOKUP_TABLE default\n").encode("ascii")
        assert rest.startswith(label), (name, rest[:40])
        body = np.frombuffer(rest[len(label):len(label) + 24 * comps * 4], dtype=">f4").reshape((4, 3, 2) + ((3,) if comps == 3 else ()))
        assert np.array_equal(body, order(getattr(grad, name)).astype(F32), equal_nan=True), name
        assert np.isnan(body[2, 1, 0]).all() and not np.isnan(body).all()
        assert rest[len(label) + body.nbytes:][:1] == b"\n"
        rest = rest[len(label) + body.nbytes + 1:]
    assert rest == b""
    assert [n for n, _, _ in grad.vtk_arrays()] == ["fill", "velocity", "density", "pressure", "fill_gradient", "vorticity", "divergence", "q_criterion",
                                                    "pressure_gradient", "density_gradient"]
    only_fill = sample.FieldGrid(weight, (weight > 0) * 7, sums[:3], planes[:3], **geom, grad_fill=grad.grad_fill, inv_h=12.5)
    assert [n for n, _, _ in only_fill.vtk_arrays()] == ["fill", "velocity", "fill_gradient"]
