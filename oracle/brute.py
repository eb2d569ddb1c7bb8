"""Independent O(N^2) NumPy restatement of one WCSPH step (no grid, no sort) and of the DFSPH neighbour sums.

TEST INFRASTRUCTURE ONLY.  Cross-checks oracle/sph_oracle.c's neighbour search:
the neighbour set here is { j != i : |x_i - x_j| < h } computed from a dense
distance matrix, so any mistake in the oracle's cell hashing / prefix sum /
27-cell traversal shows up as a difference.  Summation order differs from the
reference (row-wise pairwise sums), so comparisons use a ~1e-5 tolerance.

Formulas follow /root/reference: sph_base.py:23-68 (kernels), :91-113 (boundary
volume), :149-179 (walls), WCSPH.py:19-149 (density, forces, EOS, advect).
Valid when no particle sits in grid cell 0 (the reference never sees those as
neighbours, particle_system.py:384) and every particle is inside the domain.

dtype=np.float64 is the HIGH-PRECISION reference of the same operations: the f32 per-particle arrays and the f32 solver
scalars (density_0, stiffness, exponent, dt, g, surface_tension, domain) are promoted unchanged -- they are what the f32
kernels receive -- while everything folded from the radius (h, d, m_V0, k_w, k_dw, visc_eps, padding, wall_hi) and from
the viscosity (10 nu) is folded in f64 and stays there, and every product, power and sum is f64.  An f32 evaluation of
the same formulas (the C oracle, the HIP kernels) then differs from it by its own rounding error only.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32


def _W(r, h, k, ft=f32):
    q = r / ft(h)
    w1 = ft(k) * (ft(6.0) * q * q * q - ft(6.0) * q * q + ft(1.0))
    w2 = ft(k) * ft(2.0) * (ft(1.0) - q) ** 3
    return np.where(q <= ft(0.5), w1, np.where(q <= ft(1.0), w2, ft(0.0))).astype(ft)


def _gradW(rvec, rn, h, kd, ft=f32):
    q = rn / ft(h)
    with np.errstate(divide="ignore", invalid="ignore"):
        gq = rvec / (rn * ft(h))[..., None]
    c1 = ft(kd) * q * (ft(3.0) * q - ft(2.0))
    c2 = ft(kd) * (-(ft(1.0) - q) * (ft(1.0) - q))
    c = np.where(q <= ft(0.5), c1, c2)
    ok = (rn > ft(1e-5)) & (q <= ft(1.0))
    return np.where(ok[..., None], c[..., None] * gq, ft(0.0)).astype(ft)


class Brute:
    def __init__(self, params, arrays, dtype=np.float32):
        ft = self.ft = np.dtype(dtype).type
        if ft not in (np.float32, np.float64):
            raise ValueError("Brute: dtype must be np.float32 or np.float64")
        r = float(params["particle_radius"])
        self.d = 2 * r
        self.h = 4.0 * r
        self.m_V0 = 0.8 * self.d ** 3
        self.rho0 = ft(f32(params["density_0"]))
        self.stiffness = ft(f32(params["stiffness"]))
        self.exponent = ft(f32(params["exponent"]))
        self.dt = ft(f32(params["dt"]))
        self.g = np.asarray(params["g"], dtype=f32).astype(ft)
        self.k = 8 / np.pi / self.h ** 3
        self.kd = 6.0 * 8 / np.pi / self.h ** 3
        self.nu = float(params.get("viscosity", 0.01))
        self.sigma = float(params.get("surface_tension", 0.01))
        if ft is f32:
            self.dom = np.asarray(params["domain_size"], dtype=f32)
            self.pad = f32(self.h)
            self.wall_hi = self.dom - self.pad
        else:       # padding and wall_hi folded in f64 (the f32 sides round that fold once)
            self.dom = np.asarray(params["domain_size"], dtype=np.float64)
            self.pad = ft(self.h)
            self.wall_hi = self.dom - self.pad
        self.a = {k: np.array(v, copy=True) for k, v in arrays.items()}
        for name in ("x", "v", "acceleration"):
            self.a[name] = np.asarray(self.a.get(name, np.zeros((len(arrays["x"]), 3))), dtype=f32).astype(ft)
        for name in ("m_V", "m", "density", "pressure"):
            self.a[name] = np.asarray(self.a[name], dtype=f32).astype(ft)

    def set(self, name, value):
        """Replace one per-particle array by an f32 state (promoted unchanged)."""
        self.a[name] = np.array(value, dtype=f32).astype(self.ft)

    def _w(self, r):
        return _W(r, self.h, self.k, self.ft)

    def _gw(self, rvec, rn):
        return _gradW(rvec, rn, self.h, self.kd, self.ft)

    def _pairs(self):
        ft = self.ft
        x = self.a["x"]
        rvec = (x[:, None, :] - x[None, :, :]).astype(ft)
        rn = np.sqrt((rvec[..., 0] * rvec[..., 0] + rvec[..., 1] * rvec[..., 1]).astype(ft)
                     + rvec[..., 2] * rvec[..., 2]).astype(ft)
        nb = rn < ft(self.h)
        np.fill_diagonal(nb, False)
        return rvec, rn, nb

    def boundary_volume(self, dynamic):
        a, ft = self.a, self.ft
        rvec, rn, nb = self._pairs()
        solid = a["material"] == 0
        tgt = solid & ((a["is_dynamic"] != 0) if dynamic else (a["is_dynamic"] == 0))
        W = self._w(rn)
        delta = self._w(np.zeros(1, ft))[0] + np.where(nb & solid[None, :], W, ft(0)).sum(axis=1, dtype=ft)
        with np.errstate(divide="ignore"):
            a["m_V"] = np.where(tgt, ft(1.0) / delta * ft(3.0), a["m_V"]).astype(ft)

    def compute_densities(self):
        a, ft = self.a, self.ft
        rvec, rn, nb = self._pairs()
        W = self._w(rn)
        den = np.where(nb, a["m_V"][None, :] * W, ft(0)).sum(axis=1, dtype=ft)
        rho = (a["m_V"] * self._w(np.zeros(1, ft))[0] + den) * self.rho0
        fluid = a["material"] == 1
        a["density"] = np.where(fluid, rho, a["density"]).astype(ft)

    def compute_non_pressure_forces(self):
        a, ft = self.a, self.ft
        rvec, rn, nb = self._pairs()
        fluid = a["material"] == 1
        pair = nb & fluid[None, :]
        r2 = (rn * rn).astype(ft)
        Wst = np.where(r2 > ft(self.d * self.d), self._w(rn), self._w(np.full(1, self.d, ft))[0])
        c_st = (ft(f32(self.sigma)) / a["m"])[:, None] * a["m"][None, :]
        st = -(np.where(pair, c_st * Wst, ft(0))[..., None] * rvec).sum(axis=1, dtype=ft)
        vij = (a["v"][:, None, :] - a["v"][None, :, :]).astype(ft)
        v_xy = (vij * rvec).sum(axis=2, dtype=ft)
        gw = self._gw(rvec, rn)
        with np.errstate(divide="ignore", invalid="ignore"):
            c_v = ft(10 * self.nu) * (a["m"] / a["density"])[None, :] * v_xy / (r2 + ft(0.01 * self.h ** 2))
        visc = (np.where(pair, c_v, ft(0))[..., None] * gw).sum(axis=1, dtype=ft)
        acc = self.g[None, :] + np.where(fluid[:, None], st + visc, ft(0))
        static = (a["material"] == 0) & (a["is_dynamic"] == 0)
        a["acceleration"] = np.where(static[:, None], ft(0), acc).astype(ft)

    def eos(self):
        """The first loop of compute_pressure_forces (WCSPH.py:71-76): clamp, Tait pressure."""
        a, ft = self.a, self.ft
        fluid = a["material"] == 1
        rho = np.where(fluid, np.maximum(a["density"], self.rho0), a["density"]).astype(ft)
        a["density"] = rho
        p = self.stiffness * (np.power(rho / self.rho0, self.exponent, dtype=ft) - ft(1.0))
        a["pressure"] = np.where(fluid, p, a["pressure"]).astype(ft)

    def compute_pressure_forces(self):
        a, ft = self.a, self.ft
        fluid = a["material"] == 1
        self.eos()
        rho = a["density"]
        rvec, rn, nb = self._pairs()
        gw = self._gw(rvec, rn)
        dpi = (a["pressure"] / (rho * rho)).astype(ft)
        dpj_f = dpi[None, :]
        dpj_s = (a["pressure"] / (self.rho0 * self.rho0)).astype(ft)[:, None]
        dpj = np.where(fluid[None, :], dpj_f, dpj_s)
        c = -self.rho0 * a["m_V"][None, :] * (dpi[:, None] + dpj)
        f = np.where((nb & fluid[:, None])[..., None], c[..., None] * gw, ft(0)).astype(ft)  # f[i,j]
        dv = f.sum(axis=1, dtype=ft)
        dyn_solid = (a["material"] == 0) & (a["is_dynamic"] != 0)
        back = -(f * (self.rho0 / a["density"])[None, :, None])
        back = np.where(dyn_solid[None, :, None], back, ft(0)).sum(axis=0, dtype=ft)
        static = (a["material"] == 0) & (a["is_dynamic"] == 0)
        acc = a["acceleration"] + np.where(fluid[:, None], dv, ft(0)) + back
        a["acceleration"] = np.where(static[:, None], ft(0), acc).astype(ft)

    def advect(self):
        a, ft = self.a, self.ft
        dyn = (a["is_dynamic"] != 0)[:, None]
        v = a["v"] + self.dt * a["acceleration"]
        a["v"] = np.where(dyn, v, a["v"]).astype(ft)
        a["x"] = np.where(dyn, a["x"] + self.dt * a["v"], a["x"]).astype(ft)

    def enforce_boundary_3D(self, particle_type):
        a, ft = self.a, self.ft
        sel = (a["material"] == particle_type) & (a["is_dynamic"] != 0)
        pad = self.pad
        x, v = a["x"].copy(), a["v"].copy()
        hi = x > self.wall_hi[None, :]
        lo = x <= pad
        n = hi.astype(ft) - lo.astype(ft)
        xn = np.where(hi, self.wall_hi[None, :], x)
        xn = np.where(lo, pad, xn)
        ln = np.sqrt((n * n).sum(axis=1, dtype=ft))
        hit = sel & (ln > ft(1e-6))
        with np.errstate(divide="ignore", invalid="ignore"):
            vec = n / ln[:, None]
        vd = (v * vec).sum(axis=1, dtype=ft)
        vn = v - ft(1.5) * vd[:, None] * vec
        a["x"] = np.where(sel[:, None], xn, x).astype(ft)
        a["v"] = np.where(hit[:, None], vn, v).astype(ft)

    # ---- DFSPH (DFSPH.py:116-221): the three neighbour sums, no solver loops ----
    def dfsph_factor(self):
        """DFSPH.py:116-154: -1 / (sum_{fluid j} |m_V_j gradW_ij|^2 + |sum_j m_V_j gradW_ij|^2), 0 if the sum <= 1e-6."""
        a, ft = self.a, self.ft
        rvec, rn, nb = self._pairs()
        g = a["m_V"][None, :, None] * self._gw(rvec, rn)
        g = np.where(nb[..., None], g, ft(0))
        fluid = a["material"] == 1
        sq = (g * g).sum(axis=2, dtype=ft)
        s = np.where(fluid[None, :], sq, ft(0)).sum(axis=1, dtype=ft)
        gi = g.sum(axis=1, dtype=ft)
        s = s + (gi * gi).sum(axis=1, dtype=ft)
        with np.errstate(divide="ignore"):
            fac = np.where(s > ft(1e-6), ft(-1.0) / s, ft(0))
        return np.where(fluid, fac, ft(0)).astype(ft)

    def dfsph_velocity_divergence(self):
        """sum_j m_V_j (v_i - v_j) . gradW_ij and the neighbour count (DFSPH.py:183-197, 212-221)."""
        a, ft = self.a, self.ft
        rvec, rn, nb = self._pairs()
        gw = self._gw(rvec, rn)
        vij = (a["v"][:, None, :] - a["v"][None, :, :]).astype(ft)
        term = a["m_V"][None, :] * (vij * gw).sum(axis=2, dtype=ft)
        return np.where(nb, term, ft(0)).sum(axis=1, dtype=ft), nb.sum(axis=1)

    def dfsph_density_change(self):
        ft = self.ft
        div, cnt = self.dfsph_velocity_divergence()
        adv = np.where(cnt < 20, ft(0), np.maximum(div, ft(0)))
        return np.where(self.a["material"] == 1, adv, ft(0)).astype(ft)

    def dfsph_density_adv(self):
        ft = self.ft
        div, _ = self.dfsph_velocity_divergence()
        adv = np.maximum(self.a["density"] / self.rho0 + self.dt * div, ft(1.0))
        return np.where(self.a["material"] == 1, adv, ft(0)).astype(ft)

    def step(self):
        self.boundary_volume(dynamic=True)
        self.compute_densities()
        self.compute_non_pressure_forces()
        self.compute_pressure_forces()
        self.advect()
        self.enforce_boundary_3D(1)
