"""NumPy model of the surface frame, written from the arithmetic block at the top of sph_taichi_amd/csrc/sph_surface.hip
(NOT from its kernels): every operation in `dtype` (float32 = what the device computes; float64 = the perturbation check of
test_gpu_surface), one rounding per written operation, in the block's order.  Projection, sprites and the opaque layer are
render_model's; the filters are vectorised over the window offsets, in the block's (dj outer, di inner) order -- a tap the block
skips adds an exact zero here, which leaves the same bits.

    out = surface(x, color, object_id, material, camera, size, radius, box_end, style, invisible=(), dtype=np.float32)

`style`: a resolved render.SurfaceStyle (no None field).  `out`: dict with
    img [H, W, 3] u8, depth [H, W], thickness [H, W]          the three outputs
    zo, behind_rgb                                            the opaque layer: depth and packed colour
    z0, S, t0                                                 raw fluid depth, thickness sum (integer), raw thickness
    zs, ts                                                    smoothed depth and thickness
    R [H, W]                                                  the filter's pixel radius from z0 (0 where no fluid)
    shown [H, W] bool                                         the pixel shows fluid
    sprite_radius_px                                          (min, max) over the drawn fluid sprites, or None
"""
from __future__ import annotations

import numpy as np

import render_model
from sph_taichi_amd.render import Camera

MAX_FILTER_R = 16          # SPH_SURFACE_MAX_FILTER_R
MATERIAL_FLUID = 1


def _dot3(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def filter_radius(fw, z, ft):
    """R(z) of the block; 0 where z is not finite."""
    fin = np.isfinite(z)
    with np.errstate(all="ignore"):
        r = np.minimum(np.maximum(np.ceil(fw / np.where(fin, z, ft(1))), ft(1)), ft(MAX_FILTER_R))
    return np.where(fin, r, ft(0)).astype(np.int64)


def _window(has):
    """Bounding rows / columns of the pixels that have fluid (the others keep their value whatever the filter does)."""
    rows, cols = np.flatnonzero(has.any(axis=1)), np.flatnonzero(has.any(axis=0))
    return rows[0], rows[-1] + 1, cols[0], cols[-1] + 1


def smooth_depth(z, fw, depth_range, ft):
    """One depth-smoothing pass."""
    fin = np.isfinite(z)
    if not fin.any():
        return z.copy()
    j0, j1, i0, i1 = _window(fin)
    R = filter_radius(fw, z, ft)
    rmax = int(R.max())
    zp = np.pad(z, rmax, constant_values=np.inf)
    zc, fc = z[j0:j1, i0:i1], fin[j0:j1, i0:i1]
    R2 = np.where(fc, R[j0:j1, i0:i1] * R[j0:j1, i0:i1], 1).astype(ft)
    sw = np.zeros(zc.shape, dtype=ft)
    sz = np.zeros(zc.shape, dtype=ft)
    zero = ft(0)
    with np.errstate(all="ignore"):
        for dj in range(-rmax, rmax + 1):
            for di in range(-rmax, rmax + 1):
                c = di * di + dj * dj
                if c >= rmax * rmax:
                    continue                                    # s2 >= 1 for every pixel: R <= rmax
                zq = zp[rmax + j0 + dj:rmax + j1 + dj, rmax + i0 + di:rmax + i1 + di]
                s2 = ft(c) / R2
                m = fc & np.isfinite(zq) & (s2 < 1)
                ws = (ft(1) - s2) * (ft(1) - s2)
                d = (zq - zc) / depth_range
                r2 = d * d
                m &= r2 < 1
                wr = (ft(1) - r2) * (ft(1) - r2)
                w = ws * wr
                sw = sw + np.where(m, w, zero)
                sz = sz + np.where(m, w * zq, zero)
        out = z.copy()
        out[j0:j1, i0:i1] = np.where(fc, sz / sw, np.inf)
    return out


def smooth_thickness(z0, t0, fw, ft):
    has = np.isfinite(z0)
    out = np.zeros(z0.shape, dtype=ft)
    if not has.any():
        return out
    j0, j1, i0, i1 = _window(has)
    R = filter_radius(fw, z0, ft)
    rmax = int(R.max())
    tp = np.pad(t0, rmax, constant_values=0)
    hp = np.pad(has, rmax, constant_values=False)
    hc = has[j0:j1, i0:i1]
    R2 = np.where(hc, R[j0:j1, i0:i1] * R[j0:j1, i0:i1], 1).astype(ft)
    sw = np.zeros(hc.shape, dtype=ft)
    st = np.zeros(hc.shape, dtype=ft)
    zero = ft(0)
    with np.errstate(all="ignore"):
        for dj in range(-rmax, rmax + 1):
            for di in range(-rmax, rmax + 1):
                c = di * di + dj * dj
                if c >= rmax * rmax:
                    continue
                sl = (slice(rmax + j0 + dj, rmax + j1 + dj), slice(rmax + i0 + di, rmax + i1 + di))
                s2 = ft(c) / R2
                m = hc & hp[sl] & (s2 < 1)
                ws = (ft(1) - s2) * (ft(1) - s2)
                sw = sw + np.where(m, ws, zero)
                st = st + np.where(m, ws * tp[sl], zero)
        out[j0:j1, i0:i1] = np.where(hc, st / sw, zero)
    return out


def _shift(a, di, dj, fill):
    """b[j, i] = a[j + dj, i + di], `fill` outside the image."""
    H, W = a.shape
    b = np.full(a.shape, fill, dtype=a.dtype)
    b[max(-dj, 0):H - max(dj, 0), max(-di, 0):W - max(di, 0)] = a[max(dj, 0):H - max(-dj, 0), max(di, 0):W - max(-di, 0)]
    return b


def _point(s, ii, jj, z):
    zf = z / s.focal
    return [((ii + s.ft(0.5)) - s.cx) * zf, (s.cy - (jj + s.ft(0.5))) * zf, z]


def _shade(s, style, zs, ts, zo, behind_rgb):
    ft = s.ft
    W, H = s.W, s.H
    with np.errstate(all="ignore"):
        shown = np.isfinite(zs) & (zs < zo)
        ii = np.broadcast_to(np.arange(W).astype(ft)[None, :], (H, W))
        jj = np.broadcast_to(np.arange(H).astype(ft)[:, None], (H, W))
        z = np.where(shown, zs, ft(1))                         # (the pixels that do not show fluid are overwritten below)
        zf = z / s.focal
        P = _point(s, ii, jj, z)
        zE, zW = _shift(zs, 1, 0, np.inf), _shift(zs, -1, 0, np.inf)
        zN, zS = _shift(zs, 0, -1, np.inf), _shift(zs, 0, 1, np.inf)
        uE, uW, uN, uS = np.isfinite(zE), np.isfinite(zW), np.isfinite(zN), np.isfinite(zS)
        one, zero = ft(1), ft(0)
        PE, PW = _point(s, ii + one, jj, zE), _point(s, ii - one, jj, zW)
        PN, PS = _point(s, ii, jj - one, zN), _point(s, ii, jj + one, zS)
        takeE = uE & (~uW | (np.abs(zE - z) <= np.abs(z - zW)))
        takeN = uN & (~uS | (np.abs(zN - z) <= np.abs(z - zS)))
        flat_a = [zf, np.zeros_like(zf), np.zeros_like(zf)]
        flat_b = [np.zeros_like(zf), zf, np.zeros_like(zf)]
        A = [np.where(takeE, PE[k] - P[k], np.where(uW, P[k] - PW[k], flat_a[k])) for k in range(3)]
        B = [np.where(takeN, PN[k] - P[k], np.where(uS, P[k] - PS[k], flat_b[k])) for k in range(3)]
        c = [A[2] * B[1] - A[1] * B[2], A[0] * B[2] - A[2] * B[0], A[1] * B[0] - A[0] * B[1]]
        cl = np.sqrt(_dot3(c, c))
        ok = cl > 0
        fallback = [zero, zero, ft(-1)]
        n = [np.where(ok, c[k] / cl, fallback[k]) for k in range(3)]
        e = [zero - P[0], zero - P[1], zero - P[2]]
        el = np.sqrt(_dot3(e, e))
        v = [e[k] / el for k in range(3)]
        nv = _dot3(n, v)
        flip = nv < 0
        n = [np.where(flip, zero - n[k], n[k]) for k in range(3)]
        nv = np.where(flip, zero - nv, nv)
        l = [s.L[k] - P[k] for k in range(3)]
        ll = np.sqrt(_dot3(l, l))
        lit_ok = ll > 0
        lu = [l[k] / ll for k in range(3)]
        nl = np.where(lit_ok, np.fmax(_dot3(n, lu), zero), zero)
        h = [lu[k] + v[k] for k in range(3)]
        hl = np.sqrt(_dot3(h, h))
        nh = np.where(lit_ok & (hl > 0), np.fmax(_dot3(n, h) / hl, zero), zero)
        sp = nh
        for _ in range(6):
            sp = sp * sp
        spec = ft(np.float32(style.specular)) * sp
        m = one - np.fmax(nv, zero)
        m2 = m * m
        m4 = m2 * m2
        m5 = m4 * m
        f0 = ft(np.float32(style.f0))
        F = f0 + (one - f0) * m5
        lit = s.ambient + (one - s.ambient) * nl
        img = np.zeros((H, W, 3), dtype=np.uint8)
        for k in range(3):
            byte = (behind_rgb >> np.uint32(16 - 8 * k)) & np.uint32(255)
            behind = byte.astype(ft) / ft(255)
            ak = one + ft(np.float32(style.absorb[k])) * ts
            T = one / (ak * ak)
            col = ((T * behind + (one - T) * (ft(np.float32(style.fluid_color[k])) * lit)) * (one - F)
                   + F * ft(np.float32(style.sky[k]))) + spec
            q = (np.fmin(np.fmax(col, zero), one) * ft(255) + ft(0.5)).astype(np.uint32)
            img[..., k] = np.where(shown, q, byte).astype(np.uint8)
    depth = np.where(shown, zs, zo)
    thickness = np.where(shown, ts, zero)
    return img, depth, thickness, shown


def surface(x, color, object_id, material, camera=None, size=(256, 256), radius=0.01, box_end=(1.0, 1.0, 1.0), style=None,
            invisible=(), dtype=np.float32):
    camera = camera if camera is not None else Camera()
    s = render_model.Setup(camera, size, radius, box_end, dtype)
    ft = s.ft
    W, H = s.W, s.H
    x = np.asarray(x, dtype=np.float32)
    color, object_id, material = np.asarray(color), np.asarray(object_id), np.asarray(material)
    fluid = material == MATERIAL_FLUID
    # opaque layer: the sphere frame of everything that is not fluid, plus the box edges
    oimg, zo, _ = render_model.render(x[~fluid], color[~fluid], object_id[~fluid], camera, size, radius, box_end, invisible, dtype)
    behind_rgb = (oimg[..., 0].astype(np.uint32) << np.uint32(16)) | (oimg[..., 1].astype(np.uint32) << np.uint32(8)) | oimg[..., 2]
    # fluid splat
    z0 = np.full((H, W), np.inf, dtype=ft)
    S = np.zeros((H, W), dtype=np.uint64)
    hidden = set(int(i) for i in invisible)
    radii = []
    for p in np.flatnonzero(fluid):
        if int(object_id[p]) in hidden:
            continue
        sp = render_model.sprite(s, x[p])
        if sp is None:
            continue
        a, b, zc, px, py, R, inv, i0, i1, j0, j1 = sp
        radii.append(float(R))
        ii = np.arange(i0, i1 + 1).astype(ft)[None, :]
        jj = np.arange(j0, j1 + 1).astype(ft)[:, None]
        dx, dy = np.broadcast_arrays(((ii + ft(0.5)) - px) * inv, (py - (jj + ft(0.5))) * inv)
        h2 = (s.r2 - dx * dx) - dy * dy
        ok = h2 >= 0
        hh = np.sqrt(np.where(ok, h2, ft(0)))
        z = zc - hh
        ok &= z > 0
        zb = z0[j0:j1 + 1, i0:i1 + 1]
        zb[ok] = np.minimum(zb[ok], z[ok])
        add = ((hh / s.radius) * ft(256) + ft(0.5)).astype(np.uint64)
        front = ok & (z < zo[j0:j1 + 1, i0:i1 + 1])
        S[j0:j1 + 1, i0:i1 + 1] += np.where(front, add, np.uint64(0))
    S = S & np.uint64(0xFFFFFFFF)                               # (the device's sum is u32)
    fw = ft(np.float32(style.filter_radius)) * s.focal
    tk = s.radius * ft(2.0 / 256.0)
    depth_range = ft(np.float32(style.depth_range))
    t0 = S.astype(np.uint32).astype(ft) * tk
    zs = z0
    for _ in range(int(style.iterations)):
        zs = smooth_depth(zs, fw, depth_range, ft)
    ts = smooth_thickness(z0, t0, fw, ft)
    img, depth, thickness, shown = _shade(s, style, zs, ts, zo, behind_rgb)
    return {"img": img, "depth": depth, "thickness": thickness, "zo": zo, "behind_rgb": behind_rgb, "z0": z0, "S": S, "t0": t0,
            "zs": zs, "ts": ts, "R": filter_radius(fw, z0, ft), "shown": shown,
            "sprite_radius_px": (min(radii), max(radii)) if radii else None}
