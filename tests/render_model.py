"""NumPy model of the frame renderer, written from the arithmetic block at the top of
sph_taichi_amd/csrc/sph_render.hip (NOT from its kernels): one Python loop over particles, every operation
in `dtype` (float32 = what the device computes; float64 = the perturbation check of test_gpu_render), one rounding per
written operation, in the block's order.

    img, depth, winner = render(x, color, object_id, camera, size, radius, box_end, invisible=())

`winner` [H, W]: index of the particle a pixel shows, -1 background, -2 box line.
A pixel keeps the minimum of (z, rgb) in lexicographic order -- for positive float32 z exactly the minimum of the
device's key  bits(z) << 32 | rgb.
"""
from __future__ import annotations

import numpy as np

from sph_taichi_amd.render import Camera, view_basis

SMALL_R = 4.0      # (the device's work split; no influence on the image)
MAX_R = 512.0      # SPH_RENDER_MAX_R: larger sprites are cropped to this half-width


def _dot(a, d):
    return (a[0] * d[0] + a[1] * d[1]) + a[2] * d[2]


class Setup:
    """The block's host part in `dtype` (the basis itself is binary64 rounded to binary32, as on the device)."""

    def __init__(self, camera: Camera, size, radius, box_end, dtype=np.float32):
        ft = self.ft = dtype
        self.W, self.H = int(size[0]), int(size[1])
        r, u, f, focal = view_basis(camera, self.H)
        self.r, self.u, self.f = r.astype(ft), u.astype(ft), f.astype(ft)
        self.focal = ft(focal)
        self.eye = np.array(camera.eye, dtype=np.float32).astype(ft)
        self.cx = ft(self.W) * ft(0.5)
        self.cy = ft(self.H) * ft(0.5)
        self.radius = ft(np.float32(radius))
        self.r2 = self.radius * self.radius
        self.fr = self.focal * self.radius
        self.near = ft(np.float32(camera.near_plane))
        dl = np.array(camera.light, dtype=np.float32).astype(ft) - self.eye
        self.L = np.array([_dot(self.r, dl), _dot(self.u, dl), _dot(self.f, dl)], dtype=ft)
        self.ambient = ft(np.float32(camera.ambient))
        self.box_end = np.array(box_end, dtype=np.float32).astype(ft)
        bc = np.minimum(np.maximum(np.array(camera.box_color, dtype=np.float32).astype(ft), ft(0)), ft(1))
        q = (bc * ft(255) + ft(0.5)).astype(np.uint32)
        self.box_rgb = int(q[0]) << 16 | int(q[1]) << 8 | int(q[2])
        self.background = int(camera.background[0]) << 16 | int(camera.background[1]) << 8 | int(camera.background[2])
        self.draw_box = bool(camera.draw_box)
        self.S = 4 * (self.W + self.H)


def sprite(s: Setup, x):
    """Projection of one particle: None if culled, else (a, b, zc, px, py, R, inv, i0, i1, j0, j1)."""
    ft = s.ft
    with np.errstate(all="ignore"):
        d = x.astype(ft) - s.eye
        a, b, zc = _dot(s.r, d), _dot(s.u, d), _dot(s.f, d)
        if not zc >= s.near:
            return None
        px = s.cx + (s.focal * a) / zc
        py = s.cy - (s.focal * b) / zc
        R = s.fr / zc
        inv = zc / s.focal
        if not (np.isfinite(px) and np.isfinite(py) and np.isfinite(R)):
            return None
        Rb = min(R, ft(MAX_R))
        i0 = int(min(max(np.ceil((px - Rb) - ft(0.5)), ft(0)), ft(s.W)))
        i1 = int(max(min(np.floor((px + Rb) - ft(0.5)), ft(s.W - 1)), ft(-1)))
        j0 = int(min(max(np.ceil((py - Rb) - ft(0.5)), ft(0)), ft(s.H)))
        j1 = int(max(min(np.floor((py + Rb) - ft(0.5)), ft(s.H - 1)), ft(-1)))
    if i0 > i1 or j0 > j1:
        return None
    return a, b, zc, px, py, R, inv, i0, i1, j0, j1


def render(x, color, object_id, camera=None, size=(256, 256), radius=0.01, box_end=(1.0, 1.0, 1.0), invisible=(),
           dtype=np.float32):
    camera = camera if camera is not None else Camera()
    s = Setup(camera, size, radius, box_end, dtype)
    ft = s.ft
    W, H = s.W, s.H
    zbuf = np.full((H, W), np.inf, dtype=ft)
    rgbbuf = np.full((H, W), s.background, dtype=np.uint32)
    winner = np.full((H, W), -1, dtype=np.int64)
    x = np.asarray(x, dtype=np.float32)
    color = np.asarray(color)
    hidden = set(int(i) for i in invisible)
    for p in range(x.shape[0]):
        if int(object_id[p]) in hidden:
            continue
        sp = sprite(s, x[p])
        if sp is None:
            continue
        a, b, zc, px, py, R, inv, i0, i1, j0, j1 = sp
        kc = color[p].astype(ft) / ft(255)
        ii = np.arange(i0, i1 + 1).astype(ft)[None, :]
        jj = np.arange(j0, j1 + 1).astype(ft)[:, None]
        dx, dy = np.broadcast_arrays(((ii + ft(0.5)) - px) * inv, (py - (jj + ft(0.5))) * inv)
        h2 = (s.r2 - dx * dx) - dy * dy
        ok = h2 >= 0
        hh = np.sqrt(np.where(ok, h2, ft(0)))
        z = zc - hh
        ok &= z > 0
        nx, ny, nz = dx / s.radius, dy / s.radius, hh / s.radius
        lx = s.L[0] - (a + dx)
        ly = s.L[1] - (b + dy)
        lz = z - s.L[2]
        ll = np.sqrt((lx * lx + ly * ly) + lz * lz)
        with np.errstate(all="ignore"):
            nl = np.where(ll > 0, ((nx * lx + ny * ly) + nz * lz) / ll, ft(0))
        shade = s.ambient + (ft(1) - s.ambient) * np.maximum(nl, ft(0))
        rgb = np.zeros(z.shape, dtype=np.uint32)
        for k in range(3):
            t = np.minimum(np.maximum(kc[k] * shade, ft(0)), ft(1))
            rgb = (rgb << np.uint32(8)) | (t * ft(255) + ft(0.5)).astype(np.uint32)
        zb = zbuf[j0:j1 + 1, i0:i1 + 1]
        rb = rgbbuf[j0:j1 + 1, i0:i1 + 1]
        wb = winner[j0:j1 + 1, i0:i1 + 1]
        take = ok & ((z < zb) | ((z == zb) & (rgb < rb)))
        zb[take] = z[take]
        rb[take] = rgb[take]
        wb[take] = p
    if s.draw_box:
        _box(s, zbuf, rgbbuf, winner)
    img = np.stack([(rgbbuf >> 16) & 255, (rgbbuf >> 8) & 255, rgbbuf & 255], axis=-1).astype(np.uint8)
    return img, zbuf, winner


def _box(s: Setup, zbuf, rgbbuf, winner):
    ft = s.ft
    m = np.arange(s.S).astype(ft)
    t = (m + ft(0.5)) / ft(s.S)
    zbox = np.full(zbuf.shape, np.inf, dtype=ft)
    for e in range(12):
        axis, c1, c2 = e >> 2, e & 1, (e >> 1) & 1
        o1, o2 = (axis + 1) % 3, (axis + 2) % 3
        A = np.zeros(3, dtype=ft)
        B = np.zeros(3, dtype=ft)
        B[axis] = s.box_end[axis]
        A[o1] = B[o1] = s.box_end[o1] if c1 else ft(0)
        A[o2] = B[o2] = s.box_end[o2] if c2 else ft(0)
        d = [(A[k] + (B[k] - A[k]) * t) - s.eye[k] for k in range(3)]
        a, b, zc = _dot(s.r, d), _dot(s.u, d), _dot(s.f, d)
        with np.errstate(all="ignore"):
            px = s.cx + (s.focal * a) / zc
            py = s.cy - (s.focal * b) / zc
            ok = (zc >= s.near) & (px >= 0) & (px < ft(s.W)) & (py >= 0) & (py < ft(s.H))
        i = px[ok].astype(np.int64)
        j = py[ok].astype(np.int64)
        np.minimum.at(zbox, (j, i), zc[ok])
    take = (zbox < zbuf) | ((zbox == zbuf) & np.isfinite(zbox) & (np.uint32(s.box_rgb) < rgbbuf))
    zbuf[take] = zbox[take]
    rgbbuf[take] = s.box_rgb
    winner[take] = -2
