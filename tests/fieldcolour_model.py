"""NumPy model of the field colouring of the frames, written from the blocks "Field colouring" of
sph_taichi_amd/csrc/sph_render.hip and "WITH A FIELD COLOURING" of sph_taichi_amd/csrc/sph_surface.hip (NOT from their kernels):
every operation in `dtype` (float32 = what the device computes; float64 = the perturbation check), one rounding per written
operation, in the blocks' order.

    idx = index(s, lo, hi)                                  table index of field values s
    col = colours(ps, colour, rng)                          per-particle integer colour: lut[idx] where selected, ps.color elsewhere
    img, depth, winner = render(ps, colour, rng, camera, size, invisible=())            the sphere frame: render_model with that column
    out = surface(ps, colour, rng, camera, size, style, invisible=())                   the surface frame: surface_model's dict + "index"

`colour`: a render.FieldColour; `rng` = (lo, hi).  The state comes from the context's own downloads (x, v, density, pressure,
object_id, material, color).
"""
from __future__ import annotations

import types

import numpy as np

import render_model
import surface_model
from sph_taichi_amd import render as _render

IDX_NONE = 256             # FIELD_IDX_NONE: a fluid fragment whose particle is not selected


def state(ps):
    return {"x": ps.x.to_numpy(), "v": ps.v.to_numpy(), "density": ps.density.to_numpy(), "pressure": ps.pressure.to_numpy(),
            "object_id": ps.object_id.to_numpy(), "material": ps.material.to_numpy(), "color": ps.color.to_numpy()}


def field_values(st, field, axis_origin=0.0, dtype=np.float32):
    """s of the block, per particle."""
    ft = dtype
    v, x = st["v"].astype(ft), st["x"].astype(ft)
    with np.errstate(all="ignore"):
        if field == "speed":
            return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        if field in ("vx", "vy", "vz"):
            return v[:, "xyz".index(field[1])]
        if field in ("density", "pressure"):
            return st[field].astype(ft)
        return x[:, "xyz".index(field)] - ft(np.float32(axis_origin))


def index(s, lo, hi, dtype=np.float32):
    """idx of the block for field values s (any shape)."""
    ft = dtype
    s = np.asarray(s, dtype=ft)
    with np.errstate(all="ignore"):
        inv = ft(1) / (ft(np.float32(hi)) - ft(np.float32(lo)))
        t = (s - ft(np.float32(lo))) * inv
        t = np.where(t >= 0, np.minimum(t, ft(1)), ft(0))          # (a NaN compares false: 0)
        return (t * ft(255) + ft(0.5)).astype(np.int64)


def selected(st, colour):
    sel = np.ones(st["object_id"].shape[0], dtype=bool)
    if colour.material is not None:
        sel &= st["material"] == {"fluid": 1, "solid": 0}[colour.material]
    if colour.objects is not None:
        sel &= np.isin(st["object_id"], colour.objects)
    return sel


def particle_index(st, colour, rng, dtype=np.float32):
    """Per particle: its table index, IDX_NONE where it is not selected."""
    idx = index(field_values(st, colour.field, colour.axis_origin, dtype), rng[0], rng[1], dtype)
    return np.where(selected(st, colour), idx, IDX_NONE)


def colours(st, colour, rng, dtype=np.float32):
    idx = particle_index(st, colour, rng, dtype)
    lut = colour.lut()
    return np.where((idx != IDX_NONE)[:, None], lut[np.minimum(idx, 255)], st["color"]).astype(st["color"].dtype)


def field_range(st, colour, invisible=()):
    """(lo, hi, count, non_finite) as ParticleSystem.field_range defines them."""
    s = field_values(st, colour.field, colour.axis_origin)
    take = selected(st, colour) & ~np.isin(st["object_id"], list(invisible))
    fin = take & np.isfinite(s)
    if not fin.any():
        return float("inf"), float("-inf"), 0, int((take & ~fin).sum())
    return float(s[fin].min()), float(s[fin].max()), int(fin.sum()), int((take & ~fin).sum())


def render(ps, colour, rng, camera, size, invisible=(), dtype=np.float32, st=None):
    st = st if st is not None else state(ps)
    return render_model.render(st["x"], colours(st, colour, rng, dtype), st["object_id"], camera, size, ps.particle_radius,
                               ps.domain_end, invisible, dtype)


def _fluid_index_plane(s, st, pidx, zo, invisible):
    """The fluid splat's Q: per pixel the (z, e) minimum in lexicographic order; returns z0 and e (IDX_NONE + 1 where no fluid)."""
    ft = s.ft
    z0 = np.full((s.H, s.W), np.inf, dtype=ft)
    e0 = np.full((s.H, s.W), IDX_NONE + 1, dtype=np.int64)
    hidden = set(int(i) for i in invisible)
    for p in np.flatnonzero(st["material"] == surface_model.MATERIAL_FLUID):
        if int(st["object_id"][p]) in hidden:
            continue
        sp = render_model.sprite(s, st["x"][p])
        if sp is None:
            continue
        a, b, zc, px, py, R, inv, i0, i1, j0, j1 = sp
        ii = np.arange(i0, i1 + 1).astype(ft)[None, :]
        jj = np.arange(j0, j1 + 1).astype(ft)[:, None]
        dx, dy = np.broadcast_arrays(((ii + ft(0.5)) - px) * inv, (py - (jj + ft(0.5))) * inv)
        h2 = (s.r2 - dx * dx) - dy * dy
        ok = h2 >= 0
        z = zc - np.sqrt(np.where(ok, h2, ft(0)))
        ok &= z > 0
        zb, eb = z0[j0:j1 + 1, i0:i1 + 1], e0[j0:j1 + 1, i0:i1 + 1]
        take = ok & ((z < zb) | ((z == zb) & (pidx[p] < eb)))
        zb[take] = z[take]
        eb[take] = pidx[p]
    return z0, e0


def smooth_index(z0, e0, fw, ft):
    """The block's index smoothing: I [H, W] int, -1 where the pixel has no index."""
    has = np.isfinite(z0) & (e0 < IDX_NONE)
    out = np.full(z0.shape, -1, dtype=np.int64)
    if not has.any():
        return out
    R = surface_model.filter_radius(fw, z0, ft)
    rmax = int(R[has].max())
    vp = np.pad(np.where(has, e0, 0).astype(ft), rmax, constant_values=0)
    hp = np.pad(has, rmax, constant_values=False)
    R2 = np.where(has, R * R, 1).astype(ft)
    H, W = z0.shape
    sw = np.zeros(z0.shape, dtype=ft)
    sv = np.zeros(z0.shape, dtype=ft)
    zero = ft(0)
    with np.errstate(all="ignore"):
        for dj in range(-rmax, rmax + 1):
            for di in range(-rmax, rmax + 1):
                c = di * di + dj * dj
                if c >= rmax * rmax:
                    continue                                    # s2 >= 1 for every pixel: R <= rmax
                sl = (slice(rmax + dj, rmax + dj + H), slice(rmax + di, rmax + di + W))
                s2 = ft(c) / R2
                m = has & hp[sl] & (s2 < 1)
                ws = (ft(1) - s2) * (ft(1) - s2)
                sw = sw + np.where(m, ws, zero)
                sv = sv + np.where(m, ws * vp[sl], zero)
        v = np.where(has, sv / np.where(has, sw, ft(1)), zero)
        out[has] = np.minimum(np.maximum(v + ft(0.5), zero), ft(255)).astype(np.int64)[has]
    return out


def surface(ps, colour, rng, camera, size, style, invisible=(), dtype=np.float32, st=None):
    """surface_model.surface with the colouring: the opaque layer takes the colour column of `colours` if the colouring's
    material is not fluid; the fluid's body colour is lut[I] / 255 where the pixel has an index.  `style`: a resolved
    render.SurfaceStyle.  Adds "index" (I) to surface_model's dict."""
    st = st if st is not None else state(ps)
    ft = dtype
    opaque_field = colour.material != "fluid"
    fluid_field = colour.material in (None, "fluid")
    col = colours(st, colour, rng, dtype) if opaque_field else st["color"]
    args = (st["x"], col, st["object_id"], st["material"], camera, size, ps.particle_radius, ps.domain_end)
    if not fluid_field:
        out = surface_model.surface(*args, style, invisible, dtype)
        out["index"] = None
        return out
    plain = surface_model.surface(*args, style, invisible, dtype)          # depth, thickness and the opaque layer do not change
    s = render_model.Setup(camera, size, ps.particle_radius, ps.domain_end, dtype)
    z0, e0 = _fluid_index_plane(s, st, particle_index(st, colour, rng, dtype), plain["zo"], invisible)
    assert np.array_equal(z0, plain["z0"])
    fw = ft(np.float32(style.filter_radius)) * s.focal
    I = smooth_index(z0, e0, fw, ft)
    lut = colour.lut()
    body = [np.where(I >= 0, lut[np.maximum(I, 0), k].astype(ft) / ft(255), ft(np.float32(style.fluid_color[k]))) for k in range(3)]
    # surface_model._shade reads style.fluid_color[k] through ft(np.float32(.)), which takes a per-pixel plane as well as a number
    # (in the float64 model the body colour is therefore the binary32 value widened, like every other style parameter)
    painted = types.SimpleNamespace(**{**vars(style), "fluid_color": body})
    img, depth, thickness, shown = surface_model._shade(s, painted, plain["zs"], plain["ts"], plain["zo"], plain["behind_rgb"])
    out = dict(plain)
    out.update(img=img, depth=depth, thickness=thickness, shown=shown, index=I)
    return out
