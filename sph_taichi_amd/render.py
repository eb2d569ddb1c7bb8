"""Headless frame export: the camera of the reference's window (run_simulation.py:37-45, 90-93), the view basis the
device renderer uses (csrc/sph_render.hip states the arithmetic), and a PNG writer on zlib + struct.

The picture itself is made on the GPU (`ParticleSystem.render`); nothing here touches particle data.
`SurfaceStyle` holds the knobs of the second frame style, `ParticleSystem.render_surface` (csrc/sph_surface.hip): the fluid as one
shaded screen-space surface over the solids.
"""
from __future__ import annotations

import math
import struct
import zlib
from dataclasses import dataclass

import numpy as np

from . import _lib, selection


@dataclass
class Camera:
    """Defaults = the reference's window: position (5.5, 2.5, 4.0), lookat (-1, 0, 0), up (0, 1, 0), fov 70 degrees,
    point light (2, 2, 2), black background, box lines (0.99, 0.68, 0.28)  (run_simulation.py:37-50, 90-93)."""
    eye: tuple = (5.5, 2.5, 4.0)
    lookat: tuple = (-1.0, 0.0, 0.0)
    up: tuple = (0.0, 1.0, 0.0)
    fov_y_deg: float = 70.0
    near_plane: float = 0.05
    light: tuple = (2.0, 2.0, 2.0)
    ambient: float = 0.3
    background: tuple = (0, 0, 0)
    draw_box: bool = True
    box_color: tuple = (0.99, 0.68, 0.28)


def view_basis(camera: Camera, height: int):
    """(right, up, forward, focal) as float32: the binary64 sequence of the comment block of csrc/sph_render.hip, rounded
    once.  The library runs the same sequence on the same inputs; the tests' model takes these values.  Raises
    ValueError where the library answers SPH_E_INVALID."""
    f32 = lambda v: [float(np.float32(c)) for c in v]      # the struct carries binary32
    eye, lookat, up = f32(camera.eye), f32(camera.lookat), f32(camera.up)
    f = [lookat[k] - eye[k] for k in range(3)]
    fl = math.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
    if not fl > 0.0:
        raise ValueError("camera: eye == lookat")
    f = [c / fl for c in f]
    r = [f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]]
    rl = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    ul = math.sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2])
    if not ul > 0.0 or not rl > 1e-6 * ul:
        raise ValueError("camera: up is zero or parallel to the view direction")
    r = [c / rl for c in r]
    u = [r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]]
    fov = float(np.float32(camera.fov_y_deg))
    if not 0.0 < fov < 180.0:
        raise ValueError("camera: fov_y_deg must be in (0, 180)")
    focal = (float(height) * 0.5) / math.tan((fov * (3.141592653589793 / 180.0)) * 0.5)
    return (np.array(r, dtype=np.float32), np.array(u, dtype=np.float32), np.array(f, dtype=np.float32),
            np.float32(focal))


def render_params(camera: Camera, size, radius: float, box_end) -> "_lib.SphRenderParams":
    """The C struct for `camera` at `size` = (width, height)."""
    p = _lib.SphRenderParams()
    p.width, p.height = int(size[0]), int(size[1])
    for name in ("eye", "lookat", "up", "light", "box_color"):
        setattr(p, name, (_lib.C.c_float * 3)(*[float(v) for v in getattr(camera, name)]))
    p.box_end = (_lib.C.c_float * 3)(*[float(v) for v in box_end])
    p.fov_y_deg = float(camera.fov_y_deg)
    p.radius = float(radius)
    p.near_plane = float(camera.near_plane)
    p.ambient = float(camera.ambient)
    p.background = (_lib.C.c_uint8 * 3)(*[int(v) for v in camera.background])
    p.draw_box = 1 if camera.draw_box else 0
    return p


@dataclass
class SurfaceStyle:
    """How `ParticleSystem.render_surface` draws the fluid (csrc/sph_surface.hip states the arithmetic).  `None` fields are
    filled in by the ParticleSystem: filter_radius = 3 x particle radius, depth_range = 4 x particle radius (world units),
    fluid_color = the first fluid block's colour / 255."""
    iterations: int = 3                       # depth-smoothing passes, 0..8
    filter_radius: float | None = None        # world units; in pixels it follows the depth, at most 16
    depth_range: float | None = None          # world units: depth differences from here on do not mix
    fluid_color: tuple | None = None          # in [0, 1]
    absorb: tuple = (18.0, 6.0, 2.0)          # per world unit and channel: transmittance 1 / (1 + absorb * thickness)^2
    sky: tuple = (0.75, 0.85, 0.95)           # what the Fresnel term reflects
    f0: float = 0.02                          # reflectance at normal incidence (water)
    specular: float = 0.6                     # weight of the (n.h)^64 highlight


_STYLE_KEYS = {"iterations": "iterations", "filterRadius": "filter_radius", "depthRange": "depth_range", "fluidColor": "fluid_color",
               "absorb": "absorb", "sky": "sky", "f0": "f0", "specular": "specular"}


def surface_style_from_config(entry) -> SurfaceStyle:
    """The scene file's "surfaceStyle": {...} (camelCase keys of the fields above; colours in [0, 1]); None or {} = defaults."""
    style = SurfaceStyle()
    for key, val in (entry or {}).items():
        if key not in _STYLE_KEYS:
            raise ValueError(f"surfaceStyle: unknown key {key!r} (known: {', '.join(sorted(_STYLE_KEYS))})")
        setattr(style, _STYLE_KEYS[key], tuple(val) if isinstance(val, (list, tuple)) else val)
    return style


def resolve_style(style, radius: float, fluid_rgb255) -> SurfaceStyle:
    """A copy of `style` (None: the defaults) with its None fields filled in for a particle radius and a fluid colour (0..255)."""
    s = SurfaceStyle(**vars(style)) if style is not None else SurfaceStyle()
    if s.filter_radius is None:
        s.filter_radius = 3.0 * float(radius)
    if s.depth_range is None:
        s.depth_range = 4.0 * float(radius)
    if s.fluid_color is None:
        s.fluid_color = tuple(float(v) / 255.0 for v in fluid_rgb255)
    return s


def surface_params(style: SurfaceStyle) -> "_lib.SphSurfaceParams":
    """The C struct for a resolved style."""
    p = _lib.SphSurfaceParams()
    p.iterations = int(style.iterations)
    p.filter_radius = float(style.filter_radius)
    p.depth_range = float(style.depth_range)
    for name in ("fluid_color", "absorb", "sky"):
        setattr(p, name, (_lib.C.c_float * 3)(*[float(v) for v in getattr(style, name)]))
    p.f0 = float(style.f0)
    p.specular = float(style.specular)
    return p


# ---- field colouring of the frames (csrc/sph_render.hip states the index arithmetic) ----
# enum SphColourField, in its order
FIELDS = ("speed", "vx", "vy", "vz", "density", "pressure", "x", "y", "z")
# Control points (position in [0, 1], red, green, blue) of the built-in maps; colormap() interpolates between them.
_COLORMAPS = {
    "heat": ((0.0, 0, 0, 0), (0.3, 160, 0, 0), (0.55, 255, 70, 0), (0.8, 255, 210, 0), (1.0, 255, 255, 255)),
    "coolwarm": ((0.0, 59, 76, 192), (0.25, 141, 176, 254), (0.5, 221, 221, 221), (0.75, 244, 154, 123), (1.0, 180, 4, 38)),
    "grey": ((0.0, 0, 0, 0), (1.0, 255, 255, 255)),
    "rainbow": ((0.0, 0, 0, 255), (0.25, 0, 255, 255), (0.5, 0, 255, 0), (0.75, 255, 255, 0), (1.0, 255, 0, 0)),
}


def colormap(name: str) -> np.ndarray:
    """uint8 [256, 3] of a built-in map: entry i is the map at i / 255, each channel interpolated linearly between the control
    points in float64 and rounded (half up)."""
    if not isinstance(name, str) or name not in _COLORMAPS:
        raise ValueError(f"colormap must be one of {', '.join(sorted(_COLORMAPS))} or a uint8 [256, 3] array, not {name!r}")
    pts = np.array(_COLORMAPS[name], dtype=np.float64)
    t = np.arange(256, dtype=np.float64) / 255.0
    cols = [np.interp(t, pts[:, 0], pts[:, 1 + k]) for k in range(3)]
    return np.floor(np.stack(cols, axis=-1) + 0.5).astype(np.uint8)


@dataclass
class FieldColour:
    """Colour the selected particles of a frame by a field instead of by their object (`ParticleSystem.render(colour=...)`,
    `render_surface(colour=...)`).  `field`: one of FIELDS -- velocity magnitude or a component, density, pressure, or the position
    along an axis minus `axis_origin`.  `range` = (lo, hi): the field values of the first and the last table entry; None: minimum
    and maximum over the particles that are coloured, reduced on the device before the frame (an empty or degenerate one becomes
    (lo, lo + 1)).  `colormap`: a built-in name or a uint8 [256, 3] array.  `material` ("fluid", "solid" or None) and `objects` (ids,
    None: all) choose the particles that take the field colour; the others keep their object colour."""
    field: str
    range: tuple | None = None
    colormap: object = "heat"
    material: str | None = "fluid"
    objects: list | None = None
    axis_origin: float = 0.0

    def __post_init__(self):
        if not isinstance(self.field, str) or self.field not in FIELDS:
            raise ValueError(f"field must be one of {', '.join(FIELDS)}, not {self.field!r}")
        if self.range is not None:
            self.range = check_range(self.range)
        self.objects = selection.parse(self.material, self.objects, material_ids=False)[1] or None   # (names only: no material id)
        self.axis_origin = float(self.axis_origin)
        if not math.isfinite(self.axis_origin):
            raise ValueError("axis_origin must be finite")
        self.lut()

    def lut(self) -> np.ndarray:
        """The table as int32 [256, 3] (what the library takes)."""
        if isinstance(self.colormap, str):
            return colormap(self.colormap).astype(np.int32)
        a = np.asarray(self.colormap)
        if a.dtype != np.uint8 or a.shape != (256, 3):
            raise ValueError(f"colormap must be one of {', '.join(sorted(_COLORMAPS))} or a uint8 [256, 3] array, "
                             f"not {a.dtype} {list(a.shape)}")
        return np.ascontiguousarray(a, dtype=np.int32)

    def colormap_name(self) -> str:
        return self.colormap if isinstance(self.colormap, str) else "custom"


def check_range(rng) -> tuple:
    """(lo, hi) as floats; ValueError unless both are finite, lo < hi in binary32 and 1 / (hi - lo) is a finite binary32."""
    try:
        lo, hi = (float(v) for v in rng)
    except (TypeError, ValueError):
        raise ValueError(f"range must be (lo, hi) or None, not {rng!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"range must be finite, not ({lo}, {hi})")
    with np.errstate(all="ignore"):
        width = np.float32(hi) - np.float32(lo)
        inv = np.float32(1) / width if width > 0 else np.float32(0)
    if not lo < hi or not width > 0:
        raise ValueError(f"range needs lo < hi (in binary32), not ({lo}, {hi})")
    if not (np.isfinite(inv) and inv > 0):
        raise ValueError(f"range ({lo}, {hi}) is too narrow or too wide for binary32")
    return (lo, hi)


def auto_range(lo: float, hi: float, count: int) -> tuple:
    """The range of a frame whose FieldColour has none, from a device reduction: (0, 1) over no particle, (lo, lo + 1) where
    (lo, hi) is not a usable range."""
    if count <= 0:
        return (0.0, 1.0)
    try:
        return check_range((lo, hi))
    except ValueError:
        return (float(lo), float(np.float32(lo) + np.float32(1)))


_COLOUR_KEYS = {"field": "field", "range": "range", "colormap": "colormap", "material": "material", "objects": "objects",
                "axisOrigin": "axis_origin"}


def field_colour_from_config(entry) -> FieldColour | None:
    """The scene file's "frameColour": {"field": "speed", "range": [0, 3], "colormap": "heat", "material": "fluid", "objects": [0],
    "axisOrigin": 0} (every key but "field" optional), or just the field's name; None = no colouring.  A colormap is given by name."""
    if entry is None:
        return None
    if isinstance(entry, str):
        entry = {"field": entry}
    if not isinstance(entry, dict):
        raise ValueError(f"frameColour must be an object with a \"field\" key or a field name, not {entry!r}")
    kw = {}
    for key, val in entry.items():
        if key not in _COLOUR_KEYS:
            raise ValueError(f"frameColour: unknown key {key!r} (known: {', '.join(sorted(_COLOUR_KEYS))})")
        kw[_COLOUR_KEYS[key]] = val
    if "field" not in kw:
        raise ValueError(f"frameColour needs a \"field\" key: one of {', '.join(FIELDS)}")
    if "colormap" in kw and not isinstance(kw["colormap"], str):
        raise ValueError(f"frameColour: colormap must be one of {', '.join(sorted(_COLORMAPS))}")
    try:
        return FieldColour(**kw)
    except ValueError as e:
        raise ValueError(f"frameColour: {e}") from None


def field_colour_params(colour: FieldColour, rng=(0.0, 1.0)) -> "_lib.SphFieldColour":
    """The C struct for `colour` with the range `rng`."""
    p = _lib.SphFieldColour()
    p.field = FIELDS.index(colour.field)
    selection.fill(p, -1 if colour.material is None else selection.MATERIALS[colour.material], colour.objects or [])
    p.lo, p.hi = float(rng[0]), float(rng[1])
    p.axis_origin = colour.axis_origin
    return p


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path: str, rgb: np.ndarray, level: int = 6, text=None):
    """8-bit RGB PNG of a uint8 [H, W, 3] array (row 0 at the top): IHDR, one IDAT (filter 0 on every row), IEND.  `text`: a dict
    written as tEXt chunks (keyword, Latin-1 text) between IHDR and IDAT, in the dict's order; None: no such chunk."""
    a = np.ascontiguousarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: expected uint8 [H, W, 3]")
    chunks = []
    for key, val in (text or {}).items():
        k, v = str(key).encode("latin-1"), str(val).encode("latin-1")
        if not 1 <= len(k) <= 79 or b"\0" in k or b"\0" in v:
            raise ValueError(f"write_png: a tEXt keyword has 1 to 79 Latin-1 characters and no NUL, not {key!r}")
        chunks.append(_chunk(b"tEXt", k + b"\0" + v))
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)         # a filter-type byte in front of every row
    rows[:, 1:] = a.reshape(h, 3 * w)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n")
        fh.write(_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
        for c in chunks:
            fh.write(c)
        fh.write(_chunk(b"IDAT", zlib.compress(rows.tobytes(), level)))
        fh.write(_chunk(b"IEND", b""))
