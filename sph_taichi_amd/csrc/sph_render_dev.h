// sph_render_dev.h -- the camera record, the sprite / fragment / box-edge device functions and the splat of one LAYER of
// particles, shared by the sphere frame (sph_render.hip, whose comment block states their arithmetic and which holds the splat
// kernels) and the surface frame (sph_surface.hip: its opaque layer is the sphere frame's picture restricted to the particles
// that are not fluid, its fluid layer the same sprites with another fragment).
#pragma once
#include <math.h>

#include "sph_observe.h"

#pragma clang fp contract(off)

#define SPH_RENDER_SMALL_R 4.0f    // sprites up to this pixel radius (at most 9 x 9 pixels) are rasterised by one lane
#define SPH_RENDER_MAX_R 512.0f    // larger sprites are cropped to the square of this half-width around their centre
#define SPH_RENDER_MAX_DIM 16384
#define RTPB 256
#define FRAME_SLAB_WHY "; frames are rendered from single-domain contexts only"   // sph_observe_enter: compositing across GPUs is not built

struct RenderCam {
    int W, H, S;              // image size; samples per box edge
    int n_invisible;
    int invisible[SPH_RENDER_MAX_INVISIBLE];
    float ex, ey, ez;
    float rx, ry, rz, ux, uy, uz, fx, fy, fz;
    float focal, cx, cy, radius, r2, fr, near_plane;
    float Lx, Ly, Lz, ambient;
    float bex, bey, bez;      // box_end
    unsigned box_rgb, background;
    int draw_box;
};

// Field colouring (include/sph_hip.h, "Field colouring of the frames"; sph_render.hip states the arithmetic): which particles
// take a table colour, from which field, and the range as lo and inv = 1 / (hi - lo).  By value into the launches, like RenderCam.
struct FieldSel {
    int field;
    float lo, inv, origin;
    SphSel who;
};
#define FIELD_IDX_NONE 256                 // "this fluid fragment's particle is not selected" in the low half of a field-index key

struct FrameField {                        // what only the *_FIELD layers read; by value
    FieldSel sel;
    const int* lut;                        // [256 * 3] on the device
    unsigned long long* fzi;               // LAYER_FLUID_FIELD: per pixel min of bits(z) << 32 | index
    const float4* vf;                      // the live velocity records (filled in by frame_enqueue_layer)
};

struct SphRender {
    SphRenderParams p;
    RenderCam cam;
    bool colour_on;                        // sph_frame_set_colour: both frame styles colour the selected particles by sel / lut
    FieldSel sel;
    int* lut;                              // [256 * 3] device copy of lut_host, allocated by the first sph_frame_set_colour
    int lut_host[256 * 3];
    unsigned* range_words;                 // sph_field_range: ordered min, ordered max, then count and non_finite as u64 (24 B)
    int W, H;                              // what the block below is sized for
    void* block;                           // one allocation, carved into:
    unsigned long long* keys;              // [W * H]
    float* depth;                          // [H * W]
    unsigned char* rgb;                    // [H * W * 3]
    unsigned* big_count;                   // device counter of the large-sprite list
    bool have_frame;
};

struct Sprite { float a, b, zc, px, py, inv; int i0, i1, j0, j1; float R; };

// Which particles a splat draws, and into what: every visible one or the visible ones that are not fluid as shaded spheres into
// the min-key plane (with the box edges), or the visible fluid ones into the fluid depth / thickness planes.
// The *_FIELD layers draw what their base layer draws, with the selected particles coloured by the field (FrameField): a table
// colour instead of the object's in the min-key plane, or for the fluid the table index beside the depth in a plane of its own.
enum FrameLayer { LAYER_ALL, LAYER_OPAQUE, LAYER_FLUID, LAYER_ALL_FIELD, LAYER_OPAQUE_FIELD, LAYER_FLUID_FIELD };
constexpr bool layer_field(int layer) { return layer >= LAYER_ALL_FIELD; }
constexpr int layer_base(int layer) { return layer >= LAYER_ALL_FIELD ? layer - LAYER_ALL_FIELD : layer; }

struct FramePlanes {                       // by value; a layer touches only its own
    unsigned long long* keys;              // min-keys: written by LAYER_ALL / LAYER_OPAQUE, read (final by then) by LAYER_FLUID
    unsigned* fz;                          // LAYER_FLUID: fluid depth bits
    unsigned* thick;                       // LAYER_FLUID: thickness sums
};

// Enqueues one layer on the context's stream (sph_render.hip): k_frame_splat<LAYER>, then k_frame_large<LAYER> over the sprites
// the first one listed through `big_count`, a device counter the frame's clear kernel has zeroed.
template <int LAYER>
int frame_enqueue_layer(SphContext* c, const RenderCam& cam, const FramePlanes& planes, unsigned* big_count,
                        const FrameField& field = FrameField{});
// Before the splats of a frame of either style (sph_render.hip): materialises density / pressure if a colouring in force reads them.
int frame_colour_prepare(SphContext* c, const SphRender* r);

#ifdef __HIPCC__
__device__ __forceinline__ float rdot(float ax, float ay, float az, float dx, float dy, float dz) { return (ax * dx + ay * dy) + az * dz; }

__device__ __forceinline__ bool render_visible(const RenderCam& cam, int flags) {
    const int oid = sph_flags_object(flags);
    for (int k = 0; k < cam.n_invisible; ++k)
        if (cam.invisible[k] == oid) return false;
    return true;
}

// projection and clamped bounding box of one particle; false = culled
__device__ __forceinline__ bool render_sprite(const RenderCam& cam, float x, float y, float z, Sprite& s) {
    const float dx = x - cam.ex, dy = y - cam.ey, dz = z - cam.ez;
    s.a = rdot(cam.rx, cam.ry, cam.rz, dx, dy, dz);
    s.b = rdot(cam.ux, cam.uy, cam.uz, dx, dy, dz);
    s.zc = rdot(cam.fx, cam.fy, cam.fz, dx, dy, dz);
    if (!(s.zc >= cam.near_plane)) return false;
    s.px = cam.cx + (cam.focal * s.a) / s.zc;
    s.py = cam.cy - (cam.focal * s.b) / s.zc;
    s.R = cam.fr / s.zc;
    s.inv = s.zc / cam.focal;
    if (!(isfinite(s.px) && isfinite(s.py) && isfinite(s.R))) return false;
    const float Rb = fminf(s.R, SPH_RENDER_MAX_R);
    // clamped in float first: the conversions below see values in [-1, 16384] (a sprite beside the image: an empty range)
    s.i0 = (int)fminf(fmaxf(ceilf((s.px - Rb) - 0.5f), 0.0f), (float)cam.W);
    s.i1 = (int)fmaxf(fminf(floorf((s.px + Rb) - 0.5f), (float)(cam.W - 1)), -1.0f);
    s.j0 = (int)fminf(fmaxf(ceilf((s.py - Rb) - 0.5f), 0.0f), (float)cam.H);
    s.j1 = (int)fmaxf(fminf(floorf((s.py + Rb) - 0.5f), (float)(cam.H - 1)), -1.0f);
    return s.i0 <= s.i1 && s.j0 <= s.j1;
}

__device__ __forceinline__ void render_fragment(const RenderCam& cam, unsigned long long* __restrict__ keys, const Sprite& s,
                                                const float kc[3], int i, int j) {
    const float dx = (((float)i + 0.5f) - s.px) * s.inv;
    const float dy = (s.py - ((float)j + 0.5f)) * s.inv;
    const float h2 = (cam.r2 - dx * dx) - dy * dy;
    if (!(h2 >= 0.0f)) return;
    const float hh = sqrtf(h2);
    const float z = s.zc - hh;
    if (!(z > 0.0f)) return;
    const float nx = dx / cam.radius, ny = dy / cam.radius, nz = hh / cam.radius;
    const float lx = cam.Lx - (s.a + dx), ly = cam.Ly - (s.b + dy), lz = z - cam.Lz;
    const float ll = sqrtf((lx * lx + ly * ly) + lz * lz);
    const float nl = ll > 0.0f ? ((nx * lx + ny * ly) + nz * lz) / ll : 0.0f;
    const float shade = cam.ambient + (1.0f - cam.ambient) * fmaxf(nl, 0.0f);
    unsigned rgb = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t = fminf(fmaxf(kc[k] * shade, 0.0f), 1.0f);
        rgb = (rgb << 8) | (unsigned)(t * 255.0f + 0.5f);
    }
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | rgb;
    unsigned long long* p = keys + (size_t)j * cam.W + i;      // 0 <= i < W, 0 <= j < H by the clamped box
    if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}

// the fluid layer's fragment (sph_surface.hip states its arithmetic): the same sphere, its depth and chord instead of a colour
__device__ __forceinline__ void surface_fragment(const RenderCam& cam, const unsigned long long* __restrict__ keys,
                                                 unsigned* __restrict__ fz, unsigned* __restrict__ thick, const Sprite& s, int i, int j) {
    const float dx = (((float)i + 0.5f) - s.px) * s.inv;
    const float dy = (s.py - ((float)j + 0.5f)) * s.inv;
    const float h2 = (cam.r2 - dx * dx) - dy * dy;
    if (!(h2 >= 0.0f)) return;
    const float hh = sqrtf(h2);
    const float z = s.zc - hh;
    if (!(z > 0.0f)) return;
    const size_t p = (size_t)j * cam.W + i;                    // 0 <= i < W, 0 <= j < H by the clamped box
    const unsigned zb = __float_as_uint(z);
    if (zb < __hip_atomic_load(fz + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(fz + p, zb);
    if (zb < (unsigned)(keys[p] >> 32)) atomicAdd(thick + p, (unsigned)((hh / cam.radius) * 256.0f + 0.5f));   // (the opaque layer is final)
}

// the field-coloured fluid layer's fragment: surface_fragment with the depth's minimum taken together with the table index
__device__ __forceinline__ void surface_field_fragment(const RenderCam& cam, const unsigned long long* __restrict__ keys,
                                                       unsigned* __restrict__ thick, const Sprite& s, int i, int j,
                                                       const FrameField& ff, int idx) {
    unsigned long long* __restrict__ fzi = ff.fzi;
    const float dx = (((float)i + 0.5f) - s.px) * s.inv;
    const float dy = (s.py - ((float)j + 0.5f)) * s.inv;
    const float h2 = (cam.r2 - dx * dx) - dy * dy;
    if (!(h2 >= 0.0f)) return;
    const float hh = sqrtf(h2);
    const float z = s.zc - hh;
    if (!(z > 0.0f)) return;
    const size_t p = (size_t)j * cam.W + i;                    // 0 <= i < W, 0 <= j < H by the clamped box
    const unsigned zb = __float_as_uint(z);
    const unsigned long long key = ((unsigned long long)zb << 32) | (unsigned)idx;
    if (key < __hip_atomic_load(fzi + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(fzi + p, key);
    if (zb < (unsigned)(keys[p] >> 32)) atomicAdd(thick + p, (unsigned)((hh / cam.radius) * 256.0f + 0.5f));   // (the opaque layer is final)
}

// ---- field colouring: field value, table index (the block "Field colouring" of sph_render.hip; the selection: sph_observe.h) ----
__device__ __forceinline__ float field_value(const FieldSel& f, const float4& X, const float4& V, const float4& A) {
    switch (f.field) {
        case SPH_FIELD_SPEED: return sqrtf((V.x * V.x + V.y * V.y) + V.z * V.z);
        case SPH_FIELD_VX: return V.x;
        case SPH_FIELD_VY: return V.y;
        case SPH_FIELD_VZ: return V.z;
        case SPH_FIELD_DENSITY: return A.y;
        case SPH_FIELD_PRESSURE: return A.z;
        case SPH_FIELD_X: return X.x - f.origin;
        case SPH_FIELD_Y: return X.y - f.origin;
        default: return X.z - f.origin;
    }
}

__device__ __forceinline__ int field_index(const FieldSel& f, float s) {
    float t = (s - f.lo) * f.inv;
    t = t >= 0.0f ? fminf(t, 1.0f) : 0.0f;                     // (a NaN compares false: 0)
    return (int)(t * 255.0f + 0.5f);                           // 0 .. 255
}

__device__ __forceinline__ void field_lut_colour(const int* __restrict__ lut, int idx, float kc[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) kc[k] = (float)lut[3 * idx + k] / 255.0f;
}

// a resolved min-key: its colour bytes into rgb[0 .. 2]; returns its depth, +inf where nothing was drawn
__device__ __forceinline__ float render_resolve_key(unsigned long long key, unsigned char* __restrict__ rgb) {
    const unsigned hi = (unsigned)(key >> 32), lo = (unsigned)key;
    rgb[0] = (unsigned char)(lo >> 16);
    rgb[1] = (unsigned char)(lo >> 8);
    rgb[2] = (unsigned char)lo;
    return hi == 0xFFFFFFFFu ? __uint_as_float(0x7F800000u) : __uint_as_float(hi);
}

__device__ __forceinline__ void render_colour(const int* __restrict__ color_cold, int pid, int cold_cap, float kc[3]) {
    const bool ok = pid >= 0 && pid < cold_cap;
#pragma unroll
    for (int k = 0; k < 3; ++k) kc[k] = ok ? (float)color_cold[3 * (size_t)pid + k] / 255.0f : 0.0f;
}

__device__ __forceinline__ void render_box_sample(const RenderCam& cam, unsigned long long* __restrict__ keys, int t) {
    if (t >= 12 * cam.S) return;
    const int e = t / cam.S, m = t - e * cam.S;
    // edge e: axis e / 4, the four edges along it told apart by the two other coordinates (0 or box_end)
    const int axis = e >> 2, c1 = e & 1, c2 = (e >> 1) & 1;
    const float end[3] = {cam.bex, cam.bey, cam.bez};
    float A[3], B[3];
    const int o1 = (axis + 1) % 3, o2 = (axis + 2) % 3;
    A[axis] = 0.0f; B[axis] = end[axis];
    A[o1] = B[o1] = c1 ? end[o1] : 0.0f;
    A[o2] = B[o2] = c2 ? end[o2] : 0.0f;
    const float tt = ((float)m + 0.5f) / (float)cam.S;
    const float dx = (A[0] + (B[0] - A[0]) * tt) - cam.ex, dy = (A[1] + (B[1] - A[1]) * tt) - cam.ey, dz = (A[2] + (B[2] - A[2]) * tt) - cam.ez;
    const float a = rdot(cam.rx, cam.ry, cam.rz, dx, dy, dz);
    const float b = rdot(cam.ux, cam.uy, cam.uz, dx, dy, dz);
    const float zc = rdot(cam.fx, cam.fy, cam.fz, dx, dy, dz);
    if (!(zc >= cam.near_plane)) return;
    const float px = cam.cx + (cam.focal * a) / zc;
    const float py = cam.cy - (cam.focal * b) / zc;
    if (!(px >= 0.0f && px < (float)cam.W && py >= 0.0f && py < (float)cam.H)) return;   // (false for NaN too)
    const int i = (int)px, j = (int)py;
    const unsigned long long key = ((unsigned long long)__float_as_uint(zc) << 32) | cam.box_rgb;
    unsigned long long* p = keys + (size_t)j * cam.W + i;
    if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}
#endif  // __HIPCC__
