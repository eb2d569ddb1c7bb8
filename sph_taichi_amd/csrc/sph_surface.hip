// sph_surface.hip -- surface frames: the fluid as ONE screen-space surface (splatted depth and thickness, depth smoothed in
// image space, normals from the smoothed depth, shading with absorption by thickness) composited over the opaque layer, which
// is the sphere frame's own picture (sph_render.hip) of every particle that is not fluid plus the box edges.  A second frame
// style beside the sphere frame; it shares that frame's camera, invisible set and device functions (sph_render_dev.h) and
// changes none of them.
//
// Launches per frame (all on the context's stream; particle state is read, never written; n = width * height pixels):
//   k_surface_clear         keys = 0xFFFFFFFF'00000000 | background, fluid depth bits = 0xFFFFFFFF, thickness sum = 0, both
//                           large-sprite counters = 0                                                        writes 16 n B
//   k_frame_splat<LAYER_OPAQUE>  one lane per particle that is visible and NOT fluid: small sprites rasterised by their lane
//                           into the 64-bit min-key plane, large ones listed; the launch's last blocks: the box edges
//   k_frame_large<LAYER_OPAQUE>  one wave per listed sprite                            (32 B per particle read: xm, vf; aux + colour
//                                                                                       of the drawn ones; atomics per fragment)
//   k_frame_splat<LAYER_FLUID>   the same split over the visible FLUID particles: per fragment a u32 atomicMin into the fluid
//   k_frame_large<LAYER_FLUID>   depth and, in front of the (now final) opaque depth, a u32 atomicAdd into the thickness sum
//                                                                                      (32 B per particle; per fragment 8 B key read)
//                           (the sphere frame's splat pair, sph_render.hip, enqueued per layer by frame_enqueue_layer)
//   k_surface_smooth_depth  x iterations, ping-pong between two planes: 16 x 16 output pixels per block, the 48 x 48 window
//                           around them staged in LDS (9216 B); per pass reads 4 n B * (48 / 16)^2 = 36 n B through the cache
//                           hierarchy (4 n B of them new), writes 4 n B; up to 33^2 = 1089 LDS taps per pixel
//   k_surface_smooth_thick  once, the same tiling over the thickness: reads 2 x 4 n B (x 9 with the halo), writes 4 n B
//   k_surface_resolve       one lane per pixel: reads 8 n B keys, 5 x 4 n B smoothed depth (centre + 4 neighbours, cached),
//                           4 n B thickness; writes 3 n + 4 n + 4 n B
// Every loop is bounded: sprites as in sph_render.hip, filter windows by SPH_SURFACE_MAX_FILTER_R.  No kernel waits for
// another workgroup.
//
// Order independence: the splats accumulate an integer minimum (keys, fluid depth) and an integer sum (thickness); each
// fragment's contribution depends on its particle and its pixel only, except for the test against the opaque depth, which is
// FINAL when the fluid splat starts (a launch of its own).  Every later pass computes one pixel from a fixed window of the
// previous plane in a fixed order.  So all three outputs are functions of the SET of particles.
//
// ---- THE ARITHMETIC (tests/surface_model.py follows this block line by line) ---------------------------------------
// IEEE binary32, one rounding per written operation, evaluated left to right with the parentheses shown; no contraction
// (pragma below), correctly rounded divide and sqrt, no exp / pow / reciprocal / rsq intrinsic.  Camera, sprite, fragment and
// box-edge quantities (cx, cy, focal, radius, L, ambient, a, b, zc, px, py, inv, dx, dy, h2, hh, z, keys) are those of the
// block in sph_render.hip.  dot3(p, q) := (p.x q.x + p.y q.y) + p.z q.z.  inf = +infinity.
//
// Host, binary32: fw = filter_radius * focal;  tk = radius * (2 / 256)  (2 / 256 = 0.0078125 exactly).
//
// Opaque layer: the sphere frame's keys over the visible particles whose material is not fluid, plus the box edges.
//   zo = float of a key's high 32 bits, inf where they are 0xFFFFFFFF;  behind[k] = float(the key's colour byte k) / 255.
// Fluid fragment (a visible fluid particle's sprite at pixel i, j; dx, dy, h2, hh, z as for a sphere fragment, the same skips):
//   D = min(D, bits(z))                                                             u32, starts at 0xFFFFFFFF
//   if bits(z) < high 32 bits of the pixel's opaque key:  S = S + uint((hh / radius) * 256 + 0.5)      u32, truncation
// Raw planes: z0 = float of D, inf where D is 0xFFFFFFFF;  t0 = float(S) * tk.  A pixel HAS FLUID iff z0 is finite.
//
// Filter radius of a pixel with finite depth z:  R(z) = int(min(max(ceil(fw / z), 1), 16)).
// Depth smoothing, pass m = 1 .. iterations, from plane z(m-1) to z(m); a pixel p without fluid stays inf; else with zp = z(m-1)[p]:
//   R = R(zp);  R2 = float(R * R);  sw = 0;  sz = 0
//   for dj = -R .. R (outer), di = -R .. R (inner), q = (i + di, j + dj) inside the image with finite zq = z(m-1)[q]:
//     s2 = float(di * di + dj * dj) / R2;  skip unless s2 < 1;  ws = (1 - s2) * (1 - s2)
//     d = (zq - zp) / depth_range;  r2 = d * d;  skip unless r2 < 1;  wr = (1 - r2) * (1 - r2)
//     w = ws * wr;  sw = sw + w;  sz = sz + w * zq
//   z(m)[p] = sz / sw                                                               (the centre tap has w = 1: sw >= 1)
//   zs := z(iterations).
// Thickness smoothing, one pass; a pixel without fluid gets ts = 0; else
//   R = R(z0[p]), R2 as above;  sw = 0;  st = 0
//   for dj, di as above over the q inside the image that have fluid:  s2, ws as above;  sw = sw + ws;  st = st + ws * t0[q]
//   ts[p] = st / sw
// Shade and resolve, pixel (i, j) with z = zs[p]:  the pixel SHOWS FLUID iff z is finite and z < zo.  Otherwise it is the
// opaque layer's: rgb = the key's colour bytes, depth = zo, thickness = 0.  If it shows fluid, in view space with x right,
// y up and the third axis ALONG the view direction (a normal that faces the eye has a negative third component):
//   point of pixel (i', j') at depth z':  zf' = z' / focal;  P' = (((i' + 0.5) - cx) * zf', (cy - (j' + 0.5)) * zf', z')
//   P = the pixel's own point, zf = z / focal
//   A neighbour is USABLE if it is inside the image and its zs is finite.  E = (i + 1, j), W = (i - 1, j), N = (i, j - 1), S = (i, j + 1).
//   axis i:  E if E is usable and (W is not, or |zE - z| <= |z - zW|):  A = PE - P;  else W if usable:  A = P - PW;  else A = (zf, 0, 0)
//   axis j:  N if N is usable and (S is not, or |zN - z| <= |z - zS|):  B = PN - P;  else S if usable:  B = P - PS;  else B = (0, zf, 0)
//            (component-wise differences; a tie takes the +i / -j side)
//   c = (A.z * B.y - A.y * B.z,  A.x * B.z - A.z * B.x,  A.y * B.x - A.x * B.y)             B x A: faces the eye for a facing plane
//   cl = sqrt(dot3(c, c));  n = cl > 0 ? c / cl : (0, 0, -1)                         (cl = NaN counts as not > 0)
//   e = (0 - P.x, 0 - P.y, 0 - P.z);  el = sqrt(dot3(e, e));  v = e / el             towards the eye; el >= z > 0
//   nv = dot3(n, v);  if nv < 0:  n = (0 - n.x, 0 - n.y, 0 - n.z),  nv = 0 - nv
//   l = (L.x - P.x, L.y - P.y, L.z - P.z);  ll = sqrt(dot3(l, l))
//   if ll > 0:  lu = l / ll;  nl = max(dot3(n, lu), 0);  h = lu + v;  hl = sqrt(dot3(h, h));  nh = hl > 0 ? max(dot3(n, h) / hl, 0) : 0
//   else:       nl = 0;  nh = 0
//   s = nh;  six times s = s * s;  spec = specular * s                               (n.h)^64
//   m = 1 - max(nv, 0);  m2 = m * m;  m4 = m2 * m2;  m5 = m4 * m;  F = f0 + (1 - f0) * m5
//   lit = ambient + (1 - ambient) * nl;  t = ts[p]
//   per channel k:  ak = 1 + absorb[k] * t;  T = 1 / (ak * ak)
//     col = ((T * behind[k] + (1 - T) * (fluid_color[k] * lit)) * (1 - F) + F * sky[k]) + spec
//     byte k = uint(min(max(col, 0), 1) * 255 + 0.5)                                 truncation; a NaN col gives 0
//   depth = z;  thickness = t.
//
// ---- WITH A FIELD COLOURING (sph_frame_set_colour; tests/fieldcolour_model.py follows this block) ------------------
// A frame without one runs none of what follows and allocates none of its planes.  idx of a particle, lut and SELECTED are those
// of the block "Field colouring" in sph_render.hip.
// Opaque layer: if the colouring's material is not fluid, its selected particles take kc[k] = float(lut[idx][k]) / 255 there
//   (k_frame_splat / k_frame_large<LAYER_OPAQUE_FIELD>); else the layer is the one above.
// Fluid layer: if the colouring's material is fluid or any, k_frame_splat / k_frame_large<LAYER_FLUID_FIELD> take the place of
//   the <LAYER_FLUID> pair (else the fluid is drawn as above).  A fluid fragment (the same sphere, the same skips), with
//   e = idx if its particle is selected, else 256:
//     Q = min(Q, bits(z) << 32 | e)                                                 u64, starts at 0xFFFFFFFF'FFFFFFFF
//     S as above.
//   D := the high 32 bits of Q (k_surface_field_split); depth and thickness smoothing read it as above.  The low 32 bits are
//   the e of the pixel's nearest fluid fragment, the smaller e among fragments of equal depth: a function of the set.
// A pixel HAS AN INDEX iff it has fluid and its e is not 256; then v0 = float(e).
// Index smoothing (k_surface_smooth_index), one pass; a pixel p without an index gets I[p] = -1; else
//   R = R(z0[p]), R2 as above;  sw = 0;  sv = 0
//   for dj, di as above over the q inside the image that have an index:  s2, ws as in the thickness pass;
//     sw = sw + ws;  sv = sv + ws * v0[q]
//   v = sv / sw;  I[p] = int(min(max(v + 0.5, 0), 255))                              truncation (the centre tap has ws = 1: sw >= 1)
// Shade: in col, fluid_color[k] is replaced by float(lut[I[p]][k]) / 255 where I[p] >= 0; everything else is unchanged.
#include <math.h>

#include "sph_render_dev.h"

#pragma clang fp contract(off)

#define STILE 16
#define SHALO SPH_SURFACE_MAX_FILTER_R
#define SLDS (STILE + 2 * SHALO)     // 48: the staged window of a 16 x 16 output tile
#define SURF_INF_BITS 0x7F800000u
#define SURF_NONE 0xFFFFFFFFu        // "no depth" in every u32 depth plane (not the bits of a float any pass writes)

struct SurfK {                       // the style, by value
    float fw, depth_range, tk;
    float fluid[3], absorb[3], sky[3], f0, specular;
};

struct SphSurface {
    SphSurfaceParams p;
    bool have_params;
    int W, H;                         // what the block below is sized for
    void* block;                      // one allocation, carved into:
    unsigned long long* keys;         // [n] opaque min-keys
    unsigned* fz;                     // [n] fluid depth bits
    unsigned* thick;                  // [n] thickness sums
    unsigned* plane[2];               // [n] each: smoothed depth, ping-pong (float bits, SURF_NONE never occurs in them)
    float* ts;                        // [n] smoothed thickness
    float* depth;                     // [n] output
    float* thickness;                 // [n] output
    unsigned char* rgb;               // [3 n] output
    unsigned* counts;                 // [2] large-sprite counters: opaque, fluid
    bool have_frame;
    // only for frames with a field colouring: a second allocation, made by the first such frame
    int fW, fH;                       // what it is sized for
    void* fblock;                     // carved into:
    unsigned long long* fzi;          // [n] min of bits(z) << 32 | index over the fluid fragments
    int* fidx;                        // [n] smoothed table index, -1 where the pixel has none
    bool have_index;                  // the last frame wrote fidx
};

__device__ __forceinline__ float surf_depth(unsigned bits) { return __uint_as_float(bits == SURF_NONE ? SURF_INF_BITS : bits); }

__device__ __forceinline__ int surf_radius(float fw, float z) { return (int)fminf(fmaxf(ceilf(fw / z), 1.0f), (float)SPH_SURFACE_MAX_FILTER_R); }

__global__ __launch_bounds__(RTPB) void k_surface_clear(unsigned long long* __restrict__ keys, unsigned* __restrict__ fz,
                                                        unsigned* __restrict__ thick, int n_pix, unsigned background,
                                                        unsigned* __restrict__ counts) {
    const int i = blockIdx.x * RTPB + threadIdx.x;
    if (i < 2) counts[i] = 0u;
    if (i < n_pix) {
        keys[i] = 0xFFFFFFFF00000000ull | background;
        fz[i] = SURF_NONE;
        thick[i] = 0u;
    }
}

// One block = 16 x 16 output pixels (thread t: column t & 15, row t >> 4); the 48 x 48 window around them goes through LDS.
// Window pixels outside the image are staged as "no fluid".
__global__ __launch_bounds__(STILE * STILE) void k_surface_smooth_depth(int W, int H, float fw, float depth_range,
                                                                        const unsigned* __restrict__ src, unsigned* __restrict__ dst) {
    __shared__ float tile[SLDS][SLDS];
    const int tx = threadIdx.x & (STILE - 1), ty = threadIdx.x >> 4;
    const int bi = blockIdx.x * STILE, bj = blockIdx.y * STILE;
    for (int t = threadIdx.x; t < SLDS * SLDS; t += STILE * STILE) {
        const int ly = t / SLDS, lx = t - ly * SLDS;
        const int gi = bi - SHALO + lx, gj = bj - SHALO + ly;
        const bool in = gi >= 0 && gi < W && gj >= 0 && gj < H;
        tile[ly][lx] = surf_depth(in ? src[(size_t)gj * W + gi] : SURF_NONE);
    }
    __syncthreads();
    const int i = bi + tx, j = bj + ty;
    if (i >= W || j >= H) return;
    const float zp = tile[ty + SHALO][tx + SHALO];
    const size_t p = (size_t)j * W + i;
    if (!isfinite(zp)) { dst[p] = SURF_INF_BITS; return; }
    const int R = surf_radius(fw, zp);                     // 1 .. SHALO: every tap below lies inside the staged window
    const float R2 = (float)(R * R);
    float sw = 0.0f, sz = 0.0f;
    for (int dj = -R; dj <= R; ++dj)
        for (int di = -R; di <= R; ++di) {
            const float zq = tile[ty + SHALO + dj][tx + SHALO + di];
            if (!isfinite(zq)) continue;
            const float s2 = (float)(di * di + dj * dj) / R2;
            if (!(s2 < 1.0f)) continue;
            const float ws = (1.0f - s2) * (1.0f - s2);
            const float d = (zq - zp) / depth_range;
            const float r2 = d * d;
            if (!(r2 < 1.0f)) continue;
            const float wr = (1.0f - r2) * (1.0f - r2);
            const float w = ws * wr;
            sw = sw + w;
            sz = sz + w * zq;
        }
    dst[p] = __float_as_uint(sz / sw);
}

// The same tiling over the raw thickness; a staged value < 0 means "no fluid there" (a thickness is never negative).
__global__ __launch_bounds__(STILE * STILE) void k_surface_smooth_thick(int W, int H, float fw, float tk, const unsigned* __restrict__ fz,
                                                                        const unsigned* __restrict__ thick, float* __restrict__ ts) {
    __shared__ float tile[SLDS][SLDS];
    const int tx = threadIdx.x & (STILE - 1), ty = threadIdx.x >> 4;
    const int bi = blockIdx.x * STILE, bj = blockIdx.y * STILE;
    for (int t = threadIdx.x; t < SLDS * SLDS; t += STILE * STILE) {
        const int ly = t / SLDS, lx = t - ly * SLDS;
        const int gi = bi - SHALO + lx, gj = bj - SHALO + ly;
        float v = -1.0f;
        if (gi >= 0 && gi < W && gj >= 0 && gj < H) {
            const size_t q = (size_t)gj * W + gi;
            if (fz[q] != SURF_NONE) v = (float)thick[q] * tk;
        }
        tile[ly][lx] = v;
    }
    __syncthreads();
    const int i = bi + tx, j = bj + ty;
    if (i >= W || j >= H) return;
    const size_t p = (size_t)j * W + i;
    const unsigned zb = fz[p];
    if (zb == SURF_NONE) { ts[p] = 0.0f; return; }
    const int R = surf_radius(fw, __uint_as_float(zb));
    const float R2 = (float)(R * R);
    float sw = 0.0f, st = 0.0f;
    for (int dj = -R; dj <= R; ++dj)
        for (int di = -R; di <= R; ++di) {
            const float tq = tile[ty + SHALO + dj][tx + SHALO + di];
            if (tq < 0.0f) continue;
            const float s2 = (float)(di * di + dj * dj) / R2;
            if (!(s2 < 1.0f)) continue;
            const float ws = (1.0f - s2) * (1.0f - s2);
            sw = sw + ws;
            st = st + ws * tq;
        }
    ts[p] = st / sw;
}

struct V3 { float x, y, z; };
__device__ __forceinline__ float dot3(const V3& p, const V3& q) { return (p.x * q.x + p.y * q.y) + p.z * q.z; }
__device__ __forceinline__ V3 surf_point(const RenderCam& cam, int i, int j, float z) {
    const float zf = z / cam.focal;
    return V3{(((float)i + 0.5f) - cam.cx) * zf, (cam.cy - ((float)j + 0.5f)) * zf, z};
}
__device__ __forceinline__ V3 sub3(const V3& p, const V3& q) { return V3{p.x - q.x, p.y - q.y, p.z - q.z}; }

// the fluid's body colour of pixel pix, channel k: the style's, or with a field colouring (the two extra kernel arguments) the
// table's where the pixel has an index
__device__ __forceinline__ float surf_body(const SurfK& sk, int, int k) { return sk.fluid[k]; }
__device__ __forceinline__ float surf_body(const SurfK& sk, int pix, int k, const int* __restrict__ fidx, const int* __restrict__ lut) {
    const int fi = fidx[pix];                                  // -1 or 0 .. 255
    return fi >= 0 ? (float)lut[3 * fi + k] / 255.0f : sk.fluid[k];
}

// FIELD... = nothing: the frame without a colouring, with the arguments and the code it always had; = (fidx, lut): with one
template <class... FIELD>
__global__ __launch_bounds__(RTPB) void k_surface_resolve(RenderCam cam, SurfK sk, const unsigned long long* __restrict__ keys,
                                                          const unsigned* __restrict__ zs, const float* __restrict__ ts,
                                                          unsigned char* __restrict__ rgb, float* __restrict__ depth,
                                                          float* __restrict__ thickness, FIELD... field) {
    const int pix = blockIdx.x * RTPB + threadIdx.x;
    if (pix >= cam.W * cam.H) return;
    const int j = pix / cam.W, i = pix - j * cam.W;
    const unsigned long long key = keys[pix];
    const unsigned lo = (unsigned)key;
    const float zo = surf_depth((unsigned)(key >> 32));
    const float z = surf_depth(zs[pix]);
    if (!(isfinite(z) && z < zo)) {          // the opaque layer's pixel, as the sphere frame resolves it
        depth[pix] = render_resolve_key(key, rgb + 3 * (size_t)pix);
        thickness[pix] = 0.0f;
        return;
    }
    const float inf = __uint_as_float(SURF_INF_BITS);
    const float zE = i + 1 < cam.W ? surf_depth(zs[pix + 1]) : inf;
    const float zW = i > 0 ? surf_depth(zs[pix - 1]) : inf;
    const float zN = j > 0 ? surf_depth(zs[pix - cam.W]) : inf;
    const float zS = j + 1 < cam.H ? surf_depth(zs[pix + cam.W]) : inf;
    const bool uE = isfinite(zE), uW = isfinite(zW), uN = isfinite(zN), uS = isfinite(zS);
    const float zf = z / cam.focal;
    const V3 P = surf_point(cam, i, j, z);
    V3 A, B;
    if (uE && (!uW || fabsf(zE - z) <= fabsf(z - zW))) A = sub3(surf_point(cam, i + 1, j, zE), P);
    else if (uW) A = sub3(P, surf_point(cam, i - 1, j, zW));
    else A = V3{zf, 0.0f, 0.0f};
    if (uN && (!uS || fabsf(zN - z) <= fabsf(z - zS))) B = sub3(surf_point(cam, i, j - 1, zN), P);
    else if (uS) B = sub3(P, surf_point(cam, i, j + 1, zS));
    else B = V3{0.0f, zf, 0.0f};
    const V3 c = V3{A.z * B.y - A.y * B.z, A.x * B.z - A.z * B.x, A.y * B.x - A.x * B.y};
    const float cl = sqrtf(dot3(c, c));
    V3 n = cl > 0.0f ? V3{c.x / cl, c.y / cl, c.z / cl} : V3{0.0f, 0.0f, -1.0f};
    const V3 e = V3{0.0f - P.x, 0.0f - P.y, 0.0f - P.z};
    const float el = sqrtf(dot3(e, e));
    const V3 v = V3{e.x / el, e.y / el, e.z / el};
    float nv = dot3(n, v);
    if (nv < 0.0f) { n = V3{0.0f - n.x, 0.0f - n.y, 0.0f - n.z}; nv = 0.0f - nv; }
    const V3 l = V3{cam.Lx - P.x, cam.Ly - P.y, cam.Lz - P.z};
    const float ll = sqrtf(dot3(l, l));
    float nl = 0.0f, nh = 0.0f;
    if (ll > 0.0f) {
        const V3 lu = V3{l.x / ll, l.y / ll, l.z / ll};
        nl = fmaxf(dot3(n, lu), 0.0f);
        const V3 h = V3{lu.x + v.x, lu.y + v.y, lu.z + v.z};
        const float hl = sqrtf(dot3(h, h));
        nh = hl > 0.0f ? fmaxf(dot3(n, h) / hl, 0.0f) : 0.0f;
    }
    float s = nh;
#pragma unroll
    for (int k = 0; k < 6; ++k) s = s * s;
    const float spec = sk.specular * s;
    const float m = 1.0f - fmaxf(nv, 0.0f);
    const float m2 = m * m, m4 = m2 * m2, m5 = m4 * m;
    const float F = sk.f0 + (1.0f - sk.f0) * m5;
    const float lit = cam.ambient + (1.0f - cam.ambient) * nl;
    const float t = ts[pix];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float behind = (float)((lo >> (16 - 8 * k)) & 255u) / 255.0f;
        const float ak = 1.0f + sk.absorb[k] * t;
        const float T = 1.0f / (ak * ak);
        const float col = ((T * behind + (1.0f - T) * (surf_body(sk, pix, k, field...) * lit)) * (1.0f - F) + F * sk.sky[k]) + spec;
        rgb[3 * (size_t)pix + k] = (unsigned char)(unsigned)(fminf(fmaxf(col, 0.0f), 1.0f) * 255.0f + 0.5f);
    }
    depth[pix] = z;
    thickness[pix] = t;
}

// ---- with a field colouring --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RTPB) void k_surface_field_clear(unsigned long long* __restrict__ fzi, int n_pix) {
    const int i = blockIdx.x * RTPB + threadIdx.x;
    if (i < n_pix) fzi[i] = 0xFFFFFFFFFFFFFFFFull;
}

// the fluid depth plane the filters read = the high half of the index keys
__global__ __launch_bounds__(RTPB) void k_surface_field_split(const unsigned long long* __restrict__ fzi, unsigned* __restrict__ fz, int n_pix) {
    const int i = blockIdx.x * RTPB + threadIdx.x;
    if (i < n_pix) fz[i] = (unsigned)(fzi[i] >> 32);
}

// The tiling of k_surface_smooth_thick over the table indices; a staged value < 0 means "no index there".
__global__ __launch_bounds__(STILE * STILE) void k_surface_smooth_index(int W, int H, float fw, const unsigned long long* __restrict__ fzi,
                                                                        int* __restrict__ fidx) {
    __shared__ float tile[SLDS][SLDS];
    const int tx = threadIdx.x & (STILE - 1), ty = threadIdx.x >> 4;
    const int bi = blockIdx.x * STILE, bj = blockIdx.y * STILE;
    for (int t = threadIdx.x; t < SLDS * SLDS; t += STILE * STILE) {
        const int ly = t / SLDS, lx = t - ly * SLDS;
        const int gi = bi - SHALO + lx, gj = bj - SHALO + ly;
        float v = -1.0f;
        if (gi >= 0 && gi < W && gj >= 0 && gj < H) {
            const unsigned long long q = fzi[(size_t)gj * W + gi];
            const unsigned e = (unsigned)q;
            if ((unsigned)(q >> 32) != SURF_NONE && e < (unsigned)FIELD_IDX_NONE) v = (float)e;
        }
        tile[ly][lx] = v;
    }
    __syncthreads();
    const int i = bi + tx, j = bj + ty;
    if (i >= W || j >= H) return;
    const size_t p = (size_t)j * W + i;
    const unsigned zb = (unsigned)(fzi[p] >> 32);
    if (tile[ty + SHALO][tx + SHALO] < 0.0f) { fidx[p] = -1; return; }
    const int R = surf_radius(fw, __uint_as_float(zb));        // 1 .. SHALO: every tap below lies inside the staged window
    const float R2 = (float)(R * R);
    float sw = 0.0f, sv = 0.0f;
    for (int dj = -R; dj <= R; ++dj)
        for (int di = -R; di <= R; ++di) {
            const float vq = tile[ty + SHALO + dj][tx + SHALO + di];
            if (vq < 0.0f) continue;
            const float s2 = (float)(di * di + dj * dj) / R2;
            if (!(s2 < 1.0f)) continue;
            const float ws = (1.0f - s2) * (1.0f - s2);
            sw = sw + ws;
            sv = sv + ws * vq;
        }
    fidx[p] = (int)fminf(fmaxf(sv / sw + 0.5f, 0.0f), 255.0f);
}

// ---- host ------------------------------------------------------------------------------------------------------------
void sph_surface_release(SphContext* c) { sph_observe_release(c->surface, &SphSurface::block, &SphSurface::fblock); }

// the planes of a frame with a field colouring (12 bytes per pixel)
static int surface_field_alloc(SphContext* c, SphSurface* s, int W, int H) {
    if (s->fblock && s->fW == W && s->fH == H) return 0;
    s->fW = s->fH = 0; s->have_index = false;
    const size_t n = (size_t)W * H;        // n <= 2^28
    if (int rc = sph_observe_alloc(c, &s->fblock, 12 * n, "sph_surface_frame", "the field-index planes")) return rc;
    s->fzi = (unsigned long long*)s->fblock;
    s->fidx = (int*)((char*)s->fblock + 8 * n);
    s->fW = W; s->fH = H;
    return 0;
}

static int surface_alloc(SphContext* c, SphSurface* s, int W, int H) {
    if (s->block && s->W == W && s->H == H) return 0;
    s->W = s->H = 0; s->have_frame = false;
    const size_t n = (size_t)W * H, rgb_bytes = (3 * n + 15) & ~(size_t)15;        // n <= 2^28
    if (int rc = sph_observe_alloc(c, &s->block, 8 * n + 7 * 4 * n + rgb_bytes + 16, "sph_surface_frame", "the frame buffers")) return rc;
    char* b = (char*)s->block;
    s->keys = (unsigned long long*)b; b += 8 * n;
    s->fz = (unsigned*)b; b += 4 * n;
    s->thick = (unsigned*)b; b += 4 * n;
    s->plane[0] = (unsigned*)b; b += 4 * n;
    s->plane[1] = (unsigned*)b; b += 4 * n;
    s->ts = (float*)b; b += 4 * n;
    s->depth = (float*)b; b += 4 * n;
    s->thickness = (float*)b; b += 4 * n;
    s->rgb = (unsigned char*)b; b += rgb_bytes;
    s->counts = (unsigned*)b;
    s->W = W; s->H = H;
    return 0;
}

static const char* check_params(const SphSurfaceParams& p) {
    if (p.iterations < 0 || p.iterations > SPH_SURFACE_MAX_ITERATIONS) return "sph_surface_set_params: iterations must be in [0, 8]";
    if (!(p.filter_radius > 0.0f) || !isfinite(p.filter_radius)) return "sph_surface_set_params: filter_radius must be positive";
    if (!(p.depth_range > 0.0f) || !isfinite(p.depth_range)) return "sph_surface_set_params: depth_range must be positive";
    for (int k = 0; k < 3; ++k) {
        if (!(p.fluid_color[k] >= 0.0f && p.fluid_color[k] <= 1.0f)) return "sph_surface_set_params: fluid_color must be in [0, 1]";
        if (!(p.sky[k] >= 0.0f && p.sky[k] <= 1.0f)) return "sph_surface_set_params: sky must be in [0, 1]";
        if (!(p.absorb[k] >= 0.0f) || !isfinite(p.absorb[k])) return "sph_surface_set_params: absorb must be finite and not negative";
    }
    if (!(p.f0 >= 0.0f && p.f0 <= 1.0f)) return "sph_surface_set_params: f0 must be in [0, 1]";
    if (!(p.specular >= 0.0f) || !isfinite(p.specular)) return "sph_surface_set_params: specular must be finite and not negative";
    return nullptr;
}

// the frame; ev: null, or SPH_SURFACE_PASSES + 1 events recorded around the passes
static int surface_frame(SphContext* c, hipEvent_t* ev) {
    if (int rc = sph_observe_enter(c, "sph_surface_frame", FRAME_SLAB_WHY)) return rc;
    const SphRender* r = c->render;
    if (!r || r->cam.W <= 0) return sph_fail(c, SPH_E_STATE, "sph_surface_frame needs the camera of the sphere frame (its set_params call) first");
    SphSurface* s = c->surface;
    if (!s || !s->have_params) return sph_fail(c, SPH_E_STATE, "sph_surface_frame needs sph_surface_set_params first");
    const RenderCam& cam = r->cam;
    if (int rc = surface_alloc(c, s, cam.W, cam.H)) return rc;
    // a field colouring: which of the two layers holds selected particles (a material other than fluid: only the opaque one)
    const bool opaque_field = r->colour_on && r->sel.who.material != SPH_MATERIAL_FLUID;
    const bool fluid_field = r->colour_on && (r->sel.who.material < 0 || r->sel.who.material == SPH_MATERIAL_FLUID);
    if (fluid_field)
        if (int rc = surface_field_alloc(c, s, cam.W, cam.H)) return rc;
    if (int rc = frame_colour_prepare(c, r)) return rc;
    const FrameField field{r->sel, r->lut, fluid_field ? s->fzi : nullptr};
    s->have_index = false;
    SurfK sk;
    sk.fw = s->p.filter_radius * cam.focal;
    sk.depth_range = s->p.depth_range;
    sk.tk = cam.radius * (2.0f / 256.0f);
    for (int k = 0; k < 3; ++k) { sk.fluid[k] = s->p.fluid_color[k]; sk.absorb[k] = s->p.absorb[k]; sk.sky[k] = s->p.sky[k]; }
    sk.f0 = s->p.f0; sk.specular = s->p.specular;
    const int n_pix = cam.W * cam.H;     // <= 2^28
    const int pix_blocks = (n_pix + RTPB - 1) / RTPB;
    const FramePlanes planes{s->keys, s->fz, s->thick};
    int e = 0;
#define SURF_MARK() do { if (ev) SPH_HIP(c, hipEventRecord(ev[e++], c->stream)); } while (0)
    SURF_MARK();
    hipLaunchKernelGGL(k_surface_clear, dim3(pix_blocks), dim3(RTPB), 0, c->stream, s->keys, s->fz, s->thick, n_pix, cam.background, s->counts);
    SPH_LAUNCH_CHECK(c);
    if (fluid_field) {
        hipLaunchKernelGGL(k_surface_field_clear, dim3(pix_blocks), dim3(RTPB), 0, c->stream, s->fzi, n_pix);
        SPH_LAUNCH_CHECK(c);
    }
    SURF_MARK();
    if (opaque_field) {
        if (int rc = frame_enqueue_layer<LAYER_OPAQUE_FIELD>(c, cam, planes, s->counts + 0, field)) return rc;
    } else {
        if (int rc = frame_enqueue_layer<LAYER_OPAQUE>(c, cam, planes, s->counts + 0)) return rc;
    }
    SURF_MARK();
    if (fluid_field) {
        if (int rc = frame_enqueue_layer<LAYER_FLUID_FIELD>(c, cam, planes, s->counts + 1, field)) return rc;
        hipLaunchKernelGGL(k_surface_field_split, dim3(pix_blocks), dim3(RTPB), 0, c->stream, s->fzi, s->fz, n_pix);
        SPH_LAUNCH_CHECK(c);
    } else {
        if (int rc = frame_enqueue_layer<LAYER_FLUID>(c, cam, planes, s->counts + 1)) return rc;
    }
    SURF_MARK();
    const dim3 tiles((cam.W + STILE - 1) / STILE, (cam.H + STILE - 1) / STILE);
    const unsigned* zs = s->fz;
    for (int m = 0; m < s->p.iterations; ++m) {
        unsigned* dst = s->plane[m & 1];
        hipLaunchKernelGGL(k_surface_smooth_depth, tiles, dim3(STILE * STILE), 0, c->stream, cam.W, cam.H, sk.fw, sk.depth_range, zs, dst);
        SPH_LAUNCH_CHECK(c);
        zs = dst;
    }
    SURF_MARK();
    hipLaunchKernelGGL(k_surface_smooth_thick, tiles, dim3(STILE * STILE), 0, c->stream, cam.W, cam.H, sk.fw, sk.tk, s->fz, s->thick, s->ts);
    SPH_LAUNCH_CHECK(c);
    if (fluid_field) {
        hipLaunchKernelGGL(k_surface_smooth_index, tiles, dim3(STILE * STILE), 0, c->stream, cam.W, cam.H, sk.fw, s->fzi, s->fidx);
        SPH_LAUNCH_CHECK(c);
    }
    SURF_MARK();
    if (fluid_field)
        hipLaunchKernelGGL((k_surface_resolve<const int*, const int*>), dim3(pix_blocks), dim3(RTPB), 0, c->stream, cam, sk, s->keys, zs, s->ts,
                           s->rgb, s->depth, s->thickness, (const int*)s->fidx, (const int*)r->lut);
    else
        hipLaunchKernelGGL(k_surface_resolve<>, dim3(pix_blocks), dim3(RTPB), 0, c->stream, cam, sk, s->keys, zs, s->ts, s->rgb, s->depth, s->thickness);
    SPH_LAUNCH_CHECK(c);
    SURF_MARK();
#undef SURF_MARK
    s->have_frame = true;
    s->have_index = fluid_field;
    return 0;
}

static int surface_download(SphContext* c, void* host, size_t bytes, int which) {
    if (!c) return SPH_E_INVALID;
    SphSurface* s = c->surface;
    if (!s || !s->have_frame) return sph_fail(c, SPH_E_STATE, "sph_surface_download: no surface frame has been rendered");
    const size_t want = (size_t)s->W * s->H * (which == 0 ? 3 : 4);
    if (!host || bytes != want) return sph_fail(c, SPH_E_INVALID, "sph_surface_download: size mismatch (u8 [H, W, 3] / f32 [H, W] of the last surface frame)");
    const void* src = which == 0 ? (const void*)s->rgb : which == 1 ? (const void*)s->depth : (const void*)s->thickness;
    return sph_observe_download(c, host, src, bytes);
}

extern "C" {

int32_t sph_surface_set_params(SphContext* c, const SphSurfaceParams* params) {
    if (c && !params) return sph_fail(c, SPH_E_INVALID, "sph_surface_set_params: null argument");
    if (int rc = sph_observe_enter(c, "sph_surface_set_params", FRAME_SLAB_WHY)) return rc;
    if (const char* what = check_params(*params)) return sph_fail(c, SPH_E_INVALID, what);
    SphSurface* s = sph_observe_state(c->surface);
    if (!s) return sph_fail(c, SPH_E_NOMEM, "sph_surface_set_params: out of host memory");
    s->p = *params;
    s->have_params = true;
    return 0;
}

int32_t sph_surface_frame(SphContext* c) {
    if (!c) return SPH_E_INVALID;
    return surface_frame(c, nullptr);
}

int32_t sph_surface_frame_timed(SphContext* c, float* ms, int32_t n) {
    if (!c) return SPH_E_INVALID;
    if (!ms || n != SPH_SURFACE_PASSES) return sph_fail(c, SPH_E_INVALID, "sph_surface_frame_timed: n must be SPH_SURFACE_PASSES with an array behind it");
    hipEvent_t ev[SPH_SURFACE_PASSES + 1] = {};
    int rc = 0;
    for (int k = 0; k <= SPH_SURFACE_PASSES && rc == 0; ++k)
        if (hipEventCreate(&ev[k]) != hipSuccess) { (void)hipGetLastError(); rc = sph_fail(c, SPH_E_NOMEM, "sph_surface_frame_timed: hipEventCreate failed"); }
    if (rc == 0) rc = surface_frame(c, ev);
    if (rc == 0 && hipEventSynchronize(ev[SPH_SURFACE_PASSES]) != hipSuccess) { (void)hipGetLastError(); rc = sph_fail(c, SPH_E_STATE, "sph_surface_frame_timed: hipEventSynchronize failed"); }
    for (int k = 0; k < SPH_SURFACE_PASSES && rc == 0; ++k)
        if (hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]) != hipSuccess) { (void)hipGetLastError(); rc = sph_fail(c, SPH_E_STATE, "sph_surface_frame_timed: hipEventElapsedTime failed"); }
    for (int k = 0; k <= SPH_SURFACE_PASSES; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    return rc;
}

int32_t sph_surface_download(SphContext* c, uint8_t* rgb, size_t bytes) { return surface_download(c, rgb, bytes, 0); }

int32_t sph_surface_download_depth(SphContext* c, float* depth, size_t bytes) { return surface_download(c, depth, bytes, 1); }

int32_t sph_surface_download_thickness(SphContext* c, float* thickness, size_t bytes) { return surface_download(c, thickness, bytes, 2); }

int32_t sph_frame_download_field_index(SphContext* c, int32_t* index, size_t bytes) {
    if (!c) return SPH_E_INVALID;
    SphSurface* s = c->surface;
    if (!s || !s->have_frame || !s->have_index)
        return sph_fail(c, SPH_E_STATE, "sph_frame_download_field_index: the last surface frame (if any) coloured no fluid by a field");
    if (!index || bytes != (size_t)s->W * s->H * 4)
        return sph_fail(c, SPH_E_INVALID, "sph_frame_download_field_index: size mismatch (i32 [H, W] of the last surface frame)");
    return sph_observe_download(c, index, s->fidx, bytes);
}

}  // extern "C"
