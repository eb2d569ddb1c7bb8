// sph_render.hip -- headless frame export: what the reference's window shows (run_simulation.py:37-98: scene.particles
// with per-vertex colour under one point light, scene.lines for the domain box, window.write_image), rendered on the
// device from the context's own records.  Sphere impostors with a depth buffer; no reference kernel is replaced (the
// reference hands its vis buffers to Taichi's GGUI rasteriser).
//
// Launches per frame (all on the context's stream; particle state is read, never written):
//   k_render_clear    every pixel key = 0xFFFFFFFF'00000000 | background; the large-sprite counter = 0
//   k_frame_splat<LAYER_ALL>  one lane per particle: sprites of pixel radius <= SPH_RENDER_SMALL_R are rasterised by their
//                     lane, larger ones are appended to a compacted index list (in the context's staging buffer, which is
//                     idle between an upload / download and the next); the launch's LAST blocks rasterise the box edges,
//                     one lane per sample
//   k_frame_large<LAYER_ALL>  one WAVE per listed particle, lanes striding over the sprite's bounding box (grid-stride over
//                     the list: the count never visits the host)
//   k_render_resolve  keys -> u8 [H, W, 3] and f32 depth [H, W]
// The two splat kernels are templates over the LAYER of particles they draw (sph_render_dev.h); this file holds their only
// instances, and frame_enqueue_layer launches them for the surface frame's two layers (sph_surface.hip) as well.
// Every loop is bounded: the bounding box is clamped to the image and to SPH_RENDER_MAX_R pixels around the centre (a
// sprite larger than that is cropped to that square), particles inside the near plane or with a non-finite projection
// are culled.
//
// Order independence: a pixel ends as the MINIMUM over all fragments of key = depth bits << 32 | rgb (positive floats
// order as their bit patterns); a fragment's key depends on its particle and its pixel only.  Integer min is
// associative and commutative, so neither particle order nor scheduling can change a bit of the image.  (Two fragments
// of equal depth: the smaller rgb wins -- still a function of the set.)  The early-out read is safe because keys only
// ever decrease.
//
// ---- THE ARITHMETIC (tests/render_model.py follows this block line by line) ----------------------------------------
// Everything below is IEEE binary32, one rounding per written operation, evaluated left to right with the parentheses
// shown; no contraction (pragma below), correctly rounded divide and sqrt (the compiler's default for HIP).
// dot(a, d) := (a.x * d.x + a.y * d.y) + a.z * d.z.
//
// Host, in binary64 (render.py view_basis() is the same sequence), then rounded once to binary32:
//   f  = lookat - eye;  f = f / sqrt((f.x f.x + f.y f.y) + f.z f.z)                          forward
//   r  = (f.y up.z - f.z up.y,  f.z up.x - f.x up.z,  f.x up.y - f.y up.x);  r = r / sqrt((r.x r.x + r.y r.y) + r.z r.z)
//   u  = (r.y f.z - r.z f.y,  r.z f.x - r.x f.z,  r.x f.y - r.y f.x)
//   focal = (height * 0.5) / tan((fov_y_deg * (3.141592653589793 / 180)) * 0.5)
// Host, binary32: cx = width * 0.5, cy = height * 0.5, r2 = radius * radius, dl = light - eye,
//   L = (dot(r, dl), dot(u, dl), dot(f, dl)), fr = focal * radius.
//
// Particle (position x, colour c[3] as integers, visible object, index < particle count):
//   d = x - eye;  a = dot(r, d);  b = dot(u, d);  zc = dot(f, d)
//   cull unless zc >= near
//   px = cx + (focal * a) / zc;  py = cy - (focal * b) / zc;  R = fr / zc;  inv = zc / focal
//   cull unless px, py and R are finite
//   Rb = min(R, SPH_RENDER_MAX_R)
//   columns i in [max(ceil((px - Rb) - 0.5), 0), min(floor((px + Rb) - 0.5), width - 1)], rows j likewise with py, height
//   kc[k] = float(c[k]) / 255
// Fragment (pixel i, j):
//   dx = ((i + 0.5) - px) * inv;  dy = (py - (j + 0.5)) * inv                 view units, y up
//   h2 = (r2 - dx * dx) - dy * dy;  skip unless h2 >= 0;  hh = sqrt(h2)
//   z = zc - hh;  skip unless z > 0
//   n = (dx / radius, dy / radius, hh / radius)
//   l = (L.x - (a + dx), L.y - (b + dy), z - L.z)                            surface point -> light; third axis towards the eye
//   ll = sqrt((l.x l.x + l.y l.y) + l.z l.z);  nl = ll > 0 ? ((n.x l.x + n.y l.y) + n.z l.z) / ll : 0
//   s = ambient + (1 - ambient) * max(nl, 0)
//   q[k] = uint(min(max(kc[k] * s, 0), 1) * 255 + 0.5)                       truncation
//   key = bits(z) << 32 | q[0] << 16 | q[1] << 8 | q[2];  pixel key = min(pixel key, key)
// Box edge e = (A, B) of the twelve, sample m of S = 4 (width + height):
//   t = (m + 0.5) / S;  P = A + (B - A) * t;  d = P - eye;  a, b, zc as above;  skip unless zc >= near
//   px = cx + (focal * a) / zc;  py = cy - (focal * b) / zc;  skip unless 0 <= px < width and 0 <= py < height
//   i = int(px), j = int(py);  key = bits(zc) << 32 | box rgb, box rgb[k] = uint(min(max(box_color[k], 0), 1) * 255 + 0.5)
// Resolve: rgb = low 24 bits of the key; depth = float of the high 32 bits, +inf where they are 0xFFFFFFFF.
//
// Field colouring (sph_frame_set_colour; tests/fieldcolour_model.py follows it): k_frame_splat / k_frame_large<LAYER_ALL_FIELD>
// take the place of the <LAYER_ALL> pair; a frame without a colouring launches what it always did.  A SELECTED particle
// (material and object list of the colouring) with velocity v, position x and the record's density / pressure:
//   s   = the field:  speed = sqrt((v.x v.x + v.y v.y) + v.z v.z);  vx, vy, vz, density, pressure: the stored value;
//         x, y, z: x_a - axis_origin
//   t   = (s - lo) * inv             inv = f32(1) / (f32(hi) - f32(lo)), made by the host and passed by value
//   t   = t >= 0 ? min(t, 1) : 0     a NaN gives 0
//   idx = int(t * 255 + 0.5)         truncation; 0 .. 255
//   kc[k] = float(lut[idx][k]) / 255                                         lut: 256 x 3 i32 in [0, 255]
// and the fragment is the one above.  A particle that is not selected has kc[k] = float(c[k]) / 255 as before.
// k_field_range (sph_field_range) reduces s over the selected, visible particles whose s is finite: min and max of the
// order-preserving u32 image of the bits of s (negative floats flipped whole, the others with the sign bit set), and the two
// counts; wave shuffles, then LDS, then one atomicMin / atomicMax / two atomicAdd per block.  All integers: any order gives the
// same words.  The host maps the two words back to floats.
#include <math.h>

#include "sph_render_dev.h"   // RenderCam, SphRender, the sprite / fragment / box-edge device functions (shared with sph_surface.hip)

#pragma clang fp contract(off)

__global__ __launch_bounds__(RTPB) void k_render_clear(unsigned long long* __restrict__ keys, int n_pix, unsigned background,
                                                       unsigned* __restrict__ big_count) {
    const int i = blockIdx.x * RTPB + threadIdx.x;
    if (i == 0) *big_count = 0u;
    if (i < n_pix) keys[i] = 0xFFFFFFFF00000000ull | background;
}

// does LAYER draw the particle with these flags?
template <int LAYER>
__device__ __forceinline__ bool frame_draws(const RenderCam& cam, int flags) {
    if (layer_base(LAYER) != LAYER_ALL && sph_is_fluid(flags) != (layer_base(LAYER) == LAYER_FLUID)) return false;
    return render_visible(cam, flags);
}

// FIELD... = (the launch's FrameField, the particle's table index) for the *_FIELD layers, nothing for the others
template <int LAYER, class... FIELD>
__device__ __forceinline__ void frame_fragment(const RenderCam& cam, const FramePlanes& g, const Sprite& s, const float kc[3], int i, int j,
                                               const FIELD&... field) {
    if constexpr (LAYER == LAYER_FLUID) surface_fragment(cam, g.keys, g.fz, g.thick, s, i, j);
    else if constexpr (LAYER == LAYER_FLUID_FIELD) surface_field_fragment(cam, g.keys, g.thick, s, i, j, field...);
    else render_fragment(cam, g.keys, s, kc, i, j);
}

// A *_FIELD layer's colour of particle p: its table index if it is selected (else FIELD_IDX_NONE), and, unless the layer is the
// fluid's, kc from the table or from the object's colour.
template <int LAYER>
__device__ __forceinline__ int frame_colour(const FrameField& ff, const float4& x, const float4* __restrict__ aux,
                                            const int* __restrict__ color_cold, int cold_cap, int p, float kc[3]) {
    const float4 V = ff.vf[p], A = aux[p];
    const bool sel = sph_selected(__float_as_int(V.w), ff.sel.who);
    const int idx = sel ? field_index(ff.sel, field_value(ff.sel, x, V, A)) : FIELD_IDX_NONE;
    if (LAYER != LAYER_FLUID_FIELD) {
        if (sel) field_lut_colour(ff.lut, idx, kc);
        else render_colour(color_cold, __float_as_int(A.w), cold_cap, kc);
    }
    return idx;
}

// The two splat kernels: FIELD... = one FrameField for the *_FIELD layers; the other layers have no such argument, and their
// arguments and their code are what they were before there was a colouring.
// blocks [0, particle_blocks): one lane per particle; blocks behind them (none for LAYER_FLUID): one lane per box-edge sample
template <int LAYER, class... FIELD>
__global__ __launch_bounds__(RTPB) void k_frame_splat(RenderCam cam, const float4* __restrict__ xm, const float4* __restrict__ vf,
                                                      const float4* __restrict__ aux, const int* __restrict__ color_cold, int N,
                                                      int cold_cap, int particle_blocks, FramePlanes g, int* __restrict__ big_list,
                                                      unsigned* __restrict__ big_count, int big_cap, FIELD... field) {
    if ((int)blockIdx.x >= particle_blocks) {
        if (layer_base(LAYER) != LAYER_FLUID) render_box_sample(cam, g.keys, ((int)blockIdx.x - particle_blocks) * RTPB + (int)threadIdx.x);
        return;
    }
    const int p = blockIdx.x * RTPB + threadIdx.x;
    if (p >= N) return;
    if (!frame_draws<LAYER>(cam, __float_as_int(vf[p].w))) return;
    const float4 x = xm[p];
    Sprite s;
    if (!render_sprite(cam, x.x, x.y, x.z, s)) return;
    if (s.R > SPH_RENDER_SMALL_R) {
        const unsigned slot = atomicAdd(big_count, 1u);
        if (slot < (unsigned)big_cap) big_list[slot] = p;    // (each particle is listed at most once and big_cap >= N)
        return;
    }
    float kc[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (layer_field(LAYER)) {
        const int idx = frame_colour<LAYER>(field..., x, aux, color_cold, cold_cap, p, kc);
        for (int j = s.j0; j <= s.j1; ++j)
            for (int i = s.i0; i <= s.i1; ++i) frame_fragment<LAYER>(cam, g, s, kc, i, j, field..., idx);
    } else {
        if (LAYER != LAYER_FLUID) render_colour(color_cold, __float_as_int(aux[p].w), cold_cap, kc);
        for (int j = s.j0; j <= s.j1; ++j)           // at most 9 x 9: R <= SPH_RENDER_SMALL_R
            for (int i = s.i0; i <= s.i1; ++i) frame_fragment<LAYER>(cam, g, s, kc, i, j);
    }
}

template <int LAYER, class... FIELD>
__global__ __launch_bounds__(RTPB) void k_frame_large(RenderCam cam, const float4* __restrict__ xm, const float4* __restrict__ aux,
                                                      const int* __restrict__ color_cold, int N, int cold_cap, FramePlanes g,
                                                      const int* __restrict__ big_list, const unsigned* __restrict__ big_count,
                                                      int big_cap, FIELD... field) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * RTPB + threadIdx.x) >> 6, n_waves = (gridDim.x * RTPB) >> 6;
    unsigned n = *big_count;
    if (n > (unsigned)big_cap) n = (unsigned)big_cap;
    for (unsigned w = (unsigned)wave; w < n; w += (unsigned)n_waves) {
        const int p = big_list[w];
        if (p < 0 || p >= N) continue;
        const float4 x = xm[p];
        Sprite s;
        if (!render_sprite(cam, x.x, x.y, x.z, s)) continue;
        float kc[3] = {0.0f, 0.0f, 0.0f};
        const int bw = s.i1 - s.i0 + 1, bh = s.j1 - s.j0 + 1;   // each <= 2 * SPH_RENDER_MAX_R + 1
        if constexpr (layer_field(LAYER)) {
            const int idx = frame_colour<LAYER>(field..., x, aux, color_cold, cold_cap, p, kc);
            for (int t = lane; t < bw * bh; t += 64) {
                const int jj = t / bw;
                frame_fragment<LAYER>(cam, g, s, kc, s.i0 + (t - jj * bw), s.j0 + jj, field..., idx);
            }
        } else {
            if (LAYER != LAYER_FLUID) render_colour(color_cold, __float_as_int(aux[p].w), cold_cap, kc);
            for (int t = lane; t < bw * bh; t += 64) {
                const int jj = t / bw;
                frame_fragment<LAYER>(cam, g, s, kc, s.i0 + (t - jj * bw), s.j0 + jj);
            }
        }
    }
}

__global__ __launch_bounds__(RTPB) void k_render_resolve(const unsigned long long* __restrict__ keys, int n_pix,
                                                         unsigned char* __restrict__ rgb, float* __restrict__ depth) {
    const int i = blockIdx.x * RTPB + threadIdx.x;
    if (i < n_pix) depth[i] = render_resolve_key(keys[i], rgb + 3 * (size_t)i);
}

// ---- sph_field_range ---------------------------------------------------------------------------------------------------
#define FR_MAX_BLOCKS 256      // one block per compute unit: a block walks N / 65536 tiles and ends in four atomics
#define FR_WAVES (RTPB / 64)

// order-preserving image of f32 bits in u32 (the map of sph_columns.hip): negative values flipped whole, the others get the sign bit
__device__ __forceinline__ unsigned field_ordered(float f) {
    const unsigned b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
static float field_unordered(unsigned u) {
    const unsigned b = u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu);
    float f;
    memcpy(&f, &b, 4);
    return f;
}

struct FieldHidden { int n; int ids[SPH_RENDER_MAX_INVISIBLE]; };   // the frames' invisible objects, by value

// words: [0] ordered min, [1] ordered max, then (8-byte aligned) count and non_finite as u64
__global__ __launch_bounds__(64) void k_field_range_clear(unsigned* __restrict__ words) {
    if (threadIdx.x == 0) { words[0] = 0xffffffffu; words[1] = 0u; }
    if (threadIdx.x >= 2 && threadIdx.x < 6) words[threadIdx.x] = 0u;
}

// grid = ceil(tiles / tiles_per_block) blocks of four waves; block b takes the tiles (256 records each) [b, b + 1) * tiles_per_block
__global__ __launch_bounds__(RTPB) void k_field_range(const float4* __restrict__ xm, const float4* __restrict__ vf,
                                                      const float4* __restrict__ aux, int N, int tiles_per_block, FieldSel sel,
                                                      FieldHidden hidden, unsigned* __restrict__ words) {
    __shared__ unsigned w_min[FR_WAVES], w_max[FR_WAVES];
    __shared__ int w_count[FR_WAVES], w_bad[FR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned lo = 0xffffffffu, hi = 0u;
    int count = 0, bad = 0;              // per lane; a lane sees at most tiles_per_block <= 2^23 records
    const long long first = (long long)blockIdx.x * tiles_per_block * RTPB;
    for (int tile = 0; tile < tiles_per_block; ++tile) {
        const long long i = first + (long long)tile * RTPB + threadIdx.x;
        if (i >= N) break;
        const float4 V = vf[i];
        const int flags = __float_as_int(V.w);
        if (!sph_selected(flags, sel.who)) continue;
        const int oid = sph_flags_object(flags);
        bool visible = true;
        for (int k = 0; k < hidden.n; ++k) visible = visible && hidden.ids[k] != oid;
        if (!visible) continue;
        const bool pos = sel.field >= SPH_FIELD_X, rec = sel.field == SPH_FIELD_DENSITY || sel.field == SPH_FIELD_PRESSURE;
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float s = field_value(sel, pos ? xm[i] : zero, V, rec ? aux[i] : zero);   // (only the record the field lives in is read)
        if (isfinite(s)) {
            const unsigned u = field_ordered(s);
            lo = u < lo ? u : lo;
            hi = u > hi ? u : hi;
            ++count;
        } else {
            ++bad;
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned ol = (unsigned)__shfl_xor((int)lo, m, 64), oh = (unsigned)__shfl_xor((int)hi, m, 64);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
        count += __shfl_xor(count, m, 64);
        bad += __shfl_xor(bad, m, 64);
    }
    if (lane == 0) { w_min[wave] = lo; w_max[wave] = hi; w_count[wave] = count; w_bad[wave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long n = 0, nb = 0;
#pragma unroll
        for (int w = 0; w < FR_WAVES; ++w) {
            lo = w_min[w] < lo ? w_min[w] : lo;
            hi = w_max[w] > hi ? w_max[w] : hi;
            n += w_count[w];
            nb += w_bad[w];
        }
        if (n) {
            atomicMin(words + 0, lo);
            atomicMax(words + 1, hi);
            atomicAdd(reinterpret_cast<u64*>(words + 2), (u64)n);
        }
        if (nb) atomicAdd(reinterpret_cast<u64*>(words + 4), (u64)nb);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
// the selection part of a SphFieldColour into sel; a message = what is wrong with it
static const char* make_selection(const SphFieldColour& fc, FieldSel& sel) {
    if (fc.field < 0 || fc.field >= SPH_FIELD_COUNT_) return "unknown field (enum SphColourField)";
    switch (sph_sel_make(fc.material, fc.n_objects, fc.object_ids, true, &sel.who)) {
        case SPH_SEL_BAD_MATERIAL: return "material must be -1 or in [0, 255]";
        case SPH_SEL_BAD_COUNT: return "n_objects must be in [0, SPH_FIELD_MAX_OBJECTS = 32]";
    }
    if (!isfinite(fc.axis_origin)) return "axis_origin must be finite";
    sel.field = fc.field;
    sel.origin = fc.axis_origin;
    sel.lo = 0.0f; sel.inv = 1.0f;
    return nullptr;
}

static bool field_needs_aux(const FieldSel& sel) { return sel.field == SPH_FIELD_DENSITY || sel.field == SPH_FIELD_PRESSURE; }

static unsigned pack_unit_rgb(const float c[3]) {
    unsigned rgb = 0;
    for (int k = 0; k < 3; ++k) {
        const float t = fminf(fmaxf(c[k], 0.0f), 1.0f);
        rgb = (rgb << 8) | (unsigned)(t * 255.0f + 0.5f);
    }
    return rgb;
}

static float hdot(const float a[3], const float d[3]) { return (a[0] * d[0] + a[1] * d[1]) + a[2] * d[2]; }

// the comment block's host part; a message = what is wrong with the parameters
static const char* make_camera(const SphRenderParams& p, RenderCam& cam) {
    if (p.width < 1 || p.height < 1 || p.width > SPH_RENDER_MAX_DIM || p.height > SPH_RENDER_MAX_DIM)
        return "sph_render_set_params: width and height must be in [1, 16384]";
    const float* all[] = {p.eye, p.lookat, p.up, p.light, p.box_end, p.box_color};
    for (const float* v : all)
        for (int k = 0; k < 3; ++k)
            if (!isfinite(v[k])) return "sph_render_set_params: non-finite vector component";
    if (!(p.fov_y_deg > 0.0f && p.fov_y_deg < 180.0f)) return "sph_render_set_params: fov_y_deg must be in (0, 180)";
    if (!(p.radius > 0.0f) || !isfinite(p.radius)) return "sph_render_set_params: radius must be positive";
    if (!(p.near_plane > 0.0f) || !isfinite(p.near_plane)) return "sph_render_set_params: near_plane must be positive";
    if (!(p.ambient >= 0.0f && p.ambient <= 1.0f)) return "sph_render_set_params: ambient must be in [0, 1]";
    double f[3], r[3], u[3], up[3];
    for (int k = 0; k < 3; ++k) { f[k] = (double)p.lookat[k] - (double)p.eye[k]; up[k] = (double)p.up[k]; }
    const double fl = sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
    if (!(fl > 0.0)) return "sph_render_set_params: eye == lookat";
    for (int k = 0; k < 3; ++k) f[k] = f[k] / fl;
    r[0] = f[1] * up[2] - f[2] * up[1];
    r[1] = f[2] * up[0] - f[0] * up[2];
    r[2] = f[0] * up[1] - f[1] * up[0];
    const double rl = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    const double ul = sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]);
    if (!(ul > 0.0) || !(rl > 1e-6 * ul)) return "sph_render_set_params: up is zero or parallel to the view direction";
    for (int k = 0; k < 3; ++k) r[k] = r[k] / rl;
    u[0] = r[1] * f[2] - r[2] * f[1];
    u[1] = r[2] * f[0] - r[0] * f[2];
    u[2] = r[0] * f[1] - r[1] * f[0];
    const double focal = ((double)p.height * 0.5) / tan(((double)p.fov_y_deg * (3.141592653589793 / 180.0)) * 0.5);
    memset(&cam, 0, sizeof(cam));
    cam.W = p.width; cam.H = p.height; cam.S = 4 * (p.width + p.height);
    cam.ex = p.eye[0]; cam.ey = p.eye[1]; cam.ez = p.eye[2];
    const float rf[3] = {(float)r[0], (float)r[1], (float)r[2]}, uf[3] = {(float)u[0], (float)u[1], (float)u[2]},
                ff[3] = {(float)f[0], (float)f[1], (float)f[2]};
    cam.rx = rf[0]; cam.ry = rf[1]; cam.rz = rf[2];
    cam.ux = uf[0]; cam.uy = uf[1]; cam.uz = uf[2];
    cam.fx = ff[0]; cam.fy = ff[1]; cam.fz = ff[2];
    cam.focal = (float)focal;
    if (!(cam.focal > 0.0f) || !isfinite(cam.focal)) return "sph_render_set_params: fov_y_deg gives no usable focal length";
    cam.cx = (float)p.width * 0.5f; cam.cy = (float)p.height * 0.5f;
    cam.radius = p.radius; cam.r2 = p.radius * p.radius; cam.fr = cam.focal * p.radius; cam.near_plane = p.near_plane;
    const float dl[3] = {p.light[0] - p.eye[0], p.light[1] - p.eye[1], p.light[2] - p.eye[2]};
    cam.Lx = hdot(rf, dl); cam.Ly = hdot(uf, dl); cam.Lz = hdot(ff, dl);
    cam.ambient = p.ambient;
    cam.bex = p.box_end[0]; cam.bey = p.box_end[1]; cam.bez = p.box_end[2];
    cam.box_rgb = pack_unit_rgb(p.box_color);
    cam.background = ((unsigned)p.background[0] << 16) | ((unsigned)p.background[1] << 8) | (unsigned)p.background[2];
    cam.draw_box = p.draw_box ? 1 : 0;
    return nullptr;
}

void sph_render_release(SphContext* c) { sph_observe_release(c->render, &SphRender::block, &SphRender::lut, &SphRender::range_words); }

static int render_alloc(SphContext* c, SphRender* r) {
    const int W = r->cam.W, H = r->cam.H;
    if (r->block && r->W == W && r->H == H) return 0;
    r->W = r->H = 0; r->have_frame = false;
    const size_t n = (size_t)W * H, rgb_bytes = (3 * n + 15) & ~(size_t)15;
    if (int rc = sph_observe_alloc(c, &r->block, 12 * n + rgb_bytes + 16, "sph_render_frame", "the frame buffers")) return rc;
    char* b = (char*)r->block;
    r->keys = (unsigned long long*)b; b += 8 * n;
    r->depth = (float*)b; b += 4 * n;
    r->rgb = (unsigned char*)b; b += rgb_bytes;
    r->big_count = (unsigned*)b;
    r->W = W; r->H = H;
    return 0;
}

template <int LAYER>
int frame_enqueue_layer(SphContext* c, const RenderCam& cam, const FramePlanes& planes, unsigned* big_count, const FrameField& field) {
    if (int rc = sph_ensure_pid(c)) return rc;   // the kernels below read aux
    const SphLive in = sph_live(c);
    int* big_list = reinterpret_cast<int*>(c->stage);          // stage_bytes >= 16 * capacity; the previous layer's large launch is ahead on the stream
    const int big_cap = (int)(c->stage_bytes / 4 < (size_t)0x7fffffff ? c->stage_bytes / 4 : (size_t)0x7fffffff);
    const int particle_blocks = (in.N + RTPB - 1) / RTPB;
    const int box_blocks = layer_base(LAYER) != LAYER_FLUID && cam.draw_box ? (12 * cam.S + RTPB - 1) / RTPB : 0;
    FrameField ff = field;                    // (read by the *_FIELD layers only)
    ff.vf = in.vf;
    if (particle_blocks + box_blocks > 0) {
        if constexpr (layer_field(LAYER))
            hipLaunchKernelGGL((k_frame_splat<LAYER, FrameField>), dim3(particle_blocks + box_blocks), dim3(RTPB), 0, c->stream, cam, in.xm, in.vf,
                               in.aux, c->color_cold, in.N, c->cold_cap, particle_blocks, planes, big_list, big_count, big_cap, ff);
        else
            hipLaunchKernelGGL(k_frame_splat<LAYER>, dim3(particle_blocks + box_blocks), dim3(RTPB), 0, c->stream, cam, in.xm, in.vf, in.aux,
                               c->color_cold, in.N, c->cold_cap, particle_blocks, planes, big_list, big_count, big_cap);
        SPH_LAUNCH_CHECK(c);
    }
    if (in.N > 0) {
        int blocks = (in.N + 3) / 4;          // one wave per listed particle, at most 4096 waves striding over the list
        if (blocks > 1024) blocks = 1024;
        if constexpr (layer_field(LAYER))
            hipLaunchKernelGGL((k_frame_large<LAYER, FrameField>), dim3(blocks), dim3(RTPB), 0, c->stream, cam, in.xm, in.aux, c->color_cold, in.N,
                               c->cold_cap, planes, big_list, big_count, big_cap, ff);
        else
            hipLaunchKernelGGL(k_frame_large<LAYER>, dim3(blocks), dim3(RTPB), 0, c->stream, cam, in.xm, in.aux, c->color_cold, in.N, c->cold_cap,
                               planes, big_list, big_count, big_cap);
        SPH_LAUNCH_CHECK(c);
    }
    return 0;
}
template int frame_enqueue_layer<LAYER_ALL>(SphContext*, const RenderCam&, const FramePlanes&, unsigned*, const FrameField&);
template int frame_enqueue_layer<LAYER_OPAQUE>(SphContext*, const RenderCam&, const FramePlanes&, unsigned*, const FrameField&);
template int frame_enqueue_layer<LAYER_FLUID>(SphContext*, const RenderCam&, const FramePlanes&, unsigned*, const FrameField&);
template int frame_enqueue_layer<LAYER_ALL_FIELD>(SphContext*, const RenderCam&, const FramePlanes&, unsigned*, const FrameField&);
template int frame_enqueue_layer<LAYER_OPAQUE_FIELD>(SphContext*, const RenderCam&, const FramePlanes&, unsigned*, const FrameField&);
template int frame_enqueue_layer<LAYER_FLUID_FIELD>(SphContext*, const RenderCam&, const FramePlanes&, unsigned*, const FrameField&);

// What a frame of either style does before its splats when a colouring is in force: density / pressure of a fused step live in
// eos2 until somebody asks (as the export does).
int frame_colour_prepare(SphContext* c, const SphRender* r) {
    if (r->colour_on && field_needs_aux(r->sel)) return sph_ensure_aux(c);
    return 0;
}

extern "C" {

int32_t sph_render_set_params(SphContext* c, const SphRenderParams* params) {
    if (c && !params) return sph_fail(c, SPH_E_INVALID, "sph_render_set_params: null argument");
    if (int rc = sph_observe_enter(c, "sph_render_set_params", FRAME_SLAB_WHY)) return rc;
    RenderCam cam;
    if (const char* what = make_camera(*params, cam)) return sph_fail(c, SPH_E_INVALID, what);
    SphRender* r = sph_observe_state(c->render);
    if (!r) return sph_fail(c, SPH_E_NOMEM, "sph_render_set_params: out of host memory");
    cam.n_invisible = r->cam.n_invisible;
    memcpy(cam.invisible, r->cam.invisible, sizeof(cam.invisible));
    r->p = *params;
    r->cam = cam;
    return 0;
}

int32_t sph_render_set_invisible(SphContext* c, const int32_t* object_ids, int32_t n) {
    if (!c) return SPH_E_INVALID;
    if (n < 0 || n > SPH_RENDER_MAX_INVISIBLE || (n > 0 && !object_ids))
        return sph_fail(c, SPH_E_INVALID, "sph_render_set_invisible: n must be in [0, 32] with a list behind it");
    if (int rc = sph_observe_enter(c, "sph_render_set_invisible", FRAME_SLAB_WHY)) return rc;
    SphRender* r = sph_observe_state(c->render);
    if (!r) return sph_fail(c, SPH_E_NOMEM, "sph_render_set_invisible: out of host memory");
    r->cam.n_invisible = n;
    for (int k = 0; k < n; ++k) r->cam.invisible[k] = object_ids[k];
    return 0;
}

int32_t sph_frame_set_colour(SphContext* c, const SphFieldColour* colour, const int32_t* lut) {
    if (c && (colour == nullptr) != (lut == nullptr)) return sph_fail(c, SPH_E_INVALID, "sph_frame_set_colour: colour and lut are both null (off) or both given");
    if (int rc = sph_observe_enter(c, "sph_frame_set_colour", FRAME_SLAB_WHY)) return rc;
    if (!colour) {
        if (c->render) c->render->colour_on = false;
        return 0;
    }
    FieldSel sel;
    if (const char* what = make_selection(*colour, sel)) {
        snprintf(c->err, sizeof(c->err), "sph_frame_set_colour: %s", what);
        return SPH_E_INVALID;
    }
    if (!isfinite(colour->lo) || !isfinite(colour->hi)) return sph_fail(c, SPH_E_INVALID, "sph_frame_set_colour: lo and hi must be finite");
    if (!(colour->lo < colour->hi)) return sph_fail(c, SPH_E_INVALID, "sph_frame_set_colour: lo must be smaller than hi");
    sel.lo = colour->lo;
    sel.inv = 1.0f / (colour->hi - colour->lo);
    if (!(sel.inv > 0.0f) || !isfinite(sel.inv)) return sph_fail(c, SPH_E_INVALID, "sph_frame_set_colour: the range is too narrow or too wide for binary32");
    for (int k = 0; k < 256 * 3; ++k)
        if (lut[k] < 0 || lut[k] > 255) return sph_fail(c, SPH_E_INVALID, "sph_frame_set_colour: a table entry lies outside [0, 255]");
    SphRender* r = sph_observe_state(c->render);
    if (!r) return sph_fail(c, SPH_E_NOMEM, "sph_frame_set_colour: out of host memory");
    const bool first = !r->lut;
    if (first)
        if (int rc = sph_observe_alloc(c, (void**)&r->lut, sizeof(r->lut_host), "sph_frame_set_colour", "the colour table")) return rc;
    if (first || memcmp(r->lut_host, lut, sizeof(r->lut_host)) != 0) {
        // behind the frames that still read the old table; the host copy must not change before the copy has been made
        memcpy(r->lut_host, lut, sizeof(r->lut_host));
        SPH_HIP(c, hipMemcpyAsync(r->lut, r->lut_host, sizeof(r->lut_host), hipMemcpyHostToDevice, c->stream));
        SPH_HIP(c, hipStreamSynchronize(c->stream));
    }
    r->sel = sel;
    r->colour_on = true;
    return 0;
}

int32_t sph_field_range(SphContext* c, const SphFieldColour* colour, SphFieldRange* out) {
    if (c && (!colour || !out)) return sph_fail(c, SPH_E_INVALID, "sph_field_range: null argument");
    if (int rc = sph_observe_enter(c, "sph_field_range", FRAME_SLAB_WHY)) return rc;
    FieldSel sel;
    if (const char* what = make_selection(*colour, sel)) {
        snprintf(c->err, sizeof(c->err), "sph_field_range: %s", what);
        return SPH_E_INVALID;
    }
    SphRender* r = sph_observe_state(c->render);
    if (!r) return sph_fail(c, SPH_E_NOMEM, "sph_field_range: out of host memory");
    if (!r->range_words)
        if (int rc = sph_observe_alloc(c, (void**)&r->range_words, 32, "sph_field_range", "the result words")) return rc;
    if (field_needs_aux(sel))
        if (int rc = sph_ensure_aux(c)) return rc;
    FieldHidden hidden;
    hidden.n = r->cam.n_invisible;
    memcpy(hidden.ids, r->cam.invisible, sizeof(hidden.ids));
    if (int rc = sph_ensure_pid(c)) return rc;   // the kernels below read aux
    const SphLive in = sph_live(c);
    hipLaunchKernelGGL(k_field_range_clear, dim3(1), dim3(64), 0, c->stream, r->range_words);
    SPH_LAUNCH_CHECK(c);
    if (in.N > 0) {
        const SphWalk w = sph_observe_walk(in.N, RTPB, FR_MAX_BLOCKS);
        hipLaunchKernelGGL(k_field_range, dim3(w.blocks), dim3(RTPB), 0, c->stream, in.xm, in.vf, in.aux, in.N, w.per_block, sel, hidden, r->range_words);
        SPH_LAUNCH_CHECK(c);
    }
    unsigned words[6];
    if (int rc = sph_observe_download(c, words, r->range_words, sizeof(words))) return rc;
    memcpy(&out->count, words + 2, 8);
    memcpy(&out->non_finite, words + 4, 8);
    out->lo = out->count > 0 ? field_unordered(words[0]) : (float)INFINITY;
    out->hi = out->count > 0 ? field_unordered(words[1]) : -(float)INFINITY;
    return 0;
}

int32_t sph_render_frame(SphContext* c) {
    if (int rc = sph_observe_enter(c, "sph_render_frame", FRAME_SLAB_WHY)) return rc;
    SphRender* r = c->render;
    if (!r || r->cam.W <= 0) return sph_fail(c, SPH_E_STATE, "sph_render_frame needs sph_render_set_params first");
    if (int rc = render_alloc(c, r)) return rc;
    if (int rc = frame_colour_prepare(c, r)) return rc;
    const RenderCam& cam = r->cam;
    const int n_pix = cam.W * cam.H;     // <= 2^28
    hipLaunchKernelGGL(k_render_clear, dim3((n_pix + RTPB - 1) / RTPB), dim3(RTPB), 0, c->stream, r->keys, n_pix, cam.background, r->big_count);
    SPH_LAUNCH_CHECK(c);
    if (r->colour_on) {
        if (int rc = frame_enqueue_layer<LAYER_ALL_FIELD>(c, cam, FramePlanes{r->keys, nullptr, nullptr}, r->big_count, FrameField{r->sel, r->lut, nullptr})) return rc;
    } else {
        if (int rc = frame_enqueue_layer<LAYER_ALL>(c, cam, FramePlanes{r->keys, nullptr, nullptr}, r->big_count)) return rc;
    }
    hipLaunchKernelGGL(k_render_resolve, dim3((n_pix + RTPB - 1) / RTPB), dim3(RTPB), 0, c->stream, r->keys, n_pix, r->rgb, r->depth);
    SPH_LAUNCH_CHECK(c);
    r->have_frame = true;
    return 0;
}

static int render_download(SphContext* c, void* host, size_t bytes, bool depth) {
    if (!c) return SPH_E_INVALID;
    SphRender* r = c->render;
    if (!r || !r->have_frame) return sph_fail(c, SPH_E_STATE, "sph_render_download: no frame has been rendered");
    const size_t want = (size_t)r->W * r->H * (depth ? 4 : 3);
    if (!host || bytes != want) return sph_fail(c, SPH_E_INVALID, "sph_render_download: size mismatch (u8 [H, W, 3] / f32 [H, W] of the last frame)");
    return sph_observe_download(c, host, depth ? (const void*)r->depth : (const void*)r->rgb, bytes);
}

int32_t sph_render_download(SphContext* c, uint8_t* rgb, size_t bytes) { return render_download(c, rgb, bytes, false); }

int32_t sph_render_download_depth(SphContext* c, float* depth, size_t bytes) { return render_download(c, depth, bytes, true); }

}  // extern "C"
