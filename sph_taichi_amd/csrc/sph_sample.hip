// sph_sample.hip -- field sampling by scatter (include/sph_hip.h, "Field sampling"): SPH interpolation of velocity, density and pressure
// at the nodes of a regular grid (a volume, or a slice when one n_a is 1) and at up to SPH_SAMPLE_MAX_POINTS probe points.  The sample
// positions do not look for particles: one streaming pass over the live records in which every selected particle adds its
// kernel-weighted share to the positions inside its support radius.  Reads xm / vf (32 B per particle), aux as well when density or
// pressure is asked for (+ 16 B); writes its own planes.  Never reads the cell array, touches nothing of the sort or the sweeps and
// writes no particle state.
//
// Pair term of sample position p and selected particle j (f32, in this order, nothing contracted; sample_pair() of sph_sample_pair.h,
// shared by the grid and the points kernels and by the tracer gather so that they cannot disagree):
//     dx = p.x - x_j.x (dy, dz alike);  r2 = (dx*dx + dy*dy) + dz*dz;  r = correctly rounded sqrtf(r2);  q = r * inv_h
//     the pair contributes  <=>  q <= 1.0f                                  (a NaN does not contribute)
//     W = q <= 0.5f ? k_w * ((6.f*q3 - 6.f*q2) + 1.f)  with q2 = q*q, q3 = q2*q  :  (k_w * 2.f) * ((t*t)*t)  with t = 1.f - q
//     w = fminf(fmaxf(m_V_j * W, 0.f), 4.f)
// A grid node is p_a = origin_a + (float)k_a * spacing_a (one multiply, one add).  Per contributing pair the position receives
//     count += 1;  weight += llrint((double)w * 2^30);  sum[f] += llrint(((double)w * (double)fmaxf(fminf(A_f, 2^24), -2^24)) * 2^30)
// Determinism: every accumulation is an INTEGER sum (i64, on chip as well as in HBM), so the result is the same bits for any particle
// order, grouping and scheduling.  There is no float or double atomic anywhere.
//
// The FOOTPRINT of a particle is a node box that surely holds every node with q <= 1: floorf((x -+ h - origin) * inv_spacing), widened
// by one node and by the rounding slack of that arithmetic, clamped AS A FLOAT before the cast (a far-away position cannot overflow
// the int; a NaN gives the empty box).  It only has to be a superset: sample_pair() alone decides what contributes.
//
// Grid kernel (k_sample_grid): a block of four waves works through a CONTIGUOUS range of records.
//   wave   : the wave takes its 64 records in turn; the nodes of ONE particle's footprint are spread over the 64 lanes, so the
//            atomics of a wave-instruction go to distinct addresses (particles one spacing apart share most of their nodes: lanes
//            that held neighbouring particles would collide on almost every add);
//   grid   : every contributing (node, channel) is one 64-bit global atomic add.  Records are in cell order, so the blocks in flight
//            work on compact regions of the planes.  (A second stage that combined a block's adds in an
//            LDS tile first did not win: DESIGN_HISTORY.md, "Field sampling: the LDS-tiled grid kernel".)
// Nothing depends on the order of the records: unsorted ones only spread the adds.
// Points kernel (k_sample_points): the points of a chunk and one i64 partial per (channel, point) live in LDS; every selected particle
// tests every point of the chunk; the block's non-empty partials are added to the planes.
//
// GRADIENTS (include/sph_hip.h, "Field sampling: gradients"): the gradient of the Shepard interpolant is a ratio of sums of the same
// kind, so both kernels have a second instance (template parameter GRAD) that adds, per contributing pair, g_b = u * e_b to the planes
// Gx Gy Gz and g_b * A_f to three planes per field whose gradient is asked for; sample_gradient() below is THE gradient term, fed with
// the dx, dy, dz, r, q of sample_pair().  The planes of one result are count, weight, the fields, Gx Gy Gz, then x y z per gradient
// bit in mask order: up to 2 + 5 + 3 + 15 = 25 channels.  The plain instances are the kernels as they were: a call without gradients
// runs the same code.  The points kernel sizes its chunk from the channel count so that the block stays within the 34,816 B of LDS
// the plain instance uses at most: 164 points at 25 channels.
#include <cmath>
#include "sph_observe.h"
#include "sph_sample_grid.h"
#include "sph_sample_pair.h"

#pragma clang fp contract(off)

#define STPB 256
#define SG_MAX_BLOCKS 1024
#define SG_MAX_CHANNELS (2 + 5)   // count, weight, vx vy vz density pressure
#define SG_MAX_GRAD_CHANNELS (3 + 3 * 5)   // Gx Gy Gz, then x y z per gradient bit
#define SP_CHUNK 512              // points per LDS chunk: 512 * (12 + 7 * 8) B = 34,816 B
#define SP_LDS_BYTES (SP_CHUNK * (12 + SG_MAX_CHANNELS * 8))   // the budget the gradient instance sizes its chunk from
#define SP_MAX_BLOCKS 1024
#define S_ALL_FIELDS (SPH_SAMPLE_VX | SPH_SAMPLE_VY | SPH_SAMPLE_VZ | SPH_SAMPLE_DENSITY | SPH_SAMPLE_PRESSURE)

struct SphSample {
    long long* grid;          // [2 + F][nodes]: count, weight, then the requested fields in mask order
    size_t grid_words;        // allocated
    long long grid_nodes;     // of the last sph_sample_grid
    int grid_n[3];            // its geometry: what the mesh extraction (sph_mesh.hip) reads the weight plane with
    float grid_origin[3], grid_spacing[3];
    int grid_fields;          // number of field planes of the last sph_sample_grid
    int grid_grads;           // number of gradient planes behind them: 0 (a plain sample) or 3 + 3 Fg
    bool grid_have;
    void* pts_buf;            // one allocation: xyz [SPH_SAMPLE_MAX_POINTS][3] f32, then the planes [SG_MAX_CHANNELS + SG_MAX_GRAD_CHANNELS][SPH_SAMPLE_MAX_POINTS]
    long long* pts;
    int pts_m, pts_fields, pts_grads;
    bool pts_have;
    bool pts_copying;         // pts_host may still be read by the copy of the last sph_sample_points
    float pts_host[3 * SPH_SAMPLE_MAX_POINTS];
};

// (SampleCommon and SampleGridDev, the kernels' arguments: sph_sample_grid.h)

struct NodeBox { int lo[3], hi[3]; };   // inclusive; empty when lo > hi on any axis

// THE gradient term of a contributing pair: g_b = u * e_b, dimensionless (h grad w); zero on every axis when r == 0
__device__ __forceinline__ void sample_gradient(const SamplePairGeom& p, float m_V, float k_w, float g[3]) {
    const float q = p.q;
    float D;
    if (q <= 0.5f) {
        D = (k_w * 6.f) * (q * (3.f * q - 2.f));
    } else {
        const float t = 1.f - q;
        D = (k_w * 6.f) * (-(t * t));
    }
    const float u = fmaxf(fminf(m_V * D, 0.f), -8.f);
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const float e = p.r > 0.f ? p.d[b] / p.r : 0.f;   // the IEEE-correct division (hipcc's default, as for sqrtf)
        g[b] = u * e;
    }
}

__device__ __forceinline__ float bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ int bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// the node range [lo, hi] along one axis that surely holds every node within h of x (empty for a NaN): see the header comment
__device__ __forceinline__ void sample_axis_range(float x, float h, float origin, float inv_spacing, int n, int& lo, int& hi) {
    const float slack = ((fabsf(x) + fabsf(origin)) + h) * 0x1p-21f * inv_spacing;   // the roundings of x -+ h - origin and of the node positions, in nodes
    const float vlo = ((x - h) - origin) * inv_spacing, vhi = ((x + h) - origin) * inv_spacing;
    float flo = floorf(vlo - (fabsf(vlo) * 0x1p-20f + slack)) - 1.f;
    float fhi = floorf(vhi + (fabsf(vhi) * 0x1p-20f + slack)) + 1.f;
    if (!(flo <= fhi)) { lo = 0; hi = -1; return; }                 // a NaN anywhere
    flo = fminf(fmaxf(flo, 0.f), (float)n);                          // n <= 2^24: exact as a float
    fhi = fmaxf(fminf(fhi, (float)(n - 1)), -1.f);
    lo = (int)flo; hi = (int)fhi;
}

__device__ __forceinline__ NodeBox sample_footprint(const SampleGridDev& g, const float4& X) {
    NodeBox b;
    sample_axis_range(X.x, g.h, g.origin[0], g.inv_spacing[0], g.n[0], b.lo[0], b.hi[0]);
    sample_axis_range(X.y, g.h, g.origin[1], g.inv_spacing[1], g.n[1], b.lo[1], b.hi[1]);
    sample_axis_range(X.z, g.h, g.origin[2], g.inv_spacing[2], g.n[2], b.lo[2], b.hi[2]);
    return b;
}

__device__ __forceinline__ bool box_empty(const NodeBox& b) { return b.lo[0] > b.hi[0] || b.lo[1] > b.hi[1] || b.lo[2] > b.hi[2]; }

__global__ __launch_bounds__(STPB) void k_sample_clear(u64* __restrict__ p, size_t words) {
    for (size_t k = (size_t)blockIdx.x * STPB + threadIdx.x; k < words; k += (size_t)gridDim.x * STPB) p[k] = 0ull;
}

// grid = ceil(tiles / tiles_per_block) blocks of four waves; block b takes the tiles (256 records each) [b, b + 1) * tiles_per_block.
// All 64 lanes of a wave make every trip of the record loop (the ballot needs them).
// GRAD: the gradient-carrying instance; `gradients` is its mask of field bits (a subset of q.fields) and is not read otherwise.
template <bool GRAD>
__device__ __forceinline__ void sample_grid_body(const float4* __restrict__ xm, const float4* __restrict__ vf, const float4* __restrict__ aux,
                                                 int N, int tiles_per_block, const SampleCommon& q, const SampleGridDev& g, int gradients) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool need_aux = (q.fields & (SPH_SAMPLE_DENSITY | SPH_SAMPLE_PRESSURE)) != 0;
    const long long first = (long long)blockIdx.x * tiles_per_block * STPB;
    long long last = first + (long long)tiles_per_block * STPB;
    if (last > N) last = N;
    for (long long base = first + wave * 64; base < last; base += STPB) {
        const long long i = base + lane;
        bool act = false;
        float4 X = make_float4(0.f, 0.f, 0.f, 0.f);
        float A[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        NodeBox b;
#pragma unroll
        for (int a = 0; a < 3; ++a) { b.lo[a] = 0; b.hi[a] = -1; }
        if (i < last) {
            X = xm[i];
            const float4 V = vf[i];
            if (sph_selected(__float_as_int(V.w), q.sel)) {
                b = sample_footprint(g, X);
                act = !box_empty(b);
                if (act) {
                    A[0] = sample_clamp_field(V.x); A[1] = sample_clamp_field(V.y); A[2] = sample_clamp_field(V.z);
                    if (need_aux) {
                        const float4 Q = aux[i];
                        A[3] = sample_clamp_field(Q.y); A[4] = sample_clamp_field(Q.z);
                    }
                }
            }
        }
        u64 todo = __ballot(act);
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;   // wave-uniform
            todo &= todo - 1ull;
            const float4 Xj = make_float4(bcast(X.x, j), bcast(X.y, j), bcast(X.z, j), bcast(X.w, j));
            float Aj[5];
#pragma unroll
            for (int f = 0; f < 5; ++f) Aj[f] = bcast(A[f], j);
            const int l0 = bcast(b.lo[0], j), l1 = bcast(b.lo[1], j), l2 = bcast(b.lo[2], j);
            const int d0 = bcast(b.hi[0], j) - l0 + 1, d1 = bcast(b.hi[1], j) - l1 + 1, d2 = bcast(b.hi[2], j) - l2 + 1;
            const int total = d0 * d1 * d2;   // <= nodes <= 2^24
            for (int e = lane; e < total; e += 64) {
                const int i2 = e % d2, rest = e / d2, i1 = rest % d1, i0 = rest / d1;
                const int k0 = l0 + i0, k1 = l1 + i1, k2 = l2 + i2;   // inside the grid: the footprint was clamped to it
                const float px = g.origin[0] + (float)k0 * g.spacing[0];
                const float py = g.origin[1] + (float)k1 * g.spacing[1];
                const float pz = g.origin[2] + (float)k2 * g.spacing[2];
                float w;
                SamplePairGeom geom;
                if (!sample_pair(px, py, pz, Xj, q.inv_h, q.k_w, w, geom)) continue;
                u64* dst = (u64*)g.planes + (((size_t)k0 * g.n[1] + k1) * g.n[2] + k2);
                const size_t stride = (size_t)g.nodes;
                atomicAdd(dst, 1ull);
                atomicAdd(dst + stride, (u64)sample_weight_term(w));
                int c = 2;
#pragma unroll
                for (int f = 0; f < 5; ++f)
                    if (q.fields & (1 << f)) { atomicAdd(dst + (size_t)c * stride, (u64)sample_term(w, Aj[f])); ++c; }
                if (GRAD) {
                    float gr[3];
                    sample_gradient(geom, Xj.w, q.k_w, gr);
#pragma unroll
                    for (int b = 0; b < 3; ++b) { atomicAdd(dst + (size_t)c * stride, (u64)sample_weight_term(gr[b])); ++c; }
#pragma unroll
                    for (int f = 0; f < 5; ++f)
                        if (gradients & (1 << f)) {
#pragma unroll
                            for (int b = 0; b < 3; ++b) { atomicAdd(dst + (size_t)c * stride, (u64)sample_term(gr[b], Aj[f])); ++c; }
                        }
                }
            }
        }
    }
}

__global__ __launch_bounds__(STPB) void k_sample_grid(const float4* __restrict__ xm, const float4* __restrict__ vf, const float4* __restrict__ aux,
                                                      int N, int tiles_per_block, SampleCommon q, SampleGridDev g) {
    sample_grid_body<false>(xm, vf, aux, N, tiles_per_block, q, g, 0);
}

__global__ __launch_bounds__(STPB) void k_sample_grid_grad(const float4* __restrict__ xm, const float4* __restrict__ vf, const float4* __restrict__ aux,
                                                           int N, int tiles_per_block, SampleCommon q, SampleGridDev g, int gradients) {
    sample_grid_body<true>(xm, vf, aux, N, tiles_per_block, q, g, gradients);
}

// dynamic LDS: the partials [channels][chunk] i64, then xyz [3][chunk] f32; chunk = min(m, SP_CHUNK) rounded up to even in the plain
// instance, and in the gradient instance no more than fits SP_LDS_BYTES with q.channels channels (sample_points_chunk)
template <bool GRAD>
__device__ __forceinline__ void sample_points_body(unsigned char* sample_lds, const float4* __restrict__ xm, const float4* __restrict__ vf,
                                                   const float4* __restrict__ aux, int N, int tiles_per_block, const SampleCommon& q,
                                                   const float* __restrict__ xyz, int m, int chunk, long long* __restrict__ planes, int gradients) {
    u64* part = reinterpret_cast<u64*>(sample_lds);                       // [channels][chunk]
    float* P = reinterpret_cast<float*>(part + (size_t)q.channels * chunk);   // [3][chunk]
    const bool need_aux = (q.fields & (SPH_SAMPLE_DENSITY | SPH_SAMPLE_PRESSURE)) != 0;
    const long long first = (long long)blockIdx.x * tiles_per_block * STPB;
    long long last = first + (long long)tiles_per_block * STPB;
    if (last > N) last = N;
    for (int c0 = 0; c0 < m; c0 += chunk) {
        const int cnt = m - c0 < chunk ? m - c0 : chunk;
        for (int e = threadIdx.x; e < cnt; e += STPB) {
            P[e] = xyz[3 * (size_t)(c0 + e)]; P[chunk + e] = xyz[3 * (size_t)(c0 + e) + 1]; P[2 * chunk + e] = xyz[3 * (size_t)(c0 + e) + 2];
        }
        for (int e = threadIdx.x; e < q.channels * chunk; e += STPB) part[e] = 0ull;
        __syncthreads();
        for (long long i = first + threadIdx.x; i < last; i += STPB) {
            const float4 V = vf[i];
            if (!sph_selected(__float_as_int(V.w), q.sel)) continue;
            const float4 X = xm[i];
            float A[5] = {sample_clamp_field(V.x), sample_clamp_field(V.y), sample_clamp_field(V.z), 0.f, 0.f};
            if (need_aux) {
                const float4 Q = aux[i];
                A[3] = sample_clamp_field(Q.y); A[4] = sample_clamp_field(Q.z);
            }
            for (int e = 0; e < cnt; ++e) {
                float w;
                SamplePairGeom geom;
                if (!sample_pair(P[e], P[chunk + e], P[2 * chunk + e], X, q.inv_h, q.k_w, w, geom)) continue;
                atomicAdd(part + e, 1ull);
                atomicAdd(part + chunk + e, (u64)sample_weight_term(w));
                int c = 2;
#pragma unroll
                for (int f = 0; f < 5; ++f)
                    if (q.fields & (1 << f)) { atomicAdd(part + (size_t)c * chunk + e, (u64)sample_term(w, A[f])); ++c; }
                if (GRAD) {
                    float gr[3];
                    sample_gradient(geom, X.w, q.k_w, gr);
#pragma unroll
                    for (int b = 0; b < 3; ++b) { atomicAdd(part + (size_t)c * chunk + e, (u64)sample_weight_term(gr[b])); ++c; }
#pragma unroll
                    for (int f = 0; f < 5; ++f)
                        if (gradients & (1 << f)) {
#pragma unroll
                            for (int b = 0; b < 3; ++b) { atomicAdd(part + (size_t)c * chunk + e, (u64)sample_term(gr[b], A[f])); ++c; }
                        }
                }
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt; e += STPB) {
            if (part[e] == 0ull) continue;
            for (int c = 0; c < q.channels; ++c) {
                const u64 v = part[(size_t)c * chunk + e];
                if (v) atomicAdd((u64*)planes + (size_t)c * m + (c0 + e), v);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(STPB) void k_sample_points(const float4* __restrict__ xm, const float4* __restrict__ vf, const float4* __restrict__ aux,
                                                        int N, int tiles_per_block, SampleCommon q, const float* __restrict__ xyz, int m, int chunk,
                                                        long long* __restrict__ planes) {
    extern __shared__ __align__(16) unsigned char sample_lds[];
    sample_points_body<false>(sample_lds, xm, vf, aux, N, tiles_per_block, q, xyz, m, chunk, planes, 0);
}

__global__ __launch_bounds__(STPB) void k_sample_points_grad(const float4* __restrict__ xm, const float4* __restrict__ vf, const float4* __restrict__ aux,
                                                             int N, int tiles_per_block, SampleCommon q, const float* __restrict__ xyz, int m, int chunk,
                                                             long long* __restrict__ planes, int gradients) {
    extern __shared__ __align__(16) unsigned char sample_lds[];
    sample_points_body<true>(sample_lds, xm, vf, aux, N, tiles_per_block, q, xyz, m, chunk, planes, gradients);
}

void sph_sample_release(SphContext* c) { sph_observe_release(c->sample, &SphSample::grid, &SphSample::pts_buf); }

bool sph_sample_last_grid(const SphContext* c, SphSampledGrid* out) {
    const SphSample* s = c->sample;
    if (!s || !s->grid_have) return false;
    out->weight = s->grid + s->grid_nodes;   // plane 1: count, WEIGHT, then the fields
    out->nodes = s->grid_nodes;
    for (int a = 0; a < 3; ++a) { out->n[a] = s->grid_n[a]; out->origin[a] = s->grid_origin[a]; out->spacing[a] = s->grid_spacing[a]; }
    return true;
}

static int sample_state(SphContext* c, const char* who) {
    if (!sph_observe_state(c->sample)) { snprintf(c->err, sizeof(c->err), "%s: out of host memory", who); return SPH_E_NOMEM; }
    return 0;
}

// fields, selection and inv_h, shared by both entry points; fills q
static int sample_common(SphContext* c, const char* who, int32_t fields, const SphSampleSelect* sel, float inv_h, SampleCommon* q) {
    if (fields & ~S_ALL_FIELDS) { snprintf(c->err, sizeof(c->err), "%s: fields holds unknown bits", who); return SPH_E_INVALID; }
    if (!sel) { snprintf(c->err, sizeof(c->err), "%s: the selection is NULL", who); return SPH_E_INVALID; }
    if (int rc = sample_select(c, who, *sel, &q->sel)) return rc;
    if (!std::isfinite(inv_h) || !(inv_h > 0.f)) { snprintf(c->err, sizeof(c->err), "%s: inv_h must be finite and positive", who); return SPH_E_INVALID; }
    q->inv_h = inv_h;
    q->k_w = c->p.k_w;
    q->fields = fields;
    q->channels = 2 + __builtin_popcount((unsigned)fields);
    return 0;
}

// the gradient mask of a gradient-carrying call: known bits, each of them also in `fields` (its planes need that field's sum).
// Widens q->channels by Gx Gy Gz and three planes per bit.
static int sample_gradients(SphContext* c, const char* who, int32_t gradients, SampleCommon* q) {
    if (gradients & ~S_ALL_FIELDS) { snprintf(c->err, sizeof(c->err), "%s: gradients holds unknown bits", who); return SPH_E_INVALID; }
    if (gradients & ~q->fields) {
        snprintf(c->err, sizeof(c->err), "%s: gradients = %d names a plane that is not in fields = %d (the gradient needs that plane's sum)", who, gradients, q->fields);
        return SPH_E_INVALID;
    }
    q->channels += 3 + 3 * __builtin_popcount((unsigned)gradients);
    return 0;
}

static int sample_fail(SphContext* c, int rc, const char* who, const char* what) {
    snprintf(c->err, sizeof(c->err), "%s: %s", who, what);
    return rc;
}

static int sample_clear(SphContext* c, long long* p, size_t words) {
    size_t blocks = (words + STPB - 1) / STPB;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_sample_clear, dim3((unsigned)blocks), dim3(STPB), 0, c->stream, (u64*)p, words);
    SPH_LAUNCH_CHECK(c);
    return 0;
}

// the geometry of a public grid, checked: fills all of *g but its planes
static int sample_grid_geometry(SphContext* c, const char* who, const SphSampleGrid* p, SampleGridDev* out) {
    SampleGridDev& g = *out;
    g.h = 1.0f / p->inv_h;
    if (!std::isfinite(g.h)) return sample_fail(c, SPH_E_INVALID, who, "inv_h must be finite and positive (its reciprocal is not finite)");
    long long nodes = 1;
    for (int a = 0; a < 3; ++a) {
        if (p->n[a] < 1) return sample_fail(c, SPH_E_INVALID, who, "n[a] must be at least 1");
        nodes *= p->n[a];
        if (nodes > SPH_SAMPLE_MAX_NODES) {
            snprintf(c->err, sizeof(c->err), "%s: %d x %d x %d nodes, a grid holds at most SPH_SAMPLE_MAX_NODES = %d", who, p->n[0], p->n[1], p->n[2], SPH_SAMPLE_MAX_NODES);
            return SPH_E_INVALID;
        }
        if (!std::isfinite(p->origin[a])) return sample_fail(c, SPH_E_INVALID, who, "origin must be finite");
        if (!std::isfinite(p->spacing[a]) || !(p->spacing[a] > 0.f)) return sample_fail(c, SPH_E_INVALID, who, "spacing must be finite and positive");
        // (the second clause: the footprints are built with 1 / inv_h, which is the support radius in every intended call)
        if (p->spacing[a] < c->p.support_radius / 8.f || p->spacing[a] * p->inv_h < 0.124f) {
            snprintf(c->err, sizeof(c->err), "%s: spacing[%d] = %g is below an eighth of the support radius (%g): a particle's footprint is "
                     "bounded at 17^3 nodes", who, a, (double)p->spacing[a], (double)(c->p.support_radius / 8.f));
            return SPH_E_INVALID;
        }
        g.n[a] = p->n[a]; g.origin[a] = p->origin[a]; g.spacing[a] = p->spacing[a]; g.inv_spacing[a] = 1.0f / p->spacing[a];
    }
    g.nodes = nodes;
    g.planes = nullptr;
    return 0;
}

int sph_sample_grid_spec(SphContext* c, const char* who, const SphSampleGrid* p, SampleCommon* q, SampleGridDev* g) {
    if (int rc = sample_common(c, who, p->fields, &p->select, p->inv_h, q)) return rc;
    return sample_grid_geometry(c, who, p, g);
}

int sph_sample_grid_scatter(SphContext* c, const SampleCommon& q, const SampleGridDev& g) {
    const SphLive in = sph_live(c);
    if (in.N <= 0) return 0;
    const SphWalk w = sph_observe_walk(in.N, STPB, SG_MAX_BLOCKS);
    hipLaunchKernelGGL(k_sample_grid, dim3(w.blocks), dim3(STPB), 0, c->stream, in.xm, in.vf, in.aux, in.N, w.per_block, q, g);
    SPH_LAUNCH_CHECK(c);
    return 0;
}

// sph_sample_grid (with_grad false: `gradients` is not read) and sph_sample_grid_gradients
static int sample_grid_run(SphContext* c, const SphSampleGrid* p, bool with_grad, int32_t gradients, const char* who) {
    if (c && !p) return sample_fail(c, SPH_E_INVALID, who, "the grid is NULL");
    if (int rc = sph_observe_enter(c, who, " (its ghost records would be counted twice); fields are sampled on single-domain contexts only")) return rc;
    SampleCommon q;
    if (int rc = sample_common(c, who, p->fields, &p->select, p->inv_h, &q)) return rc;
    const int n_fields = q.channels - 2;
    if (with_grad)
        if (int rc = sample_gradients(c, who, gradients, &q)) return rc;
    SampleGridDev g;
    if (int rc = sample_grid_geometry(c, who, p, &g)) return rc;
    const long long nodes = g.nodes;
    if (int rc = sample_state(c, who)) return rc;
    SphSample* s = c->sample;
    const size_t words = (size_t)q.channels * (size_t)nodes;
    if (words > s->grid_words) {
        s->grid_words = 0; s->grid_have = false;   // (an earlier call may still be writing the planes: the helper waits for it)
        if (int rc = sph_observe_alloc(c, (void**)&s->grid, words * 8, who, "the grid's planes")) return rc;
        s->grid_words = words;
    }
    if (p->fields & (SPH_SAMPLE_DENSITY | SPH_SAMPLE_PRESSURE))
        if (int rc = sph_ensure_aux(c)) return rc;   // density / pressure of a fused step live in eos2 until somebody asks
    g.planes = s->grid;
    if (int rc = sample_clear(c, s->grid, words)) return rc;
    if (int rc = sph_ensure_pid(c)) return rc;   // the kernels below read aux
    if (with_grad) {
        const SphLive in = sph_live(c);
        if (in.N > 0) {
            const SphWalk w = sph_observe_walk(in.N, STPB, SG_MAX_BLOCKS);
            hipLaunchKernelGGL(k_sample_grid_grad, dim3(w.blocks), dim3(STPB), 0, c->stream, in.xm, in.vf, in.aux, in.N, w.per_block, q, g, (int)gradients);
            SPH_LAUNCH_CHECK(c);
        }
    } else if (int rc = sph_sample_grid_scatter(c, q, g)) {
        return rc;
    }
    s->grid_nodes = nodes;
    for (int a = 0; a < 3; ++a) { s->grid_n[a] = g.n[a]; s->grid_origin[a] = g.origin[a]; s->grid_spacing[a] = g.spacing[a]; }
    s->grid_fields = n_fields;
    s->grid_grads = q.channels - 2 - n_fields;
    s->grid_have = true;
    return 0;
}

// the points the planes are cut into: what the plain instance always took, and for the gradient instance no more than fit its LDS budget
static int sample_points_chunk(int m, int channels, bool with_grad) {
    int cap = SP_CHUNK;
    if (with_grad) {
        cap = (int)(SP_LDS_BYTES / ((size_t)channels * 8 + 12)) & ~1;   // 25 channels: 164
        if (cap > SP_CHUNK) cap = SP_CHUNK;
    }
    const int chunk = m < cap ? m : cap;
    return (chunk + 1) & ~1;
}

extern "C" {

int32_t sph_sample_grid(SphContext* c, const SphSampleGrid* p) { return sample_grid_run(c, p, false, 0, "sph_sample_grid"); }

int32_t sph_sample_grid_gradients(SphContext* c, const SphSampleGrid* p, int32_t gradients) {
    return sample_grid_run(c, p, true, gradients, "sph_sample_grid_gradients");
}

int32_t sph_sample_grid_gradients_download(SphContext* c, int64_t* grads, int64_t nodes) {
    if (!c) return SPH_E_INVALID;
    const SphSample* s = c->sample;
    if (!s || !s->grid_have) return sph_fail(c, SPH_E_STATE, "sph_sample_grid_gradients_download: nothing has been sampled (call sph_sample_grid_gradients first)");
    if (s->grid_grads == 0) return sph_fail(c, SPH_E_STATE, "sph_sample_grid_gradients_download: the last grid was sampled without gradients (call sph_sample_grid_gradients)");
    if (nodes != s->grid_nodes) {
        snprintf(c->err, sizeof(c->err), "sph_sample_grid_gradients_download: nodes = %lld, the last grid has %lld nodes", (long long)nodes, s->grid_nodes);
        return SPH_E_INVALID;
    }
    SPH_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)s->grid_nodes;
    if (grads) SPH_HIP(c, hipMemcpyAsync(grads, s->grid + (size_t)(2 + s->grid_fields) * n, (size_t)s->grid_grads * n * 8, hipMemcpyDeviceToHost, c->stream));
    return sph_observe_download(c, nullptr, nullptr, 0);
}

int32_t sph_sample_grid_download(SphContext* c, int64_t* weight, int64_t* count, int64_t* sums, int64_t nodes) {
    if (!c) return SPH_E_INVALID;
    const SphSample* s = c->sample;
    if (!s || !s->grid_have) return sph_fail(c, SPH_E_STATE, "sph_sample_grid_download: nothing has been sampled (call sph_sample_grid first)");
    if (nodes != s->grid_nodes) {
        snprintf(c->err, sizeof(c->err), "sph_sample_grid_download: nodes = %lld, the last sph_sample_grid made a grid of %lld nodes", (long long)nodes, s->grid_nodes);
        return SPH_E_INVALID;
    }
    SPH_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)s->grid_nodes;
    if (count) SPH_HIP(c, hipMemcpyAsync(count, s->grid, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (weight) SPH_HIP(c, hipMemcpyAsync(weight, s->grid + n, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (sums && s->grid_fields > 0) SPH_HIP(c, hipMemcpyAsync(sums, s->grid + 2 * n, (size_t)s->grid_fields * n * 8, hipMemcpyDeviceToHost, c->stream));
    return sph_observe_download(c, nullptr, nullptr, 0);
}

}  // extern "C"

// sph_sample_points (with_grad false: `gradients` is not read) and sph_sample_points_gradients
static int sample_points_run(SphContext* c, const float* xyz, int32_t m, int32_t fields, bool with_grad, int32_t gradients,
                             const SphSampleSelect* select, float inv_h, const char* who) {
    if (c && !xyz) return sample_fail(c, SPH_E_INVALID, who, "xyz is NULL");
    if (int rc = sph_observe_enter(c, who, " (its ghost records would be counted twice); fields are sampled on single-domain contexts only")) return rc;
    SampleCommon q;
    if (int rc = sample_common(c, who, fields, select, inv_h, &q)) return rc;
    const int n_fields = q.channels - 2;
    if (with_grad)
        if (int rc = sample_gradients(c, who, gradients, &q)) return rc;
    if (m < 1 || m > SPH_SAMPLE_MAX_POINTS) {
        snprintf(c->err, sizeof(c->err), "%s: m = %d, must be in [1, SPH_SAMPLE_MAX_POINTS = %d]", who, m, SPH_SAMPLE_MAX_POINTS);
        return SPH_E_INVALID;
    }
    for (int k = 0; k < 3 * m; ++k)
        if (!std::isfinite(xyz[k])) return sample_fail(c, SPH_E_INVALID, who, "a point is not finite");
    if (int rc = sample_state(c, who)) return rc;
    SphSample* s = c->sample;
    if (!s->pts_buf) {
        const size_t bytes = (size_t)3 * SPH_SAMPLE_MAX_POINTS * 4 + (size_t)(SG_MAX_CHANNELS + SG_MAX_GRAD_CHANNELS) * SPH_SAMPLE_MAX_POINTS * 8;
        if (int rc = sph_observe_alloc(c, &s->pts_buf, bytes, who, "the points and their planes")) return rc;
        s->pts = (long long*)((char*)s->pts_buf + (size_t)3 * SPH_SAMPLE_MAX_POINTS * 4);
    }
    if (fields & (SPH_SAMPLE_DENSITY | SPH_SAMPLE_PRESSURE))
        if (int rc = sph_ensure_aux(c)) return rc;   // density / pressure of a fused step live in eos2 until somebody asks
    if (s->pts_copying) SPH_HIP(c, hipStreamSynchronize(c->stream));   // the host copy must not change before the last copy has been made
    memcpy(s->pts_host, xyz, (size_t)3 * m * 4);
    s->pts_copying = true;
    SPH_HIP(c, hipMemcpyAsync(s->pts_buf, s->pts_host, (size_t)3 * m * 4, hipMemcpyHostToDevice, c->stream));
    if (int rc = sample_clear(c, s->pts, (size_t)q.channels * m)) return rc;
    if (int rc = sph_ensure_pid(c)) return rc;   // the kernels below read aux
    const SphLive in = sph_live(c);
    if (in.N > 0) {
        const SphWalk w = sph_observe_walk(in.N, STPB, SP_MAX_BLOCKS);
        const int chunk = sample_points_chunk(m, q.channels, with_grad);
        const size_t lds = (size_t)chunk * ((size_t)q.channels * 8 + 12);   // <= 512 * 68 B = 34,816 B
        if (with_grad)
            hipLaunchKernelGGL(k_sample_points_grad, dim3(w.blocks), dim3(STPB), lds, c->stream, in.xm, in.vf, in.aux, in.N, w.per_block, q,
                               (const float*)s->pts_buf, m, chunk, s->pts, (int)gradients);
        else
            hipLaunchKernelGGL(k_sample_points, dim3(w.blocks), dim3(STPB), lds, c->stream, in.xm, in.vf, in.aux, in.N, w.per_block, q,
                               (const float*)s->pts_buf, m, chunk, s->pts);
        SPH_LAUNCH_CHECK(c);
    }
    s->pts_m = m;
    s->pts_fields = n_fields;
    s->pts_grads = q.channels - 2 - n_fields;
    s->pts_have = true;
    return 0;
}

extern "C" {

int32_t sph_sample_points(SphContext* c, const float* xyz, int32_t m, int32_t fields, const SphSampleSelect* select, float inv_h) {
    return sample_points_run(c, xyz, m, fields, false, 0, select, inv_h, "sph_sample_points");
}

int32_t sph_sample_points_gradients(SphContext* c, const float* xyz, int32_t m, int32_t fields, int32_t gradients, const SphSampleSelect* select,
                                    float inv_h) {
    return sample_points_run(c, xyz, m, fields, true, gradients, select, inv_h, "sph_sample_points_gradients");
}

int32_t sph_sample_points_gradients_download(SphContext* c, int64_t* grads, int32_t m) {
    if (!c) return SPH_E_INVALID;
    SphSample* s = c->sample;
    if (!s || !s->pts_have) return sph_fail(c, SPH_E_STATE, "sph_sample_points_gradients_download: nothing has been sampled (call sph_sample_points_gradients first)");
    if (s->pts_grads == 0) return sph_fail(c, SPH_E_STATE, "sph_sample_points_gradients_download: the last points were sampled without gradients (call sph_sample_points_gradients)");
    if (m != s->pts_m) {
        snprintf(c->err, sizeof(c->err), "sph_sample_points_gradients_download: m = %d, the last points call took %d points", m, s->pts_m);
        return SPH_E_INVALID;
    }
    SPH_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)s->pts_m;
    if (grads) SPH_HIP(c, hipMemcpyAsync(grads, s->pts + (size_t)(2 + s->pts_fields) * n, (size_t)s->pts_grads * n * 8, hipMemcpyDeviceToHost, c->stream));
    const int rc = sph_observe_download(c, nullptr, nullptr, 0);
    if (rc <= 0) s->pts_copying = false;   // the stream has drained: the host copy of the points is free again
    return rc;
}

int32_t sph_sample_points_download(SphContext* c, int64_t* weight, int64_t* count, int64_t* sums, int32_t m) {
    if (!c) return SPH_E_INVALID;
    SphSample* s = c->sample;
    if (!s || !s->pts_have) return sph_fail(c, SPH_E_STATE, "sph_sample_points_download: nothing has been sampled (call sph_sample_points first)");
    if (m != s->pts_m) {
        snprintf(c->err, sizeof(c->err), "sph_sample_points_download: m = %d, the last sph_sample_points took %d points", m, s->pts_m);
        return SPH_E_INVALID;
    }
    SPH_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)s->pts_m;
    if (count) SPH_HIP(c, hipMemcpyAsync(count, s->pts, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (weight) SPH_HIP(c, hipMemcpyAsync(weight, s->pts + n, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (sums && s->pts_fields > 0) SPH_HIP(c, hipMemcpyAsync(sums, s->pts + 2 * n, (size_t)s->pts_fields * n * 8, hipMemcpyDeviceToHost, c->stream));
    const int rc = sph_observe_download(c, nullptr, nullptr, 0);
    if (rc <= 0) s->pts_copying = false;   // the stream has drained: the host copy of the points is free again
    return rc;
}

}  // extern "C"
