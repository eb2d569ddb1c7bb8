// sph_features.hip -- per-particle flow features (include/sph_hip.h, "Particle features"): vorticity, velocity divergence, the colour
// gradient (the raw surface normal), the kernel fill, the neighbour counts and a free-surface flag of every selected particle,
// sampled inside the WCSPH step right behind its density and pressure, as ONE row per PERSISTENT id held on the device (the latest
// sample only).  Reads xm, vf, aux and cell_end; writes the buffers of this file and, in the paint call alone, color_cold.  No
// particle state is written and no existing kernel is touched.
//
// One sample is two clears (the 4-byte target count, the rows) and two launches:
//  (a) k_features_select: a streaming walk over the flags (vf.w) of the live records.  A selected record goes into an index list: one
//      wave ballot, ONE atomic per wave that found any (on the count), as k_loads_select does.  The list's order depends on the order
//      the waves' atomics arrive in; that is immaterial, every target owning its row.  The host never reads the count.
//  (b) k_features_gather, gfx950 wave64, the shape of the load and the scalar gathers: SIXTEEN lanes (one DPP row) serve one target, a
//      wave four.  The grid is FIXED (sized from the record capacity at the set) and its waves stride over the count on the device.  A
//      row walks the nine z-runs of the 27 cells around its target -- run (i, j) is [cell_end[f(z_lo) - 1], cell_end[f(z_hi)]), z
//      clipped to the grid, the run clipped to [0, N] -- sixteen records a trip: the 16-byte xm record first, the geometry test, and
//      only for an accepted pair vf (flags, velocity) and, of a fluid candidate, aux (m, density).  Each lane keeps thirteen i64 sums
//      (fill, N[3], G[9] -- G[3 a + b], a the velocity component, b the direction), two pair counts and a saturation count; the row is combined with DPP row rotations (row_sum of sph_observe.h) and lane 0 of the row
//      FINISHES: it turns the integer sums into the 64-byte output row and stores it at rows[id].  No LDS, no atomics but the list's.
// The arithmetic is the header's, term by term: f32 pair geometry and kernel polynomial through sample_pair's own code (k_w = 1,
// m_V = 1: the bare polynomial), f64 terms with nothing contracted, the clamps, llrint, integer sums.  Every float of a row is
// (float)((double)I / 2^s) of an integer or an integer difference, so the row is one function of the sampled state whatever the lane
// split or the launch order.
// BUDGET: a term is at most 2^44 in magnitude (N, G: clamp 2^20 at scale 2^24; fill: clamp 2^14 at scale 2^30), so 2^18 pair terms AT
// THE CLAMP still fit an i64 (2^62), and the sums of three (divergence) or the differences of two (vorticity) of them as well.  A
// term of the 1.75 M workload is below 2^7 (G) and 2^5 (N): twelve orders of magnitude of head room.
#include <cmath>
#include <cstdlib>
#include "sph_observe.h"
#include "sph_sample_pair.h"

#pragma clang fp contract(off)

#define FT_TPB 256
#define FT_ROW 16                        // lanes per target: one DPP row
#define FT_PER_BLOCK (FT_TPB / FT_ROW)
#define FT_SELECT_MAX_BLOCKS 2048
#define FT_GATHER_MAX_BLOCKS 4096        // 65,536 rows in flight; more targets are taken in further trips of the waves
#define FT_SCALE 16777216.0              // 2^24 (SPH_FEATURES_SCALE_LOG2): N and G
#define FT_LIMIT 1048576.0               // 2^20
#define FT_FILL_SCALE 1073741824.0       // 2^30 (SPH_FEATURES_FILL_SCALE_LOG2)
#define FT_FILL_LIMIT 16384.0            // 2^14
#define FT_MAX_NEIGHBOURS (1 << 20)

static_assert(sizeof(SphFeatureRow) == 64, "a feature row is four 16-byte stores");
static_assert(SPH_FEATURES_SCALE_LOG2 == 24 && SPH_FEATURES_FILL_SCALE_LOG2 == 30, "FT_SCALE and FT_FILL_SCALE are the header's scales");

struct SphFeatureSet {
    int* list;                // [list_cap] record indices of the targets, then one word: their count
    size_t list_cap;
    SphFeatureRow* rows;      // [n_rows] by persistent id: the latest sample
    size_t rows_cap;          // allocated
    int* lut;                 // [256][3] the table of the last paint
    int lut_host[256 * 3];
    bool have;                // a set is registered
    bool lut_set;
    int every, min_neighbours, gather_blocks;
    float normal_min;
    long long n_rows;
    SphSel sel;
    long long samples, steps_seen, last_step;
    double last_time;
};

struct FeatArgs {
    float grid_size, inv_h, h, k_w, k_dw, normal_min;
    int n[3];                 // grid_num
    int N, list_cap, min_neighbours;
    long long n_rows;
};

__global__ __launch_bounds__(FT_TPB) void k_features_select(const float4* __restrict__ vf, SphSel sel, int N, int per_block, int* __restrict__ list,
                                                            int list_cap, int* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const long long tile0 = (long long)blockIdx.x * per_block;
    for (int tile = 0; tile < per_block; ++tile) {
        const long long i = (tile0 + tile) * FT_TPB + threadIdx.x;   // uniform trip count: every lane reaches the ballot
        const bool hit = i < N && sph_selected(__float_as_int(vf[i].w), sel);
        const u64 mask = __ballot(hit);
        if (mask == 0) continue;
        const int leader = __ffsll((long long)mask) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(count, __popcll(mask));
        base = __shfl(base, leader, 64);
        const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && pos < list_cap) list[pos] = (int)i;
    }
}

// one term into an integer: clamped, counted when the clamp changed it (a NaN ends at -limit), rounded to nearest even
__device__ __forceinline__ long long feat_term(double f, double limit, double scale, int& sat) {
    const double cl = fmin(fmax(f, -limit), limit);
    sat += cl != f;
    return llrint(cl * scale);
}

// the volume a record stands for: m / rho of a fluid record, the boundary volume of any other
__device__ __forceinline__ double feat_volume(bool fluid, const float4& X, const float4& A) {
    return fluid ? (double)A.x / (double)A.y : (double)X.w;
}

__device__ __forceinline__ float feat_float(long long I, double scale) { return (float)((double)I / scale); }

__global__ __launch_bounds__(FT_TPB) void k_features_gather(const float4* __restrict__ xm, const float4* __restrict__ vf, const float4* __restrict__ aux,
                                                            const int* __restrict__ cell_end, const int* __restrict__ list,
                                                            const int* __restrict__ count, FeatArgs a, SphFeatureRow* __restrict__ rows) {
    const int sub = threadIdx.x & (FT_ROW - 1);
    int n_targets = *count;                              // one address: the same value in every lane
    n_targets = n_targets > a.list_cap ? a.list_cap : n_targets;
    const int stride = (int)gridDim.x * FT_PER_BLOCK;    // <= 2^16
    const int wave0 = (blockIdx.x * FT_PER_BLOCK + (threadIdx.x >> 4)) & ~3;   // the first of the wave's four rows
    const int row_in_wave = (threadIdx.x >> 4) & 3;
    const double kdw = (double)a.k_dw, kw = (double)a.k_w, h = (double)a.h;
    for (long long first_t = wave0; first_t < n_targets; first_t += stride) {   // uniform over the wave: every lane reaches the DPP sums
        const long long t = first_t + row_in_wave;
        bool live = t < n_targets;
        int i = 0;
        if (live) {
            i = list[t];
            live = i >= 0 && i < a.N;
        }
        long long s_fill = 0, s_n[3] = {0, 0, 0}, s_g[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        int n_fluid = 0, n_solid = 0, sat = 0;
        float4 Xi = make_float4(0.f, 0.f, 0.f, 0.f), Vi = Xi, Ai = Xi;
        if (live) {
            Xi = xm[i]; Vi = vf[i]; Ai = aux[i];
            if (sub == 0)   // the self term of the fill, once per target: V_i * W(0), W(0) = k_w * 1
                s_fill = feat_term(feat_volume(sph_is_fluid(__float_as_int(Vi.w)), Xi, Ai) * (kw * 1.0), FT_FILL_LIMIT, FT_FILL_SCALE, sat);
            // the sort's own cell coordinates of the target (pos_to_index with its clamp): a record the sort clamped into a border
            // cell is a candidate through that cell
            const int c0 = sph_cell_coord(Xi.x, a.grid_size, 0, a.n[0]), c1 = sph_cell_coord(Xi.y, a.grid_size, 0, a.n[1]),
                      c2 = sph_cell_coord(Xi.z, a.grid_size, 0, a.n[2]);
            const int zlo = c2 - 1 < 0 ? 0 : c2 - 1, zhi = c2 + 1 > a.n[2] - 1 ? a.n[2] - 1 : c2 + 1;
            for (int di = -1; di <= 1; ++di) {
                const int cx = c0 + di;
                if (cx < 0 || cx >= a.n[0]) continue;
                for (int dj = -1; dj <= 1; ++dj) {
                    const int cy = c1 + dj;
                    if (cy < 0 || cy >= a.n[1]) continue;
                    const int f = (cx * a.n[1] + cy) * a.n[2];
                    int first = f + zlo > 0 ? cell_end[f + zlo - 1] : 0;
                    int last = cell_end[f + zhi];
                    first = first < 0 ? 0 : first;
                    last = last > a.N ? a.N : last;
                    for (int j = first + sub; j < last; j += FT_ROW) {
                        const float4 Xj = xm[j];
                        const float4 X1 = make_float4(Xj.x, Xj.y, Xj.z, 1.f);
                        float P;   // the bare kernel polynomial of q: sample_pair's W with k_w = 1 and m_V = 1 (in [0, 1]: its clamp is idle)
                        SamplePairGeom g;
                        if (!sample_pair(Xi.x, Xi.y, Xi.z, X1, a.inv_h, 1.f, P, g)) continue;   // d = x_i - x_j, q <= 1
                        if (!(g.r > 1e-5f)) continue;
                        const float4 Vj = vf[j];
                        const bool fluid = sph_is_fluid(__float_as_int(Vj.w));
                        float4 Aj = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (fluid) Aj = aux[j];                                       // (m, density, pressure, id)
                        const double vol = feat_volume(fluid, Xj, Aj);
                        const double q = (double)g.q, r = (double)g.r;
                        const double gq = g.q <= 0.5f ? q * (3.0 * q - 2.0) : -((1.0 - q) * (1.0 - q));
                        const double coef = (kdw * gq) / (r * h);
                        const double gW[3] = {coef * (double)g.d[0], coef * (double)g.d[1], coef * (double)g.d[2]};
                        s_fill += feat_term(vol * (kw * (double)P), FT_FILL_LIMIT, FT_FILL_SCALE, sat);
#pragma unroll
                        for (int b = 0; b < 3; ++b) s_n[b] += feat_term(vol * gW[b], FT_LIMIT, FT_SCALE, sat);
                        if (fluid) {
                            const float dv[3] = {Vj.x - Vi.x, Vj.y - Vi.y, Vj.z - Vi.z};
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const double vdv = vol * (double)dv[c];
#pragma unroll
                                for (int b = 0; b < 3; ++b) s_g[3 * c + b] += feat_term(vdv * gW[b], FT_LIMIT, FT_SCALE, sat);
                            }
                            n_fluid += 1;
                        } else {
                            n_solid += 1;
                        }
                    }
                }
            }
        }
        // every lane of the wave is here again: rows without a target carry zeros
        s_fill = row_sum(s_fill);
#pragma unroll
        for (int b = 0; b < 3; ++b) s_n[b] = row_sum(s_n[b]);
#pragma unroll
        for (int k = 0; k < 9; ++k) s_g[k] = row_sum(s_g[k]);
        n_fluid = row_sum(n_fluid); n_solid = row_sum(n_solid); sat = row_sum(sat);
        if (!live || sub != 0) continue;
        // ---- the finish: the integer sums of this target into its row, by persistent id ----
        const int id = __float_as_int(Ai.w);
        if (id < 0 || id >= a.n_rows) continue;
        const double nx = (double)s_n[0] / FT_SCALE, ny = (double)s_n[1] / FT_SCALE, nz = (double)s_n[2] / FT_SCALE;
        const double n2 = (nx * nx + ny * ny) + nz * nz;
        const double nm = (double)a.normal_min;
        const bool surface = n_fluid + n_solid < a.min_neighbours || (a.normal_min > 0.f && (h * h) * n2 > nm * nm);
        const int flags = SPH_FEATURE_VALID | (surface ? SPH_FEATURE_SURFACE : 0) | (sat > 0 ? SPH_FEATURE_SATURATED : 0);
        // G[3 * a + b] = d v_a / d x_b
        const float wx = feat_float(s_g[7] - s_g[5], FT_SCALE), wy = feat_float(s_g[2] - s_g[6], FT_SCALE), wz = feat_float(s_g[3] - s_g[1], FT_SCALE);
        const float div = feat_float((s_g[0] + s_g[4]) + s_g[8], FT_SCALE);
        float4* out = reinterpret_cast<float4*>(rows + id);
        out[0] = make_float4(Xi.x, Xi.y, Xi.z, wx);
        out[1] = make_float4(wy, wz, div, feat_float(s_n[0], FT_SCALE));
        out[2] = make_float4(feat_float(s_n[1], FT_SCALE), feat_float(s_n[2], FT_SCALE), feat_float(s_fill, FT_FILL_SCALE), __int_as_float(n_fluid));
        out[3] = make_float4(__int_as_float(n_solid), __int_as_float(flags), 0.f, 0.f);
    }
}

struct FeatPaint { float lo, inv; int field, cold_cap; long long n_rows; };

// the table colour of every valid row's field into the object colour of its id; sph_render.hip's index arithmetic, verbatim
__global__ __launch_bounds__(FT_TPB) void k_features_paint(const int* __restrict__ ids, int id_stride, int N, int per_block,
                                                           const SphFeatureRow* __restrict__ rows, FeatPaint p, const int* __restrict__ lut,
                                                           int* __restrict__ color_cold) {
    const long long tile0 = (long long)blockIdx.x * per_block;
    for (int tile = 0; tile < per_block; ++tile) {
        const long long i = (tile0 + tile) * FT_TPB + threadIdx.x;
        if (i >= N) return;
        const int id = ids[(size_t)i * id_stride];
        if (id < 0 || id >= p.n_rows || id >= p.cold_cap) continue;
        const SphFeatureRow R = rows[id];
        if (!(R.flags & SPH_FEATURE_VALID)) continue;
        float s;
        switch (p.field) {
            case SPH_FEATURE_FIELD_VORTICITY:
                s = sqrtf((R.vorticity[0] * R.vorticity[0] + R.vorticity[1] * R.vorticity[1]) + R.vorticity[2] * R.vorticity[2]);
                break;
            case SPH_FEATURE_FIELD_DIVERGENCE: s = R.divergence; break;
            case SPH_FEATURE_FIELD_FILL: s = R.fill; break;
            case SPH_FEATURE_FIELD_NEIGHBOURS: s = (float)(R.n_fluid + R.n_solid); break;
            default: s = (R.flags & SPH_FEATURE_SURFACE) ? 1.f : 0.f; break;
        }
        float t = (s - p.lo) * p.inv;
        t = t >= 0.f ? fminf(t, 1.f) : 0.f;
        const int idx = (int)(t * 255.f + 0.5f);
        for (int c = 0; c < 3; ++c) color_cold[3 * (size_t)id + c] = lut[3 * idx + c];
    }
}

void sph_features_release(SphContext* c) { sph_observe_release(c->features, &SphFeatureSet::list, &SphFeatureSet::rows, &SphFeatureSet::lut); }

bool sph_features_armed(const SphContext* c) { return c->features && c->features->have; }

// ONE sample of the current records, remembered as the sample of step `step` at simulated time t
static int features_take(SphContext* c, SphFeatureSet* s, double t, long long step) {
    if (int rc = sph_ensure_aux(c)) return rc;   // m, density and the id of a record are read from aux (the values every later reader would get anyway)
    const SphLive in = sph_live(c);
    SPH_HIP(c, hipMemsetAsync(s->rows, 0, (size_t)s->n_rows * sizeof(SphFeatureRow), c->stream));   // a row outside the selection is all zero
    if (in.N > 0) {
        const SphParams& p = c->p;
        FeatArgs a;
        a.grid_size = p.grid_size; a.inv_h = 1.0f / p.support_radius; a.h = p.support_radius; a.k_w = p.k_w; a.k_dw = p.k_dw;
        a.normal_min = s->normal_min;
        for (int k = 0; k < 3; ++k) a.n[k] = p.grid_num[k];
        a.N = in.N; a.list_cap = (int)s->list_cap; a.min_neighbours = s->min_neighbours; a.n_rows = s->n_rows;
        int* count = s->list + s->list_cap;
        SPH_HIP(c, hipMemsetAsync(count, 0, sizeof(int), c->stream));
        const SphWalk w = sph_observe_walk(in.N, FT_TPB, FT_SELECT_MAX_BLOCKS);
        hipLaunchKernelGGL(k_features_select, dim3(w.blocks), dim3(FT_TPB), 0, c->stream, in.vf, s->sel, in.N, w.per_block, s->list, (int)s->list_cap, count);
        SPH_LAUNCH_CHECK(c);
        hipLaunchKernelGGL(k_features_gather, dim3(s->gather_blocks), dim3(FT_TPB), 0, c->stream, in.xm, in.vf, in.aux, (const int*)c->cell_end,
                           (const int*)s->list, (const int*)count, a, s->rows);
        SPH_LAUNCH_CHECK(c);
    }
    s->last_time = t;
    s->last_step = step;
    s->samples += 1;
    return 0;
}

// step_sweeps' hook behind the step's density and pressure: x(t_k), v(t_k), this step's sort, this step's rho.  Nothing when no set
// is registered.
int sph_features_step(SphContext* c) {
    SphFeatureSet* s = c->features;
    if (!s || !s->have) return 0;
    const long long k = s->steps_seen;
    s->steps_seen += 1;
    return k % s->every == 0 ? features_take(c, s, c->sim_time, k) : 0;
}

static int features_fail(SphContext* c, int rc, const char* who, const char* what) {
    snprintf(c->err, sizeof(c->err), "%s: %s", who, what);
    return rc;
}

static const char* const FT_WHY_SLAB = " (a particle's neighbours beyond the halo belong to another rank, and the rows are by global id); particle features exist on single-domain contexts only";
static const char* const FT_NO_SET = "no feature set is registered (call sph_features_set first)";

static void features_zero_counters(SphFeatureSet* s) {
    s->samples = s->steps_seen = 0;
    s->last_step = -1;
    s->last_time = 0.0;
}

extern "C" {

int32_t sph_features_set(SphContext* c, const SphFeatureParams* fp) {
    const char* who = "sph_features_set";
    if (int rc = sph_observe_enter(c, who, FT_WHY_SLAB)) return rc;
    if (!fp) {   // clears the set; the buffers stay for the next one
        if (c->features) { c->features->have = false; features_zero_counters(c->features); }
        return 0;
    }
    SphSel sel;
    if (int rc = sample_select(c, who, fp->select, &sel)) return rc;
    if (fp->every < 1) return features_fail(c, SPH_E_INVALID, who, "every must be at least 1");
    if (fp->min_neighbours < 0 || fp->min_neighbours > FT_MAX_NEIGHBOURS) {
        snprintf(c->err, sizeof(c->err), "%s: min_neighbours = %d, must be in [0, 2^20]", who, fp->min_neighbours);
        return SPH_E_INVALID;
    }
    if (!std::isfinite(fp->normal_min) || fp->normal_min < 0.f) return features_fail(c, SPH_E_INVALID, who, "normal_min must be finite and not negative");
    if (c->cold_cap < 1) return features_fail(c, SPH_E_STATE, who, "the context holds no persistent ids");
    if (!sph_observe_state(c->features)) return features_fail(c, SPH_E_NOMEM, who, "out of host memory");
    SphFeatureSet* s = c->features;
    // grow only; whatever has to grow exists before anything old goes: a failure leaves the last good set as it was
    void *nl = nullptr, *nr = nullptr, *nt = nullptr;
    const size_t list_cap = (size_t)(c->cap > 0 ? c->cap : 1), n_rows = (size_t)c->cold_cap;
    int rc = 0;
    if (list_cap > s->list_cap) rc = sph_observe_alloc(c, &nl, (list_cap + 1) * sizeof(int), who, "the target list");
    if (!rc && n_rows > s->rows_cap) rc = sph_observe_alloc(c, &nr, n_rows * sizeof(SphFeatureRow), who, "the rows");
    if (!rc && !s->lut) rc = sph_observe_alloc(c, &nt, sizeof(s->lut_host), who, "the colour table");
    hipError_t e = rc ? hipSuccess : hipStreamSynchronize(c->stream);   // (a sample may still be writing the old buffers)
    if (rc || e != hipSuccess) {   // nothing old has gone yet
        if (nl) (void)hipFree(nl);
        if (nr) (void)hipFree(nr);
        if (nt) (void)hipFree(nt);
        if (rc) return rc;
        SPH_HIP(c, e);
    }
    if (nl) { (void)hipFree(s->list); s->list = (int*)nl; s->list_cap = list_cap; }
    if (nr) { (void)hipFree(s->rows); s->rows = (SphFeatureRow*)nr; s->rows_cap = n_rows; }
    if (nt) s->lut = (int*)nt;
    s->every = fp->every; s->min_neighbours = fp->min_neighbours; s->normal_min = fp->normal_min;
    s->n_rows = (long long)n_rows;
    s->sel = sel;
    long long blocks = ((long long)s->list_cap + FT_PER_BLOCK - 1) / FT_PER_BLOCK;
    if (blocks > FT_GATHER_MAX_BLOCKS) blocks = FT_GATHER_MAX_BLOCKS;
    if (const char* env = getenv("SPH_FEATURES_BLOCKS")) {   // test aid (sph_hip.h): can only SHRINK the grid, so that the waves take several trips over a short list
        const long long b = atoll(env);
        if (b >= 1 && b < blocks) blocks = b;
    }
    s->gather_blocks = (int)blocks;
    features_zero_counters(s);
    s->have = true;
    SPH_HIP(c, hipMemsetAsync(s->rows, 0, n_rows * sizeof(SphFeatureRow), c->stream));
    SPH_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int32_t sph_features_sample(SphContext* c) {
    const char* who = "sph_features_sample";
    if (int rc = sph_observe_enter(c, who, FT_WHY_SLAB)) return rc;
    SphFeatureSet* s = c->features;
    if (!s || !s->have) return features_fail(c, SPH_E_STATE, who, FT_NO_SET);
    if (!sphs_neighbours_ready(c->ss)) return features_fail(c, SPH_E_STATE, who, "needs the neighbour structure: call sph_initialize_particle_system first");
    return features_take(c, s, c->sim_time, s->steps_seen);
}

int32_t sph_features_info(SphContext* c, SphFeatureInfo* out) {
    if (!c) return SPH_E_INVALID;
    if (!out) return sph_fail(c, SPH_E_INVALID, "sph_features_info: the result is NULL");
    const SphFeatureSet* s = c->features;
    memset(out, 0, sizeof(*out));
    out->step = -1;
    if (!s || !s->have) return 0;
    out->every = s->every; out->rows = s->n_rows; out->samples = s->samples; out->steps_seen = s->steps_seen;
    out->step = s->last_step; out->time = s->last_time;
    return 0;
}

int32_t sph_features_download(SphContext* c, void* rows, int64_t n_rows) {
    const char* who = "sph_features_download";
    if (int rc = sph_observe_enter(c, who, FT_WHY_SLAB)) return rc;
    const SphFeatureSet* s = c->features;
    if (!s || !s->have) return features_fail(c, SPH_E_STATE, who, FT_NO_SET);
    if (n_rows != s->n_rows) {
        snprintf(c->err, sizeof(c->err), "%s: n_rows = %lld, the set holds %lld rows", who, (long long)n_rows, s->n_rows);
        return SPH_E_INVALID;
    }
    return sph_observe_download(c, rows, s->rows, (size_t)n_rows * sizeof(SphFeatureRow));
}

int32_t sph_features_paint(SphContext* c, int32_t field, float lo, float hi, const int32_t* lut) {
    const char* who = "sph_features_paint";
    if (int rc = sph_observe_enter(c, who, FT_WHY_SLAB)) return rc;
    SphFeatureSet* s = c->features;
    if (!s || !s->have) return features_fail(c, SPH_E_STATE, who, FT_NO_SET);
    if (field < 0 || field >= SPH_FEATURE_FIELDS) {
        snprintf(c->err, sizeof(c->err), "%s: field = %d, must be in [0, SPH_FEATURE_FIELDS = %d)", who, field, SPH_FEATURE_FIELDS);
        return SPH_E_INVALID;
    }
    if (!std::isfinite(lo) || !std::isfinite(hi)) return features_fail(c, SPH_E_INVALID, who, "lo and hi must be finite");
    if (!(lo < hi)) return features_fail(c, SPH_E_INVALID, who, "lo must be smaller than hi");
    FeatPaint p;
    p.lo = lo;
    p.inv = 1.0f / (hi - lo);
    if (!(p.inv > 0.0f) || !std::isfinite(p.inv)) return features_fail(c, SPH_E_INVALID, who, "the range is too narrow or too wide for binary32");
    if (!lut) return features_fail(c, SPH_E_INVALID, who, "the table is NULL");
    for (int k = 0; k < 256 * 3; ++k)
        if (lut[k] < 0 || lut[k] > 255) return features_fail(c, SPH_E_INVALID, who, "a table entry lies outside [0, 255]");
    if (!s->lut_set || memcmp(s->lut_host, lut, sizeof(s->lut_host)) != 0) {
        // behind the paints that still read the old table; the host copy must not change before the copy has been made
        SPH_HIP(c, hipStreamSynchronize(c->stream));
        memcpy(s->lut_host, lut, sizeof(s->lut_host));
        SPH_HIP(c, hipMemcpyAsync(s->lut, s->lut_host, sizeof(s->lut_host), hipMemcpyHostToDevice, c->stream));
        SPH_HIP(c, hipStreamSynchronize(c->stream));
        s->lut_set = true;
    }
    const SphLive in = sph_live(c);
    if (in.N <= 0) return 0;
    p.field = field; p.cold_cap = c->cold_cap; p.n_rows = s->n_rows;
    const SphIds ids = sph_observe_ids(c);
    const SphWalk w = sph_observe_walk(in.N, FT_TPB, FT_SELECT_MAX_BLOCKS);
    hipLaunchKernelGGL(k_features_paint, dim3(w.blocks), dim3(FT_TPB), 0, c->stream, ids.ptr, ids.stride, in.N, w.per_block,
                       (const SphFeatureRow*)s->rows, p, (const int*)s->lut, c->color_cold);
    SPH_LAUNCH_CHECK(c);
    return 0;
}

}  // extern "C"
