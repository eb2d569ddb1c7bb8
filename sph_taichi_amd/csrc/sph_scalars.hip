// sph_scalars.hip -- carried scalars (include/sph_hip.h, "Carried scalars"): up to four channels of a quantity that rides on the
// particles -- dye, heat, a concentration -- kept by PERSISTENT id in a store the sort never moves (the first evolving per-id array:
// x0_cold and color_cold are constant), and diffused between neighbours inside the step by an explicit Jacobi step of Brookshaw's
// Laplacian through the cell array of the step's sort.  Reads vf.w, xm, the record's id and cell_end; writes the buffers of this file
// and, in the paint call alone, color_cold.  No particle state is written and no existing kernel is touched.
//
// THE ID OF A RECORD lives in the pid array while a lean scatter keeps the ids apart from aux, and in aux.w otherwise (sph_derived.h).
// The kernels take a pointer and a stride (pid: 1; aux: the fourth word of a 16-byte record, stride 4) and never ask for the fold:
// sph_ensure_aux would write particle state and cost the pure-fluid step its lean and fast sorts.
//
// One sample is one 4-byte memset (the carrier count) and two launches:
//  (a) k_scalars_stage: a streaming walk over the live records (sph_observe_walk).  Per record the flags (vf.w) and the id decide the
//      role: SOURCE (its object is one of the set's sources: the prescribed value), CARRIER (selected, id inside the store: C[id], one
//      random read of 8 K bytes), or none.  It writes, in RECORD order, the snapshot Cs[k][i] -- channel planes, so that the
//      diffusion's candidate reads are coalesced -- with the mark SC_NONE in plane 0 of a record that takes no part; the role is
//      that mark plus membership of the carrier list.  The carriers' record indices go into a compact list: one wave ballot, ONE
//      atomic per wave that found any (on the count), as k_loads_select does.  The list's order depends on the order the atomics
//      arrive in; that is immaterial, every target being independent.  The host never reads the count.
//  (b) k_scalars_diffuse<K>, gfx950 wave64, the shape of the tracer and the load gathers: SIXTEEN lanes (one DPP row) serve one
//      carrier, a wave four.  The grid is FIXED (sized from the record capacity at the set) and its waves stride over the count on
//      the device.  A row walks the nine z-runs of the 27 cells around its target -- run (i, j) is [cell_end[f(z_lo) - 1],
//      cell_end[f(z_hi)]), z clipped to the grid, the run clipped to [0, N] -- sixteen records a trip: the 16-byte xm record first
//      (consecutive records: 256 B per row-load), the geometry test, and only for an accepted pair the 8 K bytes of the snapshot.
//      Each lane keeps 2 K i64 sums (terms, weights); the row is combined with DPP row rotations (row_sum of sph_observe.h) and lane
//      0 of the row writes the K new values to C[id_i] and issues a counter atomic only for a non-zero count.  No LDS, no scratch.
// Reads come from the snapshot only and writes go to the store only, so a sample is a Jacobi step whatever the order of the rows.
// The arithmetic is the header's, term by term: f32 pair geometry through sample_pair's own code, f64 weights with nothing
// contracted, llrint, integer sums.  The only atomics are integer adds on the two counters and the list count.
#include <cmath>
#include <cstdlib>
#include "sph_observe.h"
#include "sph_sample_pair.h"
#include "sph_scalars_check.h"

#pragma clang fp contract(off)

#define SC_TPB 256
#define SC_ROW 16                        // lanes per target: one DPP row
#define SC_PER_BLOCK (SC_TPB / SC_ROW)
#define SC_STAGE_MAX_BLOCKS 2048
#define SC_DIFFUSE_MAX_BLOCKS 4096       // 65,536 rows in flight; more carriers are taken in further trips of the waves
#define SC_KMAX SPH_SCALARS_MAX_CHANNELS
#define SC_SMAX SPH_SCALARS_MAX_SOURCES
#define SC_NONE ((long long)0x8000000000000000ull)   // plane 0 of a record that takes no part (a value never leaves +-2^52)
#define SC_ONE 4294967296.0              // 2^32
#define SC_LIMIT 4503599627370496ll      // 2^52

struct SphScalarSet {
    long long* store;         // [ids_cap][K] by persistent id, channel fastest
    size_t store_words;       // allocated
    long long* snap;          // [SC_KMAX][snap_cap] by record, channel planes
    size_t snap_cap;          // records per plane
    int* list;                // [list_cap] record indices of the carriers, then one word: their count
    size_t list_cap;
    unsigned long long* counters;   // [2][SC_KMAX]: overshoot, saturated
    int* lut;                 // [256][3] the table of the last paint
    int lut_host[256 * 3];
    bool have;                // a set is registered
    bool lut_set;
    int K, every, n_sources, diffuse_blocks;
    long long n_ids;
    float kappa[SC_KMAX];
    SphSel sel;
    int source_object[SC_SMAX];
    long long source_raw[SC_SMAX][SC_KMAX];
    long long samples, steps_seen;
};

struct ScalarRoles {
    SphSel sel;
    int n_sources, K;
    int source_object[SC_SMAX];
    long long source_raw[SC_SMAX][SC_KMAX];
    long long n_ids;
};

struct ScalarArgs {
    float grid_size, inv_h, h, k_dw;
    int n[3];                 // grid_num
    int N, list_cap;
    double a[SC_KMAX];        // dt * every * kappa
    long long snap_cap;
};

// slot of an object among the sources, -1: none (uniform index: scalar loads)
__device__ __forceinline__ int scalars_source(int obj, const ScalarRoles& r) {
    int slot = -1;
    for (int k = 0; k < r.n_sources; ++k) slot = obj == r.source_object[k] ? k : slot;
    return slot;
}

// the prescribed value of source `slot` in channel k (uniform indices: scalar loads, no indexed copy of the arguments)
__device__ __forceinline__ long long scalars_source_value(const ScalarRoles& r, int slot, int k) {
    long long v = 0;
    for (int s = 0; s < r.n_sources; ++s) v = slot == s ? r.source_raw[s][k] : v;
    return v;
}

enum { SC_ROLE_NONE = 0, SC_ROLE_CARRIER = 1, SC_ROLE_SOURCE = 2 };

__device__ __forceinline__ int scalars_role(int flags, int id, const ScalarRoles& r, int& slot) {
    slot = scalars_source(sph_flags_object(flags), r);
    if (slot >= 0) return SC_ROLE_SOURCE;
    return sph_selected(flags, r.sel) && id >= 0 && id < r.n_ids ? SC_ROLE_CARRIER : SC_ROLE_NONE;
}

__global__ __launch_bounds__(SC_TPB) void k_scalars_stage(const float4* __restrict__ vf, const int* __restrict__ ids, int id_stride, ScalarRoles r,
                                                          int N, int per_block, const long long* __restrict__ store, long long* __restrict__ snap,
                                                          long long snap_cap, int* __restrict__ list, int list_cap, int* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const long long tile0 = (long long)blockIdx.x * per_block;
    for (int tile = 0; tile < per_block; ++tile) {
        const long long i = (tile0 + tile) * SC_TPB + threadIdx.x;   // uniform trip count: every lane reaches the ballot
        bool hit = false;
        if (i < N && i < snap_cap) {
            const int fl = __float_as_int(vf[i].w);
            const int id = ids[(size_t)i * id_stride];
            int slot;
            const int role = scalars_role(fl, id, r, slot);
            if (role == SC_ROLE_NONE) {
                snap[i] = SC_NONE;
            } else {
                for (int k = 0; k < r.K; ++k)
                    snap[(size_t)k * snap_cap + i] = role == SC_ROLE_SOURCE ? scalars_source_value(r, slot, k) : store[(size_t)id * r.K + k];
            }
            hit = role == SC_ROLE_CARRIER;
        }
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

template <int K>
__global__ __launch_bounds__(SC_TPB) void k_scalars_diffuse(const float4* __restrict__ xm, const int* __restrict__ ids, int id_stride,
                                                            const int* __restrict__ cell_end, const int* __restrict__ list,
                                                            const int* __restrict__ count, ScalarArgs a, const long long* __restrict__ snap,
                                                            long long n_ids, long long* __restrict__ store, unsigned long long* __restrict__ counters) {
    const int sub = threadIdx.x & (SC_ROW - 1);
    int n_targets = *count;                              // one address: the same value in every lane
    n_targets = n_targets > a.list_cap ? a.list_cap : n_targets;
    const int stride = (int)gridDim.x * SC_PER_BLOCK;    // <= 2^16
    const int wave0 = (blockIdx.x * SC_PER_BLOCK + (threadIdx.x >> 4)) & ~3;   // the first of the wave's four rows
    const int row_in_wave = (threadIdx.x >> 4) & 3;
    const double kdw = (double)a.k_dw, h = (double)a.h;
    const double soft = (0.01 * h) * h;
    for (long long first_t = wave0; first_t < n_targets; first_t += stride) {   // uniform over the wave: every lane reaches the DPP sums
        const long long t = first_t + row_in_wave;
        bool live = t < n_targets;
        int i = 0;
        if (live) {
            i = list[t];
            live = i >= 0 && i < a.N && i < a.snap_cap;
        }
        long long Ci[K], sum[K], wsum[K];
#pragma unroll
        for (int k = 0; k < K; ++k) Ci[k] = sum[k] = wsum[k] = 0;
        if (live) {
            const float4 Xi = xm[i];
#pragma unroll
            for (int k = 0; k < K; ++k) Ci[k] = snap[(size_t)k * a.snap_cap + i];
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
                    last = last > a.snap_cap ? (int)a.snap_cap : last;
                    for (int j = first + sub; j < last; j += SC_ROW) {
                        const float4 Xj = xm[j];
                        float w_unused;
                        SamplePairGeom g;
                        if (!sample_pair(Xi.x, Xi.y, Xi.z, Xj, a.inv_h, 0.f, w_unused, g)) continue;   // d = x_i - x_j, q <= 1
                        if (!(g.r > 1e-5f)) continue;
                        const long long Cj0 = snap[j];
                        if (Cj0 == SC_NONE) continue;                                 // takes no part
                        const double q = (double)g.q, r = (double)g.r;
                        const double gq = g.q <= 0.5f ? q * (3.0 * q - 2.0) : -((1.0 - q) * (1.0 - q));
                        const double lap = ((2.0 * (kdw * gq)) * r) / (h * (r * r + soft));
                        const double mVj = (double)Xj.w;
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const long long Cj = k == 0 ? Cj0 : snap[(size_t)k * a.snap_cap + j];
                            const double w = fmin(fmax((-(a.a[k] * mVj)) * lap, 0.0), 1.0);
                            sum[k] += llrint((double)(Cj - Ci[k]) * w);
                            wsum[k] += llrint(w * SC_ONE);
                        }
                    }
                }
            }
        }
        // every lane of the wave is here again: rows without a target carry zeros
#pragma unroll
        for (int k = 0; k < K; ++k) { sum[k] = row_sum(sum[k]); wsum[k] = row_sum(wsum[k]); }
        if (!live || sub != 0) continue;
        const int id = ids[(size_t)i * id_stride];
        if (id < 0 || id >= n_ids) continue;            // (the stage listed only records whose id is inside the store)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const long long v = Ci[k] + sum[k];
            const long long cl = v > SC_LIMIT ? SC_LIMIT : v < -SC_LIMIT ? -SC_LIMIT : v;
            store[(size_t)id * K + k] = cl;
            if (wsum[k] > (long long)SC_ONE) atomicAdd(counters + k, 1ull);
            if (cl != v) atomicAdd(counters + SC_KMAX + k, 1ull);
        }
    }
}

struct PaintArgs { float lo, inv; int channel, cold_cap; };

// the table colour of every participant's value into the object colour of its id; sph_render.hip's index arithmetic, verbatim
__global__ __launch_bounds__(SC_TPB) void k_scalars_paint(const float4* __restrict__ vf, const int* __restrict__ ids, int id_stride, ScalarRoles r,
                                                          int N, int per_block, const long long* __restrict__ store, PaintArgs p,
                                                          const int* __restrict__ lut, int* __restrict__ color_cold) {
    const long long tile0 = (long long)blockIdx.x * per_block;
    for (int tile = 0; tile < per_block; ++tile) {
        const long long i = (tile0 + tile) * SC_TPB + threadIdx.x;
        if (i >= N) return;
        const int fl = __float_as_int(vf[i].w);
        const int id = ids[(size_t)i * id_stride];
        int slot;
        const int role = scalars_role(fl, id, r, slot);
        if (role == SC_ROLE_NONE || id < 0 || id >= p.cold_cap) continue;
        const long long C = role == SC_ROLE_SOURCE ? scalars_source_value(r, slot, p.channel) : store[(size_t)id * r.K + p.channel];
        const float s = (float)((double)C * (1.0 / SC_ONE));
        float t = (s - p.lo) * p.inv;
        t = t >= 0.f ? fminf(t, 1.f) : 0.f;
        const int idx = (int)(t * 255.f + 0.5f);
        for (int c = 0; c < 3; ++c) color_cold[3 * (size_t)id + c] = lut[3 * idx + c];
    }
}

void sph_scalars_release(SphContext* c) {
    sph_observe_release(c->scalars, &SphScalarSet::store, &SphScalarSet::snap, &SphScalarSet::list, &SphScalarSet::counters, &SphScalarSet::lut);
}

// where the ids of the current records are (sph_observe.h): nobody is asked to move them
typedef SphIds ScalarIds;
static ScalarIds scalars_ids(const SphContext* c) { return sph_observe_ids(c); }

static ScalarRoles scalars_roles(const SphScalarSet* s) {
    ScalarRoles r;
    r.sel = s->sel;
    r.n_sources = s->n_sources; r.K = s->K; r.n_ids = s->n_ids;
    for (int k = 0; k < SC_SMAX; ++k) {
        r.source_object[k] = s->source_object[k];
        for (int ch = 0; ch < SC_KMAX; ++ch) r.source_raw[k][ch] = s->source_raw[k][ch];
    }
    return r;
}

// ONE sample of the current records
static int scalars_take(SphContext* c, SphScalarSet* s) {
    const SphLive in = sph_live(c);
    if (in.N > 0) {
        const SphParams& p = c->p;
        ScalarArgs a;
        a.grid_size = p.grid_size; a.inv_h = 1.0f / p.support_radius; a.h = p.support_radius; a.k_dw = p.k_dw;
        for (int k = 0; k < 3; ++k) a.n[k] = p.grid_num[k];
        a.N = in.N; a.list_cap = (int)s->list_cap; a.snap_cap = (long long)s->snap_cap;
        for (int k = 0; k < SC_KMAX; ++k) a.a[k] = k < s->K ? ((double)p.dt * (double)s->every) * (double)s->kappa[k] : 0.0;
        const ScalarIds ids = scalars_ids(c);
        int* count = s->list + s->list_cap;
        SPH_HIP(c, hipMemsetAsync(count, 0, sizeof(int), c->stream));
        const SphWalk w = sph_observe_walk(in.N, SC_TPB, SC_STAGE_MAX_BLOCKS);
        hipLaunchKernelGGL(k_scalars_stage, dim3(w.blocks), dim3(SC_TPB), 0, c->stream, in.vf, ids.ptr, ids.stride, scalars_roles(s), in.N, w.per_block,
                           (const long long*)s->store, s->snap, (long long)s->snap_cap, s->list, (int)s->list_cap, count);
        SPH_LAUNCH_CHECK(c);
#define SC_LAUNCH(KK)                                                                                                                              \
    hipLaunchKernelGGL(k_scalars_diffuse<KK>, dim3(s->diffuse_blocks), dim3(SC_TPB), 0, c->stream, in.xm, ids.ptr, ids.stride, (const int*)c->cell_end, \
                       (const int*)s->list, (const int*)count, a, (const long long*)s->snap, s->n_ids, s->store, s->counters)
        switch (s->K) {
            case 1: SC_LAUNCH(1); break;
            case 2: SC_LAUNCH(2); break;
            case 3: SC_LAUNCH(3); break;
            default: SC_LAUNCH(4); break;
        }
#undef SC_LAUNCH
        SPH_LAUNCH_CHECK(c);
    }
    s->samples += 1;
    return 0;
}

// step_loop's hook behind the head-of-step sort: counts the step; a 4-byte clear and two launches when a sample is due
int sph_scalars_step(SphContext* c) {
    SphScalarSet* s = c->scalars;
    if (!s || !s->have) return 0;
    const bool due = s->steps_seen % s->every == 0;
    s->steps_seen += 1;
    return due ? scalars_take(c, s) : 0;
}

static int scalars_fail(SphContext* c, int rc, const char* who, const char* what) {
    snprintf(c->err, sizeof(c->err), "%s: %s", who, what);
    return rc;
}

static const char* const SC_WHY_SLAB = " (a carrier's neighbours beyond the halo belong to another rank, and the store is by global id); scalars exist on single-domain contexts only";
static const char* const SC_NO_SET = "no scalar set is registered (call sph_scalars_set first)";

extern "C" {

int32_t sph_scalars_set(SphContext* c, const double* values, int64_t n_ids, const SphScalarParams* sp) {
    const char* who = "sph_scalars_set";
    if (int rc = sph_observe_enter(c, who, SC_WHY_SLAB)) return rc;
    if (!sp || sp->K == 0) {   // clears the set; the buffers stay for the next one
        if (c->scalars) { c->scalars->have = false; c->scalars->samples = c->scalars->steps_seen = 0; }
        return 0;
    }
    if (int rc = sph_scalars_check_set(sp, values, n_ids, c->p.n_objects, c->cold_cap, c->err, sizeof(c->err))) return rc;   // sph_scalars_check.h
    SphSel sel;
    if (int rc = sample_select(c, who, sp->select, &sel)) return rc;
    const size_t words = (size_t)n_ids * (size_t)sp->K;
    long long* host = (long long*)calloc(words, sizeof(long long));
    if (!host) return scalars_fail(c, SPH_E_NOMEM, who, "out of host memory");
    if (values)
        for (size_t k = 0; k < words; ++k) host[k] = llrint(values[k] * SC_ONE);
    if (!sph_observe_state(c->scalars)) { free(host); return scalars_fail(c, SPH_E_NOMEM, who, "out of host memory"); }
    SphScalarSet* s = c->scalars;
    // grow only; whatever has to grow exists before anything old goes: a failure leaves the last good set as it was
    void *ns = nullptr, *np = nullptr, *nl = nullptr, *nc = nullptr, *nt = nullptr;
    const size_t cap = (size_t)(c->cap > 0 ? c->cap : 1);   // records: a snapshot plane, the list
    int rc = 0;
    if (words > s->store_words) rc = sph_observe_alloc(c, &ns, words * 8, who, "the store");
    if (!rc && cap > s->snap_cap) rc = sph_observe_alloc(c, &np, cap * SC_KMAX * 8, who, "the snapshot");
    if (!rc && cap > s->list_cap) rc = sph_observe_alloc(c, &nl, (cap + 1) * sizeof(int), who, "the carrier list");
    if (!rc && !s->counters) rc = sph_observe_alloc(c, &nc, 2 * SC_KMAX * 8, who, "the counters");
    if (!rc && !s->lut) rc = sph_observe_alloc(c, &nt, sizeof(s->lut_host), who, "the colour table");
    if (rc) {
        if (ns) (void)hipFree(ns);
        if (np) (void)hipFree(np);
        if (nl) (void)hipFree(nl);
        if (nc) (void)hipFree(nc);
        if (nt) (void)hipFree(nt);
        free(host);
        return rc;
    }
    hipError_t e = hipStreamSynchronize(c->stream);   // (a sample may still be writing the old buffers)
    if (e != hipSuccess) {   // nothing old has gone yet
        if (ns) (void)hipFree(ns);
        if (np) (void)hipFree(np);
        if (nl) (void)hipFree(nl);
        if (nc) (void)hipFree(nc);
        if (nt) (void)hipFree(nt);
        free(host);
        SPH_HIP(c, e);
    }
    // from here on the old set is gone: a device error below leaves NO set registered (the header says so), never a half-made one
    s->have = false;
    s->samples = s->steps_seen = 0;
    if (ns) { (void)hipFree(s->store); s->store = (long long*)ns; s->store_words = words; }
    if (np) { (void)hipFree(s->snap); s->snap = (long long*)np; s->snap_cap = cap; }
    if (nl) { (void)hipFree(s->list); s->list = (int*)nl; s->list_cap = cap; }
    if (nc) s->counters = (unsigned long long*)nc;
    if (nt) s->lut = (int*)nt;
    e = hipMemcpyAsync(s->store, host, words * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->counters, 0, 2 * SC_KMAX * 8, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    free(host);
    SPH_HIP(c, e);
    s->K = sp->K; s->every = sp->every; s->n_sources = sp->n_sources; s->n_ids = n_ids;
    s->sel = sel;
    for (int k = 0; k < SC_KMAX; ++k) s->kappa[k] = k < sp->K ? sp->kappa[k] : 0.f;
    for (int k = 0; k < SC_SMAX; ++k) {
        s->source_object[k] = k < sp->n_sources ? sp->source_object[k] : -1;
        for (int ch = 0; ch < SC_KMAX; ++ch)
            s->source_raw[k][ch] = k < sp->n_sources && ch < sp->K ? llrint(sp->source_value[k][ch] * SC_ONE) : 0;
    }
    long long blocks = ((long long)s->list_cap + SC_PER_BLOCK - 1) / SC_PER_BLOCK;
    if (blocks > SC_DIFFUSE_MAX_BLOCKS) blocks = SC_DIFFUSE_MAX_BLOCKS;
    if (const char* env = getenv("SPH_SCALARS_BLOCKS")) {   // test aid (sph_hip.h): can only SHRINK the grid, so that the waves take several trips over a short list
        const long long b = atoll(env);
        if (b >= 1 && b < blocks) blocks = b;
    }
    s->diffuse_blocks = (int)blocks;
    s->samples = s->steps_seen = 0;
    s->have = true;
    return 0;
}

int32_t sph_scalars_sample(SphContext* c) {
    const char* who = "sph_scalars_sample";
    if (int rc = sph_observe_enter(c, who, SC_WHY_SLAB)) return rc;
    SphScalarSet* s = c->scalars;
    if (!s || !s->have) return scalars_fail(c, SPH_E_STATE, who, SC_NO_SET);
    if (!sphs_neighbours_ready(c->ss)) return scalars_fail(c, SPH_E_STATE, who, "needs the neighbour structure: call sph_initialize_particle_system first");
    return scalars_take(c, s);
}

int32_t sph_scalars_info(SphContext* c, SphScalarInfo* out) {
    if (!c) return SPH_E_INVALID;
    if (!out) return sph_fail(c, SPH_E_INVALID, "sph_scalars_info: the result is NULL");
    const SphScalarSet* s = c->scalars;
    const bool have = s && s->have;
    memset(out, 0, sizeof(*out));
    if (!have) return 0;
    out->K = s->K; out->every = s->every; out->ids = s->n_ids; out->samples = s->samples; out->steps_seen = s->steps_seen;
    unsigned long long w[2 * SC_KMAX];
    if (int rc = sph_observe_download(c, w, s->counters, sizeof(w))) return rc;
    for (int k = 0; k < s->K; ++k) { out->overshoot[k] = (int64_t)w[k]; out->saturated[k] = (int64_t)w[SC_KMAX + k]; }
    return 0;
}

int32_t sph_scalars_download(SphContext* c, int64_t* raw, double* values, int64_t n_ids) {
    const char* who = "sph_scalars_download";
    if (int rc = sph_observe_enter(c, who, SC_WHY_SLAB)) return rc;
    const SphScalarSet* s = c->scalars;
    if (!s || !s->have) return scalars_fail(c, SPH_E_STATE, who, SC_NO_SET);
    if (n_ids != s->n_ids) {
        snprintf(c->err, sizeof(c->err), "%s: n_ids = %lld, the set holds %lld ids", who, (long long)n_ids, s->n_ids);
        return SPH_E_INVALID;
    }
    const size_t words = (size_t)n_ids * (size_t)s->K;
    int64_t* tmp = raw;
    if (!raw && values) {
        tmp = (int64_t*)malloc(words * 8);
        if (!tmp) return scalars_fail(c, SPH_E_NOMEM, who, "out of host memory");
    }
    const int rc = sph_observe_download(c, tmp, s->store, words * 8);
    if (!rc && values)
        for (size_t k = 0; k < words; ++k) values[k] = (double)tmp[k] * (1.0 / SC_ONE);
    if (tmp != raw) free(tmp);
    return rc;
}

int32_t sph_scalars_paint(SphContext* c, int32_t channel, float lo, float hi, const int32_t* lut) {
    const char* who = "sph_scalars_paint";
    if (int rc = sph_observe_enter(c, who, SC_WHY_SLAB)) return rc;
    SphScalarSet* s = c->scalars;
    if (!s || !s->have) return scalars_fail(c, SPH_E_STATE, who, SC_NO_SET);
    PaintArgs p;
    p.lo = lo;
    if (int rc = sph_scalars_check_paint(s->K, channel, lo, hi, lut, &p.inv, c->err, sizeof(c->err))) return rc;   // sph_scalars_check.h
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
    p.channel = channel; p.cold_cap = c->cold_cap;
    const ScalarIds ids = scalars_ids(c);
    const SphWalk w = sph_observe_walk(in.N, SC_TPB, SC_STAGE_MAX_BLOCKS);
    hipLaunchKernelGGL(k_scalars_paint, dim3(w.blocks), dim3(SC_TPB), 0, c->stream, in.vf, ids.ptr, ids.stride, scalars_roles(s), in.N, w.per_block,
                       (const long long*)s->store, p, (const int*)s->lut, c->color_cold);
    SPH_LAUNCH_CHECK(c);
    return 0;
}

}  // extern "C"
