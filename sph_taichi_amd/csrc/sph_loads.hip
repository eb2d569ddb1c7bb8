// sph_loads.hip -- fluid loads on solid objects (include/sph_hip.h, "Fluid loads"): force and torque the fluid exerts on up to 32
// selected solid objects, sampled inside the WCSPH step right behind its density and pressure, as a time series held on the device.
// The force sweep computes the same Akinci boundary term for its fluid TARGETS and keeps none of it for static or kinematic solids;
// this observer GATHERS it the other way round: every selected solid particle j looks for the fluid particles i around it through
// the cell array of the step's sort.  Reads vf.w, xm, aux and cell_end; writes the buffers of this file and nothing else.  No
// existing kernel is touched.
//
// One sample is one 4-byte memset (the target count) and two launches:
//  (a) k_loads_select: a streaming walk over the flags (vf.w) of the live records.  A solid-material record whose object is in the
//      set goes into an index list: one wave ballot, ONE atomic per wave that found any (on the count), each hit stores its index at
//      the wave's base plus the number of hits below its lane.  The list's order depends on the order the waves' atomics arrive in;
//      that is immaterial, every sum below being an integer sum.  The list has the context's record capacity, so it cannot overflow;
//      a store past it is skipped all the same.
//  (b) k_loads_gather, gfx950 wave64, the tracer kernel's shape: SIXTEEN lanes (one DPP row) serve one target, a wave four.  The grid
//      is FIXED (sized from the record capacity at registration) and its waves stride over the count the select left ON THE DEVICE:
//      the host never reads it, the hook never synchronises.  A row walks the nine z-runs of the 27 cells around its target -- run
//      (i, j) is [cell_end[f(z_lo) - 1], cell_end[f(z_hi)]), z clipped to the grid, the run clipped to [0, N] -- sixteen records a
//      trip: the flags first (the fluid test), then xm and aux of the fluid candidates.  Each lane keeps three i64 force sums, a pair
//      count and a saturation count; the row is combined with DPP row rotations (row_sum of sph_observe.h), lane 0 of the row forms
//      the torque terms of its target.  When the (up to) four targets of a wave belong to ONE object -- the usual case: solids of an
//      object are neighbours in the sort, and the select keeps a wave's hits together -- the four rows are combined across the wave
//      and ONE lane issues the nine i64 atomics into the sample's row of the history; otherwise each row issues its own.  A wave
//      (or row) whose nine numbers are all zero -- a dry target inside the body -- issues nothing.
//
// The arithmetic (sph_hip.h has it term by term): the pair geometry d = x_i - x_j, r2, r, q in f32 through sample_pair's own code
// (SamplePairGeom, the correctly rounded sqrtf), accepted iff q <= 1 and r > 1e-5; the pair coefficient and the three components in
// f64 from those f32 values and the f32 record fields, every operation an IEEE f64 multiply, divide or subtract, nothing contracted,
// no f32 divide, no rcp, no rsq; each component clamped to +-2^16 N and rounded by llrint(f * 2^24).  From there on everything is
// an integer.
// WHY THE i64 ATOMICS CANNOT CHANGE A BIT: every term that reaches an atomic is an integer fixed BEFORE the atomic is issued (a pair
// term depends on one fluid and one solid record, a torque term on the integer force sum of one target, which is complete in its
// row).  The atomics are no-return integer adds on words nobody else writes during the sample (sample k owns row k, zeroed at
// registration or reset).  Addition in Z / 2^64 is associative and commutative, so the word's final value is the sum of the same
// multiset of integers whatever the order of arrival, the lane split, the per-wave or per-row form, or the order of the list.  There
// is no float or double atomic anywhere.
// BUDGET: a force term is at most 2^40 in magnitude (the clamp 2^16 N at scale 2^24), so 2^22 pair terms AT THE CLAMP still fit an
// i64 (2^62); a torque term is clamped at 2^40 as well, so 2^22 targets at the clamp fit.  A pair term of the 1.75 M workload is
// below 2^-3 N: nine orders of magnitude of head room.
#include <cmath>
#include <cstdlib>
#include "sph_observe.h"
#include "sph_sample_pair.h"

#pragma clang fp contract(off)

#define LD_TPB 256
#define LD_ROW 16                        // lanes per target: one DPP row
#define LD_PER_BLOCK (LD_TPB / LD_ROW)
#define LD_SELECT_MAX_BLOCKS 2048
#define LD_GATHER_MAX_BLOCKS 2048        // 32,768 rows in flight; more targets are taken in further trips of the waves
#define LD_WORDS SPH_LOADS_ROW_WORDS     // Fx Fy Fz Tx Ty Tz pairs wet saturated
#define LD_F_LIMIT 65536.0               // 2^16 N
#define LD_SCALE 16777216.0              // 2^24
#define LD_T_LIMIT 1099511627776.0       // 2^40, of the scaled torque term
#define LD_MAX_HISTORY_BYTES (1ull << 31)

struct SphLoadSet {
    int* list;                // [list_cap] sorted-order indices of the selected solid particles, then one word: their count
    size_t list_cap;
    long long* hist;          // [capacity][n_objects][LD_WORDS]
    size_t hist_words;        // allocated
    double* times;            // host, [capacity]
    size_t times_cap;
    bool have;                // a set is registered
    int n_objects, every, capacity;
    int gather_blocks;
    SphSel sel;               // material solid, the set's ids: slot k of the history is object_ids[k]
    float about[3];
    long long samples, dropped, steps_seen;
};

struct LoadArgs {
    float grid_size, inv_h, h, k_dw, rho0, about[3];
    int n[3];                 // grid_num
    int N, n_objects, list_cap;
    int object_ids[32];
};

// slot of an object in the set, -1: not in it (uniform index: scalar loads)
__device__ __forceinline__ int loads_slot(int obj, const LoadArgs& a) {
    int slot = -1;
    for (int k = 0; k < a.n_objects; ++k) slot = obj == a.object_ids[k] ? k : slot;
    return slot;
}

__global__ __launch_bounds__(LD_TPB) void k_loads_select(const float4* __restrict__ vf, LoadArgs a, int per_block, int* __restrict__ list,
                                                         int* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const long long tile0 = (long long)blockIdx.x * per_block;
    for (int tile = 0; tile < per_block; ++tile) {
        const long long i = (tile0 + tile) * LD_TPB + threadIdx.x;   // uniform trip count: every lane reaches the ballot
        bool hit = false;
        if (i < a.N) {
            const int fl = __float_as_int(vf[i].w);
            hit = sph_flags_material(fl) == SPH_MATERIAL_SOLID && loads_slot(sph_flags_object(fl), a) >= 0;
        }
        const u64 mask = __ballot(hit);
        if (mask == 0) continue;
        const int leader = __ffsll((long long)mask) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(count, __popcll(mask));
        base = __shfl(base, leader, 64);
        const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && pos < a.list_cap) list[pos] = (int)i;
    }
}

__device__ __forceinline__ long long shfl_i64(long long v, int src) {
    const int lo = __shfl((int)(v & 0xffffffffll), src, 64), hi = __shfl((int)(v >> 32), src, 64);
    return ((long long)hi << 32) | (unsigned)lo;
}

__device__ __forceinline__ void loads_add(long long* row, const long long v[LD_WORDS]) {
#pragma unroll
    for (int w = 0; w < LD_WORDS; ++w)
        if (v[w] != 0) atomicAdd(reinterpret_cast<unsigned long long*>(row + w), (unsigned long long)v[w]);
}

__global__ __launch_bounds__(LD_TPB) void k_loads_gather(const float4* __restrict__ xm, const float4* __restrict__ vf, const float4* __restrict__ aux,
                                                         const int* __restrict__ cell_end, const int* __restrict__ list,
                                                         const int* __restrict__ count, LoadArgs a, long long* __restrict__ out) {
    const int sub = threadIdx.x & (LD_ROW - 1);
    const int lane = threadIdx.x & 63;
    int n_targets = *count;                              // one address: the same value in every lane
    n_targets = n_targets > a.list_cap ? a.list_cap : n_targets;
    const int stride = (int)gridDim.x * LD_PER_BLOCK;    // <= 2^15
    const int wave0 = (blockIdx.x * LD_PER_BLOCK + (threadIdx.x >> 4)) & ~3;   // the first of the wave's four rows
    const int row_in_wave = (threadIdx.x >> 4) & 3;
    const double rho0 = (double)a.rho0, kdw = (double)a.k_dw, h = (double)a.h;
    for (long long first_t = wave0; first_t < n_targets; first_t += stride) {   // uniform over the wave: every lane reaches the DPP sums
        const long long t = first_t + row_in_wave;
        bool live = t < n_targets;
        int j = 0, slot = -1;
        float4 Xj = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
            j = list[t];
            live = j >= 0 && j < a.N;
        }
        if (live) {
            Xj = xm[j];
            slot = loads_slot(sph_flags_object(__float_as_int(vf[j].w)), a);
            live = slot >= 0;
        }
        long long s_x = 0, s_y = 0, s_z = 0;
        int pairs = 0, sat = 0;
        if (live) {
            // the sort's own cell coordinates of the target (pos_to_index with its clamp): a fluid particle the sort clamped into a
            // border cell is a candidate through that cell
            const int c0 = sph_cell_coord(Xj.x, a.grid_size, 0, a.n[0]), c1 = sph_cell_coord(Xj.y, a.grid_size, 0, a.n[1]),
                      c2 = sph_cell_coord(Xj.z, a.grid_size, 0, a.n[2]);
            const int zlo = c2 - 1 < 0 ? 0 : c2 - 1, zhi = c2 + 1 > a.n[2] - 1 ? a.n[2] - 1 : c2 + 1;
            const double mVj = (double)Xj.w;
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
                    for (int k = first + sub; k < last; k += LD_ROW) {
                        if (!sph_is_fluid(__float_as_int(vf[k].w))) continue;
                        const float4 Xi = xm[k];
                        float w_unused;
                        SamplePairGeom g;
                        if (!sample_pair(Xi.x, Xi.y, Xi.z, Xj, a.inv_h, 0.f, w_unused, g)) continue;   // d = x_i - x_j, q <= 1
                        if (!(g.r > 1e-5f)) continue;
                        const float4 A = aux[k];                                   // (m, density, pressure, id)
                        const double q = (double)g.q, r = (double)g.r;
                        const double gq = g.q <= 0.5f ? q * (3.0 * q - 2.0) : -((1.0 - q) * (1.0 - q));
                        const double m = (double)A.x, rho = (double)A.y, p = (double)A.z;
                        const double dp = p / (rho * rho) + p / (rho0 * rho0);
                        const double coef = (((m * rho0) * mVj) * dp) * ((kdw * gq) / (r * h));
                        long long term[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const double fc = coef * (double)g.d[c];
                            const double cl = fmin(fmax(fc, -LD_F_LIMIT), LD_F_LIMIT);   // a NaN ends at -2^16, counted
                            sat += cl != fc;
                            term[c] = llrint(cl * LD_SCALE);
                        }
                        s_x += term[0]; s_y += term[1]; s_z += term[2];
                        pairs += 1;
                    }
                }
            }
        }
        // every lane of the wave is here again: rows without a target carry zeros
        s_x = row_sum(s_x); s_y = row_sum(s_y); s_z = row_sum(s_z);
        pairs = row_sum(pairs); sat = row_sum(sat);
        long long v[LD_WORDS];
        v[0] = s_x; v[1] = s_y; v[2] = s_z;
        {   // the torque of the target's integer force about the set's point (every lane computes its row's: lane 0 is the one read)
            const float ax = Xj.x - a.about[0], ay = Xj.y - a.about[1], az = Xj.z - a.about[2];
            const double A[3] = {(double)ax, (double)ay, (double)az};
            const double F[3] = {(double)s_x / LD_SCALE, (double)s_y / LD_SCALE, (double)s_z / LD_SCALE};
            const double T[3] = {A[1] * F[2] - A[2] * F[1], A[2] * F[0] - A[0] * F[2], A[0] * F[1] - A[1] * F[0]};
            int tsat = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double ts = T[c] * LD_SCALE;
                const double cl = fmin(fmax(ts, -LD_T_LIMIT), LD_T_LIMIT);
                tsat += cl != ts;
                v[3 + c] = llrint(cl);
            }
            v[6] = pairs;
            v[7] = pairs > 0 ? 1 : 0;
            v[8] = sat + tsat;
        }
        if (!live) {
#pragma unroll
            for (int w = 0; w < LD_WORDS; ++w) v[w] = 0;
        }
        // one object in the whole wave?  (rows without a target agree with everybody)
        const int s0 = __shfl(slot, 0, 64), s1 = __shfl(slot, 16, 64), s2 = __shfl(slot, 32, 64), s3 = __shfl(slot, 48, 64);
        int ref = s0 >= 0 ? s0 : s1 >= 0 ? s1 : s2 >= 0 ? s2 : s3;
        const bool one = (s0 < 0 || s0 == ref) && (s1 < 0 || s1 == ref) && (s2 < 0 || s2 == ref) && (s3 < 0 || s3 == ref);
        if (one) {   // uniform branch
            long long tot[LD_WORDS];
#pragma unroll
            for (int w = 0; w < LD_WORDS; ++w) tot[w] = (v[w] + shfl_i64(v[w], 16)) + (shfl_i64(v[w], 32) + shfl_i64(v[w], 48));
            if (lane == 0 && ref >= 0) loads_add(out + (size_t)ref * LD_WORDS, tot);
        } else if (sub == 0 && live) {
            loads_add(out + (size_t)slot * LD_WORDS, v);
        }
    }
}

void sph_loads_release(SphContext* c) {
    if (c->loads) free(c->loads->times);
    sph_observe_release(c->loads, &SphLoadSet::list, &SphLoadSet::hist);
}

bool sph_loads_armed(const SphContext* c) { return c->loads && c->loads->have; }

// ONE sample of the current records at simulated time t into history row `samples`; a full history counts it as dropped and enqueues nothing
static int loads_take(SphContext* c, SphLoadSet* s, double t) {
    if (s->samples >= s->capacity) { s->dropped += 1; return 0; }
    if (int rc = sph_ensure_aux(c)) return rc;   // density / pressure of a fused step live in eos2 until somebody asks
    const SphLive in = sph_live(c);
    if (in.N > 0) {
        const SphParams& p = c->p;
        LoadArgs a;
        a.grid_size = p.grid_size; a.inv_h = 1.0f / p.support_radius; a.h = p.support_radius; a.k_dw = p.k_dw; a.rho0 = p.density_0;
        for (int k = 0; k < 3; ++k) { a.about[k] = s->about[k]; a.n[k] = p.grid_num[k]; }
        a.N = in.N; a.n_objects = s->n_objects; a.list_cap = (int)s->list_cap;
        for (int k = 0; k < 32; ++k) a.object_ids[k] = s->sel.object_ids[k];
        int* count = s->list + s->list_cap;
        SPH_HIP(c, hipMemsetAsync(count, 0, sizeof(int), c->stream));
        const SphWalk w = sph_observe_walk(in.N, LD_TPB, LD_SELECT_MAX_BLOCKS);
        hipLaunchKernelGGL(k_loads_select, dim3(w.blocks), dim3(LD_TPB), 0, c->stream, in.vf, a, w.per_block, s->list, count);
        SPH_LAUNCH_CHECK(c);
        long long* row = s->hist + (size_t)s->samples * (size_t)s->n_objects * LD_WORDS;
        hipLaunchKernelGGL(k_loads_gather, dim3(s->gather_blocks), dim3(LD_TPB), 0, c->stream, in.xm, in.vf, in.aux, (const int*)c->cell_end,
                           (const int*)s->list, (const int*)count, a, row);
        SPH_LAUNCH_CHECK(c);
    }
    s->times[s->samples] = t;
    s->samples += 1;
    return 0;
}

// step_sweeps' hook behind the step's density and pressure: x(t_k), this step's sort, this step's p and rho -- the values the force
// sweep uses next.  Nothing when no set is registered.
int sph_loads_step(SphContext* c) {
    SphLoadSet* s = c->loads;
    if (!s || !s->have) return 0;
    const bool due = s->steps_seen % s->every == 0;
    s->steps_seen += 1;
    return due ? loads_take(c, s, c->sim_time) : 0;
}

static int loads_fail(SphContext* c, int rc, const char* who, const char* what) {
    snprintf(c->err, sizeof(c->err), "%s: %s", who, what);
    return rc;
}

static const char* const LD_WHY_SLAB = " (a solid's fluid neighbours beyond the halo belong to another rank); loads exist on single-domain contexts only";
static const char* const LD_NO_SET = "no load set is registered (call sph_loads_set first)";

static void loads_zero_counters(SphLoadSet* s) { s->samples = s->dropped = s->steps_seen = 0; }

// the history to zero, behind whatever the stream holds; synchronises
static int loads_clear(SphContext* c, SphLoadSet* s) {
    SPH_HIP(c, hipMemsetAsync(s->hist, 0, (size_t)s->capacity * (size_t)s->n_objects * LD_WORDS * 8, c->stream));
    SPH_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" {

int32_t sph_loads_set(SphContext* c, const SphLoadParams* lp) {
    const char* who = "sph_loads_set";
    if (int rc = sph_observe_enter(c, who, LD_WHY_SLAB)) return rc;
    if (!lp) {   // clears the set; the buffers stay for the next one
        if (c->loads) { c->loads->have = false; loads_zero_counters(c->loads); }
        return 0;
    }
    if (lp->n_objects < 1 || lp->n_objects > SPH_LOADS_MAX_OBJECTS) {
        snprintf(c->err, sizeof(c->err), "%s: n_objects = %d, must be in [1, SPH_LOADS_MAX_OBJECTS = %d]", who, lp->n_objects, SPH_LOADS_MAX_OBJECTS);
        return SPH_E_INVALID;
    }
    for (int k = 0; k < lp->n_objects; ++k) {
        if (lp->object_ids[k] < 0 || lp->object_ids[k] >= c->p.n_objects) {
            snprintf(c->err, sizeof(c->err), "%s: object id %d is outside [0, n_objects = %d)", who, lp->object_ids[k], c->p.n_objects);
            return SPH_E_INVALID;
        }
        for (int l = 0; l < k; ++l)
            if (lp->object_ids[l] == lp->object_ids[k]) {
                snprintf(c->err, sizeof(c->err), "%s: duplicate object id %d", who, lp->object_ids[k]);
                return SPH_E_INVALID;
            }
    }
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(lp->about[a])) return loads_fail(c, SPH_E_INVALID, who, "about is not finite");
    if (lp->every < 1) return loads_fail(c, SPH_E_INVALID, who, "every must be at least 1");
    const unsigned long long hist_bytes = (unsigned long long)(lp->capacity > 0 ? lp->capacity : 0) * (unsigned long long)lp->n_objects * LD_WORDS * 8ull;
    if (lp->capacity < 1 || hist_bytes > LD_MAX_HISTORY_BYTES) {
        snprintf(c->err, sizeof(c->err), "%s: capacity = %d, must be at least 1 and the history (%llu bytes) at most 2^31 bytes", who, lp->capacity, hist_bytes);
        return SPH_E_INVALID;
    }
    SphSel sel;
    sph_sel_make(SPH_MATERIAL_SOLID, lp->n_objects, lp->object_ids, false, &sel);
    if (!sph_observe_state(c->loads)) return loads_fail(c, SPH_E_NOMEM, who, "out of host memory");
    SphLoadSet* s = c->loads;
    // whatever has to grow exists before anything old goes: a failure leaves the last good set as it was
    void *nl = nullptr, *nh = nullptr;
    double* nt = nullptr;
    const size_t list_cap = (size_t)(c->cap > 0 ? c->cap : 1), words = (size_t)(hist_bytes / 8);
    if ((size_t)lp->capacity > s->times_cap) {
        nt = (double*)malloc((size_t)lp->capacity * sizeof(double));
        if (!nt) return loads_fail(c, SPH_E_NOMEM, who, "out of host memory");
    }
    if (list_cap > s->list_cap)
        if (int rc = sph_observe_alloc(c, &nl, (list_cap + 1) * sizeof(int), who, "the target list")) { free(nt); return rc; }
    if (words > s->hist_words)
        if (int rc = sph_observe_alloc(c, &nh, words * 8, who, "the load history")) { if (nl) (void)hipFree(nl); free(nt); return rc; }
    if (nl || nh) SPH_HIP(c, hipStreamSynchronize(c->stream));   // (a sample may still be writing the old ones)
    if (nt) { free(s->times); s->times = nt; s->times_cap = (size_t)lp->capacity; }
    if (nl) { (void)hipFree(s->list); s->list = (int*)nl; s->list_cap = list_cap; }
    if (nh) { (void)hipFree(s->hist); s->hist = (long long*)nh; s->hist_words = words; }
    s->n_objects = lp->n_objects; s->every = lp->every; s->capacity = lp->capacity;
    s->sel = sel;
    for (int a = 0; a < 3; ++a) s->about[a] = lp->about[a];
    long long blocks = ((long long)s->list_cap + LD_PER_BLOCK - 1) / LD_PER_BLOCK;
    if (blocks > LD_GATHER_MAX_BLOCKS) blocks = LD_GATHER_MAX_BLOCKS;
    if (const char* e = getenv("SPH_LOADS_BLOCKS")) {   // test aid: a small grid makes the waves take several trips over a short list
        const long long b = atoll(e);
        if (b >= 1 && b < blocks) blocks = b;
    }
    s->gather_blocks = (int)blocks;
    loads_zero_counters(s);
    s->have = true;
    return loads_clear(c, s);
}

int32_t sph_loads_sample(SphContext* c) {
    const char* who = "sph_loads_sample";
    if (int rc = sph_observe_enter(c, who, LD_WHY_SLAB)) return rc;
    SphLoadSet* s = c->loads;
    if (!s || !s->have) return loads_fail(c, SPH_E_STATE, who, LD_NO_SET);
    if (!sphs_neighbours_ready(c->ss)) return loads_fail(c, SPH_E_STATE, who, "needs the neighbour structure: call sph_initialize_particle_system first");
    return loads_take(c, s, c->sim_time);
}

int32_t sph_loads_info(SphContext* c, SphLoadInfo* out) {
    if (!c) return SPH_E_INVALID;
    if (!out) return sph_fail(c, SPH_E_INVALID, "sph_loads_info: the result is NULL");
    const SphLoadSet* s = c->loads;
    const bool have = s && s->have;
    out->n_objects = have ? s->n_objects : 0;
    out->every = have ? s->every : 0;
    out->samples = have ? s->samples : 0;
    out->dropped = have ? s->dropped : 0;
    out->steps_seen = have ? s->steps_seen : 0;
    return 0;
}

int32_t sph_loads_download(SphContext* c, int64_t* rows, double* times, int64_t samples, int32_t n_objects) {
    const char* who = "sph_loads_download";
    if (int rc = sph_observe_enter(c, who, LD_WHY_SLAB)) return rc;
    const SphLoadSet* s = c->loads;
    if (!s || !s->have) return loads_fail(c, SPH_E_STATE, who, LD_NO_SET);
    if (samples != s->samples || n_objects != s->n_objects) {
        snprintf(c->err, sizeof(c->err), "%s: samples = %lld, n_objects = %d; the set holds %lld samples of %d objects", who, (long long)samples,
                 n_objects, s->samples, s->n_objects);
        return SPH_E_INVALID;
    }
    if (times) memcpy(times, s->times, (size_t)samples * sizeof(double));
    const size_t bytes = (size_t)samples * (size_t)n_objects * LD_WORDS * 8;
    return sph_observe_download(c, bytes ? rows : nullptr, s->hist, bytes);
}

int32_t sph_loads_reset(SphContext* c) {
    const char* who = "sph_loads_reset";
    if (int rc = sph_observe_enter(c, who, LD_WHY_SLAB)) return rc;
    SphLoadSet* s = c->loads;
    if (!s || !s->have) return loads_fail(c, SPH_E_STATE, who, LD_NO_SET);
    loads_zero_counters(s);
    return loads_clear(c, s);
}

}  // extern "C"
