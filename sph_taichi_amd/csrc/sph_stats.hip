// sph_stats.hip -- running flow statistics (include/sph_hip.h, "Running flow statistics"): ONE registered grid per context whose
// nodes accumulate, across steps and on the device, how often they were wet and the first and second moments of the Shepard-mean
// velocity there.  The step loops take a sample every `every`-th step behind the step's sort (step_loop, next to the tracer
// advance); sph_stats_sample takes one of the current state outside a step.  Velocity only: density and pressure of a fused step
// lie in eos2 in the PRE-sort order at the hook, and asking for them (sph_ensure_aux) would write particle state and change which
// sort form the next step gets.  A sample reads xm / vf and nothing else; it writes the buffers of this file and nothing else.
//
// One sample is two launches:
//  (a) the sampler's own k_sample_grid (sph_sample_grid_scatter of sph_sample_grid.h: the kernel is not copied), fields vx vy vz, no
//      gradients, into a SCRATCH [5][nodes] i64 of this state: count, weight, S_x, S_y, S_z.  SphSample::grid is not touched: the
//      user's last sph_sample_grid, and a mesh cut from it, survive a run with statistics registered;
//  (b) k_stats_fold: per node, read weight and S_x S_y S_z, ZERO all five scratch words (so the scratch is clear for the next
//      scatter: no clear pass per sample, only registration and reset clear), and where the node is wet fold the sample into the
//      accumulators [11][nodes] i64: n_wet, sum_w, sum_u[3], sum_uu[6] (xx xy xz yy yz zz).
// The fold of a wet node (weight >= wet_min && weight > 0), f64, nothing contracted:
//     u_a = (double)S_a / (double)weight      (i64 -> f64 correctly rounded; the IEEE divide);   u_a = fmin(fmax(u_a, -1024), 1024)
//     n_wet += 1;  sum_w += weight;  sum_u[a] += llrint(u_a * 2^32);  sum_uu[ab] += llrint((u_a * u_b) * 2^24)
// (u_a * 2^32 and the scaling by 2^24 are exact; the product u_a * u_b rounds once.)  A node that is not wet adds nothing and its
// division is not evaluated: no NaN of a 0 / 0 ever reaches an llrint.
// BOUND: |u_a| <= 2^10, so a first-moment term is at most 2^42 and a second-moment term at most 2^44 in magnitude (equality only AT
// the clamp, 1024 length units per time unit); 2^19 samples of terms below that stay within an i64: SPH_STATS_MAX_SAMPLES = 1 << 19.
// sum_w: a weight stays below 2^41 (sph_hip.h, "Field sampling"), 2^19 of them below 2^60.
// Every node has ONE owner lane: the fold has no atomics, and there is no float or double atomic anywhere.
//
// k_stats_fold, gfx950: streaming and coalesced, a grid-stride loop over lane-groups of V consecutive nodes.  Per wet node it reads
// 32 B of scratch (the count word is zeroed unread), writes 40 B and read-modify-writes 88 B.  When `nodes` is even every plane
// starts on a 16-byte boundary (the allocation is 256-byte aligned, a plane is 8 * nodes bytes), and the V = 2 instance moves
// each lane's two nodes of a plane as one 16-byte access (global_load / store_dwordx4, 1 KiB per wave-instruction); an odd node
// count takes the V = 1 instance with 8-byte accesses.  A lane whose nodes are all dry touches the scratch only.  Registers, scratch
// and occupancy: profiles/stats_kernel_resources.txt; measured cost: profiles/stats_timing.json.
#include <cmath>
#include "sph_observe.h"
#include "sph_sample_grid.h"
#include "sph_sample_pair.h"

#pragma clang fp contract(off)

#define SF_TPB 256
#define SF_MAX_BLOCKS 2048
#define SF_SCRATCH_PLANES 5
#define SF_ACC_PLANES 11
#define SF_U_LIMIT 1024.0

struct SphStatsSet {
    long long* buf;           // one allocation: scratch [5][nodes], then acc [11][nodes], both with the CURRENT set's node count
    size_t cap_words;         // allocated
    bool have;                // a set is registered
    SampleCommon q;
    SampleGridDev g;          // g.planes = the scratch
    int every, capacity;
    long long wet_min;
    long long samples, dropped, steps_seen;
    double t_first, t_last;
};

static inline long long* stats_acc(const SphStatsSet* s) { return s->buf + (size_t)SF_SCRATCH_PLANES * (size_t)s->g.nodes; }

template <int V> struct SfVec;
template <> struct SfVec<1> { long long v[1]; };
template <> struct alignas(16) SfVec<2> { long long v[2]; };

// V nodes per lane; nodes % V == 0 and every plane aligned to 8 V bytes (the host picks the instance)
template <int V>
__global__ __launch_bounds__(SF_TPB) void k_stats_fold(long long* __restrict__ scratch, long long* __restrict__ acc, long long nodes,
                                                       long long wet_min) {
    typedef SfVec<V> Vec;
    const size_t stride = (size_t)nodes;
    const long long groups = nodes / V;
    for (long long gi = (long long)blockIdx.x * SF_TPB + threadIdx.x; gi < groups; gi += (long long)gridDim.x * SF_TPB) {
        const size_t i = (size_t)gi * V;
        Vec S[SF_SCRATCH_PLANES - 1];   // weight, S_x, S_y, S_z
#pragma unroll
        for (int p = 1; p < SF_SCRATCH_PLANES; ++p) S[p - 1] = *reinterpret_cast<const Vec*>(scratch + (size_t)p * stride + i);
        Vec zero;
#pragma unroll
        for (int k = 0; k < V; ++k) zero.v[k] = 0;
#pragma unroll
        for (int p = 0; p < SF_SCRATCH_PLANES; ++p) *reinterpret_cast<Vec*>(scratch + (size_t)p * stride + i) = zero;
        Vec T[SF_ACC_PLANES];
        bool any = false;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const long long w = S[0].v[k];
            const bool wet = w >= wet_min && w > 0;
            any = any || wet;
#pragma unroll
            for (int p = 0; p < SF_ACC_PLANES; ++p) T[p].v[k] = 0;
            if (wet) {
                const double W = (double)w;
                double u[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) u[a] = fmin(fmax((double)S[1 + a].v[k] / W, -SF_U_LIMIT), SF_U_LIMIT);
                T[0].v[k] = 1;
                T[1].v[k] = w;
#pragma unroll
                for (int a = 0; a < 3; ++a) T[2 + a].v[k] = llrint(u[a] * 4294967296.0);
                int p = 5;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = a; b < 3; ++b) T[p++].v[k] = llrint((u[a] * u[b]) * 16777216.0);
            }
        }
        if (!any) continue;
        Vec A[SF_ACC_PLANES];
#pragma unroll
        for (int p = 0; p < SF_ACC_PLANES; ++p) A[p] = *reinterpret_cast<const Vec*>(acc + (size_t)p * stride + i);
#pragma unroll
        for (int p = 0; p < SF_ACC_PLANES; ++p) {
#pragma unroll
            for (int k = 0; k < V; ++k) A[p].v[k] += T[p].v[k];
            *reinterpret_cast<Vec*>(acc + (size_t)p * stride + i) = A[p];
        }
    }
}

void sph_stats_release(SphContext* c) { sph_observe_release(c->stats_set, &SphStatsSet::buf); }

// ONE sample of the current records at simulated time t: the scatter, then the fold; a full set counts it as dropped and enqueues nothing
static int stats_take(SphContext* c, SphStatsSet* s, double t) {
    if (s->samples >= s->capacity) { s->dropped += 1; return 0; }
    if (int rc = sph_sample_grid_scatter(c, s->q, s->g)) return rc;
    const long long nodes = s->g.nodes;
    const int V = (nodes & 1) ? 1 : 2;
    const long long groups = nodes / V;
    long long blocks = (groups + SF_TPB - 1) / SF_TPB;
    if (blocks > SF_MAX_BLOCKS) blocks = SF_MAX_BLOCKS;
    if (V == 2) hipLaunchKernelGGL(k_stats_fold<2>, dim3((unsigned)blocks), dim3(SF_TPB), 0, c->stream, s->buf, stats_acc(s), nodes, s->wet_min);
    else hipLaunchKernelGGL(k_stats_fold<1>, dim3((unsigned)blocks), dim3(SF_TPB), 0, c->stream, s->buf, stats_acc(s), nodes, s->wet_min);
    SPH_LAUNCH_CHECK(c);
    if (s->samples == 0) s->t_first = t;
    s->t_last = t;
    s->samples += 1;
    return 0;
}

// step_loop's hook behind the head-of-step sort: the records are x(t_k), v(t_k) at sim_time.  Nothing when no set is registered.
int sph_stats_step(SphContext* c) {
    SphStatsSet* s = c->stats_set;
    if (!s || !s->have) return 0;
    const bool due = s->steps_seen % s->every == 0;
    s->steps_seen += 1;
    return due ? stats_take(c, s, c->sim_time) : 0;
}

static int stats_fail(SphContext* c, int rc, const char* who, const char* what) {
    snprintf(c->err, sizeof(c->err), "%s: %s", who, what);
    return rc;
}

static const char* const ST_WHY_SLAB = " (its ghost records would be counted twice); statistics exist on single-domain contexts only";
static const char* const ST_NO_SET = "no statistics set is registered (call sph_stats_set first)";

static void stats_zero_counters(SphStatsSet* s) {
    s->samples = s->dropped = s->steps_seen = 0;
    s->t_first = s->t_last = 0.0;
}

// scratch and accumulators to zero, behind whatever the stream holds; synchronises
static int stats_clear(SphContext* c, SphStatsSet* s) {
    SPH_HIP(c, hipMemsetAsync(s->buf, 0, (size_t)(SF_SCRATCH_PLANES + SF_ACC_PLANES) * (size_t)s->g.nodes * 8, c->stream));
    SPH_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" {

int32_t sph_stats_set(SphContext* c, const SphStatsParams* sp) {
    const char* who = "sph_stats_set";
    if (int rc = sph_observe_enter(c, who, ST_WHY_SLAB)) return rc;
    if (!sp) {   // clears the set; the buffers stay for the next one
        if (c->stats_set) { c->stats_set->have = false; stats_zero_counters(c->stats_set); }
        return 0;
    }
    if (sp->grid.fields != 0 && sp->grid.fields != (SPH_SAMPLE_VX | SPH_SAMPLE_VY | SPH_SAMPLE_VZ)) {
        snprintf(c->err, sizeof(c->err), "%s: grid.fields = %d, must be 0 or SPH_SAMPLE_VX | SPH_SAMPLE_VY | SPH_SAMPLE_VZ (the statistics are of the "
                 "velocity only: density and pressure are not in the sorted order at the step's hook)", who, sp->grid.fields);
        return SPH_E_INVALID;
    }
    if (sp->every < 1) return stats_fail(c, SPH_E_INVALID, who, "every must be at least 1");
    if (sp->capacity < 1 || sp->capacity > SPH_STATS_MAX_SAMPLES) {
        snprintf(c->err, sizeof(c->err), "%s: capacity = %d, must be in [1, SPH_STATS_MAX_SAMPLES = %d]", who, sp->capacity, SPH_STATS_MAX_SAMPLES);
        return SPH_E_INVALID;
    }
    if (sp->wet_min < 0) return stats_fail(c, SPH_E_INVALID, who, "wet_min must not be negative");
    SphSampleGrid grid = sp->grid;
    grid.fields = SPH_SAMPLE_VX | SPH_SAMPLE_VY | SPH_SAMPLE_VZ;
    SampleCommon q;
    SampleGridDev g;
    if (int rc = sph_sample_grid_spec(c, who, &grid, &q, &g)) return rc;
    if (!sph_observe_state(c->stats_set)) return stats_fail(c, SPH_E_NOMEM, who, "out of host memory");
    SphStatsSet* s = c->stats_set;
    const size_t words = (size_t)(SF_SCRATCH_PLANES + SF_ACC_PLANES) * (size_t)g.nodes;
    if (words > s->cap_words) {   // the larger planes exist before the old ones go: a failure leaves the old set as it was
        void* nb = nullptr;
        if (int rc = sph_observe_alloc(c, &nb, words * 8, who, "the statistics planes")) return rc;
        SPH_HIP(c, hipStreamSynchronize(c->stream));   // (a sample may still be writing the old ones)
        (void)hipFree(s->buf);
        s->buf = (long long*)nb;
        s->cap_words = words;
    }
    s->q = q;
    s->g = g;
    s->g.planes = s->buf;
    s->every = sp->every; s->capacity = sp->capacity;
    s->wet_min = sp->wet_min;
    stats_zero_counters(s);
    s->have = true;
    return stats_clear(c, s);
}

int32_t sph_stats_sample(SphContext* c) {
    const char* who = "sph_stats_sample";
    if (int rc = sph_observe_enter(c, who, ST_WHY_SLAB)) return rc;
    SphStatsSet* s = c->stats_set;
    if (!s || !s->have) return stats_fail(c, SPH_E_STATE, who, ST_NO_SET);
    return stats_take(c, s, c->sim_time);
}

int32_t sph_stats_info(SphContext* c, SphStatsInfo* out) {
    if (!c) return SPH_E_INVALID;
    if (!out) return sph_fail(c, SPH_E_INVALID, "sph_stats_info: the result is NULL");
    const SphStatsSet* s = c->stats_set;
    const bool have = s && s->have;
    out->nodes = have ? s->g.nodes : 0;
    for (int a = 0; a < 3; ++a) out->n[a] = have ? s->g.n[a] : 0;
    out->every = have ? s->every : 0;
    out->samples = have ? s->samples : 0;
    out->dropped = have ? s->dropped : 0;
    out->steps_seen = have ? s->steps_seen : 0;
    out->t_first = have ? s->t_first : 0.0;
    out->t_last = have ? s->t_last : 0.0;
    return 0;
}

int32_t sph_stats_download(SphContext* c, int64_t* n_wet, int64_t* sum_w, int64_t* sum_u, int64_t* sum_uu, int64_t nodes) {
    const char* who = "sph_stats_download";
    if (int rc = sph_observe_enter(c, who, ST_WHY_SLAB)) return rc;
    const SphStatsSet* s = c->stats_set;
    if (!s || !s->have) return stats_fail(c, SPH_E_STATE, who, ST_NO_SET);
    if (nodes != s->g.nodes) {
        snprintf(c->err, sizeof(c->err), "%s: nodes = %lld, the registered grid has %lld nodes", who, (long long)nodes, s->g.nodes);
        return SPH_E_INVALID;
    }
    const size_t n = (size_t)nodes;
    const long long* acc = stats_acc(s);
    if (n_wet) SPH_HIP(c, hipMemcpyAsync(n_wet, acc, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (sum_w) SPH_HIP(c, hipMemcpyAsync(sum_w, acc + n, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (sum_u) SPH_HIP(c, hipMemcpyAsync(sum_u, acc + 2 * n, 3 * n * 8, hipMemcpyDeviceToHost, c->stream));
    if (sum_uu) SPH_HIP(c, hipMemcpyAsync(sum_uu, acc + 5 * n, 6 * n * 8, hipMemcpyDeviceToHost, c->stream));
    return sph_observe_download(c, nullptr, nullptr, 0);
}

int32_t sph_stats_reset(SphContext* c) {
    const char* who = "sph_stats_reset";
    if (int rc = sph_observe_enter(c, who, ST_WHY_SLAB)) return rc;
    SphStatsSet* s = c->stats_set;
    if (!s || !s->have) return stats_fail(c, SPH_E_STATE, who, ST_NO_SET);
    stats_zero_counters(s);
    return stats_clear(c, s);
}

}  // extern "C"
