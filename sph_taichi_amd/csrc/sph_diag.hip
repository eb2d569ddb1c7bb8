// sph_diag.hip -- flow diagnostics (include/sph_hip.h, last section): one streaming reduction over the live records, per
// object id and over all particles, behind whatever the stream holds.  Reads xm / vf / aux / acc (64 B per particle, four
// 16-byte loads), writes n_objects + 1 rows.  Touches nothing of the sort or the sweeps and writes no particle state.
//
// Determinism (the fixed-order scheme, no atomics anywhere):
//   lane   : every lane adds the particles of its grid-stride walk that share one row into private accumulators;
//   wave   : when a lane meets another row (or at the end) the WAVE flushes: per distinct row present in the wave (ballot on
//            the first holding lane's row, the lanes that match reduced by an xor butterfly, the others giving the
//            operation's identity) lane 0 adds the result to the wave's own row table in LDS;
//   block  : the four wave tables are added in wave order, the block's rows in row order give the block's total;
//   grid   : k_diag_finish adds the block partials of a row: thread t takes blocks t, t + 256, ... in that order, a
//            butterfly per wave, the four waves in wave order.
// Every grouping is a function of N, the launch shape and the particle order alone: two calls on one state give the same bits.
// Sums are f64 (m x is exact in f64: two 24-bit significands); extrema are order-free.
#include "sph_observe.h"

#define DTPB SPH_DIAG_THREADS
#define DWAVES (SPH_DIAG_THREADS / 64)

struct SphDiag {
    SphDiagRow* part;   // [SPH_DIAG_BLOCKS][n_objects + 2] per-block rows: objects, "no such object", block total
    SphDiagRow* out;    // [n_objects + 1] what sph_diag_download copies
    bool have;          // a reduction has been enqueued
};

// a row under accumulation: the members of SphDiagRow with the identities of their operations (extrema: +-inf; the maxima of
// squares: 0).  The zeros the header promises for empty rows are written once, by k_diag_finish.
__device__ __forceinline__ void row_identity(SphDiagRow& r) {
    r.count = r.fluid_count = r.moving_count = 0;
    r.mass = 0.0; r.kinetic = 0.0; r.v2_max = 0.0; r.a2_max = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { r.mx[a] = 0.0; r.momentum[a] = 0.0; r.lo[a] = INFINITY; r.hi[a] = -INFINITY; }
    r.density_min = r.pressure_min = INFINITY;
    r.density_max = r.pressure_max = -INFINITY;
}

__device__ __forceinline__ void row_combine(SphDiagRow& r, const SphDiagRow& s) {
    r.count += s.count; r.fluid_count += s.fluid_count; r.moving_count += s.moving_count;
    r.mass += s.mass; r.kinetic += s.kinetic;
    r.v2_max = fmax(r.v2_max, s.v2_max); r.a2_max = fmax(r.a2_max, s.a2_max);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.mx[a] += s.mx[a]; r.momentum[a] += s.momentum[a];
        r.lo[a] = fminf(r.lo[a], s.lo[a]); r.hi[a] = fmaxf(r.hi[a], s.hi[a]);
    }
    r.density_min = fminf(r.density_min, s.density_min); r.density_max = fmaxf(r.density_max, s.density_max);
    r.pressure_min = fminf(r.pressure_min, s.pressure_min); r.pressure_max = fmaxf(r.pressure_max, s.pressure_max);
}

// all 64 lanes active; afterwards every lane holds the wave's row (both partners of a step compute the same a + b)
__device__ __forceinline__ void row_wave_reduce(SphDiagRow& r) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        SphDiagRow s;
        s.count = shfl_xor_i64(r.count, m); s.fluid_count = shfl_xor_i64(r.fluid_count, m); s.moving_count = shfl_xor_i64(r.moving_count, m);
        s.mass = __shfl_xor(r.mass, m, 64); s.kinetic = __shfl_xor(r.kinetic, m, 64);
        s.v2_max = __shfl_xor(r.v2_max, m, 64); s.a2_max = __shfl_xor(r.a2_max, m, 64);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s.mx[a] = __shfl_xor(r.mx[a], m, 64); s.momentum[a] = __shfl_xor(r.momentum[a], m, 64);
            s.lo[a] = __shfl_xor(r.lo[a], m, 64); s.hi[a] = __shfl_xor(r.hi[a], m, 64);
        }
        s.density_min = __shfl_xor(r.density_min, m, 64); s.density_max = __shfl_xor(r.density_max, m, 64);
        s.pressure_min = __shfl_xor(r.pressure_min, m, 64); s.pressure_max = __shfl_xor(r.pressure_max, m, 64);
        row_combine(r, s);
    }
}

// The wave's pending lane accumulators into its LDS table, one reduction per distinct row present (cell-sorted records: one
// or two).  `row` < 0: the lane holds nothing.  Called by all 64 lanes; leaves every lane empty.
__device__ __forceinline__ void wave_flush(SphDiagRow* table, SphDiagRow& mine, int& row, int lane) {
    unsigned long long todo = __ballot(row >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int r = __shfl(row, leader, 64);            // wave-uniform: rows are in [0, n_rows) by construction
        const bool in = row == r;
        SphDiagRow s;
        if (in) s = mine; else row_identity(s);
        row_wave_reduce(s);
        if (lane == 0) {
            SphDiagRow t = table[r];
            row_combine(t, s);
            table[r] = t;
        }
        todo &= ~__ballot(in);
    }
    row_identity(mine);
    row = -1;
}

// grid = min(ceil(N / 256), SPH_DIAG_BLOCKS) blocks of four waves; dynamic LDS = DWAVES * (n_objects + 1) rows
__global__ __launch_bounds__(DTPB) void k_diag_reduce(const float4* __restrict__ xm, const float4* __restrict__ vf,
                                                      const float4* __restrict__ aux, const float4* __restrict__ acc, int N,
                                                      int n_objects, SphDiagRow* __restrict__ part) {
    extern __shared__ __align__(16) unsigned char diag_lds[];
    SphDiagRow* tables = reinterpret_cast<SphDiagRow*>(diag_lds);
    const int n_rows = n_objects + 1;                      // the last one: particles whose object id names no object
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < DWAVES * n_rows; k += DTPB) row_identity(tables[k]);
    __syncthreads();
    SphDiagRow* table = tables + wave * n_rows;

    SphDiagRow mine;
    row_identity(mine);
    int row = -1;
    const long long stride = (long long)gridDim.x * DTPB;
    // `base` is the wave's first index: wave-uniform, so all 64 lanes make every trip (the ballots and shuffles need them)
    for (long long base = (long long)blockIdx.x * DTPB + wave * 64; base < N; base += stride) {
        const long long i = base + lane;
        const bool valid = i < N;
        float4 X = make_float4(0.f, 0.f, 0.f, 0.f), V = X, A = X, Q = X;
        if (valid) { X = xm[i]; V = vf[i]; Q = aux[i]; A = acc[i]; }
        const int fl = __float_as_int(V.w);
        const unsigned obj = (unsigned)sph_flags_object(fl);
        const int r = valid ? (obj < (unsigned)n_objects ? (int)obj : n_objects) : row;
        if (__any(row >= 0 && r != row)) wave_flush(table, mine, row, lane);
        if (valid) {
            row = r;
            const bool fluid = sph_is_fluid(fl);
            const bool moving = fluid || sph_flags_dynamic(fl);
            const double m = (double)Q.x;
            const double vx = (double)V.x, vy = (double)V.y, vz = (double)V.z;
            const double v2 = vx * vx + vy * vy + vz * vz;
            mine.count += 1; mine.fluid_count += fluid ? 1 : 0; mine.moving_count += moving ? 1 : 0;
            mine.mass += m;
            mine.mx[0] += m * (double)X.x; mine.mx[1] += m * (double)X.y; mine.mx[2] += m * (double)X.z;
            mine.momentum[0] += m * vx; mine.momentum[1] += m * vy; mine.momentum[2] += m * vz;
            mine.kinetic += 0.5 * m * v2;
            mine.v2_max = fmax(mine.v2_max, v2);
            if (moving) {
                const double ax = (double)A.x, ay = (double)A.y, az = (double)A.z;
                mine.a2_max = fmax(mine.a2_max, ax * ax + ay * ay + az * az);
            }
            if (fluid) {
                mine.density_min = fminf(mine.density_min, Q.y); mine.density_max = fmaxf(mine.density_max, Q.y);
                mine.pressure_min = fminf(mine.pressure_min, Q.z); mine.pressure_max = fmaxf(mine.pressure_max, Q.z);
            }
            mine.lo[0] = fminf(mine.lo[0], X.x); mine.lo[1] = fminf(mine.lo[1], X.y); mine.lo[2] = fminf(mine.lo[2], X.z);
            mine.hi[0] = fmaxf(mine.hi[0], X.x); mine.hi[1] = fmaxf(mine.hi[1], X.y); mine.hi[2] = fmaxf(mine.hi[2], X.z);
        }
    }
    wave_flush(table, mine, row, lane);
    __syncthreads();
    // the block's rows: wave tables in wave order (n_rows <= SPH_DIAG_MAX_OBJECTS + 1 < 256 threads)
    SphDiagRow* mine_out = part + (size_t)blockIdx.x * (n_rows + 1);
    if ((int)threadIdx.x < n_rows) {
        SphDiagRow t = tables[threadIdx.x];
#pragma unroll
        for (int w = 1; w < DWAVES; ++w) row_combine(t, tables[w * n_rows + threadIdx.x]);
        tables[threadIdx.x] = t;
        mine_out[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // the block's total: its rows in row order
        SphDiagRow t = tables[0];
        for (int k = 1; k < n_rows; ++k) row_combine(t, tables[k]);
        mine_out[n_rows] = t;
    }
}

// grid = n_objects + 1: block b < n_objects adds the blocks' rows b, block n_objects their totals
__global__ __launch_bounds__(DTPB) void k_diag_finish(const SphDiagRow* __restrict__ part, int n_blocks, int n_objects,
                                                      SphDiagRow* __restrict__ out) {
    __shared__ SphDiagRow waves[DWAVES];
    const int src = (int)blockIdx.x < n_objects ? (int)blockIdx.x : n_objects + 1;
    const int per_block = n_objects + 2;
    SphDiagRow t;
    row_identity(t);
    for (int k = threadIdx.x; k < n_blocks; k += DTPB) row_combine(t, part[(size_t)k * per_block + src]);
    row_wave_reduce(t);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < DWAVES; ++w) row_combine(t, waves[w]);
        if (t.count == 0) for (int a = 0; a < 3; ++a) { t.lo[a] = 0.f; t.hi[a] = 0.f; }
        if (t.fluid_count == 0) t.density_min = t.density_max = t.pressure_min = t.pressure_max = 0.f;
        out[blockIdx.x] = t;
    }
}

void sph_diag_release(SphContext* c) { sph_observe_release(c->diag, &SphDiag::part, &SphDiag::out); }

// the state struct and its rows (n_objects is fixed for the life of a context (sph_set_params): allocated once)
static int diag_state(SphContext* c) {
    SphDiag* g = sph_observe_state(c->diag);
    if (!g) return sph_fail(c, SPH_E_NOMEM, "sph_diag_reduce: out of host memory");
    const size_t rows = (size_t)c->p.n_objects + 2;
    if (!g->part)
        if (int rc = sph_observe_alloc(c, (void**)&g->part, (size_t)SPH_DIAG_BLOCKS * rows * sizeof(SphDiagRow), "sph_diag_reduce", "the partial rows")) return rc;
    if (!g->out)
        if (int rc = sph_observe_alloc(c, (void**)&g->out, rows * sizeof(SphDiagRow), "sph_diag_reduce", "the result rows")) return rc;
    return 0;
}

extern "C" {

int32_t sph_diag_reduce(SphContext* c) {
    if (int rc = sph_observe_enter(c, "sph_diag_reduce", " (its ghost records would be counted twice); diagnostics are reduced on single-domain contexts only")) return rc;
    if (c->p.n_objects > SPH_DIAG_MAX_OBJECTS) {
        snprintf(c->err, sizeof(c->err), "sph_diag_reduce: %d objects, the per-block row table holds %d", c->p.n_objects, SPH_DIAG_MAX_OBJECTS);
        return SPH_E_INVALID;
    }
    if (!sphs_acc_complete(c->ss)) return sph_fail(c, SPH_E_STATE, "sph_diag_reduce: the last sph_slab_forces did not write every acceleration out (see sph_download)");
    if (int rc = diag_state(c)) return rc;
    if (int rc = sph_ensure_aux(c)) return rc;   // density / pressure of a fused step live in eos2 until somebody asks
    const SphLive in = sph_live(c);
    const int n_obj = c->p.n_objects;
    int blocks = (in.N + DTPB - 1) / DTPB;
    if (blocks > SPH_DIAG_BLOCKS) blocks = SPH_DIAG_BLOCKS;
    if (blocks > 0) {
        const size_t lds = (size_t)DWAVES * (n_obj + 1) * sizeof(SphDiagRow);   // <= 4 * 97 * 144 B = 55,872 B
        hipLaunchKernelGGL(k_diag_reduce, dim3(blocks), dim3(DTPB), lds, c->stream, in.xm, in.vf, in.aux, in.acc, in.N, n_obj, c->diag->part);
        SPH_LAUNCH_CHECK(c);
    }
    hipLaunchKernelGGL(k_diag_finish, dim3(n_obj + 1), dim3(DTPB), 0, c->stream, c->diag->part, blocks, n_obj, c->diag->out);
    SPH_LAUNCH_CHECK(c);
    c->diag->have = true;
    return 0;
}

int32_t sph_diag_download(SphContext* c, SphDiagRow* rows, int32_t n_rows) {
    if (!c) return SPH_E_INVALID;
    if (!c->diag || !c->diag->have) return sph_fail(c, SPH_E_STATE, "sph_diag_download: nothing has been reduced (call sph_diag_reduce first)");
    if (!rows || n_rows != c->p.n_objects + 1) return sph_fail(c, SPH_E_INVALID, "sph_diag_download: n_rows must be n_objects + 1 (one row per object, then all particles)");
    return sph_observe_download(c, rows, c->diag->out, (size_t)n_rows * sizeof(SphDiagRow));
}

}  // extern "C"
