// sph_columns.hip -- depth-integrated column maps (include/sph_hip.h, "Depth-integrated column maps"): one streaming pass over the live records
// that bins every selected fluid particle into the column of a 2-D map it stands in.  Reads xm / vf (32 B per particle, two
// 16-byte loads), writes the map's planes.  Touches nothing of the sort or the sweeps and writes no particle state.
//
// Arithmetic per selected particle (f32, in this order, nothing contracted; ja < jb are the two axes other than `axis`):
//     f_j = floorf((x_j - origin_j) * inv_cell_j)          one subtract, one multiply, floorf
//     inside  <=>  0 <= f_j < n_j for both j  (the comparison is made on the float, so a NaN is outside); k_j = (int)f_j
//     column = k_a * n[1] + k_b
//     count += 1;  sum_v[a] += llrint((double)fmaxf(fminf(v_a, 65536.f), -65536.f) * 2^20);  top / bottom = max / min of x[axis]
// Determinism: every accumulation is an INTEGER sum, maximum or minimum (the extrema travel as the order-preserving u32 image of
// their f32 bits, on chip as well as in HBM), so the result is the same bits for any particle order, grouping and scheduling.
// There is no float or double atomic anywhere.
//
// On-chip combining (what reaches HBM is a small fraction of five atomics per particle):
//   wave   : the 64 records a wave holds are consecutive; runs of equal column are reduced by a segmented inclusive scan (head
//            flags from a ballot, six shuffle steps), the last lane of a run holds the run's total;
//   block  : a run's total goes into a direct-mapped LDS table of CT_SLOTS columns (slot = column mod CT_SLOTS, claimed with a
//            compare-and-swap on the slot's key) by LDS atomics; a run whose slot belongs to another column goes straight to
//            the global planes.  A block works through a CONTIGUOUS range of records, so in cell order (x slowest, then y, z)
//            the rows of cells it meets keep returning to the same columns;
//   grid   : at the end the block's claimed slots are added to the planes, one thread per slot: consecutive columns are
//            consecutive addresses of each plane.
// None of this is needed for correctness: unsorted records only make the runs short and the table miss.
#include <cmath>
#include "sph_observe.h"

#pragma clang fp contract(off)

#define CTPB 256
#define CWAVES (CTPB / 64)
#define CT_SLOTS 512
#define CT_MAX_BLOCKS 1024
#define CT_V_LIMIT 65536.f

struct SphColumns {
    // one allocation, planes of `nc` columns each (SoA): count, sum_v[3] (i64), then the three totals, then top, bottom (u32
    // order images under accumulation, f32 after k_columns_finish)
    void* buf;
    long long* count;
    long long* sum_v;     // [3][nc]
    long long* totals;    // selected, binned, outside (+ one word of padding)
    unsigned* top;
    unsigned* bottom;
    int nc;               // columns allocated
    int n[2];             // the last reduce's map
    bool have;
};

// order-preserving image of f32 bits in u32: negative values are flipped whole, the others get the sign bit set
__device__ __forceinline__ unsigned f32_to_ordered(float f) {
    const unsigned b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ordered_to_f32(unsigned u) {
    return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu));
}

struct ColumnTable {
    int key[CT_SLOTS];        // -1 = free
    int count[CT_SLOTS];
    u64 sum_v[3][CT_SLOTS];
    unsigned top[CT_SLOTS], bottom[CT_SLOTS];
    int selected, outside;
};

struct ColumnPlanes {
    long long* count;
    long long* sum_v;
    long long* totals;
    unsigned* top;
    unsigned* bottom;
    int nc;
};

// col in [0, nc) by construction (both k_j were range-checked)
__device__ __forceinline__ void planes_add(const ColumnPlanes& g, int col, long long cnt, const long long s[3], unsigned top, unsigned bottom) {
    atomicAdd((u64*)g.count + col, (u64)cnt);
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd((u64*)g.sum_v + (size_t)a * g.nc + col, (u64)s[a]);
    atomicMax(g.top + col, top);
    atomicMin(g.bottom + col, bottom);
}

__global__ __launch_bounds__(CTPB) void k_columns_clear(ColumnPlanes g) {
    const int c = blockIdx.x * CTPB + threadIdx.x;
    if (c < g.nc) {
        g.count[c] = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) g.sum_v[(size_t)a * g.nc + c] = 0;
        g.top[c] = 0u;                 // below the image of every float
        g.bottom[c] = 0xffffffffu;     // above
    }
    if (c < 4) g.totals[c] = 0;
}

// grid = ceil(tiles / tiles_per_block) blocks of four waves; block b takes the tiles (256 records each) [b, b + 1) * tiles_per_block
__global__ __launch_bounds__(CTPB) void k_columns_scatter(const float4* __restrict__ xm, const float4* __restrict__ vf, int N,
                                                          int tiles_per_block, SphColumnParams p, ColumnPlanes g) {
    __shared__ ColumnTable t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < CT_SLOTS; k += CTPB) {
        t.key[k] = -1; t.count[k] = 0; t.sum_v[0][k] = 0; t.sum_v[1][k] = 0; t.sum_v[2][k] = 0; t.top[k] = 0u; t.bottom[k] = 0xffffffffu;
    }
    if (threadIdx.x == 0) { t.selected = 0; t.outside = 0; }
    __syncthreads();

    const int ja = p.axis == 0 ? 1 : 0, jb = p.axis == 2 ? 1 : 2;
    int n_selected = 0, n_outside = 0;   // wave-uniform
    const long long first = (long long)blockIdx.x * tiles_per_block * CTPB;
    // wave-uniform bounds: all 64 lanes make every trip (the ballots and shuffles need them)
    for (int tile = 0; tile < tiles_per_block; ++tile) {
        const long long base = first + (long long)tile * CTPB + wave * 64;
        if (base >= N) break;
        const long long i = base + lane;
        int key = -1;
        int cnt = 0;
        long long s[3] = {0, 0, 0};
        unsigned top = 0u, bottom = 0xffffffffu;
        bool selected = false, outside = false;
        if (i < N) {
            const float4 X = xm[i], V = vf[i];
            const int fl = __float_as_int(V.w);
            selected = sph_is_fluid(fl) && (p.object_id < 0 || sph_flags_object(fl) == p.object_id);
            if (selected) {
                const float xa = ja == 0 ? X.x : X.y, xb = jb == 2 ? X.z : X.y;            // (selects, not indexed: no scratch)
                const float xu = p.axis == 0 ? X.x : p.axis == 1 ? X.y : X.z;
                const float da = xa - p.origin[0], db = xb - p.origin[1];
                const float fa = floorf(da * p.inv_cell[0]), fb = floorf(db * p.inv_cell[1]);
                if (fa >= 0.f && fa < (float)p.n[0] && fb >= 0.f && fb < (float)p.n[1]) {   // n_j <= 2^20: exact as floats
                    key = (int)fa * p.n[1] + (int)fb;
                    cnt = 1;
                    const float v[3] = {V.x, V.y, V.z};
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                        s[a] = llrint((double)fmaxf(fminf(v[a], CT_V_LIMIT), -CT_V_LIMIT) * (double)(1 << SPH_COLUMNS_V_SCALE_LOG2));
                    top = bottom = f32_to_ordered(xu);
                } else {
                    outside = true;
                }
            }
        }
        n_selected += __popcll(__ballot(selected));
        n_outside += __popcll(__ballot(outside));
        if (!__any(key >= 0)) continue;
        // runs of equal key among consecutive lanes: head flags, then a segmented inclusive scan inside each run
        const int before = __shfl_up(key, 1, 64);
        const u64 heads = __ballot(lane == 0 || key != before);
        const int head = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // lane 0 is always a head
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int c2 = __shfl_up(cnt, off, 64);
            const long long s0 = shfl_up_i64(s[0], off), s1 = shfl_up_i64(s[1], off), s2 = shfl_up_i64(s[2], off);
            const unsigned t2 = (unsigned)__shfl_up((int)top, off, 64), b2 = (unsigned)__shfl_up((int)bottom, off, 64);
            if (lane - off >= head) {
                cnt += c2; s[0] += s0; s[1] += s1; s[2] += s2;
                top = t2 > top ? t2 : top; bottom = b2 < bottom ? b2 : bottom;
            }
        }
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (tail && key >= 0) {
            const int slot = key & (CT_SLOTS - 1);
            const int owner = atomicCAS(&t.key[slot], -1, key);
            if (owner == -1 || owner == key) {
                atomicAdd(&t.count[slot], cnt);
#pragma unroll
                for (int a = 0; a < 3; ++a) atomicAdd(&t.sum_v[a][slot], (u64)s[a]);
                atomicMax(&t.top[slot], top);
                atomicMin(&t.bottom[slot], bottom);
            } else {
                planes_add(g, key, cnt, s, top, bottom);
            }
        }
    }
    if (lane == 0 && (n_selected | n_outside)) { atomicAdd(&t.selected, n_selected); atomicAdd(&t.outside, n_outside); }
    __syncthreads();
    for (int k = threadIdx.x; k < CT_SLOTS; k += CTPB) {
        const int key = t.key[k];
        if (key >= 0) {
            const long long s[3] = {(long long)t.sum_v[0][k], (long long)t.sum_v[1][k], (long long)t.sum_v[2][k]};
            planes_add(g, key, t.count[k], s, t.top[k], t.bottom[k]);
        }
    }
    if (threadIdx.x == 0 && (t.selected | t.outside)) {
        atomicAdd((u64*)g.totals + 0, (u64)t.selected);
        atomicAdd((u64*)g.totals + 2, (u64)t.outside);
    }
}

// the extrema back to f32 (0 for an empty column, as SphDiagRow's bounds of an empty row), binned = selected - outside
__global__ __launch_bounds__(CTPB) void k_columns_finish(ColumnPlanes g) {
    const int c = blockIdx.x * CTPB + threadIdx.x;
    if (c < g.nc) {
        const bool empty = g.count[c] == 0;
        g.top[c] = empty ? 0u : __float_as_uint(ordered_to_f32(g.top[c]));
        g.bottom[c] = empty ? 0u : __float_as_uint(ordered_to_f32(g.bottom[c]));
    }
    if (c == 0) g.totals[1] = g.totals[0] - g.totals[2];
}

void sph_columns_release(SphContext* c) { sph_observe_release(c->columns, &SphColumns::buf); }

// the state struct, and planes for `nc` columns (allocated again when the map size changes)
static int columns_state(SphContext* c, int nc) {
    SphColumns* g = sph_observe_state(c->columns);
    if (!g) return sph_fail(c, SPH_E_NOMEM, "sph_columns_reduce: out of host memory");
    if (g->buf && g->nc == nc) return 0;
    g->nc = 0; g->have = false;
    const size_t words64 = (size_t)4 * nc + 4;
    if (int rc = sph_observe_alloc(c, &g->buf, words64 * 8 + (size_t)2 * nc * 4, "sph_columns_reduce", "the map's planes")) return rc;
    g->count = (long long*)g->buf;
    g->sum_v = g->count + nc;
    g->totals = g->sum_v + (size_t)3 * nc;
    g->top = (unsigned*)(g->totals + 4);
    g->bottom = g->top + nc;
    g->nc = nc;
    return 0;
}

extern "C" {

int32_t sph_columns_reduce(SphContext* c, const SphColumnParams* p) {
    if (c && !p) return sph_fail(c, SPH_E_INVALID, "sph_columns_reduce: params is NULL");
    if (int rc = sph_observe_enter(c, "sph_columns_reduce", " (its ghost records would be counted twice); column maps are reduced on single-domain contexts only")) return rc;
    if (p->axis < 0 || p->axis > 2) return sph_fail(c, SPH_E_INVALID, "sph_columns_reduce: axis must be 0, 1 or 2");
    if (p->n[0] < 1 || p->n[1] < 1) return sph_fail(c, SPH_E_INVALID, "sph_columns_reduce: n[0] and n[1] must be at least 1");
    if ((long long)p->n[0] * p->n[1] > SPH_COLUMNS_MAX) {
        snprintf(c->err, sizeof(c->err), "sph_columns_reduce: %d x %d columns, a map holds at most SPH_COLUMNS_MAX = %d", p->n[0], p->n[1], SPH_COLUMNS_MAX);
        return SPH_E_INVALID;
    }
    for (int j = 0; j < 2; ++j) {
        if (!std::isfinite(p->inv_cell[j]) || !(p->inv_cell[j] > 0.f)) return sph_fail(c, SPH_E_INVALID, "sph_columns_reduce: inv_cell must be finite and positive");
        if (!std::isfinite(p->origin[j])) return sph_fail(c, SPH_E_INVALID, "sph_columns_reduce: origin must be finite");
    }
    const int nc = p->n[0] * p->n[1];
    if (int rc = columns_state(c, nc)) return rc;
    SphColumns* s = c->columns;
    ColumnPlanes g;
    g.count = s->count; g.sum_v = s->sum_v; g.totals = s->totals; g.top = s->top; g.bottom = s->bottom; g.nc = nc;
    const int map_blocks = (nc + CTPB - 1) / CTPB;
    hipLaunchKernelGGL(k_columns_clear, dim3(map_blocks), dim3(CTPB), 0, c->stream, g);
    SPH_LAUNCH_CHECK(c);
    const SphLive in = sph_live(c);
    if (in.N > 0) {
        const SphWalk w = sph_observe_walk(in.N, CTPB, CT_MAX_BLOCKS);
        hipLaunchKernelGGL(k_columns_scatter, dim3(w.blocks), dim3(CTPB), 0, c->stream, in.xm, in.vf, in.N, w.per_block, *p, g);
        SPH_LAUNCH_CHECK(c);
    }
    hipLaunchKernelGGL(k_columns_finish, dim3(map_blocks), dim3(CTPB), 0, c->stream, g);
    SPH_LAUNCH_CHECK(c);
    s->n[0] = p->n[0]; s->n[1] = p->n[1];
    s->have = true;
    return 0;
}

int32_t sph_columns_download(SphContext* c, int64_t* count, int64_t* sum_v, float* top, float* bottom, int32_t n_columns,
                             SphColumnTotals* totals) {
    if (!c) return SPH_E_INVALID;
    const SphColumns* s = c->columns;
    if (!s || !s->have) return sph_fail(c, SPH_E_STATE, "sph_columns_download: nothing has been reduced (call sph_columns_reduce first)");
    if (n_columns != s->nc) {
        snprintf(c->err, sizeof(c->err), "sph_columns_download: n_columns = %d, the last reduce made a map of %d x %d = %d columns", n_columns, s->n[0], s->n[1], s->nc);
        return SPH_E_INVALID;
    }
    SPH_HIP(c, hipSetDevice(c->device));
    const size_t nc = (size_t)s->nc;
    if (count) SPH_HIP(c, hipMemcpyAsync(count, s->count, nc * 8, hipMemcpyDeviceToHost, c->stream));
    if (sum_v) SPH_HIP(c, hipMemcpyAsync(sum_v, s->sum_v, 3 * nc * 8, hipMemcpyDeviceToHost, c->stream));
    if (top) SPH_HIP(c, hipMemcpyAsync(top, s->top, nc * 4, hipMemcpyDeviceToHost, c->stream));
    if (bottom) SPH_HIP(c, hipMemcpyAsync(bottom, s->bottom, nc * 4, hipMemcpyDeviceToHost, c->stream));
    return sph_observe_download(c, totals, s->totals, sizeof(SphColumnTotals));
}

}  // extern "C"
