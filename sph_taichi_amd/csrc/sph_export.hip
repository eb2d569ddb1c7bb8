// sph_export.hip -- particle export (include/sph_hip.h, "Particle export"): a device-side selection of the live records, ordered by
// persistent id and packed into the byte rows of a binary PLY vertex body.  Reads xm / vf / aux, writes its own buffers only.
// Touches nothing of the sort or the sweeps and writes no particle state.
//
// A compaction THROUGH THE ID TABLE: the persistent ids are unique and smaller than cold_cap (x_0 and colour are keyed by them), so a
// table of cold_cap i32 slots, slot[pid] = index of the selected record that carries pid, holds the selection already in id order; the
// marked slots are then ranked (counts per tile, one scan of the tile counts, ranks inside a tile) and gathered.  Five launches, each
// reading what the previous one wrote -- no workgroup ever waits for another:
//   k_export_clear   : slot[p] = -1 over the (tile-padded) table, the counters = 0
//   k_export_mark    : one streaming pass over the live records: aux (the id) always, vf when material or objects select, xm when the
//                      box does; a selected record i stores slot[pid] = i.  The selected count: ballot + popcount per wave, the waves'
//                      counts added in LDS, one integer atomic per block.  (A selected record whose id is outside [0, cold_cap) is
//                      counted and marks nothing: it shows up in duplicate_ids like a real duplicate.)
//   k_export_count   : one workgroup per tile of SPH_EXPORT_TILE slots counts the marked ones (four slots per thread, one 16-byte load)
//   k_export_offsets : ONE wave scans the tile counts exclusively, 64 counts per trip with the running total carried along; writes
//                      rows (the total) and duplicate_ids = selected - rows
//   k_export_pack    : one workgroup per tile: four trips of 256 slots; a marked slot's rank = tile offset + marked slots of the earlier
//                      trips + the earlier waves' totals of this trip (LDS) + popcount of the ballot below the lane; it gathers the
//                      record at slot[p] and writes the row's words.  The rows of a wave are consecutive in the output: they are
//                      staged in LDS and stored as consecutive dwords (SPH_EXPORT_PACK=direct in the environment selects per-lane
//                      row stores instead: the A/B of DESIGN.md).
// No arithmetic is done on a value: the only computations are the box comparison (f32, a NaN is outside) and pid % pid_stride.
// Determinism: which record marks a slot does not depend on order or scheduling while the ids are unique (one writer per slot), and
// every later stage is a function of the table alone.
#include <cmath>
#include <stdlib.h>
#include "sph_observe.h"

#define SPH_EXPORT_TILE 1024   // table slots per workgroup of k_export_count / k_export_pack
#define ETPB 256
#define EWAVES (ETPB / 64)
#define E_MARK_MAX_BLOCKS 2048
#define E_MAX_WORDS 11         // x y z, vx vy vz, density, pressure, mass, id, object
#define E_ALL_FIELDS (SPH_EXPORT_X | SPH_EXPORT_V | SPH_EXPORT_DENSITY | SPH_EXPORT_PRESSURE | SPH_EXPORT_MASS | SPH_EXPORT_ID | SPH_EXPORT_OBJECT)

struct SphExport {
    int* table;          // one allocation: slot[table_len], tile_count[n_tiles], tile_offset[n_tiles], counters[4]
    int* tile_count;
    int* tile_offset;
    unsigned* counters;  // selected, rows, duplicate_ids, (unused)
    int table_len;       // cold_cap rounded up to whole tiles
    int n_tiles;
    void* out;           // rows of the last select
    size_t out_bytes;    // allocated
    int out_rows;        // rows the last select's launch may write (the live count then)
    int row_words;
    bool have;           // a select has been enqueued
    bool fetched;        // host_counters hold the last select's counters
    bool direct;         // SPH_EXPORT_PACK=direct
    unsigned host_counters[4];
};

static inline int export_row_words(int fields) {
    return 3 + ((fields & SPH_EXPORT_V) ? 3 : 0) + ((fields & SPH_EXPORT_DENSITY) ? 1 : 0) + ((fields & SPH_EXPORT_PRESSURE) ? 1 : 0) +
           ((fields & SPH_EXPORT_MASS) ? 1 : 0) + ((fields & SPH_EXPORT_ID) ? 1 : 0) + ((fields & SPH_EXPORT_OBJECT) ? 1 : 0);
}

// table_len is a multiple of SPH_EXPORT_TILE, hence of ETPB
__global__ __launch_bounds__(ETPB) void k_export_clear(int* __restrict__ slot, int table_len, unsigned* __restrict__ counters) {
    const int p = blockIdx.x * ETPB + threadIdx.x;
    if (p < table_len) slot[p] = -1;
    if (p < 4) counters[p] = 0u;
}

struct ExportMark { int pid_stride, pid_phase, use_box; float box_lo[3], box_hi[3]; };   // what k_export_mark reads of the checked SphExportParams beside the SphSel

// grid = ceil(tiles / tiles_per_block) blocks of four waves; block b takes the tiles (256 records each) [b, b + 1) * tiles_per_block
__global__ __launch_bounds__(ETPB) void k_export_mark(const float4* __restrict__ xm, const float4* __restrict__ vf, const float4* __restrict__ aux,
                                                      int N, int cold_cap, int tiles_per_block, ExportMark p, SphSel sel, int* __restrict__ slot,
                                                      unsigned* __restrict__ counters) {
    __shared__ int wave_selected[EWAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool need_flags = sph_sel_any(sel);
    int n_selected = 0;   // wave-uniform
    const long long first = (long long)blockIdx.x * tiles_per_block * ETPB;
    // wave-uniform bounds: all 64 lanes make every trip (the ballot needs them)
    for (int tile = 0; tile < tiles_per_block; ++tile) {
        const long long base = first + (long long)tile * ETPB + wave * 64;
        if (base >= N) break;
        const long long i = base + lane;
        bool selected = false;
        if (i < N) {
            const int pid = __float_as_int(aux[i].w);
            selected = p.pid_stride == 1 || pid % p.pid_stride == p.pid_phase;
            if (selected && need_flags) selected = sph_selected(__float_as_int(vf[i].w), sel);
            if (selected && p.use_box) {
                const float4 X = xm[i];
                selected = X.x >= p.box_lo[0] && X.x <= p.box_hi[0] && X.y >= p.box_lo[1] && X.y <= p.box_hi[1] &&
                           X.z >= p.box_lo[2] && X.z <= p.box_hi[2];
            }
            if (selected && pid >= 0 && pid < cold_cap) slot[pid] = (int)i;
        }
        n_selected += __popcll(__ballot(selected));
    }
    if (lane == 0) wave_selected[wave] = n_selected;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < EWAVES; ++w) s += wave_selected[w];
        if (s) atomicAdd(counters + 0, (unsigned)s);
    }
}

// one workgroup per tile: thread t holds slots [4 t, 4 t + 4) of the tile
__global__ __launch_bounds__(ETPB) void k_export_count(const int* __restrict__ slot, int* __restrict__ tile_count) {
    __shared__ int wave_marked[EWAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int4 s = reinterpret_cast<const int4*>(slot + (size_t)blockIdx.x * SPH_EXPORT_TILE)[threadIdx.x];
    int n = (s.x >= 0) + (s.y >= 0) + (s.z >= 0) + (s.w >= 0);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if (lane == 0) wave_marked[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < EWAVES; ++w) t += wave_marked[w];
        tile_count[blockIdx.x] = t;
    }
}

// ONE wave: exclusive scan of the tile counts, 64 per trip
__global__ __launch_bounds__(64) void k_export_offsets(const int* __restrict__ tile_count, int n_tiles, int* __restrict__ tile_offset,
                                                       unsigned* __restrict__ counters) {
    const int lane = threadIdx.x;
    int running = 0;   // wave-uniform
    for (int base = 0; base < n_tiles; base += 64) {
        const int t = base + lane;
        const int cnt = t < n_tiles ? tile_count[t] : 0;
        const int incl = sph_wave_inclusive_scan(cnt, lane);
        if (t < n_tiles) tile_offset[t] = running + incl - cnt;
        running += __shfl(incl, 63, 64);
    }
    if (lane == 0) {
        counters[1] = (unsigned)running;
        counters[2] = counters[0] - (unsigned)running;
    }
}

// the words of the row of record s, in row order; `put(k, word)` stores word k
template <class Put>
__device__ __forceinline__ void export_row(const float4* __restrict__ xm, const float4* __restrict__ vf, const float4* __restrict__ aux,
                                           int s, int fields, Put put) {
    int k = 0;
    const float4 X = xm[s];
    put(k++, __float_as_uint(X.x)); put(k++, __float_as_uint(X.y)); put(k++, __float_as_uint(X.z));
    unsigned flags = 0u;
    if (fields & (SPH_EXPORT_V | SPH_EXPORT_OBJECT)) {
        const float4 V = vf[s];
        flags = __float_as_uint(V.w);
        if (fields & SPH_EXPORT_V) { put(k++, __float_as_uint(V.x)); put(k++, __float_as_uint(V.y)); put(k++, __float_as_uint(V.z)); }
    }
    if (fields & (SPH_EXPORT_DENSITY | SPH_EXPORT_PRESSURE | SPH_EXPORT_MASS | SPH_EXPORT_ID)) {
        const float4 A = aux[s];
        if (fields & SPH_EXPORT_DENSITY) put(k++, __float_as_uint(A.y));
        if (fields & SPH_EXPORT_PRESSURE) put(k++, __float_as_uint(A.z));
        if (fields & SPH_EXPORT_MASS) put(k++, __float_as_uint(A.x));
        if (fields & SPH_EXPORT_ID) put(k++, __float_as_uint(A.w));
    }
    if (fields & SPH_EXPORT_OBJECT) put(k++, (unsigned)sph_flags_object((int)flags));
}

// one workgroup per tile, four trips of 256 slots.  out holds out_rows rows of row_words words; a marked slot always names a live
// record (s < N) and ranks below the selected count <= N = out_rows: both are checked all the same before anything is touched.
template <bool STAGED>
__global__ __launch_bounds__(ETPB) void k_export_pack(const float4* __restrict__ xm, const float4* __restrict__ vf, const float4* __restrict__ aux,
                                                      int N, const int* __restrict__ slot, const int* __restrict__ tile_offset, int fields,
                                                      int row_words, int out_rows, unsigned* __restrict__ out) {
    __shared__ int wave_marked[EWAVES];
    __shared__ unsigned stage[STAGED ? EWAVES * 64 * E_MAX_WORDS : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base_row = tile_offset[blockIdx.x];   // block-uniform
    for (int trip = 0; trip < SPH_EXPORT_TILE / ETPB; ++trip) {
        const int s = slot[(size_t)blockIdx.x * SPH_EXPORT_TILE + trip * ETPB + threadIdx.x];
        const bool marked = s >= 0 && s < N;
        const u64 ballot = __ballot(marked);
        const int rank = __popcll(ballot & ((1ull << lane) - 1ull));
        const int wave_total = __popcll(ballot);
        if (lane == 0) wave_marked[wave] = wave_total;
        __syncthreads();
        int before = 0, block_total = 0;
#pragma unroll
        for (int w = 0; w < EWAVES; ++w) {
            const int m = wave_marked[w];
            if (w < wave) before += m;
            block_total += m;
        }
        const int wave_row = base_row + before;   // first row of this wave's rows
        if (STAGED) {
            unsigned* mine = stage + wave * 64 * E_MAX_WORDS;
            if (marked) export_row(xm, vf, aux, s, fields, [&](int k, unsigned w) { mine[rank * row_words + k] = w; });
            __syncthreads();
            // the wave's rows are one contiguous piece of the output: consecutive lanes store consecutive dwords
            const int n_words = wave_total * row_words;
            const long long room = ((long long)out_rows - wave_row) * row_words;   // words left in the buffer from this wave's first row (never short: see above)
            unsigned* dst = out + (size_t)wave_row * row_words;
            for (int j = lane; j < n_words && j < room; j += 64) dst[j] = mine[j];
        } else {
            const int row = wave_row + rank;
            if (marked && row < out_rows) {
                unsigned* dst = out + (size_t)row * row_words;
                export_row(xm, vf, aux, s, fields, [&](int k, unsigned w) { dst[k] = w; });
            }
        }
        base_row += block_total;
        __syncthreads();   // wave_marked (and the stage) are written again by the next trip
    }
}

void sph_export_release(SphContext* c) { sph_observe_release(c->exporter, &SphExport::table, &SphExport::out); }

// the state struct and the table (cold_cap is fixed for the life of a context: allocated once), and an output buffer of at least `bytes`
static int export_state(SphContext* c, size_t bytes) {
    const bool first = !c->exporter;
    SphExport* g = sph_observe_state(c->exporter);
    if (!g) return sph_fail(c, SPH_E_NOMEM, "sph_export_select: out of host memory");
    if (first) {
        const char* e = getenv("SPH_EXPORT_PACK");   // A/B aid of tools/export_timing.py: per-lane row stores instead of the LDS stage
        g->direct = e && strcmp(e, "direct") == 0;
    }
    if (!g->table) {
        const int n_tiles = (c->cold_cap + SPH_EXPORT_TILE - 1) / SPH_EXPORT_TILE;
        const size_t len = (size_t)n_tiles * SPH_EXPORT_TILE, words = len + (size_t)2 * n_tiles + 4;
        if (int rc = sph_observe_alloc(c, (void**)&g->table, words * 4, "sph_export_select", "the id table")) return rc;
        g->tile_count = g->table + len;
        g->tile_offset = g->tile_count + n_tiles;
        g->counters = (unsigned*)(g->tile_offset + n_tiles);
        g->table_len = (int)len;
        g->n_tiles = n_tiles;
    }
    if (bytes > g->out_bytes) {
        g->out_bytes = 0; g->have = false;   // (an earlier select may still be writing the rows: the helper waits for it)
        if (int rc = sph_observe_alloc(c, &g->out, bytes, "sph_export_select", "the row buffer")) return rc;
        g->out_bytes = bytes;
    }
    return 0;
}

// the counters of the last select on the host (synchronises once per select)
static int export_fetch(SphContext* c, const char* who) {
    SphExport* s = c->exporter;
    if (!s || !s->have) {
        snprintf(c->err, sizeof(c->err), "%s: nothing has been selected (call sph_export_select first)", who);
        return SPH_E_STATE;
    }
    if (s->fetched) return 0;
    const int rc = sph_observe_download(c, s->host_counters, s->counters, sizeof(s->host_counters));
    s->fetched = rc <= 0;   // (a HIP error is positive: the counters did not arrive)
    return rc;
}

extern "C" {

int32_t sph_export_select(SphContext* c, const SphExportParams* p) {
    if (c && !p) return sph_fail(c, SPH_E_INVALID, "sph_export_select: params is NULL");
    if (int rc = sph_observe_enter(c, "sph_export_select", " (its ghost records would be exported twice); particles are exported from single-domain contexts only")) return rc;
    if (!(p->fields & SPH_EXPORT_X)) return sph_fail(c, SPH_E_INVALID, "sph_export_select: fields must hold SPH_EXPORT_X (the position is always exported)");
    if (p->fields & ~E_ALL_FIELDS) return sph_fail(c, SPH_E_INVALID, "sph_export_select: fields holds unknown bits");
    SphSel sel;   // (the material's range is not checked here: an id no particle has selects nothing)
    if (sph_sel_make(p->material, p->n_objects, p->object_ids, false, &sel) == SPH_SEL_BAD_COUNT) {
        snprintf(c->err, sizeof(c->err), "sph_export_select: n_objects = %d, must be in [0, SPH_EXPORT_MAX_OBJECTS = %d]", p->n_objects, SPH_EXPORT_MAX_OBJECTS);
        return SPH_E_INVALID;
    }
    if (p->pid_stride < 1) return sph_fail(c, SPH_E_INVALID, "sph_export_select: pid_stride must be at least 1");
    if (p->pid_phase < 0 || p->pid_phase >= p->pid_stride) return sph_fail(c, SPH_E_INVALID, "sph_export_select: pid_phase must be in [0, pid_stride)");
    if (p->use_box) {
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(p->box_lo[a]) || !std::isfinite(p->box_hi[a])) return sph_fail(c, SPH_E_INVALID, "sph_export_select: the box must be finite");
            if (p->box_lo[a] > p->box_hi[a]) return sph_fail(c, SPH_E_INVALID, "sph_export_select: box_lo must not exceed box_hi");
        }
    }
    const int N = c->N, row_words = export_row_words(p->fields);
    if (int rc = export_state(c, (size_t)(N > 0 ? N : 1) * row_words * 4)) return rc;
    if (p->fields & (SPH_EXPORT_DENSITY | SPH_EXPORT_PRESSURE))
        if (int rc = sph_ensure_aux(c)) return rc;   // density / pressure of a fused step live in eos2 until somebody asks
    SphExport* s = c->exporter;
    if (int rc = sph_ensure_pid(c)) return rc;   // the kernels below read aux
    const SphLive in = sph_live(c);
    hipLaunchKernelGGL(k_export_clear, dim3(s->table_len / ETPB), dim3(ETPB), 0, c->stream, s->table, s->table_len, s->counters);
    SPH_LAUNCH_CHECK(c);
    if (N > 0) {
        const SphWalk w = sph_observe_walk(N, ETPB, E_MARK_MAX_BLOCKS);
        const ExportMark m{p->pid_stride, p->pid_phase, p->use_box, {p->box_lo[0], p->box_lo[1], p->box_lo[2]}, {p->box_hi[0], p->box_hi[1], p->box_hi[2]}};
        hipLaunchKernelGGL(k_export_mark, dim3(w.blocks), dim3(ETPB), 0, c->stream, in.xm, in.vf, in.aux, N, c->cold_cap, w.per_block, m, sel, s->table, s->counters);
        SPH_LAUNCH_CHECK(c);
    }
    hipLaunchKernelGGL(k_export_count, dim3(s->n_tiles), dim3(ETPB), 0, c->stream, s->table, s->tile_count);
    SPH_LAUNCH_CHECK(c);
    hipLaunchKernelGGL(k_export_offsets, dim3(1), dim3(64), 0, c->stream, s->tile_count, s->n_tiles, s->tile_offset, s->counters);
    SPH_LAUNCH_CHECK(c);
    if (N > 0) {
        if (s->direct)
            hipLaunchKernelGGL(k_export_pack<false>, dim3(s->n_tiles), dim3(ETPB), 0, c->stream, in.xm, in.vf, in.aux, N, s->table, s->tile_offset, p->fields,
                               row_words, N, (unsigned*)s->out);
        else
            hipLaunchKernelGGL(k_export_pack<true>, dim3(s->n_tiles), dim3(ETPB), 0, c->stream, in.xm, in.vf, in.aux, N, s->table, s->tile_offset, p->fields,
                               row_words, N, (unsigned*)s->out);
        SPH_LAUNCH_CHECK(c);
    }
    s->out_rows = N;
    s->row_words = row_words;
    s->have = true;
    s->fetched = false;
    return 0;
}

int32_t sph_export_info(SphContext* c, SphExportInfo* info) {
    if (!c) return SPH_E_INVALID;
    if (!info) return sph_fail(c, SPH_E_INVALID, "sph_export_info: info is NULL");
    if (int rc = export_fetch(c, "sph_export_info")) return rc;
    const SphExport* s = c->exporter;
    info->selected = (int64_t)s->host_counters[0];
    info->rows = (int64_t)s->host_counters[1];
    info->row_bytes = s->row_words * 4;
    info->duplicate_ids = (int32_t)s->host_counters[2];
    return 0;
}

int32_t sph_export_download(SphContext* c, void* host, size_t bytes) {
    if (!c) return SPH_E_INVALID;
    if (int rc = export_fetch(c, "sph_export_download")) return rc;
    const SphExport* s = c->exporter;
    if (s->host_counters[2] != 0u) {
        snprintf(c->err, sizeof(c->err), "sph_export_download: %u selected records but %u distinct persistent ids (duplicate_ids = %u): the ids are "
                 "not unique (or lie outside [0, %d)), no row order is defined", s->host_counters[0], s->host_counters[1], s->host_counters[2], c->cold_cap);
        return SPH_E_STATE;
    }
    const size_t want = (size_t)s->host_counters[1] * s->row_words * 4;
    if (bytes != want || (want > 0 && !host)) {
        snprintf(c->err, sizeof(c->err), "sph_export_download: bytes = %zu, the last select made %u rows of %d bytes = %zu", bytes, s->host_counters[1],
                 s->row_words * 4, want);
        return SPH_E_INVALID;
    }
    if (want == 0) return 0;
    return sph_observe_download(c, host, s->out, want);
}

}  // extern "C"
