// sph_tracers.hip -- passive tracers (include/sph_hip.h, "Passive tracers"): up to SPH_TRACERS_MAX massless points that the step loops
// advect with the Shepard mean of the velocity of the selected particles around them, one forward-Euler step per simulation step, on
// the device.  Where the sampler SCATTERS (every particle looks for positions, the cell array is never read), a tracer GATHERS: it
// reads the records of the 27 cells around it through the cell array of the step's sort.  Reads xm / vf (32 B per candidate) and
// cell_end; writes the tracer buffers and nothing else.
//
// The pair term, the selection and the fixed-point terms are the sampler's own (sph_sample_pair.h: one definition, so that a tracer
// and a probe point at the same place cannot disagree).  Every accumulation is an INTEGER sum, so the split of a tracer's candidates
// over lanes never changes a bit.
//
// Kernel (k_tracers_advance), gfx950 wave64: SIXTEEN lanes (one DPP row) serve one tracer, a wave four tracers, a block of four waves
// sixteen.  Cells flatten x-slowest and z-fastest, so the 27 cells are nine runs of three z-neighbours whose records are contiguous:
// run (i, j) is [cell_end[f(z_lo) - 1], cell_end[f(z_hi)]) with f the flat index, z clipped to the grid.  The row walks a run 16
// records a trip, lane l taking record first + trip * 16 + l: consecutive 16-byte records of xm and of vf, 256 B per row-load.
// m_V is xm.w and the flags are the bits of vf.w, as for the sampler.  Each lane keeps four i64 sums and a count; the row is then
// combined with four DPP row rotations (ror 8, 4, 2, 1: all 16 lanes end with the row's total, no LDS crossbar, no atomics) and lane
// 0 of the row advances the tracer and stores.  The tracer's own state is read by all 16 lanes from one address (a broadcast).
// Rows of a wave diverge only in the trip counts of their runs.  The runs are clipped to [0, N] before they are walked: a cell array
// that does not describe the records (it always does behind the step's sort) could not take a read outside them.
#include <cmath>
#include "sph_observe.h"
#include "sph_sample_pair.h"

#pragma clang fp contract(off)

#define TR_TPB 256
#define TR_ROW 16                       // lanes per tracer: one DPP row
#define TR_PER_BLOCK (TR_TPB / TR_ROW)

struct SphTracers {
    void* buf;                // one allocation for cap_m tracers: weight [cap] i64, x [cap][3], u [cap][3] f32, count, wet, dry [cap] i32
    size_t cap_m;
    float* hist;              // [record_capacity][m][3] f32
    size_t hist_bytes;        // allocated
    int m;
    bool have;                // a set has been made (m == 0: it was cleared)
    int record_every, record_capacity;
    long long min_weight;
    SphSel sel;
    long long advances, frames, dropped;
};

#define TR_BYTES_PER_TRACER (8 + 12 + 12 + 4 + 4 + 4)

struct TracerBufs { long long* weight; float *x, *u; int *count, *wet, *dry; };

static inline TracerBufs tracer_bufs(void* buf, size_t cap) {
    TracerBufs b;
    b.weight = (long long*)buf;
    b.x = (float*)(b.weight + cap);
    b.u = b.x + 3 * cap;
    b.count = (int*)(b.u + 3 * cap);
    b.wet = b.count + cap;
    b.dry = b.wet + cap;
    return b;
}

struct TracerArgs {
    float grid_size, inv_h, k_w, dt, pad, whi[3];
    int n[3];                 // grid_num
    int N, m;
    long long min_weight;
    float* frame;             // null: this advance stores no history frame
    SphSel sel;
};

__global__ __launch_bounds__(TR_TPB) void k_tracers_advance(const float4* __restrict__ xm, const float4* __restrict__ vf,
                                                            const int* __restrict__ cell_end, TracerArgs a, TracerBufs b) {
    const int sub = threadIdx.x & (TR_ROW - 1);
    const int t = blockIdx.x * TR_PER_BLOCK + (threadIdx.x >> 4);   // m <= 2^22: no overflow
    const bool live = t < a.m;
    float px = 0.f, py = 0.f, pz = 0.f;
    long long s_w = 0, s_x = 0, s_y = 0, s_z = 0;
    int cnt = 0;
    if (live) {
        px = b.x[3 * (size_t)t]; py = b.x[3 * (size_t)t + 1]; pz = b.x[3 * (size_t)t + 2];
        if (a.N > 0) {
            // pos_to_index (sph_internal.h, sph_cell_coord) without its clamp: a cell outside the grid is skipped below
            const int c0 = (int)(px / a.grid_size), c1 = (int)(py / a.grid_size), c2 = (int)(pz / a.grid_size);
            const int zlo = c2 - 1 < 0 ? 0 : c2 - 1, zhi = c2 + 1 > a.n[2] - 1 ? a.n[2] - 1 : c2 + 1;
            if (zlo <= zhi) {
                for (int i = -1; i <= 1; ++i) {
                    const int cx = c0 + i;
                    if (cx < 0 || cx >= a.n[0]) continue;
                    for (int j = -1; j <= 1; ++j) {
                        const int cy = c1 + j;
                        if (cy < 0 || cy >= a.n[1]) continue;
                        const int f = (cx * a.n[1] + cy) * a.n[2];
                        int first = f + zlo > 0 ? cell_end[f + zlo - 1] : 0;
                        int last = cell_end[f + zhi];
                        first = first < 0 ? 0 : first;
                        last = last > a.N ? a.N : last;
                        for (int k = first + sub; k < last; k += TR_ROW) {
                            const float4 V = vf[k];
                            if (!sph_selected(__float_as_int(V.w), a.sel)) continue;
                            const float4 X = xm[k];
                            float w;
                            if (!sample_pair(px, py, pz, X, a.inv_h, a.k_w, w)) continue;
                            cnt += 1;
                            s_w += sample_weight_term(w);
                            s_x += sample_term(w, sample_clamp_field(V.x));
                            s_y += sample_term(w, sample_clamp_field(V.y));
                            s_z += sample_term(w, sample_clamp_field(V.z));
                        }
                    }
                }
            }
        }
    }
    // every lane of the wave is here again: the rows of tracers past m carry zeros
    s_w = row_sum(s_w); s_x = row_sum(s_x); s_y = row_sum(s_y); s_z = row_sum(s_z);
    cnt = row_sum(cnt);
    if (!live || sub != 0) return;
    float ux = 0.f, uy = 0.f, uz = 0.f;
    if (s_w >= a.min_weight) {   // wet (min_weight >= 1: no division by zero)
        const double W = (double)s_w;
        ux = (float)((double)s_x / W); uy = (float)((double)s_y / W); uz = (float)((double)s_z / W);
        const float xn = px + a.dt * ux, yn = py + a.dt * uy, zn = pz + a.dt * uz;   // multiply, then add: not contracted
        px = fminf(fmaxf(xn, a.pad), a.whi[0]);
        py = fminf(fmaxf(yn, a.pad), a.whi[1]);
        pz = fminf(fmaxf(zn, a.pad), a.whi[2]);
        b.x[3 * (size_t)t] = px; b.x[3 * (size_t)t + 1] = py; b.x[3 * (size_t)t + 2] = pz;
        b.wet[t] += 1;
    } else {
        b.dry[t] += 1;
    }
    b.u[3 * (size_t)t] = ux; b.u[3 * (size_t)t + 1] = uy; b.u[3 * (size_t)t + 2] = uz;
    b.weight[t] = s_w;
    b.count[t] = cnt;
    if (a.frame) { a.frame[3 * (size_t)t] = px; a.frame[3 * (size_t)t + 1] = py; a.frame[3 * (size_t)t + 2] = pz; }
}

void sph_tracers_release(SphContext* c) { sph_observe_release(c->tracers, &SphTracers::buf, &SphTracers::hist); }

// step_loop's hook: one launch behind the head-of-step sort, nothing when no set is registered
int sph_tracers_advance(SphContext* c) {
    SphTracers* s = c->tracers;
    if (!s || s->m == 0) return 0;
    const SphParams& p = c->p;
    TracerArgs a;
    a.grid_size = p.grid_size; a.inv_h = 1.0f / p.support_radius; a.k_w = p.k_w; a.dt = p.dt; a.pad = p.padding;
    for (int k = 0; k < 3; ++k) { a.whi[k] = p.wall_hi[k]; a.n[k] = p.grid_num[k]; }
    const SphLive in = sph_live(c);
    a.N = in.N; a.m = s->m;
    a.min_weight = s->min_weight;
    a.sel = s->sel;
    a.frame = nullptr;
    const long long adv = s->advances + 1;
    bool stored = false, dropped = false;
    if (s->record_every > 0 && adv % s->record_every == 0) {
        if (s->frames < s->record_capacity) { a.frame = s->hist + (size_t)s->frames * 3 * (size_t)s->m; stored = true; }
        else dropped = true;
    }
    const unsigned blocks = (unsigned)((s->m + TR_PER_BLOCK - 1) / TR_PER_BLOCK);
    hipLaunchKernelGGL(k_tracers_advance, dim3(blocks), dim3(TR_TPB), 0, c->stream, in.xm, in.vf, (const int*)c->cell_end, a, tracer_bufs(s->buf, s->cap_m));
    SPH_LAUNCH_CHECK(c);
    s->advances = adv;
    s->frames += stored; s->dropped += dropped;
    return 0;
}

static int tracers_fail(SphContext* c, int rc, const char* who, const char* what) {
    snprintf(c->err, sizeof(c->err), "%s: %s", who, what);
    return rc;
}

static const char* const TR_WHY_SLAB = " (a tracer that crossed to another rank would have to travel with the halo); tracers exist on single-domain contexts only";

extern "C" {

int32_t sph_tracers_set(SphContext* c, const float* xyz, int32_t m, const SphTracerParams* tp) {
    const char* who = "sph_tracers_set";
    if (int rc = sph_observe_enter(c, who, TR_WHY_SLAB)) return rc;
    if (!tp) return tracers_fail(c, SPH_E_INVALID, who, "the parameters are NULL");
    if (m < 0 || m > SPH_TRACERS_MAX) {
        snprintf(c->err, sizeof(c->err), "%s: m = %d, must be in [0, SPH_TRACERS_MAX = %d]", who, m, SPH_TRACERS_MAX);
        return SPH_E_INVALID;
    }
    if (m > 0 && !xyz) return tracers_fail(c, SPH_E_INVALID, who, "xyz is NULL");
    if (!std::isfinite(tp->min_fill) || !(tp->min_fill > 0.f) || tp->min_fill > 4.f) return tracers_fail(c, SPH_E_INVALID, who, "min_fill must be finite and in (0, 4]");
    if (tp->record_every < 0 || tp->record_capacity < 0) return tracers_fail(c, SPH_E_INVALID, who, "record_every and record_capacity must not be negative");
    const unsigned long long hist_bytes = (unsigned long long)tp->record_capacity * (unsigned long long)m * 12ull;
    if (hist_bytes > (1ull << 31)) {
        snprintf(c->err, sizeof(c->err), "%s: a history of %d frames of %d tracers takes %llu bytes, more than 2^31", who, tp->record_capacity, m, hist_bytes);
        return SPH_E_INVALID;
    }
    SphSel sel;
    if (int rc = sample_select(c, who, tp->select, &sel)) return rc;
    for (int k = 0; k < m; ++k)
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[3 * (size_t)k + a];
            if (!std::isfinite(v) || v < c->p.padding || v > c->p.wall_hi[a]) {
                snprintf(c->err, sizeof(c->err), "%s: point %d has coordinate %d = %g, not finite or outside [padding, wall_hi] = [%g, %g]", who, k, a,
                         (double)v, (double)c->p.padding, (double)c->p.wall_hi[a]);
                return SPH_E_INVALID;
            }
        }
    if (!sph_observe_state(c->tracers)) return tracers_fail(c, SPH_E_NOMEM, who, "out of host memory");
    SphTracers* s = c->tracers;
    // grow only; whatever has to grow exists before anything old goes, so that a failure leaves the last good set as it was
    void *nb = nullptr, *nh = nullptr;
    const size_t buf_bytes = (size_t)m * TR_BYTES_PER_TRACER;
    hipError_t e = hipSuccess;
    if ((size_t)m > s->cap_m) e = hipMalloc(&nb, buf_bytes);
    if (e == hipSuccess && (size_t)hist_bytes > s->hist_bytes) e = hipMalloc(&nh, (size_t)hist_bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (nb) (void)hipFree(nb);
        snprintf(c->err, sizeof(c->err), "%s: hipMalloc of the tracer buffers (%zu bytes) or of the history (%llu bytes) failed: %s", who, buf_bytes,
                 hist_bytes, hipGetErrorString(e));
        return SPH_E_NOMEM;
    }
    if (nb || nh) SPH_HIP(c, hipStreamSynchronize(c->stream));   // (an advance may still be writing the old ones)
    if (nb) { (void)hipFree(s->buf); s->buf = nb; s->cap_m = (size_t)m; s->m = 0; }
    if (nh) { (void)hipFree(s->hist); s->hist = (float*)nh; s->hist_bytes = (size_t)hist_bytes; }
    if (s->buf) SPH_HIP(c, hipMemsetAsync(s->buf, 0, s->cap_m * TR_BYTES_PER_TRACER, c->stream));
    if (hist_bytes) SPH_HIP(c, hipMemsetAsync(s->hist, 0, (size_t)hist_bytes, c->stream));
    if (m > 0) SPH_HIP(c, hipMemcpyAsync(tracer_bufs(s->buf, s->cap_m).x, xyz, (size_t)m * 12, hipMemcpyHostToDevice, c->stream));
    SPH_HIP(c, hipStreamSynchronize(c->stream));   // xyz is the caller's again
    s->m = m;
    s->have = true;
    s->record_every = tp->record_every; s->record_capacity = tp->record_capacity;
    const long long mw = llrint((double)tp->min_fill * (double)(1 << SPH_SAMPLE_SCALE_LOG2));
    s->min_weight = mw < 1 ? 1 : mw;
    s->sel = sel;
    s->advances = s->frames = s->dropped = 0;
    return 0;
}

int32_t sph_tracers_info(SphContext* c, SphTracerInfo* out) {
    if (!c) return SPH_E_INVALID;
    if (!out) return sph_fail(c, SPH_E_INVALID, "sph_tracers_info: the result is NULL");
    const SphTracers* s = c->tracers;
    out->m = s ? s->m : 0;
    out->reserved_ = 0;
    out->advances = s ? s->advances : 0;
    out->frames = s ? s->frames : 0;
    out->dropped = s ? s->dropped : 0;
    return 0;
}

int32_t sph_tracers_download(SphContext* c, float* x, float* u, int64_t* weight, int32_t* count, int32_t* wet_steps, int32_t* dry_steps, int32_t m) {
    const char* who = "sph_tracers_download";
    if (int rc = sph_observe_enter(c, who, TR_WHY_SLAB)) return rc;
    const SphTracers* s = c->tracers;
    if (!s || !s->have) return tracers_fail(c, SPH_E_STATE, who, "no tracers have been set (call sph_tracers_set first)");
    if (m != s->m) {
        snprintf(c->err, sizeof(c->err), "%s: m = %d, the set holds %d tracers", who, m, s->m);
        return SPH_E_INVALID;
    }
    const TracerBufs b = tracer_bufs(s->buf, s->cap_m);
    const size_t n = (size_t)m;
    if (n) {
        if (x) SPH_HIP(c, hipMemcpyAsync(x, b.x, n * 12, hipMemcpyDeviceToHost, c->stream));
        if (u) SPH_HIP(c, hipMemcpyAsync(u, b.u, n * 12, hipMemcpyDeviceToHost, c->stream));
        if (weight) SPH_HIP(c, hipMemcpyAsync(weight, b.weight, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (count) SPH_HIP(c, hipMemcpyAsync(count, b.count, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (wet_steps) SPH_HIP(c, hipMemcpyAsync(wet_steps, b.wet, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (dry_steps) SPH_HIP(c, hipMemcpyAsync(dry_steps, b.dry, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    return sph_observe_download(c, nullptr, nullptr, 0);
}

int32_t sph_tracers_history_download(SphContext* c, float* xyz, int64_t frames, int32_t m) {
    const char* who = "sph_tracers_history_download";
    if (int rc = sph_observe_enter(c, who, TR_WHY_SLAB)) return rc;
    const SphTracers* s = c->tracers;
    if (!s || !s->have) return tracers_fail(c, SPH_E_STATE, who, "no tracers have been set (call sph_tracers_set first)");
    if (m != s->m || frames != s->frames) {
        snprintf(c->err, sizeof(c->err), "%s: frames = %lld, m = %d; the set holds %lld stored frames of %d tracers", who, (long long)frames, m, s->frames, s->m);
        return SPH_E_INVALID;
    }
    const size_t bytes = (size_t)frames * (size_t)m * 12;
    return sph_observe_download(c, bytes ? xyz : nullptr, s->hist, bytes);
}

}  // extern "C"
