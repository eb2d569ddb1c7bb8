// sph_observe.h -- what the read-only observers of the particle state share (sph_diag.hip, sph_columns.hip, sph_export.hip,
// sph_render.hip, sph_surface.hip, sph_sample.hip, sph_mesh.hip, sph_tracers.hip, sph_stats.hip, sph_loads.hip): the view of the live records, the entry
// checks, the allocation and download sequences, the grid of a contiguous walk, the 64-bit shuffles, the DPP row sums and THE particle selection
// (SphSel: who is selected by a material and a list of object ids -- the export, the field colouring of both frame styles, the
// field range, the samplers with the mesh cut from their grid, and the tracers all ask sph_selected).  An observer reads the
// records behind whatever the stream holds, writes buffers of its own and no particle state.
#pragma once
#include <new>

#include "sph_internal.h"

typedef unsigned long long u64;

struct SphLive { const float4 *xm, *vf, *aux, *acc; int N; };   // the live records (a slab rank's ghosts lie in front of in_off)
static inline SphLive sph_live(const SphContext* c) {
    return SphLive{c->xm[c->cur] + c->in_off, c->vf[c->cur] + c->in_off, c->aux[c->cur] + c->in_off, c->acc + c->in_off, c->N};
}

// Not null, not a slab rank (a context that holds a window of the domain: combining across GPUs is not built), the device set.
// `why` is the caller's clause behind "this context is a slab rank".
static inline int sph_observe_enter(SphContext* c, const char* who, const char* why) {
    if (!c) return SPH_E_INVALID;
    if (sph_is_slab(c)) {
        snprintf(c->err, sizeof(c->err), "%s: this context is a slab rank%s", who, why);
        return SPH_E_STATE;
    }
    SPH_HIP(c, hipSetDevice(c->device));
    return 0;
}

// the observer's state struct, zeroed, made on first use; null = out of host memory
template <class S>
static inline S* sph_observe_state(S*& s) {
    if (!s) s = new (std::nothrow) S();
    return s;
}

// *ptr = `bytes` of device memory.  An earlier allocation behind *ptr (another size) is freed first, after the launches that
// may still use it.  On failure *ptr is null and c->err says what was wanted.
static inline int sph_observe_alloc(SphContext* c, void** ptr, size_t bytes, const char* who, const char* what) {
    if (*ptr) {
        SPH_HIP(c, hipStreamSynchronize(c->stream));
        (void)hipFree(*ptr);
        *ptr = nullptr;
    }
    const hipError_t e = hipMalloc(ptr, bytes);
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    *ptr = nullptr;
    snprintf(c->err, sizeof(c->err), "%s: hipMalloc of %s (%zu bytes) failed: %s", who, what, bytes, hipGetErrorString(e));
    return SPH_E_NOMEM;
}

// sph_destroy's part: the state's device buffers (members of S; freeing a null pointer does nothing), then the state
template <class S, class... M>
static inline void sph_observe_release(S*& s, M... buffers) {
    if (!s) return;
    ((void)hipFree(s->*buffers), ...);
    delete s;
    s = nullptr;
}

// `bytes` from `dev` to `host` behind whatever the stream holds (host null: nothing more to copy), then the device's flags
static inline int sph_observe_download(SphContext* c, void* host, const void* dev, size_t bytes) {
    SPH_HIP(c, hipSetDevice(c->device));
    if (host) SPH_HIP(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(c, hipStreamSynchronize(c->stream));
    return sph_check_device_flags(c);
}

// THE ID OF A RECORD lives in the pid array while a lean scatter keeps the ids apart from aux, and in aux.w otherwise (sph_derived.h):
// a pointer and a stride (pid: 1; aux: the fourth word of a 16-byte record, stride 4) for kernels that must not ask for the fold
struct SphIds { const int* ptr; int stride; };
static inline SphIds sph_observe_ids(const SphContext* c) {
    if (sphd_pid_apart(c->dv)) return SphIds{c->pid[c->cur] + c->in_off, 1};
    return SphIds{reinterpret_cast<const int*>(c->aux[c->cur] + c->in_off) + 3, 4};
}

// A contiguous streaming walk over N > 0 records: block b takes the tiles (`threads` records each) [b, b + 1) * per_block, so
// that at most `max_blocks` blocks cover them.
struct SphWalk { int blocks, per_block; };
static inline SphWalk sph_observe_walk(int N, int threads, int max_blocks) {
    const int tiles = (N + threads - 1) / threads;
    const int per_block = (tiles + max_blocks - 1) / max_blocks;
    return SphWalk{(tiles + per_block - 1) / per_block, per_block};
}

// The selection of SphExportParams, SphFieldColour and SphSampleSelect (include/sph_hip.h): material -1 = any, n_objects 0 = all.
// By value into the launches, so that the ids are kernel arguments.
struct SphSel { int material, n_objects; int object_ids[32]; };
static_assert(SPH_EXPORT_MAX_OBJECTS == 32 && SPH_FIELD_MAX_OBJECTS == 32 && SPH_SAMPLE_MAX_OBJECTS == 32,
              "the three public object-list limits are one limit: SphSel holds 32 ids");

static constexpr bool sph_sel_any(const SphSel& s) { return s.material >= 0 || s.n_objects > 0; }   // host and device; false: nobody's flags need reading

// A public selection into *out, checked: n_objects in [0, 32] and, with check_material, material in [-1, 255].  The first
// n_objects ids are copied, the rest are 0.  The caller words its own message from the code.
enum { SPH_SEL_OK, SPH_SEL_BAD_MATERIAL, SPH_SEL_BAD_COUNT };
static inline int sph_sel_make(int material, int n_objects, const int32_t* ids, bool check_material, SphSel* out) {
    if (check_material && (material < -1 || material > 255)) return SPH_SEL_BAD_MATERIAL;
    if (n_objects < 0 || n_objects > 32) return SPH_SEL_BAD_COUNT;
    out->material = material;
    out->n_objects = n_objects;
    for (int k = 0; k < 32; ++k) out->object_ids[k] = k < n_objects ? ids[k] : 0;
    return SPH_SEL_OK;
}

#ifdef __HIPCC__
__device__ __forceinline__ bool sph_selected(int flags, const SphSel& s) {
    if (s.material >= 0 && sph_flags_material(flags) != s.material) return false;
    if (s.n_objects > 0) {
        const int obj = sph_flags_object(flags);
        bool in = false;
        for (int k = 0; k < s.n_objects; ++k) in = in || obj == s.object_ids[k];   // uniform index: scalar loads
        return in;
    }
    return true;
}

__device__ __forceinline__ long long shfl_xor_i64(long long v, int m) {
    const int lo = __shfl_xor((int)(v & 0xffffffffll), m, 64), hi = __shfl_xor((int)(v >> 32), m, 64);
    return ((long long)hi << 32) | (unsigned)lo;
}

__device__ __forceinline__ long long shfl_up_i64(long long v, int off) {
    const int lo = __shfl_up((int)(v & 0xffffffffll), off, 64), hi = __shfl_up((int)(v >> 32), off, 64);
    return ((long long)hi << 32) | (unsigned)lo;
}

// ---- one DPP row (16 lanes of a wave64) as a unit: the tracer gather and the load gather give a row to each target ----
template <int CTRL>
__device__ __forceinline__ int row_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }

template <int CTRL>
__device__ __forceinline__ long long row_dpp_i64(long long v) {
    const int lo = row_dpp<CTRL>((int)(v & 0xffffffffll)), hi = row_dpp<CTRL>((int)(v >> 32));
    return ((long long)hi << 32) | (unsigned)lo;
}

// the sum over the 16 lanes of a DPP row, in every lane of it (row_ror:8, :4, :2, :1 = dpp_ctrl 0x120 + n); all lanes of the wave active
__device__ __forceinline__ long long row_sum(long long v) {
    v += row_dpp_i64<0x128>(v);
    v += row_dpp_i64<0x124>(v);
    v += row_dpp_i64<0x122>(v);
    v += row_dpp_i64<0x121>(v);
    return v;
}

__device__ __forceinline__ int row_sum(int v) {
    v += row_dpp<0x128>(v);
    v += row_dpp<0x124>(v);
    v += row_dpp<0x122>(v);
    v += row_dpp<0x121>(v);
    return v;
}
#endif  // __HIPCC__
