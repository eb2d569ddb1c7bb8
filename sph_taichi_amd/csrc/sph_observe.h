// sph_observe.h -- what the read-only observers of the particle state share (sph_diag.hip, sph_columns.hip, sph_export.hip,
// sph_render.hip, sph_surface.hip): the view of the live records, the entry checks, the allocation and download sequences, the
// grid of a contiguous walk and the 64-bit shuffles.  An observer reads the records behind whatever the stream holds, writes
// buffers of its own and no particle state.
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

// A contiguous streaming walk over N > 0 records: block b takes the tiles (`threads` records each) [b, b + 1) * per_block, so
// that at most `max_blocks` blocks cover them.
struct SphWalk { int blocks, per_block; };
static inline SphWalk sph_observe_walk(int N, int threads, int max_blocks) {
    const int tiles = (N + threads - 1) / threads;
    const int per_block = (tiles + max_blocks - 1) / max_blocks;
    return SphWalk{(tiles + per_block - 1) / per_block, per_block};
}

#ifdef __HIPCC__
__device__ __forceinline__ long long shfl_xor_i64(long long v, int m) {
    const int lo = __shfl_xor((int)(v & 0xffffffffll), m, 64), hi = __shfl_xor((int)(v >> 32), m, 64);
    return ((long long)hi << 32) | (unsigned)lo;
}

__device__ __forceinline__ long long shfl_up_i64(long long v, int off) {
    const int lo = __shfl_up((int)(v & 0xffffffffll), off, 64), hi = __shfl_up((int)(v >> 32), off, 64);
    return ((long long)hi << 32) | (unsigned)lo;
}
#endif  // __HIPCC__
