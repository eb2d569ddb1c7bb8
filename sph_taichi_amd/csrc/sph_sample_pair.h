// sph_sample_pair.h -- THE pair term of the field sampling (include/sph_hip.h, "Field sampling") and its fixed-point terms, shared by
// the scatter sampler (sph_sample.hip) and the tracer gather (sph_tracers.hip) so that the two cannot disagree: does a selected (sph_observe.h)
// particle j contribute to position p and with which weight, and what one contributing pair adds to the i64 sums.  Beside them the one
// host function both users check their public SphSampleSelect with.  Everything here is compiled with contraction off (the pragma
// below holds for the rest of the including file as well: both users want that).
#pragma once
#include "sph_observe.h"

#pragma clang fp contract(off)

#define S_FIELD_LIMIT 16777216.f  // 2^24

// a public SphSampleSelect into *out (the sampler's entries and sph_tracers_set), or SPH_E_INVALID with its message
static inline int sample_select(SphContext* c, const char* who, const SphSampleSelect& sel, SphSel* out) {
    switch (sph_sel_make(sel.material, sel.n_objects, sel.object_ids, true, out)) {
        case SPH_SEL_BAD_MATERIAL: snprintf(c->err, sizeof(c->err), "%s: material = %d, must be in [-1, 255]", who, sel.material); return SPH_E_INVALID;
        case SPH_SEL_BAD_COUNT:
            snprintf(c->err, sizeof(c->err), "%s: n_objects = %d, must be in [0, SPH_SAMPLE_MAX_OBJECTS = %d]", who, sel.n_objects, SPH_SAMPLE_MAX_OBJECTS);
            return SPH_E_INVALID;
    }
    return 0;
}

#ifdef __HIPCC__
struct SamplePairGeom { float d[3], r, q; };   // what the gradient term reuses of the pair term

// THE pair term: does particle X = (x, y, z, m_V) contribute to position p, and with which weight
__device__ __forceinline__ bool sample_pair(float px, float py, float pz, const float4& X, float inv_h, float k_w, float& w, SamplePairGeom& geom) {
    const float dx = px - X.x, dy = py - X.y, dz = pz - X.z;
    const float r2 = (dx * dx + dy * dy) + dz * dz;
    const float r = sqrtf(r2);   // the correctly rounded one (hipcc's default for sqrtf; __fsqrt_rn is the 1-ulp v_sqrt_f32 here)
    const float q = r * inv_h;
    if (!(q <= 1.0f)) return false;
    geom.d[0] = dx; geom.d[1] = dy; geom.d[2] = dz; geom.r = r; geom.q = q;
    float W;
    if (q <= 0.5f) {
        const float q2 = q * q, q3 = q2 * q;
        W = k_w * ((6.f * q3 - 6.f * q2) + 1.f);
    } else {
        const float t = 1.f - q;
        W = (k_w * 2.f) * ((t * t) * t);
    }
    w = fminf(fmaxf(X.w * W, 0.f), 4.f);
    return true;
}

__device__ __forceinline__ bool sample_pair(float px, float py, float pz, const float4& X, float inv_h, float k_w, float& w) {
    SamplePairGeom unused;
    return sample_pair(px, py, pz, X, inv_h, k_w, w, unused);
}

__device__ __forceinline__ float sample_clamp_field(float a) { return fmaxf(fminf(a, S_FIELD_LIMIT), -S_FIELD_LIMIT); }
__device__ __forceinline__ long long sample_term(float w, float a) { return llrint(((double)w * (double)a) * (double)(1 << SPH_SAMPLE_SCALE_LOG2)); }
__device__ __forceinline__ long long sample_weight_term(float w) { return llrint((double)w * (double)(1 << SPH_SAMPLE_SCALE_LOG2)); }
#endif  // __HIPCC__
