// sph_scalars_check.h -- the parameter checks of sph_scalars_set and sph_scalars_paint (include/sph_hip.h, "Carried scalars").
//
// Host only, no HIP, no context: tests/scalars_abi_driver.cpp runs them on the CPU under the address and undefined-behaviour
// sanitizers.  Each returns 0 or SPH_E_INVALID with the reason in `err`; neither reads an array element before the count that
// bounds it has been checked.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/sph_hip.h"

#define SPH_SCALARS_VALUE_MAX 1048576.0   // 2^20

static inline bool sph_scalars_value_ok(double v) { return isfinite(v) && fabs(v) <= SPH_SCALARS_VALUE_MAX; }

// a set with K >= 1: `values` f64 [n_ids][K] or null; n_objects, cold_cap: the context's object count and cold capacity
static inline int sph_scalars_check_set(const SphScalarParams* sp, const double* values, int64_t n_ids, int n_objects, int cold_cap, char* err,
                                        size_t err_len) {
    const char* who = "sph_scalars_set";
    if (sp->K < 1 || sp->K > SPH_SCALARS_MAX_CHANNELS) {
        snprintf(err, err_len, "%s: K = %d, must be in [0, SPH_SCALARS_MAX_CHANNELS = %d]", who, sp->K, SPH_SCALARS_MAX_CHANNELS);
        return SPH_E_INVALID;
    }
    if (sp->every < 1) {
        snprintf(err, err_len, "%s: every = %d, must be at least 1", who, sp->every);
        return SPH_E_INVALID;
    }
    if (sp->n_sources < 0 || sp->n_sources > SPH_SCALARS_MAX_SOURCES) {
        snprintf(err, err_len, "%s: n_sources = %d, must be in [0, SPH_SCALARS_MAX_SOURCES = %d]", who, sp->n_sources, SPH_SCALARS_MAX_SOURCES);
        return SPH_E_INVALID;
    }
    for (int k = 0; k < sp->K; ++k)
        if (!isfinite(sp->kappa[k]) || sp->kappa[k] < 0.f) {
            snprintf(err, err_len, "%s: kappa[%d] = %g, must be finite and not negative", who, k, (double)sp->kappa[k]);
            return SPH_E_INVALID;
        }
    for (int k = 0; k < sp->n_sources; ++k) {
        if (sp->source_object[k] < 0 || sp->source_object[k] >= n_objects) {
            snprintf(err, err_len, "%s: source object %d is outside [0, n_objects = %d)", who, sp->source_object[k], n_objects);
            return SPH_E_INVALID;
        }
        for (int l = 0; l < k; ++l)
            if (sp->source_object[l] == sp->source_object[k]) {
                snprintf(err, err_len, "%s: source object %d is named twice", who, sp->source_object[k]);
                return SPH_E_INVALID;
            }
        for (int ch = 0; ch < sp->K; ++ch)
            if (!sph_scalars_value_ok(sp->source_value[k][ch])) {
                snprintf(err, err_len, "%s: source_value[%d][%d] = %g, must be finite and at most 2^20 in magnitude", who, k, ch, sp->source_value[k][ch]);
                return SPH_E_INVALID;
            }
    }
    if (sp->select.material < -1 || sp->select.material > 255) {
        snprintf(err, err_len, "%s: material = %d, must be in [-1, 255]", who, sp->select.material);
        return SPH_E_INVALID;
    }
    if (sp->select.n_objects < 0 || sp->select.n_objects > SPH_SAMPLE_MAX_OBJECTS) {
        snprintf(err, err_len, "%s: n_objects = %d, must be in [0, SPH_SAMPLE_MAX_OBJECTS = %d]", who, sp->select.n_objects, SPH_SAMPLE_MAX_OBJECTS);
        return SPH_E_INVALID;
    }
    if (n_ids < 1 || n_ids > (int64_t)cold_cap) {
        snprintf(err, err_len, "%s: n_ids = %lld, must be in [1, the cold capacity = %d]", who, (long long)n_ids, cold_cap);
        return SPH_E_INVALID;
    }
    if (values) {
        const size_t K = (size_t)sp->K, words = (size_t)n_ids * K;
        for (size_t k = 0; k < words; ++k)
            if (!sph_scalars_value_ok(values[k])) {
                snprintf(err, err_len, "%s: values[%zu][%zu] = %g, must be finite and at most 2^20 in magnitude", who, k / K, k % K, values[k]);
                return SPH_E_INVALID;
            }
    }
    return 0;
}

// a paint of a set of K channels; *inv = 1.f / (hi - lo) on success
static inline int sph_scalars_check_paint(int K, int channel, float lo, float hi, const int32_t* lut, float* inv, char* err, size_t err_len) {
    const char* who = "sph_scalars_paint";
    if (channel < 0 || channel >= K) {
        snprintf(err, err_len, "%s: channel = %d, the set holds %d channels", who, channel, K);
        return SPH_E_INVALID;
    }
    const char* what = nullptr;
    if (!isfinite(lo) || !isfinite(hi)) what = "lo and hi must be finite";
    else if (!(lo < hi)) what = "lo must be smaller than hi";
    else {
        *inv = 1.0f / (hi - lo);
        if (!(*inv > 0.0f) || !isfinite(*inv)) what = "the range is too narrow or too wide for binary32";
        else if (!lut) what = "the table is NULL";
        else
            for (int k = 0; k < 256 * 3 && !what; ++k)
                if (lut[k] < 0 || lut[k] > 255) what = "a table entry lies outside [0, 255]";
    }
    if (!what) return 0;
    snprintf(err, err_len, "%s: %s", who, what);
    return SPH_E_INVALID;
}
