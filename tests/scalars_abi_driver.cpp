// Prints the sizes and offsets of the scalar structs of include/sph_hip.h as the host compiler lays them out, fills and reads back
// every array element of both, and runs the library's own parameter checks of sph_scalars_set and sph_scalars_paint
// (csrc/sph_scalars_check.h, host only) over good and bad arguments, every struct and array on the heap at its exact size
// (tests/test_scalars_host.py compares layout and verdicts and builds this program with the address and undefined-behaviour
// sanitizers).  Host only: nothing of HIP.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include <cmath>
#include <limits>
#include <vector>

#include "sph_hip.h"
#include "../sph_taichi_amd/csrc/sph_scalars_check.h"

static SphScalarParams* good_params() {
    SphScalarParams* p = new SphScalarParams;
    std::memset(p, 0, sizeof(*p));
    p->K = 2; p->every = 3; p->kappa[0] = 1e-3f; p->kappa[1] = 0.f;
    p->select.material = 1;
    p->n_sources = 2; p->source_object[0] = 1; p->source_object[1] = 0;
    p->source_value[0][0] = 350.0; p->source_value[1][1] = -1048576.0;
    return p;
}

template <class F>
static void set_case(const char* name, F change, int64_t n_ids = 5, int fill = 0) {
    SphScalarParams* p = good_params();
    change(p);
    const size_t words = n_ids > 0 && p->K > 0 && p->K <= SPH_SCALARS_MAX_CHANNELS ? (size_t)n_ids * p->K : 0;
    std::vector<double>* v = new std::vector<double>(words, 1.5);   // exactly n_ids * K values: a read past them is an error
    if (fill == 1 && words) v->back() = std::numeric_limits<double>::quiet_NaN();
    if (fill == 2 && words) v->front() = 1048576.5;
    if (fill == 3 && words) v->back() = -1048576.0;
    char* err = new char[512];
    err[0] = 0;
    const int rc = sph_scalars_check_set(p, fill == 4 ? nullptr : v->data(), n_ids, 3, 8, err, 512);
    std::printf("set %s %d %s\n", name, rc, err);
    delete[] err; delete v; delete p;
}

static void paint_case(const char* name, int K, int channel, float lo, float hi, int lut_kind) {
    int32_t* lut = lut_kind == 0 ? nullptr : new int32_t[256 * 3];
    if (lut) for (int k = 0; k < 256 * 3; ++k) lut[k] = k % 256;
    if (lut_kind == 2) lut[256 * 3 - 1] = 256;
    if (lut_kind == 3) lut[0] = -1;
    char* err = new char[512];
    err[0] = 0;
    float inv = 0.f;
    const int rc = sph_scalars_check_paint(K, channel, lo, hi, lut, &inv, err, 512);
    std::printf("paint %s %d %s\n", name, rc, err);
    delete[] err; delete[] lut;
}

int main() {
    std::printf("SphScalarParams %zu K %zu kappa %zu every %zu select %zu n_sources %zu source_object %zu source_value %zu\n", sizeof(SphScalarParams),
                offsetof(SphScalarParams, K), offsetof(SphScalarParams, kappa), offsetof(SphScalarParams, every), offsetof(SphScalarParams, select),
                offsetof(SphScalarParams, n_sources), offsetof(SphScalarParams, source_object), offsetof(SphScalarParams, source_value));
    std::printf("SphScalarInfo %zu K %zu every %zu ids %zu samples %zu steps_seen %zu overshoot %zu saturated %zu\n", sizeof(SphScalarInfo),
                offsetof(SphScalarInfo, K), offsetof(SphScalarInfo, every), offsetof(SphScalarInfo, ids), offsetof(SphScalarInfo, samples),
                offsetof(SphScalarInfo, steps_seen), offsetof(SphScalarInfo, overshoot), offsetof(SphScalarInfo, saturated));
    std::printf("SPH_SCALARS_MAX_CHANNELS %d\nSPH_SCALARS_MAX_SOURCES %d\nSPH_SCALARS_SCALE_LOG2 %d\nSPH_ABI_VERSION %d\n", SPH_SCALARS_MAX_CHANNELS,
                SPH_SCALARS_MAX_SOURCES, SPH_SCALARS_SCALE_LOG2, SPH_ABI_VERSION);
    SphScalarParams* p = new SphScalarParams;
    std::memset(p, 0, sizeof(*p));
    double sum = 0.0;
    for (int s = 0; s < SPH_SCALARS_MAX_SOURCES; ++s) {
        p->source_object[s] = s;
        for (int k = 0; k < SPH_SCALARS_MAX_CHANNELS; ++k) { p->source_value[s][k] = s * 10.0 + k; p->kappa[k] = (float)k; }
    }
    for (int s = 0; s < SPH_SCALARS_MAX_SOURCES; ++s)
        for (int k = 0; k < SPH_SCALARS_MAX_CHANNELS; ++k) sum += p->source_value[s][k] + p->kappa[k] + p->source_object[s];
    delete p;
    std::printf("checksum %.1f\n", sum);
    const float nanf_ = std::numeric_limits<float>::quiet_NaN(), inff = std::numeric_limits<float>::infinity();
    const double inf = std::numeric_limits<double>::infinity();
    set_case("good", [](SphScalarParams*) {});
    set_case("good_null_values", [](SphScalarParams*) {}, 8, 4);
    set_case("good_at_the_limit", [](SphScalarParams*) {}, 5, 3);
    set_case("K_5", [](SphScalarParams* q) { q->K = 5; });
    set_case("K_negative", [](SphScalarParams* q) { q->K = -1; });
    set_case("K_huge", [](SphScalarParams* q) { q->K = 1 << 30; });
    set_case("every_0", [](SphScalarParams* q) { q->every = 0; });
    set_case("n_sources_9", [](SphScalarParams* q) { q->n_sources = 9; });
    set_case("n_sources_huge", [](SphScalarParams* q) { q->n_sources = 1 << 30; });
    set_case("n_sources_negative", [](SphScalarParams* q) { q->n_sources = -1; });
    set_case("kappa_negative", [](SphScalarParams* q) { q->kappa[1] = -1e-9f; });
    set_case("kappa_nan", [=](SphScalarParams* q) { q->kappa[0] = nanf_; });
    set_case("kappa_inf", [=](SphScalarParams* q) { q->kappa[0] = inff; });
    set_case("kappa_beyond_K_is_not_read", [=](SphScalarParams* q) { q->kappa[2] = nanf_; q->source_value[0][3] = inf; });
    set_case("source_outside", [](SphScalarParams* q) { q->source_object[1] = 3; });
    set_case("source_negative", [](SphScalarParams* q) { q->source_object[0] = -1; });
    set_case("source_twice", [](SphScalarParams* q) { q->source_object[1] = 1; });
    set_case("source_beyond_n_is_not_read", [](SphScalarParams* q) { q->source_object[2] = -7; });
    set_case("source_value_inf", [=](SphScalarParams* q) { q->source_value[1][0] = inf; });
    set_case("source_value_large", [](SphScalarParams* q) { q->source_value[0][1] = 1048577.0; });
    set_case("material_256", [](SphScalarParams* q) { q->select.material = 256; });
    set_case("select_33", [](SphScalarParams* q) { q->select.n_objects = 33; });
    set_case("select_negative", [](SphScalarParams* q) { q->select.n_objects = -1; });
    set_case("n_ids_0", [](SphScalarParams*) {}, 0);
    set_case("n_ids_negative", [](SphScalarParams*) {}, -4);
    set_case("n_ids_above_cold", [](SphScalarParams*) {}, 9);
    set_case("value_nan_last", [](SphScalarParams*) {}, 8, 1);
    set_case("value_large_first", [](SphScalarParams*) {}, 8, 2);
    paint_case("good", 2, 1, 0.f, 40.f, 1);
    paint_case("channel_2", 2, 2, 0.f, 1.f, 1);
    paint_case("channel_negative", 2, -1, 0.f, 1.f, 1);
    paint_case("lo_equals_hi", 1, 0, 1.f, 1.f, 1);
    paint_case("hi_nan", 1, 0, 0.f, nanf_, 1);
    paint_case("lo_inf", 1, 0, -inff, 0.f, 1);
    paint_case("too_narrow", 1, 0, 0.f, 1e-45f, 1);
    paint_case("too_wide", 1, 0, -3e38f, 3e38f, 1);
    paint_case("null_table", 1, 0, 0.f, 1.f, 0);
    paint_case("entry_256_last", 1, 0, 0.f, 1.f, 2);
    paint_case("entry_negative_first", 1, 0, 0.f, 1.f, 3);
    return 0;
}
