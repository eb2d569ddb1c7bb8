// The validity rules of sph_taichi_amd/csrc/sph_derived.h, executed on the CPU (tests/test_derived_state.py compiles this
// file with the host compiler and runs one scenario per test case).  The helpers below issue the events in the order the
// launch code of sph_gather.hip / sph_sort.hip does; the scenarios assert the answers a reader would get.
#include <stdio.h>
#include <string.h>

#include "sph_derived.h"

static int g_fail = 0;
#define CHECK(expr)                                                            \
    do {                                                                       \
        if (!(expr)) { printf("FAIL line %d: %s\n", __LINE__, #expr); ++g_fail; } \
    } while (0)

static const int ID = 4242;  // a partition id (footprint, cut rule, limits)

// launch_brick_cfg of a sweep that does not read lists: cuts its own partition when the cached one does not serve it
static void sweep_partition(SphDerived& s, const SphPartKey& key) {
    if (sphd_partition_hit(s, key) == SPH_PART_NO) sphd_partition_rebuilt(s, key);
}
// GM_DENSITY_EOS (stg_kind 0 / 1) or GM_DF_DENSITY (2): launch_brick_cfg, then sweep_done
static void writer(SphDerived& s, const SphPartKey& key, int stg_kind, bool records) {
    sweep_partition(s, key);
    if (records) sphd_records_written(s, key);
    sphd_lists_written(s, stg_kind);
}
static bool nothing_usable(const SphDerived& s, const SphPartKey& key) {
    return !sphd_lists_usable(s) && !sphd_records_usable(s, key) && !sphd_one_gather_wcsph(s) && !sphd_one_gather_df(s, 1) &&
           !sphd_one_gather_df(s, 2);
}

static void wcsph_fused_step() {
    SphDerived s{};
    const SphPartKey K{ID, 0, 64, 0, 0};
    sphd_count_zeroed(s, true);                         // hash kernel
    CHECK(sphd_count_is_zero(s));
    sphd_sorted(s, true, K);                            // the sort's place kernel built the step's list
    CHECK(!sphd_count_is_zero(s));
    CHECK(sphd_partition_hit(s, K) == SPH_PART_EXACT);
    CHECK(nothing_usable(s, K) && !sphd_stats_have_lists(s) && !sphd_aux_in_eos2(s));
    writer(s, K, 1, true);                              // density sweep of a uniform fluid
    CHECK(sphd_partition_hit(s, K) == SPH_PART_EXACT);  // (no rebuild in between)
    CHECK(sphd_lists_usable(s) && sphd_records_usable(s, K) && sphd_one_gather_wcsph(s));
    CHECK(!sphd_one_gather_df(s, 1) && !sphd_one_gather_df(s, 2));
    CHECK(sphd_aux_in_eos2(s) && sphd_stats_have_lists(s));
    // a fluid of several masses: lists and records, but no one-gather form, and density / pressure went to aux
    SphDerived t{};
    sphd_sorted(t, true, K);
    writer(t, K, 0, true);
    CHECK(sphd_lists_usable(t) && sphd_records_usable(t, K) && !sphd_one_gather_wcsph(t) && !sphd_aux_in_eos2(t));
    // column records switched off (or never allocated): lists alone
    SphDerived u{};
    sphd_sorted(u, true, K);
    writer(u, K, 1, false);
    CHECK(sphd_lists_usable(u) && !sphd_records_usable(u, K) && sphd_one_gather_wcsph(u));
}

static void dfsph_step() {
    SphDerived s{};
    const SphPartKey K{ID, 0, 64, 0, 0};
    sphd_sorted(s, true, K);
    writer(s, K, 2, true);                              // GM_DF_DENSITY: the step's one writer
    CHECK(sphd_lists_usable(s) && sphd_records_usable(s, K) && !sphd_one_gather_wcsph(s) && !sphd_aux_in_eos2(s));
    CHECK(!sphd_one_gather_df(s, 1) && !sphd_one_gather_df(s, 2));       // k_kind 0
    sphd_k_written(s, 1);                               // density-change sweep
    CHECK(sphd_one_gather_df(s, 1) && !sphd_one_gather_df(s, 2));
    for (int it = 0; it < 3; ++it) {                    // divergence solver bodies (df_enqueue_body)
        CHECK(sphd_one_gather_df(s, 1));                // the Jacobi sweep
        sphd_bpart_consumed(s);
        sphd_k_written(s, 1); sphd_bpart_written(s);    // refresh sweep, collecting
        CHECK(sphd_bpart_ready(s));
        sphd_bpart_consumed(s);                         // convergence test
        CHECK(!sphd_bpart_ready(s));
        CHECK(sphd_lists_usable(s) && sphd_records_usable(s, K));
    }
    sphd_k_written(s, 0);                               // sphk_df_scale_factor
    CHECK(!sphd_one_gather_df(s, 1) && !sphd_one_gather_df(s, 2));
    sphd_k_written(s, 2);                               // density-advection sweep
    CHECK(!sphd_one_gather_df(s, 1) && sphd_one_gather_df(s, 2));
    CHECK(sphd_lists_usable(s) && sphd_records_usable(s, K) && sphd_partition_hit(s, K) == SPH_PART_EXACT);
    sphd_k_written(s, 0);                               // a refresh that took the cell walk
    CHECK(!sphd_one_gather_df(s, 2) && sphd_lists_usable(s));
}

static void advect_after_density() {
    SphDerived s{};
    const SphPartKey K{ID, 0, 64, 0, 0};
    sphd_sorted(s, true, K);
    writer(s, K, 1, true);
    sphd_invalidate(s);                                 // advect
    CHECK(nothing_usable(s, K));
    CHECK(sphd_partition_hit(s, K) == SPH_PART_NO);
    CHECK(sphd_stats_have_lists(s));                    // sph_get_stats after a step: the last density sweep's lengths
    CHECK(sphd_aux_in_eos2(s));                         // ... and its density / pressure are still owed to aux
    sphd_aux_folded(s);
    CHECK(!sphd_aux_in_eos2(s));
    sphd_sorted(s, false, SphPartKey{});                // a sort that builds no list (brick sweeps off)
    CHECK(!sphd_stats_have_lists(s) && sphd_partition_hit(s, K) == SPH_PART_NO && sphd_partition_hit(s, SphPartKey{}) == SPH_PART_NO);
    // the particle set re-based: eos2 is indexed from the old first record
    SphDerived t{};
    sphd_sorted(t, true, K);
    writer(t, K, 1, true);
    sphd_set_changed(t);
    CHECK(nothing_usable(t, K) && !sphd_aux_in_eos2(t) && sphd_stats_have_lists(t));
}

static void slab_order() {
    SphDerived s{};
    const SphPartKey K{ID, 2, 30, 0, 0};               // density layers: owned + first ghost layers
    const SphPartKey boundary{ID, 3, 6, 26, 29};       // both boundary sets in one launch (side stream)
    const SphPartKey interior{ID, 6, 26, 0, 0};
    sphd_sorted(s, true, K);
    writer(s, K, 1, true);
    const SphPartKey readers[2] = {boundary, interior};
    for (const SphPartKey& r : readers) {
        CHECK(sphd_partition_hit(s, r) == SPH_PART_SUBSET);
        CHECK(sphd_lists_usable(s) && sphd_one_gather_wcsph(s));
        CHECK(!sphd_records_usable(s, r));              // a subset sweep has other target tables
    }
    CHECK(sphd_records_usable(s, K));
    // what a subset is: same cut rule, both ranges inside the cached SINGLE range
    CHECK(sphd_partition_hit(s, SphPartKey{ID + 1, 6, 26, 0, 0}) == SPH_PART_NO);
    CHECK(sphd_partition_hit(s, SphPartKey{ID, 1, 26, 0, 0}) == SPH_PART_NO);
    CHECK(sphd_partition_hit(s, SphPartKey{ID, 6, 31, 0, 0}) == SPH_PART_NO);
    CHECK(sphd_partition_hit(s, SphPartKey{ID, 3, 6, 26, 31}) == SPH_PART_NO);
    SphDerived t{};
    sphd_sorted(t, true, K);
    sweep_partition(t, boundary);                       // a subset sweep leaves the cached partition in place
    CHECK(sphd_partition_hit(t, K) == SPH_PART_EXACT);
    sphd_partition_rebuilt(t, boundary);                // a cached partition of two ranges serves only itself
    CHECK(sphd_partition_hit(t, boundary) == SPH_PART_EXACT && sphd_partition_hit(t, SphPartKey{ID, 3, 6, 0, 0}) == SPH_PART_NO);
}

// writer under K, a sweep that reads no lists rebuilds under a wider K' (per-kernel C API only), reader under K
static void foreign_rebuild() {
    SphDerived s{};
    const SphPartKey K{ID, 2, 30, 0, 0}, Kw{ID, 0, 32, 0, 0};
    sphd_sorted(s, true, K);
    writer(s, K, 2, true);
    CHECK(sphd_records_usable(s, K) && sphd_partition_hit(s, Kw) == SPH_PART_NO);
    sweep_partition(s, Kw);
    CHECK(sphd_partition_hit(s, Kw) == SPH_PART_EXACT);
    CHECK(sphd_partition_hit(s, K) == SPH_PART_SUBSET);  // the new list would serve K's targets -- but not K's lists:
    CHECK(!sphd_records_usable(s, K));
    CHECK(!sphd_lists_usable(s));
    CHECK(!sphd_one_gather_wcsph(s) && !sphd_one_gather_df(s, 1) && !sphd_one_gather_df(s, 2));
    CHECK(sphd_stats_have_lists(s));                     // gcnt itself is untouched
    // the same with a WCSPH writer and k_j current
    SphDerived t{};
    sphd_sorted(t, true, K);
    writer(t, K, 1, true);
    sweep_partition(t, Kw);
    CHECK(!sphd_lists_usable(t) && !sphd_records_usable(t, K) && !sphd_one_gather_wcsph(t));
    // a writer that has to rebuild for itself ends with its own lists and records current
    writer(t, K, 1, true);
    CHECK(sphd_partition_hit(t, K) == SPH_PART_SUBSET && sphd_lists_usable(t) && sphd_records_usable(t, K));
    const SphPartKey Kx{ID + 1, 0, 32, 0, 0};            // (another cut rule: no subset, the writer rebuilds)
    writer(t, Kx, 1, true);
    CHECK(sphd_partition_hit(t, Kx) == SPH_PART_EXACT && sphd_lists_usable(t) && sphd_records_usable(t, Kx) && !sphd_records_usable(t, K));
}

// SPH_OPT_BRICK_SHAPE, _KERNEL_VARIANT, _EXACT_MATH, _BRICK_RECORDS, _PURE_FLUID_INSTANCE and the scan's error flag all
// report sphd_invalidate (test_derived_state.py checks that the API code does)
static void everything_dropped() {
    const SphPartKey K{ID, 0, 64, 0, 0};
    for (int kind = 1; kind <= 2; ++kind) {
        SphDerived s{};
        sphd_sorted(s, true, K);
        writer(s, K, kind, true);
        sphd_k_written(s, kind == 2 ? 2 : 0);
        sphd_invalidate(s);
        CHECK(nothing_usable(s, K));
        CHECK(sphd_partition_hit(s, K) == SPH_PART_NO);
        writer(s, K, kind, true);                       // the next writer cuts its own partition and all is current again
        CHECK(sphd_partition_hit(s, K) == SPH_PART_EXACT && sphd_lists_usable(s) && sphd_records_usable(s, K));
    }
}

int main(int argc, char** argv) {
    struct { const char* name; void (*fn)(); } all[] = {
        {"wcsph_fused_step", wcsph_fused_step}, {"dfsph_step", dfsph_step}, {"advect_after_density", advect_after_density},
        {"slab_order", slab_order}, {"foreign_rebuild", foreign_rebuild}, {"everything_dropped", everything_dropped},
    };
    int ran = 0;
    for (auto& t : all)
        if (argc < 2 || strcmp(argv[1], t.name) == 0) { t.fn(); ++ran; }
    if (ran == 0) { printf("FAIL: no scenario named %s\n", argc > 1 ? argv[1] : "?"); return 2; }
    printf("%s: %d scenario(s), %d failure(s)\n", g_fail ? "FAIL" : "PASS", ran, g_fail);
    return g_fail ? 1 : 0;
}
