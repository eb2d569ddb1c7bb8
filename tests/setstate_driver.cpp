// The rules of sph_taichi_amd/csrc/sph_setstate.h, executed on the CPU (tests/test_setstate.py compiles this file with the
// host compiler and runs one scenario per test case).  The helpers below issue the events in the order the entry points
// of sph_api.hip do; the scenarios assert the answers a reader would get.  The expected values are those of the API code
// before the header existed (every entry point assigned the fields by hand), not a reading of the header.
#include <stdio.h>
#include <string.h>

#include "sph_setstate.h"

static int g_fail = 0;
#define CHECK(expr)                                                            \
    do {                                                                       \
        if (!(expr)) { printf("FAIL line %d: %s\n", __LINE__, #expr); ++g_fail; } \
    } while (0)

// the public field ids (include/sph_hip.h), written out: the header's mirror is checked against them here as well
enum { F_OBJECT_ID = 0, F_X = 1, F_X_0 = 2, F_V = 3, F_ACCELERATION = 4, F_M_V = 5, F_M = 6, F_DENSITY = 7, F_PRESSURE = 8,
       F_MATERIAL = 9, F_COLOR = 10, F_IS_DYNAMIC = 11, F_PID = 14, F_DFSPH_FACTOR = 16, F_DENSITY_ADV = 17 };
enum { OPT_GATHER_IMPL = 0, OPT_NO_DYNAMIC_SOLIDS = 4, OPT_SLAB_DROP_OUTSIDE = 6, OPT_UNIFORM_FLUID = 7 };

// refresh_dyn: counts only what is unknown; opt_no_dynamic vouches for 0; otherwise the device's count
static void refresh_dyn(SphSetState& s, bool opt_no_dynamic, int device_count) {
    if (sphs_dyn_known(s)) return;
    sphs_dyn_counted(s, opt_no_dynamic ? 0 : device_count);
}
// sph_update_grid_id, sph_prefix_sum, sph_counting_sort: false = refused with SPH_E_STATE, nothing reported
static bool hash(SphSetState& s) { sphs_hashed(s); return true; }
static bool scan(SphSetState& s) { if (!sphs_can_scan(s)) return false; sphs_scanned(s); return true; }
static bool scatter(SphSetState& s, bool opt_no_dynamic, int device_count) {
    if (!sphs_can_scatter(s)) return false;
    refresh_dyn(s, opt_no_dynamic, device_count);
    sphs_scattered(s);
    return true;
}
static bool sort(SphSetState& s, bool opt_no_dynamic, int device_count) { return hash(s) && scan(s) && scatter(s, opt_no_dynamic, device_count); }
// uniform_fluid() + sphk_check_uniform_fluid: h = (min mass bits, max mass bits, fluid m_V != m_V0, fluid particles)
static void decide_uniform(SphSetState& s, bool ruled_out, int N, float m_min, float m_max, unsigned n_bad_mv, unsigned n_fluid) {
    if (ruled_out) { sphs_uniform_ruled_out(s); return; }
    if (sphs_uniform_decided(s)) return;
    sphs_uniform_check_begun(s);
    if (N <= 0) return;
    if (n_fluid > 0 && memcmp(&m_min, &m_max, sizeof(float)) == 0 && n_bad_mv == 0) sphs_uniform_checked(s, m_min, n_fluid, N);
}
// sph_upload: the acceleration is reported before the copy, the per-field consequences behind it
static void upload(SphSetState& s, int field) {
    if (field == F_ACCELERATION) sphs_acc_written_all(s);
    sphs_field_uploaded(s, field);
}
// a single context holding N fluid particles of one mass, after one step
static SphSetState pure_after_step(int N) {
    SphSetState s;
    sphs_init(s);
    refresh_dyn(s, false, 0);
    sphs_acc_written_all(s);
    CHECK(sort(s, false, 0));
    decide_uniform(s, false, N, 0.008f, 0.008f, 0, (unsigned)N);
    return s;
}

static void stand_alone_sort() {
    SphSetState s;
    sphs_init(s);
    CHECK(!sphs_can_scan(s) && !sphs_can_scatter(s) && !sphs_neighbours_ready(s) && !sphs_cell_table_ready(s));
    CHECK(!sphs_dyn_known(s) && sphs_dyn_count(s) == -1 && !sphs_obj_info_current(s) && !sphs_uniform_decided(s) && sphs_acc_complete(s));
    CHECK(!scan(s) && !scatter(s, false, 3));            // each refused out of order
    CHECK(hash(s));
    CHECK(sphs_can_scan(s) && !sphs_can_scatter(s) && !scatter(s, false, 3));
    CHECK(scan(s));
    CHECK(sphs_can_scatter(s) && sphs_cell_table_ready(s) && !sphs_neighbours_ready(s));   // the table without the order
    CHECK(scatter(s, false, 3));
    CHECK(sphs_neighbours_ready(s) && sphs_cell_table_ready(s) && sphs_dyn_count(s) == 3);
    CHECK(!sphs_can_scan(s));                            // the histogram offsets are consumed: no second scan of them
    CHECK(sphs_can_scatter(s));                          // (the scatter looks at the table alone)
    CHECK(hash(s));                                      // the next hash pass starts a histogram in the current cell array
    CHECK(!sphs_neighbours_ready(s) && !sphs_cell_table_ready(s) && !sphs_can_scatter(s));
    CHECK(scan(s) && scatter(s, false, 99) && sphs_dyn_count(s) == 3);   // known: not counted again
}

static void step_then_truncate_append_same_n() {
    for (int vouched = 0; vouched <= 1; ++vouched) {     // SPH_OPT_NO_DYNAMIC_SOLIDS
        SphSetState s = pure_after_step(1000);
        if (vouched) { sphs_option_changed(s, OPT_NO_DYNAMIC_SOLIDS); refresh_dyn(s, true, 0); decide_uniform(s, false, 1000, 0.008f, 0.008f, 0, 1000); }
        CHECK(sphs_pure_fluid(s, 1, 1000, false) && sphs_dyn_count(s) == 0);
        sphs_truncated(s, true, vouched != 0);           // 1000 -> 990
        CHECK(!sphs_pure_fluid(s, 1, 990, false) && !sphs_pure_fluid(s, 1, 1000, false));
        CHECK(sphs_dyn_known(s) == (vouched != 0));      // unknown unless the host vouched
        CHECK(sphs_neighbours_ready(s) && sphs_cell_table_ready(s));   // truncate touches no pipeline flag
        CHECK(sphs_uniform(s));                          // ... and not the uniform verdict
        sphs_appended(s, false);                         // 990 -> 1000 again
        CHECK(!sphs_pure_fluid(s, 1, 1000, false));      // the verdict is gone although N is restored
        CHECK(!sphs_uniform_decided(s) && !sphs_dyn_known(s) && !sphs_neighbours_ready(s) && !sphs_can_scan(s) && !sphs_can_scatter(s));
    }
    SphSetState t = pure_after_step(1000);               // a truncate to the same count changes nothing
    sphs_truncated(t, false, false);
    CHECK(sphs_pure_fluid(t, 1, 1000, false) && sphs_dyn_count(t) == 0 && sphs_neighbours_ready(t));
}

static void append_vouched() {
    SphSetState s = pure_after_step(1000);
    CHECK(sphs_uniform(s) && sphs_uniform_mass(s) == 0.008f && sphs_pure_fluid(s, 1, 1000, false));
    sphs_appended(s, true);                              // opt_uniform == 1
    CHECK(sphs_uniform(s) && sphs_uniform_mass(s) == 0.008f);            // the uniform verdict survives
    CHECK(!sphs_pure_fluid(s, 1, 1010, false) && !sphs_pure_fluid(s, 1, 1000, false));   // the pure one does not
    CHECK(sphs_pure_fluid(s, 2, 1010, true));            // ... unless the host vouches for the whole scene
    CHECK(!sphs_dyn_known(s) && !sphs_neighbours_ready(s) && !sphs_cell_table_ready(s) && !sphs_can_scan(s));
    SphSetState t = pure_after_step(1000);
    sphs_appended(t, false);
    CHECK(!sphs_uniform_decided(t) && !sphs_pure_fluid(t, 2, 1010, true));
}

static void select_range() {
    SphSetState s = pure_after_step(1000);
    sphs_obj_info_read(s);
    sphs_range_selected(s);
    CHECK(!sphs_neighbours_ready(s) && !sphs_can_scan(s) && !sphs_can_scatter(s));
    CHECK(hash(s) && scan(s));
    CHECK(!sphs_neighbours_ready(s));                    // the order is dropped: a table alone does not bring it back
    CHECK(sphs_obj_info_current(s));                     // the object info stays
    CHECK(!sphs_dyn_known(s) && !sphs_pure_fluid(s, 1, 1000, false) && sphs_uniform(s));
}

static void count_set() {
    SphSetState s = pure_after_step(1000);
    sphs_obj_info_read(s);
    sphs_count_set(s);
    CHECK(!sphs_neighbours_ready(s) && !sphs_can_scan(s) && !sphs_can_scatter(s));
    CHECK(hash(s) && scan(s));
    CHECK(sphs_neighbours_ready(s));                     // the order flag was left: the table brings the sweeps back
    CHECK(!sphs_obj_info_current(s));                    // the object info goes
    CHECK(!sphs_dyn_known(s) && !sphs_pure_fluid(s, 1, 1000, false) && sphs_uniform(s));
}

static void upload_table() {
    // field -> forgets (the dynamic count, the uniform verdict, keys + table, the object info), as sph_upload's four
    // conditions had it; every other uploadable field forgets nothing
    static const struct { int field; bool dyn, uniform, table, obj; } rows[] = {
        {F_OBJECT_ID, false, false, false, true},   {F_X, false, false, true, false},        {F_X_0, false, false, false, true},
        {F_V, false, false, false, false},          {F_ACCELERATION, false, false, false, false}, {F_M_V, false, true, false, false},
        {F_M, false, true, false, false},           {F_DENSITY, true, false, false, false},  {F_PRESSURE, false, false, false, false},
        {F_MATERIAL, true, true, false, true},      {F_COLOR, false, false, false, false},   {F_IS_DYNAMIC, true, false, false, true},
        {F_PID, false, false, false, true},         {F_DFSPH_FACTOR, false, false, false, false}, {F_DENSITY_ADV, false, false, false, false},
    };
    for (const auto& r : rows) {
        for (int stage = 0; stage < 2; ++stage) {        // 0: after a sort; 1: between hash + scan and the scatter
            SphSetState s = pure_after_step(1000);
            sphs_obj_info_read(s);
            sphs_acc_interior_kept(s, true);
            if (stage == 1) CHECK(hash(s) && scan(s));
            upload(s, r.field);
            CHECK(sphs_dyn_known(s) == !r.dyn);
            CHECK(sphs_uniform_decided(s) == !r.uniform);
            CHECK(sphs_uniform_mass(s) == 0.008f);
            CHECK(sphs_cell_table_ready(s) == !r.table && sphs_can_scatter(s) == !r.table);
            CHECK(sphs_can_scan(s) == (stage == 1 && !r.table));
            CHECK(sphs_neighbours_ready(s) == !r.table);
            CHECK(sphs_obj_info_current(s) == !r.obj);
            CHECK(sphs_acc_complete(s) == (r.field == F_ACCELERATION));
            // the pure verdict itself is never touched by an upload (it is void while the uniform one is undecided)
            CHECK(sphs_pure_fluid(s, 1, 1000, false) == !r.uniform);
            if (r.table) { CHECK(hash(s) && scan(s)); CHECK(sphs_neighbours_ready(s)); }   // the order flag was left
        }
    }
}

static void window_change() {
    SphSetState s = pure_after_step(1000);
    sphs_obj_info_read(s);
    sphs_acc_interior_kept(s, true);
    sphs_window_changed(s);
    CHECK(!sphs_neighbours_ready(s) && !sphs_cell_table_ready(s) && !sphs_can_scan(s) && !sphs_can_scatter(s) && !sphs_dyn_known(s));
    CHECK(hash(s) && scan(s));
    CHECK(!sphs_neighbours_ready(s));                    // the order is dropped too
    CHECK(sphs_uniform(s) && sphs_pure_fluid(s, 1, 1000, false) && sphs_obj_info_current(s) && !sphs_acc_complete(s));   // the same set
}

static void device_error() {
    SphSetState s = pure_after_step(1000);
    sphs_obj_info_read(s);
    CHECK(hash(s));                                      // (the flag may be found between any two stages)
    sphs_device_error(s);
    CHECK(!sphs_neighbours_ready(s) && !sphs_cell_table_ready(s) && !sphs_can_scan(s) && !sphs_can_scatter(s));
    CHECK(sphs_dyn_count(s) == 0 && sphs_uniform(s) && sphs_pure_fluid(s, 1, 1000, false) && sphs_obj_info_current(s) && sphs_acc_complete(s));
    CHECK(sort(s, false, 0) && sphs_neighbours_ready(s));
}

static void slab_forces_fused() {
    SphSetState s = pure_after_step(1000);
    sphs_acc_interior_kept(s, false);                    // sph_slab_forces that could not fuse its interior advect
    CHECK(sphs_acc_complete(s));
    const int completes[3] = {0, 1, 2};                  // a full force pass, a step, an upload of the field
    for (int how : completes) {
        sphs_acc_interior_kept(s, true);
        CHECK(!sphs_acc_complete(s));
        CHECK(sort(s, true, 0));                         // the next slab step's sort, a select, an append: none completes it
        sphs_range_selected(s);
        sphs_appended(s, true);
        upload(s, F_V);
        CHECK(!sphs_acc_complete(s));
        if (how == 0) sphs_acc_written_all(s);           // sph_compute_non_pressure_forces
        if (how == 1) sphs_acc_written_all(s);           // step_loop with n_steps > 0
        if (how == 2) upload(s, F_ACCELERATION);
        CHECK(sphs_acc_complete(s));
    }
    sphs_acc_interior_kept(s, true);
    sphs_acc_interior_kept(s, false);                    // the next unfused slab force sweep writes them all
    CHECK(sphs_acc_complete(s));
}

static void uniform_check() {
    SphSetState s;
    sphs_init(s);
    CHECK(!sphs_uniform_decided(s) && !sphs_uniform(s) && sphs_uniform_mass(s) == 0.0f && !sphs_pure_fluid(s, 1, 0, false));
    CHECK(!sphs_pure_fluid(s, 2, 0, false));             // the host's word is for the instance, not for the uniform step
    decide_uniform(s, false, 0, 0.0f, 0.0f, 0, 0);       // N = 0
    CHECK(sphs_uniform_decided(s) && !sphs_uniform(s) && sphs_uniform_mass(s) == 0.0f && !sphs_pure_fluid(s, 1, 0, false));
    sphs_field_uploaded(s, F_M);
    decide_uniform(s, false, 1000, 0.008f, 0.009f, 0, 900);   // mixed masses
    CHECK(sphs_uniform_decided(s) && !sphs_uniform(s) && sphs_uniform_mass(s) == 0.0f && !sphs_pure_fluid(s, 2, 1000, false));
    sphs_field_uploaded(s, F_M);
    decide_uniform(s, false, 1000, 0.008f, 0.008f, 3, 900);   // one mass, but some fluid m_V differ from m_V0
    CHECK(sphs_uniform_decided(s) && !sphs_uniform(s));
    sphs_field_uploaded(s, F_M_V);
    decide_uniform(s, false, 1000, 0.008f, 0.008f, 0, 900);   // uniform with solids
    CHECK(sphs_uniform(s) && sphs_uniform_mass(s) == 0.008f && !sphs_pure_fluid(s, 1, 1000, false) && !sphs_pure_fluid(s, 1, 900, false));
    CHECK(sphs_pure_fluid(s, 2, 1000, true) && !sphs_pure_fluid(s, 0, 1000, false));
    decide_uniform(s, false, 1000, 0.5f, 0.5f, 0, 1000);      // decided: not checked again
    CHECK(sphs_uniform_mass(s) == 0.008f);
    sphs_field_uploaded(s, F_MATERIAL);
    decide_uniform(s, false, 1000, 0.008f, 0.008f, 0, 1000);  // pure
    CHECK(sphs_uniform(s) && sphs_pure_fluid(s, 1, 1000, false));
    CHECK(!sphs_pure_fluid(s, 1, 999, false) && !sphs_pure_fluid(s, 1, 1000, true) && !sphs_pure_fluid(s, 0, 1000, false));
    // the options rule the step out: only the verdict moves; deciding again starts from the check
    decide_uniform(s, true, 1000, 0.008f, 0.008f, 0, 1000);
    CHECK(sphs_uniform_decided(s) && !sphs_uniform(s) && sphs_uniform_mass(s) == 0.008f && !sphs_pure_fluid(s, 1, 1000, false));
    decide_uniform(s, false, 1000, 0.008f, 0.008f, 0, 1000);  // ("no" is a decision too: it stands until an option or an upload moves)
    CHECK(!sphs_uniform(s));
    sphs_option_changed(s, OPT_UNIFORM_FLUID);
    const int opts[4] = {OPT_GATHER_IMPL, OPT_NO_DYNAMIC_SOLIDS, OPT_SLAB_DROP_OUTSIDE, OPT_UNIFORM_FLUID};
    for (int o : opts) {
        refresh_dyn(s, false, 7);
        decide_uniform(s, false, 1000, 0.008f, 0.008f, 0, 1000);
        CHECK(sphs_uniform(s) && sphs_dyn_count(s) == 7);
        sphs_option_changed(s, o);
        CHECK(!sphs_uniform_decided(s));
        CHECK(sphs_dyn_known(s) == (o != OPT_NO_DYNAMIC_SOLIDS));
    }
    // a positive mass is what makes the verdict: zero-mass fluid is "no", with the count recorded
    SphSetState z;
    sphs_init(z);
    decide_uniform(z, false, 10, 0.0f, 0.0f, 0, 10);
    CHECK(sphs_uniform_decided(z) && !sphs_uniform(z) && !sphs_pure_fluid(z, 1, 10, false) && !sphs_pure_fluid(z, 2, 10, false));
}

int main(int argc, char** argv) {
    struct { const char* name; void (*fn)(); } all[] = {
        {"stand_alone_sort", stand_alone_sort}, {"step_then_truncate_append_same_n", step_then_truncate_append_same_n},
        {"append_vouched", append_vouched}, {"select_range", select_range}, {"count_set", count_set}, {"upload_table", upload_table},
        {"window_change", window_change}, {"device_error", device_error}, {"slab_forces_fused", slab_forces_fused},
        {"uniform_check", uniform_check},
    };
    int ran = 0;
    for (auto& t : all)
        if (argc < 2 || strcmp(argv[1], t.name) == 0) { t.fn(); ++ran; }
    if (ran == 0) { printf("FAIL: no scenario named %s\n", argc > 1 ? argv[1] : "?"); return 2; }
    printf("%s: %d scenario(s), %d failure(s)\n", g_fail ? "FAIL" : "PASS", ran, g_fail);
    return g_fail ? 1 : 0;
}
