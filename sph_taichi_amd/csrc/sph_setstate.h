// sph_setstate.h -- what the host knows about the particle SET, and how far the sort pipeline has got.
//
// Host only, no HIP: tests/setstate_driver.cpp runs the rules below on the CPU.  The fields of SphSetState are touched by
// the functions of this header and by nobody else; the API code reports EVENTS and asks QUESTIONS.
//
// The rules:
//   * The sort is hash -> scan -> scatter.  The hash leaves the keys and a histogram, the scan turns the histogram into the
//     cell table, the scatter consumes the keys and leaves the records in cell order.  The sweeps need the order AND the
//     cell table; the statistics and the layer offsets need the cell table alone.
//   * The number of dynamic rigid particles is counted by a sort that finds it unknown (-1), or vouched to be 0 by the host
//     (SPH_OPT_NO_DYNAMIC_SOLIDS).  Whatever may change which records are dynamic solids, or which records there are, makes
//     it unknown again.
//   * The uniform-fluid verdict (-1 not decided, 0 no, 1 yes with the one mass) is decided once per change of the masses,
//     the materials or the options it depends on.  The pure verdict ("no solid among exactly N particles") is only ever
//     set by a check of THIS set: whatever changes the set forgets it, even if a later call restores the count.
//   * The object info (counts and rest box per object) is one download of x_0 / ids / flags: an upload of any of those,
//     or a new count, asks for another.
//   * The acceleration array is incomplete after a slab force sweep that kept the interior targets' values to itself;
//     a full force pass, a step or an upload of the field completes it.
//
// What each event that changes the set or its cells leaves alone (x = forgotten, . = left as it is):
//
//   event                 keys+table  order  dyn count  obj info  uniform  pure   why the gaps
//   sphs_count_set            x         .       x          x         .       x    order: nobody reads it without the table
//   sphs_range_selected       x         x       x          .         .       x    a subset of a uniform set is uniform
//   sphs_truncated            .         .     x (1)        .         .     x (2)  only trailing records go (the strays a slab
//                                                                                 rank sorted behind every cell): order and
//                                                                                 table of the rest stand
//   sphs_appended             x         x       x          .       x (3)     x    (3) not if the caller vouches for the mass;
//                                                                                 vouching is for the MASS only: arrivals
//                                                                                 may be solids, so the pure verdict goes
//   sphs_window_changed       x         x       x          .         .       .    every cell id changes meaning; the set is
//                                                                                 the same set
//   sphs_field_uploaded     x (X)       .     x (4)      x (5)     x (6)     .    per field, see the function
//   sphs_device_error         x         x       .          .         .       .    the sort is void, the set is not
//     (1) only if the count changed and the host does not vouch for "no dynamic solids" (the vouched count is 0 for any set)
//     (2) only if the count changed    (4) material, is_dynamic, density (the scale of the rigid sums)
//     (5) x_0, object id, material, is_dynamic, pid    (6) material, m, m_V
//   None of them completes the acceleration array, and the mass of a forgotten uniform verdict stays in its field.
#pragma once

// the field and option ids the tables below speak of (sph_internal.h ties them to SPH_F_* / SPH_OPT_* of sph_hip.h)
enum {
    SPHS_F_OBJECT_ID = 0, SPHS_F_X = 1, SPHS_F_X_0 = 2, SPHS_F_M_V = 5, SPHS_F_M = 6, SPHS_F_DENSITY = 7, SPHS_F_MATERIAL = 9,
    SPHS_F_IS_DYNAMIC = 11, SPHS_F_PID = 14,
    SPHS_OPT_GATHER_IMPL = 0, SPHS_OPT_NO_DYNAMIC_SOLIDS = 4, SPHS_OPT_SLAB_DROP_OUTSIDE = 6, SPHS_OPT_UNIFORM_FLUID = 7
};

struct SphSetState {
    bool have_keys;       // the hash pass left keys and a histogram that no scatter has consumed
    bool have_prefix;     // the cell table is the scan of that histogram
    bool sorted;          // the records are in cell order
    int n_dyn_host;       // dynamic rigid particles (length of dyn_list); -1 = recount at the next sort
    bool obj_info_valid;  // obj_info[] describes the current x_0 / object ids / flags
    int uniform_state;    // -1 not decided, 0 the precondition of the uniform-fluid step fails, 1 holds (m_uniform valid)
    float m_uniform;
    int pure_fluid;       // (with uniform_state == 1) the check found no solid at all among pure_fluid_n particles: every
    int pure_fluid_n;     //   m_V is m_V0 bit for bit (single context only: a slab rank's arrivals are never checked)
    bool acc_partial;     // the last slab force sweep consumed the interior targets' accelerations and never wrote them out
};

// ---- events ----------------------------------------------------------------------------------------------------------
static inline void sphs_init(SphSetState& s) {
    s.have_keys = s.have_prefix = s.sorted = s.obj_info_valid = s.acc_partial = false;
    s.n_dyn_host = -1;  // unknown until material / is_dynamic are uploaded
    s.uniform_state = -1; s.m_uniform = 0.0f;
    s.pure_fluid = 0; s.pure_fluid_n = -1;
}
static inline void sphs_forget_sort(SphSetState& s) { s.have_keys = s.have_prefix = s.sorted = false; }
static inline void sphs_forget_pure(SphSetState& s) { s.pure_fluid = 0; s.pure_fluid_n = -1; }
// sph_set_particle_count / sph_select_range: another count / another window of the records
static inline void sphs_count_set(SphSetState& s) { s.n_dyn_host = -1; s.obj_info_valid = false; sphs_forget_pure(s); s.have_keys = s.have_prefix = false; }
static inline void sphs_range_selected(SphSetState& s) { sphs_forget_pure(s); sphs_forget_sort(s); s.n_dyn_host = -1; }
// sph_truncate: trailing records dropped (changed: the count moved; no_dynamic: the host vouches for a count of 0)
static inline void sphs_truncated(SphSetState& s, bool changed, bool no_dynamic) {
    if (changed && !no_dynamic) s.n_dyn_host = -1;  // the sort's list skipped the dropped strays: recount
    if (changed) sphs_forget_pure(s);               // a truncate + append that restores N may bring solids in
}
// sph_append_records: arrivals are unchecked unless the caller vouches for them (SPH_OPT_UNIFORM_FLUID 1)
static inline void sphs_appended(SphSetState& s, bool caller_vouches_uniform) {
    if (!caller_vouches_uniform) s.uniform_state = -1;
    sphs_forget_pure(s);
    sphs_forget_sort(s);
    s.n_dyn_host = -1;
}
static inline void sphs_window_changed(SphSetState& s) { sphs_forget_sort(s); s.n_dyn_host = -1; }
// sph_upload of a per-particle field, once the copy has succeeded
static inline void sphs_field_uploaded(SphSetState& s, int f) {
    if (f == SPHS_F_MATERIAL || f == SPHS_F_IS_DYNAMIC || f == SPHS_F_DENSITY) s.n_dyn_host = -1;
    if (f == SPHS_F_MATERIAL || f == SPHS_F_M || f == SPHS_F_M_V) s.uniform_state = -1;
    if (f == SPHS_F_X) s.have_keys = s.have_prefix = false;
    if (f == SPHS_F_X_0 || f == SPHS_F_OBJECT_ID || f == SPHS_F_MATERIAL || f == SPHS_F_IS_DYNAMIC || f == SPHS_F_PID) s.obj_info_valid = false;
}
// sph_set_option of one of the four options the verdicts depend on
static inline void sphs_option_changed(SphSetState& s, int which) {
    if (which == SPHS_OPT_NO_DYNAMIC_SOLIDS) s.n_dyn_host = -1;
    s.uniform_state = -1;
}
static inline void sphs_hashed(SphSetState& s) { s.have_keys = true; s.have_prefix = false; }
static inline void sphs_scanned(SphSetState& s) { s.have_prefix = true; }
static inline void sphs_scattered(SphSetState& s) { s.have_keys = false; s.sorted = true; }  // the histogram offsets are consumed
static inline void sphs_device_error(SphSetState& s) { sphs_forget_sort(s); }
// the options rule the uniform-fluid step out, whatever the particles are (the mass and the pure verdict stay as they were)
static inline void sphs_uniform_ruled_out(SphSetState& s) { s.uniform_state = 0; }
// the device-side check: "no" until it finds fluid particles of one mass m whose m_V all equal m_V0
static inline void sphs_uniform_check_begun(SphSetState& s) { s.uniform_state = 0; sphs_forget_pure(s); s.m_uniform = 0.0f; }
static inline void sphs_uniform_checked(SphSetState& s, float m, unsigned n_fluid, int N) {
    s.m_uniform = m;
    s.uniform_state = m > 0.0f ? 1 : 0;
    s.pure_fluid = (s.uniform_state == 1 && n_fluid == (unsigned)N) ? 1 : 0;  // every particle is a fluid particle => no solid at all
    s.pure_fluid_n = N;
}
static inline void sphs_dyn_counted(SphSetState& s, int n) { s.n_dyn_host = n; }
static inline void sphs_obj_info_read(SphSetState& s) { s.obj_info_valid = true; }
static inline void sphs_acc_written_all(SphSetState& s) { s.acc_partial = false; }
static inline void sphs_acc_interior_kept(SphSetState& s, bool fused) { s.acc_partial = fused; }

// ---- questions -------------------------------------------------------------------------------------------------------
static inline bool sphs_can_scan(const SphSetState& s) { return s.have_keys; }
static inline bool sphs_can_scatter(const SphSetState& s) { return s.have_prefix; }
static inline bool sphs_cell_table_ready(const SphSetState& s) { return s.have_prefix; }  // statistics, layer offsets
static inline bool sphs_neighbours_ready(const SphSetState& s) { return s.sorted && s.have_prefix; }
static inline bool sphs_dyn_known(const SphSetState& s) { return s.n_dyn_host >= 0; }
static inline int sphs_dyn_count(const SphSetState& s) { return s.n_dyn_host; }  // -1: not known
static inline bool sphs_obj_info_current(const SphSetState& s) { return s.obj_info_valid; }
static inline bool sphs_uniform_decided(const SphSetState& s) { return s.uniform_state >= 0; }
static inline bool sphs_uniform(const SphSetState& s) { return s.uniform_state == 1; }
static inline float sphs_uniform_mass(const SphSetState& s) { return s.m_uniform; }
// May the sweeps of the uniform-fluid step run their pure-fluid instances?  ONE rule for both (density + EOS, one-gather
// force): the device-side check found no solid among exactly the N particles the context holds now (single context), or the
// HOST vouches that the whole scene holds no solid particle (SPH_OPT_PURE_FLUID_INSTANCE 2: a slab rank, whose arrivals are
// never checked; every particle of such a scene keeps m_V = m_V0 bit for bit wherever it lives).  0 is the A/B switch.
static inline bool sphs_pure_fluid(const SphSetState& s, int opt_pure_instance, int N, bool drop_outside) {
    const bool pure_checked = opt_pure_instance == 1 && s.pure_fluid && s.pure_fluid_n == N && !drop_outside;
    return s.uniform_state == 1 && (pure_checked || opt_pure_instance == 2);
}
static inline bool sphs_acc_complete(const SphSetState& s) { return !s.acc_partial; }
