// sph_derived.h -- which derived device buffers still describe the current particle state.
//
// Host only, no HIP: tests/derived_state_driver.cpp runs the rules below on the CPU.  The fields of SphDerived are
// touched by the functions of this header and by nobody else; the launch code reports EVENTS and asks QUESTIONS.
//
// The rules:
//   * The neighbour lists (glist / gcnt) hold offsets into the tile of the brick that wrote them, so they belong to the
//     partition (brick_list) they were written over.  Whatever replaces the cached partition drops the lists, and the
//     column records (brick_rec) and staging records with them.
//   * The column records serve only a reader whose target ranges are exactly the writer's (a subset sweep -- slab
//     mode -- has other target tables); the lists serve every reader the cached partition serves.
//   * What survives sphd_invalidate(), on purpose:
//       gcnt_written      sph_get_stats after a step reports the last density sweep's list lengths although the advect
//                         has moved the particles since; only a sort (which reorders gcnt's index space) ends that.
//       aux_stale         density / pressure in eos2 stay the values of their particles when positions or options
//                         change; a sort or a new record selection (other indices) ends that.
//       df_bpart_valid    set and consumed inside one solver iteration, with nothing in between.
//       brick_count_zero  describes the counter, not the particles.
//       pid_apart         says where the ids ARE; it also survives sphd_set_changed() and a sort (see the lean scatter below).
//   * The fast sort (sph_sort.hip: stayers ranked from the previous order) reads the previous sort's keys and cell array as
//     the description of the CURRENT order.  That holds from a sort until records are moved, inserted, dropped, re-selected
//     or overwritten from the host, or the grid window changes (sphd_records_moved); positions drifting under the advect do
//     not end it -- that drift is what the next sort measures.  A sort that hashed strays into the virtual cell G leaves an
//     order the fast path has no rule for.
//   * The LEAN scatter (SPH_OPT_SORT_LEAN: sph_sort.hip, k_stable_scatter_fast's lean forms) moves the persistent id through
//     an array of its own and leaves the aux record behind: on a pure-fluid uniform step m is one known value, density and
//     pressure live in eos2, and the id is the record's only live word.  From the first lean scatter on, "the ids live
//     apart": aux of the current order holds nothing current, and only the fold (sph_ensure_aux: m, density, pressure and
//     id written back as one record) ends that.  Nothing else does: not a sort, not a change of the set, not an option --
//     whoever reads or writes aux, re-bases or resizes the set, or sorts any other way asks for the fold FIRST
//     (sphd_aux_needs_fold / sphd_pid_apart), so a forgotten demand leaves a pending fold, never a lost id.
#pragma once

// identity of a brick partition: the cut rule and the target x-layer ranges it was cut for
struct SphPartKey {
    int id;                // footprint, cut rule, limits
    int lo, hi, lo2, hi2;  // target layers [lo, hi) u [lo2, hi2)
    bool operator==(const SphPartKey& o) const { return id == o.id && lo == o.lo && hi == o.hi && lo2 == o.lo2 && hi2 == o.hi2; }
    // both ranges lie inside the SINGLE range of `o`: bricks listed for `o` that hold no target of ours leave at T == 0
    bool inside(const SphPartKey& o) const {
        const bool in1 = lo >= o.lo && hi <= o.hi;
        const bool in2 = lo2 == hi2 || (lo2 >= o.lo && hi2 <= o.hi);
        return id == o.id && o.lo2 == o.hi2 && in1 && in2;
    }
};

enum SphPartHit { SPH_PART_NO = 0, SPH_PART_SUBSET = 1, SPH_PART_EXACT = 2 };

struct SphDerived {
    bool lists_valid;       // glist / gcnt describe the current positions and order, over the cached partition
    bool gcnt_written;      // gcnt was written by a brick density sweep since the last sort
    int stg_kind;           // what stg / gat hold for the current positions: 0 nothing, 1 the WCSPH records of
                            // GM_DENSITY_EOS, 2 the DFSPH record (x, y, z, +m_V fluid / -m_V solid) of GM_DF_DENSITY
    int k_kind;             // gat-as-float holds k_j = b_j * factor_j: 0 no, 1 b = density_adv, 2 b = density_adv - 1
    bool bricks_valid;      // brick_list / brick_count describe the current order for bricks_key
    SphPartKey bricks_key;
    bool brec_valid;        // brick_rec describes the current lists for a reader of brec_key
    SphPartKey brec_key;
    bool df_bpart_valid;    // the refresh sweep of this solver iteration left its per-brick density-error partials
    bool aux_stale;         // density / pressure of the fluid live in eos2 (lean density finish), not yet in aux
    bool brick_count_zero;  // brick_count is zero (hash kernel) and no list has been built into it since
    bool order_from_sort;   // the current record order is a sort's output under the current key and cell arrays, without strays in cell G
    bool pid_apart;         // the persistent ids of the current order live in the pid array (lean scatter), not in aux
};

// ---- events ----------------------------------------------------------------------------------------------------------
// positions, flags, the particle set or an option the sweeps' instances depend on changed; also the scan's error flag
static inline void sphd_invalidate(SphDerived& s) { s.lists_valid = s.bricks_valid = s.brec_valid = false; s.stg_kind = s.k_kind = 0; }
// ... and the records were re-based (sph_set_particle_count, sph_select_range): eos2 is indexed from the old first record
static inline void sphd_set_changed(SphDerived& s) { sphd_invalidate(s); s.aux_stale = false; s.order_from_sort = false; }
// records were overwritten from the host, appended, dropped, or the cell ids changed meaning: the previous sort's keys and
// cell array no longer describe the current order
static inline void sphd_records_moved(SphDerived& s) { s.order_from_sort = false; }
// a sort has been enqueued; `built`: its place kernel cut the step's partition under `key` (into the zeroed counter)
static inline void sphd_sorted(SphDerived& s, bool built, const SphPartKey& key) {
    sphd_set_changed(s);  // (eos2 is in the old order: whoever needed density / pressure called sph_ensure_aux before)
    s.gcnt_written = false;
    s.brick_count_zero = false;
    s.bricks_valid = built;
    if (built) s.bricks_key = key;
}
// a hash pass has been enqueued: the current cell array is a histogram in the making, no longer the last sort's
static inline void sphd_hash_started(SphDerived& s) { s.order_from_sort = false; }
// ... and that sort ran to its end: its output order, keys and cell array stand (strays: it hashed with drop_outside on)
static inline void sphd_order_established(SphDerived& s, bool strays_possible) { s.order_from_sort = !strays_possible; }
// a sweep cut a partition of its own into the main stream's list: the lists of the old one cannot be read through it
static inline void sphd_partition_rebuilt(SphDerived& s, const SphPartKey& key) {
    s.lists_valid = s.brec_valid = false;
    s.brick_count_zero = false;
    s.bricks_valid = true;
    s.bricks_key = key;
}
// a list-writing sweep ran; stg_kind = the staging records it left (1 comes with density / pressure in eos2 only)
static inline void sphd_lists_written(SphDerived& s, int stg_kind) {
    s.lists_valid = s.gcnt_written = true;
    s.stg_kind = stg_kind;
    s.k_kind = 0;
    if (stg_kind == 1) s.aux_stale = true;
}
// ... and left its column records, for readers of exactly `key` (stream order: every later sweep runs behind it)
static inline void sphd_records_written(SphDerived& s, const SphPartKey& key) { s.brec_valid = true; s.brec_key = key; }
// k_j written by a density-change (1) / density-advection (2) sweep, or stale (0: the cell walk, sphk_df_scale_factor)
static inline void sphd_k_written(SphDerived& s, int kind) { s.k_kind = kind; }
static inline void sphd_bpart_written(SphDerived& s) { s.df_bpart_valid = true; }
static inline void sphd_bpart_consumed(SphDerived& s) { s.df_bpart_valid = false; }
// the fold wrote the whole aux record of every particle: (m, density, pressure, id) are where every reader looks for them
static inline void sphd_aux_folded(SphDerived& s) { s.aux_stale = false; s.pid_apart = false; }
// a lean scatter has been enqueued: it moved the ids through the pid array and left aux behind
static inline void sphd_scattered_lean(SphDerived& s) { s.pid_apart = true; }
static inline void sphd_count_zeroed(SphDerived& s, bool zero) { s.brick_count_zero = zero; }

// ---- questions -------------------------------------------------------------------------------------------------------
static inline SphPartHit sphd_partition_hit(const SphDerived& s, const SphPartKey& key) {
    if (!s.bricks_valid) return SPH_PART_NO;
    return key == s.bricks_key ? SPH_PART_EXACT : key.inside(s.bricks_key) ? SPH_PART_SUBSET : SPH_PART_NO;
}
static inline bool sphd_lists_usable(const SphDerived& s) { return s.lists_valid; }
static inline bool sphd_records_usable(const SphDerived& s, const SphPartKey& key) { return s.lists_valid && s.brec_valid && key == s.brec_key; }
// the one-gather sweeps: lists current and the staging records of the right kind (DFSPH: and k_j of the right kind)
static inline bool sphd_one_gather_wcsph(const SphDerived& s) { return s.lists_valid && s.stg_kind == 1; }
static inline bool sphd_one_gather_df(const SphDerived& s, int k_kind) { return s.lists_valid && s.stg_kind == 2 && s.k_kind == k_kind; }
static inline bool sphd_stats_have_lists(const SphDerived& s) { return s.gcnt_written; }
static inline bool sphd_bpart_ready(const SphDerived& s) { return s.df_bpart_valid; }
static inline bool sphd_aux_in_eos2(const SphDerived& s) { return s.aux_stale; }
static inline bool sphd_pid_apart(const SphDerived& s) { return s.pid_apart; }
// does aux lack anything a reader may look for in it (density / pressure still in eos2, the ids still apart)?
static inline bool sphd_aux_needs_fold(const SphDerived& s) { return s.aux_stale || s.pid_apart; }
static inline bool sphd_count_is_zero(const SphDerived& s) { return s.brick_count_zero; }
// may the next sort rank stayers from the previous order (SPH_OPT_SORT_FAST)?  Only under the reference's intra-cell order
// (previous index) and without the virtual cell
static inline bool sphd_sort_fast_usable(const SphDerived& s, bool opt_fast, bool sort_by_pid, bool drop_outside) {
    return opt_fast && s.order_from_sort && !sort_by_pid && !drop_outside;
}
// may this fast scatter be a lean one (SPH_OPT_SORT_LEAN)?  pure_uniform: the rule that admits the pure-fluid instances of
// both sweeps holds, so m is the one uniform mass; aux_dead_in_step: the step this sort heads is the fused uniform-fluid
// WCSPH step, whose sweeps neither read nor write aux, and no in-step consumer of aux is armed; sort_acc: the caller wants
// the accelerations moved too (a stand-alone sort: its caller may read any field next).  The fast sort already excludes
// sort_by_pid and the virtual cell.
static inline bool sphd_sort_lean_usable(const SphDerived&, bool opt_lean, bool fast, bool pure_uniform, bool aux_dead_in_step, bool sort_acc) {
    return opt_lean && fast && pure_uniform && aux_dead_in_step && !sort_acc;
}
// 0: the scatter moves aux; 1: lean, the ids come from the pid array; 2: lean, the ids come from aux.w (entering)
static inline int sphd_scatter_form(const SphDerived& s, bool lean) { return !lean ? 0 : s.pid_apart ? 1 : 2; }
