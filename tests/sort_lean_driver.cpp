// "Where the persistent id lives" (sph_taichi_amd/csrc/sph_derived.h: pid_apart, with the pure-fluid rule of sph_setstate.h),
// executed on the CPU: tests/test_sort_lean_state.py compiles this file with the host compiler and runs one scenario per test
// case.  The model below keeps the two aux sets and the two pid arrays of a context of N records as plain arrays and issues the
// header's events in the order sph_sort.hip / sph_gather.hip / sph_api.hip do: a sort permutes whichever array the header says
// carries the ids and leaves the other set's stale words in place, the fold writes aux back.  After every call order a reader
// that asks the way the launch code asks (fold on demand, then aux) must find every particle's own id and the uniform mass.
#include <stdio.h>
#include <string.h>

#include "sph_derived.h"
#include "sph_setstate.h"

static int g_fail = 0;
#define CHECK(expr)                                                            \
    do {                                                                       \
        if (!(expr)) { printf("FAIL line %d: %s\n", __LINE__, #expr); ++g_fail; } \
    } while (0)

enum { N = 7 };
static const float M0 = 0.008f;
static const SphPartKey K{4242, 0, 64, 0, 0};

struct Model {
    SphDerived dv{};
    SphSetState ss;
    int opt_lean = 1, opt_pure = 1, n = N, cur = 0, folds = 0, lean_sorts = 0, entering = 0;
    float aux_m[2][N];   // aux.x
    int aux_id[2][N];    // aux.w
    int pid[2][N];
    int truth[N];        // the id of the record at each place of the current order
    float truth_m[N];
    unsigned rng = 12345u;

    Model() {
        sphs_init(ss);
        for (int s = 0; s < 2; ++s)
            for (int i = 0; i < N; ++i) { aux_m[s][i] = 0.0f; aux_id[s][i] = i; pid[s][i] = -1000 - i; }   // k_init_pid; the pid arrays hold nothing
        for (int i = 0; i < N; ++i) { truth[i] = i; truth_m[i] = M0; aux_m[0][i] = M0; }
    }
    // sphk_check_uniform_fluid of a set of fluid particles of one mass
    void check_uniform(bool all_fluid) {
        ensure_pid();
        sphs_uniform_check_begun(ss);
        sphs_uniform_checked(ss, M0, all_fluid ? (unsigned)n : (unsigned)n - 1u, n);
    }
    // sph_ensure_aux
    void ensure_aux() {
        if (!sphd_aux_needs_fold(dv)) return;
        const bool apart = sphd_pid_apart(dv);
        sphd_aux_folded(dv);
        if (apart) {
            ++folds;
            for (int i = 0; i < n; ++i) { aux_m[cur][i] = sphs_uniform_mass(ss); aux_id[cur][i] = pid[cur][i]; }
        }
    }
    void ensure_pid() { if (sphd_pid_apart(dv)) ensure_aux(); }
    // hash + scan + scatter of a step of sph_step (fast: the order is a sort's output) or of a stand-alone sort
    void sort(bool in_fused_step, bool sort_acc = false) {
        const bool fast = sphd_sort_fast_usable(dv, true, false, false);
        sphd_hash_started(dv);
        const bool lean = sphd_sort_lean_usable(dv, opt_lean != 0, fast, sphs_pure_fluid(ss, opt_pure, n, false), in_fused_step, sort_acc);
        if (!lean) ensure_pid();
        const int form = sphd_scatter_form(dv, lean);
        int perm[N];
        for (int i = 0; i < n; ++i) perm[i] = i;
        for (int i = n - 1; i > 0; --i) {   // dst of every old index: any permutation will do
            rng = rng * 1664525u + 1013904223u;
            const int j = (int)((rng >> 8) % (unsigned)(i + 1)), t = perm[i];
            perm[i] = perm[j]; perm[j] = t;
        }
        const int o = cur ^ 1;
        int t_id[N]; float t_m[N];
        for (int i = 0; i < n; ++i) {
            const int dst = perm[i];
            if (form == 0) { aux_m[o][dst] = aux_m[cur][i]; aux_id[o][dst] = aux_id[cur][i]; }
            if (form == 1) pid[o][dst] = pid[cur][i];
            if (form == 2) pid[o][dst] = aux_id[cur][i];
            t_id[dst] = truth[i]; t_m[dst] = truth_m[i];
        }
        memcpy(truth, t_id, sizeof(int) * n); memcpy(truth_m, t_m, sizeof(float) * n);
        cur = o;
        if (lean) { sphd_scattered_lean(dv); ++lean_sorts; entering += form == 2; }
        sphd_sorted(dv, true, K);
        sphd_order_established(dv, false);
    }
    // the density sweep of the fused uniform-fluid step (density / pressure stay in eos2)
    void density() { sphd_lists_written(dv, sphs_uniform(ss) ? 1 : 0); }
    void step() { sort(true); density(); }
    // a reader of m and the id: sph_download, an observer, a stand-alone kernel
    bool read_ok() {
        ensure_pid();
        for (int i = 0; i < n; ++i)
            if (aux_id[cur][i] != truth[i] || aux_m[cur][i] != truth_m[i]) return false;
        return true;
    }
    // sph_upload of m (k_insert reads the id and writes aux fields: the launcher folds first)
    void upload_m(float m) {
        ensure_pid();
        for (int i = 0; i < n; ++i) aux_m[cur][i] = truth_m[i] = m;
        sphd_records_moved(dv);
        sphs_field_uploaded(ss, SPHS_F_M);
    }
    // sph_truncate
    void truncate(int k) {
        sphs_truncated(ss, k != n, false);
        sphd_records_moved(dv);
        n = k;
    }
    // sph_set_particle_count
    void set_count(int k) {
        ensure_pid();
        n = k;
        sphs_count_set(ss);
        sphd_set_changed(dv);
    }
};

// general sort, verdict, then lean sorts: the first finds the ids in aux, the later ones in the pid array; no fold in between
static void enter() {
    Model m;
    m.sort(false, true);                               // initialize(): general, moves aux
    CHECK(!sphd_pid_apart(m.dv) && m.lean_sorts == 0);
    m.sort(true); m.density();                         // first step: the verdict is not in yet
    CHECK(m.lean_sorts == 0 && !sphd_pid_apart(m.dv));
    m.check_uniform(true);
    for (int k = 0; k < 5; ++k) m.step();
    CHECK(m.lean_sorts == 5 && m.entering == 1 && m.folds == 0);
    CHECK(sphd_pid_apart(m.dv) && sphd_aux_needs_fold(m.dv));
    CHECK(m.aux_id[m.cur][0] != m.truth[0] || m.aux_id[m.cur][1] != m.truth[1] || m.aux_id[m.cur][2] != m.truth[2] ||
          m.aux_id[m.cur][3] != m.truth[3]);           // (aux really is stale: the model would notice a missing fold)
    CHECK(m.read_ok() && m.folds == 1);
}

// the fold writes the whole record once; a second demand does nothing
static void fold() {
    Model m;
    m.sort(false, true); m.check_uniform(true);
    m.step(); m.step();
    CHECK(sphd_aux_in_eos2(m.dv) && sphd_pid_apart(m.dv));
    m.ensure_aux();
    CHECK(!sphd_aux_in_eos2(m.dv) && !sphd_pid_apart(m.dv) && !sphd_aux_needs_fold(m.dv) && m.folds == 1);
    m.ensure_aux(); m.ensure_pid();
    CHECK(m.folds == 1 && m.read_ok());
    // the switch off, and the other conditions one at a time: never lean
    Model a; a.opt_lean = 0; a.sort(false, true); a.check_uniform(true); a.step(); a.step();
    CHECK(a.lean_sorts == 0 && !sphd_pid_apart(a.dv) && a.read_ok() && a.folds == 0);
    Model b; b.sort(false, true); b.check_uniform(false); b.step(); b.step();          // one solid among them
    CHECK(b.lean_sorts == 0 && b.read_ok() && b.folds == 0);
    Model c; c.sort(false, true); c.check_uniform(true); c.sort(false); c.sort(true, true);   // not the fused step; accelerations too
    CHECK(c.lean_sorts == 0 && c.read_ok());
    SphDerived s{};
    CHECK(!sphd_sort_lean_usable(s, true, false, true, true, false));                  // the general sort
    CHECK(sphd_sort_lean_usable(s, true, true, true, true, false));
}

// after a fold the next step enters again, through aux.w
static void re_enter() {
    Model m;
    m.sort(false, true); m.check_uniform(true);
    m.step(); m.step();
    CHECK(m.read_ok() && m.folds == 1 && m.entering == 1);
    m.step();
    CHECK(m.entering == 2 && sphd_pid_apart(m.dv));
    m.step(); m.step();
    CHECK(m.entering == 2 && m.lean_sorts == 5);
    CHECK(m.read_ok() && m.folds == 2);
    // a stand-alone sort (sph_sort / sph_counting_sort call sph_ensure_aux first) between lean steps
    m.step();
    m.ensure_aux(); m.sort(false, true);
    CHECK(m.folds == 3 && !sphd_pid_apart(m.dv) && m.read_ok() && m.folds == 3);
    m.step();
    CHECK(m.entering == 4);
}

// the set changes while the ids live apart: the pure verdict goes, so the next sort is not lean and asks for the fold itself;
// sphd_set_changed alone never forgets where the ids are
static void set_change_while_lean() {
    Model m;
    m.sort(false, true); m.check_uniform(true);
    m.step(); m.step();
    m.truncate(N - 2);                                 // no fold at the event ...
    CHECK(sphd_pid_apart(m.dv) && m.folds == 0);
    m.step();                                          // ... the general sort behind it folds, then moves aux
    CHECK(m.folds == 1 && !sphd_pid_apart(m.dv) && m.lean_sorts == 2);
    CHECK(m.read_ok());
    m.check_uniform(true);                             // the step's density phase decides again: lean again
    m.step(); m.step();
    CHECK(m.lean_sorts == 4 && m.read_ok());
    m.step();
    m.set_count(N - 3);                                // re-based records: folded at the old count first
    CHECK(m.folds == 3 && !sphd_pid_apart(m.dv) && m.read_ok());
    SphDerived s{};
    sphd_scattered_lean(s);
    sphd_set_changed(s); sphd_invalidate(s); sphd_records_moved(s); sphd_sorted(s, true, K);
    CHECK(sphd_pid_apart(s) && sphd_aux_needs_fold(s));
    sphd_aux_folded(s);
    CHECK(!sphd_pid_apart(s));
    // the A/B switch turned off in the middle of a run
    Model o;
    o.sort(false, true); o.check_uniform(true); o.step(); o.step();
    o.opt_lean = 0;
    o.step();
    CHECK(o.folds == 1 && !sphd_pid_apart(o.dv) && o.read_ok());
}

// an upload of m while the ids live apart: the old mass is folded in first, the new one is honoured, the verdict is made again
static void upload_while_lean() {
    Model m;
    m.sort(false, true); m.check_uniform(true);
    m.step(); m.step(); m.step();
    m.upload_m(0.004f);
    CHECK(m.folds == 1 && !sphd_pid_apart(m.dv) && !sphs_uniform_decided(m.ss));
    CHECK(m.read_ok() && m.aux_m[m.cur][0] == 0.004f);
    m.step();                                          // general sort (records overwritten from the host), no verdict yet
    CHECK(m.lean_sorts == 3 && m.read_ok() && m.aux_m[m.cur][0] == 0.004f);
    // the check's launcher folds BEFORE the verdict's mass is forgotten
    Model c;
    c.sort(false, true); c.check_uniform(true); c.step(); c.step();
    sphs_option_changed(c.ss, SPHS_OPT_UNIFORM_FLUID);
    c.check_uniform(true);
    CHECK(c.folds == 1 && c.read_ok() && c.aux_m[c.cur][0] == M0);
}

int main(int argc, char** argv) {
    struct { const char* name; void (*fn)(); } all[] = {
        {"enter", enter}, {"fold", fold}, {"re_enter", re_enter}, {"set_change_while_lean", set_change_while_lean},
        {"upload_while_lean", upload_while_lean},
    };
    int ran = 0;
    for (auto& t : all)
        if (argc < 2 || strcmp(argv[1], t.name) == 0) { t.fn(); ++ran; }
    if (ran == 0) { printf("FAIL: no scenario named %s\n", argc > 1 ? argv[1] : "?"); return 2; }
    printf("%s: %d scenario(s), %d failure(s)\n", g_fail ? "FAIL" : "PASS", ran, g_fail);
    return g_fail ? 1 : 0;
}
