/*
 * sph_hip.h -- C ABI of libsph_hip.so: the MI355X (gfx950) WCSPH step (and, at the end of the file,
 * the DFSPH step on the same neighbour machinery).
 *
 * The reference (erizmr/SPH_Taichi) has no FFI layer: its device code is
 * Taichi @ti.kernel Python.  This header is the boundary a maintainer binds
 * (ctypes) to replace each kernel of the hot path.  Every
 * entry point names the reference kernel it replaces (paths relative to the
 * reference root).  Plain pointers and sizes only; no torch / C++ types.
 *
 * Contract
 *  - One opaque context per GPU.  The context owns every device buffer and
 *    (unless a stream is handed to sph_create) one HIP stream.  A context is driven by
 *    one host thread at a time.
 *  - Compute entry points ENQUEUE on the context's stream and return;
 *    sph_download / sph_sync / sph_get_timings / sph_layer_offsets synchronise (and the DFSPH solver loops,
 *    once per iteration, like the reference's compute_density_error).
 *  - Every function returns 0 on success, a negative SPH_E_* code or a positive
 *    hipError_t otherwise; sph_last_error(ctx) gives the message.  Nothing
 *    throws.
 *  - Array layout at the boundary is the reference's (particle_system.py:
 *    101-113): vectors [N,3] f32 row-major, scalars [N] f32, ints [N] i32,
 *    color [N,3] i32.  The SoA/float4 packing inside is private.
 *  - Particle order: after sph_counting_sort / sph_step every array is in the
 *    reference's cell-sorted order with the STABLE intra-cell order a serial
 *    run of particle_system.py:322-330 produces.
 */
#ifndef SPH_HIP_H
#define SPH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPH_ABI_VERSION 6

typedef struct SphContext SphContext;

/* Scalars of ParticleSystem.__init__ (particle_system.py:17-46), SPHBase.__init__
 * (sph_base.py:8-21) and WCSPHSolver.__init__ (WCSPH.py:6-16).  Constants that
 * the reference folds in Python f64 before they enter a kernel (k_w, k_dw,
 * visc_d_nu, visc_eps) are passed already folded, as f32. */
typedef struct SphParams {
    int32_t n_particles;        /* particle_max_num              particle_system.py:83 */
    int32_t capacity;           /* >= n_particles; slack for halo/migration (multi-GPU) */
    int32_t grid_num[3];        /* LOCAL grid dims               particle_system.py:44 */
    int32_t cell_origin[3];     /* global cell coord of local cell (0,0,0); 0 on one GPU */
    int32_t n_objects;          /* len(rigid_rest_cm)            particle_system.py:93 */
    int32_t cold_capacity;      /* rows of the pid-indexed x_0 / color store; 0 = capacity (slabs: global N) */
    float grid_size;            /* = support_radius              particle_system.py:43 */
    float support_radius;       /* 4 r                           particle_system.py:37 */
    float particle_diameter;    /* 2 r                           particle_system.py:36 */
    float m_V0;                 /* 0.8 d^3                       particle_system.py:38 */
    float density_0;            /* sph_base.py:18 */
    float stiffness;            /* WCSPH.py:13 */
    float exponent;             /* WCSPH.py:10 */
    float viscosity;            /* sph_base.py:15 */
    float surface_tension;      /* WCSPH.py:15 */
    float dt;                   /* WCSPH.py:16 */
    float g[3];                 /* sph_base.py:13 */
    float domain_size[3];       /* particle_system.py:22 */
    float padding;              /* particle_system.py:46 */
    float wall_hi[3];           /* domain_size - padding, folded in f64 (sph_base.py:153-170) */
    float k_w;                  /* 8/pi/h^3          sph_base.py:33-35 */
    float k_dw;                 /* 6*8/pi/h^3        sph_base.py:57 */
    float visc_d_nu;            /* 2(dim+2)*viscosity WCSPH.py:104,112 */
    float visc_eps;             /* 0.01 h^2          WCSPH.py:113 */
} SphParams;

/* Per-particle arrays of particle_system.py:101-113, 138 (+ the grid counter
 * array :96 and a persistent particle id that the reference does not have). */
enum SphField {
    SPH_F_OBJECT_ID = 0,          /* i32 [N]   */
    SPH_F_X = 1,                  /* f32 [N,3] */
    SPH_F_X_0 = 2,                /* f32 [N,3] */
    SPH_F_V = 3,                  /* f32 [N,3] */
    SPH_F_ACCELERATION = 4,       /* f32 [N,3] */
    SPH_F_M_V = 5,                /* f32 [N]   */
    SPH_F_M = 6,                  /* f32 [N]   */
    SPH_F_DENSITY = 7,            /* f32 [N]   */
    SPH_F_PRESSURE = 8,           /* f32 [N]   */
    SPH_F_MATERIAL = 9,           /* i32 [N]   */
    SPH_F_COLOR = 10,             /* i32 [N,3] */
    SPH_F_IS_DYNAMIC = 11,        /* i32 [N]   */
    SPH_F_GRID_IDS = 12,          /* i32 [N]   particle_system.py:138 (download only) */
    SPH_F_GRID_PARTICLES_NUM = 13,/* i32 [G]   particle_system.py:96  (download only) */
    SPH_F_PID = 14,               /* i32 [N]   persistent id (default: index at creation); < cold_capacity */
    SPH_F_RIGID_REST_CM = 15,     /* f32 [n_objects,3]  particle_system.py:93 */
    SPH_F_DFSPH_FACTOR = 16,      /* f32 [N]   particle_system.py:116 (simulationMethod 4).  Like the reference's, */
    SPH_F_DENSITY_ADV = 17,       /* f32 [N]   particle_system.py:117  the values are dead across steps: they are
                                   *           NOT carried through the sort (every step recomputes them first). */
    SPH_F_COUNT_ = 18
};

enum SphError {
    SPH_OK = 0,
    SPH_E_INVALID = -1,      /* bad argument / size mismatch */
    SPH_E_NO_DEVICE = -2,    /* no HIP device / wrong architecture */
    SPH_E_NOMEM = -3,
    SPH_E_STATE = -4         /* call order violated (e.g. sort before grid ids) */
};

/* Neighbour-gather implementation: 0 = per-particle cell walk through L1/L2,
 * 1 = LDS-staged cell bricks (default). */
enum SphOption {
    SPH_OPT_GATHER_IMPL = 0,
    SPH_OPT_TIMING = 1,        /* k > 0 = record per-phase HIP events inside every k-th step (sph_step, sph_dfsph_step, the slab
                                  calls); SphTimings then holds sums over the timed steps.  An event is a packet of its own
                                  between two kernels: k = 1 costs the 1.75 M step 4 %, k = 8 half a percent */
    SPH_OPT_FUSED_STEP = 2,    /* 1 (default) = sph_step uses the fused density+EOS / force kernels */
    SPH_OPT_BRICK_SHAPE = 3,   /* how the LDS-brick sweeps cut the grid: 0 (default) = 4 x 2 cell columns times a height chosen
                                  per brick from the cell histogram (at most 4 layers, at most 256 targets, shell within the
                                  LDS tile); 1 = fixed 4 x 2 x 4 bricks (the partition of ABI <= 2 builds, kept for A/B) */
    SPH_OPT_NO_DYNAMIC_SOLIDS = 4 /* 1 = the caller guarantees no dynamic solid particle exists (slab ranks
                                  cannot know this locally); skips the per-step device count */,
    SPH_OPT_DEBUG_ABLATE = 5,  /* profiling BUILD only (-DSPH_PROFILE: libsph_hip_profile.so): bit mask of sweep sections to skip (results
                                  are then wrong); the production library refuses any value but 0 */
    SPH_OPT_SLAB_DROP_OUTSIDE = 6 /* slab ranks: a particle whose x cell layer is outside the local grid is hashed to
                                  a virtual cell G (sorted behind every real cell) instead of being clamped; the
                                  host then truncates the particle set with sph_truncate */,
    SPH_OPT_UNIFORM_FLUID = 7  /* fused force sweep with ONE neighbour gather per pair instead of two.  Exact, but only
                                  valid when every fluid particle has the same mass m and m_V == m_V0 (what the
                                  reference's add_particle produces for scenes whose fluid blocks share one density).
                                  -1 (default) = check on the device whenever m / m_V / material were uploaded or the
                                  particle set changed, and use it when it holds; 0 = never; 1 = check once, then the
                                  caller vouches for later arrivals (slab ranks: migrating particles of the same scene) */,
    SPH_OPT_UNIFORM_FLUID_STATE = 8 /* read-only (sph_get_option): -1 not decided yet, 0 general sweep, 1 one-gather sweep */,
    SPH_OPT_SORT_BY_PID = 9    /* 1 = inside a cell, order by persistent id instead of by previous index.  The reference
                                  order (previous index) is kept on a single GPU; slab ranks running DFSPH need an order
                                  that the owner of a boundary band and the neighbour holding it as ghosts agree on, so
                                  that ghost velocities can be refreshed record for record */,
    SPH_OPT_KERNEL_VARIANT = 10 /* A/B switch for the brick sweeps of the fused WCSPH step: bit mask of
                                  SPH_VAR_* below.  Every combination computes the same sums (list order and rounding
                                  apart); -1 = the library's default */,
    SPH_OPT_RIGID_BATCH = 11   /* 1 (default) = solve_rigid_body() (sph_base.py:247-260) of ALL dynamic bodies in three launches
                                  inside sph_step / sph_dfsph_step, the per-body solid wall passes replayed per particle;
                                  0 = body by body (4 launches each).  Same results bit for bit.  (One launch behind grid-wide
                                  barriers was built too and is slower: commit 98934a4.) */,
    SPH_OPT_DF_RUNAHEAD = 13,  /* DFSPH solver loops: 1 = the host enqueues Jacobi iteration k + 1 before it waits for iteration k's
                                  convergence test (made on the device either way); a body enqueued past convergence leaves at
                                  once and the GPU never waits for the host.  0 (default) = enqueue, wait, decide: a host round
                                  trip per iteration, as in the reference's loop -- measured 2 % FASTER at 1.75 M particles
                                  (2.906 vs 2.965 ms per step): the empty launches of the one speculative body per solve cost
                                  more than the bubbles.  Same iteration counts, same results. */
    SPH_OPT_EXACT_MATH = 12    /* A/B of the fast-math choice (never the default): 1 = the brick sweeps of the fused WCSPH step
                                  (density + EOS, force) evaluate r.norm(), r / (|r| h), x / y with IEEE sqrt and divide
                                  as the reference's f32 expressions do, instead of v_rsq_f32 / v_rcp_f32 (~1 ulp).
                                  profiles/r04_parity_fastmath_ab.json holds the two builds side by side.
                                  RESTRICTION: exact-math instances exist for the uniform-fluid step only (GM_DENSITY_EOS
                                  inline / lean and GM_FORCE_FUSED_U); scenes with any solid run the general sweeps, whose
                                  pair physics keeps v_rsq / v_rcp, and so do the cell-walk fallbacks.  sph_get_option
                                  reports the EFFECTIVE state: 1 only while the context's step actually runs those
                                  instances (SPH_OPT_UNIFORM_FLUID_STATE == 1), else 0. */,
    SPH_OPT_RIGID_SUMS_FROM_X0 = 14, /* 1 = the centre-of-mass sums of sph_compute_rigid_rest_cm and sph_rigid_partial_sums read the REST
                                  positions x_0 instead of x.  In the reference x_0 == x when initialize() computes
                                  rigid_rest_cm (sph_base.py:80-90); a RESTART (positions given, x_0 from the scene file) must not
                                  take the displaced body's centre for the rest centre.  The Python layer sets it around the
                                  rest-cm computation of a restarted ParticleSystem and clears it again; default 0. */
    SPH_OPT_PURE_FLUID_INSTANCE = 15 /* 1 (default) = a single context found (on the device) to hold no solid particle at all runs the
                                  pure-fluid instances of the uniform-fluid step's two sweeps: density (m_V_j = m_V0 from a register)
                                  and one-gather force (the branch-free pair term without its solid-neighbour path).  Both issue fewer
                                  instructions for the same operations on the same operands: bit-identical results;
                                  0 = always the general instances (the A/B switch; was the SPH_DISABLE_PURE_FLUID environment
                                  variable in ABI 4); 2 = the CALLER vouches that the whole scene holds no solid particle at all
                                  (slab ranks: arrivals are never checked on the device; the Python layer sets it when the scene
                                  file has no rigid block and no rigid body) */,
    SPH_OPT_BRICK_RECORDS = 16 /* 1 (default) = the list-WRITING brick sweep (density) leaves each brick's column tables (what step A of
                                  the sweep computes from the cell array: 512 bytes per brick) in HBM, and the list-READING sweeps
                                  over the same partition and target ranges (the fused force sweep; the ~18 sweeps of a DFSPH step)
                                  load them with one 16-byte read per lane instead of recomputing them; 0 = every sweep recomputes
                                  (A/B).  Same tables, same results bit for bit. */,
    SPH_OPT_DF_FUSE_ERROR = 17 /* 1 (default) = inside the DFSPH solver loops (sph_dfsph_divergence_solve / _pressure_solve) the density-change
                                  / density-advection sweep of an iteration also reduces compute_density_error()'s sum (DFSPH.py:224-230)
                                  over its own targets -- one f64 partial per brick, added up in brick-list order by the convergence
                                  test -- instead of a streaming kernel that re-reads every particle; 0 = that kernel (A/B).  The same
                                  per-particle f32 terms either way; the f64 grouping differs (both deterministic). */,
    SPH_OPT_SORT_FAST = 18     /* 1 = the sort at the head of a step of sph_step / sph_dfsph_step ranks the particles that STAY in their
                                  cell from the previous order (previous cell array, a ballot of the movers) and compares only movers
                                  and the members of cells with arrivals against those arrivals: no intra-cell offsets, no place
                                  kernel, records read in order.  Taken only while the current order is a sort's output that nothing
                                  has touched since (no upload, append, selection, truncate, window change), with SPH_OPT_SORT_BY_PID
                                  and SPH_OPT_SLAB_DROP_OUTSIDE off; every other sort -- the first, stand-alone sph_sort /
                                  sph_counting_sort, slab ranks -- is the general one.  0 = the general sort everywhere (A/B).  Same
                                  order, same arrays, bit for bit.  sph_get_option reports the requested value. */,
    SPH_OPT_SORT_FAST_COUNT = 19,   /* read-only: sorts of this context that ran on the fast path ... */
    SPH_OPT_SORT_GENERAL_COUNT = 20, /* ... and on the general path (both wrap at 2^31) */
    SPH_OPT_SORT_LEAN = 21     /* 1 (default) = a fast sort (SPH_OPT_SORT_FAST) at the head of a step of sph_step moves the persistent id alone, through
                                  an array of its own, in place of the 16-byte (m, density, pressure, id) record: 40 B per particle each
                                  way instead of 52.  Taken only on the step whose sweeps leave that record alone -- the fused
                                  uniform-fluid step under the rule that admits the pure-fluid instances (SPH_OPT_PURE_FLUID_INSTANCE),
                                  without registered kinematic motions -- where m is one value and density / pressure wait in the
                                  step's own 8-byte record.  Whoever asks for any of the four words (a download, an upload, an
                                  observer, a stand-alone call, another kind of sort, a change of the particle set) gets the record
                                  written back first, once: same arrays, same results, bit for bit.  0 = the record is moved by
                                  every sort (A/B; profiles/sort_lean_ab.json).  sph_get_option reports the requested value. */
};
#define SPH_VAR_GROUPS 1   /* density: all nine runs filtered first (masks in registers), hits emitted centre run / edge runs / corner
                              runs, each group by descending hit count */
/* (bit 2 was SPH_VAR_RING, the per-lane LDS ring of hit masks with ONE balanced emission loop per lane: built, parity-green,
   slower than GROUPS -- profiles/archive/r03f_variants_partition_x_emission.json, DESIGN.md 4.5 -- and removed after commit 1bbd9b5;
   a mask with that bit set is refused) */
#define SPH_VAR_MFMA 32     /* density (with GROUPS): the candidate filter on the MATRIX pipe -- v_mfma_f32_16x16x4_f32 tests 16 candidate
                              rows against 16 target columns; a wave's 64 targets are four tiles of 16 consecutive targets, the
                              4-bit row pieces reach their target's lane through a v_permlane32/16_swap transpose (round 5:
                              the A/B the verdict asked for; DESIGN_HISTORY.md).  Same hits, same lists, same sums. */
#define SPH_VAR_GAT_LDS 2   /* (round 6) uniform-fluid force sweep: the neighbour's SECOND record (v, p / rho^2) is staged in LDS beside the first
                              instead of gathered through the L1 per pair; tile of 1,408 shell records x 32 B, three workgroups per CU;
                              the step's bricks are cut for that tile.  Implies FORCE_BF | DEEP.  Same sums (the partition, hence the
                              list order, differs from the default's where a shell exceeds the smaller tile) */
#define SPH_VAR_GAT_LDS4 4  /* the same with a tile of 1,200 records: four workgroups per CU, more bricks cut short */
#define SPH_VAR_FORCE_BF 8 /* force sweep: branch-free fluid pair term, buffer addressing for list and gather */
#define SPH_VAR_DEEP 16    /* list-reading sweeps: list entries loaded a whole round (3 pairs) before they are decoded */
/* (r04: bit 64 was SPH_VAR_PERSIST -- both sweeps as PERSISTENT workgroups, grid = the chip's resident slots, bricks taken by
   per-XCD TICKETS with the next ticket fetched while computing: built, parity-green, slower like round 2's static walk (density
   +17 %, force +25 %: profiles/r04c_variants_persistent_tickets.json, DESIGN_HISTORY.md) and removed after commit e7af346) */
/* 0 = the baseline: run-by-run emission in the reference's (dx, dy) order, plain list loop in the force sweep.
 * Default = GROUPS | FORCE_BF | DEEP.  (Rounds 1-2 also carried PAD, MICRO -- now always on -- and 2PHASE, MIRROR,
 * SORTED: measured, superseded and removed; their tables are profiles/archive/r02c, r02o, r02p.) */

/* ms accumulated by sph_step since the last sph_reset_timings (HIP events on
 * the context's stream).  sort = K1+K2+K3 (initialize_particle_system),
 * neighbour = K4+K5 (boundary volume + density/EOS), force = K6+K7,
 * integrate = K8+K9+K10, halo = multi-GPU exchange packing. */
typedef struct SphTimings {
    double sort_ms, neighbour_ms, force_ms, integrate_ms, halo_ms, total_ms;
    int64_t steps;
} SphTimings;

int32_t sph_abi_version(void);
int32_t sph_device_count(void);

/* ParticleSystem.__init__ field allocation (particle_system.py:91-145). `stream`
 * may be NULL (the context creates its own) or a hipStream_t to enqueue on. */
int32_t sph_create(const SphParams* params, int32_t device, void* stream, SphContext** out);
int32_t sph_destroy(SphContext* ctx);
const char* sph_last_error(const SphContext* ctx);
int32_t sph_set_option(SphContext* ctx, int32_t option, int32_t value);
int32_t sph_get_option(const SphContext* ctx, int32_t option, int32_t* value);
/* Replace the solver scalars (WCSPHSolver.__init__, WCSPH.py:6-16); the sizes in
 * `params` (n_particles, capacity, grid_num, cell_origin, n_objects) must be unchanged. */
int32_t sph_set_params(SphContext* ctx, const SphParams* params);
int32_t sph_set_dt(SphContext* ctx, float dt);                        /* solver.dt[None] = ..  sph_base.py:20-21 */
int32_t sph_set_particle_count(SphContext* ctx, int32_t n);           /* owned+ghost count (multi-GPU) */

/* ti.field.from_numpy / to_numpy / _add_particles (particle_system.py:260-284,
 * 409-418).  `host` is borrowed for the duration of the call. */
int32_t sph_upload(SphContext* ctx, int32_t field, const void* host, size_t bytes);
int32_t sph_download(SphContext* ctx, int32_t field, void* host, size_t bytes);

/* --- K1-K3: neighbour structure (particle_system.py:311-375) --- */
int32_t sph_update_grid_id(SphContext* ctx);       /* update_grid_id          :311-320 */
int32_t sph_prefix_sum(SphContext* ctx);           /* PrefixSumExecutor.run   :374 (scan_single_buffer.py:108-146) */
int32_t sph_counting_sort(SphContext* ctx);        /* counting_sort           :322-369 */
int32_t sph_initialize_particle_system(SphContext* ctx); /* :372-375 */

/* --- K4-K10: solver kernels --- */
int32_t sph_compute_boundary_volume(SphContext* ctx, int32_t dynamic); /* sph_base.py:91-98 (0) / :106-113 (1) */
int32_t sph_compute_densities(SphContext* ctx);             /* WCSPH.py:33-43 */
int32_t sph_compute_non_pressure_forces(SphContext* ctx);   /* WCSPH.py:128-140 */
int32_t sph_compute_pressure_forces(SphContext* ctx);       /* WCSPH.py:70-85 */
int32_t sph_advect(SphContext* ctx);                        /* WCSPH.py:143-149 */
int32_t sph_enforce_boundary_3D(SphContext* ctx, int32_t particle_type); /* sph_base.py:149-179 */
int32_t sph_compute_rigid_rest_cm(SphContext* ctx, int32_t object_id);   /* sph_base.py:87-89 */
/* solve_constraints (sph_base.py:200-222).  R_out (9 floats, row-major) may be
 * NULL; when non-NULL the call synchronises, like the reference's return. */
int32_t sph_solve_constraints(SphContext* ctx, int32_t object_id, float* R_out);
/* compute_com_kernel (sph_base.py:195-197); synchronises. */
int32_t sph_compute_com(SphContext* ctx, int32_t object_id, float* cm_out);

/* SPHBase.step() x n_steps (sph_base.py:263-271) entirely on the device.
 * dynamic_ids = objectIds of dynamic RigidBodies (sph_base.py:249-250). */
int32_t sph_step(SphContext* ctx, int32_t n_steps, const int32_t* dynamic_ids, int32_t n_dynamic);

int32_t sph_sync(SphContext* ctx);
int32_t sph_get_timings(SphContext* ctx, SphTimings* out);
int32_t sph_reset_timings(SphContext* ctx);

/* Neighbourhood statistics of the LAST density sweep of the LDS-brick path (no reference counterpart; the
 * reference's for_all_neighbors, particle_system.py:378-385, has no capacity limits to report on).  They say how
 * far a flow state is from the rest lattice and whether any target left the fast path.  Synchronises. */
typedef struct SphStats {
    int64_t targets;               /* fluid particles that gathered */
    int64_t list_entries;          /* sum of their neighbour-list lengths (superset filter: includes the particle
                                      itself and pairs within 1e-4 h beyond h) */
    int32_t max_list;              /* longest list */
    int32_t list_overflow_targets; /* lists longer than the hand-off capacity (95): the force sweep walks the cells */
    int32_t lds_overflow_targets;  /* targets of bricks whose shell did not fit the LDS tile: both sweeps walk the cells */
    int32_t max_cell_occupancy;    /* particles in the fullest cell */
    int32_t nonempty_cells;
    int32_t polar_fallbacks;       /* solve_constraints() calls since sph_create whose polar rotation (sph_base.py:212) left the Newton
                                      iteration for the Jacobi-SVD form: degenerate bodies (flat = rank-2 A, rods, reflections) */
} SphStats;
int32_t sph_get_stats(SphContext* ctx, SphStats* out);

/* --- multi-GPU slab support (no reference counterpart) -------------
 * Cells are flattened x-slowest (particle_system.py:294), so after the sort every
 * set of x-layers is ONE contiguous index range.  A slab rank exchanges such ranges
 * with its x-neighbours as packed records (48 B/particle: `count` xm float4s, then
 * `count` vf float4s, then `count` aux float4s) through device buffers it owns
 * (torch tensors + torch.distributed/RCCL on the host side). */
#define SPH_RECORD_BYTES 48
int32_t sph_get_particle_count(SphContext* ctx, int32_t* n);
/* out[k] = number of particles in local x-layers < layers[k] (valid after
 * sph_prefix_sum / the sort).  Synchronises. */
int32_t sph_layer_offsets(SphContext* ctx, const int32_t* layers, int32_t n, int32_t* out);
/* Split form: _begin enqueues the copies (pinned host memory + an event) right behind the sort and returns;
 * _end waits for that event only, so kernels enqueued in between (sph_sweeps) keep the GPU busy. n <= 16. */
int32_t sph_layer_offsets_begin(SphContext* ctx, const int32_t* layers, int32_t n);
int32_t sph_layer_offsets_end(SphContext* ctx, int32_t* out, int32_t n);
/* Keep only [first, first+count) of the current order as the particle set (drops
 * ghosts); must be followed by a sort before any sweep. */
int32_t sph_select_range(SphContext* ctx, int32_t first, int32_t count);
/* Shrink the particle set to its first n records without invalidating the neighbour structure
 * (drops the particles the sort moved into the virtual cell, SPH_OPT_SLAB_DROP_OUTSIDE). */
int32_t sph_truncate(SphContext* ctx, int32_t n);
int32_t sph_pack_range(SphContext* ctx, int32_t first, int32_t count, void* device_dst);
/* Append `count` packed records after the current particles (count += n). */
int32_t sph_append_records(SphContext* ctx, const void* device_src, int32_t count);
/* Restrict the TARGETS of the density (+EOS) and force sweeps to local x layers [lo, hi) (candidates are never
 * restricted).  A slab rank sets density = owned + first ghost layer, force = owned: the outer ghost layer only
 * serves as neighbours.  Default: all layers. */
int32_t sph_set_target_layers(SphContext* ctx, int32_t density_lo, int32_t density_hi, int32_t force_lo, int32_t force_hi);
/* Re-cut (load balance, SURVEY 8e "re-cut every K steps"): move the context's window of global x layers to
 * [origin_x, origin_x + nx), nx <= the grid_num[0] given to sph_create (which is the allocation).  Takes effect at
 * the next sort: records outside the new window fall into the virtual cell and are dropped like any stray.  Resets
 * the target layers to all layers (call sph_set_target_layers afterwards). */
int32_t sph_slab_set_window(SphContext* ctx, int32_t origin_x, int32_t nx);
/* One slab step's device work in two calls (same effect as the individual calls, fewer host round trips):
 *   sph_slab_pack : pack [firstL, firstL+nL) into dstL and [firstR, ...) into dstR, then synchronise (the
 *                   buffers are handed to the transport next);
 *   sph_slab_advance : select [keep_first, keep_first+keep_count), append the two received ranges, sort,
 *                   enqueue the offset read-back for `layers` (sph_layer_offsets_begin), enqueue the sweeps
 *                   (if do_sweeps).  Follow with sph_layer_offsets_end + sph_truncate. */
int32_t sph_slab_pack(SphContext* ctx, int32_t firstL, int32_t nL, void* dstL, int32_t firstR, int32_t nR, void* dstR);
int32_t sph_slab_advance(SphContext* ctx, int32_t keep_first, int32_t keep_count, const void* srcL, int32_t nL,
                         const void* srcR, int32_t nR, const int32_t* layers, int32_t n_layers, int32_t do_sweeps);
/* Exchange hidden behind compute.  sph_slab_advance(..., do_sweeps = 2) runs only the boundary-volume and density
 * sweeps after the sort.  sph_slab_forces then enqueues: force sweep of the boundary layers [bl_lo,bl_hi) and
 * [br_lo,br_hi); the two halo packers (records [firstL,+nL) / [firstR,+nR) advanced by this step's Euler + wall
 * update, written to dstL / dstR, arrays untouched); an event; the force sweep of the remaining owned layers; the
 * in-place advect.  sph_slab_wait_pack blocks until the packers are done -- the caller starts the exchange while
 * the interior force sweep is still running.  (With the advect fused into the interior sweep's finish the interior
 * particles' `acceleration` field is not materialised by this call: only the boundary sets' is, for the packers;
 * sph_download(SPH_F_ACCELERATION) then fails with SPH_E_STATE until something writes every acceleration again:
 * sph_compute_non_pressure_forces (+ sph_compute_pressure_forces), sph_step, or an upload.) */
int32_t sph_slab_forces(SphContext* ctx, int32_t bl_lo, int32_t bl_hi, int32_t br_lo, int32_t br_hi,
                        int32_t firstL, int32_t nL, void* dstL, int32_t firstR, int32_t nR, void* dstR);
int32_t sph_slab_wait_pack(SphContext* ctx);
int32_t sph_slab_density(SphContext* ctx);   /* moving boundary volume + density/EOS sweep (what do_sweeps = 2 runs) */
/* The sort of sph_step (no acceleration permutation): hash + scan + scatter. */
int32_t sph_sort(SphContext* ctx);
/* One step's sweeps without the sort: boundary volume, density+EOS, force, advect +
 * fluid walls (the slab driver sorts and exchanges halos itself). */
int32_t sph_sweeps(SphContext* ctx);

/* ---- shape matching across slabs (sph_base.py:182-222 with the sums split over ranks) ----
 * A body's particles may live on several ranks.  Each rank adds up ITS OWN particles of `object_id` (indices
 * [first, first+count) of the current order = its owned range), the 16 sums of all ranks are added (one
 * all-reduce of 16 doubles), and every rank moves all local particles of the body -- ghosts included -- with the
 * same cm and rotation.  sums (DEVICE pointers, doubles): [0] sum m, [1..3] sum m x, [4..6] sum m q,
 * [7..15] sum m x (x) q row-major, with m = m_V0 * density, q = x_0 - rigid_rest_cm[object]; so
 * A = sum m (x - cm)(x) q = [7..15] - cm (x) [4..6] exactly as sph_base.py:206-210.
 * sph_rigid_partial_sums enqueues on the context's stream (sph_sync before handing the buffer to the
 * communication library).  sph_rigid_apply_sums: mode 0 = rest centre of mass (sph_base.py:87-89), mode 1 =
 * solve_constraints (cm, polar rotation, x = cm + R q).  x_0 lives in a persistent-id-indexed table; ranks that
 * can receive a body's particles later load the whole body's rest positions with sph_upload_rest_positions. */
int32_t sph_rigid_partial_sums(SphContext* ctx, int32_t object_id, int32_t first, int32_t count, double* dev_sums16);
int32_t sph_rigid_apply_sums(SphContext* ctx, int32_t object_id, const double* dev_sums16, int32_t mode);
int32_t sph_upload_rest_positions(SphContext* ctx, const int32_t* pid, const float* x0, int32_t n);

/* ---- the slab exchange itself: RCCL point-to-point over xGMI, enqueued on the device (sph_comm.hip) ----
 * SURVEY 8(b) sph_exchange_halo / sph_migrate.  One SphComm per context (= per GPU / rank).  The host gets the 128-byte
 * RCCL unique id on rank 0 (sph_comm_unique_id), distributes it by whatever it has (torch.distributed, MPI, a file)
 * and every rank calls sph_comm_create.  left / right below = the x-neighbours' ranks, -1 at a domain end (a rank may
 * name itself: the loop-back used by the one-GPU tests).  librccl is dlopen'ed at the first call.
 * Per step:  sph_slab_announce   after the sort, when the layer offsets -- hence the record counts of THIS step's
 *                                messages -- are known: sends them ahead (non-blocking);
 *            sph_slab_incoming   the counts the neighbours announced (waits for the tiny message: normally long there),
 *                                so that the host can size its receive buffers;
 *            sph_slab_exchange   ncclGroupStart; ncclSend / ncclRecv x <= 4; ncclGroupEnd on the communication stream,
 *                                which first waits for the halo packers' event of sph_slab_forces (after_packers = 1;
 *                                the interior force sweep keeps running on the main stream) or for the main stream
 *                                (after_packers = 0); the main stream then waits for the exchange.  Nothing blocks the host.
 * sph_comm_swap: fixed-size exchange (DFSPH ghost-velocity refresh); sph_comm_all_reduce: in-place sum of n doubles
 * (dtype 0) or int64 (dtype 1) in device memory; both are ordered after the main stream's work and before what it
 * does next.  sph_comm_halo_time: accumulated duration of the payload exchanges on the communication stream. */
typedef struct SphComm SphComm;
const char* sph_comm_last_error(void);
/* 0 if librccl (or the library named by SPH_RCCL_LIB) can be opened and exports what this file binds: lets the ranks of a
 * job agree on the transport BEFORE anybody enters the collective sph_comm_create. */
int32_t sph_comm_available(void);
int32_t sph_comm_unique_id(uint8_t* out128);
int32_t sph_comm_create(SphContext* ctx, const uint8_t* id128, int32_t rank, int32_t world, SphComm** out);
int32_t sph_comm_destroy(SphComm* comm);
int32_t sph_slab_announce(SphContext* ctx, SphComm* comm, int32_t left, int32_t right, int32_t n_to_left, int32_t n_to_right);
int32_t sph_slab_incoming(SphContext* ctx, SphComm* comm, int32_t* n_from_left, int32_t* n_from_right);
int32_t sph_slab_exchange(SphContext* ctx, SphComm* comm, int32_t left, int32_t right, const void* send_left, int32_t n_to_left,
                          const void* send_right, int32_t n_to_right, void* recv_left, int32_t n_from_left, void* recv_right,
                          int32_t n_from_right, int32_t after_packers);
int32_t sph_comm_swap(SphContext* ctx, SphComm* comm, int32_t left, int32_t right, const void* send_left, int64_t bytes_to_left,
                      const void* send_right, int64_t bytes_to_right, void* recv_left, int64_t bytes_from_left, void* recv_right,
                      int64_t bytes_from_right);
int32_t sph_comm_all_reduce(SphContext* ctx, SphComm* comm, void* dev, int32_t n, int32_t dtype);
int32_t sph_comm_sync(SphContext* ctx, SphComm* comm);
int32_t sph_comm_halo_time(SphContext* ctx, SphComm* comm, double* ms, int64_t* exchanges);
/* rank / world of the communicator as the communication library reports them (ncclCommUserRank / ncclCommCount) */
int32_t sph_comm_info(SphContext* ctx, SphComm* comm, int32_t* rank, int32_t* world);

/* ======================================================================================
 * DFSPH (simulationMethod 4): DFSPHSolver of /root/reference/DFSPH.py on the same neighbour
 * machinery.  The density sweep writes every fluid particle's neighbour list once per step;
 * all later sweeps of the step (factor, density change / advection, both Jacobi solvers,
 * non-pressure forces) read those lists.  The solver loops run inside the library.  The
 * reference's loop has the host between two iterations (compute_density_error returns a
 * float that Python compares with eta); here the test is made on the device with the same
 * arithmetic and the host reads its verdict (sph_api.hip: df_solve_loop).  With
 * SPH_OPT_DF_RUNAHEAD 1 the host enqueues iteration k + 1 before it waits for iteration
 * k's verdict and sweeps enqueued past convergence leave at once; the iteration counts
 * are the reference's either way.
 * ==================================================================================== */
typedef struct SphDfsphParams {
    int32_t enable_divergence_solver; /* DFSPH.py:12 */
    int32_t m_max_iterations_v;       /* DFSPH.py:14 */
    int32_t m_max_iterations;         /* DFSPH.py:15 */
    int32_t fluid_particle_num;       /* particle_system.py:57-62: divisor of the average density error */
    float m_eps;                      /* DFSPH.py:17 */
    float reserved_;
    double max_error_V;               /* DFSPH.py:19 (Python-scope floats: f64) */
    double max_error;                 /* DFSPH.py:20 */
} SphDfsphParams;

typedef struct SphDfsphStats {
    int32_t iterations_v;             /* what DFSPH.py:258 prints for the last divergence solve */
    int32_t iterations;               /* what DFSPH.py:353 prints for the last pressure solve */
    double avg_density_err_v;
    double avg_density_err;
    int64_t total_iterations_v;       /* solver iterations run since sph_create (incl. the unconditional first one) */
    int64_t total_iterations;
    int64_t steps;
} SphDfsphStats;

int32_t sph_dfsph_set_params(SphContext* ctx, const SphDfsphParams* params);
int32_t sph_dfsph_get_stats(SphContext* ctx, SphDfsphStats* out);
int32_t sph_dfsph_compute_densities(SphContext* ctx);              /* DFSPH.py:37-47 */
int32_t sph_dfsph_compute_DFSPH_factor(SphContext* ctx);           /* DFSPH.py:116-154 */
int32_t sph_dfsph_compute_density_change(SphContext* ctx);         /* DFSPH.py:157-197 */
int32_t sph_dfsph_compute_density_adv(SphContext* ctx);            /* DFSPH.py:200-221 */
int32_t sph_dfsph_compute_density_error(SphContext* ctx, float offset, float* out); /* DFSPH.py:224-230; synchronises */
int32_t sph_dfsph_multiply_time_step(SphContext* ctx, float time_step);            /* DFSPH.py:233-237 on dfsph_factor */
int32_t sph_dfsph_divergence_solver_iteration_kernel(SphContext* ctx);             /* DFSPH.py:285-321 */
int32_t sph_dfsph_pressure_solve_iteration_kernel(SphContext* ctx);                /* DFSPH.py:356-394 */
int32_t sph_dfsph_divergence_solve(SphContext* ctx);               /* DFSPH.py:240-283 (loop included) */
int32_t sph_dfsph_pressure_solve(SphContext* ctx);                 /* DFSPH.py:324-354 (loop included) */
int32_t sph_dfsph_compute_non_pressure_forces(SphContext* ctx);    /* DFSPH.py:49-112 */
int32_t sph_dfsph_predict_velocity(SphContext* ctx);               /* DFSPH.py:388-394 */
int32_t sph_dfsph_advect(SphContext* ctx);                         /* DFSPH.py:100-107 */
/* n_steps x SPHBase.step() with DFSPHSolver.substep (sph_base.py:263-271, DFSPH.py:400-408).  Phase timings:
 * neighbour = boundary volume + density + factor, force = both solvers + non-pressure forces + predict_velocity. */
int32_t sph_dfsph_step(SphContext* ctx, int32_t n_steps, const int32_t* dynamic_ids, int32_t n_dynamic);
/* DFSPH across slabs: a rank's share of compute_density_error over its OWNED records [first, first+count) (f64, to be
 * all-reduced; synchronises), and the velocity records (v + flags, 16 B each) of a contiguous range copied to
 * (to_context = 0) or from (1) a caller-owned device buffer -- each Jacobi sweep is followed by a refresh of the ghost
 * layers' velocities from their owners. */
int32_t sph_dfsph_compute_density_error_range(SphContext* ctx, float offset, int32_t first, int32_t count, double* out);
int32_t sph_copy_velocity_records(SphContext* ctx, int32_t first, int32_t count, void* device_buf, int32_t to_context);

/* ======================================================================================
 * Headless frame export (run_simulation.py:37-98 of the reference: the window, its camera, scene.particles,
 * scene.lines, window.write_image): a sphere-impostor point renderer with a depth buffer, on the device, next to
 * the particles; only the finished 8-bit image crosses PCIe.  Three launches per frame (clear; splat -- plus one
 * over the compacted list of large sprites; box + resolve), all on the context's stream, so a frame is ordered
 * behind the steps before it without a synchronisation.  A frame READS the particle state and writes none of it.
 * The image is a per-pixel 64-bit minimum of (depth bits << 32 | rgb), which does not depend on particle order or
 * scheduling: frames are bit-reproducible.  csrc/sph_render.hip states the arithmetic operation by operation.
 * Key, image and depth buffers are allocated by the first frame call (and again when the size changes) and freed
 * by the context's destructor.  Single-domain contexts only: a slab rank answers SPH_E_STATE.
 * ==================================================================================== */
#define SPH_RENDER_MAX_INVISIBLE 32
typedef struct SphRenderParams {
    int32_t width, height;          /* 1024 x 1024: the reference's window (run_simulation.py:37) */
    float eye[3], lookat[3], up[3]; /* (5.5, 2.5, 4.0), (-1, 0, 0), (0, 1, 0)   run_simulation.py:41-43 */
    float fov_y_deg;                /* 70                                        run_simulation.py:44 */
    float radius;                   /* world radius of a particle's sphere: particle_radius (run_simulation.py:91) */
    float near_plane;               /* > 0: particles whose centre is nearer along the view direction draw nothing */
    float light[3];                 /* point light, white: (2, 2, 2)             run_simulation.py:90 */
    float ambient;                  /* in [0, 1]: shade = ambient + (1 - ambient) max(0, n.l) */
    uint8_t background[3], draw_box;/* (0, 0, 0); draw_box != 0: the twelve edges of the box (0,0,0)-box_end */
    float box_end[3];               /* domainEnd                                 run_simulation.py:59-69 */
    float box_color[3];             /* (0.99, 0.68, 0.28)                        run_simulation.py:93 */
} SphRenderParams;
/* SPH_E_INVALID: width or height outside [1, 16384], eye == lookat, up zero or parallel to the view direction, fov not in
 * (0, 180), radius / near_plane not positive, ambient outside [0, 1], a non-finite number. */
int32_t sph_render_set_params(SphContext* ctx, const SphRenderParams* params);
/* particles of these objects are not drawn (invisibleObjects of the scene file); n <= SPH_RENDER_MAX_INVISIBLE, n = 0 clears */
int32_t sph_render_set_invisible(SphContext* ctx, const int32_t* object_ids, int32_t n);
int32_t sph_render_frame(SphContext* ctx);                                  /* enqueues; needs sph_render_set_params before */
int32_t sph_render_download(SphContext* ctx, uint8_t* rgb, size_t bytes);   /* u8 [height, width, 3], row 0 at the top; synchronises */
/* f32 [height, width]: distance along the view direction of what the pixel shows, +inf where nothing was drawn; synchronises */
int32_t sph_render_download_depth(SphContext* ctx, float* depth, size_t bytes);

/* ======================================================================================
 * Kinematic rigid bodies (no reference counterpart: the reference's solids are frozen or shape-matched): a
 * NON-dynamic solid object whose motion the caller prescribes -- a piston, a flap, a stirrer, a gate.
 *
 * Motion of a registered object, with tau = clamp(t, start_time, end_time) - start_time and t the context's clock:
 *     d(tau) = lin_vel tau + osc_amplitude (sin(2 pi osc_frequency tau + osc_phase) - sin(osc_phase))
 *     R(tau) = rotation about ang_vel / |ang_vel| by |ang_vel| tau (Rodrigues; identity when ang_vel = 0)
 *     x(t)   = pivot + d + R (x_0 - pivot)
 *     v(t)   = d'(tau) + ang_vel x (x - pivot - d);   v = 0 for t outside [start_time, end_time]
 * The CLOCK is an f64 held by the context: 0 at sph_create, advanced by the current dt at the end of every step of
 * sph_step / sph_dfsph_step (so sph_set_dt between two calls is honoured), read and set with sph_get_time /
 * sph_set_time.  It advances whether or not a motion is registered.
 * WHERE IN THE STEP: while motions are registered, every step of sph_step / sph_dfsph_step ends -- behind the substep,
 * the dynamic bodies' solve and the fluid wall pass, i.e. where the reference moves its bodies (sph_base.py:263-271)
 * -- by placing every registered object at the pose of the step's END time: one launch for all objects, the pose
 * evaluated on the host in f64, rounded to f32 and passed by value.  During step k the fluid therefore sees the body
 * at pose(t_{k-1}) with velocity(t_{k-1}).  Nothing synchronises; sph_step(n) still only enqueues.  With no motion
 * registered the two step calls enqueue exactly what they enqueue without this section.
 * The kernel writes x and v of the object's particles (from the pid-indexed x_0) and nothing else; what it writes
 * does not depend on particle order or scheduling (csrc/sph_integrate.hip states the f32 arithmetic).
 * CONTAINMENT: before a step is enqueued the object's rest bounding box (eight corners, f64) is carried through the
 * step's end pose; unless all of it lies inside [padding, domain_size - padding] the call returns SPH_E_INVALID with the
 * object and the step named in sph_last_error -- that step and the later ones are not enqueued, the earlier steps of
 * the call stand, the clock stays at the last enqueued step's end.  sph_kinematic_apply checks the same way.
 * BOUNDARY VOLUMES: a kinematic object keeps the m_V that compute_static_boundary_volume (sph_base.py:91-98) gave it
 * at initialize().  Rigid motion preserves the distances inside the object, so that is exact while the object stays
 * a support radius away from every OTHER solid; sph_compute_boundary_volume(ctx, 0) refreshes all static volumes on
 * demand (there is no per-step refresh).
 * SPH_E_INVALID: object id outside [0, n_objects) or without particles, an object with dynamic (or fluid)
 * particles, n > SPH_MAX_KINEMATIC, an id given twice, a non-finite field (end_time may be +inf), end_time <
 * start_time, for sph_kinematic_apply an R that is not orthonormal to 1e-4.  Single-domain contexts only: a slab rank
 * answers SPH_E_STATE.
 * ==================================================================================== */
#define SPH_MAX_KINEMATIC 8
typedef struct SphKinematicMotion {
    int32_t object_id;
    float pivot[3];
    double lin_vel[3], ang_vel[3], osc_amplitude[3], osc_frequency, osc_phase, start_time, end_time;
} SphKinematicMotion;
typedef struct SphBodyPose {
    int32_t object_id;
    float R[9];         /* row-major */
    float pivot[3], origin[3], lin_vel[3], ang_vel[3];   /* x = origin + R (x_0 - pivot), v = lin_vel + ang_vel x (x - origin) */
} SphBodyPose;
/* Replace the set of registered motions (n = 0 clears; n <= SPH_MAX_KINEMATIC).  Reads the objects' rest bounding boxes from
 * one download of x_0 the first time (synchronises then). */
int32_t sph_kinematic_set(SphContext* ctx, const SphKinematicMotion* motions, int32_t n);
/* Stand-alone: place n objects at the given poses now (enqueues; trajectories scripted by the caller). */
int32_t sph_kinematic_apply(SphContext* ctx, const SphBodyPose* poses, int32_t n);
int32_t sph_get_time(SphContext* ctx, double* t);
int32_t sph_set_time(SphContext* ctx, double t);

/* ======================================================================================
 * Flow diagnostics (the reference's older engine prints max velocity / acceleration / density / pressure from whole-array
 * downloads every step and sets dt from them; its current engine has neither): ONE streaming reduction over the live
 * records in their current order -- 64 bytes read per particle, nothing written but the rows -- per object and over
 * all particles.  Row k < n_objects collects the particles whose object id is k (indexed as rigid_rest_cm is); the LAST
 * row, n_objects, collects every particle, those whose object id names no object included.
 * "fluid" = material fluid; "moving" = fluid or is_dynamic: the particles advect integrates.
 * The values are those sph_download would return at that moment: density / pressure that a fused step left in its own
 * record are materialised first (as any download of them does); nothing else of the context is written, and a run with
 * diagnostics calls between its steps ends bit-identical to the run without.  While sph_download of the acceleration
 * refuses (after sph_slab_forces), sph_diag_reduce answers SPH_E_STATE for the same reason.
 * DETERMINISTIC: sums are f64, grouped in a fixed order (lane -> wave -> block -> row; csrc/sph_diag.hip) that depends on
 * the particle count and order alone, never on scheduling: two calls on one state return the same bits.
 * sph_diag_reduce enqueues two launches on the context's stream (grid: at most SPH_DIAG_BLOCKS blocks of SPH_DIAG_THREADS,
 * striding over the records); sph_diag_download copies the rows of the LAST reduce and synchronises -- SPH_E_STATE if there
 * was none, SPH_E_INVALID unless n_rows == n_objects + 1.  More than SPH_DIAG_MAX_OBJECTS objects: SPH_E_INVALID (the
 * per-block row table lives in LDS).  Single-domain contexts only: a slab rank, whose ghost records would be counted
 * twice, answers SPH_E_STATE.
 * ==================================================================================== */
#define SPH_DIAG_BLOCKS 1024
#define SPH_DIAG_THREADS 256
#define SPH_DIAG_MAX_OBJECTS 96
typedef struct SphDiagRow {
    int64_t count;              /* particles of the row */
    int64_t fluid_count;        /* of those, fluid */
    int64_t moving_count;       /* of those, fluid or is_dynamic */
    double mass;                /* sum m */
    double mx[3];               /* sum m x: / mass = centre of mass; -g . mx = potential energy */
    double momentum[3];         /* sum m v */
    double kinetic;             /* sum 1/2 m |v|^2 */
    double v2_max;              /* max |v|^2 over the row, formed in f64 from the f32 components */
    double a2_max;              /* max |a|^2 over the row's moving particles; 0 if there are none */
    float density_min, density_max, pressure_min, pressure_max;   /* over the row's fluid particles; 0 if there are none */
    float lo[3], hi[3];         /* axis-aligned bounds of x over the row; 0 if it is empty */
} SphDiagRow;
int32_t sph_diag_reduce(SphContext* ctx);                                     /* enqueues */
int32_t sph_diag_download(SphContext* ctx, SphDiagRow* rows, int32_t n_rows); /* n_rows == n_objects + 1; synchronises */

/* ======================================================================================
 * Depth-integrated column maps (no reference counterpart: the quantities a dam-break run is compared on -- wave gauges,
 * depth profiles, the position of the wet front): ONE streaming pass over the live records in their current order that
 * bins the selected particles into the columns of a 2-D map.  The columns run along `axis`; the map spans the two other
 * axes ja < jb, n[0] columns along ja times n[1] along jb, column (k_a, k_b) at index k_a * n[1] + k_b.
 * The call READS x, v and the flags (32 bytes per particle) and writes NOTHING of the particle state -- it does not even
 * fold density and pressure back out of a fused step's record, as the diagnostics do: a run with map calls between its
 * steps ends bit-identical to the run without.
 * SELECTED: a particle whose material is fluid and, unless object_id < 0, whose object id equals object_id.
 * ARITHMETIC per selected particle, f32, operation by operation, nothing contracted into an fma, no reciprocal, no divide:
 *     f_j = floorf((x_j - origin_j) * inv_cell_j)      for j = ja, jb: one subtract, one multiply, floorf
 *     k_j = (int)f_j; the particle is OUTSIDE unless 0 <= f_j < n_j for both j (a NaN is outside): it is counted in
 *     `outside` and binned nowhere.  Otherwise its column receives
 *     count    += 1                                                         (i64)
 *     sum_v[a] += llrint((double)fmaxf(fminf(v_a, 65536.f), -65536.f) * 2^20)   a = 0, 1, 2  (i64; round to nearest even)
 *     top       = max(top, x[axis]),  bottom = min(bottom, x[axis])         (f32)
 * inv_cell is computed by the caller (the Python layer: f32(1) / f32(cell)) and passed by value.  Each velocity term is
 * bounded by 2^36, so the i64 sums hold 2^26 particles in one column.
 * DETERMINISTIC: every accumulation is an integer sum or an extremum (which travels as the order-preserving u32 image of
 * the f32 bits, so negative coordinates and signed zeros order one way only); the map is the same bits for any particle
 * order and any scheduling.  There is no floating-point atomic.  csrc/sph_columns.hip describes the on-chip combining.
 * An empty column has count 0, sums 0 and top = bottom = 0 (as the bounds of an empty SphDiagRow).
 * sph_columns_reduce enqueues three launches (clear, scatter, finish) on the context's stream; sph_columns_download copies
 * the map of the LAST reduce (count [n0 * n1], sum_v [3][n0 * n1], top, bottom [n0 * n1]; any pointer may be NULL) and
 * synchronises.  The map's buffers are allocated by the first reduce, again when n[0] * n[1] changes, and freed with the
 * context.
 * SPH_E_INVALID: axis outside 0..2, n[j] < 1, n[0] * n[1] > SPH_COLUMNS_MAX, an inv_cell that is not finite and positive, a
 * non-finite origin; for the download n_columns != n[0] * n[1] of the last reduce.  SPH_E_STATE: download before any
 * reduce; single-domain contexts only: a slab rank, whose ghost records would be counted twice, answers SPH_E_STATE.
 * ==================================================================================== */
#define SPH_COLUMNS_MAX (1 << 20)
#define SPH_COLUMNS_V_SCALE_LOG2 20
typedef struct SphColumnParams {
    int32_t axis;          /* 0, 1, 2: the axis the columns run along */
    int32_t n[2];          /* columns along the two other axes, ascending axis order; n[0] * n[1] <= SPH_COLUMNS_MAX */
    float origin[2], inv_cell[2];
    int32_t object_id;     /* -1: every fluid particle */
} SphColumnParams;
typedef struct SphColumnTotals { int64_t selected, binned, outside; } SphColumnTotals;
int32_t sph_columns_reduce(SphContext* ctx, const SphColumnParams* params);   /* enqueues */
int32_t sph_columns_download(SphContext* ctx, int64_t* count, int64_t* sum_v /* [3][n0*n1] */, float* top, float* bottom,
                             int32_t n_columns, SphColumnTotals* totals);   /* any pointer may be NULL; synchronises */

/* ======================================================================================
 * Particle export (the reference's exportPly path, run_simulation.py:101-107 + ParticleSystem.dump, particle_system.py:409-418,
 * downloads object_id, x and v of ALL particles, masks them on the host and writes text, in the cell-sorted order of the moment):
 * a device-side SELECTION of the live records, ORDERED BY PERSISTENT ID and packed on the device into the exact byte rows of a
 * binary PLY vertex body; the host writes a header and one contiguous buffer, and vertex k is the same particle in every file.
 * SELECTED: a record whose material equals `material` (unless -1), whose object id is in object_ids[0..n_objects) (unless n_objects
 * is 0), whose persistent id satisfies pid % pid_stride == pid_phase (a decimation that keeps the SAME particles in every frame)
 * and, if use_box, whose position satisfies box_lo[a] <= x[a] <= box_hi[a] on all three axes, compared as f32 (a NaN is outside).
 * ROW: the chosen fields in the order of the SPH_EXPORT_* bits, 4 bytes per word, no padding: x y z [vx vy vz] [density] [pressure]
 * [mass] [id] [object]; row_bytes = 4 * words.  ORDER: row r belongs to the selected particle with the r-th smallest persistent id.
 * VALUES: the bits sph_download would return for those fields at that moment; when density or pressure is requested, what a fused
 * step left in its own record is materialised first (as any download of them does), otherwise not.  The kernels do NO arithmetic on
 * a value: the only computations are the box comparison and pid % pid_stride.
 * The call READS xm / vf / aux and writes nothing of the particle state: a run with export calls between its steps ends bit-identical
 * to the run without.  DETERMINISTIC by construction: the output is a function of the SET of selected records, never of their order
 * in memory or of scheduling (csrc/sph_export.hip: a compaction through a table indexed by the id; no kernel waits for another
 * workgroup).
 * DUPLICATE IDS: unique persistent ids below cold_capacity are an invariant of the context (x_0 and color are keyed by them).  If the
 * number of DISTINCT ids marked differs from the number of records selected, duplicate_ids is their difference and
 * sph_export_download answers SPH_E_STATE with a message; no row order is defined then.
 * sph_export_select enqueues five launches (clear, mark, tile counts, tile offsets, pack) on the context's stream; sph_export_info
 * returns the counts of the LAST select and synchronises; sph_export_download copies its rows (bytes == rows * row_bytes) and
 * synchronises.  Buffers: an i32 slot table of cold_capacity entries (rounded up to whole tiles), the tile counts and offsets, and a
 * row buffer for the live count times row_bytes; allocated by the first select, the row buffer again when a later select needs
 * more, freed with the context.  A context that never exports allocates nothing.
 * SPH_E_INVALID: fields without SPH_EXPORT_X or with unknown bits, n_objects outside [0, SPH_EXPORT_MAX_OBJECTS], pid_stride < 1,
 * pid_phase outside [0, pid_stride), with use_box a non-finite bound or box_lo > box_hi; for the download a `bytes` that does not
 * match.  SPH_E_STATE: info or download before any select; single-domain contexts only: a slab rank, whose ghost records would be
 * exported twice, answers SPH_E_STATE.
 * ==================================================================================== */
#define SPH_EXPORT_X        1   /* f32 x 3  (always required)            */
#define SPH_EXPORT_V        2   /* f32 x 3                                */
#define SPH_EXPORT_DENSITY  4   /* f32                                    */
#define SPH_EXPORT_PRESSURE 8   /* f32                                    */
#define SPH_EXPORT_MASS     16  /* f32  (SPH_F_M)                         */
#define SPH_EXPORT_ID       32  /* i32  persistent id                     */
#define SPH_EXPORT_OBJECT   64  /* i32  object id                         */
#define SPH_EXPORT_MAX_OBJECTS 32
typedef struct SphExportParams {
    int32_t fields;                 /* mask of the above; row = the chosen fields in THIS order, 4 bytes per word, no padding */
    int32_t material;               /* -1: any; else == the particle's SPH_F_MATERIAL */
    int32_t n_objects;              /* 0: every object; else the particle's object id must be in object_ids[0..n) */
    int32_t object_ids[SPH_EXPORT_MAX_OBJECTS];
    int32_t pid_stride, pid_phase;  /* keep pid % pid_stride == pid_phase (stride >= 1, 0 <= phase < stride): a decimation that keeps
                                       the SAME particles in every frame */
    int32_t use_box;                /* != 0: keep lo[a] <= x[a] <= hi[a] for a = 0, 1, 2, compared as f32 (a NaN is outside) */
    float box_lo[3], box_hi[3];
} SphExportParams;
typedef struct SphExportInfo { int64_t selected, rows; int32_t row_bytes, duplicate_ids; } SphExportInfo;
int32_t sph_export_select(SphContext* ctx, const SphExportParams* params);   /* enqueues on the context's stream */
int32_t sph_export_info(SphContext* ctx, SphExportInfo* info);               /* of the last select; synchronises */
int32_t sph_export_download(SphContext* ctx, void* host, size_t bytes);      /* bytes == rows * row_bytes; synchronises */

/* ======================================================================================
 * Surface frames (no reference counterpart: its window draws every particle as a sphere): a SECOND frame style beside the
 * sphere frame above, which it leaves untouched.  The fluid is drawn as one screen-space surface -- per pixel the nearest
 * fluid depth and the summed fluid thickness are splatted, the depth is smoothed in image space by a compactly supported
 * bilateral (biweight) filter whose pixel radius follows the depth, normals are taken from the smoothed depth, and the
 * surface is shaded (diffuse + Blinn-Phong + Schlick Fresnel) with absorption by thickness over the OPAQUE layer: the
 * sphere frame's own picture of every particle that is not fluid plus the box edges.
 * Camera, image size, particle radius, box and invisible objects are those of the last sph_render_set_params /
 * sph_render_set_invisible; a surface frame before them answers SPH_E_STATE, and so does one before sph_surface_set_params.
 * Passes per frame, all enqueued on the context's stream (csrc/sph_surface.hip states the arithmetic operation by operation
 * and lists the bytes): clear; opaque splat; fluid splat; `iterations` depth-smoothing passes; one thickness-smoothing pass;
 * shade and resolve.  A frame READS xm, vf (flags), the pid and the colours and writes NOTHING of the particle state; density
 * and pressure are not needed and are not folded out of a fused step's record.  The only accumulations are a 64-bit integer
 * minimum, a 32-bit integer minimum and a 32-bit integer sum; every later pass computes one pixel from a fixed window in a fixed
 * order: the three outputs are functions of the SET of particles, bit for bit, whatever their order or the scheduling.
 * The buffers (39 bytes per pixel) are allocated by the first surface frame, again when the size changes, and freed with the
 * context; a context that never asks for a surface frame allocates nothing.
 * SPH_E_INVALID (sph_surface_set_params; the last good parameters stay in force): iterations outside [0, 8], filter_radius or
 * depth_range not positive and finite, a fluid_color / sky component outside [0, 1], a negative or non-finite absorb component,
 * f0 outside [0, 1], specular negative or non-finite; for a download a `bytes` that does not match the last frame.
 * SPH_E_STATE: a frame before the parameters, a download before any frame; single-domain contexts only: a slab rank answers
 * SPH_E_STATE, as for the sphere frame.
 * ==================================================================================== */
#define SPH_SURFACE_MAX_FILTER_R 16   /* the filter window never exceeds (2 * 16 + 1)^2 pixels */
#define SPH_SURFACE_MAX_ITERATIONS 8
#define SPH_SURFACE_PASSES 6          /* clear, opaque splat, fluid splat, depth smoothing (all iterations), thickness smoothing, shade */
typedef struct SphSurfaceParams {
    int32_t iterations;        /* depth-smoothing passes, 0..SPH_SURFACE_MAX_ITERATIONS */
    float filter_radius;       /* world units: the filter's pixel radius at depth z is ceil(filter_radius * focal / z), at most 16 */
    float depth_range;         /* world units: a neighbour whose depth differs by this much or more has weight 0 */
    float fluid_color[3];      /* in [0, 1] */
    float absorb[3];           /* >= 0, per world unit: transmittance 1 / (1 + absorb * thickness)^2 */
    float sky[3];              /* in [0, 1]: what the Fresnel term reflects */
    float f0;                  /* in [0, 1]: reflectance at normal incidence (water: 0.02) */
    float specular;            /* >= 0: weight of the (n.h)^64 highlight */
} SphSurfaceParams;
int32_t sph_surface_set_params(SphContext* ctx, const SphSurfaceParams* params);
int32_t sph_surface_frame(SphContext* ctx);                                   /* enqueues */
int32_t sph_surface_download(SphContext* ctx, uint8_t* rgb, size_t bytes);    /* u8 [height, width, 3], row 0 at the top; synchronises */
/* f32 [height, width]: the smoothed fluid depth where the fluid is shown, else the opaque layer's depth, +inf where nothing is */
int32_t sph_surface_download_depth(SphContext* ctx, float* depth, size_t bytes);
/* f32 [height, width]: smoothed fluid thickness in front of the opaque layer, world units; 0 where no fluid is shown */
int32_t sph_surface_download_thickness(SphContext* ctx, float* thickness, size_t bytes);
/* A measuring aid: one surface frame with a HIP event between its passes; ms[k] = device time of pass k in the order of
 * SPH_SURFACE_PASSES (n must equal it).  Synchronises; the frame it leaves is an ordinary one. */
int32_t sph_surface_frame_timed(SphContext* ctx, float* ms, int32_t n);

/* ======================================================================================
 * Field colouring of the frames (no reference counterpart: its window colours a particle by its object): the SELECTED
 * particles take a colour from a 256-entry table, indexed by a scalar field of the particle mapped linearly from [lo, hi] to
 * 0..255; every other particle keeps its object colour.  It applies to both frame styles and stays in force until it is switched
 * off.  csrc/sph_render.hip states the index arithmetic (binary32, no contraction), csrc/sph_surface.hip what the surface frame
 * does with the index of the nearest fluid fragment of a pixel.
 * SELECTED: a particle whose material equals `material` (unless -1) and whose object id is in object_ids[0..n_objects) (unless
 * n_objects == 0).  Density and pressure that a fused step left in its own record are materialised by a frame (or a range)
 * that needs them, as any download of them does; nothing else of the context is written.
 * sph_frame_set_colour(ctx, NULL, NULL) switches the colouring off: frames are then made by the launches, and hold the bytes,
 * of a context that never switched it on.  `lut`: 256 x 3 int32 in [0, 255], red green blue; it is uploaded when it differs from
 * the one in force.
 * sph_field_range: minimum and maximum of the field over the particles that are selected, not of an invisible object
 * (sph_render_set_invisible) and whose field value is finite, their number, and the number of selected, visible particles whose
 * value is NOT finite; lo / hi of `colour` are not read.  One streaming pass; the extrema travel as integers, so the result does not
 * depend on particle order.  count == 0 gives lo = +inf, hi = -inf.  Synchronises.
 * SPH_E_INVALID: an unknown field, material outside [-1, 255], n_objects outside [0, SPH_FIELD_MAX_OBJECTS], lo or hi not finite,
 * lo >= hi, a range whose reciprocal width is not a positive finite binary32, a table entry outside [0, 255], one of
 * colour / lut null and the other not.  SPH_E_STATE: a slab rank, as for the frames.
 * ==================================================================================== */
#define SPH_FIELD_MAX_OBJECTS 32
enum SphColourField { SPH_FIELD_SPEED = 0, SPH_FIELD_VX, SPH_FIELD_VY, SPH_FIELD_VZ, SPH_FIELD_DENSITY, SPH_FIELD_PRESSURE,
                      SPH_FIELD_X, SPH_FIELD_Y, SPH_FIELD_Z, SPH_FIELD_COUNT_ };
typedef struct SphFieldColour {
    int32_t field;                  /* enum SphColourField */
    int32_t material;               /* -1: any; else == the particle's material */
    int32_t n_objects;              /* 0: any object */
    int32_t object_ids[SPH_FIELD_MAX_OBJECTS];
    float lo, hi;                   /* the field values that map to the table's first and last entry */
    float axis_origin;              /* subtracted from a position field (SPH_FIELD_X / _Y / _Z) before anything else */
} SphFieldColour;
typedef struct SphFieldRange { float lo, hi; int64_t count, non_finite; } SphFieldRange;
int32_t sph_frame_set_colour(SphContext* ctx, const SphFieldColour* colour, const int32_t* lut);
int32_t sph_field_range(SphContext* ctx, const SphFieldColour* colour, SphFieldRange* out);
/* i32 [height, width] of the last surface frame made with a colouring: the smoothed table index of the pixel's fluid colour, -1
 * where the pixel holds no field-coloured fluid; SPH_E_STATE if the last surface frame had none.  Synchronises. */
int32_t sph_frame_download_field_index(SphContext* ctx, int32_t* index, size_t bytes);

/* ======================================================================================
 * Field sampling (the reference has none; its validation cases report pressure at a sensor, a velocity profile in a section, a
 * regular volume for a viewer): SPH interpolation of velocity, density and pressure AT PLACES -- the nodes of a regular grid (a
 * volume; a slice when one n[a] is 1) or up to SPH_SAMPLE_MAX_POINTS probe points -- by SCATTER: one streaming pass over the live
 * records in their current order in which every selected particle adds its kernel-weighted share to the sample positions inside
 * its support radius.  No neighbour search: the cell array, which describes the positions of the last sort, is never read.
 * SELECTED: as in the export, a particle whose material equals `material` (unless -1) and whose object id is in
 * object_ids[0..n_objects) (unless n_objects == 0).
 * SAMPLE POSITIONS: grid node (k0, k1, k2), at index (k0 * n[1] + k1) * n[2] + k2, is p_a = origin_a + (float)k_a * spacing_a: one
 * multiply, one add, not contracted.  A probe point is the f32 triple as given.
 * PAIR TERM of sample position p and selected particle j: f32, in this order, nothing contracted into an fma:
 *     dx = p.x - x_j.x (dy, dz alike);  r2 = (dx*dx + dy*dy) + dz*dz;  r = correctly rounded sqrtf(r2);  q = r * inv_h
 *     the pair contributes  <=>  q <= 1.0f                    (a NaN does not contribute)
 *     W = q <= 0.5f ? k_w * ((6.f*q3 - 6.f*q2) + 1.f)         with q2 = q*q, q3 = q2*q
 *                   : (k_w * 2.f) * ((t*t)*t)                 with t = 1.f - q
 *     w = fminf(fmaxf(m_V_j * W, 0.f), 4.f)
 * the reference's cubic_kernel (sph_base.py:24-44) with the context's folded constant k_w.  inv_h is computed by the caller (the
 * Python layer: f32(1) / f32(support_radius)) and passed by value, as inv_cell is for the column maps.  m_V is the particle's own
 * volume: m_V0 for fluid, the boundary volume for solids.  The weights never read a density, so they are valid before the first
 * step and never stale.
 * ACCUMULATION per sample position, all sums i64 (llrint: round to nearest even):
 *     count  += 1
 *     weight += llrint((double)w * 2^30)
 *     sum[f] += llrint(((double)w * (double)fmaxf(fminf(A_f, 2^24), -2^24)) * 2^30)      for every requested field f
 * the fields being the bits of `fields` in the order vx vy vz density pressure.  The f64 product of two f32 values is exact and so is
 * the scaling: each term rounds once.  BOUND: for every state the library produces w <= 1 (fluid: m_V0 * k_w = 0.8 * 8 / (8 pi) <
 * 0.255; a boundary volume is at most 1 / k_w), so a term is below 2^54 and an i64 holds 2^9 contributors AT THE CLAMP, against about
 * 34 at rest spacing; with the clamp of w at 4 (uploaded volumes) a term is below 2^56 and 2^7 such contributors fit.  `count` is
 * downloaded so that a caller can see the occupancy.  A value is sum[f] / weight where weight != 0; weight / 2^30 is the Shepard
 * sum, 0.8 inside a fluid at rest spacing (m_V0 = 0.8 d^3).
 * FRESHNESS: x, v, density and pressure are the values sph_download would return at that moment.  After sph_step, x and v are
 * end-of-step values; density and pressure are those of the step's density sweep, one dt behind.  When density or pressure is
 * requested, what a fused step left in its own record is materialised first (as the diagnostics do and as any download of them
 * does); otherwise NOTHING of the context is written.  A run with sample calls between its steps ends bit-identical to the run
 * without.
 * DETERMINISTIC: every accumulation is an integer sum, so the result is the same bits for any particle order, grouping and
 * scheduling; there is no float or double atomic anywhere.  csrc/sph_sample.hip describes the footprints and the kernels.
 * sph_sample_grid enqueues clear plus scatter on the context's stream; sph_sample_grid_download copies the planes of the LAST grid
 * (weight [nodes], count [nodes], sums [F][nodes] with F the number of requested fields; any pointer may be NULL) and synchronises.
 * sph_sample_points copies the m points (xyz: host pointer, [m][3], free again when the call returns), enqueues clear plus scatter;
 * sph_sample_points_download returns the same planes over m.  Buffers are allocated by the first call, the grid's again when a
 * later grid needs more, and freed with the context; a context that never samples allocates nothing.
 * SPH_E_INVALID: n[a] < 1; more than SPH_SAMPLE_MAX_NODES nodes; m outside [1, SPH_SAMPLE_MAX_POINTS]; a non-finite origin or point;
 * a spacing that is not finite and positive; a spacing below support_radius / 8 (that bounds a particle's footprint at 17^3 nodes; a
 * slice still gives a spacing for its axis; the footprints are built with 1 / inv_h, so spacing * inv_h below 1 / 8 is refused
 * alike); an inv_h that is not finite and positive; unknown field bits; material outside [-1, 255] or n_objects outside
 * [0, SPH_SAMPLE_MAX_OBJECTS]; for a download a size that does not match the last call.  A refused call changes nothing: the last
 * good result stays downloadable.  SPH_E_STATE: a download before any sample; single-domain contexts only: a slab rank, whose ghost
 * records would be counted twice, answers SPH_E_STATE.  (The diagnostics also refuse a context whose last sph_slab_forces left the
 * acceleration partly written; that case does not arise here: the acceleration is not read.)
 * ==================================================================================== */
#define SPH_SAMPLE_VX       1
#define SPH_SAMPLE_VY       2
#define SPH_SAMPLE_VZ       4
#define SPH_SAMPLE_DENSITY  8
#define SPH_SAMPLE_PRESSURE 16
#define SPH_SAMPLE_MAX_NODES (1 << 24)
#define SPH_SAMPLE_MAX_POINTS 1024
#define SPH_SAMPLE_MAX_OBJECTS 32
#define SPH_SAMPLE_SCALE_LOG2 30
typedef struct SphSampleSelect {
    int32_t material;               /* -1: any; else == the particle's SPH_F_MATERIAL */
    int32_t n_objects;              /* 0: every object; else the particle's object id must be in object_ids[0..n) */
    int32_t object_ids[SPH_SAMPLE_MAX_OBJECTS];
} SphSampleSelect;
typedef struct SphSampleGrid {
    int32_t n[3];                   /* nodes per axis; n[0] * n[1] * n[2] <= SPH_SAMPLE_MAX_NODES */
    float origin[3], spacing[3];
    float inv_h;                    /* f32(1) / f32(support_radius), computed by the caller */
    int32_t fields;                 /* mask of SPH_SAMPLE_*; the sums' planes follow in THIS order */
    SphSampleSelect select;
} SphSampleGrid;
int32_t sph_sample_grid(SphContext* ctx, const SphSampleGrid* grid);   /* enqueues */
int32_t sph_sample_grid_download(SphContext* ctx, int64_t* weight, int64_t* count, int64_t* sums /* [F][nodes] */,
                                 int64_t nodes);                        /* any pointer may be NULL; synchronises */
int32_t sph_sample_points(SphContext* ctx, const float* xyz /* host, [m][3] */, int32_t m, int32_t fields,
                          const SphSampleSelect* select, float inv_h);  /* enqueues */
int32_t sph_sample_points_download(SphContext* ctx, int64_t* weight, int64_t* count, int64_t* sums /* [F][m] */,
                                   int32_t m);                          /* any pointer may be NULL; synchronises */

/* --------------------------------------------------------------------------------------
 * Field sampling: gradients.  The Shepard interpolant A(p) = sum[f] / weight has an analytic gradient that is a ratio of sums of the
 * same kind:   grad A(p) = ( sum_j grad w_j A_j  -  A(p) sum_j grad w_j ) / sum_j w_j.
 * The gradient-carrying calls below add those sums to the planes of a sample; sum_j grad w_j alone is the gradient of the fill, so
 * -grad fill / |grad fill| is the free-surface normal.  Vorticity, divergence, strain rate and the Q-criterion follow on the host
 * from the velocity gradient (sample.py).
 * GRADIENT TERM of a contributing pair (q <= 1.0f), from the dx, dy, dz, r, q of the pair term above: f32, in this order, nothing
 * contracted into an fma:
 *     D = q <= 0.5f ? (k_w * 6.f) * (q * (3.f*q - 2.f))
 *                   : (k_w * 6.f) * (-(t*t))                  with t = 1.f - q
 *     u = fmaxf(fminf(m_V_j * D, 0.f), -8.f)
 *     e_b = r > 0.f ? d_b / r : 0.f                           b = x, y, z; the IEEE-correct f32 division
 *     g_b = u * e_b
 * D is dW/dq, the reference's cubic_kernel_derivative (sph_base.py) without its 1 / h factor and without the unit vector; D <= 0 on
 * [0, 1].  The sums are therefore DIMENSIONLESS (h grad w): the host multiplies by inv_h.
 * ACCUMULATION per sample position, i64, llrint as above:
 *     G_b    += llrint((double)g_b * 2^30)
 *     S_f,b  += llrint(((double)g_b * (double)fmaxf(fminf(A_f, 2^24), -2^24)) * 2^30)    for every field f of `gradients`
 * A particle exactly on the sample position (r == 0) contributes to count, weight and the field sums as before and ZERO to every
 * gradient sum.  BOUND: |D| <= 2 k_w (its extremum, at q = 1/3), so for every state the library produces |u| <= 2 m_V k_w: below
 * 0.51 for fluid and at most 2 for a boundary volume; |e_b| <= 1.  A term is then at most 2^55 in magnitude (|u| = 2 together with
 * a field at its clamp) and an i64 holds 2^8 - 1 such contributors, against about 34 at rest spacing; at the clamp of u at 8
 * (uploaded volumes) a term is at most 2^57 and 2^6 - 1 such contributors fit.
 * PLANES of one result, in this order: count, weight, the fields of `fields`, Gx Gy Gz, then S_f,x S_f,y S_f,z for every bit f of
 * `gradients` in mask order: at most 2 + 5 + 3 + 15 = 25.  weight stays the second plane: the mesh extraction reads what it read.
 * `gradients` is a mask of SPH_SAMPLE_* bits, each of which must also be in `fields` (its term needs that field's sum); 0 asks for
 * the fill gradient alone.  The base planes of a gradient-carrying call come through sph_sample_grid_download /
 * sph_sample_points_download and equal those of the plain call bit for bit; the gradient planes come through the two downloads
 * below as [3 + 3 Fg][nodes] or [3 + 3 Fg][m], Fg the number of bits of `gradients`.  The plain calls run the kernels they ran
 * before.  Everything said above about selection, freshness, determinism, buffers and what is written holds unchanged.
 * SPH_E_INVALID: every refusal of the plain calls; unknown bits in `gradients`; a bit of `gradients` that is not in `fields`; a
 * gradients download whose size does not match the last sample of that kind.  SPH_E_STATE: a gradients download before any
 * sample of that kind, or when the last one carried no gradients; a slab rank.  A refused call changes nothing.
 * ------------------------------------------------------------------------------------ */
int32_t sph_sample_grid_gradients(SphContext* ctx, const SphSampleGrid* grid, int32_t gradients);   /* enqueues */
int32_t sph_sample_grid_gradients_download(SphContext* ctx, int64_t* grads /* [3 + 3 Fg][nodes] */, int64_t nodes);   /* synchronises */
int32_t sph_sample_points_gradients(SphContext* ctx, const float* xyz /* host, [m][3] */, int32_t m, int32_t fields, int32_t gradients,
                                    const SphSampleSelect* select, float inv_h);                   /* enqueues */
int32_t sph_sample_points_gradients_download(SphContext* ctx, int64_t* grads /* [3 + 3 Fg][m] */, int32_t m);        /* synchronises */

/* ======================================================================================
 * Surface mesh (the reference offers exportPly, particles to be meshed elsewhere): the fluid surface as an indexed triangle mesh,
 * by SURFACE NETS on a sampled grid -- one vertex per mixed cell, one quad per sign-changing grid edge.  (Named sph_mesh_: "surface"
 * is the screen-space frame style.)
 * INPUT: the weight plane of the LAST successful sph_sample_grid of the context (any fields, also none; the selection of that call
 * decides what the surface encloses), with the n, origin and spacing of that grid.  Node (k0, k1, k2) has linear index
 * L = (k0 * n1 + k1) * n2 + k2.  Every n[a] >= 2 is needed.
 * THRESHOLD: T = llrint((double)iso * 2^30), iso an f32 that is finite and in (0, 4].  weight / 2^30 is about 0.8 inside a fluid at
 * rest spacing and falls to 0 across the free surface.
 * CAPPED FIELD: phi(node) = 0 if `cap` is set and the node lies on the outer layer of the grid (some k_a == 0 or k_a == n_a - 1),
 * otherwise phi(node) = weight[node].  A node is INSIDE iff phi >= T.  With cap the mesh is closed wherever the fluid meets the
 * grid's border; without it the mesh is open there.
 * CELLS: cell c = (c0, c1, c2), 0 <= c_a <= n_a - 2, linear index (c0 * (n1 - 1) + c1) * (n2 - 1) + c2, is ACTIVE iff its 8 corners
 * are neither all inside nor all outside.
 * VERTEX of an active cell.  Its 12 edges are visited in this order: for axis a = 0, 1, 2, with b < c the other two axes, the
 * corner bits (i_b, i_c) run (0,0), (1,0), (0,1), (1,1).  An edge from corner lo to lo + e_a CROSSES iff exactly one end is inside;
 * its crossing parameter is t = (double)(T - phi_lo) / (double)(phi_hi - phi_lo), both differences formed in i64 first (exact:
 * weights stay below 2^41 at the bound stated for the sampling: 2^9 contributors of at most 4 * 2^30); its crossing point in
 * cell-local units has component a equal to t and components b, c equal to the corner bits.  The crossing points are summed per
 * component in f64, in that order, starting from 0.0, and divided by the number m of crossing edges; u_a = (float)mean_a;
 *     pos_a = origin_a + ((float)c_a + u_a) * spacing_a            in f32, not contracted.
 * NORMAL of that vertex: g_a = the i64 sum over the cell's 4 edges along a of phi_hi - phi_lo; gd_a = (double)g_a;
 * s = (gd0*gd0 + gd1*gd1) + gd2*gd2; n_a = (float)(-gd_a / sqrt(s)), and (0, 0, 0) when s == 0.  It points out of the fluid.
 * VERTEX NUMBERING: active cells by ascending cell linear index.
 * FACES: node k owns the three edges k -> k + e_a; the axis triples (a, b, c) are (0,1,2), (1,2,0), (2,0,1).  An owned edge emits a
 * quad iff it crosses and k_a <= n_a - 2, 1 <= k_b <= n_b - 2, 1 <= k_c <= n_c - 2, that is, all four cells round it exist (with
 * cap this holds for every crossing edge).  The quad's vertices are those of the cells with low corners C0 = k - e_b - e_c,
 * C1 = k - e_c, C2 = k, C3 = k - e_b, all active by construction.  If lo is inside and hi outside the triangles are (C0, C1, C2),
 * (C0, C2, C3), otherwise (C0, C3, C2), (C0, C2, C1).  Quads are ordered by ascending key 3 * L + a; quad q gives triangles 2q, 2q+1.
 * So the whole result -- counts, positions, normals, index buffer -- is one function of the weight plane and (iso, cap), independent
 * of scheduling.  csrc/sph_mesh.hip describes the kernels.
 * sph_mesh_extract classifies, scans, and emits vertices and faces on the context's stream; it synchronises once (the counts size
 * the buffers) and the counts are known when it returns.  sph_mesh_counts returns them; sph_mesh_download copies positions [V][3],
 * normals [V][3] and triangles [T][3] (any pointer may be NULL; sizes 0 are fine) and synchronises.  The mesh lives in buffers of its
 * own: a later sph_sample_grid changes nothing of a mesh already extracted.  Buffers grow only, are allocated on first use and freed
 * with the context; a context that never meshes allocates nothing.  Nothing of the particle state and nothing of the sampler's
 * planes is written.
 * SPH_E_INVALID: a NULL spec; iso not finite or outside (0, 4]; a sampled grid with an n[a] < 2; download sizes that do not match
 * the last extract.  SPH_E_STATE: no sampled grid yet; a slab rank; counts or download before any extract.  A refused call leaves
 * the last good mesh downloadable.
 * ==================================================================================== */
typedef struct SphMeshSpec { float iso; int32_t cap; } SphMeshSpec;
int32_t sph_mesh_extract(SphContext* ctx, const SphMeshSpec* spec);     /* on the last sampled grid; counts are known on return */
int32_t sph_mesh_counts(SphContext* ctx, int64_t* vertices, int64_t* triangles);
int32_t sph_mesh_download(SphContext* ctx, float* pos /*[V][3]*/, float* nrm /*[V][3]*/, int32_t* tri /*[T][3]*/,
                          int64_t vertices, int64_t triangles);         /* any pointer may be NULL; synchronises */

/* ======================================================================================
 * Passive tracers (the reference has none; every observer above is Eulerian): a context may hold ONE set of m tracers,
 * 0 <= m <= SPH_TRACERS_MAX: massless points that follow the flow, for pathlines, streaklines, dye and residence times.  No sweep
 * ever sees them and nothing of the particle state is written for them.
 * THE HOOK: while a set is registered, every step of sph_step / sph_dfsph_step advances it by ONE forward-Euler step with the state
 * at the BEGINNING of that step.  The advance is enqueued right behind the step's sort, before the step's sweeps: there the current
 * cell array (the inclusive prefix over the G cells) describes exactly the positions of the sorted records, and their velocities are
 * v(t_k).  One launch per step on the context's stream, no synchronisation, nothing crosses to the host; in a timed step
 * (SPH_OPT_TIMING) it falls into neighbour_ms.  With no set registered (never set, or cleared) both step calls enqueue exactly what
 * they enqueue without this section.  The per-kernel entry points (sph_compute_densities, ...) and the slab calls never advance it.
 * GATHER of one tracer at position p (f32): its cell coordinates are c_a = (int)(p_a / grid_size) -- the IEEE f32 division and the
 * truncation the sort hashes the particles with, here WITHOUT a clamp.  CANDIDATES are the records of the 27 cells (c0+i, c1+j, c2+k),
 * i, j, k in {-1, 0, 1}; a cell with a coordinate outside [0, grid_num) is skipped; cell f (flat index (cx * ny + cy) * nz + cz)
 * holds the records [f > 0 ? cell_end[f-1] : 0, cell_end[f]).  (The sort clamps a PARTICLE's cell coordinates into the grid, so a
 * particle outside the domain is a candidate through the border cell it was hashed into.)  A candidate CONTRIBUTES iff it is
 * SELECTED by the set's SphSampleSelect (as in "Field sampling") and the PAIR TERM of that section admits it: the same dx, r2, r, q,
 * W, w sequence, verbatim, with inv_h = 1.f / support_radius formed in f32 by the library, the correctly rounded sqrt and the clamp
 * of w to [0, 4].  So the contributing set is "in the 27 cells AND q <= 1.0f": a record that a rounding error puts outside that block
 * does not contribute even if its q <= 1.0f.  Per tracer, over its contributing candidates:
 *     count  += 1                                                                        (i32)
 *     weight += llrint((double)w * 2^30)                                                 (i64)
 *     sum_a  += llrint(((double)w * (double)fmaxf(fminf(v_a, 2^24), -2^24)) * 2^30)      (i64; a = x, y, z)
 * the sampler's scale, rounding and bounds.  All sums are integers: the result does not depend on the order of the records or on how
 * the work is split.
 * ADVANCE: min_weight = max(llrint((double)min_fill * 2^30), 1), computed once per set.  A tracer is WET this step iff
 * weight >= min_weight.  A wet tracer moves, in f32 with the multiply and the add NOT contracted:
 *     u_a = (float)((double)sum_a / (double)weight);   xn_a = x_a + dt * u_a;   x_a = fminf(fmaxf(xn_a, padding), wall_hi_a)
 * and its wet_steps += 1.  A dry tracer gets u = 0, keeps its position, and its dry_steps += 1.  dt is the context's f32 dt at that
 * step (sph_set_dt between calls is honoured).  weight, count and u are those of the LAST advance.
 * HISTORY: with record_every > 0, every record_every-th advance since the set was made also stores all m new positions as frame f
 * of a device buffer [record_capacity][m][3] f32 while f < record_capacity; later frames are counted as dropped and not stored.
 * sph_step(ctx, 1000, ...) then yields whole pathlines in one download at its end.
 * WHAT IS WRITTEN: the tracer buffers, nothing else.  Density / pressure of a fused step are not materialised, no derived-state flag
 * is touched (SPH_OPT_SORT_FAST stays eligible): a run with tracers ends bit-identical to the run without.
 * sph_tracers_set copies the m points (xyz: host pointer, free again when the call returns: the call synchronises), REPLACES the set
 * and zeroes its counters and its history; m == 0 clears the set and frees nothing.  sph_tracers_info returns m, the advances made,
 * the frames stored and the frames dropped; it holds no device data and does not synchronise.  sph_tracers_download copies the
 * state of the m tracers (any pointer may be NULL) and synchronises; sph_tracers_history_download copies the stored frames
 * [frames][m][3], `frames` being exactly the number stored, and synchronises.  Buffers are allocated by the first set, grow only and
 * are freed with the context; a context that never sets tracers allocates nothing.
 * SPH_E_INVALID: m outside [0, SPH_TRACERS_MAX]; a point that is not finite or lies outside [padding, wall_hi_a] on some axis;
 * min_fill not finite or outside (0, 4]; a negative record_every or record_capacity; record_capacity * m * 12 bytes above 2^31;
 * material outside [-1, 255] or n_objects outside [0, SPH_SAMPLE_MAX_OBJECTS]; a download whose m (or frames) does not match.
 * SPH_E_STATE: a download before any set; a slab rank (set and downloads).  A refused call changes nothing: the last good set goes
 * on being advanced and stays downloadable.  Tracers are not part of a checkpoint.  csrc/sph_tracers.hip describes the kernel.
 * ==================================================================================== */
#define SPH_TRACERS_MAX (1 << 22)
typedef struct SphTracerParams {
    float min_fill;                 /* a tracer moves iff its Shepard sum (weight / 2^30) reaches this; finite, in (0, 4] */
    int32_t record_every;           /* 0: no history; k > 0: every k-th advance stores a frame */
    int32_t record_capacity;        /* frames the history holds */
    SphSampleSelect select;         /* whose velocity the tracers follow */
} SphTracerParams;
typedef struct SphTracerInfo {
    int32_t m;                      /* tracers of the registered set (0: none) */
    int32_t reserved_;
    int64_t advances;               /* since the set was made */
    int64_t frames;                 /* history frames stored */
    int64_t dropped;                /* history frames that found the buffer full */
} SphTracerInfo;
int32_t sph_tracers_set(SphContext* ctx, const float* xyz /* host, [m][3] */, int32_t m, const SphTracerParams* params);   /* synchronises */
int32_t sph_tracers_info(SphContext* ctx, SphTracerInfo* info);
int32_t sph_tracers_download(SphContext* ctx, float* x /*[m][3]*/, float* u /*[m][3]*/, int64_t* weight, int32_t* count,
                             int32_t* wet_steps, int32_t* dry_steps, int32_t m);   /* any pointer may be NULL; synchronises */
int32_t sph_tracers_history_download(SphContext* ctx, float* xyz /*[frames][m][3]*/, int64_t frames, int32_t m);   /* synchronises */

/* ======================================================================================
 * Running flow statistics (the reference has none; every Eulerian observer above is of one instant): a context may hold ONE
 * registered statistics set -- a grid as in "Field sampling" (a volume, or a slice when one n[a] is 1), whose nodes accumulate ON THE
 * DEVICE, across steps, how often they were wet and the first and second moments of the velocity there: time-mean velocity, RMS
 * fluctuations, Reynolds stresses, turbulent kinetic energy and intermittency follow on the host from 11 integers per node.
 * VELOCITY ONLY: grid.fields must be 0 or exactly SPH_SAMPLE_VX | SPH_SAMPLE_VY | SPH_SAMPLE_VZ (both mean the same).  Density and
 * pressure statistics are out of scope: at the hook below those of a fused step lie in the step's own record in the PRE-sort order,
 * and materialising them would write particle state.  A sample reads positions, volumes, velocities and flags and nothing else.
 * THE HOOK: while a set is registered, every step of sph_step / sph_dfsph_step is counted (steps_seen, from 0 at registration, carried
 * across calls), and step k is SAMPLED iff steps_seen % every == 0 before it is counted.  The sample is enqueued where the tracers
 * advance: behind the step's sort and before its sweeps, so it is of x(t_k), v(t_k) at the simulated time t_k of the step's
 * beginning.  Two launches per sampled step on the context's stream, no synchronisation, nothing crosses to the host; in a timed step
 * (SPH_OPT_TIMING) they fall where the tracer advance falls.  With no set registered (never set, or cleared) both step calls enqueue
 * exactly what they enqueue without this section.  The per-kernel entry points and the slab calls never sample.
 * sph_stats_sample takes ONE sample of the current state outside a step, with the same two launches, at the current simulated time;
 * it does not touch steps_seen.
 * ONE SAMPLE: (a) the grid scatter of "Field sampling" -- its kernel, its pair term, its selection, its i64 terms -- with the fields
 * vx vy vz and no gradients, into a scratch of the statistics' own: per node count, weight, S_x, S_y, S_z.  The planes of the last
 * sph_sample_grid are NOT touched: they, and a mesh cut from them, survive a run with statistics.  (b) the FOLD, per node:
 *     wet  <=>  weight >= wet_min && weight > 0
 *     a node that is not wet adds nothing (no division is evaluated for it); a wet node, in f64, nothing contracted:
 *     u_a = (double)S_a / (double)weight        a = x, y, z; i64 -> f64 correctly rounded, the IEEE division
 *     u_a = fmin(fmax(u_a, -1024.0), 1024.0)
 *     n_wet      += 1
 *     sum_w      += weight                                    (exact)
 *     sum_u[a]   += llrint(u_a * 2^32)
 *     sum_uu[ab] += llrint((u_a * u_b) * 2^24)                ab = xx xy xz yy yz zz; the product rounds once, the scalings are exact
 * and the node's five scratch words are zeroed for the next sample.  All accumulators are i64 planes over the nodes, node (k0, k1, k2)
 * at (k0 * n[1] + k1) * n[2] + k2.  wet_min is in the units of the sampler's weight plane: llrint(fill * 2^30).
 * BOUND: a first-moment term is at most 2^42 and a second-moment term at most 2^44 in magnitude (equality only at the clamp), so
 * 2^19 samples fit an i64: capacity <= SPH_STATS_MAX_SAMPLES.  Once samples == capacity further samples are SKIPPED -- no launch --
 * and counted in `dropped`, as the tracers count dropped frames.
 * DETERMINISTIC: the scatter's sums are integers, every node of the fold has one owner and the fold has no atomics; there is no float
 * or double atomic anywhere.  The result is one function of the sampled states.
 * WHAT IS WRITTEN: the statistics' own planes, nothing else.  Density / pressure of a fused step are not materialised, no
 * derived-state flag is touched (SPH_OPT_SORT_FAST and SPH_OPT_SORT_LEAN stay eligible): a run with statistics ends bit-identical
 * to the run without.
 * sph_stats_set REPLACES the set and zeroes its accumulators and counters; NULL clears the set (and frees nothing); it synchronises.
 * sph_stats_reset zeroes accumulators and counters (steps_seen too) and keeps the set; it synchronises.  sph_stats_info returns host
 * data only and does not synchronise: the grid, `every`, the samples taken and dropped, steps_seen and the simulated times of the
 * first and the last sample (0 while there is none); all zero without a set.  sph_stats_download copies n_wet [nodes], sum_w
 * [nodes], sum_u [3][nodes], sum_uu [6][nodes] (any pointer may be NULL) and synchronises.  The planes are allocated by the first
 * set, again when a later grid needs more, and freed with the context; a context that never registers statistics allocates nothing.
 * SPH_E_INVALID: every refusal of sph_sample_grid for the grid (the same checks); grid.fields other than 0 or vx | vy | vz;
 * every < 1; capacity outside [1, SPH_STATS_MAX_SAMPLES]; wet_min < 0; a download whose `nodes` does not match the set.
 * SPH_E_STATE: a sample, download or reset without a registered set; a slab rank (set, sample, download, reset).  A refused
 * sph_stats_set changes nothing: the last good set goes on being sampled and stays downloadable.  Statistics are not part of a
 * checkpoint.  csrc/sph_stats.hip describes the fold kernel.
 * ==================================================================================== */
#define SPH_STATS_MAX_SAMPLES (1 << 19)
typedef struct SphStatsParams {
    SphSampleGrid grid;             /* geometry, inv_h and selection as for sph_sample_grid; fields 0 or vx | vy | vz */
    int32_t every;                  /* >= 1: every every-th step of the context is sampled */
    int32_t capacity;               /* samples the set accepts, in [1, SPH_STATS_MAX_SAMPLES] */
    int64_t wet_min;                /* a node is wet iff weight >= wet_min && weight > 0; >= 0 */
} SphStatsParams;
typedef struct SphStatsInfo {
    int64_t nodes;                  /* of the registered grid (0: no set) */
    int32_t n[3];
    int32_t every;
    int64_t samples, dropped, steps_seen;
    double t_first, t_last;         /* simulated time of the first and the last sample taken */
} SphStatsInfo;
int32_t sph_stats_set(SphContext* ctx, const SphStatsParams* params);   /* NULL clears; synchronises */
int32_t sph_stats_sample(SphContext* ctx);                              /* one sample of the current state; enqueues */
int32_t sph_stats_info(SphContext* ctx, SphStatsInfo* info);            /* host data only */
int32_t sph_stats_download(SphContext* ctx, int64_t* n_wet, int64_t* sum_w, int64_t* sum_u /*[3][nodes]*/, int64_t* sum_uu /*[6][nodes]*/,
                           int64_t nodes);                              /* any pointer may be NULL; synchronises */
int32_t sph_stats_reset(SphContext* ctx);                               /* keeps the set; synchronises */

/* ======================================================================================
 * Fluid loads (the reference has none; the force sweep keeps the boundary term only as the fluid's acceleration): a context may hold
 * ONE registered load set -- up to SPH_LOADS_MAX_OBJECTS solid objects (static, kinematic or dynamic) -- for which it records, as a
 * time series ON THE DEVICE, the force and the torque the fluid exerts on each object.  WCSPH only.
 * THE QUANTITY.  For a solid particle j of a selected object and a fluid particle i with r = |x_i - x_j| < h:
 *     F_j = sum_i  m_i * rho0 * m_V_j * (p_i / rho_i^2 + p_i / rho0^2) * gradW(x_i - x_j)
 * which is minus m_i times the acceleration WCSPH.py:58-68 gives fluid i from boundary particle j (the reference has no boundary
 * viscosity, so this is the whole fluid-solid interaction).  Per object: force = sum_j F_j; torque = sum_j (x_j - c) x F_j about ONE
 * fixed world point c of the set (`about`); the number of contributing pairs; of wet solid particles (at least one pair); of
 * saturated terms.  Nine i64 per object and sample, in this order: Fx Fy Fz Tx Ty Tz pairs wet saturated.  Forces are in N and
 * torques in N m at scale 2^24: value = integer / 2^24.
 * TERM BY TERM.  Candidates of target j are the records of the 27 cells around the cell the sort hashed j into (its clamped cell
 * coordinates), read through the cell array; a candidate contributes iff it is of fluid material and, with the pair geometry of
 * "Field sampling" taken verbatim (f32: d_a = x_i,a - x_j,a; r2 = (dx*dx + dy*dy) + dz*dz; r = sqrtf(r2) correctly rounded;
 * q = r * inv_h, inv_h = 1.f / support_radius), q <= 1.0f and r > 1e-5f.  (A pair that a rounding error puts outside the 27 cells
 * although its q <= 1.0f does not contribute; its term would be of the order of the last bit of q.)  Then in f64, every operation
 * an IEEE multiply, divide or subtract, nothing contracted, no f32 divide, no reciprocal or reciprocal square root:
 *     g    = q <= 0.5 ? q * (3.0 * q - 2.0) : -((1.0 - q) * (1.0 - q))
 *     dp   = p_i / (rho_i * rho_i) + p_i / (rho0 * rho0)
 *     coef = (((m_i * rho0) * m_V_j) * dp) * ((k_dw * g) / (r * h))
 *     f_a  = coef * d_a;   c_a = fmin(fmax(f_a, -65536.0), 65536.0);   saturated += (c_a != f_a);   F_j,a += llrint(c_a * 2^24)
 * with m_i, rho_i, p_i the f32 mass, density and pressure of i as this step computed them, m_V_j the f32 boundary volume, and rho0,
 * k_dw, h = support_radius the context's f32 parameters, each converted to f64.  A NaN ends at -65536 and is counted.  F_j is the
 * INTEGER sum of its pair terms.  The torque term of target j, with a_b = (double)(x_j,b - about_b) (the subtraction in f32) and
 * F_b = (double)F_j,b / 2^24:
 *     T_x = a_y * F_z - a_z * F_y  (cyclic);   s = T_a * 2^24;   c = fmin(fmax(s, -2^40), 2^40);   saturated += (c != s);   T += llrint(c)
 * OVERFLOW BUDGET: a force term is at most 2^40 in magnitude and so is a torque term: 2^22 pair terms (or targets) AT THE CLAMP
 * still fit an i64.  DETERMINISTIC: every accumulation is an integer add (lane sums, DPP row sums, no-return i64 atomics into the
 * sample's own row), so the nine numbers are one function of the sampled state, whatever the lane split, the launch order or the
 * order the atomics arrive in.  There is no float or double atomic.
 * THE HOOK: while a set is registered, every step of sph_step (and of sph_sweeps) is counted (steps_seen, from 0 at registration), and
 * step k is SAMPLED iff steps_seen % every == 0 before it is counted.  The sample is enqueued directly behind the step's density and
 * equation of state and before its force sweep: the positions are x(t_k), the cell array is this step's sort, p and rho are this
 * step's -- exactly what the force sweep then uses.  Density and pressure of a fused step are materialised in the particle record
 * first (the values every later reader would get anyway).  Sample k writes row k of the history at time = the simulated time t_k.  One
 * 4-byte clear and two launches per sampled step on the context's stream, no synchronisation, nothing crosses to the host.  Once
 * samples == capacity further samples are SKIPPED -- no launch -- and counted in `dropped`.  With no set registered (never set, or
 * cleared) the step enqueues exactly what it enqueues without this section.  While a set is registered SPH_OPT_SORT_LEAN is not
 * taken (the sample reads the particle record); positions and velocities of a run with a set are bit-identical to the run without.
 * sph_dfsph_step with a registered set returns SPH_E_STATE: DFSPH couples through velocity changes, loads there are out of scope.
 * sph_loads_sample takes ONE sample of the current state outside a step -- for callers that drive the kernels stage by stage -- with
 * whatever density and pressure the particle record holds; it needs the neighbour structure of the current positions
 * (sph_initialize_particle_system) and does not touch steps_seen.
 * sph_loads_set REPLACES the set, zeroes its history and counters and synchronises; NULL clears the set (and frees nothing).
 * sph_loads_reset zeroes history and counters and keeps the set; it synchronises.  sph_loads_info returns host data only.
 * sph_loads_download copies rows [samples][n_objects][9] and times [samples] (either may be NULL), `samples` and `n_objects` being
 * exactly the info's, synchronises, then checks the device's error flags.  Buffers are allocated by the first set (a target list of
 * the context's record capacity, the history, the times), grow only and are freed with the context.
 * SPH_E_INVALID: n_objects outside [1, SPH_LOADS_MAX_OBJECTS]; an object id outside [0, the context's n_objects); a duplicate id; a
 * non-finite `about`; every < 1; capacity < 1 or a history above 2^31 bytes; a download whose sizes do not match.
 * SPH_E_STATE: a sample, download or reset without a registered set; a sample without the neighbour structure; sph_dfsph_step with a
 * registered set; a slab rank (every entry but info).  A refused sph_loads_set changes nothing.  Loads are not part of a checkpoint
 * (save_state).  csrc/sph_loads.hip describes the kernels.
 * ==================================================================================== */
#define SPH_LOADS_MAX_OBJECTS 32
#define SPH_LOADS_ROW_WORDS 9
#define SPH_LOADS_SCALE_LOG2 24
typedef struct SphLoadParams {
    int32_t object_ids[SPH_LOADS_MAX_OBJECTS];   /* slot k of every history row is object_ids[k] */
    int32_t n_objects;              /* in [1, SPH_LOADS_MAX_OBJECTS] */
    float about[3];                 /* the fixed world point the torques are about */
    int32_t every;                  /* >= 1: every every-th step of the context is sampled */
    int32_t capacity;               /* >= 1: rows the history holds */
} SphLoadParams;
typedef struct SphLoadInfo {
    int32_t n_objects;              /* of the registered set (0: no set) */
    int32_t every;
    int64_t samples, dropped, steps_seen;
} SphLoadInfo;
int32_t sph_loads_set(SphContext* ctx, const SphLoadParams* params);    /* NULL clears; synchronises */
int32_t sph_loads_sample(SphContext* ctx);                              /* one sample of the current state; enqueues */
int32_t sph_loads_info(SphContext* ctx, SphLoadInfo* info);             /* host data only */
int32_t sph_loads_download(SphContext* ctx, int64_t* rows /*[samples][n_objects][9]*/, double* times /*[samples]*/, int64_t samples,
                           int32_t n_objects);                          /* either pointer may be NULL; synchronises */
int32_t sph_loads_reset(SphContext* ctx);                               /* keeps the set; synchronises */

/* ======================================================================================
 * Carried scalars (the reference has none: a particle carries position, velocity, density, pressure and an object colour): a context
 * may hold ONE scalar set of K channels, 1 <= K <= SPH_SCALARS_MAX_CHANNELS -- dye, heat, a concentration -- that ride on the
 * particles (advection is free in a Lagrangian method) and DIFFUSE between neighbours, on the device, inside the step.
 * THE STORE.  int64 C[id][k], indexed by PERSISTENT id (channel fastest), the physical value times 2^32 (SPH_SCALARS_SCALE_LOG2),
 * |value| <= 2^20 when set.  The sort never moves it and does not know it exists.  A difference of two stored values is an exact f64.
 * WHO TAKES PART.  SOURCES: the records (fluid or solid) of up to SPH_SCALARS_MAX_SOURCES objects hold a prescribed value per channel
 * (Dirichlet: a body at 350 K); a source is never updated and its stored value is not read.  CARRIERS: the records selected by
 * `select` (as in "Field sampling") that are not of a source object and whose id is inside the store.  Every other record is
 * invisible to the sum: zero flux, the natural SPH wall.
 * ONE SAMPLE is one explicit Jacobi step of Brookshaw's Laplacian, the form of the reference's viscosity term (sph_base.py:71-78):
 *     C_i <- C_i + a * sum_j m_V_j (C_j - C_i) * (-2 (r . gradW) / (r^2 + 0.01 h^2)),       a = dt * every * kappa
 * TERM BY TERM.  All reads are from a SNAPSHOT of the participants' values taken before any write.  Candidates of carrier i are the
 * records of the 27 cells around the cell the sort hashed i into (its clamped cell coordinates), read through the cell array, runs
 * clipped to [0, N]; candidate j contributes iff it takes part and, with the pair geometry of "Field sampling" taken verbatim (f32:
 * d = x_i - x_j; r2 = (dx*dx + dy*dy) + dz*dz; r = sqrtf(r2) correctly rounded; q = r * inv_h, inv_h = 1.f / support_radius),
 * q <= 1.0f and r > 1e-5f (which excludes i itself).  Then in f64 from those f32 values, every operation an IEEE multiply, add or
 * divide, nothing contracted (h = support_radius, k_dw the context's folded constant, both f32 converted):
 *     g    = q <= 0.5 ? q * (3.0 * q - 2.0) : -((1.0 - q) * (1.0 - q))                        (as in "Fluid loads")
 *     lap  = ((2.0 * (k_dw * g)) * r) / (h * (r * r + (0.01 * h) * h))                        <= 0
 *     and per channel k, with a_k = ((double)dt * (double)every) * (double)kappa_k formed once per sample on the host:
 *     w_k    = fmin(fmax((-(a_k * (double)m_V_j)) * lap, 0.0), 1.0)                            (a NaN gives 0)
 *     term_k = llrint((double)(C_k[j] - C_k[i]) * w_k);      wsum_k += llrint(w_k * 2^32)
 *     C_k[i] <- clamp(C_k[i] + sum_j term_k, -2^52, 2^52)
 * A carrier whose wsum_k > 2^32 is counted in overshoot[k]: the explicit step is beyond its stability limit there (the new value
 * may leave the range of its neighbours'), lower kappa or `every`.  A result the clamp changed is counted in saturated[k].  Both
 * counters run from the set on.  BUDGET: |C_j - C_i| <= 2^53 and w <= 1, so 2^9 pair terms at the extreme still fit an i64.
 * DETERMINISTIC: every sum is an integer sum (lane sums, DPP row sums), so the result depends neither on record order nor on the
 * work split, and a brute-force model reproduces every word.  Where all participants have bit-equal m_V (one fluid),
 * term_ij = -term_ji exactly, so with no sources sum_i C_k[i] is conserved to the last bit (unless a value saturates); with unequal
 * volumes conservation holds to rounding only.
 * THE HOOK: while a set is registered every step of sph_step and sph_dfsph_step is counted (steps_seen, from 0 at the set), and step k
 * is SAMPLED iff steps_seen % every == 0 before it is counted; the sample is enqueued behind the step's sort and before its sweeps:
 * positions x(t_k), this step's cell array.  One 4-byte clear and two launches on the context's stream (the stage: snapshot, roles
 * and the carriers' index list with its count, which stays on the device; the diffusion), no synchronisation, nothing crosses to the
 * host, no particle state is written: a run with a set is bit-identical in x, v, density, pressure to the run without, and keeps its
 * lean and fast sorts.  With no set registered the step loops enqueue exactly what they enqueue without this section.  The
 * per-kernel entries and the slab calls never sample.  sph_scalars_sample takes ONE sample of the current state outside a step; it
 * needs the neighbour structure of the current positions (sph_initialize_particle_system) and does not touch steps_seen.
 * sph_scalars_set REPLACES the set: `values` is f64 [n_ids][K] in id order (NULL: zeros), stored as llrint(value * 2^32); counters
 * start from zero; params->K == 0 (or params NULL) clears the set (values and n_ids are then not read); synchronises.
 * sph_scalars_info: host counters and the two device counters (synchronises).  sph_scalars_download: raw i64 [n_ids][K] and / or
 * values f64 [n_ids][K] = raw / 2^32 (either may be NULL), n_ids being the set's; synchronises.
 * sph_scalars_paint(ctx, channel, lo, hi, lut): one streaming pass that writes, for every carrier and source record, the table
 * colour of its value (a source: the prescribed one) into the object colour of its id (SPH_F_COLOR, which both frame styles draw),
 * and nothing else: s = (float)((double)C * 2^-32), then the index arithmetic of "Field colouring" verbatim -- t = (s - lo) * inv,
 * inv = 1.f / (hi - lo); t = t >= 0 ? min(t, 1) : 0; idx = int(t * 255 + 0.5) -- and colour[c] = lut[idx][c], lut 256 x 3 int32
 * in [0, 255].  An explicit call; other records keep their colour.  Enqueues.
 * Buffers (store, snapshot, list, counters, table) are allocated by the first set, grow only and are freed with the context; a
 * context that never sets scalars allocates nothing.
 * TEST AID: the environment variable SPH_SCALARS_BLOCKS = b >= 1, read by sph_scalars_set, caps the diffusion's grid at b blocks of
 * sixteen rows (it can only shrink the grid; results are the same words): the waves then take several trips over a short list, which
 * a small test scene would never make them do.  Not for production use.
 * SPH_E_INVALID: K outside [0, SPH_SCALARS_MAX_CHANNELS]; every < 1; n_sources outside [0, SPH_SCALARS_MAX_SOURCES]; a source object
 * outside [0, the context's n_objects) or named twice; a selection out of range; kappa negative or not finite; a value (initial or
 * source) not finite or beyond 2^20 in magnitude; n_ids < 1 or above the cold capacity; a download with another n_ids; paint: a
 * channel outside [0, K), lo or hi not finite, lo >= hi, a reciprocal width that is not a positive finite f32, a NULL table or an
 * entry outside [0, 255].  SPH_E_STATE: sample, download or paint without a set; a sample without the neighbour structure; a slab
 * rank (every entry but info).  A refused call changes nothing: the last good set goes on sampling.  (A DEVICE error during the
 * upload of a set that passed every check -- none is known to occur -- returns the HIP error code and leaves NO set registered: the
 * old one had to go before the new one could be written.)  Scalars are not part of a
 * checkpoint (save_state): download the values and set them again.  csrc/sph_scalars.hip describes the kernels.
 * ==================================================================================== */
#define SPH_SCALARS_MAX_CHANNELS 4
#define SPH_SCALARS_MAX_SOURCES 8
#define SPH_SCALARS_SCALE_LOG2 32
typedef struct SphScalarParams {
    int32_t K;                      /* channels, 1 .. SPH_SCALARS_MAX_CHANNELS; 0 clears the set */
    float kappa[SPH_SCALARS_MAX_CHANNELS];   /* diffusivity per channel, m^2/s, >= 0 */
    int32_t every;                  /* >= 1: every every-th step of the context is sampled, with a = dt * every * kappa */
    SphSampleSelect select;         /* the carriers */
    int32_t n_sources;              /* 0 .. SPH_SCALARS_MAX_SOURCES */
    int32_t source_object[SPH_SCALARS_MAX_SOURCES];
    double source_value[SPH_SCALARS_MAX_SOURCES][SPH_SCALARS_MAX_CHANNELS];
} SphScalarParams;
typedef struct SphScalarInfo {
    int32_t K;                      /* of the registered set (0: no set) */
    int32_t every;
    int64_t ids;                    /* n_ids of the set */
    int64_t samples, steps_seen;
    int64_t overshoot[SPH_SCALARS_MAX_CHANNELS], saturated[SPH_SCALARS_MAX_CHANNELS];
} SphScalarInfo;
int32_t sph_scalars_set(SphContext* ctx, const double* values /* host, [n_ids][K], id order; NULL: zeros */, int64_t n_ids,
                        const SphScalarParams* params);                 /* K == 0 clears; synchronises */
int32_t sph_scalars_sample(SphContext* ctx);                            /* one sample of the current state; enqueues */
int32_t sph_scalars_info(SphContext* ctx, SphScalarInfo* info);         /* synchronises when a set is registered */
int32_t sph_scalars_download(SphContext* ctx, int64_t* raw /*[n_ids][K]*/, double* values /*[n_ids][K]*/, int64_t n_ids);   /* synchronises */
int32_t sph_scalars_paint(SphContext* ctx, int32_t channel, float lo, float hi, const int32_t* lut /* host, 256 x 3 */);   /* enqueues */

/* ======================================================================================
 * Particle features (the reference has none): a context may hold ONE registered feature set, for which it evaluates the flow AT THE
 * PARTICLES THEMSELVES -- vorticity, velocity divergence, the colour gradient (a raw surface normal), the kernel fill, the neighbour
 * counts and a free-surface flag -- inside the step, ON THE DEVICE, one 64-byte row per persistent id.  WCSPH only.
 * THE SET.  TARGETS are the records selected by `select` (as in "Field sampling": a material, -1 = any, and up to 32 object ids, 0 =
 * all).  CANDIDATES of target i are the records j of the 27 cells around the cell the sort hashed i into (its clamped cell
 * coordinates), read through the cell array, runs clipped to [0, N], of EVERY material and object (a record that is no target is a
 * candidate all the same).
 * TERM BY TERM.  The pair geometry of "Field sampling" taken verbatim (f32: d_a = x_i,a - x_j,a; r2 = (dx*dx + dy*dy) + dz*dz;
 * r = sqrtf(r2) correctly rounded; q = r * inv_h, inv_h = 1.f / support_radius); a pair contributes iff q <= 1.0f and r > 1e-5f
 * (which excludes i itself; a pair that a rounding error puts outside the 27 cells although its q <= 1.0f does not contribute).
 * P(q) is the kernel polynomial of "Field sampling" in f32 with k_w = 1: q <= 0.5f ? (6.f*q3 - 6.f*q2) + 1.f : 2.f * ((t*t)*t),
 * q2 = q*q, q3 = q2*q, t = 1.f - q.  Then in f64 from those f32 values, every operation an IEEE multiply, divide or subtract, nothing
 * contracted, no f32 divide, no reciprocal (the rules of "Fluid loads"; h = support_radius, k_w and k_dw the context's f32
 * parameters, each converted):
 *     V_j  = fluid material ? (double)m_j / (double)rho_j : (double)m_V_j          (rho_j: the density this step computed)
 *     g    = q <= 0.5 ? q * (3.0 * q - 2.0) : -((1.0 - q) * (1.0 - q))           (as in "Fluid loads")
 *     gW_b = ((k_dw * g) / (r * h)) * d_b
 *     fill term   V_j * (k_w * P)                              clamp 2^14, scale 2^30 (SPH_FEATURES_FILL_SCALE_LOG2)
 *     N_b  term   V_j * gW_b                                   clamp 2^20, scale 2^24 (SPH_FEATURES_SCALE_LOG2), every material
 *     G_ab term   (V_j * (double)(v_j,a - v_i,a)) * gW_b       clamp 2^20, scale 2^24, FLUID candidates only; the difference in f32
 * each term f: c = fmin(fmax(f, -limit), limit); saturated += (c != f); sum += llrint(c * scale).  A NaN ends at -limit and is
 * counted.  The fill has one more term, the target's own: V_i * (k_w * 1.0), clamped and rounded alike.  n_fluid and n_solid count the
 * contributing pairs with a fluid and with any other candidate.  G_ab is d v_a / d x_b in DIFFERENCE form without renormalisation:
 * exact for a uniform flow, first order only where the kernel support is full.
 * OVERFLOW BUDGET: a term is at most 2^44 in magnitude: 2^18 pair terms AT THE CLAMP still fit an i64, sums of three or differences of
 * two of them included.  DETERMINISTIC: every accumulation is an integer add (lane sums, DPP row sums; the only atomics are integer
 * adds on the target list's count), so a row is one function of the sampled state, whatever the lane split or the launch order.
 * There is no float or double atomic.
 * THE ROW (SphFeatureRow, stored BY PERSISTENT ID, not in sorted order; a row outside the selection is all zero).  Every float is
 * (float)((double)I / 2^s) of an integer sum I or of an integer sum or difference of such sums:
 *     vorticity = (G_zy - G_yz, G_xz - G_zx, G_yx - G_xy);   divergence = (G_xx + G_yy) + G_zz;   normal = N (raw: it points INTO the
 *     fluid; the host normalises and flips it);   fill;   n_fluid, n_solid;   x = the f32 position at the sample;
 *     flags: SPH_FEATURE_VALID (the particle was a target), SPH_FEATURE_SURFACE, SPH_FEATURE_SATURATED (a term of it was clamped).
 * SURFACE: n_fluid + n_solid < min_neighbours, or, when normal_min > 0, (h*h) * ((Nx*Nx + Ny*Ny) + Nz*Nz) > normal_min * normal_min in
 * f64 with N_b = (double)I_b / 2^24.  The default min_neighbours = 24 comes from the rest lattice of spacing d with h = 2 d: a face
 * particle has at most 22 neighbours, any particle one layer in at least 26 even when every pair at exactly r = 2 d rounds outside
 * the support; 24 separates the two whichever way those pairs round.
 * THE HOOK: while a set is registered, every step of sph_step (and of sph_sweeps) is counted (steps_seen, from 0 at registration), and
 * step k is SAMPLED iff steps_seen % every == 0 before it is counted.  The sample is enqueued directly behind the step's density and
 * equation of state and before its force sweep: positions x(t_k), velocities v(t_k), this step's sort and density.  Density and the
 * id of a fused step are materialised in the particle record first (the values every later reader would get anyway).  Two clears (the
 * 4-byte target count, the rows) and two launches per sampled step on the context's stream, no synchronisation, nothing crosses to
 * the host.  Only the LATEST sample is kept, with its time and its step index k; there is no history.  With no set registered (never
 * set, or cleared) the step enqueues exactly what it enqueues without this section.  While a set is registered SPH_OPT_SORT_LEAN is
 * not taken (the sample reads the particle record), as with a load set; positions and velocities of a run with a set are
 * bit-identical to the run without.  sph_dfsph_step with a registered set returns SPH_E_STATE (WCSPH only, the precedent of the
 * load set).  COST: a 27-cell walk of every fluid particle with thirteen f64 terms per pair -- more than a carried-scalar sample, which
 * costs several steps' time -- so `every` > 1 is the normal use (profiles/features_timing.json once measured).
 * sph_features_sample takes ONE sample of the current state outside a step -- for callers that drive the kernels stage by stage --
 * with whatever density the particle record holds; it needs the neighbour structure of the current positions
 * (sph_initialize_particle_system) and does not touch steps_seen; its step index is the current steps_seen.
 * sph_features_set REPLACES the set, zeroes rows and counters and synchronises; NULL clears the set (and frees nothing).  The row
 * count is the context's id capacity.  sph_features_info returns host data only (step = -1 before the first sample).
 * sph_features_download copies the rows, n_rows being exactly the info's, synchronises, then checks the device's error flags.
 * sph_features_paint(ctx, field, lo, hi, lut): one streaming pass that writes, for every live record whose row of the latest sample is
 * valid, the table colour of the row's field into the object colour of its id (SPH_F_COLOR, which both frame styles draw), and
 * nothing else.  s (f32) is: SPH_FEATURE_FIELD_VORTICITY sqrtf((wx*wx + wy*wy) + wz*wz); _DIVERGENCE; _FILL; _NEIGHBOURS
 * (float)(n_fluid + n_solid); _SURFACE 1.f or 0.f; then the index arithmetic of "Field colouring" verbatim -- t = (s - lo) * inv,
 * inv = 1.f / (hi - lo); t = t >= 0 ? min(t, 1) : 0; idx = int(t * 255 + 0.5) -- and colour[c] = lut[idx][c], lut 256 x 3 int32 in
 * [0, 255].  An explicit call; other records keep their colour.  Enqueues.
 * Buffers (a target list of the context's record capacity, the rows, the table) are allocated by the first set, grow only and are
 * freed with the context; a context that never sets features allocates nothing.
 * TEST AID: the environment variable SPH_FEATURES_BLOCKS = b >= 1, read by sph_features_set, caps the gather's grid at b blocks of
 * sixteen rows (it can only shrink the grid; results are the same words).  Not for production use.
 * SPH_E_INVALID: a selection out of range; every < 1; min_neighbours outside [0, 2^20]; normal_min negative or not finite; a download
 * with another n_rows; paint: a field outside [0, SPH_FEATURE_FIELDS), lo or hi not finite, lo >= hi, a reciprocal width that is not
 * a positive finite f32, a NULL table or an entry outside [0, 255].  SPH_E_STATE: a sample, download or paint without a registered
 * set; a sample without the neighbour structure; sph_dfsph_step with a registered set; a slab rank (every entry but info).  A refused
 * sph_features_set changes nothing.  Features are not part of a checkpoint (save_state).  csrc/sph_features.hip describes the kernels.
 * ==================================================================================== */
#define SPH_FEATURES_SCALE_LOG2 24
#define SPH_FEATURES_FILL_SCALE_LOG2 30
#define SPH_FEATURE_VALID 1
#define SPH_FEATURE_SURFACE 2
#define SPH_FEATURE_SATURATED 4
enum SphFeatureField { SPH_FEATURE_FIELD_VORTICITY = 0, SPH_FEATURE_FIELD_DIVERGENCE, SPH_FEATURE_FIELD_FILL, SPH_FEATURE_FIELD_NEIGHBOURS,
                       SPH_FEATURE_FIELD_SURFACE, SPH_FEATURE_FIELDS };
typedef struct SphFeatureParams {
    SphSampleSelect select;         /* the targets */
    int32_t every;                  /* >= 1: every every-th step of the context is sampled */
    int32_t min_neighbours;         /* surface iff n_fluid + n_solid < min_neighbours (24: the rest lattice, above) */
    float normal_min;               /* > 0: surface also iff h |N| > normal_min; 0: off */
} SphFeatureParams;
typedef struct SphFeatureRow {      /* 64 bytes */
    float x[3];                     /* the position at the sample */
    float vorticity[3];             /* 1/s */
    float divergence;               /* 1/s */
    float normal[3];                /* the raw colour gradient N, 1/m: into the fluid */
    float fill;                     /* about 1 inside the fluid at rest */
    int32_t n_fluid, n_solid;
    int32_t flags;                  /* SPH_FEATURE_VALID | _SURFACE | _SATURATED */
    int32_t reserved_[2];           /* zero */
} SphFeatureRow;
typedef struct SphFeatureInfo {
    int32_t every;                  /* of the registered set (0: no set) */
    int32_t reserved_;
    int64_t rows;                   /* rows of a download: the context's id capacity */
    int64_t samples, steps_seen;
    int64_t step;                   /* step index of the latest sample, -1: none yet */
    double time;                    /* simulated time of the latest sample */
} SphFeatureInfo;
int32_t sph_features_set(SphContext* ctx, const SphFeatureParams* params);   /* NULL clears; synchronises */
int32_t sph_features_sample(SphContext* ctx);                                /* one sample of the current state; enqueues */
int32_t sph_features_info(SphContext* ctx, SphFeatureInfo* info);            /* host data only */
int32_t sph_features_download(SphContext* ctx, void* rows /* SphFeatureRow [n_rows] */, int64_t n_rows);   /* synchronises */
int32_t sph_features_paint(SphContext* ctx, int32_t field, float lo, float hi, const int32_t* lut /* host, 256 x 3 */);   /* enqueues */

#ifdef __cplusplus
}
#endif
#endif /* SPH_HIP_H */
