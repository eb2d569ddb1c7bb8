// sph_gather.hip -- the 27-cell neighbour sweeps K4..K7 of the hot path.
// Replaces particle_system.py:378-385 (for_all_neighbors) and the tasks it is
// instantiated with: sph_base.py:91-113 (boundary volume), WCSPH.py:19-43
// (density), WCSPH.py:88-140 (surface tension + viscosity), WCSPH.py:46-85
// (Tait EOS + pressure gradient + two-way coupling scatter).
//
// Two implementations of the same sweeps:
//  * k_gather_simple : one lane per target particle walks its 9 (x,y) cell
//    columns; the 3 z-cells of a column are ONE contiguous index range because
//    the flatten order is z-fastest (particle_system.py:294).  Candidates come
//    through L1/L2.  Same traversal order as the reference.  Used for small
//    target sets (rigid particles) and as the overflow path.
//  * k_gather_brick  : a 256-lane workgroup owns a BXxBYxBZ brick of cells and
//    stages the brick + one-cell shell (per column one contiguous segment) in
//    LDS.  FILTERING sweeps (density) test every candidate with the expanded
//    square (ds_read_b128 + 3 FMA + compare), collect hits in bitmask registers
//    and write them out as u16 neighbour lists in HBM; LIST-READING sweeps (the
//    fused force sweep, every DFSPH sweep after the density one) skip the filter
//    and run their pair physics over those lists, gathering the neighbour's
//    other records through L2 with the next entry prefetched.
// The DFSPH pair terms (DFSPH.py) are further MODEs of the same two kernels.
//
// No MFMA: this is a bandwidth/VALU-bound gather, not a contraction.
#include "sph_internal.h"
#include "sph_bricks.h"

#define TPB 256

// Section ablation (which parts of a sweep cost what: DESIGN.md "what was tried") exists only in the PROFILING build of
// this library (-DSPH_PROFILE -> libsph_hip_profile.so, built on demand by bench.py --ablate / --ablate-mask).  In the
// production build SPH_ABL is the constant 0: no mask argument, no branch, nothing to read past.
#ifdef SPH_PROFILE
#define SPH_ABL(d_, m_) ((d_).ablate & (m_))
// Per-workgroup time line (profiling build, ablate bit 28 = the list-writing sweeps, bit 29 = the list-reading ones): wave
// 0's first lane stamps the 100 MHz wall clock when the workgroup enters, after the step-A barrier (column table), after the
// step-B barrier (tile staged), when ITS target is computed (before the finish) and when it leaves, plus where it ran
// (HW_ID, XCC_ID) and how much it held -- 8 words per hardware block in d.prof_ts (sph_profile_read).  What the
// table answers: how much of a workgroup's residence is staging / compute / finish, and whether the staging of one
// resident workgroup is covered by the compute of its neighbours on the CU (tools/brick_timeline.py).
#define SPH_TS(slot_)                                                                                         \
    do {                                                                                                      \
        if (ts_on && threadIdx.x == 0) d.prof_ts[(size_t)blockIdx.x * 8 + (slot_)] = wall_clock64();          \
    } while (0)
#else
#define SPH_ABL(d_, m_) 0
#define SPH_TS(slot_) do { } while (0)
#endif

// ---------------------------------------------------------------------------
// per-target state and pair physics, shared by both implementations
// ---------------------------------------------------------------------------
struct Target {
    float x, y, z, mV;
    float vx, vy, vz;
    int flags;
    float m, rho, p, dpi;  // own mass, density (clamped where the mode needs it), pressure, p/rho^2
    float s0;              // scalar accumulator (density / boundary volume)
    float ax, ay, az;      // non-pressure accumulator (starts at g)
    float px, py, pz;      // pressure accumulator
    float st_c;            // surface_tension / m_i
    float dpj_solid;       // p_i / rho0^2 (WCSPH.py:60)
    bool self_in_sum;      // density: the brick path sums the self pair (= m_V_i W(0)) with the neighbours
    int nn;                // DFSPH.py:197 num_neighbors
    float df_err;          // density-change / -advection finish: this target's term of compute_density_error() (DFSPH.py:224-230), 0 for a non-fluid one
};

template <int MODE>
__host__ __device__ constexpr bool mode_is_df_iter_u() { return MODE == GM_DF_DIV_ITER_U || MODE == GM_DF_PRESSURE_ITER_U; }
template <int MODE>
__host__ __device__ constexpr bool mode_is_df_iter() {
    return MODE == GM_DF_DIV_ITER || MODE == GM_DF_PRESSURE_ITER || mode_is_df_iter_u<MODE>();
}
template <int MODE>
__host__ __device__ constexpr bool mode_is_df_pressure() { return MODE == GM_DF_PRESSURE_ITER || MODE == GM_DF_PRESSURE_ITER_U; }
// the sweeps a DFSPH solver iteration consists of: enqueued ahead of the previous iteration's convergence test, they leave
// at once when that test has closed the solve (DevView::gate, sph_api.hip: df_solve_loop)
template <int MODE>
__host__ __device__ constexpr bool mode_is_df_gated() {
    return MODE == GM_DF_DIV_ITER || MODE == GM_DF_PRESSURE_ITER || MODE == GM_DF_DIV_ITER_U || MODE == GM_DF_PRESSURE_ITER_U ||
           MODE == GM_DF_DENSITY_CHANGE || MODE == GM_DF_DENSITY_ADV;
}

template <int MODE>
__host__ __device__ constexpr bool mode_is_df_vdiv() { return MODE == GM_DF_DENSITY_CHANGE || MODE == GM_DF_DENSITY_ADV; }
template <int MODE>
__device__ __forceinline__ bool mode_needs_B() {
    return MODE != GM_DENSITY && MODE != GM_DENSITY_EOS && MODE != GM_DF_DENSITY && !mode_is_df_iter_u<MODE>();
}
template <int MODE>
__device__ __forceinline__ bool mode_needs_C() {
    return MODE == GM_NONPRESSURE || MODE == GM_PRESSURE || MODE == GM_FORCE_FUSED ||
           (mode_is_df_iter<MODE>() && !mode_is_df_iter_u<MODE>()) ||
           MODE == GM_DF_NONPRESSURE;  // (GM_FORCE_FUSED_U: no -- that is its point; *_ITER_U: 4 bytes, see fetch)
}
// the exact cell walk of a mode (overflow fallback): the uniform-fluid force sweep falls back to the general one
template <int MODE>
__host__ __device__ constexpr int mode_walk() {
    return MODE == GM_DF_DIV_ITER_U ? GM_DF_DIV_ITER : MODE == GM_DF_PRESSURE_ITER_U ? GM_DF_PRESSURE_ITER : MODE;
}

// is particle (flags) a gather target of this mode?
template <int MODE>
__device__ __forceinline__ bool target_gathers(int fl) {
    if (MODE == GM_BVOL_STATIC) return sph_is_static_rigid(fl);    // sph_base.py:93-94
    if (MODE == GM_BVOL_DYNAMIC) return sph_is_dynamic_rigid(fl);  // sph_base.py:108-109
    return sph_is_fluid(fl);  // WCSPH.py:36-37, 80-83, 138
}

// candidate record C = (p/rho^2, m/rho_raw, m, rho) built from the aux record
// (m, density, pressure, pid) for the stand-alone (API) modes
template <int MODE>
__device__ __forceinline__ float4 make_C_from_aux(const float4 aux) {
    float4 c;
    c.x = (MODE == GM_PRESSURE) ? aux.z / (aux.y * aux.y) : 0.0f;  // WCSPH.py:54
    c.y = (MODE == GM_NONPRESSURE) ? aux.x / aux.y : 0.0f;         // WCSPH.py:112
    c.z = aux.x;
    c.w = aux.y;
    return c;
}

// E = the target's own aux (stand-alone force modes) or eos (fused force) record, loaded by the caller
template <int MODE>
__device__ __forceinline__ float4 target_load_E(const DevView& d, int i) {
    // (GM_DENSITY_EOS: the aux record its finish rewrites -- requested with the target's other records, so that the
    // finish does not end every brick with a load it has to wait for; the lean finish of the uniform-fluid step
    // (write_sg) neither reads nor writes aux)
    if (MODE == GM_DENSITY_EOS) return d.write_sg ? make_float4(0.f, 0.f, 0.f, 0.f) : d.aux[i];
    if (MODE == GM_NONPRESSURE || MODE == GM_PRESSURE) return d.aux[i];
    if (MODE == GM_FORCE_FUSED_U) { const float2 e = d.eos2[i]; return make_float4(e.x, e.y, 0.f, 0.f); }  // lean record (p, rho)
    if (MODE == GM_FORCE_FUSED || mode_is_df_iter<MODE>() || mode_is_df_vdiv<MODE>() || MODE == GM_DF_NONPRESSURE)
        return d.eos[i];
    return make_float4(0.f, 0.f, 0.f, 0.f);
}

// SOLIDS = false (the pure-fluid instance of the one-gather force sweep): what only a solid neighbour's term reads stays 0
template <int MODE, bool EXACT = false, bool SOLIDS = true>
__device__ __forceinline__ void target_init(const DevView& d, Target& t, const float4 A, const float4 B, const float4 E) {
    t.x = A.x; t.y = A.y; t.z = A.z; t.mV = A.w;
    t.vx = B.x; t.vy = B.y; t.vz = B.z;
    t.flags = __float_as_int(B.w);
    t.s0 = 0.0f;
    t.ax = d.gx; t.ay = d.gy; t.az = d.gz;  // WCSPH.py:135-136 d_v = g
    t.px = t.py = t.pz = 0.0f;
    t.m = t.rho = t.p = t.dpi = t.st_c = t.dpj_solid = 0.0f;
    t.self_in_sum = false;
    if (MODE == GM_NONPRESSURE || MODE == GM_PRESSURE) {
        t.m = E.x; t.rho = E.y; t.p = E.z;
        t.dpi = E.z / (E.y * E.y);  // WCSPH.py:49
        t.st_c = d.sigma / E.x;     // WCSPH.py:100
        t.dpj_solid = E.z / (d.rho0 * d.rho0);
    }
    if (MODE == GM_FORCE_FUSED) {
        t.dpi = E.x; t.m = E.z; t.rho = E.w;
        t.p = E.x * (E.w * E.w);
        t.st_c = d.sigma / E.z;
        t.dpj_solid = t.p / (d.rho0 * d.rho0);
    }
    if (MODE == GM_FORCE_FUSED_U) {  // lean record E = (p, rho); p / rho^2 exactly as the density finish wrote it into gat
        t.p = E.x; t.rho = E.y; t.m = d.m_u;
        t.dpi = EXACT ? __fdiv_rn(E.x, E.y * E.y) : E.x * __builtin_amdgcn_rcpf(E.y * E.y);
        t.st_c = (d.sigma / d.m_u) * d.m_u;  // (sigma / m_i) * m_j with the common mass (WCSPH.py:100)
        if (SOLIDS) t.dpj_solid = t.p / (d.rho0 * d.rho0);
    }
    if (MODE == GM_BVOL_STATIC || MODE == GM_BVOL_DYNAMIC) t.s0 = d.w_zero;  // sph_base.py:95, 110
    t.nn = 0;
    // DFSPH: E = (dfsph_factor, density_adv, m, density)
    if (MODE == GM_DF_FACTOR) t.ax = t.ay = t.az = 0.0f;  // grad_p_i (DFSPH.py:122)
    if (mode_is_df_vdiv<MODE>()) { t.rho = E.w; t.p = E.x; }  // t.p: the target's own dfsph_factor (for k_i)
    if (MODE == GM_DF_DIV_ITER || MODE == GM_DF_DIV_ITER_U) {  // DFSPH.py:292-294: b_i = density_adv, k_i = b_i * factor; dv starts at 0
        t.dpi = E.y * E.x; t.rho = E.w;
        t.ax = t.ay = t.az = 0.0f;
    }
    if (mode_is_df_pressure<MODE>()) {  // DFSPH.py:362-363: b_i = density_adv - 1; v[p_i] is updated pair by pair
        t.dpi = (E.y - 1.0f) * E.x; t.rho = E.w;
        t.ax = B.x; t.ay = B.y; t.az = B.z;
    }
    if (MODE == GM_DF_NONPRESSURE) {
        t.m = E.z; t.rho = E.w;
        t.st_c = d.sigma / E.z;  // DFSPH.py:62
    }
}

// Fast reciprocal / rsqrt (v_rsq_f32 / v_rcp_f32, ~1 ulp).  The reference's
// r.norm(), r / (r_norm * h), x / y become r2 * rsq(r2), r * (rsq * 1/h), x * rcp(y):
// same formulas, a few ulp apart, far inside the 1e-4 position budget; hipcc's
// correctly-rounded div/sqrt expansions (~10 VALU each) were the dominant cost.
// (x = 0 only for a particle paired with itself or an exact duplicate: rsq(1e-30) * 0 = 0 gives r = 0 like the
// guarded form did, with one v_max instead of a compare + select)
__device__ __forceinline__ float sph_rsq(float x) { return __builtin_amdgcn_rsqf(fmaxf(x, 1e-30f)); }
__device__ __forceinline__ float sph_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// sph_base.py:23-44 cubic_kernel as a function of q = r/h (q <= 1 is guaranteed by the caller's r < h)
__device__ __forceinline__ float sph_W_q(const DevView& d, float q) {
    const float t = 1.0f - q;
    const float inner = d.k_w * ((6.0f * q - 6.0f) * q * q + 1.0f);
    const float outer = d.k_w * 2.0f * (t * t * t);
    return q <= 0.5f ? inner : outer;
}
// sph_base.py:46-68 cubic_kernel_derivative = coef * (rx, ry, rz); coef folds grad_q = r / (|r| h)
__device__ __forceinline__ float sph_gradW_coef(const DevView& d, float q, float r_norm, float rinv) {
    const float f = 1.0f - q;
    const float c = q <= 0.5f ? d.k_dw * q * (3.0f * q - 2.0f) : d.k_dw * (-f * f);
    return r_norm > 1e-5f ? c * (rinv * d.inv_h) : 0.0f;
}

// particle_system.py:385: accept iff |x_i - x_j| < h (strict).  Every pair term vanishes continuously at r = h, so
// the ~1 ulp of the fast rsqrt is immaterial -- except where neighbours are COUNTED (DFSPH.py:172-177 switches the
// divergence source off below 20 neighbours): a rest lattice is full of pairs at exactly r = 2d = h, and there the
// decision must be the correctly rounded sqrt's (what a plain f32 evaluation of r.norm() < h gives).
template <int MODE>
__device__ __forceinline__ bool sph_within(const DevView& d, float r2, float rn) {
    bool in = rn < d.h;
    if (mode_is_df_vdiv<MODE>()) {
        const float h2 = d.h * d.h;
        if (fabsf(r2 - h2) <= 4e-6f * h2) in = __fsqrt_rn(r2) < d.h;
    }
    return in;
}

// Two-way coupling (WCSPH.py:66-68, DFSPH.py:313, 389-390): the reaction on a dynamic rigid particle is collected
// from many fluid lanes of many workgroups.  f32 atomic adds would make the sum depend on the order the hardware
// happens to serve them in; here every contribution is rounded once to 2^-32 fixed point and added as a 64-bit
// integer -- associative, hence bit-reproducible -- and k_fold_coupling adds the total to the particle's
// acceleration after the sweep (range +-2^31 m/s^2, resolution 2.3e-10: far below an f32 ulp of any acceleration
// that matters).
__device__ __forceinline__ void couple_scatter(const DevView& d, int gj, float fx, float fy, float fz) {
    unsigned long long* a = reinterpret_cast<unsigned long long*>(d.acc_fx) + 3 * (size_t)gj;
    atomicAdd(a + 0, (unsigned long long)__float2ll_rn(fx * 4294967296.0f));
    atomicAdd(a + 1, (unsigned long long)__float2ll_rn(fy * 4294967296.0f));
    atomicAdd(a + 2, (unsigned long long)__float2ll_rn(fz * 4294967296.0f));
}

// One accepted pair (i != j, r_norm = |x_i - x_j| < h).  gj = global (sorted)
// index of j, needed only for the coupling scatter.
template <int MODE>
__device__ __forceinline__ void pair_physics(const DevView& d, Target& t, float rx, float ry, float rz, float r2,
                                             float r_norm, float rinv, const float4 A, const float4 B,
                                             const float4 Cc, int gj) {
    const float q = r_norm * d.inv_h;
    if (MODE == GM_DENSITY || MODE == GM_DENSITY_EOS || MODE == GM_DF_DENSITY) {
        // WCSPH.py:19-30 (= DFSPH.py:22-34): fluid and solid neighbours add m_V_j * W identically
        t.s0 += A.w * sph_W_q(d, q);
        return;
    }
    const int fj = __float_as_int(B.w);  // (GM_FORCE_FUSED_U: B.w is not the flag word, fj unused)
    if (MODE == GM_BVOL_STATIC || MODE == GM_BVOL_DYNAMIC) {
        if (sph_flags_material(fj) == SPH_MATERIAL_SOLID) t.s0 += sph_W_q(d, q);  // sph_base.py:100-103
        return;
    }
    const bool j_fluid = sph_is_fluid(fj);
    const float gc = sph_gradW_coef(d, q, r_norm, rinv);
    if (MODE == GM_FORCE_FUSED_U) {
        // A = (x_j, U_j), B = (v_j, p_j/rho_j^2) for a fluid neighbour (U = m_j/rho_raw_j > 0; m_j = m_u, m_V_j = m_V0);
        // for a solid one U = -m_V_j and B.w = 1 if it is dynamic.  Same formulas as GM_FORCE_FUSED below.
        if (A.w > 0.0f) {
            const float w = (r2 > d.d2) ? sph_W_q(d, q) : d.w_d;
            const float c = t.st_c * w;                                           // WCSPH.py:93-102
            const float v_xy = (t.vx - B.x) * rx + (t.vy - B.y) * ry + (t.vz - B.z) * rz;
            const float cv = d.visc_d_nu * A.w * v_xy * sph_rcp(r2 + d.visc_eps) * gc;  // WCSPH.py:105-116
            const float k = cv - c;
            t.ax += k * rx; t.ay += k * ry; t.az += k * rz;
            const float cp = -d.rho0 * d.m_V0 * (t.dpi + B.w) * gc;                // WCSPH.py:51-57
            t.px += cp * rx; t.py += cp * ry; t.pz += cp * rz;
        } else {
            const float cp = -d.rho0 * (-A.w) * (t.dpi + t.dpj_solid) * gc;        // WCSPH.py:58-68
            const float fx = cp * rx, fy = cp * ry, fz = cp * rz;
            t.px += fx; t.py += fy; t.pz += fz;
            if (B.w != 0.0f) {
                const float sc = d.rho0 * sph_rcp(d.aux[gj].y);  // density[p_j] of the body particle
                couple_scatter(d, gj, -fx * sc, -fy * sc, -fz * sc);
            }
        }
        return;
    }
    // ---- DFSPH: grad_p_j = -m_V_j gradW(x_i - x_j) = -(c rx, c ry, c rz) with c = m_V_j * gc ----
    if (MODE == GM_DF_FACTOR) {
        const float c = A.w * gc;
        if (j_fluid) t.s0 += (c * c) * r2;           // DFSPH.py:145 sum_grad_p_k (fluid neighbours only)
        t.ax += c * rx; t.ay += c * ry; t.az += c * rz;  // DFSPH.py:146-153 grad_p_i -= grad_p_j (both materials)
        return;
    }
    if (mode_is_df_vdiv<MODE>()) {
        // DFSPH.py:183-197 / :212-221: m_V_j (v_i - v_j) . gradW, fluid and boundary neighbours alike
        t.s0 += A.w * (gc * ((t.vx - B.x) * rx + (t.vy - B.y) * ry + (t.vz - B.z) * rz));
        t.nn += 1;
        return;
    }
    if (mode_is_df_iter_u<MODE>()) {
        // A.w = +m_V_j (fluid) / -m_V_j (solid); Cc.x = k_j = b_j * factor_j.  Formulas of the general sweep below.
        const float mV = fabsf(A.w);
        if (A.w > 0.0f) {
            const float k_sum = t.dpi + Cc.x;
            if (fabsf(k_sum) > d.m_eps) {
                const float c = (d.dt * k_sum) * (mV * gc);
                t.ax += c * rx; t.ay += c * ry; t.az += c * rz;
            }
        } else if (fabsf(t.dpi) > d.m_eps) {
            const float c = (d.dt * t.dpi) * (mV * gc);
            const float fx = c * rx, fy = c * ry, fz = c * rz;
            t.ax += fx; t.ay += fy; t.az += fz;
            if (sph_is_dynamic_rigid(__float_as_int(d.vf[gj].w))) {  // solid neighbours are few: fetched only here
                const float sc = t.rho * sph_rcp(d.eos[gj].w) * sph_rcp(d.dt);
                couple_scatter(d, gj, -fx * sc, -fy * sc, -fz * sc);
            }
        }
        return;
    }
    if (mode_is_df_iter<MODE>()) {
        const float off = (MODE == GM_DF_PRESSURE_ITER) ? 1.0f : 0.0f;
        if (j_fluid) {
            const float k_sum = t.dpi + (Cc.y - off) * Cc.x;  // DFSPH.py:299-301 / :370-372
            if (fabsf(k_sum) > d.m_eps) {
                const float c = (d.dt * k_sum) * (A.w * gc);  // dv -= dt k_sum grad_p_j
                t.ax += c * rx; t.ay += c * ry; t.az += c * rz;
            }
        } else if (fabsf(t.dpi) > d.m_eps) {  // DFSPH.py:305-312 / :380-388 (Akinci boundary)
            const float c = (d.dt * t.dpi) * (A.w * gc);  // vel_change = -dt k_i grad_p_j
            const float fx = c * rx, fy = c * ry, fz = c * rz;
            t.ax += fx; t.ay += fy; t.az += fz;
            if (sph_is_dynamic_rigid(fj)) {  // DFSPH.py:313 / :389-390: -vel_change / dt * rho_i / rho_j
                const float sc = t.rho * sph_rcp(Cc.w) * sph_rcp(d.dt);
                couple_scatter(d, gj, -fx * sc, -fy * sc, -fz * sc);
            }
        }
        return;
    }
    if (MODE == GM_DF_NONPRESSURE) {
        if (j_fluid) {  // DFSPH.py:53-83, the formulas of WCSPH.py:93-116; solid neighbours carry boundary_viscosity = 0
            const float w = (r2 > d.d2) ? sph_W_q(d, q) : d.w_d;
            const float c = t.st_c * Cc.z * w;
            const float v_xy = (t.vx - B.x) * rx + (t.vy - B.y) * ry + (t.vz - B.z) * rz;
            const float cv = d.visc_d_nu * (Cc.z * sph_rcp(Cc.w)) * v_xy * sph_rcp(r2 + d.visc_eps) * gc;
            const float k = cv - c;
            t.ax += k * rx; t.ay += k * ry; t.az += k * rz;
        }
        return;
    }
    if (MODE == GM_NONPRESSURE || MODE == GM_FORCE_FUSED) {
        if (j_fluid) {
            // surface tension  WCSPH.py:93-102
            const float w = (r2 > d.d2) ? sph_W_q(d, q) : d.w_d;
            const float c = t.st_c * Cc.z * w;
            // viscosity  WCSPH.py:105-116
            const float v_xy = (t.vx - B.x) * rx + (t.vy - B.y) * ry + (t.vz - B.z) * rz;
            const float cv = d.visc_d_nu * Cc.y * v_xy * sph_rcp(r2 + d.visc_eps) * gc;
            const float k = cv - c;
            t.ax += k * rx; t.ay += k * ry; t.az += k * rz;
        }
        // solid neighbour: boundary_viscosity = 0.0 => contributes exactly 0 (WCSPH.py:117-125)
    }
    if (MODE == GM_PRESSURE || MODE == GM_FORCE_FUSED) {
        if (j_fluid) {
            // WCSPH.py:51-57
            const float c = -d.rho0 * A.w * (t.dpi + Cc.x) * gc;
            t.px += c * rx; t.py += c * ry; t.pz += c * rz;
        } else if (sph_flags_material(fj) == SPH_MATERIAL_SOLID) {
            // WCSPH.py:58-68 (Akinci 2012 boundary pressure + two-way coupling)
            const float c = -d.rho0 * A.w * (t.dpi + t.dpj_solid) * gc;
            const float fx = c * rx, fy = c * ry, fz = c * rz;
            t.px += fx; t.py += fy; t.pz += fz;
            if (sph_is_dynamic_rigid(fj)) {
                const float sc = d.rho0 * sph_rcp(Cc.w);
                couple_scatter(d, gj, -fx * sc, -fy * sc, -fz * sc);
            }
        }
    }
}

// GM_FORCE_FUSED_U pair term, branch-free for a fluid neighbour (SPH_VAR_FORCE_BF): the formulas of pair_physics above
// with (1 - q) clamped at 0, so W, grad W and with them every contribution vanish from r = h on exactly as if the pair
// had been rejected (particle_system.py:385), and the self pair (r = 0) multiplies finite coefficients by r = 0.  Only a
// solid neighbour still needs the accept test (its reaction is scattered with atomics).
// a uniform value held in a VGPR: on gfx950 a VALU instruction with an SGPR source issues at half rate
// (profiles/archive/r02b_ubench_valu_table2.txt: v_fma_f32 with one SGPR operand 4.4 cycles, all-VGPR 2.6)
__device__ __forceinline__ float sph_in_vgpr(float x) { float r; asm("v_mov_b32 %0, %1" : "=v"(r) : "v"(x)); return r; }
__device__ __forceinline__ unsigned sph_in_vgpr(unsigned x) { unsigned r; asm("v_mov_b32 %0, %1" : "=v"(r) : "v"(x)); return r; }
// The constants of the pair term sit in VGPRs (sph_in_vgpr below).
struct ForceK { float inv_h, kg, kw2, kw8, d2, w_d, visc, veps, cpk; };
__device__ __forceinline__ ForceK force_k(const DevView& d) {
    ForceK K;
    K.inv_h = d.inv_h; K.kg = d.k_dw * d.inv_h;
    K.kw2 = d.k_w * 2.0f; K.kw8 = d.k_w * 8.0f;
    K.d2 = d.d2; K.w_d = d.w_d;
    K.visc = d.visc_d_nu; K.veps = d.visc_eps;
    K.cpk = -d.rho0 * d.m_V0;
    return K;
}
// PURE (SPH_VAR_PURE_INTERNAL: the context holds no solid particle at all, see sph_pure_fluid_instances): every neighbour is a
// fluid particle, so the fluid term stands alone -- no compare on A.w with its exec-mask save / restore / branch, no solid body
// (accept test, dependent aux load, 64-bit atomics), and gj / not_self, which only that body read, are dead.  The fluid term is
// the SAME expression tree on the same operand values: results are bit-identical to the general instance.
template <bool PURE = false>
__device__ __forceinline__ void pair_force_u_bf(const DevView& d, const ForceK& K, Target& t, float rx, float ry, float rz, float r2,
                                                const float4 A, const float4 B, int gj, bool not_self) {
    const float rinv = __builtin_amdgcn_rsqf(r2 + 1e-30f);
    const float rn = r2 * rinv;
    // sph_base.py:23-68 without branches: with t = (1-q)+ and u = (1/2-q)+,  W = k (2 t^3 - 8 u^3)  and
    // dW/dq = 6k (4 u^2 - t^2)  reproduce both pieces of the cubic spline and vanish from q = 1 on.
    const float f = fminf(fmaxf(fmaf(-K.inv_h, rn, 1.0f), 0.0f), 1.0f);
    const float u = fminf(fmaxf(fmaf(-K.inv_h, rn, 0.5f), 0.0f), 1.0f);
    const float f2 = f * f, u2 = u * u;
    const float cg = K.kg * (4.0f * u2 - f2);   // (k_dw / h) (4 u^2 - t^2)
    const float gc = rn > 1e-5f ? cg * rinv : 0.0f;
    if (PURE || A.w > 0.0f) {
        const float wq = K.kw2 * (f2 * f) - K.kw8 * (u2 * u);
        const float w = (r2 > K.d2) ? wq : K.w_d;
        const float c = t.st_c * w;                                               // WCSPH.py:93-102
        const float v_xy = (t.vx - B.x) * rx + (t.vy - B.y) * ry + (t.vz - B.z) * rz;
        const float cv = K.visc * A.w * v_xy * sph_rcp(r2 + K.veps) * gc;          // WCSPH.py:105-116
        const float k = cv - c;
        t.ax += k * rx; t.ay += k * ry; t.az += k * rz;
        const float cp = K.cpk * (t.dpi + B.w) * gc;                               // WCSPH.py:51-57
        t.px += cp * rx; t.py += cp * ry; t.pz += cp * rz;
    } else if (rn < d.h && not_self) {
        const float cp = -d.rho0 * (-A.w) * (t.dpi + t.dpj_solid) * gc;            // WCSPH.py:58-68
        const float fx = cp * rx, fy = cp * ry, fz = cp * rz;
        t.px += fx; t.py += fy; t.pz += fz;
        if (B.w != 0.0f) {
            const float sc = d.rho0 * sph_rcp(d.aux[gj].y);  // density[p_j] of the body particle
            couple_scatter(d, gj, -fx * sc, -fy * sc, -fz * sc);
        }
    }
}

// ---- SPH_OPT_EXACT_MATH: the A/B instance of the fast-math choice (never the default) ----
// The same pair terms written the way the reference's f32 expressions evaluate on an IEEE machine (which is also how the
// CPU restatement the tests compare with evaluates them): r.norm() by the correctly rounded sqrt, q = r_norm / h, grad_q = r / (r_norm h),
// x / y by the IEEE divide, the cubic spline in its two-branch form, no contraction into FMAs.  If the errors the fast
// forms show after an impact (VERDICT r03 "weak" #1: C2 velocity 4e-3 at step 300) are rounding, they collapse with this
// instance; profiles/r04_parity_fastmath_ab.json holds both.
__device__ __forceinline__ float sph_W_exact(const DevView& d, float r_norm) {
#pragma clang fp contract(off)
    const float q = __fdiv_rn(r_norm, d.h);
    float res = 0.0f;
    if (q <= 1.0f) {
        if (q <= 0.5f) {
            const float q2 = q * q, q3 = q2 * q;
            res = d.k_w * (6.0f * q3 - 6.0f * q2 + 1.0f);  // sph_base.py:41
        } else {
            const float f = 1.0f - q;
            res = d.k_w * 2.0f * (f * f * f);               // sph_base.py:43 ti.pow(1 - q, 3.0)
        }
    }
    return res;
}
__device__ __forceinline__ void pair_force_u_exact(const DevView& d, Target& t, float rx, float ry, float rz, float r2,
                                                   const float4 A, const float4 B, int gj, bool not_self) {
#pragma clang fp contract(off)
    const float rn = __fsqrt_rn(r2);
    if (!(rn < d.h) || !not_self) return;  // particle_system.py:385
    const float q = __fdiv_rn(rn, d.h);
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;  // sph_base.py:46-68
    if (rn > 1e-5f && q <= 1.0f) {
        const float inv = rn * d.h;
        const float f = 1.0f - q;
        const float c = q <= 0.5f ? d.k_dw * q * (3.0f * q - 2.0f) : d.k_dw * (-f * f);
        gx = c * __fdiv_rn(rx, inv); gy = c * __fdiv_rn(ry, inv); gz = c * __fdiv_rn(rz, inv);
    }
    if (A.w > 0.0f) {  // fluid neighbour: A.w = m_j / rho_j, B = (v_j, p_j / rho_j^2)
        const float w = (r2 > d.d2) ? sph_W_exact(d, rn) : d.w_d;
        t.ax -= t.st_c * rx * w; t.ay -= t.st_c * ry * w; t.az -= t.st_c * rz * w;            // WCSPH.py:93-102
        const float v_xy = (t.vx - B.x) * rx + (t.vy - B.y) * ry + (t.vz - B.z) * rz;
        const float cv = __fdiv_rn(d.visc_d_nu * A.w * v_xy, rn * rn + d.visc_eps);             // WCSPH.py:105-116
        t.ax += cv * gx; t.ay += cv * gy; t.az += cv * gz;
        const float cp = -d.rho0 * d.m_V0 * (t.dpi + B.w);                                      // WCSPH.py:51-57
        t.px += cp * gx; t.py += cp * gy; t.pz += cp * gz;
    } else {           // solid neighbour: A.w = -m_V_j, B.w = 1 if dynamic
        const float cp = -d.rho0 * (-A.w) * (t.dpi + t.dpj_solid);                              // WCSPH.py:58-68
        const float fx = cp * gx, fy = cp * gy, fz = cp * gz;
        t.px += fx; t.py += fy; t.pz += fz;
        if (B.w != 0.0f) {
            const float sc = __fdiv_rn(d.rho0, d.aux[gj].y);
            couple_scatter(d, gj, -fx * sc, -fy * sc, -fz * sc);
        }
    }
}

// write-back of one particle (target or not) for the given mode
template <int MODE, bool EXACT = false>
__device__ __forceinline__ void target_finish(const DevView& d, Target& t, int i, bool gathered, const float4 E = make_float4(0.f, 0.f, 0.f, 0.f)) {
    if (MODE == GM_BVOL_STATIC || MODE == GM_BVOL_DYNAMIC) {
        // sph_base.py:98, 113: m_V = 1/delta * 3.0   (only .w is written; .xyz are read concurrently)
        if (gathered) reinterpret_cast<float*>(&d.xm[i])[3] = 1.0f / t.s0 * 3.0f;
        return;
    }
    if (MODE == GM_DENSITY) {
        // WCSPH.py:39-43
        if (gathered) reinterpret_cast<float*>(&d.aux[i])[1] = (t.self_in_sum ? t.s0 : t.mV * d.w_zero + t.s0) * d.rho0;
        return;
    }
    if (MODE == GM_DENSITY_EOS) {
        float rho_raw = 0.0f, rho = 0.0f, p = 0.0f;
        if (gathered) {
            rho_raw = (t.self_in_sum ? t.s0 : t.mV * d.w_zero + t.s0) * d.rho0;  // WCSPH.py:39-43
            if (SPH_ABL(d, 1 | 16 | 32)) rho_raw = d.rho0;  // profiling runs that skip pair terms: keep the state finite
            rho = fmaxf(rho_raw, d.rho0);                 // WCSPH.py:75
            // WCSPH.py:76 ti.pow(rho / rho0, exponent): integer exponents by multiplication (sph_tait_pow); the ratio is
            // the IEEE quotient (once per particle; its error is amplified by stiffness * exponent), the later
            // divisions are reciprocals.  Exactly 0 at rho = rho0, where most of a resting fluid sits after the clamp.
            const float xr = rho / d.rho0;
            p = d.stiffness * (sph_tait_pow<true>(d, xr) - 1.0f);
        } else {
            // WCSPH.py:131-137 for non-fluid particles: static a = 0, dynamic rigid a = g
            const bool st = sph_is_static_rigid(t.flags);
            d.acc[i] = st ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(d.gx, d.gy, d.gz, 0.f);
        }
        if (d.write_sg) {
            // Uniform-fluid step (every fluid particle has mass m_u and m_V0; positions do not change before the force
            // sweep runs): what that sweep needs of a NEIGHBOUR goes to stg (staged in LDS) and gat (gathered), what it
            // needs of the TARGET besides those to the 8-byte record (p, rho).  aux is neither read nor written here:
            // density and pressure are folded into it from eos2 when somebody asks (sph_ensure_aux).
            const bool fl = sph_is_fluid(t.flags);
            if (gathered) d.eos2[i] = make_float2(p, rho);
            const float u_i = EXACT ? __fdiv_rn(d.m_u, rho_raw) : d.m_u * sph_rcp(rho_raw);      // m / rho  (WCSPH.py:112)
            const float dp_i = EXACT ? __fdiv_rn(p, rho * rho) : p * sph_rcp(rho * rho);        // p / rho^2 (WCSPH.py:49)
            d.stg[i] = make_float4(t.x, t.y, t.z, fl ? u_i : -t.mV);
            d.gat[i] = make_float4(t.vx, t.vy, t.vz, fl ? dp_i : (sph_is_dynamic_rigid(t.flags) ? 1.0f : 0.0f));
            return;
        }
        float4 aux = E;  // = d.aux[i], loaded by the caller (target_load_E)
        float4 e;
        if (gathered) {
            e = make_float4(p * sph_rcp(rho * rho), aux.x * sph_rcp(rho_raw), aux.x, rho);
            aux.y = rho; aux.z = p;
            d.aux[i] = aux;
        } else {
            e = make_float4(0.0f, 0.0f, aux.x, aux.y);
        }
        d.eos[i] = e;
        return;
    }
    if (MODE == GM_NONPRESSURE || MODE == GM_DF_NONPRESSURE) {
        // WCSPH.py:130-140 / DFSPH.py:100-112
        if (sph_is_static_rigid(t.flags)) d.acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        else d.acc[i] = make_float4(t.ax, t.ay, t.az, 0.f);
        return;
    }
    if (MODE == GM_DF_DENSITY) {  // DFSPH.py:42-47; eos = (factor, density_adv, m, density)
        float4 aux = d.aux[i];
        if (gathered) {
            aux.y = (t.self_in_sum ? t.s0 : t.mV * d.w_zero + t.s0) * d.rho0;
            reinterpret_cast<float*>(&d.aux[i])[1] = aux.y;
        }
        float* e = reinterpret_cast<float*>(&d.eos[i]);  // .x/.y (factor, density_adv) live until they are recomputed
        e[2] = aux.x; e[3] = aux.y;
        if (d.write_sg) d.stg[i] = make_float4(t.x, t.y, t.z, sph_is_fluid(t.flags) ? t.mV : -t.mV);
        return;
    }
    if (MODE == GM_DF_FACTOR) {  // DFSPH.py:128-139
        if (gathered) {
            const float sum_grad_p_k = t.s0 + (t.ax * t.ax + t.ay * t.ay + t.az * t.az);
            reinterpret_cast<float*>(&d.eos[i])[0] = sum_grad_p_k > 1e-6f ? -1.0f / sum_grad_p_k : 0.0f;
        }
        return;
    }
    if (MODE == GM_DF_DENSITY_CHANGE) {  // DFSPH.py:165-180
        t.df_err = 0.0f;
        if (gathered) {
            float adv = fmaxf(t.s0, 0.0f);
            if (t.nn < 20) adv = 0.0f;
            reinterpret_cast<float*>(&d.eos[i])[1] = adv;
            if (d.write_k) d.kbuf[i] = adv * t.p;  // k_i = b_i * factor_i (DFSPH.py:292-294), for the neighbours
            t.df_err = fmaf(d.rho0, adv, -0.0f);    // the term k_df_density_error_gated computes from eos.y (offset 0: divergence solve)
        }
        return;
    }
    if (MODE == GM_DF_DENSITY_ADV) {  // DFSPH.py:206-209
        t.df_err = 0.0f;
        if (gathered) {
            const float adv = fmaxf(t.rho / d.rho0 + d.dt * t.s0, 1.0f);
            reinterpret_cast<float*>(&d.eos[i])[1] = adv;
            if (d.write_k) d.kbuf[i] = (adv - 1.0f) * t.p;  // DFSPH.py:362-363
            t.df_err = fmaf(d.rho0, adv, -d.rho0);  // ... with the pressure solve's offset density_0 (DFSPH.py:346)
        }
        return;
    }
    if (mode_is_df_iter<MODE>()) {  // DFSPH.py:296 v += dv  /  :378, :387 v updated in place (t.a started at v)
        if (gathered) {
            float* v = reinterpret_cast<float*>(&d.vf[i]);  // .w (flags) is read concurrently by other lanes
            if (!mode_is_df_pressure<MODE>()) { v[0] = t.vx + t.ax; v[1] = t.vy + t.ay; v[2] = t.vz + t.az; }
            else { v[0] = t.ax; v[1] = t.ay; v[2] = t.az; }
        }
        return;
    }
    if (MODE == GM_PRESSURE) {
        // WCSPH.py:77-85
        if (sph_is_static_rigid(t.flags)) d.acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        else if (gathered) {
            float4 a = d.acc[i];
            a.x += t.px; a.y += t.py; a.z += t.pz;
            d.acc[i] = a;
        }
        return;
    }
    if (MODE == GM_FORCE_FUSED || MODE == GM_FORCE_FUSED_U) {
        // fluid: a = (g + non-pressure) + pressure  (WCSPH.py:140 then :85)
        if (gathered) {
            const float4 a = make_float4(t.ax + t.px, t.ay + t.py, t.az + t.pz, 0.f);
            if (MODE != GM_FORCE_FUSED_U || d.store_acc) d.acc[i] = a;
            if (MODE == GM_FORCE_FUSED_U && d.fuse_advect) {  // advect (WCSPH.py:143-149) + fluid walls, see step_sweeps
                float4 xm = make_float4(t.x, t.y, t.z, t.mV);
                float4 vf = make_float4(t.vx, t.vy, t.vz, __int_as_float(t.flags));
                const float hi[3] = {d.whx, d.why, d.whz};
                advect_one<true>(d, hi, xm, vf, a);
                d.xm[i] = xm;
                d.vf[i] = vf;
            }
        }
        return;
    }
}

template <int MODE>
__device__ __forceinline__ float4 load_C_global(const DevView& d, int j) {
    if (MODE == GM_FORCE_FUSED || mode_is_df_iter<MODE>() || MODE == GM_DF_NONPRESSURE) return d.eos[j];
    if (MODE == GM_NONPRESSURE || MODE == GM_PRESSURE) return make_C_from_aux<MODE>(d.aux[j]);
    return make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---------------------------------------------------------------------------
// v0: per-target cell walk through global memory (reference traversal order)
// ---------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ void gather_walk_global(const DevView& d, Target& t, int i) {
    const int c = d.key[i];
    const int cz = c % d.nz;
    const int cy = (c / d.nz) % d.ny;
    const int cx = c / (d.nz * d.ny);
    const int zlo = cz > 0 ? cz - 1 : 0;
    const int zhi = cz < d.nz - 1 ? cz + 1 : d.nz - 1;
    for (int dx = -1; dx <= 1; ++dx) {
        const int nx = cx + dx;
        if (nx < 0 || nx >= d.nx) continue;
        for (int dy = -1; dy <= 1; ++dy) {
            const int ny = cy + dy;
            if (ny < 0 || ny >= d.ny) continue;
            const int flo = sph_flatten(d, nx, ny, zlo);
            const int fhi = sph_flatten(d, nx, ny, zhi);
            const int beg = d.cell_end[flo > 0 ? flo - 1 : 0];  // particle_system.py:384 max(0, idx-1)
            const int end = d.cell_end[fhi];
            for (int j = beg; j < end; ++j) {
                if (j == i) continue;
                // (the one-gather force sweep never reads another particle's xm / vf: its finish may overwrite them)
                const float4 A = (MODE == GM_FORCE_FUSED_U ? d.stg : d.xm)[j];
                const float rx = t.x - A.x, ry = t.y - A.y, rz = t.z - A.z;
                const float r2 = rx * rx + ry * ry + rz * rz;
                const float rinv = sph_rsq(r2);
                const float rn = r2 * rinv;
                if (sph_within<MODE>(d, r2, rn)) {  // particle_system.py:385
                    float4 B = make_float4(0.f, 0.f, 0.f, 0.f), Cc = B;
                    if (mode_needs_B<MODE>()) B = (MODE == GM_FORCE_FUSED_U ? d.gat : d.vf)[j];
                    if (mode_needs_C<MODE>()) Cc = load_C_global<MODE>(d, j);
                    pair_physics<MODE>(d, t, rx, ry, rz, r2, rn, rinv, A, B, Cc, j);
                }
            }
        }
    }
}

// list == nullptr: all particles [0,N); else the n entries of list
template <int MODE>
__global__ __launch_bounds__(TPB) void k_gather_simple(DevView d, const int* __restrict__ list, int n) {
    if (mode_is_df_gated<MODE>() && d.gate && *d.gate == d.gate_epoch) return;  // a solver iteration enqueued past convergence
    const int tix = blockIdx.x * TPB + threadIdx.x;
    if (tix >= n) return;
    const int i = list ? list[tix] : tix;
    Target t;
    const float4 A = d.xm[i];
    const float4 B = d.vf[i];
    const float4 E = target_load_E<MODE>(d, i);
    target_init<MODE>(d, t, A, B, E);
    const bool g = target_gathers<MODE>(t.flags);
    if (g) gather_walk_global<MODE>(d, t, i);
    target_finish<MODE>(d, t, i, g, E);
}

// Boundary volume of a short target list (the dynamic rigid particles, every step): one target per 16 lanes, lane r
// walks column r of the 3x3 (x,y) neighbourhood, the partial sums meet through wave shuffles.  9x the parallelism
// of k_gather_simple for a sweep that is pure latency (a few 10^4 targets on 256 CUs).
template <int MODE>
__global__ __launch_bounds__(TPB) void k_gather_bvol_split(DevView d, const int* __restrict__ list, int n) {
    static_assert(MODE == GM_BVOL_STATIC || MODE == GM_BVOL_DYNAMIC, "scalar accumulator only");
    const int tix = (blockIdx.x * TPB + threadIdx.x) >> 4, r = threadIdx.x & 15;
    const bool live = tix < n;
    const int i = live ? list[tix] : 0;
    const float4 A = d.xm[i];
    const int fl = __float_as_int(d.vf[i].w);
    const int c = d.key[i];
    const int cz = c % d.nz, cy = (c / d.nz) % d.ny, cx = c / (d.nz * d.ny);
    // slab rank: the outermost ghost layer has no neighbours beyond it; its volumes arrive with the owner's records
    const bool g = live && target_gathers<MODE>(fl) && !(d.drop_outside && (cx < 1 || cx >= d.nx - 1));
    float sum = 0.0f;
    if (g && r < 9) {
        const int nx = cx + r / 3 - 1, ny = cy + r % 3 - 1;
        if (nx >= 0 && nx < d.nx && ny >= 0 && ny < d.ny) {
            const int zlo = cz > 0 ? cz - 1 : 0, zhi = cz < d.nz - 1 ? cz + 1 : d.nz - 1;
            const int flo = sph_flatten(d, nx, ny, zlo), fhi = sph_flatten(d, nx, ny, zhi);
            const int beg = d.cell_end[flo > 0 ? flo - 1 : 0], end = d.cell_end[fhi];  // particle_system.py:384
            // four candidates per trip, their eight loads in flight together: this sweep is pure latency (a few 10^4 targets
            // on 256 CUs), and one candidate per trip made every pair wait for its own two loads (18 us per step at C3, r04h)
            for (int j0 = beg; j0 < end; j0 += 4) {
                float4 Aj[4];
                int fj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = min(j0 + u, end - 1);
                    Aj[u] = d.xm[j];
                    fj[u] = __float_as_int(reinterpret_cast<const float*>(&d.vf[j])[3]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u;
                    if (j >= end || j == i) continue;
                    const float rx = A.x - Aj[u].x, ry = A.y - Aj[u].y, rz = A.z - Aj[u].z;
                    const float r2 = rx * rx + ry * ry + rz * rz;
                    const float rn = r2 * sph_rsq(r2);
                    if (rn < d.h && sph_flags_material(fj[u]) == SPH_MATERIAL_SOLID)
                        sum += sph_W_q(d, rn * d.inv_h);  // sph_base.py:100-103
                }
            }
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (g && r == 0) reinterpret_cast<float*>(&d.xm[i])[3] = 1.0f / (d.w_zero + sum) * 3.0f;  // sph_base.py:110-113
}

// ---------------------------------------------------------------------------
// v1: LDS-staged cell bricks
// ---------------------------------------------------------------------------
// LDS holds one float4 per shell record (see the carve in BrickCfg): for a
// filtering sweep (-2x', -2y', -2z', |x'|^2) in shell-local coordinates plus a
// separate m_V array, for a list-reading sweep the record (x, y, z, m_V) itself (the one-gather sweeps
// GM_FORCE_FUSED_U / GM_DF_*_ITER_U stage the `stg` record instead, whose 4th word also tells fluid from solid).
// List entries are u16: (shell column << 11) | LDS slot, so CAP <= 2048 and
// NCOL <= 32; the global index of a slot is slot + sColG[col] (sColG = global start - LDS start of the column).
// In the fused step the density sweep writes each target's list to HBM
// (glist, gcnt[i]) and the force sweep -- same positions, same brick layout -- reads it back instead of filtering again.
// Entry r of particle i sits at byte (r >> 2) << lshift | i * 8 | (r & 3) * 2 (2^lshift >= cap * 8, sph_api.hip): four
// consecutive entries are one 8-byte word, which the readers fetch with one load per four pairs.  All offsets are 32-bit.
// The emission loop advances its offset once per hit with a SATURATING add (a target can have as many hits as the tile
// has records; groups beyond the allocation are dropped by the buffer's range check, and an offset stuck at 2^32 - 1
// stays out of range); the readers clamp the group index to the lane's last group, so every entry they fetch was written.
#define SPH_BRICK_MAX_NZ 800  // k_brick_list (and the scatter kernel that hosts it) keeps five per-layer arrays per column group in LDS: 80 (nz + 1) bytes must stay inside the 64 KB a kernel gets without an opt-in; taller grids take the cell walk
#define SPH_CNT_WALK 255  // gcnt sentinel: this target must take the exact global cell walk (its brick's shell overflowed the LDS tile)
#define SPH_CNT_LIST_OVF 254  // same consequence, other cause: the target's own list outgrew LISTCAP
#define SPH_VAR_EXACT 32      // internal template bit (not part of SPH_OPT_KERNEL_VARIANT): the SPH_OPT_EXACT_MATH instances

template <int MODE>
__host__ __device__ constexpr bool mode_writes_list() { return MODE == GM_DENSITY_EOS || MODE == GM_DF_DENSITY; }
template <int MODE>
__host__ __device__ constexpr bool mode_reads_list() { return MODE == GM_FORCE_FUSED || MODE >= GM_DF_FACTOR; }
// sweeps whose pair term needs only (r, m_V_j): evaluated inside the filter's emission loop
template <int MODE>
__host__ __device__ constexpr bool mode_inline_physics() {
    return MODE == GM_DENSITY || MODE == GM_DENSITY_EOS || MODE == GM_DF_DENSITY;
}

template <int BX_, int BY_, int BZ_, int CAP_, int LISTCAP_>
struct BrickCfg {
    static constexpr int BX = BX_, BY = BY_, BZ = BZ_, CAP = CAP_, LISTCAP = LISTCAP_;
    static constexpr int NCOL = (BX + 2) * (BY + 2);
    static constexpr int NCELL = BX * BY * BZ;  // target cells of a brick
    static constexpr int NZS = BZ + 3;  // cell-end entries per column (start + BZ+2 ends)
    static constexpr int PER = (CAP + TPB - 1) / TPB;  // staged records per lane
    // LDS carve (bytes, every offset a multiple of 16).  Filtering sweeps stage float4 (-2x', -2y', -2z', |x'|^2)
    // + a separate m_V array (20 B per record); the list-reading force sweep needs no |x'|^2 and stages
    // float4 (-2x', -2y', -2z', m_V) only (16 B per record -> one more workgroup per CU).
    static constexpr int OFF_Q = 0;
    static constexpr int off_w(bool has_w) { return OFF_Q + CAP * 16; }
    static constexpr int off_ce(bool has_w) { return off_w(has_w) + (has_w ? CAP * 4 : 0); }
    static constexpr int off_colg(bool has_w) { return off_ce(has_w) + ((NCOL * NZS * 4 + 15) / 16) * 16; }
    static constexpr int off_cols(bool has_w) { return off_colg(has_w) + 64 * 4; }
    static constexpr int off_tg(bool has_w) { return off_cols(has_w) + 80 * 4; }
    static constexpr int off_toff(bool has_w) { return off_tg(has_w) + 64 * 4; }
    // [NCELL][9] u32, filtering sweeps: the nine candidate runs of a target cell (column << 11 | first LDS slot | length << 16)
    static constexpr int off_run(bool has_w) { return off_toff(has_w) + 80 * 4; }
    static constexpr int bytes(bool has_w) { return off_run(has_w) + (has_w ? NCELL * 9 * 4 : 0); }
    static_assert(NCOL <= 32, "column id must fit 5 bits of a list entry");
    static_assert(CAP <= 2048, "LDS slot must fit 11 bits of a list entry");
    static_assert(CAP % 4 == 0, "the m_V array starts on a 16-byte boundary");
    static_assert(LISTCAP < SPH_CNT_LIST_OVF && LISTCAP <= SPH_GLIST_ROWS, "gcnt is a byte; glist has SPH_GLIST_ROWS rows");
    static_assert(bytes(true) <= 40960, "filtering sweeps: at least four workgroups per CU (160 KiB LDS)");
    static_assert(bytes(false) <= 32768, "force sweep: five workgroups per CU");
};

// The bricks of one sweep.  A brick is a BX x BY footprint of (x, y) cell columns times a run of z layers whose HEIGHT
// this kernel chooses, column group by column group, from the cell histogram: as many layers (<= BZ) as keep the
// brick's targets within one round of the gather workgroup (tmax = 256 lanes) and its shell within the LDS tile
// (smax records).  A resting lattice (8 particles per cell) gives 4-layer bricks of 256 targets; once the fluid has
// settled to its rest density (10 per cell: the lattice of the scene files is 20 % under-dense, m_V0 = 0.8 d^3) a fixed
// 4-layer brick would hold 320 targets -- a second round with one wave in four busy while the tile stays allocated --
// and the cut moves to 3 layers of 240.  Empty layers are skipped; a brick is listed iff it holds a target.
// fixed_bz > 0 = the fixed partition of rounds 1-2 (bricks aligned to multiples of fixed_bz layers), kept as the A/B
// baseline (SPH_OPT_BRICK_SHAPE 1).
// One wave per column group: lane z counts layer z's targets and shell records (cell_end differences), a wave64 scan
// gives the prefixes, lane 0 walks them greedily; a workgroup (four column groups) takes ONE returning atomic per list.
// Two lists in one array: bricks with many targets from the front (count[0]), light ones -- the partly filled
// bricks along the fluid's surface and the tank walls -- from the back (count[1]).  The gather kernel starts
// the heavy ones first, so that the launch drains on short jobs instead of on whatever came last.
template <class CFG>
__global__ __launch_bounds__(TPB) void k_brick_list(DevView d, int nbx, int nby, int2* __restrict__ list,
                                                    int* __restrict__ count, int list_cap, int tmax, int smax, int fixed_bz) {
    extern __shared__ int sm_bl[];
    static_assert(CFG::BX == SPH_BRICK_BX && CFG::BY == SPH_BRICK_BY && CFG::BZ == SPH_BRICK_BZ, "one footprint: the sort's scatter kernel builds the same lists");
    BrickView bv;
    bv.nx = d.nx; bv.ny = d.ny; bv.nz = d.nz; bv.tgt_lo = d.tgt_lo; bv.tgt_hi = d.tgt_hi; bv.tgt_lo2 = d.tgt_lo2; bv.tgt_hi2 = d.tgt_hi2;
    bv.cell_end = d.cell_end;
    sph_brick_list_block<CFG::BX, CFG::BY, CFG::BZ>(bv, nbx, nby, list, count, list_cap, tmax, smax, fixed_bz, (int)blockIdx.x, sm_bl);
}

// raw buffer descriptor (gfx9 dword 3): byte offsets in a VGPR, hardware range check against `bytes`
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sph_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}

template <int MODE, int VAR>
__host__ __device__ constexpr int brick_waves_per_simd() {
    if (!mode_reads_list<MODE>()) return 4;
    if (MODE == GM_FORCE_FUSED_U && (VAR & SPH_VAR_GAT_LDS) != 0) return 3;
    if (MODE == GM_FORCE_FUSED_U && (VAR & SPH_VAR_GAT_LDS4) != 0) return 4;
    return 5;
}
// second launch bound = waves per SIMD the LDS tile allows anyway (four workgroups per CU for the filtering sweeps, five
// for the list-reading ones): the register allocator must not go past 128 / 96 VGPRs, or a resident slot is lost
template <int MODE, class CFG, int VAR = 0>
__global__ __launch_bounds__(TPB, (brick_waves_per_simd<MODE, VAR>())) void k_gather_brick(DevView d, int nby, const int2* __restrict__ brick_list,
                                                      const int* __restrict__ brick_count,
                                                      unsigned short* __restrict__ glist,
                                                      unsigned char* __restrict__ gcnt, int cap, int list_cap, int lshift,
                                                      int4* __restrict__ brec, int use_rec) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool HAS_W = !mode_reads_list<MODE>();
    constexpr bool V_GROUPS = (VAR & SPH_VAR_GROUPS) != 0 && !mode_reads_list<MODE>();
    constexpr bool V_MFMA = (VAR & SPH_VAR_MFMA) != 0 && V_GROUPS && MODE == GM_DENSITY_EOS;  // the filter on the matrix pipe
    // A context WITHOUT ANY SOLID particle (checked on the device: sphs_pure_fluid): every m_V_j is m_V0 BIT FOR BIT, so the
    // density pair term takes it from a register instead of the tile -- one LDS read per hit less, the tile's m_V array is
    // not written -- and computes exactly what it computed before (the same fma with the same operand values: results are
    // bit-identical, unlike a form that would scale the sum of W once).  Chosen by the launcher, not a user-visible bit.
    constexpr bool V_PURE = (VAR & SPH_VAR_PURE_INTERNAL) != 0 && MODE == GM_DENSITY_EOS;
    constexpr bool V_BF = (VAR & SPH_VAR_FORCE_BF) != 0 && MODE == GM_FORCE_FUSED_U;
    // ... and the counterpart in the one-gather force sweep: no neighbour is a solid, so the branch-free pair term drops the solid
    // path (pair_force_u_bf<true>) and every target is a fluid particle with m_V = m_V0.  Instruction count only: the sums are the
    // general instance's, operation for operation.  (The exact-math instance and the per-target cell walk keep their general form.)
    constexpr bool V_PUREF = (VAR & SPH_VAR_PURE_INTERNAL) != 0 && V_BF;
    constexpr bool V_DEEP = (VAR & SPH_VAR_DEEP) != 0 && mode_reads_list<MODE>();
    // SPH_VAR_GAT_LDS / _LDS4 (round 6, VERDICT r05 "next" #5): the neighbour's second record (gat: v, p / rho^2) staged in LDS beside
    // the first instead of gathered through the L1 -- the counters say the force sweep's vector-memory path is busy with TAG
    // LOOK-UPS, not misses: a wave's 16-byte gather touches ~33 cache lines (profiles/r06b_pmc_ta_*: 51 M L1 accesses for 1.57 M
    // load instructions, 87 % of them hits, address unit stalled by the cache 27-40 % of the kernel)
    constexpr bool V_GLDS = (VAR & (SPH_VAR_GAT_LDS | SPH_VAR_GAT_LDS4)) != 0 && MODE == GM_FORCE_FUSED_U;
    constexpr bool V_EXACT = (VAR & SPH_VAR_EXACT) != 0 && (MODE == GM_DENSITY_EOS || MODE == GM_FORCE_FUSED_U);  // SPH_OPT_EXACT_MATH
    constexpr bool INLINE_PHYS = mode_inline_physics<MODE>();  // pair terms inside the emission loop
    float4* sQ = reinterpret_cast<float4*>(smem + CFG::OFF_Q);
    float* sW = reinterpret_cast<float*>(smem + CFG::off_w(HAS_W));  // only when HAS_W
    float4* sG = reinterpret_cast<float4*>(smem + CFG::bytes(HAS_W));  // only when V_GLDS: the gat records of the shell, behind everything else
    // Shell origin.  Candidates are staged in shell-local coordinates as (-2x', -2y', -2z', |x'|^2) so the
    // filter is |x_i - x_j|^2 - |x_i'|^2 = s_j + x_i'.(-2 x_j') : 3 FMA + 1 compare per candidate.  Local
    // coordinates are <= 6 cells, so the cancellation error (~1e-8) is far below the 2e-4 h^2 filter margin,
    // and x' = x - O is exact (Sterbenz) away from the first cells, so phase 2 recovers x_i - x_j unchanged.
    int* sCE = reinterpret_cast<int*>(smem + CFG::off_ce(HAS_W));      // [NCOL][NZS] raw cell_end values of the shell
    int* sColG = reinterpret_cast<int*>(smem + CFG::off_colg(HAS_W));  // global - LDS start of the column segment
    int* sColS = reinterpret_cast<int*>(smem + CFG::off_cols(HAS_W));  // LDS start of the column segment (+ total at [64])
    int* sTG = reinterpret_cast<int*>(smem + CFG::off_tg(HAS_W));      // global start of the column's targets
    int* sTOff = reinterpret_cast<int*>(smem + CFG::off_toff(HAS_W));  // target-number start of the column (+ total at [64])

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // A DFSPH solver iteration enqueued past convergence leaves without touching anything (DevView::gate).  The gate word is
    // REQUESTED here and looked at behind step A's barrier: as the first thing a workgroup waits for, its scalar load cost
    // every sweep of a solve ~2 % (r05: 2.97 vs 2.91 ms per DFSPH step); under the column-table loads it costs nothing.
    unsigned gate_word = 0u;
    if (mode_is_df_gated<MODE>() && d.gate) gate_word = *d.gate;

    // One workgroup per LISTED brick (the hardware scheduler balances them).  Hardware block b runs on XCD b%8:
    // XCD x takes the x-th eighth of the list, so neighbouring bricks share that XCD's L2 and -- because the list
    // holds work, not space -- all 8 XCDs are loaded evenly however the fluid sits in the tank.  The grid is sized
    // for the worst case (every brick non-empty); surplus blocks leave here.
#ifdef SPH_PROFILE
    const bool ts_on = d.prof_ts != nullptr && (d.ablate & (mode_reads_list<MODE>() ? (1 << 29) : (1 << 28))) != 0;
    if (ts_on && threadIdx.x == 0) {
        unsigned long long* row = d.prof_ts + (size_t)blockIdx.x * 8;
        row[1] = row[2] = row[3] = row[4] = 0ull;
        row[5] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);  // XCC_ID | HW_ID
        row[6] = 0ull;
    }
    SPH_TS(0);
#endif
    const int nbh = brick_count[0], nbl = brick_count[1];
    const int chunkh = (nbh + 7) >> 3, chunkl = (nbl + 7) >> 3;
    const int xcd = (int)(blockIdx.x & 7), slot = (int)(blockIdx.x >> 3);
    int2 brick;
    int bidx;  // the brick's index in the list (= row of its column record, see step A)
    if (slot < chunkh) {  // heavy bricks first (blocks are dispatched in blockIdx order) ...
        const int kb = xcd * chunkh + slot;
        if (kb >= nbh) return;
        bidx = kb;
    } else {  // ... the light ones fill the tail
        const int kb = xcd * chunkl + (slot - chunkh);
        if (slot - chunkh >= chunkl || kb >= nbl) return;
        bidx = list_cap - 1 - kb;
    }
    // A list-READING sweep over the partition and the target ranges of the sweep that wrote the lists (use_rec) finds the
    // outcome of step A -- the four column tables -- in that sweep's per-brick record and needs nothing else of the brick:
    // one round trip (16 bytes per lane) instead of list entry -> 7 cell_end words per column -> two wave scans.  Positions do
    // not change between the density sweep and the last sweep that reads its lists (one force sweep in WCSPH, ~18 sweeps in a
    // DFSPH step), so every reader was recomputing the same tables (VERDICT r05 "next" #8).
    const bool from_rec = mode_reads_list<MODE>() && use_rec != 0;
    if (from_rec) brick = make_int2(0, 0);
    else brick = brick_list[bidx];
    {
    // (column group, first z layer | height << 16): the partition of k_brick_list
    const int byi = brick.x % nby;
    const int bxi = brick.x / nby;
    const int cx0 = bxi * CFG::BX, cy0 = byi * CFG::BY, cz0 = brick.y & 0xffff;
    const int cx1 = min(cx0 + CFG::BX, d.nx), cy1 = min(cy0 + CFG::BY, d.ny), cz1 = min(cz0 + (brick.y >> 16), d.nz);  // excl.
    const int sx0 = max(cx0 - 1, 0), sy0 = max(cy0 - 1, 0), sz0 = max(cz0 - 1, 0);
    const int sx1 = min(cx1, d.nx - 1), sy1 = min(cy1, d.ny - 1), sz1 = min(cz1, d.nz - 1);  // incl.
    const int ncy = sy1 - sy0 + 1;
    const int ncols = (sx1 - sx0 + 1) * ncy;
    const int nzs = sz1 - sz0 + 1;
    const float Ox = (float)(sx0 + d.ox) * d.grid_size, Oy = (float)(sy0 + d.oy) * d.grid_size,
                Oz = (float)(sz0 + d.oz) * d.grid_size;

    // ---- step A: per shell column, the cell-end table and the segment scan (wave 0) ----
    if (from_rec) {
        static_assert((CFG::BX + 2) * (CFG::BY + 2) < 32, "a column record has 32 rows: the shell columns and at least one row of totals");
        if (tid < 32) {   // (lanes >= the brick's column count hold the totals, like the tables they stand for)
            const int4 r = brec[(size_t)bidx * 32 + tid];
            sColG[tid] = r.x; sColS[tid] = r.y; sTG[tid] = r.z; sTOff[tid] = r.w;
            if (tid == 31) { sColS[64] = r.y; sTOff[64] = r.w; }
        }
    } else
    if (wave == 0) {
        int len = 0, tlen = 0, gstart = 0, tstart = 0;
        if (lane < ncols) {
            const int ix = sx0 + lane / ncy, iy = sy0 + lane % ncy;
            const int base = sph_flatten(d, ix, iy, sz0);
            gstart = d.cell_end[base > 0 ? base - 1 : 0];  // particle_system.py:384 max(0, idx-1): cell 0 quirk kept
            sCE[lane * CFG::NZS] = gstart;
#pragma unroll
            for (int k = 1; k < CFG::NZS; ++k)
                if (k <= nzs) sCE[lane * CFG::NZS + k] = d.cell_end[base + k - 1];
            len = sCE[lane * CFG::NZS + nzs] - gstart;
            if (ix >= cx0 && ix < cx1 && iy >= cy0 && iy < cy1 &&
                ((ix >= d.tgt_lo && ix < d.tgt_hi) || (ix >= d.tgt_lo2 && ix < d.tgt_hi2))) {
                // targets: cells cz0 .. cz1-1 of this column (true start, also for flat cell 0)
                tstart = (base + (cz0 - sz0) > 0) ? sCE[lane * CFG::NZS + (cz0 - sz0)] : 0;
                tlen = sCE[lane * CFG::NZS + (cz1 - sz0)] - tstart;
            }
        }
        const int incl = sph_wave_inclusive_scan(len, lane);
        const int tincl = sph_wave_inclusive_scan(tlen, lane);
        sColG[lane] = gstart - (incl - len);  // global index = LDS slot + this
        sColS[lane] = incl - len;
        sTG[lane] = tstart;
        sTOff[lane] = tincl - tlen;
        if (lane == 63) { sColS[64] = incl; sTOff[64] = tincl; }
        // the list-writing sweep leaves the tables behind for the readers of its lists (32 x 16 bytes per brick)
        if (mode_writes_list<MODE>() && brec != nullptr && lane < 32)
            brec[(size_t)bidx * 32 + lane] = make_int4(gstart - (incl - len), incl - len, tstart, tincl - tlen);
    }
    __syncthreads();
    SPH_TS(1);
    if (mode_is_df_gated<MODE>() && d.gate && gate_word == d.gate_epoch) return;  // (no barrier lies ahead of a workgroup that leaves here)
    const int T = sTOff[64];
    const int total = sColS[64];
    if (T == 0) {
        if (mode_is_df_vdiv<MODE>() && d.df_bpart != nullptr && tid == 0) d.df_bpart[bidx] = 0.0;   // (a listed brick without a target of this sweep)
        return;
    }
#ifdef SPH_PROFILE
    if (ts_on && threadIdx.x == 0) d.prof_ts[(size_t)blockIdx.x * 8 + 6] = ((unsigned long long)(unsigned)T << 32) | (unsigned)total;
#endif
    const bool overflow = total > CFG::CAP;

    // round-0 target loads are issued here, together with the staging loads below, so that their latency is
    // not a third dependent phase after the staging barrier
    // Lane -> target number.  The filter's ds_read_b128 is served in four fixed groups of 16 lanes
    // ({0-3,12-15,20-27}, {4-11,16-19,28-31}, same +32); with targets in natural order every group holds lanes of
    // all four z-cells of a column, whose runs start 8 records = 128 B = half a bank row apart at rest: cells 0/2
    // and 1/3 sit on the same banks (2-way conflict on every filter read).  Within each full block of 32 targets
    // the lanes are therefore assigned so that a group only holds cells {0,1} or {2,3}.  The same cache lines are
    // touched by the wave's global accesses either way.
    auto tmap = [&](int tn) -> int {
        if (mode_reads_list<MODE>() || V_MFMA || (tn | 31) >= T) return tn;  // (V_MFMA: a tile is 16 CONSECUTIVE targets; no per-lane ds_read_b128 left to place)
        const int l = tn & 31;
        return (tn & ~31) | (int)(((0x73261540u >> ((l >> 2) * 4)) & 7u) << 2) | (l & 3);
    };
    int col_0 = 0, gi_0 = 0, key_0 = 0;
    float4 Ai_0 = make_float4(0.f, 0.f, 0.f, 0.f), Bi_0 = Ai_0, Ei_0 = Ai_0;
    if (V_MFMA || tid < T) {   // (V_MFMA: every lane of a wave that holds a target takes part in the tiles: lanes past T mirror target T - 1)
        const int tq = tmap(V_MFMA ? min(tid, T - 1) : tid);
#pragma unroll
        for (int step = 16; step > 0; step >>= 1)
            if (sTOff[col_0 + step] <= tq) col_0 += step;
        gi_0 = sTG[col_0] + (tq - sTOff[col_0]);
        // (the one-gather force sweep finds its targets' positions in the tile it stages: the stg record IS (x, y, z, U))
        if (!(MODE == GM_FORCE_FUSED_U && !overflow)) Ai_0 = d.xm[gi_0];
        Bi_0 = d.vf[gi_0];
        Ei_0 = target_load_E<MODE>(d, gi_0);
        if (!mode_reads_list<MODE>()) key_0 = d.key[gi_0];  // (the cell's z layer: only the filter asks)
    }

    // ---- step B: stage the shell's (x, y, z, m_V) records; all loads of a lane in flight together ----
    if (!overflow) {
        float4 buf[CFG::PER];
        float4 bufg[V_GLDS ? CFG::PER : 1];
        (void)bufg;
#pragma unroll
        for (int u = 0; u < CFG::PER; ++u) {
            const int idx = min(tid + u * TPB, total - 1);  // clamped: the load is always valid
            int col = 0;  // largest col with sColS[col] <= idx (entries >= ncols hold `total`)
#pragma unroll
            for (int step = 16; step > 0; step >>= 1)
                if (sColS[col + step] <= idx) col += step;
            buf[u] = ((MODE == GM_FORCE_FUSED_U || mode_is_df_iter_u<MODE>()) ? d.stg : d.xm)[sColG[col] + idx];
            if (V_GLDS) bufg[u] = d.gat[sColG[col] + idx];
        }
        // SPH_VAR_GROUPS: the nine candidate runs of every target cell, once per brick instead of once per target (all
        // targets of a cell walk the same runs), computed while the staging loads are in flight: entry (cell, r) =
        // column << 11 | first LDS slot | length << 16, length 0 for a column outside the domain.
        if (V_GROUPS) {
            unsigned* const sRun = reinterpret_cast<unsigned*>(smem + CFG::off_run(HAS_W));
            for (int e = tid; e < CFG::NCELL * 9; e += TPB) {
                const int cell = e / 9, r = e - cell * 9;
                const int colb = cell / CFG::BZ, zc = cell - colb * CFG::BZ;
                const int ix = cx0 + colb / CFG::BY, iy = cy0 + colb % CFG::BY, cz = cz0 + zc;
                const int nx = ix + r / 3 - 1, ny = iy + r % 3 - 1;
                unsigned word = 0u;
                if (ix < cx1 && iy < cy1 && cz < cz1 && nx >= 0 && nx < d.nx && ny >= 0 && ny < d.ny) {
                    const int klo = (cz > 0 ? cz - 1 : 0) - sz0, khi = (cz < d.nz - 1 ? cz + 1 : d.nz - 1) - sz0;
                    const int ncol = (nx - sx0) * ncy + (ny - sy0);
                    const int rel = -sColG[ncol];
                    const int lo = sCE[ncol * CFG::NZS + klo] + rel, hi = sCE[ncol * CFG::NZS + khi + 1] + rel;
                    word = ((unsigned)ncol << 11) | (unsigned)lo | ((unsigned)(hi - lo) << 16);
                }
                sRun[e] = word;
            }
        }
#pragma unroll
        for (int u = 0; u < CFG::PER; ++u) {
            const int idx = tid + u * TPB;
            if (idx < total) {
                const float xl = buf[u].x - Ox, yl = buf[u].y - Oy, zl = buf[u].z - Oz;
                if (HAS_W) {
                    sQ[idx] = make_float4(-2.0f * xl, -2.0f * yl, -2.0f * zl, xl * xl + yl * yl + zl * zl);
                    if (!V_PURE) sW[idx] = buf[u].w;
                } else {
                    sQ[idx] = buf[u];  // list-reading sweeps: the record as it is, so x_i - x_j is the reference's own f32 difference
                    if (V_GLDS) sG[idx] = bufg[u];
                }
            }
        }
    }
    __syncthreads();
    SPH_TS(2);

    // ---- step C: targets ----
    double df_errsum = 0.0;   // density-change / -advection sweeps inside a solver loop: this lane's share of compute_density_error()
    for (int tn = tid; V_MFMA ? (tn & ~63) < T : tn < T; tn += TPB) {
        const bool valid = !V_MFMA || tn < T;   // V_MFMA: whole waves run the loop (wave-uniform trip count), lanes past T idle
        int col = col_0, gi = gi_0, key_i = key_0;
        float4 Ai = Ai_0, Bi = Bi_0, Ei = Ei_0;
        if (tn != tid) {  // later rounds (bricks with more than 256 targets)
            const int tq = tmap(V_MFMA ? min(tn, T - 1) : tn);
            col = 0;
#pragma unroll
            for (int step = 16; step > 0; step >>= 1)
                if (sTOff[col + step] <= tq) col += step;
            gi = sTG[col] + (tq - sTOff[col]);
            if (!(MODE == GM_FORCE_FUSED_U && !overflow)) Ai = d.xm[gi];
            Bi = d.vf[gi];
            Ei = target_load_E<MODE>(d, gi);
            if (!mode_reads_list<MODE>()) key_i = d.key[gi];
        }
        const int li = gi - sColG[col];  // own LDS slot
        if (MODE == GM_FORCE_FUSED_U && !overflow) {
            if (li >= sColS[col]) {
                Ai = sQ[li];
                Ai.w = (V_PUREF || Ai.w > 0.0f) ? d.m_V0 : -Ai.w;  // U = m / rho_raw of a fluid particle (whose m_V is m_V0 on this path), -m_V of a solid one
            } else {
                Ai = d.xm[gi];  // a target in flat cell 0: its own range is never staged (the max(0, idx-1) quirk, step A)
            }
        }
        Target t;
        target_init<MODE, V_EXACT, !V_PUREF>(d, t, Ai, Bi, Ei);
        const bool g = valid && target_gathers<MODE>(t.flags);
        bool walk = g && overflow;
        int cnt = 0;
        // ---- V_MFMA: the hit masks of the nine runs' first 32 candidates for all 64 targets of the wave, on the matrix pipe.
        // One v_mfma_f32_16x16x4_f32 = 16 candidate rows (A: (|x'|^2, -2z', -2y', -2x') of a staged record, one component per lane
        // quarter) x 16 target columns (B: (1, z', y', x') of 16 consecutive targets); D[row][col] = r^2 - |x_i'|^2, compared with
        // the target's threshold.  Lane l holds rows 4 (l >> 4) .. + 3 of column l & 15: candidate -> row is permuted so that
        // a lane quarter collects a CONTIGUOUS block of the rows, and after the four tiles of a run a 4 x 4 transpose of the four
        // mask registers (v_permlane32_swap + v_permlane16_swap) hands every lane the four blocks of ITS OWN target.
        // Rows = the union of the z windows of the tile's targets in one (x, y) column (a tile that straddles columns runs
        // once per column).  Everything below is wave-uniform control flow: EXEC is all ones at every MFMA.
        unsigned mfma_mk[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        unsigned mfma_big = 0u;   // bit r: run r has a tile with more than 64 rows -- that run takes the VALU filter
        if (V_MFMA && !overflow) {
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            typedef unsigned v2u __attribute__((ext_vector_type(2)));
            const int ixm = sx0 + col / ncy, iym = sy0 + col % ncy;
            const int czm = key_i - sph_flatten(d, ixm, iym, 0);
            const int cellidx = ((ixm - cx0) * CFG::BY + (iym - cy0)) * CFG::BZ + (czm - cz0);   // row of the run table
            const float mx = t.x - Ox, my = t.y - Oy, mz = t.z - Oz;
            const float mthr = g ? d.h * d.h * 1.0002f - (mx * mx + my * my + mz * mz) : -INFINITY;   // idle lanes: no hit
            const int q4 = lane >> 4, j16 = lane & 15;
            float Bop[4], bthr[4];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int src = 16 * gq + j16;
                const float bx = __shfl(mx, src, 64), by = __shfl(my, src, 64), bz = __shfl(mz, src, 64);
                bthr[gq] = __shfl(mthr, src, 64);
                Bop[gq] = q4 == 0 ? 1.0f : q4 == 1 ? bz : q4 == 2 ? by : bx;   // k = 0 pairs with |x_j'|^2, k = 1..3 with -2 z', -2 y', -2 x'
            }
            const unsigned* const sRunAll = reinterpret_cast<const unsigned*>(smem + CFG::off_run(HAS_W));
            // byte offset of this lane's A component inside a record, and of its row inside a block layout with stride 4C records
            const unsigned a_comp = (unsigned)(CFG::OFF_Q + (3 - q4) * 4 + (j16 & 3) * 16);
            const unsigned a_blk = (unsigned)(j16 >> 2);
            // -- the (x, y) columns of the four tiles, ONCE per round: a tile's targets are ordered by column, then z cell, so it
            // holds at most... usually one or two columns (slot A = the first lane's, slot B = the next one); a tile with a
            // third column sends the whole wave to the VALU filter (columns of < 8 targets: the fluid's surface and edges)
            unsigned selB[4];          // which of the tile's 16 targets sit in slot B's column (0: none)
            int cA0[4], cA1[4], cB0[4], cB1[4];   // run-table rows of the first / last target of each slot
            bool slow = false;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int colA = __builtin_amdgcn_readlane(col, 16 * gq);
                const unsigned sA = (unsigned)(__ballot(col == colA) >> (16 * gq)) & 0xffffu;
                const unsigned remB = 0xffffu & ~sA;
                cA0[gq] = __builtin_amdgcn_readlane(cellidx, 16 * gq);
                cA1[gq] = __builtin_amdgcn_readlane(cellidx, 16 * gq + 31 - __builtin_clz(sA));
                selB[gq] = 0u; cB0[gq] = cA0[gq]; cB1[gq] = cA0[gq];
                if (remB) {
                    const int fb = __builtin_ctz(remB);
                    const int colB = __builtin_amdgcn_readlane(col, 16 * gq + fb);
                    const unsigned sB = (unsigned)(__ballot(col == colB) >> (16 * gq)) & remB;
                    if (remB & ~sB) slow = true;
                    selB[gq] = sB;
                    cB0[gq] = __builtin_amdgcn_readlane(cellidx, 16 * gq + fb);
                    cB1[gq] = __builtin_amdgcn_readlane(cellidx, 16 * gq + 31 - __builtin_clz(sB));
                }
            }
            // -- the row ranges of all (tile, slot, run) at once: lane 9 * tile + run reads the run-table words of the slot's first
            // and last target cell -- two LDS round trips for the whole round instead of two per pass
            const int tl = lane / 9 < 4 ? lane / 9 : 3, rl = lane % 9;
            int va0 = cA0[0], va1 = cA1[0], vb0 = cB0[0], vb1 = cB1[0];
#pragma unroll
            for (int gq = 1; gq < 4; ++gq) {
                va0 = tl == gq ? cA0[gq] : va0; va1 = tl == gq ? cA1[gq] : va1;
                vb0 = tl == gq ? cB0[gq] : vb0; vb1 = tl == gq ? cB1[gq] : vb1;
            }
            const unsigned wa0 = sRunAll[va0 * 9 + rl], wa1 = sRunAll[va1 * 9 + rl];
            const unsigned wb0 = sRunAll[vb0 * 9 + rl], wb1 = sRunAll[vb1 * 9 + rl];
            const int rloA = (int)(wa0 & 2047u), nA = (int)(wa1 & 2047u) + (int)(wa1 >> 16) - rloA;
            const int rloB = (int)(wb0 & 2047u), nB = (int)(wb1 & 2047u) + (int)(wb1 >> 16) - rloB;
            const unsigned tabA = (unsigned)rloA | ((unsigned)(nA > 0 ? nA : 0) << 11);   // (rows | count << 11), count up to the tile
            const unsigned tabB = (unsigned)rloB | ((unsigned)(nB > 0 ? nB : 0) << 11);
            {   // runs with a pass of more than 64 rows (crowded cells) take the VALU filter; so does everything in a slow wave
                const bool bigl = lane < 36 && (nA > 64 || (nB > 64 && selB[tl] != 0u));
                unsigned bb = bigl ? (1u << rl) : 0u;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) bb |= __shfl_xor(bb, off, 64);
                mfma_big = slow ? 0x1ffu : bb;
            }
            // one pass = one (tile, slot, run): up to four chunks of 16 rows; loads first, then the MFMAs back to back on
            // independent accumulators, then the sign bits
            auto pass = [&](unsigned pk, int gq) -> unsigned {
                const int rlo = (int)(pk & 2047u), nrows = (int)(pk >> 11);
                const int C = nrows > 64 ? 0 : (nrows + 15) >> 4;
                unsigned mx_ = 0u;
                if (C > 0) {
                    const unsigned abase = a_comp + (unsigned)rlo * 16u + a_blk * (unsigned)(C * 64);
                    // (chunks past C re-read chunk 0: a harmless load that keeps the four requests unconditional)
                    const float a0 = *reinterpret_cast<const float*>(smem + abase);
                    const float a1 = *reinterpret_cast<const float*>(smem + abase + (C > 1 ? 64u : 0u));
                    const float a2 = *reinterpret_cast<const float*>(smem + abase + (C > 2 ? 128u : 0u));
                    const float a3 = *reinterpret_cast<const float*>(smem + abase + (C > 3 ? 192u : 0u));
                    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
                    const float bt = bthr[gq];
#define SPH_SIGN4(D_) mx_ = __builtin_amdgcn_alignbit(mx_, __float_as_uint((D_)[3] - bt), 31); \
                      mx_ = __builtin_amdgcn_alignbit(mx_, __float_as_uint((D_)[2] - bt), 31); \
                      mx_ = __builtin_amdgcn_alignbit(mx_, __float_as_uint((D_)[1] - bt), 31); \
                      mx_ = __builtin_amdgcn_alignbit(mx_, __float_as_uint((D_)[0] - bt), 31);
                    if (C > 2) {
                        const f32x4 d3 = C > 3 ? __builtin_amdgcn_mfma_f32_16x16x4f32(a3, Bop[gq], z4, 0, 0, 0) : z4;
                        const f32x4 d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, Bop[gq], z4, 0, 0, 0);
                        const f32x4 d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, Bop[gq], z4, 0, 0, 0);
                        const f32x4 d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, Bop[gq], z4, 0, 0, 0);
                        if (C > 3) { SPH_SIGN4(d3) }
                        SPH_SIGN4(d2) SPH_SIGN4(d1) SPH_SIGN4(d0)
                    } else {
                        const f32x4 d1 = C > 1 ? __builtin_amdgcn_mfma_f32_16x16x4f32(a1, Bop[gq], z4, 0, 0, 0) : z4;
                        const f32x4 d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, Bop[gq], z4, 0, 0, 0);
                        if (C > 1) { SPH_SIGN4(d1) }
                        SPH_SIGN4(d0)
                    }
#undef SPH_SIGN4
                }
                return mx_;
            };
            // (the run loop stays ROLLED -- unrolled, its 72 passes were 10 k instructions, more than the instruction cache holds --
            // and the nine masks travel through a shift register instead of being indexed by the run)
#pragma unroll 1
            for (int r = 0; r < 9; ++r) {
                unsigned m4[4];
                int rloL = 0, s1L = 0;   // of this lane's OWN target: first row and 4 C of its (tile, column)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const unsigned pkA = __builtin_amdgcn_readlane(tabA, 9 * gq + r);
                    m4[gq] = pass(pkA, gq);
                    const bool own = q4 == gq;
                    const int nrA = (int)(pkA >> 11);
                    rloL = own ? (int)(pkA & 2047u) : rloL;
                    s1L = own ? ((nrA + 15) >> 4) * 4 : s1L;
                    if (selB[gq]) {   // the tile straddles two columns: a second pass over the other column's rows
                        const unsigned pkB = __builtin_amdgcn_readlane(tabB, 9 * gq + r);
                        const unsigned mB = pass(pkB, gq);
                        const bool pieceB = ((selB[gq] >> j16) & 1u) != 0u;      // the piece's target (column j of the tile) sits in slot B's column
                        m4[gq] = pieceB ? mB : m4[gq];
                        const bool ownB = own && pieceB;
                        const int nrB = (int)(pkB >> 11);
                        rloL = ownB ? (int)(pkB & 2047u) : rloL;
                        s1L = ownB ? ((nrB + 15) >> 4) * 4 : s1L;
                    }
                }
                // 4 x 4 transpose: piece q of target (16 G + J) moves from lane 16 q + J of register G to lane 16 G + J of register q
                v2u s02 = __builtin_amdgcn_permlane32_swap(m4[0], m4[2], false, false);
                v2u s13 = __builtin_amdgcn_permlane32_swap(m4[1], m4[3], false, false);
                v2u p01 = __builtin_amdgcn_permlane16_swap(s02.x, s13.x, false, false);
                v2u p23 = __builtin_amdgcn_permlane16_swap(s02.y, s13.y, false, false);
                const unsigned a01 = p01.x | (p01.y << s1L), a23 = p23.x | (p23.y << s1L);
                const unsigned long long m64 = (unsigned long long)a01 | ((unsigned long long)a23 << (2 * s1L));
                const unsigned w = sRunAll[cellidx * 9 + r];
                const int lo = (int)(w & 2047u), len = (int)(w >> 16);
                const unsigned win = (unsigned)(m64 >> ((lo - rloL) & 63));
                const unsigned mnew = len > 0 ? (win & (0xffffffffu >> (32 - min(len, 32)))) : 0u;
#pragma unroll
                for (int k = 0; k < 8; ++k) mfma_mk[k] = mfma_mk[k + 1];
                mfma_mk[8] = mnew;   // after the ninth run mfma_mk[r] is run r's mask
            }
        }
        if (g && !overflow && !mode_reads_list<MODE>() && !SPH_ABL(d, 4)) {
            const int ix = sx0 + col / ncy, iy = sy0 + col % ncy;
            const int cz = key_i - sph_flatten(d, ix, iy, 0);  // key = flatten(ix, iy, cz)
            const int klo = (cz > 0 ? cz - 1 : 0) - sz0;  // first cell of the z-run, shell-relative
            const int khi = (cz < d.nz - 1 ? cz + 1 : d.nz - 1) - sz0;
            const float txl_ = t.x - Ox, tyl_ = t.y - Oy, tzl_ = t.z - Oz;
            // superset filter (exact r < h test in phase 2): r2 - |x_i'|^2 < h^2 (1 + 2e-4) - |x_i'|^2
            const float thr = d.h * d.h * 1.0002f - (txl_ * txl_ + tyl_ * tyl_ + tzl_ * tzl_);
            // The list goes through a raw buffer the size of its 24 entry groups -- a store beyond them is dropped by the
            // hardware range check (no compare, no branch), the byte offset is one 32-bit VGPR -- and the constants of
            // the pair term sit in VGPRs (an SGPR source halves a VALU instruction's issue rate).
            // Entry r of particle i lives at (r >> 2) << lshift | i * 8 | (r & 3) * 2: four consecutive entries of a
            // particle are one 8-byte word (the list-reading sweeps fetch them with one load), a wave's words of one
            // entry group are contiguous, and a group spans 2^lshift >= cap * 8 bytes.  The running offset `voff` keeps the
            // particle field filled with ones (lmask), so that `+ 2` carries out of the entry field straight into the group
            // field: next = (voff + 2, saturating) | lmask, address = voff ^ lflip.
            const __amdgpu_buffer_rsrc_t lrs = sph_rsrc(glist, (unsigned)(SPH_GLIST_ROWS / 4) << lshift);
            const unsigned lmask = sph_in_vgpr((1u << lshift) - 8u);
            const unsigned lflip = lmask ^ ((unsigned)gi * 8u);
            unsigned voff = lmask;
            const float v_inv_h = sph_in_vgpr(d.inv_h);
            const float v_kw2 = sph_in_vgpr(d.k_w * 2.0f);
            const float v_kw8 = sph_in_vgpr(d.k_w * 8.0f);
            const float v_mV0 = sph_in_vgpr(d.m_V0);
            (void)lrs; (void)voff; (void)lflip; (void)v_inv_h; (void)v_kw2; (void)v_kw8; (void)v_mV0;
// Hits are collected in a per-run bitmask register (no LDS traffic while filtering) and turned into list
// entries once per chunk of <= 32 candidates: ~7 ds_write per run instead of one per candidate.
// One candidate = 3 FMA + 1 add + 1 v_alignbit: the test value r2' - thr' is negative for a hit, and alignbit shifts
// its SIGN BIT into the mask ((mask << 1) | sign) -- no compare, no select.  A chunk is walked from its last candidate
// to its first, so candidate k ends up at bit k and the hits come out in ascending order with ffs / clear-lowest-bit.
#define SPH_ACC(Q_) mask = __builtin_amdgcn_alignbit(mask, __float_as_uint(fmaf(txl_, (Q_).x, fmaf(tyl_, (Q_).y, fmaf(tzl_, (Q_).z, (Q_).w - thr)))), 31)
            // hit mask of the n <= 32 candidates from LDS slot `base` on (n >= 1)
            auto filter_chunk = [&](int base, int n) -> unsigned {
                unsigned mask = 0;
                // Whole groups of 8 only.  Up to 7 records past the run's end are tested too (they are
                // the next run's, or the first bytes of the m_V array behind the last record: always inside
                // this workgroup's LDS) and their bits are cleared afterwards -- 7 wasted tests at 5 VALU each
                // instead of up to 7 one-candidate trips that each wait for their own ds_read.
                int k = (n + 7) & ~7;
                while (k > 0) {
                    k -= 8;
                    const float4* q = &sQ[base + k];
                    const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
                    const float4 q4 = q[4], q5 = q[5], q6 = q[6], q7 = q[7];
                    SPH_ACC(q7); SPH_ACC(q6); SPH_ACC(q5); SPH_ACC(q4);
                    SPH_ACC(q3); SPH_ACC(q2); SPH_ACC(q1); SPH_ACC(q0);
                }
                mask &= 0xffffffffu >> (32 - n);
#ifdef SPH_PROFILE
                if (d.ablate & 16) mask &= (d.ablate >> 8);  // profiling: filter only (mask kept live, no hit emitted)
#endif
                return mask;
            };
#undef SPH_ACC
            // density pair term of the hit whose record sits at LDS byte offset aq of the Q array (addresses and
            // constants arranged for the issue rates)
            auto pair_term = [&](unsigned aq) {
                const float4 q4 = *reinterpret_cast<const float4*>(smem + CFG::OFF_Q + aq);
                const float mVj = V_PURE ? v_mV0 : *reinterpret_cast<const float*>(smem + CFG::off_w(true) + (aq >> 2));
                const float rx = fmaf(0.5f, q4.x, txl_), ry = fmaf(0.5f, q4.y, tyl_), rz = fmaf(0.5f, q4.z, tzl_);
                const float r2 = rx * rx + ry * ry + rz * rz;
                if (V_EXACT) { t.s0 += mVj * sph_W_exact(d, __fsqrt_rn(r2)); return; }  // WCSPH.py:19-30 as the reference's f32 expressions
                const float qn = __builtin_amdgcn_sqrtf(r2) * v_inv_h;  // v_sqrt_f32 (1 ulp; exact 0 for the self pair)
                // sph_base.py:23-44 in one expression for both branches: with t = (1-q)+ and
                // u = (1/2-q)+ the cubic spline is k (2 t^3 - 8 u^3) -- for q <= 1/2 this IS
                // k (6 q^3 - 6 q^2 + 1), beyond it u = 0 leaves the outer branch, from q = 1 on t = 0.
                // Two clamped FMAs replace the compare + select and the second polynomial (all
                // full-rate opcodes); rounding differs from the two-branch form by ~2e-7 of W(0).
                const float tq = fminf(fmaxf(1.0f - qn, 0.0f), 1.0f);                // one v_fma ... clamp
                const float uq = fminf(fmaxf(0.5f - qn, 0.0f), 1.0f);
                const float w = v_kw2 * (tq * tq * tq) - v_kw8 * (uq * uq * uq);
                t.s0 += mVj * w;
            };
            // the hits of one mask become list entries `tagbase + bit` and (inline sweeps) density terms
            unsigned last_e = 0u;  // the entry written last (pads the final group of four)
            auto emit_micro = [&](unsigned mask, unsigned tagbase, unsigned base16) {
                cnt += __popc(mask);
                while (mask) {
                    const unsigned bit = (unsigned)__ffs((int)mask) - 1u;
                    mask &= mask - 1u;
                    last_e = tagbase + bit;
                    if (!SPH_ABL(d, 2)) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)last_e, lrs, (int)(voff ^ lflip), 0, 0);
                    voff = __builtin_elementwise_add_sat(voff, 2u) | lmask;
                    if (INLINE_PHYS && !SPH_ABL(d, 32)) pair_term(base16 + (bit << 4));
                }
            };
            if (V_GROUPS) {
                // SPH_VAR_GROUPS (default): all nine runs are filtered first (their first 32 candidates: one mask and
                // one tag|base per run stay in registers; longer runs emit their further chunks at once), then every
                // lane emits its runs by descending hit count within three groups -- the centre run (it always holds the
                // most hits), the four edge runs, the four corner runs: phase p then costs the wave about the p-th
                // largest count of its busiest lane (tools/emission_model.py: 109 -> ~69 trips per wave in a settled flow).
                unsigned mk[9], tk[9];
                const unsigned* const runs = reinterpret_cast<const unsigned*>(smem + CFG::off_run(HAS_W)) +
                                             (((ix - cx0) * CFG::BY + (iy - cy0)) * CFG::BZ + (cz - cz0)) * 9;
                bool longrun = false;
#pragma unroll
                for (int r = 0; r < 9; ++r) {
                    const unsigned w = runs[r];
                    const int len = (int)(w >> 16);
                    if (V_MFMA && !((mfma_big >> r) & 1u)) mk[r] = mfma_mk[r];
                    else mk[r] = len > 0 ? filter_chunk((int)(w & 2047u), min(32, len)) : 0u;
                    tk[r] = w & 0xffffu;
                    longrun |= len > 32;
                }
                if (longrun)  // (rare) chunks beyond the first 32 candidates of a run
                    for (int r = 0; r < 9; ++r) {
                        const unsigned w = runs[r];
                        const int lo = (int)(w & 2047u), hi = lo + (int)(w >> 16);
                        for (int base = lo + 32; base < hi; base += 32)
                            emit_micro(filter_chunk(base, min(32, hi - base)), (w & 0xf800u) | (unsigned)base, (unsigned)base << 4);
                    }
#pragma unroll
                for (int r = 0; r < 9; ++r) tk[r] |= (unsigned)__popc(mk[r]) << 16;
                // ten compare-exchanges on the words (hits << 16 | tag|base), the mask travelling with its word
#define SPH_CE(A_, B_) { const bool sw_ = tk[A_] < tk[B_]; const unsigned ta_ = tk[A_], ma_ = mk[A_]; \
                         tk[A_] = sw_ ? tk[B_] : ta_; mk[A_] = sw_ ? mk[B_] : ma_; tk[B_] = sw_ ? ta_ : tk[B_]; mk[B_] = sw_ ? ma_ : mk[B_]; }
                SPH_CE(1, 3) SPH_CE(5, 7) SPH_CE(1, 5) SPH_CE(3, 7) SPH_CE(3, 5)
                SPH_CE(0, 2) SPH_CE(6, 8) SPH_CE(0, 6) SPH_CE(2, 8) SPH_CE(2, 6)
#undef SPH_CE
                constexpr int order[9] = {4, 1, 3, 5, 7, 0, 2, 6, 8};
#pragma unroll
                for (int p = 0; p < 9; ++p) emit_micro(mk[order[p]], tk[order[p]] & 0xffffu, (tk[order[p]] & 2047u) << 4);
            } else
            // baseline (variant 0; also what the stand-alone filtering sweeps run): run by run in the reference's
            // (dx, dy) order, every chunk emitted as soon as it is filtered
            for (int dx = -1; dx <= 1; ++dx) {
                const int nx = ix + dx;
                if (nx < 0 || nx >= d.nx) continue;
                for (int dy = -1; dy <= 1; ++dy) {
                    const int ny = iy + dy;
                    if (ny < 0 || ny >= d.ny) continue;
                    const int ncol = (nx - sx0) * ncy + (ny - sy0);
                    const int rel = -sColG[ncol];
                    const int lo = sCE[ncol * CFG::NZS + klo] + rel;
                    const int hi = sCE[ncol * CFG::NZS + khi + 1] + rel;
                    for (int base = lo; base < hi; base += 32)
                        emit_micro(filter_chunk(base, min(32, hi - base)), ((unsigned)ncol << 11) | (unsigned)base, (unsigned)base << 4);
                }
            }
            // The readers fetch whole groups of four: the rest of the last group repeats the last entry written -- a staged
            // record by construction (the target's own slot would not do: a target in flat cell 0 is never staged, the
            // max(0, idx-1) quirk).  Entries beyond the count are fetched, never paired.
            if ((cnt & 3) && !SPH_ABL(d, 2)) {
                for (int u = cnt & 3; u < 4; ++u) {
                    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)last_e, lrs, (int)(voff ^ lflip), 0, 0);
                    voff = __builtin_elementwise_add_sat(voff, 2u) | lmask;
                }
            }
            // list overflow (extreme compression): the list-reading sweep must take the exact slow path; this
            // sweep too, unless its pair term was already summed inline (complete regardless of the list length)
            const bool list_ovf = cnt > CFG::LISTCAP && !SPH_ABL(d, 8);
            // (flat cell 0's own range is never visited -- the reference's max(0, idx-1) quirk -- so a target that
            // lives there does not meet itself in the list and keeps the explicit self term)
            if (INLINE_PHYS) t.self_in_sum = key_i != 0;
            else if (list_ovf) walk = true;
            if (mode_writes_list<MODE>()) gcnt[gi] = (unsigned char)(walk ? SPH_CNT_WALK : list_ovf ? SPH_CNT_LIST_OVF : cnt);
            __threadfence_block();  // this lane re-reads its own entries below
        }
        if (mode_reads_list<MODE>() && g && !overflow) {
            cnt = gcnt[gi];
            if (cnt >= SPH_CNT_LIST_OVF) { walk = true; cnt = 0; }
        }
        if (mode_writes_list<MODE>() && g && overflow) gcnt[gi] = (unsigned char)SPH_CNT_WALK;
        if (g && !walk && !SPH_ABL(d, 1) && !mode_inline_physics<MODE>()) {
            // phase 2: pair physics over the list.  Register sets rotate: while pair k is computed from one, the
            // records of the next entries are in flight into the others.  Every fetch is UNCONDITIONAL (past the end it re-reads
            // the last entry), so each set is always defined by loads and never by a copy of the other -- the
            // conditional form cost ~30 v_mov per pair in register shuffling.
            const float txl = t.x - Ox, tyl = t.y - Oy, tzl = t.z - Oz;
            (void)txl; (void)tyl; (void)tzl;
            struct Slot { float4 A, B, C; int g, j; };
            ForceK FK;
            if (V_BF) FK = force_k(d);
            // the list groups through a raw buffer; V_BF: the gat gather too (32-bit byte offsets instead of 64-bit pointer arithmetic)
            const __amdgpu_buffer_rsrc_t grs = sph_rsrc(d.gat, (unsigned)d.N * 16u);
            const __amdgpu_buffer_rsrc_t lrs3 = sph_rsrc(glist, (unsigned)(SPH_GLIST_ROWS / 4) << lshift);
            (void)grs; (void)lrs3;
            auto fetch = [&](Slot& s_, unsigned e) {
                s_.j = e & 2047;
                s_.A = sQ[s_.j];  // list-reading sweeps: (x, y, z, m_V)
                if (HAS_W) s_.A.w = sW[s_.j];
                s_.g = sColG[e >> 11] + s_.j;
#ifdef SPH_PROFILE
                if ((d.ablate & 128) && mode_needs_B<MODE>()) {  // profiling build: no neighbour gather
                    s_.B = make_float4(0.f, 0.f, 0.f, 1.0f);
                } else
#endif
                if (V_GLDS) {
                    s_.B = sG[s_.j];
                } else
                if (V_BF) {
                    typedef float v4f __attribute__((ext_vector_type(4)));
                    const v4f b = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(grs, s_.g << 4, 0, 0));
                    s_.B = make_float4(b.x, b.y, b.z, b.w);
                } else
                s_.B = mode_needs_B<MODE>() ? (MODE == GM_FORCE_FUSED_U ? d.gat : d.vf)[s_.g] : make_float4(0.f, 0.f, 0.f, 0.f);
                s_.C = mode_needs_C<MODE>() ? load_C_global<MODE>(d, s_.g) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (mode_is_df_iter_u<MODE>()) s_.C.x = d.kbuf[s_.g];  // the one 4-byte gather of these sweeps
            };
            auto pair = [&](const Slot& s_) {
                // filtering sweeps hold x_j' = -A/2 in shell-local coordinates; list-reading sweeps hold x_j itself
                const float rx = HAS_W ? fmaf(0.5f, s_.A.x, txl) : t.x - s_.A.x;
                const float ry = HAS_W ? fmaf(0.5f, s_.A.y, tyl) : t.y - s_.A.y;
                const float rz = HAS_W ? fmaf(0.5f, s_.A.z, tzl) : t.z - s_.A.z;
                const float r2 = rx * rx + ry * ry + rz * rz;
                if (V_EXACT) { pair_force_u_exact(d, t, rx, ry, rz, r2, s_.A, s_.B, s_.g, s_.j != li); return; }
                if (V_PUREF) { pair_force_u_bf<true>(d, FK, t, rx, ry, rz, r2, s_.A, s_.B, 0, true); return; }
                if (V_BF) { pair_force_u_bf(d, FK, t, rx, ry, rz, r2, s_.A, s_.B, s_.g, s_.j != li); return; }
                const float rinv = sph_rsq(r2);
                const float rn = r2 * rinv;
                if (sph_within<MODE>(d, r2, rn) && s_.j != li)  // particle_system.py:385
                    pair_physics<MODE>(d, t, rx, ry, rz, r2, rn, rinv, s_.A, s_.B, s_.C, s_.g);
            };
            if (cnt > 0) {
                // Four entries per load: group g of this lane (g is wave-uniform, clamped to the lane's last group, so every
                // entry that is fetched is one the density sweep wrote -- its own or the padding behind them).
                const unsigned gi8 = (unsigned)gi * 8u;
                const int lastg = (cnt - 1) >> 2;
                auto ldg = [&](int g) -> uint2 {
                    typedef unsigned v2u __attribute__((ext_vector_type(2)));
                    const v2u w = __builtin_bit_cast(v2u, __builtin_amdgcn_raw_buffer_load_b64(lrs3, (int)(((unsigned)min(g, lastg) << lshift) + gi8), 0, 0));
                    return make_uint2(w.x, w.y);
                };
                // Four slots, three of them live at any time: the records of pairs k+1 and k+2 are in flight while pair k
                // is computed (the fourth name only keeps the rotation in step with the groups of four).
                Slot s0, s1, s2, s3;
                uint2 cur = ldg(0), nxt = ldg(1);
                fetch(s0, cur.x & 0xffffu);
                fetch(s1, cur.x >> 16);
                if (V_DEEP) {
                    // The entries head a dependent chain (entry -> column table in LDS -> record gather): the group three
                    // ahead is requested at the top of the round, two rounds of slack for its trip to L2.
                    uint2 nn = ldg(2);
                    for (int k = 0; k < cnt; k += 4) {
                        const uint2 n3 = ldg((k >> 2) + 3);
                        fetch(s2, cur.y & 0xffffu);
                        pair(s0);
                        fetch(s3, cur.y >> 16);
                        if (k + 1 < cnt) pair(s1);
                        fetch(s0, nxt.x & 0xffffu);
                        if (k + 2 < cnt) pair(s2);
                        fetch(s1, nxt.x >> 16);
                        if (k + 3 < cnt) pair(s3);
                        cur = nxt; nxt = nn; nn = n3;
                    }
                } else
                for (int k = 0; k < cnt; k += 4) {
                    const uint2 nn = ldg((k >> 2) + 2);
                    fetch(s2, cur.y & 0xffffu);
                    pair(s0);
                    fetch(s3, cur.y >> 16);
                    if (k + 1 < cnt) pair(s1);
                    fetch(s0, nxt.x & 0xffffu);
                    if (k + 2 < cnt) pair(s2);
                    fetch(s1, nxt.x >> 16);
                    if (k + 3 < cnt) pair(s3);
                    cur = nxt; nxt = nn;
                }
            }
        }
        if (walk) {
            target_init<mode_walk<MODE>()>(d, t, Ai, Bi, Ei);
            gather_walk_global<mode_walk<MODE>()>(d, t, gi);
        }
        SPH_TS(3);
        if (valid) target_finish<MODE, V_EXACT>(d, t, gi, g, Ei);
        if (mode_is_df_vdiv<MODE>() && d.df_bpart != nullptr) df_errsum += (double)t.df_err;
    }
    SPH_TS(4);
    // SPH_OPT_DF_FUSE_ERROR (round 6): the iteration's convergence test needs sum over fluid of (density_0 * density_adv - offset); the
    // values are in registers here, so the brick leaves its partial (f64, fixed order: lane's rounds, wave tree, waves 0..3) and the
    // streaming kernel that re-read eos + flags of every particle (10.6 us, 7-8 times per step at 1.75 M) is not launched
    if constexpr (mode_is_df_vdiv<MODE>()) {
        __shared__ double df_red[TPB / 64];
        if (d.df_bpart != nullptr) {   // (uniform over the launch)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) df_errsum += __shfl_down(df_errsum, off, 64);
            if (lane == 0) df_red[wave] = df_errsum;
            __syncthreads();
            if (tid == 0) {
                double tot = 0.0;
                for (int w = 0; w < TPB / 64; ++w) tot += df_red[w];
                d.df_bpart[bidx] = tot;
            }
        }
    }
    }
}

// after a sweep that scatters coupling reactions: acc of every dynamic rigid particle += its fixed-point sums, which
// return to zero (the accumulators are all zero between sweeps, whatever the order of the particles becomes)
__global__ __launch_bounds__(TPB) void k_fold_coupling(DevView d, const int* __restrict__ list, int first, int n) {
    if (d.gate && *d.gate == d.gate_epoch) return;  // (inside a DFSPH solver loop only: the sweep it would fold never ran)
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    // list == nullptr: the list of dynamic rigid particles is not current (a slab rank between its truncate and the
    // next sort): every particle looks at its own flags instead
    const int i = list ? list[t] : first + t;
    if (!list && !sph_is_dynamic_rigid(__float_as_int(d.vf[i].w))) return;
    long long* f = d.acc_fx + 3 * (size_t)i;
    const long long fx = f[0], fy = f[1], fz = f[2];
    if ((fx | fy | fz) == 0) return;
    f[0] = 0; f[1] = 0; f[2] = 0;
    float4 a = d.acc[i];
    a.x += (float)((double)fx * (1.0 / 4294967296.0));
    a.y += (float)((double)fy * (1.0 / 4294967296.0));
    a.z += (float)((double)fz * (1.0 / 4294967296.0));
    d.acc[i] = a;
}

int sphk_fold_coupling(SphContext* c) {
    if (c->opt_no_dynamic || sph_n_dyn(c) == 0 || c->N <= 0) return 0;
    DevView d = sph_view(c);
    const bool have_list = sph_n_dyn(c) > 0;
    const int n = have_list ? sph_n_dyn(c) : c->N;
    hipLaunchKernelGGL(k_fold_coupling, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, d, have_list ? c->dyn_list : nullptr, 0, n);
    SPH_LAUNCH_CHECK(c);
    return 0;
}

// the same for the records [first, first + count) only, on the stream of the sweep that scattered to them (slab mode:
// the halo packers advance the boundary layers' records right behind the boundary force launch and need those
// particles' reactions -- complete by then, sph_slab_forces -- while the interior launch is still scattering to others)
int sphk_fold_coupling_range(SphContext* c, int first, int count, hipStream_t st) {
    if (c->opt_no_dynamic || sph_n_dyn(c) == 0 || count <= 0) return 0;
    DevView d = sph_view(c);
    hipLaunchKernelGGL(k_fold_coupling, dim3((count + TPB - 1) / TPB), dim3(TPB), 0, st, d, (const int*)nullptr, first, count);
    SPH_LAUNCH_CHECK(c);
    return 0;
}

// density / pressure of the fluid from the lean record (p, rho) of the uniform-fluid step into aux (sph_ensure_aux)
__global__ __launch_bounds__(TPB) void k_aux_from_eos2(DevView d) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= d.N) return;
    if (!sph_is_fluid(__float_as_int(d.vf[i].w))) return;
    const float2 e = d.eos2[i];
    float* a = reinterpret_cast<float*>(&d.aux[i]);
    a[1] = e.y;
    a[2] = e.x;
}

// ... and, behind a lean scatter (sph_sort.hip), the WHOLE record: the one uniform mass, density / pressure (from eos2 when
// EOS2; else the words aux holds stay -- nobody has computed newer ones for this order), and the id from the pid array.  Every
// particle of a lean run is a fluid particle of that mass (sphd_sort_lean_usable).
template <bool EOS2>
__global__ __launch_bounds__(TPB) void k_aux_from_pid(DevView d) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= d.N) return;
    const float w = __int_as_float(d.pid[i]);
    if (EOS2) {
        const float2 e = d.eos2[i];
        d.aux[i] = make_float4(d.m_u, e.y, e.x, w);
    } else {
        float* a = reinterpret_cast<float*>(&d.aux[i]);
        a[0] = d.m_u;
        a[3] = w;
    }
}

int sph_ensure_aux(SphContext* c) {
    if (!sphd_aux_needs_fold(c->dv)) return 0;
    const bool eos2 = sphd_aux_in_eos2(c->dv), apart = sphd_pid_apart(c->dv);
    sphd_aux_folded(c->dv);
    if (c->N <= 0) return 0;
    DevView d = sph_view(c);
    const dim3 grid((c->N + TPB - 1) / TPB);
    if (!apart) hipLaunchKernelGGL(k_aux_from_eos2, grid, dim3(TPB), 0, c->stream, d);
    else if (eos2) hipLaunchKernelGGL(k_aux_from_pid<true>, grid, dim3(TPB), 0, c->stream, d);
    else hipLaunchKernelGGL(k_aux_from_pid<false>, grid, dim3(TPB), 0, c->stream, d);
    SPH_LAUNCH_CHECK(c);
    return 0;
}

// EOS alone (first loop of compute_pressure_forces, WCSPH.py:71-76)
__global__ __launch_bounds__(TPB) void k_eos(DevView d) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= d.N) return;
    if (!sph_is_fluid(__float_as_int(d.vf[i].w))) return;
    float4 aux = d.aux[i];
    aux.y = fmaxf(aux.y, d.rho0);
    aux.z = d.stiffness * (sph_tait_pow<false>(d, aux.y / d.rho0) - 1.0f);
    d.aux[i] = aux;
}

// ---------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------
typedef BrickCfg<4, 2, 4, 1792, 95> Cfg0;  // 4x2 columns x up to 4 layers: 1152 candidates / 256 targets at rest
// SPH_VAR_GAT_LDS / _LDS4: the force sweep's tile holds two records per shell particle (32 B): smaller tiles, so that three / four
// workgroups still fit a CU's 160 KiB (45 + 2.3 KiB / 37.5 + 2.3 KiB); the partition of the whole step is cut for them
typedef BrickCfg<4, 2, 4, 1408, 95> CfgG3;
typedef BrickCfg<4, 2, 4, 1200, 95> CfgG4;
// shell records a brick may hold (the cut rule of k_brick_list): the smallest tile among the kernels of the step
static int brick_smax(const SphContext* c) {
    if (c->opt_variant & SPH_VAR_GAT_LDS) return CfgG3::CAP;
    if (c->opt_variant & SPH_VAR_GAT_LDS4) return CfgG4::CAP;
    return Cfg0::CAP;
}

template <int MODE>
static int launch_simple(SphContext* c, const int* list, int n) {
    if (n <= 0) return 0;
    DevView d = sph_view(c);
    hipLaunchKernelGGL(k_gather_simple<MODE>, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, d, list, n);
    SPH_LAUNCH_CHECK(c);
    return 0;
}

// The brick sweeps address their list entries with 32-bit byte offsets (SPH_GLIST_ROWS / 4 groups of 2^glist_shift bytes,
// sph_api.hip) and k_brick_list keeps per-layer arrays in LDS (SPH_BRICK_MAX_NZ): contexts beyond either limit (> 16.7 M
// particles of capacity, > 1000 cell layers in z) take the per-particle cell walk.
static bool brick_ok(const SphContext* c) {
    return c->glist_shift > 0 && c->p.grid_num[2] <= SPH_BRICK_MAX_NZ;
}

bool sphk_brick_sweeps_reach(const SphContext* c) { return brick_ok(c); }

// identity of a partition: footprint, cut rule, limits (the target ranges complete the key)
static int brick_partition_id(const SphContext* c) {
    const int fixed_bz = c->opt_brick_shape == 1 ? SPH_BRICK_BZ : 0;
    return ((SPH_BRICK_BX * 10 + SPH_BRICK_BY) * 10 + SPH_BRICK_BZ) * 4096 + fixed_bz * 2048 + brick_smax(c);
}
static SphPartKey brick_key(const SphContext* c, const DevView& d) { return {brick_partition_id(c), d.tgt_lo, d.tgt_hi, d.tgt_lo2, d.tgt_hi2}; }

// The list for the step's default sweeps (targets = the density layers), to be built by the sort's place kernel in
// extra workgroups: fills `a` (nblocks = 0 if the brick sweeps will not run) and `key`; the caller reports both once the
// sort has been enqueued.
int sphk_brick_list_prepare(SphContext* c, BrickListArgs* a, SphPartKey* key) {
    memset(a, 0, sizeof(*a));
    *key = SphPartKey{};
    if (c->N <= 0 || c->opt_gather_impl != 1 || !brick_ok(c)) return 0;
    DevView d = sph_view(c);
    d.tgt_lo = c->tgt_layers[0]; d.tgt_hi = c->tgt_layers[1]; d.tgt_lo2 = d.tgt_hi2 = 0;
    if (d.tgt_hi <= d.tgt_lo) return 0;
    const int nbx = (d.nx + SPH_BRICK_BX - 1) / SPH_BRICK_BX, nby = (d.ny + SPH_BRICK_BY - 1) / SPH_BRICK_BY;
    if (nbx * nby * d.nz > c->brick_cap) return 0;
    a->d.nx = d.nx; a->d.ny = d.ny; a->d.nz = d.nz;
    a->d.tgt_lo = d.tgt_lo; a->d.tgt_hi = d.tgt_hi; a->d.tgt_lo2 = 0; a->d.tgt_hi2 = 0;
    a->d.cell_end = d.cell_end;
    a->nbx = nbx; a->nby = nby;
    a->list = c->brick_list; a->count = c->brick_count; a->list_cap = c->brick_cap;
    a->tmax = TPB; a->smax = brick_smax(c); a->fixed_bz = c->opt_brick_shape == 1 ? SPH_BRICK_BZ : 0;
    a->nblocks = (nbx * nby + TPB / 64 - 1) / (TPB / 64);
    a->lds_bytes = (unsigned)((TPB / 64) * 5 * (d.nz + 1) * sizeof(int));
    *key = brick_key(c, d);
    return 0;
}

template <int MODE, class CFG, int VAR = 0>
static int launch_brick_cfg(SphContext* c, const SweepArgs& a) {
    DevView d = sph_view(c);
    d.fuse_advect = a.fuse_advect;
    d.store_acc = a.store_acc || !a.fuse_advect;  // (only the fused advect has consumed the acceleration it does not store)
    d.df_bpart = a.collect_bpart ? c->df_bpart : nullptr;
    if (MODE == GM_DENSITY_EOS) { d.tgt_lo = c->tgt_layers[0]; d.tgt_hi = c->tgt_layers[1]; d.write_sg = sphs_uniform(c->ss); }
    if (MODE == GM_DF_DENSITY) d.write_sg = 1;
    if (mode_is_df_vdiv<MODE>()) d.write_k = 1;
    if (MODE == GM_FORCE_FUSED || MODE == GM_FORCE_FUSED_U) { d.tgt_lo = c->tgt_layers[2]; d.tgt_hi = c->tgt_layers[3]; }
    if (a.lo >= 0) { d.tgt_lo = a.lo; d.tgt_hi = a.hi; d.tgt_lo2 = a.lo2; d.tgt_hi2 = a.hi2; }
    if (d.tgt_hi2 <= d.tgt_lo2) d.tgt_lo2 = d.tgt_hi2 = 0;
    if (d.tgt_hi <= d.tgt_lo) { d.tgt_lo = d.tgt_lo2; d.tgt_hi = d.tgt_hi2; d.tgt_lo2 = d.tgt_hi2 = 0; }
    if (d.tgt_hi <= d.tgt_lo) return 0;
    const int nbx = (d.nx + CFG::BX - 1) / CFG::BX, nby = (d.ny + CFG::BY - 1) / CFG::BY;
    const int ncg = nbx * nby;          // column groups
    const int nbricks = ncg * d.nz;     // at worst every z layer is a brick of its own
    if (nbricks > c->brick_cap) return sph_fail(c, SPH_E_INVALID, "brick list capacity exceeded");
    const int bytes = CFG::bytes(!mode_reads_list<MODE>()) +
                      (((VAR & (SPH_VAR_GAT_LDS | SPH_VAR_GAT_LDS4)) && MODE == GM_FORCE_FUSED_U) ? CFG::CAP * 16 : 0);
    static bool attr_set[64] = {};  // per device: the attribute belongs to the function ON a device
    const int dev = c->device >= 0 && c->device < 64 ? c->device : 0;
    if (!attr_set[dev]) {
        SPH_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gather_brick<MODE, CFG, VAR>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        attr_set[dev] = true;
    }
    const int grid = (nbricks + 7) / 8 * 8 + 8;  // per XCD: ceil(heavy / 8) + ceil(light / 8) <= ceil(nbricks / 8) + 1 slots
    // The partition depends only on the order, the target layers and the cut rule: every sweep of a step that shares
    // them (density + force; all ~30 sweeps of a DFSPH step) reuses it -- and MUST, where one sweep reads the lists
    // another wrote (list entries are brick-relative).
    const int fixed_bz = c->opt_brick_shape == 1 ? CFG::BZ : 0;
    const int tmax = TPB, smax = brick_smax(c);
    const SphPartKey key = brick_key(c, d);
    hipStream_t st = a.side ? c->side : c->stream;
    int2* blist = a.side ? c->brick_list2 : c->brick_list;
    int* bcount = a.side ? c->brick_count2 : c->brick_count;
    // A cached list also serves a sweep whose target ranges lie INSIDE the cached (single) one -- slab mode: the force
    // sweeps over the boundary layers (side stream) and the interior after the density sweep over owned + first ghost
    // layers. Bricks listed for the wider range that hold no target of this sweep leave at T == 0. For a sweep that
    // reads the neighbour lists this is not an economy but the rule: the entries are offsets into the tile of the brick
    // that wrote them, and the adaptive cut depends on the target ranges, so a partition of its own would misread them.
    if (sphd_partition_hit(c->dv, key) != SPH_PART_NO) {
        blist = c->brick_list; bcount = c->brick_count;  // (read-only here; the side stream forked after it was built)
    } else {
        if (mode_reads_list<MODE>())
            return sph_fail(c, SPH_E_INVALID, "the sweep reads neighbour lists but its targets lie outside the partition that wrote them");
        if (a.side || !sphd_count_is_zero(c->dv)) SPH_HIP(c, hipMemsetAsync(bcount, 0, 2 * sizeof(int), st));
        hipLaunchKernelGGL((k_brick_list<CFG>), dim3((ncg + TPB / 64 - 1) / (TPB / 64)), dim3(TPB), (size_t)(TPB / 64) * 5 * (d.nz + 1) * sizeof(int),
                           st, d, nbx, nby, blist, bcount, c->brick_cap, tmax, smax, fixed_bz);
        SPH_LAUNCH_CHECK(c);
        // (the side stream's list is private to that launch and never cached)  The main stream's replaces the cached one, and
        // the lists and column records written over that one go with it: their entries are relative to ITS bricks.
        if (!a.side) sphd_partition_rebuilt(c->dv, key);
    }
    // the per-brick column records: written by a list-writing sweep over the cached list of the main stream, read back by
    // the list readers whose target ranges are exactly the writer's (a subset sweep -- slab mode -- has other target tables)
    int use_rec = 0;
    int4* brec = nullptr;
    if (c->brick_rec && blist == c->brick_list && c->opt_brick_rec) {
        if (mode_writes_list<MODE>()) {
            brec = c->brick_rec;
            sphd_records_written(c->dv, key);
        } else if (mode_reads_list<MODE>() && sphd_records_usable(c->dv, key)) {
            brec = c->brick_rec;
            use_rec = 1;
        }
    }
    hipLaunchKernelGGL((k_gather_brick<MODE, CFG, VAR>), dim3(grid), dim3(TPB), bytes, st, d, nby, blist, bcount, c->glist,
                       c->gcnt, c->cap, c->brick_cap, c->glist_shift, brec, use_rec);
    SPH_LAUNCH_CHECK(c);
    return 0;
}

template <int MODE>
static int launch_brick(SphContext* c, const SweepArgs& a) {
    // SPH_OPT_KERNEL_VARIANT: the instances of the two sweeps of the fused WCSPH step (include/sph_hip.h)
    const int var = c->opt_variant;
    if constexpr (MODE == GM_DENSITY_EOS) {
        if (c->opt_exact_math) return launch_brick_cfg<MODE, Cfg0, SPH_VAR_GROUPS | SPH_VAR_EXACT>(c, a);
        if ((var & SPH_VAR_GROUPS) && (var & SPH_VAR_MFMA)) return launch_brick_cfg<MODE, Cfg0, SPH_VAR_GROUPS | SPH_VAR_MFMA>(c, a);
        // (the rule that admits the pure-fluid instances: sph_pure_fluid_instances, sph_internal.h)
        if ((var & SPH_VAR_GROUPS) && sph_pure_fluid_instances(c))
            return launch_brick_cfg<MODE, Cfg0, SPH_VAR_GROUPS | SPH_VAR_PURE_INTERNAL>(c, a);
        if (var & SPH_VAR_GROUPS) return launch_brick_cfg<MODE, Cfg0, SPH_VAR_GROUPS>(c, a);
    }
    if constexpr (MODE == GM_FORCE_FUSED_U) {
        if (c->opt_exact_math) return launch_brick_cfg<MODE, Cfg0, SPH_VAR_EXACT>(c, a);
        if (var & SPH_VAR_GAT_LDS) return launch_brick_cfg<MODE, CfgG3, SPH_VAR_FORCE_BF | SPH_VAR_DEEP | SPH_VAR_GAT_LDS>(c, a);
        if (var & SPH_VAR_GAT_LDS4) return launch_brick_cfg<MODE, CfgG4, SPH_VAR_FORCE_BF | SPH_VAR_DEEP | SPH_VAR_GAT_LDS4>(c, a);
        // the pure-fluid instance of the default force loop, under the rule that admits the density sweep's
        if ((var & (SPH_VAR_FORCE_BF | SPH_VAR_DEEP)) == (SPH_VAR_FORCE_BF | SPH_VAR_DEEP) && sph_pure_fluid_instances(c))
            return launch_brick_cfg<MODE, Cfg0, SPH_VAR_FORCE_BF | SPH_VAR_DEEP | SPH_VAR_PURE_INTERNAL>(c, a);
        switch (var & (SPH_VAR_FORCE_BF | SPH_VAR_DEEP)) {
            case SPH_VAR_FORCE_BF: return launch_brick_cfg<MODE, Cfg0, SPH_VAR_FORCE_BF>(c, a);
            case SPH_VAR_DEEP: return launch_brick_cfg<MODE, Cfg0, SPH_VAR_DEEP>(c, a);
            case SPH_VAR_FORCE_BF | SPH_VAR_DEEP: return launch_brick_cfg<MODE, Cfg0, SPH_VAR_FORCE_BF | SPH_VAR_DEEP>(c, a);
            default: break;
        }
    }
    if constexpr (MODE == GM_FORCE_FUSED) {
        if (var & SPH_VAR_DEEP) return launch_brick_cfg<MODE, Cfg0, SPH_VAR_DEEP>(c, a);
    }
    return launch_brick_cfg<MODE, Cfg0>(c, a);
}

// what a brick sweep that was enqueued without error leaves behind (sph_derived.h)
template <int MODE>
static int sweep_done(SphContext* c, const SweepArgs& a, int rc) {
    if (rc) return rc;
    if (MODE == GM_DENSITY_EOS) sphd_lists_written(c->dv, sphs_uniform(c->ss) ? 1 : 0);
    if (MODE == GM_DF_DENSITY) sphd_lists_written(c->dv, 2);
    if (mode_is_df_vdiv<MODE>() && a.collect_bpart) sphd_bpart_written(c->dv);  // every listed brick leaves its partial of the density error
    if (MODE == GM_DF_DENSITY_CHANGE) sphd_k_written(c->dv, 1);
    if (MODE == GM_DF_DENSITY_ADV) sphd_k_written(c->dv, 2);
    return 0;
}

// force sweep over the targets of x layers [lo, hi) u [lo2, hi2) only (slab mode: boundary layers first, interior later)
int sphk_gather_layers(SphContext* c, int mode, const SweepArgs& args) {
    if (c->N <= 0 || (args.hi <= args.lo && args.hi2 <= args.lo2)) return 0;
    if (c->opt_gather_impl == 1 && !brick_ok(c))
        return sph_fail(c, SPH_E_INVALID, "a slab rank needs the brick sweeps, and this context is beyond their reach (capacity > 16.7 M particles "
                                          "or more than 1000 cell layers in z): cut the domain into more slabs");
    if (mode != GM_FORCE_FUSED || c->opt_gather_impl == 0) return sph_fail(c, SPH_E_INVALID, "layer-restricted sweeps need the brick force kernel");
    if (int rc = sph_ensure_pid(c)) return rc;   // (a slab rank never sorts lean; a context that did and became one gets its aux back)
    SweepArgs a = args;
    if (a.hi < a.lo) a.hi = a.lo;
    if (sphs_uniform(c->ss) && sphd_one_gather_wcsph(c->dv)) return sweep_done<GM_FORCE_FUSED_U>(c, a, launch_brick<GM_FORCE_FUSED_U>(c, a));
    return sweep_done<GM_FORCE_FUSED>(c, a, launch_brick<GM_FORCE_FUSED>(c, a));
}

template <int MODE>
static int launch_sweep(SphContext* c, const SweepArgs& a) {
    if (c->N <= 0) return 0;
    if (c->opt_gather_impl == 0 || !brick_ok(c)) return launch_simple<MODE>(c, nullptr, c->N);
    return sweep_done<MODE>(c, a, launch_brick<MODE>(c, a));
}

// DFSPH sweeps: one brick shape (the lists of GM_DF_DENSITY are read back by every later sweep of the step, so
// writer and readers must agree on it); a list-reading sweep called while the lists are stale (positions moved
// since the density sweep: only possible through the stand-alone API calls) takes the exact cell walk instead.
template <int MODE>
static int launch_df(SphContext* c, const SweepArgs& a) {
    if (c->N <= 0) return 0;
    if (c->opt_gather_impl == 0 || !brick_ok(c) || (mode_reads_list<MODE>() && !sphd_lists_usable(c->dv))) {
        if (mode_is_df_vdiv<MODE>()) sphd_k_written(c->dv, 0);  // density_adv changes, the walk does not refresh k_j
        return launch_simple<MODE>(c, nullptr, c->N);
    }
    // (the group-sorted emission and the early entry loads of SPH_VAR_DEEP do nothing measurable for these sweeps: DFSPH
    // step 3.46 vs 3.51 ms with DEEP, profiles/archive/r02g -- their pair terms gather 4 bytes, not a 16-byte record)
    // (round 6) ... but the list-WRITING sweep of the step is the same filter + emission as the WCSPH density sweep, and the
    // group-sorted emission is worth as much to it: 0.333 -> 0.24 ms on the settled 1.75 M box (tools/list_reuse_probe.py had
    // timed it at the baseline emission's 0.333 against the WCSPH sweep's 0.245)
    if constexpr (MODE == GM_DF_DENSITY) {
        if (c->opt_variant & SPH_VAR_GROUPS) return sweep_done<MODE>(c, a, launch_brick_cfg<MODE, Cfg0, SPH_VAR_GROUPS>(c, a));
    }
    return sweep_done<MODE>(c, a, launch_brick_cfg<MODE, Cfg0>(c, a));
}

static int gather_dispatch(SphContext* c, int mode, const SweepArgs& a);

int sphk_gather(SphContext* c, int mode, const SweepArgs& a) {
    int rc = gather_dispatch(c, mode, a);
    // sweeps that scatter two-way coupling reactions (WCSPH.py:66-68, DFSPH.py:313, 389-390) are followed by the fold
    if (!rc && sph_n_dyn(c) != 0 && (mode == GM_PRESSURE || mode == GM_FORCE_FUSED || mode == GM_DF_DIV_ITER || mode == GM_DF_PRESSURE_ITER))
        rc = sphk_fold_coupling(c);
    return rc;
}

static int gather_dispatch(SphContext* c, int mode, const SweepArgs& a) {
    // ids apart from aux (lean scatter): only the pair of sweeps of the fused uniform-fluid step runs without the record -- the
    // density sweep of the brick path when it writes the staged records (write_sg), the force sweep when it takes its one-gather form
    if (sphd_pid_apart(c->dv)) {
        const bool brick_u = sphs_uniform(c->ss) && c->opt_gather_impl == 1 && brick_ok(c) && c->N > 0;
        const bool alone = (mode == GM_DENSITY_EOS && brick_u) || (mode == GM_FORCE_FUSED && brick_u && sphd_one_gather_wcsph(c->dv));
        if (!alone) { int rc = sph_ensure_aux(c); if (rc) return rc; }
    }
    // every sweep but the fused step's own pair reads or rewrites density / pressure in aux
    if (sphd_aux_in_eos2(c->dv) && mode != GM_DENSITY_EOS && mode != GM_FORCE_FUSED && mode != GM_BVOL_STATIC && mode != GM_BVOL_DYNAMIC) {
        int rc = sph_ensure_aux(c);
        if (rc) return rc;
    }
    switch (mode) {
        case GM_BVOL_STATIC: return launch_simple<GM_BVOL_STATIC>(c, nullptr, c->N);  // init only
        case GM_BVOL_DYNAMIC: {
            if (sph_n_dyn(c) <= 0) return 0;
            DevView d = sph_view(c);
            hipLaunchKernelGGL(k_gather_bvol_split<GM_BVOL_DYNAMIC>, dim3((sph_n_dyn(c) * 16 + TPB - 1) / TPB), dim3(TPB), 0,
                               c->stream, d, c->dyn_list, sph_n_dyn(c));
            SPH_LAUNCH_CHECK(c);
            return 0;
        }
        case GM_DENSITY: return launch_sweep<GM_DENSITY>(c, a);
        case GM_DENSITY_EOS: return launch_sweep<GM_DENSITY_EOS>(c, a);
        case GM_NONPRESSURE: return launch_sweep<GM_NONPRESSURE>(c, a);
        case GM_PRESSURE: return launch_sweep<GM_PRESSURE>(c, a);
        case GM_FORCE_FUSED:
            // one gather per pair when every fluid particle has the same mass (and the density sweep of this step
            // left its stg / gat records): see SPH_OPT_UNIFORM_FLUID
            if (sphs_uniform(c->ss) && c->opt_gather_impl == 1 && brick_ok(c) && sphd_one_gather_wcsph(c->dv) && c->N > 0)
                return sweep_done<GM_FORCE_FUSED_U>(c, a, launch_brick<GM_FORCE_FUSED_U>(c, a));
            return launch_sweep<GM_FORCE_FUSED>(c, a);
        case GM_DF_DENSITY: return launch_df<GM_DF_DENSITY>(c, a);
        case GM_DF_FACTOR: return launch_df<GM_DF_FACTOR>(c, a);
        case GM_DF_DENSITY_CHANGE: return launch_df<GM_DF_DENSITY_CHANGE>(c, a);
        case GM_DF_DENSITY_ADV: return launch_df<GM_DF_DENSITY_ADV>(c, a);
        // Jacobi sweeps: with the lists, the sign-coded staging records and k_j = b_j * factor_j all current (the
        // solver loops inside the library keep them so), the neighbour costs one 4-byte gather instead of two records
        case GM_DF_DIV_ITER:
            if (c->opt_gather_impl == 1 && sphd_one_gather_df(c->dv, 1)) return launch_df<GM_DF_DIV_ITER_U>(c, a);
            return launch_df<GM_DF_DIV_ITER>(c, a);
        case GM_DF_PRESSURE_ITER:
            if (c->opt_gather_impl == 1 && sphd_one_gather_df(c->dv, 2)) return launch_df<GM_DF_PRESSURE_ITER_U>(c, a);
            return launch_df<GM_DF_PRESSURE_ITER>(c, a);
        case GM_DF_NONPRESSURE: return launch_df<GM_DF_NONPRESSURE>(c, a);
    }
    return sph_fail(c, SPH_E_INVALID, "unknown gather mode");
}

// sph_get_stats: what the last density sweep left in gcnt, plus the cell histogram.  Two stages without a single atomic:
// <= 512 workgroups stride over particles and cells and write one row of seven partials each, a 64-lane kernel folds the
// rows (the first version sent seven same-address atomics per wave: 1.05 ms for 1.75 M bytes -- three times the step it
// reports on).
#define SPH_STATS_BLOCKS 512
__global__ __launch_bounds__(TPB) void k_stats(DevView d, const unsigned char* __restrict__ gcnt, unsigned long long* __restrict__ part) {
    __shared__ unsigned long long red[TPB / 64][7];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long tgt = 0, sum = 0, lovf = 0, sovf = 0, ne = 0;
    int mx = 0, occ = 0;
    const int n = max(d.N, d.G);
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        if (gcnt && i < d.N && sph_is_fluid(__float_as_int(d.vf[i].w))) {
            const int c = gcnt[i];
            tgt += 1;
            if (c == SPH_CNT_WALK) sovf += 1;
            else if (c == SPH_CNT_LIST_OVF) lovf += 1;
            else { sum += (unsigned long long)c; mx = max(mx, c); }
        }
        if (i < d.G) {
            const int o = d.cell_end[i] - (i > 0 ? d.cell_end[i - 1] : 0);
            occ = max(occ, o);
            ne += o > 0 ? 1 : 0;
        }
    }
    unsigned long long v[7] = {tgt, sum, (unsigned long long)mx, lovf, sovf, (unsigned long long)occ, ne};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const bool is_max = k == 2 || k == 5;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(v[k], off, 64);
            v[k] = is_max ? max(v[k], o) : v[k] + o;
        }
        if (lane == 0) red[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int k = threadIdx.x;
        unsigned long long t = red[0][k];
        for (int w = 1; w < TPB / 64; ++w) t = (k == 2 || k == 5) ? max(t, red[w][k]) : t + red[w][k];
        part[(size_t)blockIdx.x * 7 + k] = t;
    }
}

__global__ __launch_bounds__(TPB) void k_stats_total(const unsigned long long* __restrict__ part, int nb, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[TPB / 64][7];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long v[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < nb; b += TPB) {  // a thread takes whole rows: the seven loads of a row in flight together
        const unsigned long long* row = part + (size_t)b * 7;
#pragma unroll
        for (int k = 0; k < 7; ++k) v[k] = (k == 2 || k == 5) ? max(v[k], row[k]) : v[k] + row[k];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const bool is_max = k == 2 || k == 5;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(v[k], off, 64);
            v[k] = is_max ? max(v[k], o) : v[k] + o;
        }
        if (lane == 0) red[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int k = threadIdx.x;
        unsigned long long t = red[0][k];
        for (int w = 1; w < TPB / 64; ++w) t = (k == 2 || k == 5) ? max(t, red[w][k]) : t + red[w][k];
        out[k] = t;
    }
}

int sphk_stats(SphContext* c, SphStats* out) {
    memset(out, 0, sizeof(*out));
    if (c->N <= 0) return 0;
    int fb = 0;
    SPH_HIP(c, hipMemcpyAsync(&fb, c->dyn_count + 3, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    DevView d = sph_view(c);
    const int n = max(c->N, c->G);
    int nb = (n + TPB - 1) / TPB;
    if (nb > SPH_STATS_BLOCKS) nb = SPH_STATS_BLOCKS;
    unsigned long long* dev = reinterpret_cast<unsigned long long*>(c->stage);  // 7 totals, then nb rows of 7 partials, in the staging buffer
    unsigned long long* part = dev + 8;
    if ((size_t)(8 + 7 * nb) * sizeof(unsigned long long) > c->stage_bytes) return sph_fail(c, SPH_E_NOMEM, "sph_get_stats: staging buffer too small");
    unsigned long long h[7];
    // (list lengths only if a brick density sweep wrote gcnt for the current order: ADVICE r02 -- otherwise the
    // fields stay 0 instead of showing stale or never-written bytes)
    hipLaunchKernelGGL(k_stats, dim3(nb), dim3(TPB), 0, c->stream, d, sphd_stats_have_lists(c->dv) ? c->gcnt : nullptr, part);
    SPH_LAUNCH_CHECK(c);
    hipLaunchKernelGGL(k_stats_total, dim3(1), dim3(TPB), 0, c->stream, part, nb, dev);
    SPH_LAUNCH_CHECK(c);
    SPH_HIP(c, hipMemcpyAsync(h, dev, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(c, hipStreamSynchronize(c->stream));
    out->targets = (int64_t)h[0]; out->list_entries = (int64_t)h[1]; out->max_list = (int32_t)h[2];
    out->list_overflow_targets = (int32_t)h[3]; out->lds_overflow_targets = (int32_t)h[4];
    out->max_cell_occupancy = (int32_t)h[5]; out->nonempty_cells = (int32_t)h[6];
    out->polar_fallbacks = fb;
    return 0;
}

int sphk_eos(SphContext* c) {
    if (c->N <= 0) return 0;
    DevView d = sph_view(c);
    hipLaunchKernelGGL(k_eos, dim3((c->N + TPB - 1) / TPB), dim3(TPB), 0, c->stream, d);
    SPH_LAUNCH_CHECK(c);
    return 0;
}
