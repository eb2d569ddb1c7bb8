// sph_mesh.hip -- the fluid surface as a triangle mesh (include/sph_hip.h, "Surface mesh"): surface nets on the weight plane that the
// LAST sph_sample_grid left on the device.  One vertex per mixed cell, one quad (two triangles) per sign-changing grid edge whose four
// cells exist.  Reads the sampler's weight plane, writes buffers of its own and no particle state; the sort, the sweeps and the
// sampler's planes are not touched.
//
// Everything is a function of the integer plane and (iso, cap): inside / outside is an i64 compare, the numbering is a rank in
// ascending linear index, so counts, positions, normals and the index buffer do not depend on scheduling.  No atomics anywhere.
//
// One thread per NODE, 256 consecutive linear nodes (k2 fastest) per workgroup; node L handles the cell whose low corner it is and
// the three edges L -> L + e_a it owns.  Four launches, each reading what the previous one wrote -- no workgroup waits for another:
//   k_mesh_classify : the 8 corners of the node's cell -> one flag byte per node (cell active; per owned edge: emits a quad, its
//                     low end is inside) and the block's (vertex, quad) counts
//   k_mesh_scan     : ONE workgroup scans the block counts exclusively, MESH_SCAN_CHUNK = 1024 blocks per trip (four per thread,
//                     wave64 shuffle scan, the four waves' totals through LDS) with the running totals carried along; writes (V, Q)
//   (the host reads V and Q here -- the one synchronisation of an extract -- and grows the mesh's buffers if they are short)
//   k_mesh_vertices : rank of an active cell = block offset + the earlier waves' counts + the lanes below; position and normal go
//                     to that rank, the rank to vmap[L]
//   k_mesh_faces    : launched separately because it needs the complete map: rank of a node's first quad likewise (the key 3 L + a
//                     ascends with the lane, then with a); the four cells round the edge are vmap[L - s_b - s_c], [L - s_c], [L],
//                     [L - s_b] with s the nodes' linear strides
// The later passes read the flag byte (1 B per node), not the plane again; only active cells reload their 8 corners.
//
// WHERE THE CORNERS COME FROM: no LDS tile; L2 serves the reuse.  A wave's 8 corner loads are four row segments of 64 * 8 B (rows L,
// L + n2, L + n1 n2, L + n1 n2 + n2), each read twice one node apart -- coalesced, 2 of 8 from the same lines in L1.  A node's weight is
// wanted by 8 cells that lie at most one k0-plane apart, n1 * n2 * 8 B: 197 KB on the 157^3 grid of the timing profile, 2 MB at the
// largest square plane a 2^24-node grid can have with n0 = 2 (then nothing is re-read across planes at all), against 4 MiB of L2 per XCD.
// Workgroups are dealt round-robin to the 8 XCDs, so each L2 fetches the rows its own blocks touch (up to 4 x a block's own 2 KB) from
// the Infinity Cache, which holds the whole plane (at most 128 MiB) behind the scatter that has just written it: HBM sees each
// weight once.  The L2 -> CU traffic is 64 B per node, 250 MB on 3.9 M nodes: some ten microseconds at the L2's rate.  An LDS tile
// would cut those 64 B to about 12, of a pass that is bound by neither.
#include <cmath>
#include "sph_observe.h"
#include "sph_sample_grid.h"

#pragma clang fp contract(off)

#define MTPB 256
#define MWAVES (MTPB / 64)
#define MESH_SCAN_CHUNK (4 * MTPB)   // block counts per trip of k_mesh_scan
#define MF_ACTIVE 1u                 // the cell whose low corner the node is holds a vertex
#define MF_EMIT(a) (2u << (a))       // the owned edge along a emits a quad
#define MF_LO_IN(a) (16u << (a))     // ... and its low end is the inside one

struct SphMesh {
    void* scratch;            // one allocation: vmap i32 [nodes], block_count int2 [blocks], block_offset int2 [blocks], totals i32 [2], flags u8 [nodes]
    long long scratch_nodes;  // nodes the allocation holds
    float* verts;             // positions [vert_cap][3], then normals [vert_cap][3]
    long long vert_cap;
    int* tris;                // [tri_cap][3]
    long long tri_cap;
    long long V, T;           // of the last extract
    bool have;
};

struct MeshGrid {
    int n[3];
    int cap;
    long long T;              // the threshold: a node is inside iff phi >= T
    long long nodes;
    float origin[3], spacing[3];
};

struct MeshScratch { int* vmap; int2* block_count; int2* block_offset; int* totals; unsigned char* flags; };

static inline MeshScratch mesh_scratch(void* base, long long nodes) {
    const long long blocks = (nodes + MTPB - 1) / MTPB;
    MeshScratch s;
    s.vmap = (int*)base;
    s.block_count = (int2*)(s.vmap + ((nodes + 1) & ~1ll));   // (8-byte aligned)
    s.block_offset = s.block_count + blocks;
    s.totals = (int*)(s.block_offset + blocks);
    s.flags = (unsigned char*)(s.totals + 2);
    return s;
}
static inline size_t mesh_scratch_bytes(long long nodes) {
    const long long blocks = (nodes + MTPB - 1) / MTPB;
    return (size_t)((nodes + 1) & ~1ll) * 4 + (size_t)blocks * 16 + 8 + (size_t)nodes;
}

// the capped field at node (k0, k1, k2); 0 beyond the grid (such a corner belongs to no cell and no edge that is used)
__device__ __forceinline__ long long mesh_phi(const long long* __restrict__ w, const MeshGrid& g, int k0, int k1, int k2) {
    if (k0 >= g.n[0] || k1 >= g.n[1] || k2 >= g.n[2]) return 0;
    if (g.cap && (k0 == 0 || k0 == g.n[0] - 1 || k1 == 0 || k1 == g.n[1] - 1 || k2 == 0 || k2 == g.n[2] - 1)) return 0;
    return w[((size_t)k0 * g.n[1] + k1) * g.n[2] + k2];
}

// corner (i0, i1, i2) of the cell is phi[4 i0 + 2 i1 + i2]
__device__ __forceinline__ void mesh_corners(const long long* __restrict__ w, const MeshGrid& g, int k0, int k1, int k2, long long phi[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) phi[j] = mesh_phi(w, g, k0 + (j >> 2), k1 + ((j >> 1) & 1), k2 + (j & 1));
}

__device__ __forceinline__ void mesh_node(int L, const MeshGrid& g, int& k0, int& k1, int& k2) {
    k2 = L % g.n[2];
    const int rest = L / g.n[2];
    k1 = rest % g.n[1];
    k0 = rest / g.n[1];
}

// exclusive rank of this thread's count `v` among the block's, and the block's total; `wave_total` is MWAVES ints of LDS
__device__ __forceinline__ int mesh_block_rank(int v, int* wave_total, int& block_total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = sph_wave_inclusive_scan(v, lane);
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int before = 0;
    block_total = 0;
#pragma unroll
    for (int w = 0; w < MWAVES; ++w) {
        const int t = wave_total[w];
        if (w < wave) before += t;
        block_total += t;
    }
    return before + incl - v;
}

__global__ __launch_bounds__(MTPB) void k_mesh_classify(const long long* __restrict__ w, MeshGrid g, unsigned char* __restrict__ flags,
                                                        int2* __restrict__ block_count) {
    __shared__ int wave_v[MWAVES], wave_q[MWAVES];
    const long long L = (long long)blockIdx.x * MTPB + threadIdx.x;
    unsigned f = 0u;
    if (L < g.nodes) {
        int k[3];
        mesh_node((int)L, g, k[0], k[1], k[2]);
        long long phi[8];
        mesh_corners(w, g, k[0], k[1], k[2], phi);
        unsigned in = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) in |= (phi[j] >= g.T ? 1u : 0u) << j;
        const bool has_hi[3] = {k[0] <= g.n[0] - 2, k[1] <= g.n[1] - 2, k[2] <= g.n[2] - 2};
        const bool interior[3] = {k[0] >= 1 && has_hi[0], k[1] >= 1 && has_hi[1], k[2] >= 1 && has_hi[2]};
        if (has_hi[0] && has_hi[1] && has_hi[2] && in != 0u && in != 0xFFu) f |= MF_ACTIVE;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            const unsigned lo_in = in & 1u, hi_in = (in >> (4 >> a)) & 1u;
            if (lo_in != hi_in && has_hi[a] && interior[b] && interior[c]) f |= MF_EMIT(a) | (lo_in ? MF_LO_IN(a) : 0u);
        }
        flags[L] = (unsigned char)f;
    }
    int total_v, total_q;
    mesh_block_rank((int)(f & MF_ACTIVE), wave_v, total_v);
    mesh_block_rank(__popc(f & (MF_EMIT(0) | MF_EMIT(1) | MF_EMIT(2))), wave_q, total_q);
    if (threadIdx.x == 0) block_count[blockIdx.x] = make_int2(total_v, total_q);
}

// ONE workgroup: exclusive scan of the block counts, MESH_SCAN_CHUNK per trip; thread t holds counts [4 t, 4 t + 4) of the chunk
__global__ __launch_bounds__(MTPB) void k_mesh_scan(const int2* __restrict__ block_count, int blocks, int2* __restrict__ block_offset,
                                                    int* __restrict__ totals) {
    __shared__ int wave_v[MWAVES], wave_q[MWAVES];
    int run_v = 0, run_q = 0;   // block-uniform
    for (int base = 0; base < blocks; base += MESH_SCAN_CHUNK) {
        int2 c[4];
        int sv = 0, sq = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = base + 4 * (int)threadIdx.x + j;
            c[j] = b < blocks ? block_count[b] : make_int2(0, 0);
            sv += c[j].x; sq += c[j].y;
        }
        int total_v, total_q;
        int v = run_v + mesh_block_rank(sv, wave_v, total_v);
        int q = run_q + mesh_block_rank(sq, wave_q, total_q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = base + 4 * (int)threadIdx.x + j;
            if (b < blocks) block_offset[b] = make_int2(v, q);
            v += c[j].x; q += c[j].y;
        }
        run_v += total_v; run_q += total_q;
        __syncthreads();   // the wave totals are written again by the next trip
    }
    if (threadIdx.x == 0) { totals[0] = run_v; totals[1] = run_q; }
}

// pos / nrm hold V rows; a rank is below V by construction (the same flags gave the counts) and is checked all the same
__global__ __launch_bounds__(MTPB) void k_mesh_vertices(const long long* __restrict__ w, MeshGrid g, const unsigned char* __restrict__ flags,
                                                        const int2* __restrict__ block_offset, int V, int* __restrict__ vmap,
                                                        float* __restrict__ pos, float* __restrict__ nrm) {
    __shared__ int wave_v[MWAVES];
    const long long L = (long long)blockIdx.x * MTPB + threadIdx.x;
    const bool active = L < g.nodes && (flags[L] & MF_ACTIVE);
    int total;
    const int rank = block_offset[blockIdx.x].x + mesh_block_rank(active ? 1 : 0, wave_v, total);
    if (!active || rank >= V) return;
    int k[3];
    mesh_node((int)L, g, k[0], k[1], k[2]);
    long long phi[8];
    mesh_corners(w, g, k[0], k[1], k[2], phi);
    double sum[3] = {0.0, 0.0, 0.0};
    long long grad[3] = {0, 0, 0};
    int m = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;   // the other two axes, b < c
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ib = e & 1, ic = e >> 1;
            const int lo = ib * (4 >> b) + ic * (4 >> c), hi = lo + (4 >> a);
            const long long d = phi[hi] - phi[lo];
            grad[a] += d;
            if ((phi[lo] >= g.T) != (phi[hi] >= g.T)) {
                const double t = (double)(g.T - phi[lo]) / (double)d;
                sum[a] += t; sum[b] += (double)ib; sum[c] += (double)ic;
                ++m;
            }
        }
    }
    const double gd0 = (double)grad[0], gd1 = (double)grad[1], gd2 = (double)grad[2];
    const double s = (gd0 * gd0 + gd1 * gd1) + gd2 * gd2;
    const double root = sqrt(s);
    const double gd[3] = {gd0, gd1, gd2};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float u = (float)(sum[a] / (double)m);   // m >= 1: an active cell has a crossing edge
        pos[3 * (size_t)rank + a] = g.origin[a] + ((float)k[a] + u) * g.spacing[a];
        nrm[3 * (size_t)rank + a] = s == 0.0 ? 0.f : (float)(-gd[a] / root);
    }
    vmap[L] = rank;
}

// tri holds Q quads of six indices; a rank is below Q by construction and is checked all the same.  An emitting edge has
// k_b, k_c >= 1, so the four map entries lie inside the plane, and they were written: the four cells round a crossing edge are active.
__global__ __launch_bounds__(MTPB) void k_mesh_faces(MeshGrid g, const unsigned char* __restrict__ flags, const int2* __restrict__ block_offset,
                                                     int Q, const int* __restrict__ vmap, int* __restrict__ tri) {
    __shared__ int wave_q[MWAVES];
    const long long L = (long long)blockIdx.x * MTPB + threadIdx.x;
    const unsigned f = L < g.nodes ? flags[L] : 0u;
    int total;
    int q = block_offset[blockIdx.x].y + mesh_block_rank(__popc(f & (MF_EMIT(0) | MF_EMIT(1) | MF_EMIT(2))), wave_q, total);
    const long long stride[3] = {(long long)g.n[1] * g.n[2], (long long)g.n[2], 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(f & MF_EMIT(a))) continue;
        if (q >= Q) return;
        const long long sb = stride[(a + 1) % 3], sc = stride[(a + 2) % 3];
        const int c0 = vmap[L - sb - sc], c1 = vmap[L - sc], c2 = vmap[L], c3 = vmap[L - sb];
        int* t = tri + 6 * (size_t)q;
        t[0] = c0; t[3] = c0; t[4] = c2;
        if (f & MF_LO_IN(a)) { t[1] = c1; t[2] = c2; t[5] = c3; }
        else                 { t[1] = c3; t[2] = c2; t[5] = c1; }
        ++q;
    }
}

void sph_mesh_release(SphContext* c) { sph_observe_release(c->mesh, &SphMesh::scratch, &SphMesh::verts, &SphMesh::tris); }

static int mesh_fetch(SphContext* c, const char* who, const SphMesh*& m) {
    m = c->mesh;
    if (m && m->have) return 0;
    snprintf(c->err, sizeof(c->err), "%s: no mesh has been extracted (call sph_mesh_extract first)", who);
    return SPH_E_STATE;
}

extern "C" {

int32_t sph_mesh_extract(SphContext* c, const SphMeshSpec* p) {
    static const char* who = "sph_mesh_extract";
    if (c && !p) return sph_fail(c, SPH_E_INVALID, "sph_mesh_extract: the spec is NULL");
    if (int rc = sph_observe_enter(c, who, " (the grid it would read cannot have been sampled there); meshes are extracted on single-domain contexts only")) return rc;
    if (!std::isfinite(p->iso) || !(p->iso > 0.f) || p->iso > 4.f) {
        snprintf(c->err, sizeof(c->err), "sph_mesh_extract: iso = %g, must be finite and in (0, 4]", (double)p->iso);
        return SPH_E_INVALID;
    }
    SphSampledGrid in;
    if (!sph_sample_last_grid(c, &in)) return sph_fail(c, SPH_E_STATE, "sph_mesh_extract: no grid has been sampled (call sph_sample_grid first)");
    MeshGrid g;
    for (int a = 0; a < 3; ++a) {
        if (in.n[a] < 2) {
            snprintf(c->err, sizeof(c->err), "sph_mesh_extract: the sampled grid has %d x %d x %d nodes, a mesh needs at least 2 per axis", in.n[0], in.n[1], in.n[2]);
            return SPH_E_INVALID;
        }
        g.n[a] = in.n[a]; g.origin[a] = in.origin[a]; g.spacing[a] = in.spacing[a];
    }
    g.cap = p->cap != 0;
    g.T = llrint((double)p->iso * (double)(1 << SPH_SAMPLE_SCALE_LOG2));
    g.nodes = in.nodes;   // <= SPH_SAMPLE_MAX_NODES = 2^24: every linear index and every count below fits an int
    SphMesh* m = sph_observe_state(c->mesh);
    if (!m) return sph_fail(c, SPH_E_NOMEM, "sph_mesh_extract: out of host memory");
    if (g.nodes > m->scratch_nodes) {
        m->scratch_nodes = 0;
        if (int rc = sph_observe_alloc(c, &m->scratch, mesh_scratch_bytes(g.nodes), who, "the flags, the vertex map and the block counts")) return rc;
        m->scratch_nodes = g.nodes;
    }
    const MeshScratch s = mesh_scratch(m->scratch, g.nodes);
    const int blocks = (int)((g.nodes + MTPB - 1) / MTPB);
    m->have = false;   // from here on the last mesh is being replaced
    hipLaunchKernelGGL(k_mesh_classify, dim3(blocks), dim3(MTPB), 0, c->stream, in.weight, g, s.flags, s.block_count);
    SPH_LAUNCH_CHECK(c);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MTPB), 0, c->stream, s.block_count, blocks, s.block_offset, s.totals);
    SPH_LAUNCH_CHECK(c);
    int totals[2] = {0, 0};
    if (int rc = sph_observe_download(c, totals, s.totals, sizeof(totals))) return rc;
    const long long V = totals[0], Q = totals[1];
    if (V > m->vert_cap) {
        m->vert_cap = 0;
        if (int rc = sph_observe_alloc(c, (void**)&m->verts, (size_t)V * 24, who, "the vertices")) return rc;
        m->vert_cap = V;
    }
    if (2 * Q > m->tri_cap) {
        m->tri_cap = 0;
        if (int rc = sph_observe_alloc(c, (void**)&m->tris, (size_t)Q * 24, who, "the triangles")) return rc;
        m->tri_cap = 2 * Q;
    }
    if (V > 0) {
        hipLaunchKernelGGL(k_mesh_vertices, dim3(blocks), dim3(MTPB), 0, c->stream, in.weight, g, s.flags, s.block_offset, (int)V, s.vmap,
                           m->verts, m->verts + 3 * (size_t)m->vert_cap);
        SPH_LAUNCH_CHECK(c);
    }
    if (Q > 0) {
        hipLaunchKernelGGL(k_mesh_faces, dim3(blocks), dim3(MTPB), 0, c->stream, g, s.flags, s.block_offset, (int)Q, s.vmap, m->tris);
        SPH_LAUNCH_CHECK(c);
    }
    m->V = V;
    m->T = 2 * Q;
    m->have = true;
    return 0;
}

int32_t sph_mesh_counts(SphContext* c, int64_t* vertices, int64_t* triangles) {
    if (!c) return SPH_E_INVALID;
    const SphMesh* m;
    if (int rc = mesh_fetch(c, "sph_mesh_counts", m)) return rc;
    if (vertices) *vertices = m->V;
    if (triangles) *triangles = m->T;
    return 0;
}

int32_t sph_mesh_download(SphContext* c, float* pos, float* nrm, int32_t* tri, int64_t vertices, int64_t triangles) {
    if (!c) return SPH_E_INVALID;
    const SphMesh* m;
    if (int rc = mesh_fetch(c, "sph_mesh_download", m)) return rc;
    if (vertices != m->V || triangles != m->T) {
        snprintf(c->err, sizeof(c->err), "sph_mesh_download: vertices = %lld, triangles = %lld, the last extract made %lld vertices and %lld triangles",
                 (long long)vertices, (long long)triangles, m->V, m->T);
        return SPH_E_INVALID;
    }
    SPH_HIP(c, hipSetDevice(c->device));
    if (pos && m->V > 0) SPH_HIP(c, hipMemcpyAsync(pos, m->verts, (size_t)m->V * 12, hipMemcpyDeviceToHost, c->stream));
    if (nrm && m->V > 0) SPH_HIP(c, hipMemcpyAsync(nrm, m->verts + 3 * (size_t)m->vert_cap, (size_t)m->V * 12, hipMemcpyDeviceToHost, c->stream));
    if (tri && m->T > 0) SPH_HIP(c, hipMemcpyAsync(tri, m->tris, (size_t)m->T * 12, hipMemcpyDeviceToHost, c->stream));
    return sph_observe_download(c, nullptr, nullptr, 0);
}

}  // extern "C"
