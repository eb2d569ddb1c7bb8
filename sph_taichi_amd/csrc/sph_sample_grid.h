// sph_sample_grid.h -- what another observer may see of the field sampling (sph_sample.hip):
//  * the weight plane of the LAST successful sph_sample_grid of the context and the geometry it was made with.  The mesh extraction
//    (sph_mesh.hip) reads it on the context's stream, behind the scatter that wrote it; nobody else writes it;
//  * the checks of a public SphSampleGrid and the launch of the plain grid scatter into planes of the CALLER's, which the running
//    statistics (sph_stats.hip) take their samples with: one set of checks, one kernel, nothing of SphSample touched.
#pragma once
#include "sph_observe.h"

struct SphSampledGrid {
    const long long* weight;   // [nodes] i64: sum of llrint(w * 2^30); node (k0, k1, k2) at (k0 * n[1] + k1) * n[2] + k2
    long long nodes;
    int n[3];
    float origin[3], spacing[3];
};

// false: nothing has been sampled on a grid yet
bool sph_sample_last_grid(const SphContext* c, SphSampledGrid* out);

struct SampleCommon {
    float inv_h, k_w;
    int fields;               // mask
    int channels;             // 2 + popcount(fields)
    SphSel sel;
};

struct SampleGridDev {
    int n[3];
    float origin[3], spacing[3], inv_spacing[3];
    float h;                  // the radius the footprints are built with: 1 / inv_h
    long long nodes;
    long long* planes;
};

// The checks sph_sample_grid makes of *p (fields, selection, inv_h, node counts, origin, spacing), in its order and with its
// messages under the name `who`; fills *q and all of *g but g->planes.  Allocates nothing, enqueues nothing.
int sph_sample_grid_spec(SphContext* c, const char* who, const SphSampleGrid* p, SampleCommon* q, SampleGridDev* g);
// The plain scatter (k_sample_grid, no gradients) of the live records into g.planes = [q.channels][g.nodes] i64, which the caller
// owns and has cleared; nothing is enqueued for an empty context.  Reads xm / vf, and aux only when q.fields asks for density or
// pressure (the caller then has made it current).
int sph_sample_grid_scatter(SphContext* c, const SampleCommon& q, const SampleGridDev& g);
