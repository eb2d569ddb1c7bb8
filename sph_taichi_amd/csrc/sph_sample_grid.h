// sph_sample_grid.h -- what another observer may see of the field sampling (sph_sample.hip): the weight plane of the LAST successful
// sph_sample_grid of the context and the geometry it was made with.  The mesh extraction (sph_mesh.hip) reads it on the context's
// stream, behind the scatter that wrote it; nobody else writes it.
#pragma once
#include "sph_internal.h"

struct SphSampledGrid {
    const long long* weight;   // [nodes] i64: sum of llrint(w * 2^30); node (k0, k1, k2) at (k0 * n[1] + k1) * n[2] + k2
    long long nodes;
    int n[3];
    float origin[3], spacing[3];
};

// false: nothing has been sampled on a grid yet
bool sph_sample_last_grid(const SphContext* c, SphSampledGrid* out);
