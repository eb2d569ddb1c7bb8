// Prints the sizes and offsets of the feature structs of include/sph_hip.h as the host compiler lays them out
// (tests/test_features_host.py compares them with the ctypes mirror and the numpy row type).  Host only: nothing of HIP.
#include <cstddef>
#include <cstdio>

#include "sph_hip.h"

int main() {
    std::printf("SphFeatureParams %zu select %zu every %zu min_neighbours %zu normal_min %zu\n", sizeof(SphFeatureParams),
                offsetof(SphFeatureParams, select), offsetof(SphFeatureParams, every), offsetof(SphFeatureParams, min_neighbours),
                offsetof(SphFeatureParams, normal_min));
    std::printf("SphFeatureRow %zu x %zu vorticity %zu divergence %zu normal %zu fill %zu n_fluid %zu n_solid %zu flags %zu reserved_ %zu\n",
                sizeof(SphFeatureRow), offsetof(SphFeatureRow, x), offsetof(SphFeatureRow, vorticity), offsetof(SphFeatureRow, divergence),
                offsetof(SphFeatureRow, normal), offsetof(SphFeatureRow, fill), offsetof(SphFeatureRow, n_fluid), offsetof(SphFeatureRow, n_solid),
                offsetof(SphFeatureRow, flags), offsetof(SphFeatureRow, reserved_));
    std::printf("SphFeatureInfo %zu every %zu reserved_ %zu rows %zu samples %zu steps_seen %zu step %zu time %zu\n", sizeof(SphFeatureInfo),
                offsetof(SphFeatureInfo, every), offsetof(SphFeatureInfo, reserved_), offsetof(SphFeatureInfo, rows), offsetof(SphFeatureInfo, samples),
                offsetof(SphFeatureInfo, steps_seen), offsetof(SphFeatureInfo, step), offsetof(SphFeatureInfo, time));
    std::printf("SPH_FEATURES_SCALE_LOG2 %d\nSPH_FEATURES_FILL_SCALE_LOG2 %d\nSPH_FEATURE_FLAGS %d %d %d\nSPH_FEATURE_FIELDS %d\nSPH_ABI_VERSION %d\n",
                SPH_FEATURES_SCALE_LOG2, SPH_FEATURES_FILL_SCALE_LOG2, SPH_FEATURE_VALID, SPH_FEATURE_SURFACE, SPH_FEATURE_SATURATED,
                (int)SPH_FEATURE_FIELDS, SPH_ABI_VERSION);
    return 0;
}
