// Prints the sizes and offsets of the load structs of include/sph_hip.h as the host compiler lays them out
// (tests/test_loads_host.py compares them with the ctypes mirror).  Host only: nothing of HIP.
#include <cstddef>
#include <cstdio>

#include "sph_hip.h"

int main() {
    std::printf("SphLoadParams %zu object_ids %zu n_objects %zu about %zu every %zu capacity %zu\n", sizeof(SphLoadParams),
                offsetof(SphLoadParams, object_ids), offsetof(SphLoadParams, n_objects), offsetof(SphLoadParams, about),
                offsetof(SphLoadParams, every), offsetof(SphLoadParams, capacity));
    std::printf("SphLoadInfo %zu n_objects %zu every %zu samples %zu dropped %zu steps_seen %zu\n", sizeof(SphLoadInfo),
                offsetof(SphLoadInfo, n_objects), offsetof(SphLoadInfo, every), offsetof(SphLoadInfo, samples), offsetof(SphLoadInfo, dropped),
                offsetof(SphLoadInfo, steps_seen));
    std::printf("SPH_LOADS_MAX_OBJECTS %d\nSPH_LOADS_ROW_WORDS %d\nSPH_LOADS_SCALE_LOG2 %d\nSPH_ABI_VERSION %d\n", SPH_LOADS_MAX_OBJECTS,
                SPH_LOADS_ROW_WORDS, SPH_LOADS_SCALE_LOG2, SPH_ABI_VERSION);
    return 0;
}
