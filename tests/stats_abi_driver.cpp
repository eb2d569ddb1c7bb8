// Prints the sizes and offsets of the statistics structs of include/sph_hip.h as the host compiler lays them out
// (tests/test_stats_host.py compares them with the ctypes mirror).  Host only: nothing of HIP.
#include <cstddef>
#include <cstdio>

#include "sph_hip.h"

int main() {
    std::printf("SphSampleGrid %zu\n", sizeof(SphSampleGrid));
    std::printf("SphStatsParams %zu every %zu capacity %zu wet_min %zu\n", sizeof(SphStatsParams), offsetof(SphStatsParams, every),
                offsetof(SphStatsParams, capacity), offsetof(SphStatsParams, wet_min));
    std::printf("SphStatsInfo %zu n %zu every %zu samples %zu dropped %zu steps_seen %zu t_first %zu t_last %zu\n", sizeof(SphStatsInfo),
                offsetof(SphStatsInfo, n), offsetof(SphStatsInfo, every), offsetof(SphStatsInfo, samples), offsetof(SphStatsInfo, dropped),
                offsetof(SphStatsInfo, steps_seen), offsetof(SphStatsInfo, t_first), offsetof(SphStatsInfo, t_last));
    std::printf("SPH_STATS_MAX_SAMPLES %d\n", SPH_STATS_MAX_SAMPLES);
    return 0;
}
