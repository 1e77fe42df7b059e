// rt_stats_merge.h -- the rt_stats of a frame from the rt_stats of its shards.  Host only, nothing of HIP: the library merges
// with it (rt_host_frame.inc) and librt_hostcheck.so exports it to the CPU tests (tests/test_stats_merge_host.py).
#ifndef RT_STATS_MERGE_H
#define RT_STATS_MERGE_H

#include <algorithm>

#include "../../include/rtcuda_amd.h"

// sub[0 .. n-1] (n >= 1), in shard order.  sub_shards: the shards were sub-shards of ONE shard on one device (RT_SPLIT);
// otherwise they were device shards (rt_render_multi).
//
//   field                                                            sub-shards   device shards
//   the seven event counts, launches_trace, reserved[4..6]           sum          sum
//   seconds_render, seconds_rng_init, seconds_reference_tree         max          max
//   iterations, seconds_trace, seconds_advance                       sum          max
//   reserved[0] (launches the event timer sampled)                   sum          shard 0's
//   reserved[2] (node records k_paths staged in LDS)                 max          shard 0's
//   bvh_nodes, bvh_depth, reserved[1]                                shard 0's    shard 0's
//   reserved[3] (device shards behind the totals)                    shard 0's    n
static inline rt_stats merge_shard_stats(const rt_stats *sub, int n, bool sub_shards) {  // (static: no library exports it)
    rt_stats tot = sub[0];  // one scene, one launch plan: bvh_nodes, bvh_depth and reserved[1] are every shard's
    for (int k = 1; k < n; k++) {
        const rt_stats &s = sub[k];
        // work that was done, whoever did it
        tot.camera_rays += s.camera_rays;
        tot.shade_events += s.shade_events;
        tot.closest_rays += s.closest_rays;
        tot.any_rays += s.any_rays;
        tot.emission_adds += s.emission_adds;
        tot.shadow_adds += s.shadow_adds;
        tot.rr_draws += s.rr_draws;
        tot.launches_trace += s.launches_trace;
        for (int q = 4; q < 7; q++) tot.reserved[q] += s.reserved[q];
        // spans between two events of a shard's own stream, and one-offs: the shards' host threads run side by side
        tot.seconds_render = std::max(tot.seconds_render, s.seconds_render);
        tot.seconds_rng_init = std::max(tot.seconds_rng_init, s.seconds_rng_init);
        tot.seconds_reference_tree = std::max(tot.seconds_reference_tree, s.seconds_reference_tree);
        if (sub_shards) {
            // sub-shards of one device queue on the same hardware: their rounds and their kernel times add up to the device's
            tot.iterations += s.iterations;
            tot.seconds_trace += s.seconds_trace;
            tot.seconds_advance += s.seconds_advance;
            tot.reserved[0] += s.reserved[0];  // (counted like the rounds it samples)
            tot.reserved[2] = std::max(tot.reserved[2], s.reserved[2]);
        } else {
            // device shards run side by side on hardware of their own: the frame took the longest one's rounds and kernel times
            tot.iterations = std::max(tot.iterations, s.iterations);
            tot.seconds_trace = std::max(tot.seconds_trace, s.seconds_trace);
            tot.seconds_advance = std::max(tot.seconds_advance, s.seconds_advance);
            // reserved[0] and reserved[2] stay shard 0's.  The code gives no reason why they are not merged as above (equal
            // shards report equal values in reserved[2]; reserved[0] would follow iterations): kept as it has always been.
        }
    }
    if (!sub_shards) tot.reserved[3] = n;
    return tot;
}

#endif
