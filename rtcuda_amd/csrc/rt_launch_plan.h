// rt_launch_plan.h -- the launch geometry of the persistent frame kernels (k_paths / k_paths<PathsRays> / k_paths<PathsKeyed>) as a pure
// function of plain numbers and the experiment knobs (rt_bvh.h): no HIP state is touched, so what the measured speed of a
// frame rests on -- every number in the comments is a measurement -- is tested on a CPU (rt_host_check.cpp exports it).
#pragma once

#include <algorithm>
#include <cstdlib>

#include "rt_bvh.h"

namespace rtplan {
constexpr int kBlock = 256, kSlots = 1 << 20;  // lanes of a workgroup, RT_NUM_WORKING_PATHS (rtcuda_amd.hip asserts both)

struct PathsLaunch {
    int blocks;        // workgroups of the one launch
    bool few_blocks;   // at most 2 per CU: the 2-waves-per-SIMD builds
    size_t lds_bytes;  // dynamic LDS of a workgroup
    int top_n, adv_batch, gen_batch, tri_follow, prio_rotate, rot_wave, rot_set;  // (see where they are set)
    int slot_chunk;    // camera rays per task of the chunked deal (rt_slot_chunks.h); 0: the static deal; kSlotChunkAuto: by the
                       // length of the frame's chains (slot_chunk_for)
    int slot_head;     // slot sets a lane runs as the static deal does before the deal begins; kSlotHeadAuto: slot_head_for's default
};
// The hand-over costs the same per chunk whatever the frame, and what it buys -- the spread of the lanes' totals -- shrinks
// relative to a lane's work as the chains get longer: the best chunk grows with the chain, kChunksPerSlot tasks per slot (the
// sweeps on 506-, 1 012- and 2 025-ray chains: profiles/slot_chunks.md).  It wins 3 % at 506 rays, 0.6 % at 1 012 -- less than
// what the kernel with the deal compiled in loses to the plain one on its common path -- and nothing at 2 025; chunks below
// 48 rays put a hand-over into nearly every GEN block.  So by default the deal is used around the one chain length at which
// it was timed, 506 rays: chains of kChunkChainLo .. kChunkChainHi rays (G = 48 .. 96), and every other frame runs the plain
// kernel.  The two edges are NOT measured: they are the range of G that was flat at 506 rays (48 .. 96) turned into chain
// lengths at 8 tasks per slot; the gain must fall to the loss seen at 1 012 rays somewhere above 506, possibly before 768.
constexpr int kSlotChunkAuto = -1, kChunksPerSlot = 8, kChunkChainLo = 384, kChunkChainHi = 768;
// A lane's totals differ from its neighbours' only at the end, and a hand-over balances something only while a lane has at
// least two dealt slots: the last kDealtSetsDefault sets are dealt, the sets before them run as in the static deal (half the
// hand-overs of a full pool's frame; the 2-shard frame, two sets, is dealt whole).  The workgroup's semaphores (2 KB of static
// LDS in k_paths<PathsChunked>, rtchunks::kSemWords) hold kDealtSetsMax dealt sets; with them a workgroup must still be one of
// kChunkWorkgroupsPerCu on its CU, or the frame keeps the static deal (slot_chunk_if_resident).
constexpr int kSlotHeadAuto = -1, kDealtSetsDefault = 2, kDealtSetsMax = 4, kChunkWorkgroupsPerCu = 4;
// G (at most 2^20) and the head reach the kernel in one int: the head above G's kChunkHeadShift bits, so at most kChunkSetsMax sets
constexpr int kChunkHeadShift = 21, kChunkSetsMax = 1 << (31 - kChunkHeadShift);

// `n`: slots of the shard; `paths_cap`: stack entries of a lane kept in LDS; `lattice`: the rays follow the camera's pixel
// lattice (not a table's); `fixed_lds_bytes`: the shading tables (if staged in LDS) + the camera + the frame's parameters.
inline PathsLaunch plan_paths_launch(int n, int cus, bool wide, int n_nodes, int paths_cap, bool lattice, int width, int spp,
                                     size_t fixed_lds_bytes) {
    using rtbvh::knob;
    PathsLaunch p{};
    p.lds_bytes = sizeof(int) * (size_t)kBlock * (size_t)(paths_cap + 26) + fixed_lds_bytes;
    // all workgroups resident at once (4 per CU at <= 128 VGPRs), lane count a divisor of n
    p.blocks = (n + kBlock - 1) / kBlock;
    {
        int want = 1024;
        if (const char *e = knob("RT_PATHS_BLOCKS")) want = std::max(1, atoi(e));
        while (p.blocks > want && p.blocks % 2 == 0) p.blocks /= 2;
    }
    p.few_blocks = p.blocks <= 2 * cus;
    if (p.few_blocks) {
        // records of the top of the tree kept in LDS (within the 64 KB of dynamic LDS a launch gets without further
        // ado, ~36 KB of it slot state): 384 records of the binary tree.  For the 4-wide tree the copy buys nothing
        // (1/8 shard of C2: 2 013 / 2 017 / 2 016 / 2 015 Msamples/s with 0 / 64 / 128 / 224 nodes in LDS -- the
        // first levels are L2 hits the two waves' other work hides), so it is off unless RT_TOP_NODES asks for it
        const int prefix = std::min(n_nodes, (int)rtbvh::kTopPrefix * (wide ? 2 : 1));
        int top_n = std::min(wide ? 0 : 384, prefix);
        if (const char *e = knob("RT_TOP_NODES")) top_n = std::max(0, std::min(std::min(768, atoi(e)), prefix));
        if (wide) top_n &= ~1;  // whole nodes
        // (never more than the 64 KB of dynamic LDS a launch gets without further ado: scenes with many materials / lights
        // have larger tables)
        const size_t room = p.lds_bytes < 65536 ? (65536 - p.lds_bytes) / 64 : 0;
        p.top_n = (int)std::min<size_t>((size_t)top_n, room) & (wide ? ~1 : ~0);
        p.lds_bytes += (size_t)p.top_n * 64;
    }
    // lanes waiting for the ADV block before it runs: full pool flat 16..24 (round 3, with the triangle block behind the
    // node block and no trip through the loop head after ADV / GEN: 20 and GEN 6 are 1 % ahead of 24 and 8); the
    // 2-waves-per-SIMD shards want 30..38 (24: -2.5 %)
    p.adv_batch = p.few_blocks ? 34 : 20;
    p.gen_batch = 6;  // lanes waiting for the GEN block before it runs (unless nothing else can); flat 4..8
    if (const char *e = knob("RT_ADV_BATCH")) p.adv_batch = std::max(1, std::min(64, atoi(e)));
    if (const char *e = knob("RT_GEN_BATCH")) p.gen_batch = std::max(1, std::min(64, atoi(e)));
    p.tri_follow = 1;  // a triangle block right behind a node block when this many lanes hold a leaf by then; 0 = never
    if (const char *e = knob("RT_TRI_FOLLOW")) p.tri_follow = std::max(0, std::min(64, atoi(e)));
    // log2 of the priority-rotation period in scheduling decisions; 0 = off (128 ms for C2's frame).  Full pool: 111.7 - 112.2 /
    // 111.8 / 111.9 / 112.1 / 112.5 ms at 4 / 5 / 6 / 7 / 8 (late round 5; C3 -0.9 % at 4, C4 flat); 1/8 shards want 8 (+1 % at 4)
    p.prio_rotate = p.few_blocks ? 8 : 5;
    // period, in 64-slot blocks, after which slots repeat the same pixel-column lattice (see k_paths)
    {
        long long period = 0;
        if (lattice && spp % 64 == 0 && kSlots % spp == 0) {  // (a table's rays follow no pixel lattice: the fallback below)
            const long long step = (kSlots / spp) % width;  // columns a slot moves per generation
            long long a = step, b = width;
            while (b) { long long t = a % b; a = b; b = t; }
            period = a * (spp / 64);  // gcd(step, width) columns x blocks per pixel
        }
        const int waves = p.blocks * (kBlock / 64);
        if (period < 16 || period > waves) period = std::max(16, waves / 8);
        p.rot_wave = (int)(period / 4);                // measured best on the bunny scenes: 128 / 160 blocks
        p.rot_set = (int)(period / 4 + period / 16);
        if (const char *e = knob("RT_ROT_WAVE")) p.rot_wave = atoi(e);
        if (const char *e = knob("RT_ROT_SET")) p.rot_set = atoi(e);
        p.rot_wave &= ~3;  // keeps wave j of a workgroup on blocks = j (mod 4): the map stays a bijection
    }
    if (const char *e = knob("RT_PRIO_ROTATE")) p.prio_rotate = atoi(e);
    // The 4-waves-per-SIMD reference-mode builds deal a workgroup's slots to its lanes a chunk of camera rays at a time
    // (the caller drops it for ray tables, for per-sample streams and for frames of one generation, which never run a chain in
    // k_paths).
    // The lanes of the grid must divide the shard evenly: a workgroup's entries are (slot set, lane).
    // With one slot per lane there is nothing to balance (a lane that runs ahead only leaves claims): the static deal, unless asked.
    p.slot_chunk = (p.few_blocks || n / (p.blocks * kBlock) < 2) ? 0 : kSlotChunkAuto;
    if (const char *e = knob("RT_SLOT_CHUNK")) p.slot_chunk = p.few_blocks ? 0 : std::max(0, std::min(1 << 20, atoi(e)));
    if (n % (p.blocks * kBlock) != 0) p.slot_chunk = 0;
    if (n / (p.blocks * kBlock) > kChunkSetsMax) p.slot_chunk = 0;  // (RT_PATHS_BLOCKS far below its default)
    p.slot_head = kSlotHeadAuto;
    if (const char *e = knob("RT_SLOT_HEAD")) p.slot_head = std::max(0, atoi(e));
    return p;
}
// The static head of the chunked deal for a shard of `sets` slots per lane: 0 .. sets - 1 (at least one set is dealt), and never
// more dealt sets than the semaphores hold.
inline int slot_head_for(const PathsLaunch &p, int sets) {
    const int head = p.slot_head == kSlotHeadAuto ? sets - kDealtSetsDefault : p.slot_head;
    return std::max(std::max(0, sets - kDealtSetsMax), std::min(head, sets - 1));
}
// k_paths<PathsChunked>'s static LDS must leave the workgroups as resident as the plan assumes (`workgroups_per_cu`: the device's
// answer for that kernel at p.lds_bytes of dynamic LDS); scenes whose tables in LDS leave no room keep the static deal.
inline int slot_chunk_if_resident(int chunk, int workgroups_per_cu) { return workgroups_per_cu >= kChunkWorkgroupsPerCu ? chunk : 0; }
// G for a frame whose slots run `chain` camera rays each inside k_paths (= the index of the final generation)
inline int slot_chunk_for(const PathsLaunch &p, int chain) {
    if (p.slot_chunk != kSlotChunkAuto) return p.slot_chunk;
    if (chain < kChunkChainLo || chain > kChunkChainHi) return 0;
    return (chain + kChunksPerSlot - 1) / kChunksPerSlot;
}
}  // namespace rtplan
