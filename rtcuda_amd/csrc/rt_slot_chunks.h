// rt_slot_chunks.h -- the chunked deal of a workgroup's slots to its lanes (k_paths, reference mode, 4 waves per SIMD): the
// pure decisions, shared by the kernel and by host programs (rt_host_check.cpp exports the mapping; tests/cpp/slot_chunks_check.cpp
// plays the protocol with std::atomic).
//
// A workgroup keeps exactly the slots the static deal gives it: S = sets x 256, entry idx <-> (set = idx / 256, lane of the
// workgroup = idx % 256) <-> slot_of(set, that lane).  Its lanes take them G camera rays at a time: task t of the workgroup
// means "run up to G camera rays of entry t % S" (level t / S, level-major), tasks are dealt from one counter, and a slot's
// chain changes lanes only between two camera rays -- where its live state is gen and the six RNG words.
//
// Hand-over without waiting: one int per slot (1 = banked: the state is stored and nobody runs the slot).
//   taker            old = fetch_sub(sem, 1, acquire);  taker_runs(old): load the state and run; otherwise the -1 stays as a
//                    claim and the taker draws its next task at once
//   runner, at a     (chunk_ends) stores the state, then old = fetch_add(sem, 1, release);  runner_keeps(old): a claim was
//   chunk's end      pending, the runner runs the next chunk itself from registers; otherwise the slot is banked and the
//                    runner draws a new task
// A runner that finds the slot's chain at its end does not bank it (the final state is stored as in the static deal), so a
// banked slot always has a ray left and every chunk that is started consumes one task: ceil(rays / G) tasks per slot are
// enough, surplus tasks leave claims nobody needs.  Nobody ever waits: every decision is one atomic.
#pragma once

#if defined(__HIPCC__)
#define RT_CHUNKS_FN __host__ __device__ inline
#else
#define RT_CHUNKS_FN inline
#endif

namespace rtchunks {
constexpr unsigned kLanes = 256;  // lanes of a workgroup (kBlock)

// tasks of one slot: chunks of G in a chain of `rays` camera rays
RT_CHUNKS_FN unsigned levels(unsigned rays, unsigned G) { return (rays + G - 1u) / G; }
// tasks of a workgroup of `sets` slots per lane
RT_CHUNKS_FN unsigned task_count(unsigned sets, unsigned rays, unsigned G) { return sets * kLanes * levels(rays, G); }

struct Entry {
    unsigned set, lane, level;
};
RT_CHUNKS_FN Entry task_entry(unsigned t, unsigned sets) {
    const unsigned S = sets * kLanes, idx = t % S;
    return Entry{idx / kLanes, idx % kLanes, t / S};
}

// The static deal's slot of (slot set, lane of the grid): a wave owns 64 consecutive slots; the j-th wave of a workgroup is
// shifted by j * rot_wave 64-slot blocks and the k-th slot set by k * rot_set (see k_paths).  `lanes_in_grid`: a power of two.
RT_CHUNKS_FN int slot_of(unsigned set, unsigned lane_in_grid, unsigned lanes_in_grid, unsigned rot_wave, unsigned rot_set) {
    const unsigned wave_in_grid = lane_in_grid >> 6, lane_in_wave = lane_in_grid & 63u;
    const unsigned b = (wave_in_grid + (wave_in_grid & 3u) * rot_wave + set * rot_set) & ((lanes_in_grid >> 6) - 1u);
    return (int)(set * lanes_in_grid + b * 64u + lane_in_wave);
}

RT_CHUNKS_FN bool taker_runs(int old_sem) { return old_sem >= 1; }
RT_CHUNKS_FN bool runner_keeps(int old_sem) { return old_sem < 0; }

// "gen is a multiple of G" without a division in the GEN block: gen * (odd part of G)^-1 mod 2^32, rotated right by G's
// trailing zeros, is at most (2^32 - 1) / G exactly for the multiples (Lemire, Kaser, Kurz 2019).
struct Multiple {
    unsigned inv, shift, limit;
};
RT_CHUNKS_FN Multiple multiple_of(unsigned G) {
    unsigned shift = 0;
    while (((G >> shift) & 1u) == 0u) shift++;
    const unsigned odd = G >> shift;
    unsigned inv = odd;  // (correct to 3 bits; each step doubles them)
    for (int k = 0; k < 5; k++) inv *= 2u - odd * inv;
    return Multiple{inv, shift, 0xffffffffu / G};
}
RT_CHUNKS_FN bool is_multiple(unsigned gen, const Multiple &m) {
    const unsigned q = gen * m.inv;
    return ((q >> m.shift) | (m.shift ? q << (32u - m.shift) : 0u)) <= m.limit;
}
// the runner's test in the GEN block: the slot has made at least one ray on this lane (`fresh`: none yet) and stands at a
// multiple of G
RT_CHUNKS_FN bool chunk_ends(unsigned gen, const Multiple &m, bool fresh) { return !fresh && is_multiple(gen, m); }
}  // namespace rtchunks
