// rt_slot_chunks.h -- the chunked deal of a workgroup's slots to its lanes (k_paths<PathsChunked>, reference mode, 4 waves per SIMD):
// the pure decisions, shared by the kernel and by host programs (rt_host_check.cpp exports the mapping;
// tests/cpp/slot_chunks_check.cpp and slot_chunks_head_check.cpp play the protocol with std::atomic).
//
// A workgroup keeps exactly the slots the static deal gives it: sets x 256, (set, lane of the workgroup) <-> slot_of(set, that
// lane).  Static head, dealt tail: a lane first runs its own slots of the sets 0 .. head - 1 for their whole chains, exactly as
// the static deal does -- no task, no semaphore, no test for a chunk's end.  Only the sets head .. sets - 1 are dealt (a lane's
// totals differ only at the end, and at least two dealt slots per lane are what makes a hand-over balance anything): S =
// (sets - head) x 256 entries, entry idx <-> (set = head + idx / 256, lane = idx % 256).  The lanes take them G camera rays at
// a time: task t of the workgroup means "run up to G camera rays of entry t % S" (level t / S, level-major), tasks are dealt
// from one counter, and a slot's chain changes lanes only between two camera rays -- where its live state is gen and the six
// RNG words.
//
// Hand-over without waiting: one semaphore per entry (1 = banked: the state is stored and nobody runs the slot).
//   taker            old = fetch_sub(sem, 1, acquire);  taker_runs(old): load the state and run; otherwise the -1 stays as a
//                    claim and the taker draws its next task at once
//   runner, at a     (chunk_ends) stores the state, then old = fetch_add(sem, 1, release);  runner_keeps(old): a claim was
//   chunk's end      pending, the runner runs the next chunk itself from registers; otherwise the slot is banked and the
//                    runner draws a new task
// A runner that finds the slot's chain at its end does not bank it (the final state is stored as in the static deal), so a
// banked slot always has a ray left and every chunk that is started consumes one task: ceil(rays / G) tasks per slot are
// enough, surplus tasks leave claims nobody needs.  Nobody ever waits: every decision is one atomic.
//
// Only the lanes of the workgroup touch its semaphores, so they live in its LDS (workgroup scope; the release still orders the
// runner's global stores of the state before it): 16-bit fields, two to a word, biased so that a field never borrows from or
// carries into its neighbour -- sem_word / sem_unit / sem_value below.  The ended camera ray's sum goes to the framebuffer
// after the hand-over, so that no hand-over waits for a float atomic's acknowledgement.
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

// The semaphores of a workgroup's dealt entries, packed: entry idx is the 16-bit field idx & 1 of word idx >> 1, and holds
// kSemBias + the semaphore's value.  The atomics add or subtract sem_unit(idx); sem_value(old word, idx) is the `old_sem` of
// the two decisions above.
// Bound: a field starts at kSemBias + 1 (banked) and never exceeds it (a release follows a take or a claim).  It is lowered
// once per task of its slot at most (the take or the claim of that task), and a slot has at most 2 047 tasks: levels(rays, G)
// <= rays <= 2 047, because render_shard_impl refuses frames whose camera-ray ids come within 13 W of 2^31.  So a field stays
// within [kSemBias - 2 046, kSemBias + 1], inside (0, 0xffff): no borrow, no carry.
constexpr unsigned kSemBias = 0x4000u, kSemBanked = kSemBias + 1u;
constexpr unsigned kSemWordInit = kSemBanked | (kSemBanked << 16);  // both fields banked
constexpr unsigned kDealtSetsMax = 4;                               // dealt sets of a workgroup: 1 024 fields, 2 KB of LDS
constexpr unsigned kSemWords = kDealtSetsMax * kLanes / 2u;
static_assert(kSemBias > 2046u && kSemBias + 1u < 0x10000u, "a field must hold [bias - 2046, bias + 1]");
RT_CHUNKS_FN unsigned sem_word(unsigned idx) { return idx >> 1; }
RT_CHUNKS_FN unsigned sem_unit(unsigned idx) { return 1u << (16u * (idx & 1u)); }
RT_CHUNKS_FN int sem_value(unsigned word, unsigned idx) { return (int)((word >> (16u * (idx & 1u))) & 0xffffu) - (int)kSemBias; }

// The inverse of slot_of: the (slot set, lane of the grid) whose slot `slot` is.  A runner finds its slot's semaphore with it
// at a chunk's end, so that no entry index lives in a register across the kernel's main loop.  `rot_wave`: a multiple of 4
// (rt_launch_plan.h), so the low two bits of the wave are those of b - set * rot_set.
struct Owner {
    unsigned set, lane_in_grid;
};
RT_CHUNKS_FN Owner owner_of(unsigned slot, unsigned lanes_in_grid, unsigned rot_wave, unsigned rot_set) {
    const unsigned mask = (lanes_in_grid >> 6) - 1u;
    const unsigned set = slot >> (31u - (unsigned)__builtin_clz(lanes_in_grid)), b = (slot >> 6) & mask;
    const unsigned low = (b - set * rot_set) & 3u;
    const unsigned wave = (b - low * rot_wave - set * rot_set) & mask;
    return Owner{set, wave * 64u + (slot & 63u)};
}

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

// The smallest multiple of G above gen, without a division: floor(gen / G) = floor((gen + 1/2) / G) is the high word of
// (2 gen + 1) * ceil(2^31 / G).  Exact for gen, G <= 2 047: the constant exceeds 2^31 / G by less than G / 2^31 of itself,
// which moves the quotient by less than (2 gen + 1) G / 2^32 < 1 / (2 G) -- the distance (gen + 1/2) / G keeps from the next
// integer.  (The half is what lets G = 1 in: its constant is 2^31, not 2^32.)
RT_CHUNKS_FN unsigned next_multiple_mul(unsigned G) { return (0x80000000u + G - 1u) / G; }
RT_CHUNKS_FN unsigned next_multiple(unsigned gen, unsigned G, unsigned mul) {
    return ((unsigned)(((unsigned long long)(2u * gen + 1u) * mul) >> 32) + 1u) * G;
}
// Where a lane's run over background pixels ends at the latest (the GEN block of k_paths<PathsBg>), fixed before the run: the run
// goes on while gen < run_limit.  g_stop: the generation at which the slot's chain ends; a dealt lane also stops at the next
// chunk's end (the generation the per-turn test chunk_ends(gen, m, false) would stop it at: gen reaches a multiple of G exactly
// when it reaches the next one); a lane that cannot step its pixel takes one turn.
RT_CHUNKS_FN unsigned run_limit(unsigned gen, unsigned g_stop, bool dealt, bool can_loop, unsigned G, unsigned mul) {
    unsigned limit = g_stop;
    if (dealt) {
        const unsigned e = next_multiple(gen, G, mul);
        limit = e < limit ? e : limit;
    }
    if (!can_loop) limit = gen + 1u < limit ? gen + 1u : limit;
    return limit;
}
}  // namespace rtchunks
