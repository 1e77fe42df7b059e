// The chunked deal of k_paths with a static head and packed semaphores (rtcuda_amd/csrc/rt_slot_chunks.h), played by host
// threads.  Each thread is a lane.  A lane first runs the slots of its first `head` slot sets for their whole chains, as the
// static deal does, and consults neither the task counter nor a semaphore for them.  The remaining sets are dealt G camera
// rays at a time: std::atomic<uint32_t> words hold two 16-bit semaphore fields each, packed and decided by the functions of
// rt_slot_chunks.h, and one more atomic is the workgroup's task counter.  A slot's "state" is the index of its next camera
// ray.  Lanes yield at random between the steps of the protocol.
//
// Checked: every ray index of every slot ran exactly once and in order; no slot ever had two runners; all tasks were dealt;
// no field of a semaphore word -- the one operated on or its neighbour -- ever left [bias - tasks of a slot, bias + 1].
// Nobody waits for anybody: there is no loop in a lane's life that does not draw a task or run a ray.
//
// usage: slot_chunks_head_check [lanes] [sets] [G] [head] [seed] [surplus levels] [live dealt entries, 0 = all]
//        (fewer live entries than (sets - head) x 256: the entries past them are slots the shard does not have, which the
//        kernel never touches -- an odd number leaves the last word with one field)                exit status 0 = all held
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <thread>
#include <vector>

#include "../../rtcuda_amd/csrc/rt_slot_chunks.h"

namespace {
struct Slot {
    int gen = 0;                  // the stored state: next camera ray (plain: the semaphore orders it)
    int rays = 0;                 // length of the chain
    std::atomic<int> runners{0};  // lanes inside the slot right now (must never exceed 1)
    std::vector<int> ran;         // ray indices in the order they ran (written by the one runner)
    bool finished = false;
};

int fail(const char *what, long a = 0, long b = 0) {
    fprintf(stderr, "slot_chunks_head_check: %s (%ld, %ld)\n", what, a, b);
    return 1;
}
}  // namespace

int main(int argc, char **argv) {
    const int lanes = argc > 1 ? atoi(argv[1]) : 8;
    const unsigned sets = argc > 2 ? (unsigned)atoi(argv[2]) : 4u;
    const unsigned G = argc > 3 ? (unsigned)atoi(argv[3]) : 3u;
    const unsigned head = argc > 4 ? (unsigned)atoi(argv[4]) : 2u;
    const unsigned seed = argc > 5 ? (unsigned)atoi(argv[5]) : 1u;
    const unsigned surplus = argc > 6 ? (unsigned)atoi(argv[6]) : 2u;
    if (lanes < 1 || sets < 1 || G < 1 || head >= sets || sets - head > rtchunks::kDealtSetsMax) return fail("bad arguments");
    const unsigned dealt_sets = sets - head;
    const unsigned S = dealt_sets * rtchunks::kLanes;  // entries of the deal
    const unsigned live = argc > 7 && atoi(argv[7]) > 0 ? std::min(S, (unsigned)atoi(argv[7])) : S;
    // slot (set, lane of the workgroup) at [set * 256 + lane]; the dealt entry idx is slot (head + idx / 256, idx % 256)
    std::vector<Slot> slots((size_t)sets * rtchunks::kLanes);
    std::mt19937 rng(seed);
    unsigned max_rays = 0;
    for (Slot &s : slots) {  // ragged chains
        s.rays = 20 + (int)(rng() % 31u);
        s.ran.reserve((size_t)s.rays);
        max_rays = std::max(max_rays, (unsigned)s.rays);
    }
    // levels for the longest chain, and some more: surplus tasks must be harmless
    const unsigned tasks_of_slot = rtchunks::levels(max_rays, G) + surplus;
    const unsigned tasks = S * tasks_of_slot;
    if (tasks_of_slot > 2047u) return fail("more tasks per slot than a field holds");
    const rtchunks::Multiple mult = rtchunks::multiple_of(G);
    const unsigned words = (live + 1u) / 2u;
    std::unique_ptr<std::atomic<uint32_t>[]> sem(new std::atomic<uint32_t>[words]);
    // as the kernel's prologue leaves them: every field banked (a last word with one live field keeps its spare one banked too)
    for (unsigned k = 0; k < words; k++) sem[k].store(rtchunks::kSemWordInit, std::memory_order_relaxed);
    std::atomic<unsigned> next_task{0};
    std::atomic<int> errors{0}, out_of_range{0};
    std::atomic<long> dealt{0};

    // both fields of a word seen by an atomic, and the operated field after it
    auto in_range = [&](int v) { return v >= -(int)tasks_of_slot && v <= 1; };
    auto check_word = [&](uint32_t old_word, unsigned idx, int delta) {
        const int mine = rtchunks::sem_value(old_word, idx), other = rtchunks::sem_value(old_word, idx ^ 1u);
        if (!in_range(mine) || !in_range(other) || !in_range(mine + delta)) out_of_range++;
    };

    auto lane = [&](int id) {
        std::mt19937 r(seed * 7919u + (unsigned)id);
        auto maybe_yield = [&]() { if ((r() & 3u) == 0u) std::this_thread::yield(); };
        // ---- the static head: this lane's own slots of sets 0 .. head - 1, each for its whole chain
        for (unsigned set = 0; set < head; set++)
            for (unsigned l = (unsigned)id; l < rtchunks::kLanes; l += (unsigned)lanes) {
                Slot &s = slots[set * rtchunks::kLanes + l];
                if (s.runners.fetch_add(1) != 0) errors++;
                for (int gen = s.gen; gen < s.rays; gen++) {
                    s.ran.push_back(gen);
                    maybe_yield();
                }
                s.gen = s.rays;
                s.finished = true;
                if (s.runners.fetch_sub(1) != 1) errors++;
            }
        // ---- the dealt tail
        Slot *mine = nullptr;
        unsigned my_idx = 0;
        int gen = 0;        // "registers": the state of the slot this lane runs
        bool fresh = true;  // no ray of this slot made on this lane yet
        while (true) {
            if (!mine) {  // take
                const unsigned t = next_task.fetch_add(1u, std::memory_order_relaxed);
                if (t >= tasks) return;  // out of tasks: done
                dealt.fetch_add(1, std::memory_order_relaxed);
                const rtchunks::Entry e = rtchunks::task_entry(t, dealt_sets);
                if (e.set >= dealt_sets || e.lane >= rtchunks::kLanes) { errors++; return; }
                const unsigned idx = e.set * rtchunks::kLanes + e.lane;
                if (idx >= live) continue;  // a slot the shard does not have: the kernel does not touch a semaphore for it
                Slot &s = slots[(head + e.set) * rtchunks::kLanes + e.lane];
                maybe_yield();
                const uint32_t old = sem[rtchunks::sem_word(idx)].fetch_sub(rtchunks::sem_unit(idx), std::memory_order_acquire);
                check_word(old, idx, -1);
                if (!rtchunks::taker_runs(rtchunks::sem_value(old, idx))) continue;  // a claim stays behind; draw the next task at once
                if (s.runners.fetch_add(1) != 0) errors++;
                if (s.finished) errors++;  // a finished slot is never banked
                mine = &s;
                my_idx = idx;
                gen = s.gen;
                fresh = true;
                maybe_yield();
            } else if (rtchunks::chunk_ends((unsigned)gen, mult, fresh) && gen < mine->rays) {  // a chunk's end, not the chain's
                mine->gen = gen;  // store_slot
                maybe_yield();
                if (mine->runners.fetch_sub(1) != 1) errors++;
                const uint32_t old = sem[rtchunks::sem_word(my_idx)].fetch_add(rtchunks::sem_unit(my_idx), std::memory_order_release);
                check_word(old, my_idx, +1);
                if (rtchunks::runner_keeps(rtchunks::sem_value(old, my_idx))) {
                    if (mine->runners.fetch_add(1) != 0) errors++;  // (the claim's task runs here: nobody else may have come in)
                    fresh = true;  // the next chunk, from registers; its first ray is not a chunk's end
                } else {
                    mine = nullptr;
                    continue;
                }
            }
            if (mine) {  // gen()
                if (gen >= mine->rays) {  // the chain's end: the final state is stored, the slot is not banked
                    mine->gen = gen;
                    mine->finished = true;
                    if (mine->runners.fetch_sub(1) != 1) errors++;
                    mine = nullptr;
                    continue;
                }
                mine->ran.push_back(gen);
                gen++;
                fresh = false;
                maybe_yield();
            }
        }
    };
    std::vector<std::thread> th;
    for (int k = 0; k < lanes; k++) th.emplace_back(lane, k);
    for (std::thread &t : th) t.join();

    if (errors.load()) return fail("a slot had two runners, or a finished slot was taken", errors.load());
    if (out_of_range.load()) return fail("a semaphore field left [bias - tasks of a slot, bias + 1]", out_of_range.load(), (long)tasks_of_slot);
    if (next_task.load() < tasks || dealt.load() != (long)tasks) return fail("tasks left undealt", (long)next_task.load(), (long)tasks);
    for (unsigned k = 0; k < words; k++)  // the fields as the frame leaves them: within the bound too, spare field untouched
        for (unsigned f = 0; f < 2u; f++) {
            const int v = rtchunks::sem_value(sem[k].load(), 2u * k + f);
            if (2u * k + f >= live ? v != 1 : !in_range(v)) return fail("a semaphore field ended out of range", (long)(2u * k + f), (long)v);
        }
    for (unsigned k = 0; k < (unsigned)slots.size(); k++) {
        const Slot &s = slots[k];
        const bool is_live = k < head * rtchunks::kLanes || k - head * rtchunks::kLanes < live;
        if (!is_live) {
            if (!s.ran.empty() || s.finished) return fail("a slot the shard does not have ran", (long)k);
            continue;
        }
        if (!s.finished) return fail("a slot did not finish", (long)k, (long)s.gen);
        if ((int)s.ran.size() != s.rays) return fail("a slot ran the wrong number of rays", (long)k, (long)s.ran.size());
        for (int g = 0; g < s.rays; g++)
            if (s.ran[(size_t)g] != g) return fail("a slot's rays ran out of order", (long)k, (long)g);
        if (s.runners.load() != 0) return fail("a runner was left inside a slot", (long)k);
    }
    printf("ok lanes=%d sets=%u G=%u head=%u seed=%u dealt entries=%u of %u words=%u tasks=%u\n", lanes, sets, G, head, seed, live, S, words, tasks);
    return 0;
}
