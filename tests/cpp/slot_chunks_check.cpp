// The hand-over protocol of k_paths' chunked deal (rtcuda_amd/csrc/rt_slot_chunks.h), played by host threads: each thread is
// a lane, std::atomic<int> stands in for a slot's semaphore and for the workgroup's task counter, a slot's "state" is the
// index of its next camera ray.  Lanes yield at random between the steps of the protocol.  Checked: every ray index of every
// slot ran exactly once and in order, no lane ever ran a slot another lane was running, all tasks were dealt, and nobody
// waited for anybody (there is no loop in a lane's life that does not draw a task or run a ray).
//
// usage: slot_chunks_check [lanes] [sets] [G] [seed] [surplus levels]       exit status 0 = all held
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "../../rtcuda_amd/csrc/rt_slot_chunks.h"

namespace {
struct Slot {
    std::atomic<int> sem{1};       // as k_pool_init leaves it: banked
    int gen = 0;                   // the stored state: next camera ray (plain: the semaphore orders it)
    int rays = 0;                  // length of the chain
    std::atomic<int> runners{0};   // lanes inside the slot right now (must never exceed 1)
    std::vector<int> ran;          // ray indices in the order they ran (written by the one runner)
    bool finished = false;
};

int fail(const char *what, long a = 0, long b = 0) {
    fprintf(stderr, "slot_chunks_check: %s (%ld, %ld)\n", what, a, b);
    return 1;
}
}  // namespace

int main(int argc, char **argv) {
    const int lanes = argc > 1 ? atoi(argv[1]) : 8;
    const unsigned sets = argc > 2 ? (unsigned)atoi(argv[2]) : 1u;
    const unsigned G = argc > 3 ? (unsigned)atoi(argv[3]) : 3u;
    const unsigned seed = argc > 4 ? (unsigned)atoi(argv[4]) : 1u;
    const unsigned surplus = argc > 5 ? (unsigned)atoi(argv[5]) : 2u;
    // the workgroup's entries: sets x 256, as in the kernel (the threads share them whatever their number)
    const unsigned S = sets * rtchunks::kLanes;
    std::vector<Slot> slots(S);
    std::mt19937 rng(seed);
    unsigned max_rays = 0;
    for (Slot &s : slots) {  // ragged chains
        s.rays = 20 + (int)(rng() % 31u);
        s.ran.reserve((size_t)s.rays);
        max_rays = std::max(max_rays, (unsigned)s.rays);
    }
    // levels for the longest chain, and some more: surplus tasks must be harmless
    const unsigned tasks = S * (rtchunks::levels(max_rays, G) + surplus);
    const rtchunks::Multiple mult = rtchunks::multiple_of(G);
    std::atomic<unsigned> next_task{0};
    std::atomic<int> errors{0};
    std::atomic<long> dealt{0};

    auto lane = [&](int id) {
        std::mt19937 r(seed * 7919u + (unsigned)id);
        auto maybe_yield = [&]() { if ((r() & 3u) == 0u) std::this_thread::yield(); };
        Slot *mine = nullptr;
        int gen = 0;        // "registers": the state of the slot this lane runs
        bool fresh = true;  // no ray of this slot made on this lane yet
        while (true) {
            if (!mine) {  // take
                const unsigned t = next_task.fetch_add(1u, std::memory_order_relaxed);
                if (t >= tasks) return;  // out of tasks: done
                dealt.fetch_add(1, std::memory_order_relaxed);
                const rtchunks::Entry e = rtchunks::task_entry(t, sets);
                if (e.set >= sets || e.lane >= rtchunks::kLanes) { errors++; return; }
                Slot &s = slots[e.set * rtchunks::kLanes + e.lane];
                maybe_yield();
                const int old = s.sem.fetch_sub(1, std::memory_order_acquire);
                if (!rtchunks::taker_runs(old)) continue;  // a claim stays behind; draw the next task at once
                if (s.runners.fetch_add(1) != 0) errors++;
                if (s.finished) errors++;  // a finished slot is never banked
                mine = &s;
                gen = s.gen;
                fresh = true;
                maybe_yield();
            } else if (rtchunks::chunk_ends((unsigned)gen, mult, fresh) && gen < mine->rays) {  // a chunk's end, not the chain's
                mine->gen = gen;  // store_slot
                maybe_yield();
                if (mine->runners.fetch_sub(1) != 1) errors++;
                const int old = mine->sem.fetch_add(1, std::memory_order_release);
                if (rtchunks::runner_keeps(old)) {
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
    if (next_task.load() < tasks || dealt.load() != (long)tasks) return fail("tasks left undealt", (long)next_task.load(), (long)tasks);
    for (unsigned k = 0; k < S; k++) {
        const Slot &s = slots[k];
        if (!s.finished) return fail("a slot did not finish", (long)k, (long)s.gen);
        if ((int)s.ran.size() != s.rays) return fail("a slot ran the wrong number of rays", (long)k, (long)s.ran.size());
        for (int g = 0; g < s.rays; g++)
            if (s.ran[(size_t)g] != g) return fail("a slot's rays ran out of order", (long)k, (long)g);
        if (s.runners.load() != 0) return fail("a runner was left inside a slot", (long)k);
    }
    printf("ok lanes=%d sets=%u G=%u seed=%u slots=%u tasks=%u\n", lanes, sets, G, seed, S, tasks);
    return 0;
}
