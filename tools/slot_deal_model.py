#!/usr/bin/env python3
"""A CPU MODEL (not a measurement) of k_paths<PathsChunked>'s deal of a workgroup's slots to its lanes, to price a change to the
deal before it is built: the protocol of rtcuda_amd/csrc/rt_slot_chunks.h played for one workgroup in simulated time.

The model: 256 lanes and `sets` x 256 chains of `rays` camera rays; a ray's cost is gamma distributed with coefficient of
variation `cv` (1.08 reproduces the 5 to 6 % lane-idle tail measured on C2's static deal); a hand-over -- the runner's store
and release at a chunk's end, whether it keeps the slot or not -- costs `handover` mean rays (1.0 is what the sweep of G in
profiles/slot_chunks.md implies).  Lanes run independently: there are no waves, no blocks issued for a whole wave, no memory
system.  A lane runs its first `head` slot sets statically and whole; the remaining sets are dealt G rays at a time from one
task counter, with the semaphore decisions of the header (take, claim, keep).

Prints per deal: T / ideal (the workgroup's finishing time over total ray cost / 256), the lane tail (mean time between a
lane's end and T, as a share of T) and the hand-overs per lane.

usage: slot_deal_model.py [--sets 4] [--rays 506] [--cv 1.08] [--seeds 8]"""
import argparse
import heapq

import numpy as np

LANES = 256


def play(cost, head, G, handover):
    """cost[set, lane, ray].  Returns (finishing time, per-lane end times, hand-overs)."""
    sets, _, rays = cost.shape
    if G <= 0:
        head = sets                      # the static deal: every set whole
    cum = np.concatenate([np.zeros((sets, LANES, 1)), np.cumsum(cost, axis=2)], axis=2)
    t_lane = cum[:head, :, rays].sum(axis=0) if head else np.zeros(LANES)   # the static head: whole chains, no hand-over
    if G <= 0 or head >= sets:
        return t_lane.max(), t_lane, 0
    dealt = sets - head
    S = dealt * LANES
    levels = -(-rays // G)
    tasks = S * levels
    sem = np.ones(S, np.int64)          # 1 = banked
    gen = np.zeros(S, np.int64)         # next ray of the entry
    next_task, handovers = 0, 0
    end = np.zeros(LANES)
    # events: (time, lane, entry it runs or -1)
    heap = [(float(t_lane[l]), l, -1) for l in range(LANES)]
    heapq.heapify(heap)
    while heap:
        t, l, e = heapq.heappop(heap)
        if e >= 0:                       # the lane's chunk of entry e has ended at t
            if gen[e] >= rays:           # the chain's end: not banked
                e = -1
            else:                        # a chunk's end: store + release
                t += handover
                handovers += 1
                old = sem[e]
                sem[e] += 1
                if old >= 0:             # no claim pending: banked
                    e = -1
        while e < 0:                     # draw tasks until one is taken or they are out (claims cost nothing here)
            if next_task >= tasks:
                break
            k = next_task % S
            next_task += 1
            old = sem[k]
            sem[k] -= 1
            if old >= 1:
                e = k
        if e < 0:
            end[l] = t
            continue
        g0 = gen[e]
        g1 = min(rays, (g0 // G + 1) * G)
        gen[e] = g1
        s, ln = head + e // LANES, e % LANES
        heapq.heappush(heap, (t + cum[s, ln, g1] - cum[s, ln, g0], l, e))
    assert (gen == rays).all()
    return end.max(), end, handovers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--rays", type=int, default=506)
    ap.add_argument("--cv", type=float, default=1.08)
    ap.add_argument("--seeds", type=int, default=8)
    a = ap.parse_args()
    shape = 1.0 / (a.cv * a.cv)
    deals = [("static", 0, 0, 0.0), ("every set dealt, G = 64", 0, 64, 1.0)]
    for head in range(1, a.sets):
        deals.append((f"sets 0 .. {head - 1} static, the rest dealt, G = 64", head, 64, 1.0))
        deals.append((f"  head {head} with the hand-over at half its cost", head, 64, 0.5))
    deals.append(("every set dealt, G = 64, hand-over at half its cost", 0, 64, 0.5))
    rows = {name: [] for name, *_ in deals}
    for seed in range(a.seeds):
        rng = np.random.default_rng(seed)
        cost = rng.gamma(shape, 1.0 / shape, size=(a.sets, LANES, a.rays))   # mean 1
        ideal = cost.sum() / LANES
        for name, head, G, ho in deals:
            T, end, n = play(cost, head, G, ho)
            rows[name].append((T / ideal, float((T - end).mean() / T), n / LANES))
    print(f"model: {a.sets} sets x {LANES} chains of {a.rays} rays, gamma cost cv {a.cv}, {a.seeds} seeds")
    print(f"{'deal':58s} {'T / ideal':>9s} {'lane tail':>10s} {'hand-overs per lane':>20s}")
    for name, *_ in deals:
        r = np.mean(rows[name], axis=0)
        print(f"{name:58s} {r[0]:9.3f} {100 * r[1]:9.1f} % {r[2]:20.1f}")


if __name__ == "__main__":
    main()
