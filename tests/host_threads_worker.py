"""Worker of tests/test_gpu_host_threads.py: several host threads against one library, in a process of its own.

    python tests/host_threads_worker.py --out verdicts.json [--only t1,t6]

A lock-order mistake shows as a deadlock, and a deadlocked ctypes call cannot be interrupted from Python: so the threaded work
runs here, under the parent's time limit.  Every case first computes its SERIAL answers -- one thread, default stream,
everything synchronised, on scene objects of its own made from the same arrays -- and then the threaded ones; a result is
compared as bits (torch.equal, tobytes, == of event totals).  After each case the verdicts so far are written to --out
({"in_progress": next case, "cases": {name: {"passed": bool, "detail": ...}}}), so a parent that had to kill the worker can
name the case it hung in.

Threads are threading.Thread (ctypes releases the GIL for the length of a library call), at most 8, each with its own
torch.cuda.Stream and output buffers, each doing three rounds with a threading.Barrier in front of every round so that the
calls really coincide -- the first calls on fresh state above all."""
import argparse
import ctypes
import dataclasses
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ["RTCUDA_EXPERIMENTAL"] = "1"  # (the gate of the experiment knobs, as tests/conftest.py sets it: t2 uses RT_STACK_CAP)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rtcuda_amd import api, scenes  # noqa: E402
from test_scene_update_host import deform  # noqa: E402
import raygen  # noqa: E402
import denoise_expected as de  # noqa: E402

ROUNDS = 3
EVENTS = ("shade_events", "any_rays", "emission_adds", "shadow_adds", "rr_draws", "camera_rays")
BIG = (128, 72, 256)   # 2.25 generations of the W slots: the persistent k_paths chain and the lockstep final generation
SMALL = (64, 48, 4)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def events(st):
    return {k: int(st[k]) for k in EVENTS}


def frame(sc, whs, seed=1, flags=0, shard=(0, 1), stream=None):
    """(fixed-point sums, event totals) of one render_shard_fixed into a fresh zeroed buffer, on `stream` (None: the default)."""
    w, h, spp = whs
    cam = api.make_camera(aspect=w / h)
    if stream is None:
        sums = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
        st = sc.render_shard_fixed(cam, w, h, spp, shard[0], shard[1], sums.data_ptr(), seed=seed, flags=flags)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            sums = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
            st = sc.render_shard_fixed(cam, w, h, spp, shard[0], shard[1], sums.data_ptr(), seed=seed, flags=flags,
                                       stream=stream.cuda_stream)  # (synchronous on its stream at return)
    return sums, events(st)


def same_frame(got, want):
    """None, or what differs between two (sums, events)."""
    if got[1] != want[1]:
        return f"event totals {got[1]} != {want[1]}"
    if not torch.equal(got[0], want[0]):
        return f"{int((got[0] != want[0]).sum().item())} fixed-point sums differ"
    return None


def same_tensors(got, want, names):
    for g, w, name in zip(got, want, names):
        if g.is_floating_point():
            g, w = g.view(torch.int32), w.view(torch.int32)
        if not torch.equal(g, w):
            return f"{name}: {int((g != w).sum().item())} values differ"
    return None


class Threads:
    """Runs one function per thread for ROUNDS rounds behind a barrier; collects what each reports as wrong."""

    def __init__(self, bodies):
        assert len(bodies) <= 8
        self.bodies = bodies
        self.barrier = threading.Barrier(len(bodies))
        self.wrong = []
        self.lock = threading.Lock()

    def _run(self, k, body):
        try:
            stream = torch.cuda.Stream()
            for r in range(ROUNDS):
                self.barrier.wait()
                msg = body(r, stream)
                if msg:
                    with self.lock:
                        self.wrong.append(f"thread {k} round {r}: {msg}")
            stream.synchronize()
        except Exception as e:  # (an RtError, or a broken barrier after another thread's)
            self.barrier.abort()
            with self.lock:
                self.wrong.append(f"thread {k}: {type(e).__name__}: {e}")

    def run(self):
        torch.cuda.synchronize()
        th = [threading.Thread(target=self._run, args=(k, b)) for k, b in enumerate(self.bodies)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        return self.wrong


# ---- T1: one context, four seeds
def t1():
    full = scenes.cornell_bunny("full_bsdf")
    serial_scene, sc = api.Scene(full), api.Scene(full)
    want = {seed: frame(serial_scene, BIG, seed=seed) for seed in (1, 2, 3, 4)}
    if same_frame(want[1], want[2]) is None:
        return ["the seeds must give different frames"]

    def body(seed):
        return lambda r, stream: same_frame(frame(sc, BIG, seed=seed, stream=stream), want[seed])
    return Threads([body(seed) for seed in (1, 2, 3, 4)]).run()


# ---- T2: three contexts in flight, overflow stacks in use
def t2():
    full = scenes.cornell_bunny("full_bsdf")
    os.environ["RT_STACK_CAP"] = "2"  # (read by every render call; set and removed while no thread is running)
    try:
        serial_scene, sc = api.Scene(full), api.Scene(full)
        whs, shards = (256, 256, 4), ((0, 1), (0, 2), (1, 4))
        want = {sh: frame(serial_scene, whs, shard=sh) for sh in shards}

        def body(sh):
            return lambda r, stream: same_frame(frame(sc, whs, shard=sh, stream=stream), want[sh])
        return Threads([body(sh) for sh in shards]).run()
    finally:
        del os.environ["RT_STACK_CAP"]


# ---- T3: first use of everything at once
def _default_rays(n=20_000, seed=31):
    o, d = raygen.camera_rays(api.make_camera(aspect=16 / 9), 1920, 1080, n, seed=seed)
    return _dev(o), _dev(d)


def t3():
    full = scenes.cornell_bunny("full_bsdf")
    o, d = _default_rays()
    w, h, spp = SMALL
    cam = api.make_camera(aspect=w / h)
    n_pixels, rpp = w * h, 7

    def calls(sc, stream):
        """The six entry points on `sc`; with a stream: what a thread does, else the serial answer."""
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.default_stream())

        def closest():
            with ctx:
                return sc.query_closest(o, d, flags=0)

        def any_():
            with ctx:
                return (sc.query_any(o, d, tmax=tmax, excluded=excluded),)

        def aov():
            with ctx:
                sums, ids, _ = sc.render_aov(cam, w, h, spp, ids=True, stream=stream)
                return sums, ids

        def rays():
            with ctx:
                sums, st = sc.render_rays(o, d, n_pixels, rays_per_pixel=rpp, fixed=True)
                return sums, events(st)

        def shard():
            return frame(sc, SMALL, stream=stream)

        def host():
            img, st = sc.render(cam, w, h, spp, flags=api.FLAG_DETERMINISTIC)
            return img.tobytes(), events(st)
        return closest, any_, aov, rays, shard, host

    serial_scene = api.Scene(full)
    hit, t, _, _ = serial_scene.query_closest(o, d)
    torch.cuda.synchronize()
    n_tris = serial_scene.n_tris()
    tmax = torch.where(hit >= 0, t * 1.001, torch.full_like(t, 3.0e38))
    excluded = torch.where((hit >= 0) & (torch.arange(len(hit), device="cuda") % 2 == 0), hit, (hit + 1) % n_tris).to(torch.int32)
    torch.cuda.synchronize()
    want = []
    for call in calls(serial_scene, None):
        want.append(call())
        torch.cuda.synchronize()
    fresh = api.Scene(full)  # (no call has touched it: reference tree, query scratch, inverse order, events are all to be made)

    def compare(k, got):
        w_ = want[k]
        if k in (0, 1, 2):
            return same_tensors(got, w_, ("hit", "t", "u", "v") if k == 0 else ("occluded",) if k == 1 else ("sums", "ids"))
        if k == 5:
            return None if got == w_ else ("image bytes differ" if got[0] != w_[0] else f"event totals {got[1]} != {w_[1]}")
        return same_frame(got, w_)

    def body(k):
        def run(r, stream):
            got = calls(fresh, stream)[k]()
            stream.synchronize()
            return compare(k, got)
        return run
    return Threads([body(k) for k in range(6)]).run()


# ---- T4: the node records re-padded under load
def _far_batches(seed=41, n=20_000):
    """Four batches whose origins lie 10, 1e2, 1e3 and 1e4 scene sizes out, aimed at the scene (as tests/test_gpu_scene_update.py
    builds them): each is beyond twice the radius the one before left the records padded for, so each re-pads them."""
    out = []
    for k, factor in enumerate((10.0, 1e2, 1e3, 1e4)):
        rng = np.random.default_rng(seed + k)
        target = rng.uniform(0.1, 0.9, (n, 3)) * np.array([1.0, 1.0, -1.0])
        dirs = rng.normal(size=(n, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        o = (target - dirs * factor).astype(np.float32)
        d = target - o.astype(np.float64)
        out.append((_dev(o), _dev((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))))
    return out


def t4():
    full = scenes.cornell_bunny("full_bsdf")
    batches = _far_batches()
    serial_scene = api.Scene(full)
    want_frames = {flags: frame(serial_scene, BIG, flags=flags) for flags in (0, api.FLAG_WATERTIGHT)}
    fresh = api.Scene(full)
    want_hits = []
    for o, d in batches:
        want_hits.append(tuple(x.clone() for x in fresh.query_closest(o, d)))
        torch.cuda.synchronize()
    if not all(0.3 < (h[0] >= 0).float().mean().item() for h in want_hits):
        return ["the far batches must hit the scene"]
    # one warm scene per round (the radius only grows: a scene re-pads for these batches once)
    warm = [api.Scene(full) for _ in range(ROUNDS)]
    for sc in warm:
        frame(sc, SMALL)  # (the default camera is inside the padded radius now; the reference's tree is built)
    b_done = [threading.Event() for _ in range(ROUNDS)]
    frames_of_a = [0]

    def thread_a(r, stream):
        k = 0
        while True:
            flags = (0, api.FLAG_WATERTIGHT)[k % 2]
            msg = same_frame(frame(warm[r], BIG, flags=flags, stream=stream), want_frames[flags])
            k += 1
            frames_of_a[0] += 1
            if msg:
                return f"frame {k} (flags {flags}): {msg}"
            if b_done[r].is_set() and k >= 2:
                return None

    def thread_b(r, stream):
        try:
            for k, (o, d) in enumerate(batches):
                with torch.cuda.stream(stream):
                    got = warm[r].query_closest(o, d)
                stream.synchronize()
                msg = same_tensors(got, want_hits[k], ("hit", "t", "u", "v"))
                if msg:
                    return f"batch {k}: {msg}"
            return None
        finally:
            b_done[r].set()
    wrong = Threads([thread_a, thread_b]).run()
    if frames_of_a[0] < 3:
        wrong.append(f"thread A rendered {frames_of_a[0]} frames, fewer than three")
    return wrong


# ---- T5: edits of one scene while another renders
def _edit_states(full):
    """Per round: (deformed vertices, material table, (lights, tri_light)) -- each different from the state before it."""
    point = np.zeros(1, scenes.LIGHT_DTYPE)
    swapped = np.array(full.tri_light, np.int32)
    swapped[full.tri_light == 0], swapped[full.tri_light == 1] = 1, 0
    states = []
    for r in range(ROUNDS):
        mats = np.ascontiguousarray(full.materials[::-1] if r % 2 == 0 else full.materials).copy()
        mats["albedo"] *= np.float32(1.0 - 0.25 * r)
        point[0] = (0, (0.2 + 0.1 * r, 0.6, -0.3), -1, (0.1, 0.4, 0.2))
        lights = np.concatenate([full.lights[::-1] if r % 2 == 0 else full.lights, point])
        states.append((deform(full.tris, amp=0.01 * (r + 1)), mats, (lights, swapped if r % 2 == 0 else np.array(full.tri_light, np.int32))))
    return states


def t5():
    full, box = scenes.cornell_bunny("full_bsdf"), scenes.cornell_bunny("matte", bunny=False)
    states = _edit_states(full)
    # the serial answers: scenes created anew from each edited state (a rebuild leaves the state of the update before it)
    want_x, cur = [], full
    for tris, mats, (lights, tl) in states:
        per_round = []
        for change in (dict(tris=tris), dict(materials=mats), dict(lights=lights, tri_light=tl)):
            cur = dataclasses.replace(cur, **change)
            anew = api.Scene(cur)
            per_round.append(frame(anew, SMALL))
            anew.close()
        want_x.append(per_round)
    for a, b in ((want_x[0][0], want_x[0][1]), (want_x[0][1], want_x[0][2]), (want_x[0][2], want_x[1][0])):
        if same_frame(a, b) is None:
            return ["every edit must change the frame"]
    y_serial, y = api.Scene(box), api.Scene(box)
    want_y = frame(y_serial, SMALL)
    x = api.Scene(full)
    a_done = [threading.Event() for _ in range(ROUNDS)]

    def thread_a(r, stream):
        tris, mats, (lights, tl) = states[r]
        try:
            edits = (("update", lambda: x.update(tris), 0), ("rebuild", lambda: x.rebuild(), 0),
                     ("set_materials", lambda: x.set_materials(mats), 1), ("set_lights", lambda: x.set_lights(lights, tl), 2))
            for name, edit, k in edits:
                edit()
                msg = same_frame(frame(x, SMALL, stream=stream), want_x[r][k])
                if msg:
                    return f"after {name}: {msg}"
            return None
        finally:
            a_done[r].set()

    def thread_b(r, stream):
        k = 0
        while True:
            msg = same_frame(frame(y, SMALL, stream=stream), want_y)
            k += 1
            if msg:
                return f"frame {k} of the other scene: {msg}"
            if a_done[r].is_set():
                return None
    return Threads([thread_a, thread_b]).run()


# ---- T6: rt_last_error belongs to the thread
def t6():
    L = api.lib()
    full = scenes.cornell_bunny("full_bsdf")
    sc, serial_scene = api.Scene(full), api.Scene(full)
    o, d = _default_rays(n=256)
    hit = torch.full((256,), -7, dtype=torch.int32, device="cuda")
    w, h = 5, 5
    fr = de.synthetic_frame(w, h)
    beauty, aov = _dev(fr[0]), _dev(fr[2])
    scratch = torch.zeros(api.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    out = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    vp = ctypes.c_void_p

    def refused_query():
        rc = L.rt_query_closest_device(sc.h, 0x40, 256, vp(o.data_ptr()), vp(d.data_ptr()), None, vp(hit.data_ptr()), None, None, None, None)
        return rc, L.rt_last_error().decode()

    def refused_denoise():
        prm = api.RtDenoiseParams(passes=9, sigma_color=1.0, sigma_depth=1.0, normal_power_log2=1, flags=0)
        rc = L.rt_denoise_fixed(vp(beauty.data_ptr()), int(fr[1]), vp(aov.data_ptr()), int(fr[3]), w, h, ctypes.byref(prm), vp(scratch.data_ptr()),
                                vp(out.data_ptr()), None)
        return rc, L.rt_last_error().decode()
    (rc_q, msg_q), (rc_d, msg_d) = refused_query(), refused_denoise()
    if not (rc_q and rc_d and msg_q.startswith("rt_query_closest_device: ") and msg_d.startswith("rt_denoise_fixed: ") and "passes" in msg_d):
        return [f"the serial refusals: {rc_q} {msg_q!r}, {rc_d} {msg_d!r}"]
    want = frame(serial_scene, SMALL)
    b_done = [threading.Event() for _ in range(ROUNDS)]

    def thread_a(r, stream):
        k = 0
        while k < 200 or not b_done[r].is_set():  # (refusals all the while B is at work, so that they interleave with B's)
            rc, msg = refused_query()
            k += 1
            if rc == 0 or msg != msg_q:
                return f"refusal {k}: rc {rc}, read {msg!r}, its own message is {msg_q!r}"
        return None

    def thread_b(r, stream):
        try:
            for k in range(6):
                msg = same_frame(frame(sc, SMALL, stream=stream), want)
                if msg:
                    return msg
                for _ in range(50):
                    rc, msg = refused_denoise()
                    if rc == 0 or msg != msg_d:
                        return f"refusal after frame {k}: rc {rc}, read {msg!r}, its own message is {msg_d!r}"
            return None
        finally:
            b_done[r].set()
    wrong = Threads([thread_a, thread_b]).run()
    if int((hit != -7).sum().item()) or int((out != 0).sum().item()):
        wrong.append("a refused call wrote to its output")
    return wrong


# ---- T7: the host-output path, its cached buffers regrown between calls
def t7():
    full = scenes.cornell_bunny("full_bsdf")
    serial_scene, sc = api.Scene(full), api.Scene(full)
    sizes = ((64, 48, 4), (256, 256, 4), (100, 60, 8))

    def image(s, whs):
        w, h, spp = whs
        img, st = s.render(api.make_camera(aspect=w / h), w, h, spp, flags=api.FLAG_DETERMINISTIC)
        return img.tobytes(), events(st)
    want = {whs: image(serial_scene, whs) for whs in sizes}

    def body(whs):
        def run(r, stream):
            got = image(sc, whs)
            if got[1] != want[whs][1]:
                return f"{whs}: event totals {got[1]} != {want[whs][1]}"
            return None if got[0] == want[whs][0] else f"{whs}: image bytes differ"
        return run
    return Threads([body(whs) for whs in sizes]).run()


CASES = (("t1", t1), ("t2", t2), ("t3", t3), ("t4", t4), ("t5", t5), ("t6", t6), ("t7", t7))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    only = [c for c in args.only.split(",") if c]
    api.lib()
    verdicts = {"in_progress": None, "cases": {}, "seconds": {}}

    def write():
        tmp = args.out + ".tmp"
        with open(tmp, "w") as f:
            json.dump(verdicts, f, indent=1)
        os.replace(tmp, args.out)
    t_all = time.time()
    for name, case in CASES:
        if only and name not in only:
            continue
        verdicts["in_progress"] = name
        write()
        t0 = time.time()
        try:
            wrong = case()
        except Exception as e:  # (the serial part failed: the case has no verdict to give but this)
            wrong = [f"{type(e).__name__}: {e}"]
        torch.cuda.synchronize()
        verdicts["cases"][name] = {"passed": not wrong, "detail": wrong}
        verdicts["seconds"][name] = round(time.time() - t0, 3)
        print(name, "passed" if not wrong else wrong, verdicts["seconds"][name], "s", flush=True)
    verdicts["in_progress"] = None
    verdicts["seconds"]["total"] = round(time.time() - t_all, 3)
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
