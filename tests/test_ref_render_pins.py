"""The oracle's literal render against the REFERENCE'S OWN render(), frame by frame and bit for bit.  CPU only.

tests/golden/ref_render_fixture.npz holds, for every frame of tests/shade_scenes.py FRAMES, the scene as plain arrays and
what the reference's source -- compiled for the CPU under oracle/ref_shim.h, driven by oracle/ref_render_driver.cpp --
computed for it: the Camera, the raw fp32 sums, the post-processed image, the per-iteration (mat, gen, ah, ch) queue counts
and the emission / any-hit / closest-hit-shadow deposit counts (tests/golden/make_ref_render_fixture.py).  The pinned oracle
must give the same numbers exactly: every BSDF, light sample, MIS weight, roulette draw, ray offset, queue order and float
add of the frame is in them.  The shim's substitutions -- and so what "the reference" means here -- are listed in
oracle/ref_shim.h and DESIGN.md section 2.3."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import shade_scenes as ss

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = np.load(os.path.join(HERE, "golden", "ref_render_fixture.npz"))
W = 1 << 20


def test_the_fixture_holds_every_frame_and_the_frames_cover_what_they_claim():
    assert FIXTURE["frames"].tolist() == list(ss.FRAMES) and len(ss.FRAMES) >= 12
    par = {n: ss.fixture_frame(FIXTURE, n)["params"].tolist() for n in ss.FRAMES}
    assert all(w <= 64 and h <= 64 for w, h, *_ in par.values())
    assert sum(w * h * spp > W for w, h, spp, _, _ in par.values()) >= 2            # several generations, slot reuse
    assert {0, 1} <= {p[3] for p in par.values()} and max(p[3] for p in par.values()) > 4   # max_bounces 0, 1, above RR_START
    assert len({p[4] for p in par.values()}) >= 2                                   # two seeds
    kinds = {}
    for n in ss.FRAMES:
        d = ss.fixture_frame(FIXTURE, n)
        a = ss.scene_from_arrays(d)
        kinds[n] = (sorted(set(a.lights["type"].tolist())), len(a.lights))
        v = a.tris.reshape(-1, 3)
        assert (v.min(axis=0) < -0.9).all() and (v.max(axis=0) > 0.9).all()           # the box is centred on the origin
        bad = (~np.isfinite(d["image"])).any(axis=2).sum()
        assert bad * 10000 <= d["image"].shape[0] * d["image"].shape[1]
    assert kinds["lights_point"][0] == [0] and kinds["lights_mixed"][0] == [0, 1] and kinds["lights_none"][1] == 0
    assert kinds["lights_seven"][1] >= 5
    glass = ss.scene_from_arrays(ss.fixture_frame(FIXTURE, "glass")).materials
    ior = glass["ior"][glass["type"] == ss.GLASS]
    assert (ior == 1.0).any() and (ior < 1.0).any() and (ior > 2.0).any()
    assert ss.fixture_frame(FIXTURE, "emitter")["deposits"][0] > 500                # bounce-0 emission
    assert ss.fixture_frame(FIXTURE, "bounces_0")["deposits"][1] == 0


@pytest.mark.parametrize("name", list(ss.FRAMES))
def test_generator_reproduces_the_stored_arrays(name):
    want, got = ss.fixture_frame(FIXTURE, name), ss.frame_arrays(name)
    for k, v in got.items():
        assert want[k].dtype == v.dtype and np.array_equal(want[k].view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), k


@pytest.mark.parametrize("name", list(ss.FRAMES))
def test_oracle_render_equals_the_reference_bit_for_bit(oracle, name):
    d = ss.fixture_frame(FIXTURE, name)
    w, h, spp, max_bounces, seed = (int(x) for x in d["params"])
    cp = d["camera_params"]
    cam = oracle.camera(cp[0:3], cp[3:6], cp[6:9], float(cp[9]), float(cp[10]))
    assert np.array_equal(cam.view(np.uint32), d["cam12"].view(np.uint32))          # Camera::Camera (camera.cuh:15-29)
    sc = oracle.scene(ss.scene_from_arrays(d, name))
    image, sums, st = sc.render(d["cam12"], w, h, spp, max_bounces=max_bounces, seed=seed, threads=1)
    sc.close()
    assert np.array_equal(st["iter_counts"], d["iter_counts"]), (st["iter_counts"][:4], d["iter_counts"][:4])
    assert [st["emission_adds"], st["ah_adds"], st["ch_adds"]] == d["deposits"].tolist()
    nan_s, nan_w = np.isnan(sums), np.isnan(d["sums"])
    assert np.array_equal(nan_s, nan_w)
    diff = (sums.view(np.uint32) != d["sums"].view(np.uint32)) & ~nan_w
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4], sums[diff][:4], d["sums"][diff][:4])
    diff = (image.view(np.uint32) != d["image"].view(np.uint32)) & ~np.isnan(d["image"])
    assert not diff.any() and np.array_equal(np.isnan(image), np.isnan(d["image"]))


@pytest.mark.skipif(not (os.path.isdir(os.environ.get("REF", "/root/reference")) and os.path.isdir(os.path.join(ROOT, "oracle", "_ref"))),
                    reason="the reference tree and oracle/_ref exist only where the fixtures are made")
@pytest.mark.parametrize("which", ["render", "shade"])
def test_rerunning_the_maker_reproduces_the_committed_bytes(tmp_path, which):
    out = str(tmp_path / f"ref_{which}_fixture.npz")
    subprocess.check_call([sys.executable, os.path.join(HERE, "golden", f"make_ref_{which}_fixture.py"), out], stdout=subprocess.DEVNULL)
    assert filecmp.cmp(out, os.path.join(HERE, "golden", f"ref_{which}_fixture.npz"), shallow=False)
