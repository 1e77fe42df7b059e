"""CPU tests of what the five ray-table entry points refuse on the host, before any device call: every bad argument of the
checks they share, with the exact message, and which message wins when two arguments are bad.  The expected strings
(tests/golden/table_arg_messages.json) were recorded by tests/golden/make_table_arg_messages.py from the library as it stood
before these checks were folded into one body each: the messages, and the order of the checks, are part of the interface.

The scene handle of these calls is a block of host memory that is no scene: every case here is refused before the scene is
looked at.  Should a check ever let a case through, the call must still end in an error and not on the GPU: the block's first
word, where rt_scene keeps its device, names a device that does not exist, and every one of these entry points makes the
scene's device current (and fails there) before it takes a lock, allocates or launches anything."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "table_arg_messages.json")
PLAIN = ("rt_render_rays_device", "rt_render_rays_fixed_device")
KEYED = ("rt_render_rays_keyed_device", "rt_render_rays_keyed_fixed_device")
AOV = ("rt_render_aov_rays_fixed_device",)
ENTRY_POINTS = PLAIN + KEYED + AOV
REFERENCE_WALK, WATERTIGHT = 8, 16
NO_SUCH_DEVICE = 0x7FFFFFF0

# one bad argument each (a changed argument of the valid call below); "keys": only the entry points that take keys
BAD = {
    "null_origin": dict(o=None),
    "null_dir": dict(d=None),
    "null_out": dict(out=None),
    "n_rays_zero": dict(n_rays=0),
    "n_rays_int32_range": dict(n_rays=2 ** 31 - 13 * 2 ** 20),
    "n_pixels_zero": dict(n_pixels=0),
    "n_pixels_too_many": dict(n_pixels=715827883),
    "rays_per_pixel_zero": dict(rays_per_pixel=0),
    "last_ray_one_pixel_past_the_end": dict(n_rays=9),
    "last_ray_past_the_end_two_per_pixel": dict(n_rays=17, rays_per_pixel=2),
    "unknown_flag": dict(flags=1 << 20),
    "both_hit_flags": dict(flags=REFERENCE_WALK | WATERTIGHT),
    "max_bounces_negative": dict(max_bounces=-1),
    "key_stride_zero": dict(key_stride=0),
    "key_wraps": dict(key_first=2 ** 64 - 1, n_rays=2),
    "key_wraps_by_stride": dict(key_first=2 ** 64 - 2 ** 33, n_rays=4, key_stride=2 ** 32 - 1),
    "last_key_one_pixel_past_the_end": dict(key_first=6, n_rays=3),
}
KEYS_ONLY = ("key_stride_zero", "key_wraps", "key_wraps_by_stride", "last_key_one_pixel_past_the_end")
NO_MAX_BOUNCES = AOV
# two bad arguments at once: the order of the checks decides which message the caller sees
PAIRS = [("null_dir", "unknown_flag"), ("unknown_flag", "n_rays_zero"), ("n_rays_zero", "n_pixels_zero"),
         ("n_pixels_too_many", "rays_per_pixel_zero"), ("key_stride_zero", "rays_per_pixel_zero"), ("n_pixels_zero", "key_wraps")]


def cases(entry):
    """[(case name, changed arguments)] of one entry point: every single bad argument it has, then the pairs."""
    def has(name):
        return not (name in KEYS_ONLY and entry in PLAIN) and not (name == "max_bounces_negative" and entry in NO_MAX_BOUNCES)
    out = [(name, BAD[name]) for name in BAD if has(name)]
    out += [(f"{a}+{b}", {**BAD[a], **BAD[b]}) for a, b in PAIRS if has(a) and has(b)]
    return out


_keep = []


def call(L, entry, o=1, d=1, out=1, n_rays=8, rays_per_pixel=1, n_pixels=8, max_bounces=10, flags=0, key_first=0, key_stride=1):
    """The entry point with a valid table of 8 rays over 8 pixels, but for what the case changes; returns (rc, message).
    o, d, out: None or any non-null address -- nothing here gets as far as reading them."""
    scene = np.zeros(1 << 16, np.uint8)
    scene[:4].view(np.int32)[0] = NO_SUCH_DEVICE  # rt_scene::device: hipSetDevice refuses it, nothing after it runs
    _keep.append(scene)
    ptr = lambda x: None if x is None else ctypes.c_void_p(scene.ctypes.data)
    head = (ctypes.c_void_p(scene.ctypes.data), n_rays, ptr(o), ptr(d), None, rays_per_pixel, n_pixels)
    if entry in PLAIN:
        rc = getattr(L, entry)(*head, max_bounces, 1, flags, ptr(out), None, None)
    elif entry in KEYED:
        rc = getattr(L, entry)(*head, max_bounces, 1, key_first, key_stride, flags, ptr(out), None, None)
    else:
        rc = getattr(L, entry)(*head, key_first, key_stride, flags, ptr(out), None, None, None)
    return rc, L.rt_last_error().decode()


@pytest.fixture(scope="module")
def lib():
    from rtcuda_amd import api
    return api.lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_golden_file_covers_every_case(golden):
    assert sorted(golden) == sorted(ENTRY_POINTS)
    for entry in ENTRY_POINTS:
        assert sorted(golden[entry]) == sorted(name for name, _ in cases(entry)), entry
        singles = [n for n in golden[entry] if "+" not in n]
        assert len(singles) >= 13 and len(golden[entry]) - len(singles) >= 2
        for name, msg in golden[entry].items():
            assert msg.startswith(entry + ": "), (name, msg)


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_refusals_are_the_recorded_messages(lib, golden, entry):
    for name, changed in cases(entry):
        rc, msg = call(lib, entry, **changed)
        assert rc != 0 and msg == golden[entry][name], (entry, name, msg)


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_the_first_check_in_order_wins(lib, golden, entry):
    """Of two bad arguments the caller is told about the one whose check comes first -- the message of that single case."""
    seen = 0
    for a, b in PAIRS:
        if f"{a}+{b}" not in golden[entry]:
            continue
        rc, msg = call(lib, entry, **{**BAD[a], **BAD[b]})
        assert rc != 0 and msg == golden[entry][a] and msg != golden[entry][b], (entry, a, b, msg)
        seen += 1
    assert seen >= 2
