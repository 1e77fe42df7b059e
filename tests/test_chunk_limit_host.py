"""CPU tests of the limit of a run over background pixels in k_paths<PathsBg>'s GEN block (rtcuda_amd/csrc/rt_slot_chunks.h through
librt_hostcheck.so): one generation fixed before the run, against the stop tests the loop used to make turn by turn."""
import ctypes
import os

import numpy as np
import pytest

G_MAX = GEN_MAX = 2047  # a slot's chain has at most 2 047 camera rays (rt_slot_chunks.h), so G and gen stay within it


@pytest.fixture(scope="module")
def L():
    from rtcuda_amd import api
    api.build()
    lib = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    ci, cu, vp = ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p
    lib.rt_slot_chunk_next_multiple.argtypes = [cu, cu]
    lib.rt_slot_chunk_next_multiple.restype = cu
    lib.rt_slot_chunk_run_limit.argtypes = [cu, cu, ci, ci, cu]
    lib.rt_slot_chunk_run_limit.restype = cu
    lib.rt_slot_chunk_run_limit_check.argtypes = [cu, cu, vp]
    lib.rt_slot_chunk_run_limit_check.restype = None
    lib.rt_slot_chunk_ends.argtypes = [cu, cu, ci]
    return lib


def test_every_run_stops_where_the_per_turn_tests_stopped_it(L):
    """Every G in 1 .. 2 047, every gen in 0 .. 2 047, g_stop in {gen + 1, the next multiple of G - 1, that multiple, that
    multiple + 1, 2 047} (a lane only runs with gen < g_stop), dealt and not, can_loop and not: walking gen upward over
    background pixels under the old condition -- can_loop, gen < g_stop, no chunk's end (is_multiple per turn) -- stops at the
    generation at which `gen < run_limit` stops it."""
    out = np.zeros(4, np.int64)
    L.rt_slot_chunk_run_limit_check(1, G_MAX, out.ctypes.data)
    runs, bad, first_g, first_gen = (int(v) for v in out)
    assert bad == 0, f"{bad} of {runs} runs stop elsewhere; the first: G = {first_g}, gen = {first_gen}"
    # 5 values of g_stop, fewer where gen < g_stop fails (the next multiple - 1 is gen itself) or 2 047 is not above gen
    assert 4 * 3 * G_MAX * (GEN_MAX + 1) < runs <= 4 * 5 * G_MAX * (GEN_MAX + 1)


def test_the_walks_of_the_check_are_the_rules(L):
    """The exhaustive check compares two walks inside the library; here a sample of them is walked in Python from the rules
    alone (a multiple of G by `%`), so that the check cannot agree with itself for the wrong reason."""
    rng = np.random.default_rng(7)
    cases = [(1, 0), (1, 2046), (2, 1), (3, 2045), (2047, 0), (2047, 2046), (2046, 2045), (1024, 1023), (1024, 1024)]
    cases += [(int(g), int(x)) for g, x in zip(rng.integers(1, G_MAX + 1, 300), rng.integers(0, GEN_MAX + 1, 300))]
    for G, gen in cases:
        nxt = (gen // G + 1) * G
        assert L.rt_slot_chunk_next_multiple(gen, G) == nxt, (G, gen)
        for g_stop in (gen + 1, nxt - 1, nxt, nxt + 1, 2047):
            if not gen < g_stop:
                continue
            for dealt in (0, 1):
                for can_loop in (0, 1):
                    g = gen
                    while True:  # the loop as it was: one turn, then the four tests
                        g += 1
                        if not (can_loop and g < g_stop and not (dealt and g % G == 0)):
                            break
                    limit = L.rt_slot_chunk_run_limit(gen, g_stop, dealt, can_loop, G)
                    assert max(gen + 1, limit) == g, (G, gen, g_stop, dealt, can_loop, limit)
                    assert limit > gen  # a lane that runs makes its first turn with gen < limit


def test_the_next_multiple_needs_no_division_for_any_pair(L):
    """next_multiple for every (gen, G) of the range, against integer division."""
    gen = np.arange(GEN_MAX + 1, dtype=np.uint64)
    for G in range(1, G_MAX + 1):
        mul = (2 ** 31 + G - 1) // G  # next_multiple_mul
        got = ((((2 * gen + 1) * np.uint64(mul)) >> np.uint64(32)) + np.uint64(1)) * np.uint64(G)
        assert np.array_equal(got, (gen // np.uint64(G) + np.uint64(1)) * np.uint64(G)), G
    for G, g in ((1, 0), (1, 2047), (2047, 2047), (2047, 2046), (7, 48), (7, 49), (64, 63), (64, 64)):
        assert L.rt_slot_chunk_next_multiple(g, G) == (g // G + 1) * G
        assert bool(L.rt_slot_chunk_ends(L.rt_slot_chunk_next_multiple(g, G), G, 0))
