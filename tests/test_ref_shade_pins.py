"""The oracle's shading functions against the REFERENCE'S OWN statements, row by row and bit for bit.  CPU only.

tests/golden/ref_shade_fixture.npz holds, per function, a table of inputs and what the reference's source -- compiled for
the CPU under oracle/ref_shim.h, called one function at a time by oracle/ref_shade_driver.cpp -- returned for each row, as
32-bit patterns (tests/golden/make_ref_shade_fixture.py; the row layouts are listed in the driver).  The tables hold random
unit vectors and the edges (tests/shade_scenes.py shade_tables): dot(wo, n) of exactly 0 and +-1, the critical angle to
within an ulp on either side, ior 1, a shading point on a point light, wi in the plane of the light triangle, zero-area
light triangles, p components of 0, -0, +-1/32 and their neighbours, negative p, uniforms of 2^-33 and 1.0, and every class
of (f_pdf, g_pdf) the int parameter of power_heuristic distinguishes below 2^31.

Every output word must be equal as an integer; a NaN must be a NaN (its payload is the compiler's choice).  Where a row
supplies uniforms the fixture holds the raw draws and the oracle's XORWOW is started from a state that makes exactly those
draws next (shade_scenes.xorwow_state_for), so the oracle's own generator and uniform conversion are in the loop and the
number of draws a function consumes is compared too."""
import os

import numpy as np
import pytest

import shade_scenes as ss

FIXTURE = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_shade_fixture.npz"))
WEYL = 362437


def _canon(words):
    """NaN payload aside: every NaN pattern -> one."""
    w = np.array(words, np.uint32).reshape(-1)
    w[np.isnan(w.view(np.float32))] = 0x7FC00000
    return w


def _f(words):
    return np.ascontiguousarray(words, np.uint32).view(np.float32)


def _material(words):
    m = np.zeros(1, dtype=ss.scenes.MATERIAL_DTYPE)
    m["albedo"], m["ior"], m["type"] = _f(words[0:3]), _f(words[3:4])[0], int(words[4])
    return m


def _state(raws):
    return ss.xorwow_state_for([int(r) for r in raws])


def _draws(state):
    """Draws made since xorwow_state_for's state (d = 0): d advances by the Weyl constant each."""
    return np.uint32((int(state[0]) * pow(WEYL, -1, 1 << 32)) % (1 << 32))


def _bits(*parts):
    return np.concatenate([np.atleast_1d(np.asarray(p)).view(np.uint32) if np.asarray(p).dtype == np.float32
                           else np.atleast_1d(np.asarray(p, np.uint32)) for p in parts])


def _light(w):
    return int(w[0]), _f(w[1:4]), _f(w[4:7]), _f(w[7:16])


def _row(o, func, w):
    """The oracle's output words for one input row."""
    if func == "sample_f":
        st = _state(w[11:13])
        out = o.sample_f(_material(w), _f(w[5:8]), _f(w[8:11]), st)
        return _bits(out, _draws(st))
    if func == "get_f":
        r, out = o.get_f(_material(w), _f(w[5:8]), _f(w[8:11]), _f(w[11:14]))
        return _bits(np.uint32(r), out)
    if func == "sample_Li":
        st = _state(w[19:21])
        r, out = o.sample_Li(*_light(w), _f(w[16:19]), st)
        return _bits(np.uint32(r), out, _draws(st))
    if func == "pdf_Li":
        return _bits(o.pdf_Li(*_light(w), _f(w[16:19]), _f(w[19:22])))
    if func == "sample_p":
        st = _state(w[9:11])
        return _bits(o.sample_p(_f(w[0:9]), st), _draws(st))
    if func == "intersect":
        hit, tuv = o.triangle_intersect(_f(w[0:9]), _f(w[9:12]), _f(w[12:15]), float(_f(w[15:16])[0]))
        return _bits(np.uint32(hit), tuv)
    if func == "offset_ray_origin":
        return _bits(o.offset_ray_origin(_f(w[0:3]), _f(w[3:6])))
    if func == "power_heuristic":
        f, g = _f(w[0:2])
        return _bits(np.float32(o.lib.orc_power_heuristic(float(f), float(g))))
    if func == "same_hemisphere":
        return _bits(np.uint32(o.same_hemisphere(_f(w[0:3]), _f(w[3:6]), _f(w[6:9]))))
    if func == "reflect":
        return _bits(o.reflect(_f(w[0:3]), _f(w[3:6])))
    if func == "refract":
        eta, cos = _f(w[6:8])
        return _bits(o.refract(_f(w[0:3]), _f(w[3:6]), eta, cos))
    if func == "uniform_sample_sphere":
        st = _state(w[0:2])
        return _bits(o.uniform_sample_sphere(st), _draws(st))
    if func == "get_ray":
        x, y = _f(w[12:14])
        return _bits(o.camera_get_ray(_f(w[0:12]), float(x), float(y)))
    raise KeyError(func)


@pytest.mark.parametrize("func", list(ss.FUNCTIONS.values()))
def test_oracle_function_equals_the_reference_on_every_row(oracle, func):
    rows, want = FIXTURE["in_" + func], FIXTURE["out_" + func]
    fid = [k for k, v in ss.FUNCTIONS.items() if v == func][0]
    assert rows.shape[1] == ss.WORDS_IN[fid] and want.shape == (len(rows), ss.WORDS_OUT[fid]) and len(rows) >= 600
    bad = []
    for k in range(len(rows)):
        got = _canon(_row(oracle, func, rows[k]))
        if not np.array_equal(got, _canon(want[k])):
            bad.append((k, rows[k].tolist(), got.tolist(), _canon(want[k]).tolist()))
    assert not bad, (len(bad), bad[:3])


def test_the_tables_hold_the_edges_they_claim():
    """The edge rows are in the committed fixture (not only in the generator), and they do what they are there for."""
    f32 = lambda a: np.ascontiguousarray(a).view(np.float32)
    # offset_ray_origin: both signs and the |p| < 1/32 branch in every coordinate, 0, -0 and +-1/32 exactly
    p = f32(FIXTURE["in_offset_ray_origin"][:, 0:3])
    for c in range(3):
        assert (p[:, c] < 0).sum() > 200 and (p[:, c] > 0).sum() > 200
        assert ((np.abs(p[:, c]) < 1 / 32) & (p[:, c] != 0)).sum() > 100 and (np.abs(p[:, c]) >= 1 / 32).sum() > 100
    bits = FIXTURE["in_offset_ray_origin"][:, 0]
    for v in (0.0, -0.0, 1 / 32, -1 / 32):
        assert (bits == np.float32(v).view(np.uint32)).any(), v
    # sample_f: all three materials; glass rows that reflect totally, that reflect by Fresnel and that refract; ior 1, < 1, > 2
    rows, out = FIXTURE["in_sample_f"], FIXTURE["out_sample_f"]
    kind, ior, draws = rows[:, 4], f32(rows[:, 3]), out[:, 10]
    assert {0, 1, 2} == set(kind.tolist())
    glass = kind == 2
    assert (glass & (draws == 0)).sum() > 20 and (glass & (draws == 1)).sum() > 100     # total internal reflection draws nothing
    assert (glass & (ior == 1.0)).any() and (glass & (ior < 1.0)).any() and (glass & (ior > 2.0)).any()
    assert ((kind == 0) & (draws == 2)).sum() > 100 and ((kind == 1) & (draws == 0)).sum() > 100
    d = np.einsum("nk,nk->n", f32(rows[:, 5:8]).astype(np.float64), f32(rows[:, 8:11]).astype(np.float64))
    assert (d == 0).sum() >= 30 and (d == 1).sum() >= 6 and (d == -1).sum() >= 6
    # uniforms of 2^-33 (raw 0) and 1.0 (raw 2^32 - 1) reach every sampling function
    for name, col in (("sample_f", 11), ("sample_Li", 19), ("sample_p", 9), ("uniform_sample_sphere", 0)):
        r = FIXTURE["in_" + name][:, col:col + 2]
        assert (r == 0).any() and (r == 0xFFFFFFFF).any(), name
    assert ss.uniform_of([0, 0xFFFFFFFF]).tolist() == [2.0 ** -33, 1.0]
    # sample_Li: a shading point ON a point light (t = 0) and zero-area light triangles (pdf inf or NaN)
    rows, out = FIXTURE["in_sample_Li"], FIXTURE["out_sample_Li"]
    on_light = (rows[:, 0] == 0) & (rows[:, 1:4] == rows[:, 16:19]).all(axis=1)
    assert on_light.sum() >= 2 and (f32(out[on_light, 7]) == 0).all()
    assert (~np.isfinite(f32(out[:, 8]))).sum() >= 2
    # power_heuristic: g below 1, exact squares, wrapped squares, negative g
    g = f32(FIXTURE["in_power_heuristic"][:, 1])
    assert ((np.abs(g) < 1).sum() > 100 and ((g >= 1) & (g < 46341)).sum() > 100 and (g >= 46341).sum() > 100 and (g <= -1).sum() > 100)
    assert np.abs(g).max() < 2.0 ** 31
    # refract: rows on either side of the critical angle (a NaN past it, a finite direction before it)
    nan = np.isnan(f32(FIXTURE["out_refract"])).any(axis=1)
    assert nan[-70:].any() and (~nan[-70:]).any()
