"""Views, placed scenes and moved scenes for the tests of the background rectangle (rt_background.h; numpy only).

tests/test_background_rect_host.py holds the rectangle of every input here to the product's CPU walks, exhaustively around its
edges; tests/test_gpu_background_views.py renders the same inputs on the device and compares the frames with the CPU oracle's
and with RT_BG_SKIP=0.  Both import the tables from here, so the CPU file and the GPU file use the same inputs.

The default view -- lookfrom (0.5, 0.5, 1.5), lookat (0.5, 0.5, 0), up (0, 1, 0), vfov 37.8 -- only ever cuts columns off the
Cornell box ((35, 0, 125, 90) at 160 x 90).  The views below give rectangles with rows cut off, rectangles that start at the
frame's first column or end at its last row, one a few columns wide, and rolled and oblique image planes.
"""
import dataclasses

import placed_scenes

DEFAULT_VIEW = ((0.5, 0.5, 1.5), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8)

# name -> (lookfrom, lookat, up, vfov)
VIEWS = {
    "oblique": ((1.6, 1.1, 1.4), (0.5, 0.4, -0.5), (0.0, 1.0, 0.0), 50.0),
    "rolled": ((0.5, 0.5, 1.5), (0.5, 0.5, 0.0), (0.5, 1.0, 0.2), 37.8),
    "rolled_oblique": ((-0.6, 1.3, 1.2), (0.5, 0.4, -0.5), (-0.4, 1.0, 0.3), 45.0),
    "scene_left": ((0.5, 0.5, 0.6), (0.9, 0.5, -0.5), (0.0, 1.0, 0.0), 30.0),
    "from_above": ((0.5, 2.5, -0.5), (0.5, 0.0, -0.5), (0.0, 0.0, -1.0), 40.0),
    "far_narrow": ((3.0, 2.0, 4.0), (0.5, 0.5, -0.5), (0.0, 1.0, 0.0), 15.0),
    "thin_column": ((0.5, 0.5, 1.5), (2.2, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8),
    "wide_fov": ((0.5, 0.5, 0.4), (0.5, 0.5, -1.0), (0.0, 1.0, 0.0), 120.0),
}

# name -> (scale per axis, shift per axis): the scene somewhere else, seen through placed_view()
PLACES = {
    "scale_100": ((100.0, 100.0, 100.0), (0.0, 0.0, 0.0)),
    "scale_1e-3": ((1e-3, 1e-3, 1e-3), (0.0, 0.0, 0.0)),
    "shift_30": ((1.0, 1.0, 1.0), (30.0, -20.0, 10.0)),
    "shift_300": ((1.0, 1.0, 1.0), (300.0, -200.0, 100.0)),
    "stretch_x_1e3": placed_scenes.PLACES["stretch_x_1e3"],
    "squash_y_1e-3": placed_scenes.PLACES["squash_y_1e-3"],
    "stretch_z_50_shift": ((1.0, 1.0, 50.0), (5.0, 5.0, -70.0)),
}
# the two views a placed scene is seen through: (lookfrom, lookat) before the move; up (0, 1, 0), vfov 37.8 (placed_camera)
PLACED_VIEWS = {"default": (DEFAULT_VIEW[0], DEFAULT_VIEW[1]), "oblique": (VIEWS["oblique"][0], VIEWS["oblique"][1])}

# name -> (uniform scale, shift): the scene moved under the FIXED default camera
MOVES = {
    "right_0.6": (1.0, (0.6, 0.0, 0.0)),
    "half": (0.5, (0.25, 0.25, -0.25)),
    "up_left": (1.0, (-0.45, 0.4, 0.0)),
    "double": (2.0, (-0.5, -0.5, 0.0)),
}


def view_camera(make_camera, name, aspect):
    """The 12 floats of a view: make_camera(lookfrom, lookat, up, vfov, aspect) is Oracle.camera or api.make_camera."""
    lookfrom, lookat, up, vfov = DEFAULT_VIEW if name == "default" else VIEWS[name]
    return make_camera(lookfrom, lookat, up, vfov, aspect)


def placed_view(make_camera, place, view, aspect):
    """The camera of PLACED_VIEWS[view] moved with the scene of PLACES[place]."""
    scale3, shift3 = PLACES[place]
    lookfrom, lookat = PLACED_VIEWS[view]
    return placed_scenes.placed_camera(make_camera, scale3, shift3, aspect, lookfrom=lookfrom, lookat=lookat)


def placed(arrays, place):
    return placed_scenes.placed(arrays, *PLACES[place])


def moved(arrays, move):
    """The SceneArrays of MOVES[move]: every vertex times the scale plus the shift, in float64, rounded once to fp32.  Only the
    triangles change -- what update() and rebuild() take -- so the scene's lights must be triangles (the bunny scenes' are)."""
    s, shift = MOVES[move]
    assert (arrays.lights["tri"] >= 0).all()
    return dataclasses.replace(arrays, tris=placed_scenes.placed(arrays, (s, s, s), shift).tris, name=f"{arrays.name}_{move}")


def rectangle(cam, w, h, arrays):
    """(x0, y0, x1, y1): the library's rectangle (rt_background_rect) for a camera, a frame and the bounds of the triangles."""
    from test_background_rect_host import bounds, rect
    return rect(cam, w, h, *bounds(arrays))


def whole(r, w, h):
    return tuple(r) == (0, 0, w, h)


def empty(r):
    return r[0] == r[2] and r[1] == r[3]


def area(r):
    return (r[2] - r[0]) * (r[3] - r[1])


def strictly_inside(r, w, h):
    """All four edges of the rectangle lie strictly inside the frame."""
    return 0 < r[0] < r[2] < w and 0 < r[1] < r[3] < h


def covers(outer, inner):
    """Every pixel of `inner` is a pixel of `outer`."""
    return empty(inner) or (outer[0] <= inner[0] and outer[1] <= inner[1] and outer[2] >= inner[2] and outer[3] >= inner[3])


def pixels_outside(r, other):
    """The number of pixels of rectangle `r` that are not pixels of `other`."""
    ix = max(0, min(r[2], other[2]) - max(r[0], other[0]))
    iy = max(0, min(r[3], other[3]) - max(r[1], other[1]))
    return area(r) - ix * iy
