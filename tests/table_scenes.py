"""Scenes with large shading tables: more than 64 materials or lights, up to the C-ABI's limits.  TEST HELPER.

Every BASELINE scene has at most 6 materials and 16 lights, so every one of them renders with the shading tables staged in
LDS (kLdsTable = 64 in rtcuda_amd.hip).  The recipes here start from the full-BSDF bunny and make a wrong table index
VISIBLE: every material and every light is distinct from its neighbours, the highest material indices sit on the walls the
camera sees, and the highest light indices are area lights on the visible ceiling -- so a table offset computed from the
wrong count, a table row written from the wrong source or a packed id one bit short changes the image.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from rtcuda_amd import scenes

MAX_MATS, MAX_LIGHTS = 65535, 32766  # rt_scene_create's limits: 16-bit material id, light + 1 below the sign bit
N_WALLS = 10                         # the Cornell box's triangles follow the bunny's in cornell_bunny()
# wall triangles that carry the highest material indices, highest first: left, right, floor and back wall (not the ceiling,
# which the light grid covers in part)
TOP_WALLS = (0, 1, 2, 3, 8, 9, 4, 5)
GRID = (0.35, 0.65, -0.35, -0.65)    # x0, x1, z0, z1 of the ceiling's light grid (the reference's light is 0.4 .. 0.6)
GRID_Y = 0.999
MAX_AREA = 128                       # area-light triangles at most; the other lights are point lights
AREA_POWER, POINT_POWER = 0.6, 0.2   # total L * area of the grid (the reference's 15 * 0.04) and total point intensity


def tab_dwords(n_mats: int, n_lights: int) -> int:
    """Size of a scene's shading tables in dwords (rt_scene_create: 5 per material, 8 + 12 + 4 per light)."""
    return 5 * n_mats + 24 * n_lights


def lds_tables(n_mats: int, n_lights: int) -> bool:
    """Whether rt_render_shard stages the tables in LDS (kLdsTable)."""
    return n_mats <= 64 and n_lights <= 64


def n_area_lights(n_lights: int) -> int:
    return min(MAX_AREA, max(2, n_lights // 2), n_lights)


def _materials(n: int, rng) -> np.ndarray:
    """n distinct materials: seeded albedo, mostly matte, some mirror, some glass of varied IOR."""
    mats = np.zeros(n, dtype=scenes.MATERIAL_DTYPE)
    mats["albedo"] = rng.uniform(0.15, 0.9, (n, 3)).astype(np.float32)
    kind = rng.uniform(size=n)
    mats["type"] = np.where(kind < 0.7, scenes.MATTE, np.where(kind < 0.85, scenes.MIRROR, scenes.GLASS))
    mats["ior"] = np.where(mats["type"] == scenes.GLASS, rng.uniform(1.2, 2.2, n), 0.0).astype(np.float32)
    return mats


def _grid_triangles(n: int) -> np.ndarray:
    """n triangles tiling the light grid on the ceiling (two per cell, cells in rows of up to 8), facing down like the
    reference's light triangles."""
    cells = -(-n // 2)
    nx = min(cells, 8)
    nz = -(-cells // nx)
    x0, x1, z0, z1 = GRID
    xs = np.linspace(x0, x1, nx + 1, dtype=np.float32)
    zs = np.linspace(z0, z1, nz + 1, dtype=np.float32)
    y = np.float32(GRID_Y)
    out = []
    for j in range(nz):
        for i in range(nx):
            a, b = xs[i], xs[i + 1]
            c, d = zs[j], zs[j + 1]
            out.append((a, y, c, b, y, c, b, y, d))
            out.append((a, y, c, a, y, d, b, y, d))
    return np.array(out[:n], dtype=np.float32)


def table_scene(n_mats: int, n_lights: int, seed: int = 0) -> scenes.SceneArrays:
    """The full-BSDF bunny with n_mats materials and n_lights lights (n_mats >= 8, n_lights >= 2).

    * Bunny triangle i has material (i * 7919) % n_mats, so every index is used; the eight visible wall triangles carry
      n_mats - 1, n_mats - 2, ... (TOP_WALLS), the ceiling and the light triangles the spread of the rest.
    * The reference's two light triangles become a grid of n_area_lights(n_lights) small area lights; the other lights are
      point lights inside the box.  Light indices are permuted against triangle order, and the highest ones (n_lights - 1
      first) are area lights of the grid.
    * Radiances are distinct and scaled with the counts: the total power stays the reference light's.
    """
    assert 8 <= n_mats <= MAX_MATS and 2 <= n_lights <= MAX_LIGHTS
    rng = np.random.default_rng([seed, n_mats, n_lights])
    base = scenes.cornell_bunny("full_bsdf")
    n_bunny = base.n_tris - N_WALLS - 2
    n_area = n_area_lights(n_lights)
    n_point = n_lights - n_area
    tris = np.concatenate([base.tris[:n_bunny + N_WALLS], _grid_triangles(n_area)])
    mat = np.empty(len(tris), np.int32)
    mat[:n_bunny] = (np.arange(n_bunny, dtype=np.int64) * 7919) % n_mats
    walls = n_bunny + np.arange(N_WALLS)
    mat[walls] = (np.arange(N_WALLS, dtype=np.int64) * 7919 + 3) % n_mats
    for k, w in enumerate(TOP_WALLS):
        mat[n_bunny + w] = n_mats - 1 - k
    mat[n_bunny + N_WALLS:] = (np.arange(n_area, dtype=np.int64) * 104729 + 11) % n_mats

    # light indices: the top half of the area lights take the highest indices, the rest fall anywhere below
    top = max(1, n_area // 2)
    rest = rng.choice(n_lights - top, size=n_area - top, replace=False)
    area_idx = np.concatenate([np.arange(n_lights - top, n_lights), rest])
    rng.shuffle(area_idx)  # which grid triangle gets which index
    lights = np.zeros(n_lights, dtype=scenes.LIGHT_DTYPE)
    tri_light = np.full(len(tris), -1, np.int32)
    cell_area = np.float32((GRID[1] - GRID[0]) * (GRID[2] - GRID[3]) / (2 * -(-n_area // 2)))
    for k, li in enumerate(area_idx):
        ti = n_bunny + N_WALLS + k
        L = AREA_POWER / (cell_area * n_area) * rng.uniform(0.5, 1.5, 3)
        lights[li] = (scenes.AREA_LIGHT, (0, 0, 0), ti, L)
        tri_light[ti] = li
    point_idx = np.setdiff1d(np.arange(n_lights), area_idx)
    assert len(point_idx) == n_point
    if n_point:
        pos = rng.uniform((0.08, 0.25, -0.92), (0.92, 0.95, -0.08), (n_point, 3))
        col = POINT_POWER / n_point * rng.uniform(0.3, 1.7, (n_point, 3))
        lights["type"][point_idx] = scenes.POINT_LIGHT
        lights["pos"][point_idx] = pos.astype(np.float32)
        lights["L"][point_idx] = col.astype(np.float32)
        lights["tri"][point_idx] = -1
    return scenes.SceneArrays(tris=np.ascontiguousarray(tris, np.float32), tri_material=mat, tri_light=tri_light,
                              materials=_materials(n_mats, rng), lights=lights, name=f"tables_{n_mats}x{n_lights}",
                              meta={"n_bunny": n_bunny, "n_area": n_area, "seed": seed})


def padded(arrays: scenes.SceneArrays, n_mats: int) -> scenes.SceneArrays:
    """The same scene with never-referenced materials appended up to n_mats.  Their values are distinct and implausible
    (albedo above 1, IOR 9, every type), so a renderer that reads one of them shows it; nothing in the estimator reads the
    material COUNT, so the padded scene must render bit for bit like the original -- while its tables leave LDS at 65."""
    n0 = len(arrays.materials)
    assert n_mats >= n0
    k = np.arange(n_mats - n0)
    extra = np.zeros(n_mats - n0, dtype=scenes.MATERIAL_DTYPE)
    extra["albedo"] = np.stack([1.5 + (k % 97) / 97.0, 2.0 + (k % 89) / 89.0, 3.0 + (k % 83) / 83.0], axis=1)
    extra["ior"] = 9.0
    extra["type"] = k % 3
    return dataclasses.replace(arrays, materials=np.concatenate([arrays.materials, extra]),
                               name=f"{arrays.name}_pad{n_mats}")
