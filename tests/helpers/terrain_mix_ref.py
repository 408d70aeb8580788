"""The small sub-terrain mix and the planted origins that tests/test_terrain_mix.py (CPU: the oracle alone) and
tests/test_gpu_terrain_mix.py (the kernels) share.

small_mix(): 2 rows x 6 columns, one column per type of isaaclab_rough_terrains_cfg, 1 m border, 0.05 m cells:
361 x 1001 cells.  Row 0 is generated at difficulty 0 .. 0.02 and row 1 at 0.98 .. 1 (two one-row runs of the generator
stitched along their shared 0-height edge), so the hard row has steps of 0.23 m, boxes of +-0.2 m and slopes of 0.4.

contact_case(name): a (2, 2) origin table planted on the hard row, for the 128-env teacher-forced contact runs.
"""
from __future__ import annotations

import functools

import numpy as np

import terrain_ref as TR
from h12env import terrain as T
from h12env.cfg import isaaclab_rough_terrains_cfg

SEED = 11
COLS = ("pyramid_stairs", "pyramid_stairs_inv", "boxes", "random_rough", "hf_pyramid_slope", "hf_pyramid_slope_inv")
EASY, HARD = (0.0, 0.02), (0.98, 1.0)


def small_cfg(rows=1, difficulty=(0.0, 1.0)):
    g = isaaclab_rough_terrains_cfg()
    assert tuple(g.sub_terrains) == COLS
    for s in g.sub_terrains.values():
        s.proportion = 1.0
    g.num_rows, g.num_cols, g.border_width, g.difficulty_range = rows, len(COLS), 1.0, difficulty
    return g


@functools.lru_cache(maxsize=None)
def small_mix() -> T.Terrain:
    a, b = T.generate(small_cfg(1, EASY), SEED), T.generate(small_cfg(1, HARD), SEED + 1)
    assert a.type_names == list(COLS) and b.type_names == list(COLS)
    rs = a.hscale
    bp, sp = int(round(1.0 / rs)), int(round(8.0 / rs))
    assert a.shape == b.shape == (sp + 1 + 2 * bp, len(COLS) * sp + 1 + 2 * bp)
    assert not a.heights[bp + sp].any() and not b.heights[bp].any()     # the edge the two rows share is 0 in both
    H = np.concatenate([a.heights[:bp + sp], b.heights[bp:]], axis=0)
    org = np.concatenate([a.origins, b.origins], axis=0)
    org[0, :, 0] -= 4.0
    org[1, :, 0] += 4.0
    return T.Terrain(np.ascontiguousarray(H), rs, -8.0 - bp * rs, a.y0, org, sub_names=a.sub_names,
                     types=np.concatenate([a.types, b.types]), difficulty=np.concatenate([a.difficulty, b.difficulty]),
                     type_names=list(COLS))


def args(t: T.Terrain):
    return t.heights, t.hscale, t.x0, t.y0


def sub_origin(t: T.Terrain, row: int, name: str) -> np.ndarray:
    return t.origins[row, COLS.index(name)].astype(np.float64)


def step_height(t: T.Terrain, row: int, name: str) -> float:
    lo, hi = isaaclab_rough_terrains_cfg().sub_terrains[name].step_height_range
    return lo + t.difficulty[row, COLS.index(name)] * (hi - lo)


# ------------------------------------------------------------------ planted origins of the contact runs (hard row)
# offsets (dx, dy) from a sub-terrain's centre.  Stairs: the platform is |d| <= 1.5, ring k (from inside) spans
# 1.5 + 0.3 k .. 1.8 + 0.3 k, so 1.95 is the middle of a tread and 1.8 the top of a riser (its ramp is the fine cell
# below it).  Boxes: the platform is |d| <= 1, the walls lie at 0.175 + 0.45 j from the sub-terrain's edge, i.e. at
# centre + 0.225 + 0.45 j.  Slopes: the face between the platform and the border.
CONTACT_CASES = {
    "stairs": [("pyramid_stairs", 0.0, 0.0), ("pyramid_stairs", 1.95, 0.3), ("pyramid_stairs", 0.2, 1.8 - 0.025),
               ("pyramid_stairs_inv", -1.95, -0.4)],
    "boxes": [("boxes", 0.0, 0.0), ("boxes", 1.0, 0.3), ("boxes", 2.025, 1.8), ("boxes", -1.8, -2.025)],
    "slopes": [("hf_pyramid_slope", 2.4, 0.3), ("hf_pyramid_slope_inv", 0.2, -2.4), ("hf_pyramid_slope", 1.9, 1.9),
               ("random_rough", 1.0, -2.0)],
}
# the issue's list: platform, tread, astride a riser (stairs); platform, its wall, walls between boxes (boxes); slope
# faces along x, along y and on the pyramid's diagonal, and the 10 cm noise (slopes)


def planted_mix(name: str, origins: np.ndarray) -> TR.Planted:
    """The small mix as a planted terrain (padded with 1000.0 on both sides, as terrain_ref.planted) with the given
    origin table."""
    t = small_mix()
    buf = np.full(2 * TR.PAD + t.heights.size, TR.PAD_VALUE, np.float32)
    buf[TR.PAD:TR.PAD + t.heights.size] = t.heights.ravel()
    heights = buf[TR.PAD:TR.PAD + t.heights.size].reshape(t.shape)
    return TR.Planted(name, T.Terrain(heights, TR._f32(t.hscale), TR._f32(t.x0), TR._f32(t.y0),
                                      np.asarray(origins, np.float32), sub_names=t.sub_names, types=t.types,
                                      difficulty=t.difficulty), buf)


@functools.lru_cache(maxsize=None)
def whole_mix() -> TR.Planted:
    """... with the generator's own (2, 6) origin table: one origin per type and row."""
    return planted_mix("mix", small_mix().origins)


@functools.lru_cache(maxsize=None)
def contact_case(name: str) -> TR.Planted:
    """... with a (2, 2) origin table that holds the case's four points of the hard row, each at the mesh height under
    it."""
    t = small_mix()
    org = np.zeros((2, 2, 3), np.float32)
    for k, (sub, dx, dy) in enumerate(CONTACT_CASES[name]):
        c = sub_origin(t, 1, sub)
        x, y = np.float32(c[0] + dx), np.float32(c[1] + dy)
        org[k // 2, k % 2] = (x, y, TR.mesh_height(*args(t), x, y)[0])
    return planted_mix(name, org)


def contact_actions(name):
    rng = np.random.default_rng(57 + sum(map(ord, name)))
    return [(TR.ACTION_SCALE * rng.normal(size=(TR.N_CONTACT, 12))).astype(np.float32) for _ in range(TR.CONTACT_STEPS)]


# ------------------------------------------------------------------ planted poses of the scan test
@functools.lru_cache(maxsize=None)
def scan_case():
    """terrain_ref.scan_case's 67 poses (interior and tilted, on the lattice, outside every side and corner, straddling
    every edge, clipped) laid over a window of the hard row that spans the stairs / inverted stairs seam and the boxes:
    the window's geometry stands in for the planted grid's, the field is the whole small mix."""
    t = small_mix()
    base = TR.scan_case("relief")
    bt = base.p.terrain
    bx, by = base.p.extent
    # window: x over the hard row's sub-terrains, y from the stairs' platform edge to the boxes' far side
    wx0, wx1 = 0.2, 7.8
    wy0, wy1 = float(sub_origin(t, 1, "pyramid_stairs")[1]) + 1.0, float(sub_origin(t, 1, "boxes")[1]) + 3.9
    pos = base.pos.astype(np.float64).copy()
    pos[:, 0] = wx0 + (pos[:, 0] - bt.x0) / bx * (wx1 - wx0)
    pos[:, 1] = wy0 + (pos[:, 1] - bt.y0) / by * (wy1 - wy0)
    # the outside class leaves the field itself: past each side and corner by what it was past the planted grid's
    ex, ey = (t.shape[0] - 1) * t.hscale, (t.shape[1] - 1) * t.hscale
    for e in base.classes["outside"]:
        px, py = float(base.pos[e, 0]), float(base.pos[e, 1])
        if px < bt.x0:
            pos[e, 0] = t.x0 - (bt.x0 - px)
        elif px > bt.x0 + bx:
            pos[e, 0] = t.x0 + ex + (px - bt.x0 - bx)
        if py < bt.y0:
            pos[e, 1] = t.y0 - (bt.y0 - py)
        elif py > bt.y0 + by:
            pos[e, 1] = t.y0 + ey + (py - bt.y0 - by)
    quat = base.quat.copy()
    rng = np.random.default_rng(5)
    clip = base.classes["clip"]
    rest = np.setdiff1d(np.arange(TR.N_SCAN), clip)
    h = TR.mesh_height(*args(t), pos[:, 0], pos[:, 1])[0]
    pos[rest, 2] = h[rest] + 0.5 + rng.uniform(-0.3, 0.3, rest.size)
    wxr, wyr, *_ = TR.ray_geometry(pos[clip].astype(np.float32), quat[clip].astype(np.float32))
    hh = TR.mesh_height(*args(t), wxr, wyr)[0]
    pos[clip, 2] = [hh[0].max() + 0.5 + 1.3, hh[1].min() + 0.5 - 1.3, 0.5 * (hh[2].max() + hh[2].min()) + 0.5]
    pos[TR.ENV_B], quat[TR.ENV_B] = pos[TR.ENV_A], quat[TR.ENV_A]
    pos[TR.ENV_NEGQ], quat[TR.ENV_NEGQ] = pos[TR.ENV_Q], -quat[TR.ENV_Q]
    pos32, quat32 = pos.astype(np.float32), quat.astype(np.float32)
    ref = TR.scan_ref(*args(t), pos32, quat32)
    return pos32, quat32, base.classes, ref, TR.scan_bound(*args(t), pos32, ref)
