"""CPU: the sub-terrain mix of the reference's Rough task (h12env.cfg.isaaclab_rough_terrains_cfg, h12env.terrain
generate_mix): the default terrain and every cfg dump are what they were, the layout, each shape against its published
definition, the exact up-sampling of the heightfield types, random mode, the condition of the GPU contact gate of
tests/test_gpu_terrain_mix.py (the oracle alone), and the way from the scripts' --terrain flag to the cfg and back out
of a run's env.yaml.
"""
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle as O
import terrain_mix_ref as M
import terrain_ref as TR
from forced import TOL_PHYS, n_threads, perturbed, phys_err
from h12env import cfg as K
from h12env import terrain as T
from h12env._abi import F as FIELDS
from h12env.startup import apply_to_arrays, startup_state

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "h1v2-isaac_amd"
sys.path[:0] = [str(PKG / "shims"), str(PKG / "scripts")]

RS = 0.05
SUB = 160          # fine cells per sub-terrain edge
BORDER = 400       # fine cells of the 20 m border


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def mix():
    return T.generate(K.isaaclab_rough_terrains_cfg(), 42)


def sub_block(t, r, c, sub=SUB, border=BORDER):
    return t.heights[border + r * sub:border + (r + 1) * sub + 1, border + c * sub:border + (c + 1) * sub + 1]


# ------------------------------------------------------------------ the default is what it was
# SHA-256 of the arrays, taken on the parent commit of the change that added cfg.sub_terrains (commit cba9529)
PARENT = {
    (0, "heights"): "191e180a531f70299a5c8c930c8eb1bf7df99478488c5832f3898abf37a06428",
    (42, "heights"): "b2191c9e5c43ece5610cadfff91d214f8d673872c3b48f4b716f7d185de20c3e",
    "origins": "0de262d8987639722d707bdd4b9669e93a4f97426e32be1adc85ef65ef53670c",
    (0, "levels"): "4ca2e3c2a4a04178047c3dbf010269bdc58fa5ea2bc217f1fae32d0deb7fec95",
    (42, "levels"): "308b602909ce21247f8284fd99e09be317ee441a21e60c6fc68e2ef70dc45a4b",
    "types": "b876a67266235bbd23594528ff41eb773dc29f8b77453fbc5cb7b299f5374413",
    "play_heights": "1885ed891baf5fa6921441f6c423948464f20f157028d261656fd638d4311cdd",
    "play_origins": "ef46dc21ac20df262bc50940e50ad0be2f6de9f7ff0e5ac599a983eb06617fcc",
    "play_levels": "e6bc763e4426a1a56fd9d3be46d7328d436b6c4571960c5494146517cab0eb2c",
    "play_types": "548d4dab4d49d198958ba98f96f5c5974097f5608b17a66bf3a04db8425bc78f",
}
# SHA-256 of json.dumps(class_to_dict(env cfg), sort_keys=True) of every registered task, taken on the same commit
PARENT_DUMPS = {
    "Isaac-Velocity-CaT-Flat-H12_12dof-Play-v0": "1d25cb11559e787fd2c7ea79984173d123ea2f75772867dac88affe6b2064e21",
    "Isaac-Velocity-CaT-Flat-H12_12dof-v0": "1eadff27d84cc61ae0bc804fce4e6d9cc0076f894fd2062ab1b09395bf6fdaa6",
    "Isaac-Velocity-Flat-H12_12dof-Play-v0": "fe3eb453e7ef5bed424c32c068d487e307c123261c4180f61f1b8ca43ee6af72",
    "Isaac-Velocity-Flat-H12_12dof-v0": "0375acde69df5de2c129a90ade1e632489565673370b3b96cd495d112623ac83",
    "Isaac-Velocity-Rough-H12_12dof-Play-v0": "ce97243fcbf59136e81babf000e5589f54e175a4e9136f7c3af5c3a950faa328",
    "Isaac-Velocity-Rough-H12_12dof-v0": "d9c71f2aa3f3b72001016cf6859f6eb9ecf6fb226a3d496ed6ad01a3bf715a69",
    "Isaac-Velocity-Rsl-H12_12dof-Play-v0": "5cc84f34c356da4b20ed580ad17b3995748cebd7fb88359ef6026fabb7033de4",
    "Isaac-Velocity-Rsl-H12_12dof-v0": "a6bbff0b533f73991eada575392fe94d4201a1170400b954ac829d34abc643bb",
}


def test_default_terrain_is_byte_for_byte_the_parents():
    g = K.TerrainGeneratorCfg()
    assert g.sub_terrains is None and g.raster_scale is None and g.difficulty_range == (0.0, 1.0)
    for seed in (0, 42):
        t = T.generate(g, seed)
        assert t.shape == (1201, 2001) and t.heights.dtype == np.float32
        assert (t.hscale, t.x0, t.y0) == (0.1, -60.0, -100.0)
        assert sha(t.heights) == PARENT[(seed, "heights")] and sha(t.origins) == PARENT["origins"]
        assert t.type_names is None and t.types is None and t.difficulty is None and t.sub_names is None
        lv, ty = T.initial_cells(4096, g, 5, seed)
        assert lv.dtype == ty.dtype == np.int32
        assert sha(lv) == PARENT[(seed, "levels")] and sha(ty) == PARENT["types"]
    g = K.H12RoughEnvCfg_PLAY().scene.terrain.terrain_generator
    assert (g.num_rows, g.num_cols, g.curriculum) == (5, 5, False)
    t = T.generate(g, 42)
    assert sha(t.heights) == PARENT["play_heights"] and sha(t.origins) == PARENT["play_origins"]
    lv, ty = T.initial_cells(50, g, None, 42)
    assert sha(lv) == PARENT["play_levels"] and sha(ty) == PARENT["play_types"]


def test_cfg_dumps_of_all_registered_tasks_are_unchanged():
    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from isaaclab.utils.dict import class_to_dict
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    ids = sorted(k for k in gym.registry if "H12" in k)
    assert ids == sorted(PARENT_DUMPS)
    for k in ids:
        d = class_to_dict(load_cfg_from_registry(k, "env_cfg_entry_point"))
        assert hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest() == PARENT_DUMPS[k], k
    d = class_to_dict(K.H12RoughEnvCfg())["scene"]["terrain"]["terrain_generator"]
    assert not {"sub_terrains", "difficulty_range", "raster_scale"} & set(d)


# ------------------------------------------------------------------ layout at the published mix
def test_published_mix_values():
    g = K.isaaclab_rough_terrains_cfg()
    assert (g.size, g.border_width, g.num_rows, g.num_cols) == ((8.0, 8.0), 20.0, 10, 20)
    assert (g.horizontal_scale, g.vertical_scale, g.slope_threshold, g.raster_scale) == (0.1, 0.005, 0.75, 0.05)
    assert g.curriculum and g.difficulty_range == (0.0, 1.0)
    s = g.sub_terrains
    assert list(s) == list(M.COLS)
    assert [s[k].proportion for k in s] == [0.2, 0.2, 0.2, 0.2, 0.1, 0.1]
    for k, inv in (("pyramid_stairs", False), ("pyramid_stairs_inv", True)):
        assert isinstance(s[k], K.MeshPyramidStairsTerrainCfg) and s[k].inverted is inv
        assert (s[k].step_height_range, s[k].step_width, s[k].platform_width, s[k].border_width) == \
            ((0.05, 0.23), 0.3, 3.0, 1.0)
    b = s["boxes"]
    assert isinstance(b, K.MeshRandomGridTerrainCfg)
    assert (b.grid_width, b.grid_height_range, b.platform_width) == (0.45, (0.05, 0.2), 2.0)
    r = s["random_rough"]
    assert isinstance(r, K.HfRandomUniformTerrainCfg)
    assert (r.noise_range, r.noise_step, r.border_width) == ((0.02, 0.10), 0.02, 0.25)
    for k, inv in (("hf_pyramid_slope", False), ("hf_pyramid_slope_inv", True)):
        assert isinstance(s[k], K.HfPyramidSlopedTerrainCfg) and s[k].inverted is inv
        assert (s[k].slope_range, s[k].platform_width, s[k].border_width) == ((0.0, 0.4), 2.0, 0.25)


def test_layout(mix):
    t = mix
    cols = [4, 4, 4, 4, 2, 2]
    assert t.type_names == [n for n, k in zip(M.COLS, cols) for _ in range(k)]
    assert t.sub_names == M.COLS and (t.types == np.repeat(np.arange(6), cols)[None, :]).all()
    assert t.shape == (2401, 4001) and t.heights.dtype == np.float32 and t.hscale == RS
    assert (t.x0, t.y0) == (-60.0, -100.0)
    H = t.heights
    assert not H[:BORDER + 1].any() and not H[-BORDER - 1:].any()          # the 20 m border and the grid's own edge
    assert not H[:, :BORDER + 1].any() and not H[:, -BORDER - 1:].any()
    assert not H[BORDER::SUB].any() and not H[:, BORDER::SUB].any()        # every sub-terrain's outer edge
    assert np.abs(H).max() > 1.0
    r, c = np.meshgrid(np.arange(10), np.arange(20), indexing="ij")
    assert (t.origins[..., 0] == -40.0 + 8.0 * r + 4.0).all() and (t.origins[..., 1] == -80.0 + 8.0 * c + 4.0).all()
    d = t.difficulty
    assert d.shape == (10, 20) and (d >= r / 10).all() and (d < (r + 1) / 10).all()
    assert len(np.unique(d)) == 200                                         # u is drawn per sub-terrain


def test_column_types_follow_the_cumulative_proportions():
    assert T.column_types([0.2, 0.2, 0.2, 0.2, 0.1, 0.1], 20).tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 + [4, 4, 5, 5]
    assert T.column_types([1, 1, 1, 1, 1, 1], 6).tolist() == [0, 1, 2, 3, 4, 5]
    assert T.column_types([3, 1], 4).tolist() == [0, 0, 0, 1]
    assert T.column_types([0.5, 0.5], 5).tolist() == [0, 0, 0, 1, 1]        # 2 / 5 + 0.001 < 0.5


# ------------------------------------------------------------------ stairs
def test_ring_count_does_not_hang_on_the_floating_point_floor():
    """Five rings of 0.3 m fit between the 1 m border and the 3 m platform.  A bare `//` counts by the rounding of the
    divisor (3.0 // 0.6 is 5.0 but 1.0 // 0.1 is 9.0, not 10.0); the count here is the same for every way of writing
    the same sizes."""
    s = K.MeshPyramidStairsTerrainCfg()
    assert 3.0 // 0.6 == 5.0 and 1.0 // 0.1 == 9.0
    assert T.stairs_ring_count(K.MeshPyramidStairsTerrainCfg(step_width=0.05, platform_width=5.0), 8.0) == 10
    assert T.stairs_ring_count(s, 8.0) == 5
    assert T.stairs_ring_count(K.MeshPyramidStairsTerrainCfg(step_width=0.15), 8.0) == 10
    assert T.stairs_ring_count(K.MeshPyramidStairsTerrainCfg(step_width=0.31), 8.0) == 4
    assert T.stairs_ring_count(K.MeshPyramidStairsTerrainCfg(platform_width=3.0 + 1e-12), 8.0) == 5


@pytest.mark.parametrize("row", [0, 9])
@pytest.mark.parametrize("col", [0, 4])
def test_stairs(mix, row, col):
    t = mix
    inverted = col == 4
    assert t.type_names[col] == ("pyramid_stairs_inv" if inverted else "pyramid_stairs")
    sign = -1.0 if inverted else 1.0
    step = 0.05 + t.difficulty[row, col] * (0.23 - 0.05)
    assert (0.05 if row == 0 else 0.212) <= step < (0.068 if row == 0 else 0.23)
    blk = sub_block(t, row, col)
    for axis in (blk[:, SUB // 2], blk[SUB // 2, :], blk[:, SUB // 2 + 7]):   # through the centre, and beside it
        assert (axis == axis[::-1]).all()
        half = axis[:SUB // 2 + 1].astype(np.float64) * sign
        # piecewise constant: 20 cells of border, then five treads of exactly step_width = 6 fine vertices (the tread's
        # own vertex on top of its riser and the five after it), then the platform
        levels, starts, counts = [], [], []
        for i, h in enumerate(half):
            if not levels or h != levels[-1]:
                levels.append(h), starts.append(i), counts.append(0)
            counts[-1] += 1
        assert len(levels) == 7 and levels[0] == 0.0
        assert starts == [0, 20, 26, 32, 38, 44, 50] and counts == [20, 6, 6, 6, 6, 6, 31]
        # every riser is one fine cell (between the last vertex of a tread and the first of the next) ...
        jumps = np.diff(levels)
        # ... and as high as the row's step, to float32
        assert np.abs(jumps - step).max() <= 2.0 ** -23 * 6 * step, (jumps, step)
        assert [np.float32(lv) for lv in levels] == [np.float32(k * step) for k in range(7)]
    # the platform is flat over platform_width (3 m: vertices 50 .. 110)
    plat = blk[50:111, 50:111]
    assert (plat == plat[0, 0]).all() and plat[0, 0] == np.float32(sign * 6 * step)
    assert (np.abs(blk[49, 50:111]) < abs(plat[0, 0])).all()
    # the origin: the platform's centre at its height, and the mesh says the same
    o = t.origins[row, col]
    assert o[2] == plat[0, 0]
    assert TR.mesh_height(t.heights, t.hscale, t.x0, t.y0, o[0], o[1])[0] == float(o[2])
    ix, iy = (o[0] - t.x0) / RS, (o[1] - t.y0) / RS
    assert (ix, iy) == (BORDER + row * SUB + 80, BORDER + col * SUB + 80)


def test_inverted_stairs_are_the_exact_negative():
    g = K.isaaclab_rough_terrains_cfg()
    up, inv = g.sub_terrains["pyramid_stairs"], g.sub_terrains["pyramid_stairs_inv"]
    for d in (0.0, 0.37, 1.0):
        a, oa = T.make_sub_terrain(up, g, d, None)
        b, ob = T.make_sub_terrain(inv, g, d, None)
        assert (a == -b).all() and oa == -ob and a.max() == oa > 0
        assert not np.signbit(b[0]).any()                                    # (no -0.0 on the shared edges)
    # the same holds for the sloped pyramid: truncation and rounding are symmetric
    up, inv = g.sub_terrains["hf_pyramid_slope"], g.sub_terrains["hf_pyramid_slope_inv"]
    for d in (0.21, 1.0):
        a, oa = T.make_sub_terrain(up, g, d, None)
        b, ob = T.make_sub_terrain(inv, g, d, None)
        assert (a == -b).all() and a.max() > 0 and oa == a.max() and ob == b.min() == -oa


# ------------------------------------------------------------------ boxes
@pytest.mark.parametrize("row", [0, 9])
def test_boxes(mix, row):
    t = mix
    col = 8
    assert t.type_names[col] == "boxes"
    g = 0.05 + t.difficulty[row, col] * (0.2 - 0.05)
    blk = sub_block(t, row, col).astype(np.float64)
    assert int(8.0 / 0.45) == 17
    # the frame: 0.175 m = 3.5 fine cells on every side, so vertices 0 .. 3 and 157 .. 160 are 0
    assert not blk[:4].any() and not blk[-4:].any() and not blk[:, :4].any() and not blk[:, -4:].any()
    # square j spans 3.5 + 9 j .. 12.5 + 9 j: its 9 x 9 fine vertices 4 + 9 j .. 12 + 9 j are constant, the wall to the
    # next square is the ramp of the one cell between them
    vals = np.zeros((17, 17))
    for i in range(17):
        for j in range(17):
            sq = blk[4 + 9 * i:13 + 9 * i, 4 + 9 * j:13 + 9 * j]
            assert sq.shape == (9, 9)
            inner = (60 <= 4 + 9 * i <= 100 - 8) and (60 <= 4 + 9 * j <= 100 - 8)   # wholly under the platform
            touches = (4 + 9 * i <= 100 and 12 + 9 * i >= 60) and (4 + 9 * j <= 100 and 12 + 9 * j >= 60)
            if not touches:
                assert (sq == sq[0, 0]).all(), (i, j)
                vals[i, j] = sq[0, 0]
            elif inner:
                assert (sq == np.float32(g)).all()
            vals[i, j] = sq[0, 0] if not touches else np.nan
    free = vals[~np.isnan(vals)]
    assert free.size > 200 and np.abs(free).max() <= g and len(np.unique(free)) == free.size
    assert free.min() < -0.5 * g and free.max() > 0.5 * g                     # U(-g, g), not U(0, g)
    assert np.abs(blk).max() <= np.float32(g)
    # the platform at +g over 2 m (vertices 60 .. 100), and the origin on it
    assert (blk[60:101, 60:101] == np.float32(g)).all()
    assert t.origins[row, col, 2] == np.float32(g)


# ------------------------------------------------------------------ slopes and noise
@pytest.mark.parametrize("row", [0, 9])
@pytest.mark.parametrize("col", [16, 18])
def test_slopes(mix, row, col):
    t = mix
    inverted = col == 18
    assert t.type_names[col] == ("hf_pyramid_slope_inv" if inverted else "hf_pyramid_slope")
    sign = -1.0 if inverted else 1.0
    slope = 0.4 * t.difficulty[row, col]
    blk = sub_block(t, row, col).astype(np.float64) * sign
    coarse = blk[::2, ::2]                                                   # the pixels the type was generated at
    units = coarse / 0.005
    assert np.abs(units - np.rint(units)).max() < 1e-4                       # integer multiples of vertical_scale
    assert not coarse[:3].any() and not coarse[-3:].any() and not coarse[:, :3].any() and not coarse[:, -3:].any()
    top = coarse.max()
    assert (coarse[30:51, 30:51] == top).all()                               # the platform: flat over 2 m
    assert t.origins[row, col, 2] == np.float32(sign * top)
    for axis in (coarse[:, 40], coarse[40, :]):                              # through the centre
        assert (axis == axis[::-1]).all()
        rise = np.diff(axis[3:41])
        face = axis[4:41] < top                                              # cells that end below the platform
        assert face.sum() >= (10 if row == 9 else 0)
        # the gradient is the row's slope to one vertical quantum per cell
        assert (np.abs(rise[face] - slope * 0.1) <= 0.005 + 1e-9).all(), (rise[face], slope)
        assert (rise[~face] >= 0).all() and (rise[~face] <= slope * 0.1 + 0.005 + 1e-9).all()
    if row == 9:
        assert 0.36 <= slope < 0.4 and top > 0.6


def test_noise(mix):
    t = mix
    for row in (0, 9):                                                       # the noise does not grow with the row
        blk = sub_block(t, row, 12)
        assert t.type_names[12] == "random_rough"
        coarse = blk[::2, ::2].astype(np.float64)
        assert coarse.shape == (81, 81)
        assert not coarse[:3].any() and not coarse[-3:].any() and not coarse[:, :3].any() and not coarse[:, -3:].any()
        units = np.rint(coarse[3:-3, 3:-3] / 0.005)
        assert sorted(np.unique(units)) == [4, 8, 12, 16, 20]
        assert np.abs(coarse[3:-3, 3:-3] - units * 0.005).max() < 1e-8
        assert t.origins[row, 12, 2] == np.float32(0.1)


# ------------------------------------------------------------------ up-sampling leaves the surface alone
@pytest.mark.parametrize("name", ["random_rough", "hf_pyramid_slope", "hf_pyramid_slope_inv"])
def test_upsampled_heightfield_is_the_same_surface(name):
    g = K.isaaclab_rough_terrains_cfg()
    sc = g.sub_terrains[name]
    fine, _ = T.make_sub_terrain(sc, g, 0.83, np.random.default_rng(3))
    coarse_g = K.isaaclab_rough_terrains_cfg()
    coarse_g.raster_scale = None
    coarse, _ = T.make_sub_terrain(sc, coarse_g, 0.83, np.random.default_rng(3))
    assert fine.shape == (161, 161) and coarse.shape == (81, 81) and fine.dtype == coarse.dtype == np.float64
    assert (fine[::2, ::2] == coarse).all()
    rng = np.random.default_rng(4)
    x, y = rng.uniform(0, 8, 1000), rng.uniform(0, 8, 1000)
    # 0.125 and 0.0625 stand in for 0.1 and 0.05: exact in float32, which mesh_height takes its cell size as
    hf, gxf, gyf = TR.mesh_height(fine, 0.0625, 0.0, 0.0, x * 0.625, y * 0.625)
    hc, gxc, gyc = TR.mesh_height(coarse, 0.125, 0.0, 0.0, x * 0.625, y * 0.625)
    assert np.abs(hf - hc).max() <= 1e-12
    assert np.abs(hc).max() > 0.05


# ------------------------------------------------------------------ random mode
def test_random_mode():
    g = K.isaaclab_rough_terrains_cfg()
    g.num_rows = g.num_cols = 20
    g.curriculum, g.border_width, g.raster_scale = False, 1.0, None          # (0.1 m cells keep this quick)
    t = T.generate(g, 5)
    assert t.type_names is None and t.types.shape == (20, 20) and t.shape == (1621, 1621)
    n = 400
    for k, p in enumerate([0.2, 0.2, 0.2, 0.2, 0.1, 0.1]):
        assert abs((t.types == k).sum() - n * p) <= 4 * np.sqrt(n * p * (1 - p)), (k, (t.types == k).sum())
    assert (t.difficulty >= 0).all() and (t.difficulty < 1).all() and t.difficulty.std() > 0.2
    assert abs(np.corrcoef(t.difficulty.ravel(), np.repeat(np.arange(20), 20))[0, 1]) < 0.2   # no curriculum
    assert not t.heights[10::80].any() and not t.heights[:, 10::80].any()
    t2 = T.generate(g, 5)
    assert sha(t2.heights) == sha(t.heights) and (t2.types == t.types).all() and (t2.difficulty == t.difficulty).all()
    assert (t2.origins == t.origins).all()
    t3 = T.generate(g, 6)
    assert (t3.types != t.types).any() and sha(t3.heights) != sha(t.heights)
    gp = K.enable_reference_rough_terrain(K.H12RoughEnvCfg_PLAY()).scene.terrain.terrain_generator
    assert (gp.num_rows, gp.num_cols, gp.curriculum) == (5, 5, False)
    assert T.generate(gp, 1).shape == (5 * 160 + 801, 5 * 160 + 801)


def test_curriculum_mode_repeats_and_seeds_differ():
    g = M.small_cfg(2)
    a, b, c = T.generate(g, 3), T.generate(g, 3), T.generate(g, 4)
    assert sha(a.heights) == sha(b.heights) and (a.difficulty == b.difficulty).all()
    assert sha(a.heights) != sha(c.heights)
    assert a.shape == (361, 1001)


# ------------------------------------------------------------------ the small mix of the GPU tests
def test_small_mix():
    t = M.small_mix()
    assert t.shape == (361, 1001) and t.hscale == 0.05 and (t.x0, t.y0) == (-9.0, -25.0)
    assert t.type_names == list(M.COLS)
    assert (t.difficulty[0] < 0.02).all() and (t.difficulty[1] >= 0.98).all()
    for c in range(6):
        for r in range(2):
            o = t.origins[r, c]
            assert (o[0], o[1]) == (-4.0 + 8.0 * r, -20.0 + 8.0 * c)
            h = TR.mesh_height(*M.args(t), o[0], o[1])[0]
            assert h == pytest.approx(float(o[2]), abs=0.1 + 1e-6)           # (heightfield types: the 2 x 2 m maximum)
    assert M.step_height(t, 1, "pyramid_stairs") > 0.226
    gx, gy = TR.slopes(t.heights, t.hscale)
    assert gx > 4.5 and gy > 4.5                                             # a 0.23 m riser over a 0.05 m cell
    # the planted origins sit where the case says
    p = M.contact_case("stairs")
    o = p.terrain.origins.reshape(4, 3)
    s = M.step_height(t, 1, "pyramid_stairs")
    assert o[0, 2] == pytest.approx(6 * s) and o[1, 2] == pytest.approx(4 * s)
    assert 4 * s < o[2, 2] < 5 * s                                           # astride: half-way up a riser's ramp
    assert o[3, 2] == pytest.approx(-4 * M.step_height(t, 1, "pyramid_stairs_inv"))
    assert (p.buf[:TR.PAD] == 1000.0).all() and (p.buf[-TR.PAD:] == 1000.0).all()
    assert (p.terrain.heights == t.heights).all()
    # the scan poses cross risers and box walls, clip at both ends, and leave the field on every side
    pos, quat, cls, ref, bound = M.scan_case()
    rows = ref.h.reshape(TR.N_SCAN, TR.SCAN_NY, TR.SCAN_NX)
    jump = np.abs(np.diff(rows, axis=2)).max(axis=(1, 2))
    assert (jump > 0.1).sum() >= 20, (jump > 0.1).sum()
    assert (ref.raw > 1 + bound).any() and (ref.raw < -1 - bound).any()
    ex, ey = 18.0, 50.0
    out = (ref.wx < t.x0) | (ref.wx > t.x0 + ex) | (ref.wy < t.y0) | (ref.wy > t.y0 + ey)
    assert out[cls["outside"][-8:]].all() and not out[cls["interior"]].any()
    # the fp32 restatement of the scan stays inside the a-priori bound on this field
    got = TR.scan32(p, pos, quat)
    frac = np.abs(got - ref.clipped) / bound
    print(f"\nsmall mix: scan32 worst |error| / bound {frac.max():.3f}")
    assert frac.max() <= 1.0


# ------------------------------------------------------------------ the GPU contact runs, oracle alone
@pytest.mark.parametrize("name", list(M.CONTACT_CASES))
def test_contact_runs_are_well_conditioned(model, name):
    """The condition of test_gpu_terrain_mix's contact gate (the probe of
    test_terrain_emulation.test_contact_runs_are_well_conditioned on the hard row of the small mix): an oracle run from
    a state perturbed by 1e-7 leaves TOL_PHYS of the unperturbed oracle on fewer than 0.75 % of the env-steps, half the
    1.5 % the gate allows, and both feet touch in at least 0.6 of the envs."""
    n = TR.N_CONTACT
    cfg = TR.contact_cfg(n)
    p = M.contact_case(name)
    t = p.terrain
    st = startup_state(cfg, n)
    O.set_terrain(t.heights, t.hscale, t.x0, t.y0, t.origins)
    env = O.OracleEnv(model, cfg.to_c(), n)
    apply_to_arrays(st, env.F, env.I)
    TR.plant_origins(p, env.F, st.terrain_cell)
    env.reset()
    org = env.F[FIELDS["ORIGIN"][0]:FIELDS["ORIGIN"][0] + 3].T
    assert {tuple(o) for o in org} == {tuple(o) for o in t.origins.reshape(-1, 3)}  # all four origins in use
    rng = np.random.default_rng(1)
    bad = 0
    both = np.zeros(n, bool)
    for k, a in enumerate(M.contact_actions(name)):
        F0, I0, obs0 = env.F.copy(), env.I.copy(), env.obs.copy()
        env.F[:] = perturbed(rng, F0, 1e-7)
        env.step(a, k + 1, n_threads=n_threads())
        Fp = env.F.copy()
        env.F[:], env.I[:], env.obs = F0, I0, obs0
        env.step(a, k + 1, n_threads=n_threads())
        bad += int((phys_err(Fp, env.F) > TOL_PHYS).sum())
        bits = (env.I[1] >> 13) & 0xFF
        both |= ((bits & 0x0F) != 0) & ((bits & 0xF0) != 0)
    share = bad / (n * TR.CONTACT_STEPS)
    print(f"\n{name}: {bad} of {n * TR.CONTACT_STEPS} env-steps leave TOL_PHYS under a 1e-7 perturbation "
          f"({share:.4f}); both feet in contact in {both.mean():.2f} of the envs")
    assert np.isfinite(env.F).all()
    assert share < 0.0075
    assert both.mean() >= 0.6


# ------------------------------------------------------------------ scripts, cfg round trip, log keys
def test_terrain_flag_reaches_the_cfg_and_overrides_reach_the_table():
    import train
    from isaaclab_tasks.utils.hydra import apply_overrides
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    args, rest = train.build_parser().parse_known_args(
        ["--task", "Isaac-Velocity-Rough-H12_12dof-v0", "--terrain", "isaaclab_rough",
         "env.scene.terrain.terrain_generator.num_rows=3",
         "env.scene.terrain.terrain_generator.sub_terrains.boxes.grid_width=0.5"])
    assert args.terrain == "isaaclab_rough"
    assert train.build_parser().parse_known_args([])[0].terrain == "project"
    env_cfg = load_cfg_from_registry(args.task, "env_cfg_entry_point")
    before = (env_cfg.scene.terrain.max_init_terrain_level, env_cfg.curriculum.terrain_levels)
    K.apply_terrain_choice(env_cfg, "project")
    assert env_cfg.scene.terrain.terrain_generator.sub_terrains is None
    K.apply_terrain_choice(env_cfg, args.terrain)
    apply_overrides(env_cfg, None, rest)
    g = env_cfg.scene.terrain.terrain_generator
    assert list(g.sub_terrains) == list(M.COLS) and g.raster_scale == 0.05
    assert g.num_rows == 3 and g.sub_terrains["boxes"].grid_width == 0.5
    assert (env_cfg.scene.terrain.max_init_terrain_level, env_cfg.curriculum.terrain_levels) == before == (5, True)
    assert env_cfg.to_c().terrain_size == 8.0
    c5 = K.enable_reference_rough_terrain(K.c5_cfg(64))
    assert c5.scene.terrain.terrain_generator.sub_terrains is not None and c5.events.add_base_mass is not None
    src = (PKG / "scripts" / "train.py").read_text()
    assert src.index("apply_terrain_choice(env_cfg, args.terrain)") < src.index("apply_overrides(env_cfg, agent_cfg")
    for script in ("play.py", "eval_policy.py"):
        s = (PKG / "scripts" / script).read_text()
        assert '"--terrain"' in s and "apply_terrain_choice" in s
    assert "terrain_from_run" in (PKG / "scripts" / "play.py").read_text()


def test_plane_tasks_refuse_the_flag():
    for cfg in (K.H12FlatEnvCfg(), K.H12RslEnvCfg(), K.H12CaTEnvCfg(), K.mujoco_cfg()):
        with pytest.raises(SystemExit, match="runs on the plane"):
            K.apply_terrain_choice(cfg, "isaaclab_rough")
        assert K.apply_terrain_choice(cfg, "project") is cfg and cfg.scene.terrain.terrain_generator is None
    with pytest.raises(ValueError, match="runs on the plane"):
        K.enable_reference_rough_terrain(K.H12FlatEnvCfg())
    # the script itself: the message, a failing exit status, and no env is built (this runs without a GPU)
    p = subprocess.run([sys.executable, str(PKG / "scripts" / "train.py"), "--task", "Isaac-Velocity-Flat-H12_12dof-v0",
                        "--terrain", "isaaclab_rough", "--headless"], capture_output=True, text=True, cwd=str(ROOT))
    assert p.returncode != 0 and "--terrain isaaclab_rough" in p.stderr and "runs on the plane" in p.stderr, p.stderr


def test_env_yaml_and_pickle_round_trip_the_table(tmp_path):
    import pickle

    import yaml

    from isaaclab.utils.io import dump_pickle, dump_yaml

    cfg = K.enable_reference_rough_terrain(K.H12RoughEnvCfg())
    g = cfg.scene.terrain.terrain_generator
    g.num_rows, g.num_cols = 2, 6
    g.sub_terrains["boxes"].grid_height_range = (0.05, 0.15)
    g.difficulty_range = (0.25, 0.75)
    run = tmp_path / "run"
    dump_yaml(str(run / "params" / "env.yaml"), cfg)
    dump_pickle(str(run / "params" / "env.pkl"), cfg)
    d = yaml.safe_load((run / "params" / "env.yaml").read_text())["scene"]["terrain"]["terrain_generator"]
    assert list(d["sub_terrains"]) == list(M.COLS) and d["raster_scale"] == 0.05 and d["difficulty_range"] == [0.25, 0.75]
    assert d["sub_terrains"]["pyramid_stairs_inv"]["inverted"] is True
    back = K.terrain_generator_from_dict(d)
    assert back == g
    with open(run / "params" / "env.pkl", "rb") as f:
        assert pickle.load(f).scene.terrain.terrain_generator == g
    assert sha(T.generate(back, 9).heights) == sha(T.generate(g, 9).heights)
    # play.py: the run's table on the Play task's own 5 x 5 grid without curriculum; a run without a table changes nothing
    play = K.H12RoughEnvCfg_PLAY()
    assert K.terrain_from_run(play, run) is True
    gp = play.scene.terrain.terrain_generator
    assert (gp.num_rows, gp.num_cols, gp.curriculum) == (5, 5, False)
    assert gp.sub_terrains == g.sub_terrains and gp.difficulty_range == (0.25, 0.75) and gp.raster_scale == 0.05
    plain = tmp_path / "plain"
    dump_yaml(str(plain / "params" / "env.yaml"), K.H12RoughEnvCfg())
    play = K.H12RoughEnvCfg_PLAY()
    assert K.terrain_from_run(play, plain) is False and play.scene.terrain.terrain_generator.sub_terrains is None
    assert K.terrain_from_run(K.H12FlatEnvCfg(), run) is False


def test_per_type_log_keys_only_with_a_mix():
    g = K.TerrainGeneratorCfg()
    g.num_rows, g.num_cols, g.border_width = 2, 6, 1.0
    lv, ty = T.initial_cells(64, g, 1, 0)
    assert T.level_log_weights(T.generate(g, 0), ty) == {}
    t = M.small_mix()
    w = T.level_log_weights(t, ty)
    assert list(w) == [f"Curriculum/terrain_levels/{n}" for n in M.COLS]
    for n, v in zip(M.COLS, w.values()):
        m = np.asarray(t.type_names)[ty] == n
        assert v.dtype == np.float32 and v @ lv == pytest.approx(lv[m].mean())
    assert list(T.level_log_weights(t, ty[:8])) == ["Curriculum/terrain_levels/pyramid_stairs"]   # no envs, no key
    one = T.generate(M.small_cfg(1), 0)
    one.type_names = ["boxes"] * 6
    assert T.level_log_weights(one, ty) == {}
