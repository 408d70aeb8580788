"""Heightfield terrain of the rough task (replaces IsaacLab's TerrainGenerator + TerrainImporter).

Restates the published algorithm of isaaclab.terrains (IsaacLab 2.1, not installed here -- parity of the
samples against it is unpinned, the layout and statistics follow it):

* ROUGH_TERRAINS_CFG (biped_tasks/utils/mdp/terrains.py:11-28): num_rows x num_cols sub-terrains of
  8 x 8 m, one type (HfRandomUniform, noise 0-2 cm in 5 mm steps), 20 m flat border, 0.1 m pixels,
  5 mm vertical scale.
* height_field_to_mesh: each sub-terrain is an (8/0.1 + 1)^2 pixel grid with a flat border of
  int(0.25/0.1) + 1 = 3 pixels; the inner pixels take random heights from {0, ..., 4} x 5 mm (the
  RectBivariateSpline up-sampling of random_uniform_terrain is the identity when the down-sampled scale
  equals the horizontal scale).  Sub-terrain origin: its centre at the maximum height of the central
  2 x 2 m.
* TerrainGenerator centres the whole grid on the world origin; TerrainImporter assigns env i the type
  floor(i / (N / num_cols)) and a random initial level in [0, max_init_terrain_level].

All sub-terrains are stitched into ONE heightfield (shared 0-height edges), which is what the kernels
sample (h12env_set_terrain).

With ``cfg.sub_terrains`` set (isaaclab_rough_terrains_cfg: upstream's ROUGH_TERRAINS_CFG) the grid is a mix of types,
laid out as TerrainGenerator._generate_curriculum_terrains / _generate_random_terrains do, and the field is rasterised
at ``cfg.raster_scale`` (generate_mix below).  Heightfield types are generated at horizontal_scale as upstream does and
up-sampled by evaluating their triangle mesh at the fine vertices, which leaves the surface what it was; the two mesh
types (stair pyramids, box grids) are sampled at the fine vertices, the higher side where the surface jumps, so a riser
is a ramp one fine cell wide lying on the lower tread.  No kernel knows about any of this: they sample a heightfield.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .cfg import TerrainGeneratorCfg


@dataclass
class Terrain:
    heights: np.ndarray   # (nx, ny) float32 metres, heights[ix, iy] at (x0 + ix*hs, y0 + iy*hs)
    hscale: float
    x0: float
    y0: float
    origins: np.ndarray   # (rows, cols, 3) float32 sub-terrain origins (world)
    # a mix of sub-terrain types (cfg.sub_terrains) also says what lies where; None on the single-type terrain
    sub_names: tuple | None = None       # the names of cfg.sub_terrains, in its order
    types: np.ndarray | None = None      # (rows, cols) int32 index into sub_names
    difficulty: np.ndarray | None = None  # (rows, cols) float64 difficulty each sub-terrain was generated at
    type_names: list | None = None       # curriculum mode: the type of every column (one type per column)

    @property
    def shape(self):
        return self.heights.shape


def generate(cfg: TerrainGeneratorCfg, seed: int) -> Terrain:
    if cfg.sub_terrains is not None:
        return generate_mix(cfg, seed)
    rng = np.random.default_rng(seed)
    hs, vs = cfg.horizontal_scale, cfg.vertical_scale
    sub_px = int(round(cfg.size[0] / hs))                 # 80 pixels per sub-terrain edge
    if int(round(cfg.size[1] / hs)) != sub_px:
        raise ValueError("square sub-terrains only")
    border_px = int(round(cfg.border_width / hs))         # 200
    inner_border = int(cfg.sub_border_width / hs) + 1     # 3 (height_field_to_mesh)
    nx = cfg.num_rows * sub_px + 1 + 2 * border_px
    ny = cfg.num_cols * sub_px + 1 + 2 * border_px
    hmin = int(cfg.noise_range[0] / vs)
    hmax = int(cfg.noise_range[1] / vs)
    hstep = max(1, int(cfg.noise_step / vs))
    levels = np.arange(hmin, hmax + hstep, hstep)
    H = np.zeros((nx, ny), dtype=np.int16)
    origins = np.zeros((cfg.num_rows, cfg.num_cols, 3), dtype=np.float32)
    x_grid0 = -0.5 * cfg.num_rows * cfg.size[0]
    y_grid0 = -0.5 * cfg.num_cols * cfg.size[1]
    c1 = int((cfg.size[0] * 0.5 - 1) / hs)
    c2 = int((cfg.size[0] * 0.5 + 1) / hs)
    for r in range(cfg.num_rows):
        for c in range(cfg.num_cols):
            sub = np.zeros((sub_px + 1, sub_px + 1), dtype=np.int16)
            n_in = sub_px + 1 - 2 * inner_border
            sub[inner_border:-inner_border, inner_border:-inner_border] = rng.choice(levels, size=(n_in, n_in))
            ix0 = border_px + r * sub_px
            iy0 = border_px + c * sub_px
            H[ix0:ix0 + sub_px + 1, iy0:iy0 + sub_px + 1] = np.maximum(H[ix0:ix0 + sub_px + 1, iy0:iy0 + sub_px + 1],
                                                                        sub)
            oz = float(sub[c1:c2, c1:c2].max()) * vs
            origins[r, c] = (x_grid0 + (r + 0.5) * cfg.size[0], y_grid0 + (c + 0.5) * cfg.size[1], oz)
    heights = (H.astype(np.float64) * vs).astype(np.float32)
    return Terrain(heights, hs, x_grid0 - border_px * hs, y_grid0 - border_px * hs, origins)


# ------------------------------------------------------------------ a mix of sub-terrain types (cfg.sub_terrains)
_EPS = 1e-9   # metres: a fine vertex this close to a wall of a mesh type counts as on it (and takes the higher side)


def column_types(proportions, num_cols: int) -> np.ndarray:
    """TerrainGenerator._generate_curriculum_terrains: column c takes the first type whose cumulative normalised
    proportion exceeds c / num_cols + 0.001."""
    p = np.asarray(proportions, np.float64)
    cum = np.cumsum(p / p.sum())
    return np.array([int(np.min(np.where(c / num_cols + 0.001 < cum)[0])) for c in range(num_cols)], np.int32)


def _ranged(rng_lo_hi, difficulty: float) -> float:
    lo, hi = rng_lo_hi
    return lo + difficulty * (hi - lo)


def upsample(coarse: np.ndarray, factor: int) -> np.ndarray:
    """The triangle mesh of ``coarse`` (float64 heights, unit cells) evaluated at the vertices of a grid ``factor``
    times finer: the fine mesh, split along the same diagonal, is the same surface."""
    if factor == 1:
        return np.array(coarse, np.float64)
    t = Terrain(np.asarray(coarse, np.float64), 1.0, 0.0, 0.0, np.zeros((1, 1, 3), np.float32))
    n0, n1 = coarse.shape
    u = np.arange((n0 - 1) * factor + 1) / factor
    v = np.arange((n1 - 1) * factor + 1) / factor
    return ground_height(t, u[:, None], v[None, :])


def _hf_frame(cfg: TerrainGeneratorCfg, border_width: float):
    """height_field_to_mesh: (pixels per edge, flat frame in pixels, pixels the type itself fills)."""
    n = int(cfg.size[0] / cfg.horizontal_scale) + 1
    b = int(border_width / cfg.horizontal_scale) + 1
    return n, b, n - 2 * b


def _hf_origin_z(cfg: TerrainGeneratorCfg, sub: np.ndarray) -> float:
    c1 = int((cfg.size[0] * 0.5 - 1) / cfg.horizontal_scale)
    c2 = int((cfg.size[0] * 0.5 + 1) / cfg.horizontal_scale)
    return float(sub[c1:c2, c1:c2].max()) * cfg.vertical_scale


def hf_random_uniform(sc, cfg: TerrainGeneratorCfg, rng) -> np.ndarray:
    """hf_terrains.random_uniform_terrain at downsampled_scale = horizontal_scale: int16 pixels (difficulty-free)."""
    n, b, n_in = _hf_frame(cfg, sc.border_width)
    vs = cfg.vertical_scale
    hmin, hmax, hstep = int(sc.noise_range[0] / vs), int(sc.noise_range[1] / vs), max(1, int(sc.noise_step / vs))
    sub = np.zeros((n, n), np.int16)
    sub[b:-b, b:-b] = rng.choice(np.arange(hmin, hmax + hstep, hstep), size=(n_in, n_in))
    return sub


def hf_pyramid_sloped(sc, cfg: TerrainGeneratorCfg, difficulty: float) -> np.ndarray:
    """hf_terrains.pyramid_sloped_terrain: height_max x (1 - |x|) (1 - |y|) over the type's own pixels, cut off at the
    height of the platform's corner, rounded to int16 pixels.  The faces rise by the cfg's slope: |x| is measured in
    half-widths of the type's own extent (37.5 pixels at the published sizes).  Upstream, restated from memory, divides
    by int(pixels / 2) = 37 instead, which would make every face 1.35 % steeper than the slope its cfg names (unpinned,
    DESIGN.md section 9)."""
    n, b, n_in = _hf_frame(cfg, sc.border_width)
    hs, vs = cfg.horizontal_scale, cfg.vertical_scale
    slope = _ranged(sc.slope_range, difficulty) * (-1.0 if sc.inverted else 1.0)
    height_max = int(slope * (n_in * hs) / 2 / vs)
    c = int(n_in / 2)
    x = np.arange(n_in)
    w = (c - np.abs(c - x)) / (0.5 * n_in)
    raw = height_max * w[:, None] * w[None, :]
    pf = n_in // 2 - int(sc.platform_width / hs / 2)
    z_pf = raw[pf, pf]
    raw = np.clip(raw, min(0.0, z_pf), max(0.0, z_pf))
    sub = np.zeros((n, n), np.int16)
    sub[b:-b, b:-b] = np.rint(raw).astype(np.int16)
    return sub


def stairs_ring_count(sc, size: float) -> int:
    """The rings of step_width that fit between the flat border and the platform: 5 at the published values, which
    leaves the platform its full platform_width.  (Counted with a tolerance, not with Python's `//`: 3.0 // 0.6 is 5.0
    but 1.0 // 0.1 is 9.0, so a bare floor counts by which side of the quotient the nearest double of the divisor
    falls on.
    Upstream's own count, restated from memory as `... // (2 step_width) + 1`, would be 6 rings around a 2.4 m
    platform if it is evaluated as written; which of the two the package builds is unpinned)"""
    return int(np.floor((size - 2 * sc.border_width - sc.platform_width) / (2 * sc.step_width) + 1e-9))


def mesh_pyramid_stairs(sc, cfg: TerrainGeneratorCfg, difficulty: float, rs: float):
    """(heights at the fine vertices, origin z).  Concentric square rings step_width wide inside a flat border: ring k
    (from outside) at (k + 1) steps, the platform inside the last ring one step above it."""
    size = cfg.size[0]
    step = _ranged(sc.step_height_range, difficulty)
    rings = stairs_ring_count(sc, size)
    n = int(round(size / rs)) + 1
    d = np.arange(n) * rs
    d = np.minimum(d, size - d)                      # distance to the nearer edge, per axis
    m = np.minimum(d[:, None], d[None, :])           # ... of the vertex: constant on square rings
    level = np.floor((m - sc.border_width + _EPS) / sc.step_width) + 1   # a vertex on a riser takes the upper tread
    level = np.clip(level, 0, rings + 1)
    sign = -1.0 if sc.inverted else 1.0
    return sign * level * step + 0.0, sign * (rings + 1) * step   # (+ 0.0: no -0.0 on the inverted border)


def mesh_random_grid(sc, cfg: TerrainGeneratorCfg, difficulty: float, rs: float, rng):
    """(heights at the fine vertices, origin z).  int(size / grid_width) squares per side, centred, each constant at
    U(-g, g); the leftover is a flat frame at 0 and the central platform is at +g."""
    size = cfg.size[0]
    g = _ranged(sc.grid_height_range, difficulty)
    k = int(size / sc.grid_width)
    frame = 0.5 * (size - k * sc.grid_width)
    box = rng.uniform(-g, g, size=(k, k))
    n = int(round(size / rs)) + 1
    x = np.arange(n) * rs

    def sample(lo_side: bool):
        # the square a vertex lies in; one on a wall belongs to the square on its low (high) side
        q = (x - frame) / sc.grid_width + (-_EPS if lo_side else _EPS)
        idx = np.floor(q).astype(np.int64)
        inside = (idx >= 0) & (idx < k)
        return np.clip(idx, 0, k - 1), inside

    h = None
    for ax in (True, False):
        for ay in (True, False):
            (ix, inx), (iy, iny) = sample(ax), sample(ay)
            v = np.where(inx[:, None] & iny[None, :], box[ix[:, None], iy[None, :]], 0.0)
            h = v if h is None else np.maximum(h, v)
    half = 0.5 * sc.platform_width
    on = (np.abs(x - 0.5 * size) <= half + _EPS)
    h = np.where(on[:, None] & on[None, :], g, h)
    return h, g


def make_sub_terrain(sc, cfg: TerrainGeneratorCfg, difficulty: float, rng):
    """One sub-terrain at cfg.raster_scale: (float64 heights at the fine vertices, 0 on the outer edge; origin z)."""
    from . import cfg as C

    hs = cfg.horizontal_scale
    rs = hs if cfg.raster_scale is None else cfg.raster_scale
    factor = int(round(hs / rs))
    if factor < 1 or abs(factor * rs - hs) > 1e-9:
        raise ValueError(f"raster_scale {rs} must divide horizontal_scale {hs}")
    if isinstance(sc, (C.HfRandomUniformTerrainCfg, C.HfPyramidSlopedTerrainCfg)):
        sub = (hf_random_uniform(sc, cfg, rng) if isinstance(sc, C.HfRandomUniformTerrainCfg)
               else hf_pyramid_sloped(sc, cfg, difficulty))
        # fine heights as multiples of vertical_scale / factor: a fine vertex on a coarse one is the same float
        units = np.rint(upsample(sub.astype(np.float64), factor) * factor)
        return units * (cfg.vertical_scale / factor), _hf_origin_z(cfg, sub)
    if isinstance(sc, C.MeshPyramidStairsTerrainCfg):
        return mesh_pyramid_stairs(sc, cfg, difficulty, rs)
    if isinstance(sc, C.MeshRandomGridTerrainCfg):
        return mesh_random_grid(sc, cfg, difficulty, rs, rng)
    raise TypeError(f"unknown sub-terrain cfg {type(sc).__name__}")


def generate_mix(cfg: TerrainGeneratorCfg, seed: int) -> Terrain:
    """The grid of cfg.sub_terrains as one heightfield at cfg.raster_scale (module doc)."""
    rng = np.random.default_rng(seed)
    if abs(cfg.size[0] - cfg.size[1]) > 1e-9:
        raise ValueError("square sub-terrains only")
    names = tuple(cfg.sub_terrains)
    subs = [cfg.sub_terrains[k] for k in names]
    props = np.array([s.proportion for s in subs], np.float64)
    rows, cols = cfg.num_rows, cfg.num_cols
    rs = cfg.horizontal_scale if cfg.raster_scale is None else cfg.raster_scale
    sub_px = int(round(cfg.size[0] / rs))
    border_px = int(round(cfg.border_width / rs))
    lo, hi = cfg.difficulty_range
    types = np.zeros((rows, cols), np.int32)
    difficulty = np.zeros((rows, cols), np.float64)
    if cfg.curriculum:
        col_type = column_types(props, cols)
        cells = [(r, c) for c in range(cols) for r in range(rows)]   # upstream's loop order
    else:
        col_type = None
        cells = [(i // cols, i % cols) for i in range(rows * cols)]
    H = np.zeros((rows * sub_px + 1 + 2 * border_px, cols * sub_px + 1 + 2 * border_px), np.float64)
    origins = np.zeros((rows, cols, 3), np.float32)
    x_grid0, y_grid0 = -0.5 * rows * cfg.size[0], -0.5 * cols * cfg.size[1]
    for r, c in cells:
        if cfg.curriculum:
            k = int(col_type[c])
            d = lo + (hi - lo) * (r + rng.uniform()) / rows
        else:
            k = int(rng.choice(len(subs), p=props / props.sum()))
            d = rng.uniform(lo, hi)
        types[r, c], difficulty[r, c] = k, d
        h, oz = make_sub_terrain(subs[k], cfg, d, rng)
        if h.shape != (sub_px + 1, sub_px + 1):
            raise ValueError(f"sub-terrain {names[k]}: {h.shape} vertices, expected {sub_px + 1} per edge")
        if h[0].any() or h[-1].any() or h[:, 0].any() or h[:, -1].any():
            raise ValueError(f"sub-terrain {names[k]} is not 0 on its outer edge (neighbours share it)")
        ix0, iy0 = border_px + r * sub_px, border_px + c * sub_px
        H[ix0:ix0 + sub_px + 1, iy0:iy0 + sub_px + 1] = h
        origins[r, c] = (x_grid0 + (r + 0.5) * cfg.size[0], y_grid0 + (c + 0.5) * cfg.size[1], oz)
    return Terrain(H.astype(np.float32), rs, x_grid0 - border_px * rs, y_grid0 - border_px * rs, origins,
                   sub_names=names, types=types, difficulty=difficulty,
                   type_names=[names[k] for k in col_type] if col_type is not None else None)


def level_log_weights(t: Terrain, env_cols: np.ndarray) -> dict:
    """"Curriculum/terrain_levels/<type>" -> (n,) float32 weights whose dot product with the envs' levels is the mean
    level of the envs in that type's columns.  Empty unless the terrain has one type per column and more than one type;
    a type none of the envs stands on gets no key."""
    names = t.type_names
    if names is None or len(set(names)) < 2:
        return {}
    out = {}
    col_names = np.asarray(names)[np.asarray(env_cols, np.int64)]
    for name in dict.fromkeys(names):
        m = col_names == name
        if m.any():
            out[f"Curriculum/terrain_levels/{name}"] = (m / m.sum()).astype(np.float32)
    return out


def initial_cells(num_envs: int, cfg: TerrainGeneratorCfg, max_init_level: int | None, seed: int):
    """TerrainImporter._compute_env_origins_curriculum: (levels, types) per env."""
    rng = np.random.default_rng(seed + 7919)
    max_lvl = cfg.num_rows - 1 if max_init_level is None else min(max_init_level, cfg.num_rows - 1)
    levels = rng.integers(0, max_lvl + 1, size=num_envs)
    types = np.floor(np.arange(num_envs) / (num_envs / cfg.num_cols)).astype(np.int64)
    return levels.astype(np.int32), np.minimum(types, cfg.num_cols - 1).astype(np.int32)


def ground_height(t: Terrain, x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """Vectorised twin of the kernels' ground() (host-side checks and tools)."""
    u = np.clip((np.asarray(x) - t.x0) / t.hscale, 0, t.shape[0] - 1 - 1e-3)
    v = np.clip((np.asarray(y) - t.y0) / t.hscale, 0, t.shape[1] - 1 - 1e-3)
    ix, iy = u.astype(np.int64), v.astype(np.int64)
    fu, fv = u - ix, v - iy
    h = t.heights.astype(np.float64)
    h00, h01, h10, h11 = h[ix, iy], h[ix, iy + 1], h[ix + 1, iy], h[ix + 1, iy + 1]
    upper = fv >= fu
    a = np.where(upper, h11 - h01, h10 - h00)
    b = np.where(upper, h01 - h00, h11 - h10)
    return h00 + fu * a + fv * b
