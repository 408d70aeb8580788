"""CPU: the heightfield query and the height scan against the mesh definition, on planted relief and poses.

orc_ground (oracle), h12env.terrain.ground_height (host twin) and the kernel's ground() are three transcriptions of the
same few lines; tests/helpers/terrain_ref.py:mesh_height is written from the mesh definition instead (the plane
through the three vertices of the containing triangle).  Here

* the oracle and the host twin are pinned to it on every planted terrain, gradients included;
* a numpy float32 restatement of ground(), ground_local(), the scan and the contact normal is shown to stay inside the
  a-priori bound on every case tests/test_gpu_terrain.py runs on the MI355X, and every planted mistake (MUTANTS) to
  leave it by at least 10 x on a named case -- the bound is tight enough to see each of them;
* ground_local() + org.z equals ground() inside the bound except in the last 1e-3 of the last cell;
* the contact runs of the GPU test are shown well-conditioned by the oracle alone.
"""
import numpy as np
import pytest

import oracle as O
import terrain_ref as TR
from forced import TOL_PHYS, n_threads, perturbed, phys_err
from h12env import terrain as T
from h12env._abi import F as FIELDS
from h12env.startup import apply_to_arrays, startup_state


# ------------------------------------------------------------------ the planted inputs are what the tests rely on
def test_planted_terrains():
    r = TR.planted("relief").terrain.heights.astype(np.float64)
    assert r.shape == (37, 29)
    gx, gy = TR.slopes(r, 0.1)
    assert 1.8 < gx <= 2.0 and 1.5 < gy <= 2.0
    assert r.max() - r.min() > 2.5
    for edge in (r[0], r[-1], r[:, 0], r[:, -1]):       # relief out to the last vertex on all four sides
        assert np.abs(np.diff(edge)).min() > 0
    assert np.abs(r[:29, :29] - r[:29, :29].T).max() > 1.0                       # asymmetric in (ix, iy)
    assert np.abs(r[:-1, :-1] + r[1:, 1:] - r[1:, :-1] - r[:-1, 1:]).min() >= 0  # (most cells are non-planar:)
    assert (np.abs(r[:-1, :-1] + r[1:, 1:] - r[1:, :-1] - r[:-1, 1:]) > 0.01).mean() > 0.5
    for name in ("far", "coarse"):
        assert (TR.planted(name).terrain.heights == r).all()
    assert TR.planted("coarse").terrain.hscale == 0.25 and TR.planted("far").terrain.x0 == -100.0
    hs = TR.planted("ramp_x").terrain.hscale
    ix, iy = np.meshgrid(np.arange(37), np.arange(29), indexing="ij")
    assert (TR.planted("ramp_x").terrain.heights == 0.25 * ix * hs).all()
    assert (TR.planted("ramp_y").terrain.heights == 0.25 * iy * hs).all()
    c = TR.planted("cell").terrain.heights
    assert c.shape == (2, 2) and len(set(c.ravel().tolist())) == 4
    m = TR.planted("mild").terrain.heights
    assert max(TR.slopes(m, 0.1)) <= 0.5 and (m[-1] == m[-2]).all() and (m[:, -1] == m[:, -2]).all()
    for name in TR.ALL_TERRAINS:
        p = TR.planted(name)
        h = p.terrain.heights.astype(np.float64) * 1024
        assert (h == np.round(h)).all()                  # multiples of 2^-10 m: exact in float32
        assert (p.buf[:TR.PAD] == 1000.0).all() and (p.buf[-TR.PAD:] == 1000.0).all()
        assert np.shares_memory(p.buf, p.terrain.heights)
    # the clip class: all above, all below, and on relief both ends within the middle row
    for name in TR.SCAN_TERRAINS:
        c = TR.scan_case(name)
        hi, lo, mix = c.classes["clip"]
        assert (c.ref.raw[hi] > 1 + c.bound[hi]).all() and (c.ref.raw[lo] < -1 - c.bound[lo]).all()
    c = TR.scan_case("relief")
    row = c.ref.raw[mix].reshape(11, 17)[5]
    assert row.max() > 1.01 and row.min() < -1.01 and (np.abs(row) < 0.9).any()
    # every class holds clamped rays where it should
    t = c.p.terrain
    out = (c.ref.wx < t.x0) | (c.ref.wx > t.x0 + c.p.extent[0]) | (c.ref.wy < t.y0) | (c.ref.wy > t.y0 + c.p.extent[1])
    assert out[c.classes["outside"][-8:]].all() and out[c.classes["straddle"]].any(axis=1).all()
    assert not out[c.classes["straddle"]].all(axis=1).any() and not out[c.classes["lattice"]].any()


# ------------------------------------------------------------------ oracle and host twin against the mesh
def query_points(p):
    """(x, y, kind): interior points of both triangles, points on vertices, edges and the diagonal, and points
    outside each side and each corner."""
    t = p.terrain
    nx, ny = t.shape
    hs = t.hscale
    rng = np.random.default_rng(3)
    k = 40
    ix, iy = rng.integers(0, nx - 1, k), rng.integers(0, ny - 1, k)
    pts = []
    for fu, fv in [(0.7, 0.2), (0.2, 0.7), (0.31, 0.93), (0.93, 0.31),       # interior, below / above the diagonal
                   (0.0, 0.0), (0.0, 0.4), (0.6, 0.0), (0.45, 0.45)]:         # vertex, edges, diagonal
        pts.append((t.x0 + (ix + fu) * hs, t.y0 + (iy + fv) * hs))
    ex, ey = p.extent
    for d in (0.003, 0.05, 1.0, 30.0):
        for sx, sy in [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)]:
            bx = t.x0 + rng.uniform(0.1, 0.9, 5) * ex
            by = t.y0 + rng.uniform(0.1, 0.9, 5) * ey
            pts.append(({-1: t.x0 - d + 0 * bx, 0: bx, 1: t.x0 + ex + d + 0 * bx}[sx],
                        {-1: t.y0 - d + 0 * by, 0: by, 1: t.y0 + ey + d + 0 * by}[sy]))
    # the last vertex itself and the last 1e-3 of the last cell (clamped to n - 1 - 1e-3)
    pts.append((np.array([t.x0 + ex, t.x0 + ex - 5e-4 * hs, t.x0 + 0.3 * ex]),
                np.array([t.y0 + ey, t.y0 + 0.3 * ey, t.y0 + ey - 5e-4 * hs])))
    x = np.concatenate([a for a, _ in pts])
    y = np.concatenate([b for _, b in pts])
    return x, y


def off_borders(p, x, y, eps=1e-6):
    """Points whose clamped cell coordinates keep eps from every triangle border."""
    t = p.terrain
    u = np.clip((x - t.x0) / t.hscale, 0, t.shape[0] - 1 - 1e-3)
    v = np.clip((y - t.y0) / t.hscale, 0, t.shape[1] - 1 - 1e-3)
    fu, fv = u - np.floor(u), v - np.floor(v)
    return np.minimum.reduce([fu, fv, 1 - fu, 1 - fv, np.abs(fu - fv)]) > eps


@pytest.mark.parametrize("name", TR.ALL_TERRAINS)
def test_oracle_and_host_twin_match_mesh(name):
    p = TR.planted(name)
    t = p.terrain
    x, y = query_points(p)
    h, gx, gy = TR.mesh_height(*p.args, x, y)
    assert np.abs(h).max() < 10  # (nothing read the 1000.0 around the array)
    O.set_terrain(t.heights, t.hscale, t.x0, t.y0, t.origins)
    c = TR.contact_cfg(1).to_c()
    assert c.terrain == 1
    got = np.array([O.ground(c, a, b) for a, b in zip(x, y)])
    tol = 1e-12 * np.maximum(1, np.abs(h))
    assert (np.abs(got[:, 0] - h) <= tol).all(), np.abs(got[:, 0] - h).max()
    assert (np.abs(T.ground_height(t, x, y) - h) <= tol).all()
    ok = off_borders(p, x, y)
    outside = (x < t.x0) | (y < t.y0) | (x > t.x0 + p.extent[0]) | (y > t.y0 + p.extent[1])
    assert ok.sum() > 100 and (ok & outside).sum() > 20
    assert (np.abs(got[ok, 1] - gx[ok]) <= 1e-12 * np.maximum(1, np.abs(gx[ok]))).all()
    assert (np.abs(got[ok, 2] - gy[ok]) <= 1e-12 * np.maximum(1, np.abs(gy[ok]))).all()
    # the gradient against a finite difference of the reference's own height, both axes
    e = 1e-7
    fx = (TR.mesh_height(*p.args, x + e, y)[0] - TR.mesh_height(*p.args, x - e, y)[0]) / (2 * e)
    fy = (TR.mesh_height(*p.args, x, y + e)[0] - TR.mesh_height(*p.args, x, y - e)[0]) / (2 * e)
    inner = off_borders(p, x, y, 1e-4) & ~outside  # (the difference quotient must not straddle a border)
    # (nor lie in the clamped last 1e-3 of the last cell, where the height is constant and the slope is not)
    inner &= (x < t.x0 + p.extent[0] - 2e-3 * t.hscale) & (y < t.y0 + p.extent[1] - 2e-3 * t.hscale)
    assert inner.sum() > 100
    np.testing.assert_allclose(gx[inner], fx[inner], atol=1e-6)
    np.testing.assert_allclose(gy[inner], fy[inner], atol=1e-6)
    if name == "ramp_x":
        assert (gx[inner] == 0.25).all() and (gy[inner] == 0).all()
    if name == "ramp_y":
        assert (gy[inner] == 0.25).all() and (gx[inner] == 0).all()


def test_outside_the_grid_height_is_constant_but_slope_is_the_edge_cells():
    """The clamp semantics DESIGN.md records: past a border the height no longer changes along the clamped direction,
    while the returned slope stays the edge triangle's."""
    p = TR.planted("relief")
    t = p.terrain
    y = t.y0 + 1.234
    h = [TR.mesh_height(*p.args, t.x0 - d, y) for d in (0.0, 0.5, 30.0)]
    assert h[0][0] == h[1][0] == h[2][0]
    assert h[0][1] == h[2][1] != 0.0


# ------------------------------------------------------------------ fp32 restatement and its mutants
def scan_ratio(name, mut=None):
    c = TR.scan_case(name)
    return float((np.abs(TR.scan32(c.p, c.pos, c.quat, mut) - c.ref.clipped) / c.bound).max())


def local_ratio(name, mut=None, strip=False):
    p, org, xl, yl = TR.local_case(name)
    o, a, b = org.astype(np.float64), xl.astype(np.float64), yl.astype(np.float64)
    h = TR.mesh_height(*p.args, o[:, 0] + a, o[:, 1] + b)[0]
    bound = TR.local_bound(*p.args, o, a, b, h)
    got = TR.ground_local32(p, org, xl, yl, mut)[0].astype(np.float64) + o[:, 2]
    gx, gy = TR.slopes(*p.args[:2])
    e_pos = bound / max(gx + gy, 1e-9)
    s = TR.strip_mask(p, o[:, 0] + a, o[:, 1] + b, e_pos)
    err = np.abs(got - h)
    if strip:
        return err[s], bound[s], s
    return float((err[~s] / bound[~s]).max())


def normal_ratio(name, mut=None):
    p = TR.with_origins(TR.planted(name))
    rng = np.random.default_rng(5)
    m = 200
    org = p.terrain.origins.reshape(-1, 3)[rng.integers(0, 4, m)]
    xw = np.stack([rng.uniform(-0.6, 0.6, m), rng.uniform(-0.6, 0.6, m), rng.uniform(-0.05, 0.1, m)], axis=1)
    worst = 0.0
    for sg in (1.0, -1.0):
        n32, d32 = TR.normal32(p, org, xw.astype(np.float32), sg, 0.02, mut)
        n64, d64 = TR.normal_ref(p, org, xw.astype(np.float32), sg, 0.02)
        worst = max(worst, float(np.abs(n32 - n64).max() / TR.NORMAL_BOUND))
        # the depth rad - (z - h) / |(-h_x, -h_y, 1)|: the height's bound, and 10 u of the products around it
        o = org.astype(np.float64)
        x, y = xw[:, 0].astype(np.float32).astype(np.float64), sg * xw[:, 1].astype(np.float32).astype(np.float64)
        h = TR.mesh_height(*p.args, o[:, 0] + x, o[:, 1] + y)[0]
        db = TR.local_bound(*p.args, o, x, y, h) + 10 * TR.U * (np.abs(o[:, 2] + xw[:, 2] - h) + 0.02)
        worst = max(worst, float((np.abs(d32 - d64) / db).max()))
    return worst


SCAN_MUTANTS = ("other_diagonal", "transposed_index", "no_upper_clamp", "no_lower_clamp", "rays_y_fastest",
                "yaw_unnormalised", "clip_before_offset")
LOCAL_MUTANTS = ("other_diagonal", "transposed_index", "no_upper_clamp", "no_lower_clamp", "trunc_local")
NORMAL_MUTANTS = ("gy_not_mirrored",)
CASES = ([(f"scan:{n}", scan_ratio, n, SCAN_MUTANTS) for n in TR.SCAN_TERRAINS] +
         [(f"local:{n}", local_ratio, n, LOCAL_MUTANTS) for n in TR.ALL_TERRAINS] +
         [(f"normal:{n}", normal_ratio, n, NORMAL_MUTANTS) for n in TR.CONTACT_TERRAINS])
# the case on which each planted mistake must leave the bound by at least 10 x
NAMED = dict(other_diagonal="scan:relief", transposed_index="scan:relief", no_upper_clamp="scan:relief",
             no_lower_clamp="scan:relief", trunc_local="local:relief", gy_not_mirrored="normal:ramp_y",
             rays_y_fastest="scan:ramp_x", yaw_unnormalised="scan:relief", clip_before_offset="scan:ramp_y")


def test_restatement_inside_bound_and_every_mutant_far_outside():
    table = {}
    for label, fn, name, muts in CASES:
        table[label] = {None: fn(name)}
        for m in muts:
            table[label][m] = fn(name, m)
    w = max(len(c) for c in table)
    print("\nworst error / bound, fp32 restatement (mutant x case)")
    print(" " * 20 + " ".join(f"{c:>{w}}" for c in table))
    for m in (None,) + TR.MUTANTS:
        cells = [f"{table[c][m]:>{w}.3g}" if m in table[c] else f"{'-':>{w}}" for c in table]
        print(f"{str(m or 'restatement'):<20}" + " ".join(cells))
    for label in table:
        assert table[label][None] <= 1.0, (label, table[label][None])
    assert set(NAMED) == set(TR.MUTANTS)
    for m, label in NAMED.items():
        assert table[label][m] >= 10.0, (m, label, table[label][m])


# ------------------------------------------------------------------ ground_local against ground
@pytest.mark.parametrize("name", TR.ALL_TERRAINS)
def test_ground_local_equals_ground_except_in_the_last_strip(name):
    """ground_local(org, xl, yl) + org.z is the mesh height at org + (xl, yl) inside the bound -- origins at `far`'s
    magnitude included -- except where the cell coordinate lies in the last 1e-3 of the last cell: there ground()
    clamps the fraction to 1 - 1e-3 and ground_local keeps it, a difference of at most 1e-3 hs G."""
    assert local_ratio(name) <= 1.0
    p, org, xl, yl = TR.local_case(name)
    x, y = org[:, 0] + xl, org[:, 1] + yl          # float32, as the kernel's world-coordinate path forms them
    h = TR.mesh_height(*p.args, x.astype(np.float64), y.astype(np.float64))[0]
    g = TR.ground32(p, x, y)[0]
    # ground() in world coordinates obeys the scan's bound with a zero lever arm
    gx, gy = TR.slopes(*p.args[:2])
    t = p.terrain
    b = (gx * TR.U * 3 * (np.abs(x) + abs(t.x0)) + gy * TR.U * 3 * (np.abs(y) + abs(t.y0)) +
         4 * TR.U * (np.abs(h) + (gx + gy) * t.hscale))
    assert (np.abs(g - h) <= b).all()
    err, bound, s = local_ratio(name, strip=True)
    assert s.sum() >= 12
    assert (err <= bound + 1e-3 * t.hscale * (gx + gy)).all()
    if name in ("relief", "coarse"):  # (on `far` the bound itself is as large as the strip's 1e-3 hs G)
        assert (err > 2 * bound).any()             # the strip is real on relief that reaches the last vertex ...
    if name == "mild":
        assert (err <= bound).all()                # ... and empty where the last cell is flat along the clamped axis


# ------------------------------------------------------------------ the GPU contact runs, oracle alone
@pytest.mark.parametrize("name", TR.CONTACT_TERRAINS)
def test_contact_runs_are_well_conditioned(model, name):
    """The condition of test_gpu_terrain's contact gate: over the same 12 steps, an oracle run from a state perturbed
    by 1e-7 leaves TOL_PHYS of the unperturbed oracle on fewer than half the 1.5 % of env-steps the gate allows."""
    n = TR.N_CONTACT
    cfg = TR.contact_cfg(n)
    p = TR.with_origins(TR.planted(name))
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
    for k, a in enumerate(TR.contact_actions(name)):
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
    assert share < 0.5 * 0.015
    assert both.mean() >= 0.5
