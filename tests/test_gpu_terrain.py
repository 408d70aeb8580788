"""GPU: ground(), the 187-ray height scan of rough_obs_kernel and the heightfield contact (ground_local, the mirrored
normal of the right-leg lane) on planted relief and planted poses, against the float64 mesh reference and the a-priori
fp32 bound of tests/helpers/terrain_ref.py.

The generated terrain has 2 cm of relief and a flat border no robot leaves; here the relief is metres high with
neighbour slopes up to 2, runs out to the last vertex, sits at world coordinates of 100 m, and the poses reach every
clamp, both clips and tilts of 0.5 rad.  Every planted terrain is bound as a slice from the middle of a larger device
tensor of 1000.0, so a read one row before or after the array cannot hide inside any bound.

Each test prints what it measured (worst |scan - reference| / bound per terrain and pose class, ForcedParity's
report); the MI355X's figures are in the tests' docstrings and in DESIGN.md section 7b.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
import terrain_ref as TR
from forced import ForcedParity
from h12env._abi import F as FIELDS
from h12env._abi import I as IFIELDS
from h12env._abi import NOBS_ROUGH
from h12env.env import H12VelocityEnv

pytestmark = pytest.mark.gpu

SCAN0 = NOBS_ROUGH - TR.NRAY  # 48


def make_env(n):
    cfg = TR.contact_cfg(n)
    cfg.sim.device = "cuda:0"
    return H12VelocityEnv(cfg)


def bind(env, p):
    """Swap the env's terrain for a planted one the way _apply_startup binds the generated one."""
    nx, ny = p.terrain.shape
    big = torch.from_numpy(p.buf).to(env.device)
    env.terrain = p.terrain
    env._t_heights = big[p.off:p.off + nx * ny].view(nx, ny)
    env._t_origins = torch.from_numpy(p.terrain.origins).to(env.device)
    assert env._t_heights.data_ptr() == big.data_ptr() + 4 * p.off and env._t_origins.shape[:2] == (2, 2)
    env._bind_terrain()


def scan(env, pos, quat):
    o, q = FIELDS["POS"][0], FIELDS["QUAT"][0]
    env._fstate[o:o + 3].copy_(torch.from_numpy(np.ascontiguousarray(pos.T)))
    env._fstate[q:q + 4].copy_(torch.from_numpy(np.ascontiguousarray(quat.T)))
    return env.observe()["policy"][:, SCAN0:].cpu().numpy().copy()


@pytest.fixture(scope="module")
def envs(gpu):
    e67, e1 = make_env(TR.N_SCAN), make_env(1)
    yield e67, e1
    e67.close()
    e1.close()


@pytest.mark.parametrize("name", TR.SCAN_TERRAINS)
def test_scan_on_planted_terrain(envs, name):
    """Every scan value of 67 planted poses (interior and tilted, on vertices / edges / the diagonal, outside every
    side and corner by 0.05 - 3 m, straddling every edge, clipped at either and at both ends) is within scan_bound of
    scan_ref; clipped values are exactly +-1; q and -q, env 3 and env 60, n = 67 and n = 1, and two calls agree bit
    for bit.

    Worst |error| / bound measured on the MI355X: relief 0.126, far 0.157, coarse 0.180, ramp_x 0.101, ramp_y 0.086,
    cell 0.056 (the numpy fp32 restatement: 0.131, 0.157, 0.180, 0.105, 0.091, 0.064).  No kernel change was
    needed."""
    e67, e1 = envs
    c = TR.scan_case(name)
    bind(e67, c.p)
    got = scan(e67, c.pos, c.quat)
    assert got.shape == (TR.N_SCAN, TR.NRAY) and np.isfinite(got).all()
    frac = np.abs(got - c.ref.clipped) / c.bound
    per_class = {k: float(f"{frac[i].max():.3g}") for k, i in c.classes.items()}
    print(f"\nscan on {name}: worst |error| / bound {frac.max():.3f} (per pose class {per_class}); "
          f"bound {c.bound.min():.2e} .. {c.bound.max():.2e} m")
    assert (frac <= 1.0).all(), (name, np.argwhere(frac > 1.0)[:8], frac.max())
    hi, lo = c.ref.raw > 1 + c.bound, c.ref.raw < -1 - c.bound
    assert hi.any() and lo.any()
    assert (got[hi] == 1.0).all() and (got[lo] == -1.0).all()
    assert np.abs(got).max() <= 1.0
    assert (got[TR.ENV_NEGQ] == got[TR.ENV_Q]).all()
    assert (got[TR.ENV_A] == got[TR.ENV_B]).all()
    assert (scan(e67, c.pos, c.quat) == got).all()
    bind(e1, c.p)
    one = np.concatenate([scan(e1, c.pos[i:i + 1], c.quat[i:i + 1]) for i in range(TR.N_SCAN)])
    assert (one == got).all()


def test_set_terrain_refusals_leave_the_bound_terrain(envs):
    """h12env_set_terrain refuses nx = 1, ny = 1, hscale = 0, null heights and origins without rows (or rows without
    origins); each refusal returns an error, says why, and leaves the bound terrain as it was."""
    env, _ = envs
    c = TR.scan_case("relief")
    bind(env, c.p)
    before = scan(env, c.pos, c.quat)
    t = c.p.terrain
    nx, ny = t.shape
    hp, op = C.c_void_p(env._t_heights.data_ptr()), C.c_void_p(env._t_origins.data_ptr())
    lib = env._lib
    for args, why in [((hp, 1, ny, t.hscale, t.x0, t.y0, op, 2, 2), "nx, ny >= 2"),
                      ((hp, nx, 1, t.hscale, t.x0, t.y0, op, 2, 2), "nx, ny >= 2"),
                      ((hp, nx, ny, 0.0, t.x0, t.y0, op, 2, 2), "hscale > 0"),
                      ((None, nx, ny, t.hscale, t.x0, t.y0, op, 2, 2), "heights"),
                      ((hp, nx, ny, t.hscale, t.x0, t.y0, op, 0, 2), "rows in 1..65535"),
                      ((hp, nx, ny, t.hscale, t.x0, t.y0, op, 2, 0), "cols in 1..32767"),
                      ((hp, nx, ny, t.hscale, t.x0, t.y0, None, 2, 2), "origins need rows"),
                      ((hp, nx, ny, t.hscale, t.x0, t.y0, op, 65536, 2), "rows in 1..65535"),
                      ((hp, nx, ny, t.hscale, t.x0, t.y0, op, 2, 32768), "cols in 1..32767")]:
        rc = lib.h12env_set_terrain(env._h, *args)
        assert rc != 0, args
        assert why in lib.h12env_last_error().decode(), (args, lib.h12env_last_error())
        assert (scan(env, c.pos, c.quat) == before).all(), args
    assert lib.h12env_set_terrain(env._h, hp, nx, ny, t.hscale, t.x0, t.y0, op, 2, 2) == 0


@pytest.mark.parametrize("name", TR.CONTACT_TERRAINS)
def test_contact_on_planted_relief(gpu, name):
    """Reset and 12 teacher-forced MDP steps on a ramp along y (the mirrored normal of the right-leg lane is a
    first-order term in every step), a ramp along x and relief with slopes up to 0.5, origins spread over the grid and
    two cells from its borders: every env within tolerance of the oracle or shown threshold-sensitive by it, at most
    1.5 % of env-steps off (test_c5_full_size_forced's cap; its condition is checked on the CPU by
    test_terrain_emulation.test_contact_runs_are_well_conditioned), and both feet of at least half the envs touch.

    Measured on the MI355X (ForcedParity's report): env-steps off tolerance 2 / 4 / 2 of 1536 (ramp_y / ramp_x / mild),
    every one threshold-sensitive at a 1e-7 or 1e-6 perturbation, none unexplained; phys p50 2.4e-5 / 2.7e-5 / 2.2e-5,
    p99 2.6e-4 / 2.3e-4 / 2.2e-4; both feet in contact in 0.92 / 0.89 / 0.84 of the envs."""
    n = TR.N_CONTACT
    env = make_env(n)
    p = TR.with_origins(TR.planted(name))
    bind(env, p)
    t = p.terrain
    O.set_terrain(t.heights, t.hscale, t.x0, t.y0, t.origins)
    F = env._fstate.cpu().numpy()
    TR.plant_origins(p, F, env._istate.cpu().numpy()[IFIELDS["TERRAIN"][0]])
    env._fstate.copy_(torch.from_numpy(F))
    ref = O.OracleEnv(env._model, env._ccfg, n)
    ref.F[:], ref.I[:] = F, env._istate.cpu().numpy()
    obs, _ = env.reset()
    np.testing.assert_allclose(obs["policy"].cpu().numpy(), ref.reset(), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(env._fstate.cpu().numpy(), ref.F, rtol=1e-6, atol=1e-6)
    assert (env._istate.cpu().numpy() == ref.I).all()
    org = env._fstate.cpu().numpy()[FIELDS["ORIGIN"][0]:FIELDS["ORIGIN"][0] + 3].T
    assert {tuple(o) for o in org} == {tuple(o) for o in t.origins.reshape(-1, 3)}  # all four origins in use
    fp = ForcedParity(env, seed=33)
    both = np.zeros(n, bool)
    for a in TR.contact_actions(name):
        (_, gi, _, rew, _, _), _, _, _ = fp.step(a)
        assert np.isfinite(rew).all()
        bits = (gi[IFIELDS["PACK"][0]] >> 13) & 0xFF
        both |= ((bits & 0x0F) != 0) & ((bits & 0xF0) != 0)
    print(f"\ncontact on {name}: both feet in contact in {both.mean():.2f} of the envs; {fp.report()}")
    fp.check(max_bad_frac=0.015)
    assert both.mean() >= 0.5
    env.close()
