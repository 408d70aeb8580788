"""GPU: the kernels on the relief of the reference's Rough task -- stair pyramids with 0.23 m risers, box grids of
+-0.2 m, 10 cm noise and slopes of 0.4, rasterised at 0.05 m (tests/helpers/terrain_mix_ref.py: 2 rows x 6 types,
361 x 1001 cells, the easy row at difficulty ~0 and the hard row at ~1).  No kernel was written or changed for this
relief; until now the height scan was tested on slopes up to 2 at 0.1 m cells and the contacts on slopes up to 0.5.

* the 187-ray scan of 67 planted poses, rays crossing risers and box walls, inside terrain_ref.scan_bound of the float64
  mesh reference (the bound scales with the field's largest neighbour slope: 7.7 here, where +-0.2 m boxes meet);
* reset on every type and row against the oracle at test_gpu_rough's tolerances;
* 12 teacher-forced steps of 128 envs whose origins are planted on platforms, treads, astride a riser, on box walls and
  on slope faces of the hard row: test_gpu_terrain's gate, fp.check(max_bad_frac=0.015), whose condition
  tests/test_terrain_mix.py checks with the oracle alone;
* the in-kernel curriculum across columns of different types, and the per-type level means of the log;
* train.py --terrain isaaclab_rough, play.py on that run, and a rendered frame over stairs.

Each test prints what it measured; the MI355X's figures are in the docstrings and in DESIGN.md section 7b.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import oracle as O
import terrain_mix_ref as M
import terrain_ref as TR
from forced import ForcedParity
from h12env import cfg as K
from h12env._abi import F as FIELDS
from h12env._abi import I as IFIELDS
from h12env._abi import NOBS_ROUGH
from h12env.env import H12VelocityEnv

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "h1v2-isaac_amd"
SCAN0 = NOBS_ROUGH - TR.NRAY


def make_env(n, rows=2, cols=2):
    cfg = TR.contact_cfg(n)
    g = cfg.scene.terrain.terrain_generator
    g.num_rows, g.num_cols = rows, cols
    cfg.sim.device = "cuda:0"
    return H12VelocityEnv(cfg)


def bind(env, p):
    """Swap the env's terrain for a planted one the way _apply_startup binds the generated one (as test_gpu_terrain)."""
    nx, ny = p.terrain.shape
    big = torch.from_numpy(p.buf).to(env.device)
    env.terrain = p.terrain
    env._t_heights = big[p.off:p.off + nx * ny].view(nx, ny)
    env._t_origins = torch.from_numpy(p.terrain.origins).to(env.device)
    assert env._t_heights.data_ptr() == big.data_ptr() + 4 * p.off
    env._bind_terrain()


def planted_start(env, p):
    """ORIGIN / POS of every env from the planted origin table, on the env and on a fresh oracle."""
    t = p.terrain
    O.set_terrain(t.heights, t.hscale, t.x0, t.y0, t.origins)
    F = env._fstate.cpu().numpy()
    TR.plant_origins(p, F, env._istate.cpu().numpy()[IFIELDS["TERRAIN"][0]])
    env._fstate.copy_(torch.from_numpy(F))
    ref = O.OracleEnv(env._model, env._ccfg, env.num_envs)
    ref.F[:], ref.I[:] = F, env._istate.cpu().numpy()
    return ref


def test_scan_across_risers_and_box_walls(gpu):
    """Every scan value of the 67 planted poses on the hard row of the mix is within scan_bound of scan_ref; clipped
    values are exactly +-1; q and -q, env 3 and env 60 and two calls agree bit for bit.

    Measured on the MI355X: worst |error| / bound 0.138 (the numpy fp32 restatement: 0.138; per pose class: interior
    0.090, straddle 0.088, lattice 0.020); the bound is 5.3e-5 .. 1.2e-4 m at largest neighbour slopes of 7.3 and 7.7."""
    env = make_env(TR.N_SCAN)
    p = M.whole_mix()
    bind(env, p)
    pos, quat, cls, ref, bound = M.scan_case()
    o, q = FIELDS["POS"][0], FIELDS["QUAT"][0]

    def scan():
        env._fstate[o:o + 3].copy_(torch.from_numpy(np.ascontiguousarray(pos.T)))
        env._fstate[q:q + 4].copy_(torch.from_numpy(np.ascontiguousarray(quat.T)))
        return env.observe()["policy"][:, SCAN0:].cpu().numpy().copy()

    got = scan()
    assert got.shape == (TR.N_SCAN, TR.NRAY) and np.isfinite(got).all()
    frac = np.abs(got - ref.clipped) / bound
    per_class = {k: float(f"{frac[i].max():.3g}") for k, i in cls.items()}
    print(f"\nscan on the mix: worst |error| / bound {frac.max():.3f} (per pose class {per_class}); "
          f"bound {bound.min():.2e} .. {bound.max():.2e} m; slopes {TR.slopes(p.terrain.heights, p.terrain.hscale)}")
    assert (frac <= 1.0).all(), (np.argwhere(frac > 1.0)[:8], frac.max())
    hi, lo = ref.raw > 1 + bound, ref.raw < -1 - bound
    assert hi.any() and lo.any()
    assert (got[hi] == 1.0).all() and (got[lo] == -1.0).all() and np.abs(got).max() <= 1.0
    assert (got[TR.ENV_NEGQ] == got[TR.ENV_Q]).all() and (got[TR.ENV_A] == got[TR.ENV_B]).all()
    assert (scan() == got).all()
    env.close()


def test_reset_on_every_type(gpu):
    """Reset of 96 envs spread over both rows of all six types: base z is the sub-terrain's origin z + 1.05 (platform
    tops at +-1.38 m, box platform, noise and slope plateaus), observations (the scan included), state and integers
    match the oracle at test_gpu_rough's tolerances."""
    n = 96
    env = make_env(n, 2, 6)
    p = M.whole_mix()
    bind(env, p)
    ref = planted_start(env, p)
    obs, _ = env.reset()
    np.testing.assert_allclose(obs["policy"].cpu().numpy(), ref.reset(), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(env._fstate.cpu().numpy(), ref.F, rtol=1e-6, atol=1e-6)
    gi = env._istate.cpu().numpy()
    assert (gi == ref.I).all()
    F = env._fstate.cpu().numpy()
    cell = gi[IFIELDS["TERRAIN"][0]]
    lv, ty = cell & 0xFFFF, cell >> 16
    assert {(a, b) for a, b in zip(lv, ty)} == {(r, c) for r in range(2) for c in range(6)}   # every type, both rows
    org = p.terrain.origins[lv, ty]
    o, q = FIELDS["ORIGIN"][0], FIELDS["POS"][0]
    assert (F[o:o + 3].T == org).all()
    assert (F[q + 2] == org[:, 2] + np.float32(1.05)).all()
    assert np.abs(F[q:q + 2].T - org[:, 0:2]).max() <= 0.5 + 1e-6
    assert np.ptp(org[:, 2]) > 2.5
    scan = obs["policy"][:, SCAN0:].cpu().numpy()
    assert np.abs(scan).max() <= 1.0 and scan.std() > 0.01
    env.close()


@pytest.mark.parametrize("name", list(M.CONTACT_CASES))
def test_contact_on_the_hard_row(gpu, name):
    """Reset and 12 teacher-forced MDP steps of 128 envs around four origins planted on the hard row (stairs: platform,
    tread, astride a riser, a tread of the inverted pyramid; boxes: platform, its wall, two walls between boxes; slopes:
    faces along x, along y and on the diagonal of the 0.4 pyramids, and the 10 cm noise): every env within tolerance of
    the oracle or shown threshold-sensitive by it, at most 1.5 % of env-steps off, both feet of at least half the envs
    touch, rewards finite.

    Measured on the MI355X (ForcedParity's report): env-steps off tolerance 1 / 4 / 4 of 1536 (stairs / boxes / slopes),
    every one threshold-sensitive at a 1e-7 perturbation, none unexplained; phys p50 2.8e-5 / 2.8e-5 / 5.9e-5, p99
    4.1e-4 / 3.1e-4 / 5.5e-4; both feet in contact in 0.66 / 0.77 / 0.84 of the envs.  No kernel change was needed."""
    n = TR.N_CONTACT
    env = make_env(n)
    p = M.contact_case(name)
    bind(env, p)
    ref = planted_start(env, p)
    t = p.terrain
    obs, _ = env.reset()
    np.testing.assert_allclose(obs["policy"].cpu().numpy(), ref.reset(), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(env._fstate.cpu().numpy(), ref.F, rtol=1e-6, atol=1e-6)
    assert (env._istate.cpu().numpy() == ref.I).all()
    org = env._fstate.cpu().numpy()[FIELDS["ORIGIN"][0]:FIELDS["ORIGIN"][0] + 3].T
    assert {tuple(o) for o in org} == {tuple(o) for o in t.origins.reshape(-1, 3)}  # all four origins in use
    fp = ForcedParity(env, seed=35)
    both = np.zeros(n, bool)
    for a in M.contact_actions(name):
        (_, gi, _, rew, _, _), _, _, _ = fp.step(a)
        assert np.isfinite(rew).all()
        bits = (gi[IFIELDS["PACK"][0]] >> 13) & 0xFF
        both |= ((bits & 0x0F) != 0) & ((bits & 0xF0) != 0)
    print(f"\ncontact on {name}: both feet in contact in {both.mean():.2f} of the envs; {fp.report()}")
    fp.check(max_bad_frac=0.015)
    assert both.mean() >= 0.5
    env.close()


def mix_env(n, rows=3):
    cfg = K.enable_reference_rough_terrain(TR.contact_cfg(n))
    g = cfg.scene.terrain.terrain_generator
    g.num_rows, g.num_cols, g.border_width = rows, 6, 1.0
    for s in g.sub_terrains.values():
        s.proportion = 1.0
    cfg.sim.device = "cuda:0"
    return H12VelocityEnv(cfg)


def test_curriculum_across_types_and_per_type_log(gpu):
    """An env built from the cfg (3 rows x 6 types): envs placed beyond 4 m of their origin move up, envs short of
    their commanded distance move down, the others stay, each within its own column: cells and origins equal the
    oracle's bit for bit, and Curriculum/terrain_levels/<type> is the mean level of that type's envs."""
    n = 96
    env = mix_env(n)
    t = env.terrain
    assert t.type_names == list(M.COLS) and t.shape == (3 * 160 + 41, 1001) and t.origins.shape == (3, 6, 3)
    O.set_terrain(t.heights, t.hscale, t.x0, t.y0, t.origins)
    ref = O.OracleEnv(env._model, env._ccfg, n)
    ref.F[:], ref.I[:] = env._fstate.cpu().numpy(), env._istate.cpu().numpy()
    obs, _ = env.reset()
    np.testing.assert_allclose(obs["policy"].cpu().numpy(), ref.reset(), rtol=1e-5, atol=2e-5)
    rng = np.random.default_rng(29)
    F = env._fstate.cpu().numpy()
    o, p, cmd = FIELDS["ORIGIN"][0], FIELDS["POS"][0], FIELDS["CMD"][0]
    ang, d = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 6, n)
    d[::3] = rng.uniform(4.2, 6, d[::3].size)                                 # a third certainly beyond 4 m
    F[p] = F[o] + d * np.cos(ang)
    F[p + 1] = F[o + 1] + d * np.sin(ang)
    F[cmd] = rng.uniform(0, 1, n)
    env._fstate.copy_(torch.from_numpy(F))
    ref.F[:] = F
    before = env._istate.cpu().numpy()[IFIELDS["TERRAIN"][0]].copy()
    env.reset()
    ref.reset()
    gi = env._istate.cpu().numpy()
    cell = gi[IFIELDS["TERRAIN"][0]]
    assert (cell == ref.I[IFIELDS["TERRAIN"][0]]).all()
    assert (env._fstate.cpu().numpy()[o:o + 3] == ref.F[o:o + 3].astype(np.float32)).all()
    lv, ty = cell & 0xFFFF, cell >> 16
    assert (ty == before >> 16).all() and set(ty) == set(range(6))            # an env keeps its column
    moved = lv.astype(int) - (before & 0xFFFF)
    assert (moved > 0).any() and (moved < 0).any() and (moved == 0).any()
    assert (env._fstate.cpu().numpy()[o:o + 3].T == t.origins[lv, ty]).all()
    log = env.step(torch.zeros(n, 12, device="cuda"))[4]["log"]
    cell2 = env._istate.cpu().numpy()[IFIELDS["TERRAIN"][0]]
    lv2, ty2 = cell2 & 0xFFFF, cell2 >> 16
    assert float(log["Curriculum/terrain_levels"]) == pytest.approx(lv2.mean())
    for k, name in enumerate(M.COLS):
        assert float(log[f"Curriculum/terrain_levels/{name}"]) == pytest.approx(lv2[ty2 == k].mean(), abs=1e-6)
    assert len([k for k in log if k.startswith("Curriculum/terrain_levels/")]) == 6
    env.close()
    plain = make_env(16)
    keys = plain.step(torch.zeros(16, 12, device="cuda"))[4]["log"].keys()
    assert "Curriculum/terrain_levels" in keys and not [k for k in keys if k.startswith("Curriculum/terrain_levels/")]
    plain.close()


def test_train_play_and_render_on_the_mix(gpu, tmp_path):
    """train.py --terrain isaaclab_rough on a reduced grid (2 x 6) for two iterations: finite losses, the sub-terrain
    table in the run's env.yaml and env.pkl; play.py loads the run and says it plays on the run's mix (read from the
    run's cfg, no flag); one env.render() frame of a robot on the hard stairs is a picture."""
    envv = dict(os.environ, PYTHONPATH=os.pathsep.join([str(PKG), os.environ.get("PYTHONPATH", "")]))
    small = ["--headless", "--num_envs", "64", "agent.num_steps_per_env=8", "agent.save_interval=1",
             "env.scene.terrain.terrain_generator.num_rows=2", "env.scene.terrain.terrain_generator.num_cols=6",
             "env.scene.terrain.terrain_generator.border_width=2.0"]
    p = subprocess.run([sys.executable, str(PKG / "scripts" / "train.py"), "--task", "Isaac-Velocity-Rough-H12_12dof-v0",
                        "--terrain", "isaaclab_rough", "--max_iterations", "2", "--run_name", "mix"] + small,
                       cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    run = next((tmp_path / "logs" / "rsl_rl").glob("*/*_mix"))
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2
    for x in lines:
        losses = {k: v for k, v in x.items() if k.startswith("Loss/")}
        assert losses and all(np.isfinite(v) for v in losses.values()), losses
    import pickle

    import yaml

    sys.path[:0] = [str(PKG / "shims")]
    d = yaml.safe_load((run / "params" / "env.yaml").read_text())["scene"]["terrain"]["terrain_generator"]
    assert list(d["sub_terrains"]) == list(M.COLS) and (d["num_rows"], d["num_cols"], d["raster_scale"]) == (2, 6, 0.05)
    with open(run / "params" / "env.pkl", "rb") as f:
        assert list(pickle.load(f).scene.terrain.terrain_generator.sub_terrains) == list(M.COLS)
    p = subprocess.run([sys.executable, str(PKG / "scripts" / "play.py"), "--task",
                        "Isaac-Velocity-Rough-H12_12dof-Play-v0", "--num_envs", "16", "--load_run", run.name, "--steps",
                        "5"], cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "playing on the run's sub-terrain mix: pyramid_stairs, pyramid_stairs_inv, boxes" in p.stdout
    assert (run / "exported" / "policy.pt").exists()
    # a frame over the hard stairs: the tracked robot stands on the platform of a 0.23 m stair pyramid
    cfg = K.enable_reference_rough_terrain(K.H12RoughEnvCfg())
    g = cfg.scene.terrain.terrain_generator
    g.num_rows, g.num_cols, g.border_width, g.difficulty_range = 1, 6, 1.0, M.HARD
    cfg.scene.num_envs, cfg.sim.device = 6, "cuda:0"
    env = H12VelocityEnv(cfg, render_mode="rgb_array")
    env.reset()
    assert env.terrain.type_names[0] == "pyramid_stairs" and env.terrain.origins[0, 0, 2] > 1.3
    frame = env.render()
    assert isinstance(frame, np.ndarray) and frame.ndim == 3 and frame.shape[2] == 3 and frame.dtype == np.uint8
    assert len(np.unique(frame.reshape(-1, 3), axis=0)) > 20
    env.close()
