"""GPU: the privileged ("critic") observation group (h12env.priv, csrc/h12_priv.hip).

Values: the terms shared with the policy group and the height scan against the fp64 oracle's observe() of the same
state with corruption off (the state copied as tests/helpers/forced.py does), base_lin_vel against its definition in
float64, base_height on the heightfield against tests/helpers/terrain_ref.mesh_height -- all within the tolerance the
forced harness applies to observation rows, |g - o| <= TOL_OBS * max(1, |o|).  The copied terms are bit-equal to the
state fields they come from.  Then: the group only reads (an env with it equals an env without), a returned tensor
lives for one further step, a non-finite base pose leaves every other row alone, and the runner trains with it."""
import copy
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import oracle as O
from forced import TOL_OBS
from h12env import cfg as K
from h12env import priv
from h12env._abi import F as FIELDS
from h12env._abi import I as IFIELDS
from h12env.env import H12VelocityEnv
from terrain_ref import mesh_height

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "h1v2-isaac_amd" / "shims"), str(ROOT / "h1v2-isaac_amd" / "scripts")]

pytestmark = pytest.mark.gpu

FRAME_WIDTHS = (3, 3, 3, 12, 12, 12)  # ang_vel, gravity, command, joint_pos, joint_vel, actions


def make(name, n, critic=True, tweak=None, **kw):
    cfg = getattr(K, name)()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    if name == "H12RslEnvCfg":
        cfg.events.add_base_mass = K.MassEventCfg(".*torso_link", (0.0, 6.0), "add")  # every randomised term is live
    g = cfg.scene.terrain.terrain_generator
    if g is not None:  # a smaller grid keeps the oracle's terrain setup quick
        g.num_rows, g.num_cols, g.border_width = 6, 8, 5.0
    if critic:
        cfg.observations.critic = K.CriticObsCfg()
    if tweak is not None:
        tweak(cfg)
    env = H12VelocityEnv(cfg, **kw)
    if env.terrain is not None:
        t = env.terrain
        O.set_terrain(t.heights, t.hscale, t.x0, t.y0, t.origins)
    return env


def run_steps(env, steps, seed, force_reset_at=None):
    """Random-action steps; at step force_reset_at env 0 (and env n - 1) is put one step before its time-out, so that
    step resets it."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = None
    for t in range(steps):
        if t == force_reset_at:
            buf = env.episode_length_buf
            buf[0] = env.max_episode_length - 1
            buf[-1] = env.max_episode_length - 1
        out = env.step(torch.randn(env.num_envs, 12, generator=g).to(env.device))
    return out


def state(env):
    torch.cuda.synchronize()
    return env._fstate.cpu().numpy().copy(), env._istate.cpu().numpy().copy()


def fld(F, name):
    o, c = FIELDS[name]
    return F[o:o + c]


def columns(env):
    w, table = priv.layout(env.terrain is not None)
    assert w == env.critic_obs_dim
    return {name: slice(o, o + k) for name, o, k in table}


def close(g, o):
    return np.abs(g - o) <= TOL_OBS * np.maximum(1.0, np.abs(o))


def oracle_frame(env, F, I):
    """The oracle's noise-free observation of the state: (shared 45 columns in frame order, lin_vel or None, scan or
    None)."""
    cc = copy.copy(env._ccfg)
    cc.enable_corruption = 0
    ref = O.OracleEnv(env._model, cc, env.num_envs, env.env_offset)
    ref.F[:], ref.I[:] = F, I
    row = ref.observe(np.ones(env.num_envs, np.uint8)).astype(np.float64)
    if env.terrain is not None:
        return row[:, 3:48], row[:, 0:3], row[:, 48:235]
    return newest_slots(row, int(cc.history_length)), None, None


def newest_slots(row, h):
    parts, off = [], 0
    for w in FRAME_WIDTHS:  # term-major history, oldest slot first
        parts.append(row[:, off + (h - 1) * w:off + h * w])
        off += h * w
    assert off == row.shape[1]
    return np.concatenate(parts, axis=1)


def lin_vel_ref(env, F):
    """R^T (VLIN + (R WANG) x (R ROOT_COM)) in float64."""
    q = fld(F, "QUAT").astype(np.float64).T
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    c = np.asarray(list(env._model.root_com), np.float64)
    ww = np.einsum("nij,nj->ni", R, fld(F, "WANG").astype(np.float64).T)
    cw = np.einsum("nij,j->ni", R, c)
    v = fld(F, "VLIN").astype(np.float64).T + np.cross(ww, cw)
    return np.einsum("nji,nj->ni", R, v)


def check_copied(env, crit, F, I, force):
    """Bit-equal: commands, actions, timers, lags, friction, mass, contact flags, foot forces."""
    col = columns(env)
    s = priv.term_scales(env.cfg)
    f32 = np.float32
    pk = I[IFIELDS["PACK"][0]]
    eq = lambda name, want: np.testing.assert_array_equal(crit[:, col[name]], want, err_msg=name)  # noqa: E731
    eq("velocity_commands", fld(F, "CMD").T * f32(s["velocity_commands"]))
    eq("actions", fld(F, "ACT").T * f32(s["actions"]))
    eq("feet_air_time", fld(F, "AIR").T)
    eq("feet_contact_time", fld(F, "CONTACT").T)
    eq("actuator_lag", np.stack([(pk >> (3 * g)) & 7 for g in range(3)], 1).astype(f32))
    contact = np.stack([((pk >> (13 + 4 * f)) & 0xF) != 0 for f in range(2)], 1)
    eq("feet_contact", contact.astype(f32))
    fresh = ((pk >> 9) & 3) == 0
    want = force * f32(s["feet_force"])
    want[fresh] = 0.0
    eq("feet_force", want)
    cc = env._ccfg
    mu = fld(F, "MU").T if cc.per_env_friction else np.tile(np.array([cc.mu_static, cc.mu_dynamic], f32), (len(pk), 2))
    eq("sole_friction", mu)
    eq("added_mass", fld(F, "DMASS").T if cc.per_env_mass else np.zeros((len(pk), 1), f32))
    return fresh, contact


# ---------------------------------------------------------------------------------------------- values
# the plane kernel owns 64 envs per block, the heightfield kernel 16: both block edges +- 1 and a ragged tail
CASES = ([(t, n) for t in ("H12FlatEnvCfg", "H12RslEnvCfg") for n in (1, 63, 65, 97)] +
         [("H12RoughEnvCfg", n) for n in (15, 17, 97)])


@pytest.mark.parametrize("task,n", CASES, ids=[f"{t[3:-6]}-{n}" for t, n in CASES])
def test_values_against_the_oracle_and_the_state(gpu, task, n):
    env = make(task, n)
    obs, _ = env.reset()
    assert obs["critic"].shape == (n, 252 if env.terrain is not None else 65)
    assert env.observation_manager.group_obs_dim["critic"] == (env.critic_obs_dim,)
    assert env.observation_manager.active_terms["critic"] == priv.term_names(env.terrain is not None)
    assert env.single_observation_space["critic"].shape == (env.critic_obs_dim,)
    obs = run_steps(env, 30, seed=n, force_reset_at=29)[0]
    F, I = state(env)
    crit = obs["critic"].cpu().numpy()
    force = env.foot_contact_force.cpu().numpy()
    for k in ("critic", "policy"):
        assert torch.equal(env.get_observations()[k], obs[k]) and torch.equal(env.obs_buf[k], obs[k])
        assert torch.equal(env.observation_manager.compute()[k], obs[k])
    assert np.isfinite(crit).all()
    col = columns(env)
    shared, lin, scan = oracle_frame(env, F, I)
    got = crit[:, 3:48].astype(np.float64)
    ok = close(got, shared)
    print(f"{task} n={n}: shared terms max err / tol {(np.abs(got - shared) / (TOL_OBS * np.maximum(1, np.abs(shared)))).max():.3g}")
    assert ok.all(), np.argwhere(~ok)[:8]
    lv = lin_vel_ref(env, F)
    assert close(crit[:, col["base_lin_vel"]].astype(np.float64), lv).all()
    z = fld(F, "POS")[2].astype(np.float64)
    if env.terrain is not None:
        assert close(crit[:, col["base_lin_vel"]].astype(np.float64), lin).all()
        g = crit[:, col["height_scan"]].astype(np.float64)
        print(f"scan max err / tol {(np.abs(g - scan) / (TOL_OBS * np.maximum(1, np.abs(scan)))).max():.3g}")
        assert close(g, scan).all()
        t = env.terrain
        cells = I[IFIELDS["TERRAIN"][0]]
        assert len(np.unique(cells)) > 1 or n < 97  # envs in different terrain cells
        h, _, _ = mesh_height(t.heights, t.hscale, t.x0, t.y0, fld(F, "POS")[0], fld(F, "POS")[1])
        assert np.abs(h).max() > 0
        z = z - h
    assert close(crit[:, col["base_height"]].astype(np.float64)[:, 0], z).all()
    fresh, _ = check_copied(env, crit, F, I, force)
    assert fresh[0] and fresh[-1]  # the forced time-outs of the last step
    env.close()


def test_copied_terms_are_bit_equal_over_a_run_with_resets_and_contacts(gpu):
    env = make("H12RslEnvCfg", 97)
    obs, _ = env.reset()
    F, I = state(env)
    fresh, _ = check_copied(env, obs["critic"].cpu().numpy(), F, I, env.foot_contact_force.cpu().numpy())
    assert fresh.all()  # reset(): every env is new, every foot force reads 0
    assert (obs["critic"][:, columns(env)["feet_force"]] == 0).all()
    n_fresh = n_contact = n_air = n_force = 0
    g = torch.Generator(device="cpu").manual_seed(5)
    for t in range(30):
        if t == 12:
            env.episode_length_buf[3] = env.max_episode_length - 1
        obs = env.step(0.3 * torch.randn(97, 12, generator=g).to(env.device))[0]
        F, I = state(env)
        crit = obs["critic"].cpu().numpy()
        fresh, contact = check_copied(env, crit, F, I, env.foot_contact_force.cpu().numpy())
        if t == 12:
            assert fresh[3]
        if t >= 1:
            n_fresh += int(fresh.sum())
        n_contact += int(contact.sum())
        n_air += int((~contact).sum())
        n_force += int((crit[:, columns(env)["feet_force"]] > 0).sum())
    print(f"fresh env-steps {n_fresh}, feet in contact {n_contact}, in the air {n_air}, non-zero forces {n_force}")
    assert n_fresh >= 1 and n_contact >= 1 and n_force >= 1, (n_fresh, n_contact, n_air, n_force)
    mu = obs["critic"][:, columns(env)["sole_friction"]]
    assert len(torch.unique(mu)) > 4 and len(torch.unique(obs["critic"][:, columns(env)["added_mass"]])) > 4
    env.close()


@pytest.mark.parametrize("task", ["H12FlatEnvCfg", "H12RslEnvCfg_PLAY", "H12RoughEnvCfg_PLAY"])
def test_critic_matches_the_policy_row_without_corruption(gpu, task):
    env = make(task, 97, tweak=lambda c: setattr(c.observations.policy, "enable_corruption", False))
    assert not env._ccfg.enable_corruption
    env.reset()
    obs = run_steps(env, 30, seed=2)[0]
    torch.cuda.synchronize()
    pol, crit = obs["policy"].cpu().numpy().astype(np.float64), obs["critic"].cpu().numpy().astype(np.float64)
    if env.terrain is not None:
        assert close(crit[:, 0:48], pol[:, 0:48]).all() and close(crit[:, 48:235], pol[:, 48:235]).all()
    else:
        assert close(crit[:, 3:48], newest_slots(pol, int(env._ccfg.history_length))).all()
    env.close()


# ---------------------------------------------------------------------------------------------- behaviour
def test_the_group_only_reads(gpu):
    a, b = make("H12RslEnvCfg", 65, critic=True), make("H12RslEnvCfg", 65, critic=False)
    oa, _ = a.reset()
    ob, _ = b.reset()
    assert set(ob) == {"policy"} and set(oa) == {"policy", "critic"} and b.critic_obs_dim is None
    assert "critic" not in b.observation_manager.group_obs_dim and "critic" not in b.single_observation_space.spaces
    assert torch.equal(oa["policy"], ob["policy"])
    g = torch.Generator(device="cpu").manual_seed(11)
    for _ in range(50):
        act = torch.randn(65, 12, generator=g).cuda()
        ra, rb = a.step(act), b.step(act)
        assert torch.equal(ra[0]["policy"], rb[0]["policy"])
        for x, y in zip(ra[1:4], rb[1:4]):
            assert torch.equal(x, y)
    assert torch.equal(a._state, b._state)
    a.close()
    b.close()


def test_returned_rows_live_for_one_further_step_and_snapshot_restores_them(gpu):
    env = make("H12FlatEnvCfg", 65)
    env.reset()
    run_steps(env, 3, seed=1)
    act = torch.zeros(65, 12, device="cuda")
    c_t = env.step(act)[0]["critic"]
    keep = c_t.clone()
    snap = env.snapshot()
    c_t1 = env.step(act)[0]["critic"]
    assert c_t1.data_ptr() != c_t.data_ptr()
    assert torch.equal(c_t, keep) and not torch.equal(c_t1, keep)
    want = c_t1.clone()
    env.step(act)
    env.restore(snap)
    assert torch.equal(env.get_observations()["critic"], keep)
    assert torch.equal(env.step(act)[0]["critic"], want)
    env.close()
    env = make("H12FlatEnvCfg", 65, obs_copy=True)
    env.reset()
    c0 = env.step(act)[0]["critic"]
    keep = c0.clone()
    for _ in range(3):
        env.step(act)
    assert torch.equal(c0, keep)  # obs_copy: the returned tensor is the caller's
    env.close()


def test_bind_rollout_is_refused_with_the_group(gpu):
    from h12env.rollout import RolloutRecorder

    env = make("H12FlatEnvCfg", 64)
    env.reset()
    rec = RolloutRecorder(64, 4, gpu, 10)
    with pytest.raises(ValueError, match="critic"):
        env.bind_rollout(rec)
    env.close()
    env = make("H12FlatEnvCfg", 64, critic=False)
    env.reset()
    env.bind_rollout(rec)  # the same recorder binds to the env without the group
    env.unbind_rollout()
    env.close()


def test_non_finite_base_pose_leaves_the_other_rows_alone(gpu):
    """The heightfield indices come from bit-checked values and are clamped with integer operations: a NaN / inf / huge
    base pose reads the heightfield inside its bounds (csrc/h12_priv.hip, sane_bits / ground_at)."""
    env = make("H12RoughEnvCfg", 97)
    env.reset()
    run_steps(env, 5, seed=4)
    env._critic_rows()
    before = env._crit[env._k].clone()
    saved = env._state.clone()
    pos, quat = FIELDS["POS"][0], FIELDS["QUAT"][0]
    planted = {5: (pos, float("nan")), 7: (pos + 1, float("inf")), 9: (pos, 1.0e30), 11: (quat + 2, float("nan")),
               13: (pos + 1, -4.0e5), 96: (pos, -float("inf"))}
    for e, (f, v) in planted.items():
        env._fstate[f, e] = v
    env._critic_rows()
    torch.cuda.synchronize()
    after = env._crit[env._k]
    others = [e for e in range(97) if e not in planted]
    assert torch.equal(after[others], before[others])
    assert torch.isfinite(after[13]).all()  # a finite pose far outside the grid reads the flat border
    env._state.copy_(saved)
    env._critic_rows()
    assert torch.equal(env._crit[env._k], before)
    env.close()


# ---------------------------------------------------------------------------------------------- training
@pytest.mark.parametrize("symmetry", [None, "both"])
def test_runner_trains_with_the_group_and_the_checkpoint_needs_the_flag(gpu, tmp_path, monkeypatch, symmetry):
    import train
    from h12env import ppo

    seen = []
    learn = ppo.OnPolicyRunner.learn

    def spy(self, *a, **kw):
        seen.append(self)
        return learn(self, *a, **kw)

    monkeypatch.setattr(ppo.OnPolicyRunner, "learn", spy)
    monkeypatch.chdir(tmp_path)
    argv = ["--task", "Isaac-Velocity-Flat-H12_12dof-v0", "--headless", "--num_envs", "256", "--max_iterations", "2",
            "--privileged_critic", "agent.save_interval=1"]
    if symmetry:
        argv += ["--symmetry", symmetry]
    assert train.main(argv) == 0
    runner = seen[0]
    alg = runner.alg
    assert alg.policy.critic[0].weight.shape[1] == 65 and alg.policy.actor[0].weight.shape[1] == 450
    assert alg.storage.t["privileged_observations"].shape == (24, 256, 65)
    assert getattr(alg, "_ga", None) is not None and alg._ga_cobs.shape == (256, 65)  # graph-captured collection
    assert alg._graph is not None                                                       # ... and update
    run = next((tmp_path / "logs" / "rsl_rl" / "h12_12dof_flat").iterdir())
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2 and all(v == v for x in lines for v in x.values() if isinstance(v, float))
    assert ("Loss/symmetry" in lines[-1]) == bool(symmetry)
    assert "critic:" in (run / "params" / "env.yaml").read_text()
    ck = run / "model_2.pt"

    import gymnasium as gym
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    task = "Isaac-Velocity-Flat-H12_12dof-Play-v0"
    agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    for flag in (True, False):
        cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
        if flag:
            K.enable_privileged_critic(cfg)
        env = RslRlVecEnvWrapper(gym.make(task, cfg=cfg))
        play = ppo.OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0")
        if flag:
            play.load(str(ck))
            policy = play.get_inference_policy(device="cuda:0")
            obs, _ = env.get_observations()
            with torch.inference_mode():
                for _ in range(5):
                    obs, rew, _, extras = env.step(policy(obs))
            assert torch.isfinite(obs).all() and extras["observations"]["critic"].shape[1] == 65
        else:
            with pytest.raises(ValueError, match=r"65-wide.*450 wide.*--privileged_critic"):
                play.load(str(ck))
        env.close()
