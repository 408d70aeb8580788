"""CPU: the mirror map of the H1-2 tasks (h12env.symmetry) and rsl_rl 2.3's symmetry options in the PPO runner.

The tables are involutions built from term and joint names; the map itself is pinned by the physics on the CPU oracle
(mirrored actions in mirrored envs give mirrored observations, and no other column / sign candidate comes close) and,
for the height scan, by two oracle runs on a heightfield and on its y-mirrored copy.  The PPO semantics (augmentation,
mirror loss, logging only) are compared with a plain torch restatement of rsl_rl's update written here."""
import copy
import ctypes as C
import json
import math
import random
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch.distributions import Normal

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "shims"))
sys.path.insert(0, str(ROOT / "tests" / "helpers"))

import mirror_check as MC  # noqa: E402
import oracle as O  # noqa: E402
from h12env import cfg as K  # noqa: E402
from h12env import model as M  # noqa: E402
from h12env import symmetry as S  # noqa: E402
from h12env._abi import F as FIELDS  # noqa: E402
from h12env.ppo import PPO, ActorCritic, OnPolicyRunner  # noqa: E402
from h12env.startup import apply_to_arrays, startup_state  # noqa: E402

LAYOUTS = {"flat": (K.H12FlatEnvCfg, 450), "rsl": (K.H12RslEnvCfg, 270), "cat": (K.H12CaTEnvCfg, 270),
           "rough": (K.H12RoughEnvCfg, 235)}


def planted(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    flat = x.view(-1)
    for i, v in enumerate((float("nan"), float("inf"), float("-inf"), -0.0, 0.0)):
        flat[i::11][: max(1, flat.numel() // 40)] = v
    return x


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- 1. tables
def all_tables():
    return [(name, S.mirror_table(c())) for name, (c, _) in LAYOUTS.items()] + [("actions", S.action_table())]


def test_tables_are_involutions_of_the_layout_widths():
    for name, t in all_tables():
        want = 12 if name == "actions" else LAYOUTS[name][1]
        assert t.width == want and t.src.dtype == torch.int32 and t.flip.dtype == torch.bool, name
        s = t.src.long()
        assert torch.equal(s[s], torch.arange(want)), name
        assert torch.equal(t.flip[s], t.flip), name
        x = planted((7, want), seed=want)
        assert torch.equal(bits(t.mirror(t.mirror(x))), bits(x)), name
        assert not torch.equal(bits(t.mirror(x)), bits(x)), name
        p = t.packed("cpu")
        assert torch.equal(p & 0x7FFFFFFF, t.src) and torch.equal(p < 0, t.flip), name
    # mirror_obs finds the layout by its width; the env cfg and a wrapped env give the same table
    x = planted((3, 450))
    assert torch.equal(bits(S.mirror_obs(x)), bits(S.mirror_table(K.H12FlatEnvCfg()).mirror(x)))
    assert torch.equal(S.mirror_table(K.H12RslEnvCfg()).src, S.mirror_table(K.H12CaTEnvCfg()).src)
    with pytest.raises(ValueError, match="pass the env"):
        S.mirror_obs(torch.zeros(2, 44))


def test_table_rules_per_term():
    """The newest frame of the Flat layout, spelled out: term-major history, oldest slot first."""
    t = S.mirror_table(K.H12FlatEnvCfg())
    h = 10
    x = torch.arange(1.0, 451.0).unsqueeze(0)
    y = t.mirror(x)[0]
    for slot in (0, 9):
        w0, g0, c0 = 0 + 3 * slot, 3 * h + 3 * slot, 6 * h + 3 * slot
        assert y[w0:w0 + 3].tolist() == [-x[0, w0], x[0, w0 + 1], -x[0, w0 + 2]]            # axial
        assert y[g0:g0 + 3].tolist() == [x[0, g0], -x[0, g0 + 1], x[0, g0 + 2]]             # polar
        assert y[c0:c0 + 3].tolist() == [x[0, c0], -x[0, c0 + 1], -x[0, c0 + 2]]            # (vx, -vy, -wz)
        for term in range(3):
            q0 = 9 * h + term * 12 * h + 12 * slot
            names = M.joint_names()
            for j, n in enumerate(names):
                partner = names.index(n.replace("left_", "RIGHT_").replace("right_", "left_").replace("RIGHT_", "right_"))
                sign = -1.0 if ("_yaw_" in n or "_roll_" in n) else 1.0
                assert y[q0 + j] == sign * x[0, q0 + partner], (term, slot, n)
    r = S.mirror_table(K.H12RoughEnvCfg())
    z = torch.arange(235.0).unsqueeze(0)
    scan = r.mirror(z)[0, 48:].view(11, 17)
    assert torch.equal(scan, z[0, 48:].view(11, 17).flip(0))
    assert r.mirror(z)[0, :3].tolist() == [0.0, -1.0, 2.0]                                  # base_lin_vel: polar


def test_unknown_term_raises():
    with pytest.raises(ValueError, match="no mirror rule"):
        S.table_from_terms(["base_ang_vel", "foot_contact"], 1)
    env = SimpleNamespace(observation_manager=SimpleNamespace(active_terms={"policy": ["imu_orientation"]},
                                                              group_obs_dim={"policy": (4,)}),
                          cfg=K.H12FlatEnvCfg())
    with pytest.raises(ValueError, match="imu_orientation"):
        S.mirror_table(env)
    with pytest.raises(ValueError):
        S.mirror_table(K.H12FlatEnvCfg(), "critic")


def test_table_follows_the_joint_names(monkeypatch):
    names = M.joint_names()
    order = list(range(12))
    random.Random(3).shuffle(order)
    shuffled = [names[i] for i in order]
    assert shuffled != names
    monkeypatch.setattr(M, "joint_names", lambda: list(shuffled))
    t = S.action_table()
    for j, n in enumerate(shuffled):
        partner = shuffled[int(t.src[j])]
        assert {n.split("_", 1)[0], partner.split("_", 1)[0]} == {"left", "right"}
        assert n.split("_", 1)[1] == partner.split("_", 1)[1]
        assert bool(t.flip[j]) == ("_yaw_" in n or "_roll_" in n)
    assert not torch.equal(t.src, torch.tensor([6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5], dtype=torch.int32))
    # a joint whose name and model axis disagree is caught when the table is built
    monkeypatch.setattr(M, "joint_names", lambda: [n.replace("hip_pitch", "hip_yaw_b") for n in names])
    with pytest.raises((AssertionError, ValueError, KeyError)):
        S.action_table()


def test_augment_signature_and_none():
    obs, act = planted((5, 270)), planted((5, 12), 1)
    o, a = S.augment(obs=obs, actions=act, env=K.H12RslEnvCfg(), obs_type="policy")
    assert o.shape == (10, 270) and a.shape == (10, 12)
    assert torch.equal(bits(o[:5]), bits(obs)) and torch.equal(bits(o[5:]), bits(S.mirror_obs(obs)))
    assert torch.equal(bits(a[:5]), bits(act)) and torch.equal(bits(a[5:]), bits(S.mirror_actions(act)))
    assert S.augment(obs=obs)[1] is None and S.augment(actions=act)[0] is None
    idx = torch.tensor([4, 0, 0])
    assert torch.equal(bits(S.augment(obs=obs, idx=idx)[0]), bits(S.augment(obs=obs[idx])[0]))
    assert S.resolve_func("h12env.symmetry:augment") is S.augment and S.resolve_func(S.augment) is S.augment
    with pytest.raises(ValueError):
        S.resolve_func(None)


# ---------------------------------------------------------------------------------------------- 2. physics
def oracle_pairs(model, layout):
    cfg = MC.pair_cfg(layout)
    env = O.OracleEnv(model, cfg.to_c(), MC.N_ENVS)
    env.reset()
    c0 = FIELDS["CMD"][0]
    assert FIELDS["CMD"] == (61, 3)
    MC.mirror_commands(env.F[c0:c0 + 3])
    a_rows, b_rows = [], []
    for k, act in enumerate(MC.paired_actions()):
        obs, _, term, _, _ = env.step(act, k + 1)
        assert not term.any()
        a_rows.append(obs[0::2])
        b_rows.append(obs[1::2])
    return cfg, np.concatenate(a_rows), np.concatenate(b_rows)


@pytest.mark.parametrize("layout,columns", [("flat", 45), ("rough_plane", 48)])
def test_map_is_pinned_by_the_physics(model, layout, columns):
    """Measured on the oracle: 0 misidentified columns, worst ratio 0.0053 (Flat) against the 0.1 asserted.  The Rough
    layout runs on the plane (its scan is a constant there, so the scan columns are left to the heightfield test) and
    puts base_lin_vel through the same identification."""
    cfg, obs_a, obs_b = oracle_pairs(model, layout)
    table = S.mirror_table(cfg)
    terms, h = S._cfg_terms(cfg, "policy")
    bad, worst, seen = MC.identify(table, terms, h, obs_a, obs_b)
    print(f"\n{layout}: {seen} columns, {len(bad)} misidentified, worst ratio {worst:.4f}")
    assert seen == columns
    assert not bad, bad
    assert worst <= MC.MARGIN


# ---------------------------------------------------------------------------------------------- 3. height scan
def test_height_scan_mirror_on_a_y_mirrored_heightfield(model):
    """Two oracle runs, Rough-Play cfg (no corruption), robot at yaw 0 on the line y = 0: one on a heightfield that is
    asymmetric in y, one on its y-mirrored copy.  The mirrored row of the first equals the row of the second.

    The heightfield is a sum a(ix) + b(iy), so every cell is planar: the mesh splits a cell along one fixed diagonal,
    which a y-mirror turns into the other one, and only on planar cells do the two triangulations agree.  The mirror
    line is y = 0 so that the ray coordinates +-0.1 k are exact mirror images in floating point.

    Tolerance: 4 x the largest difference between two observe() calls of one oracle state.  Measured: 0.0 -- observe()
    is deterministic with corruption off -- so the rows are compared exactly (measured difference 0.0; the unmirrored
    rows differ by 0.17)."""
    nx, ny, hs = 33, 25, 0.125
    rng = np.random.default_rng(5)
    units = np.cumsum(rng.integers(-40, 41, (1, ny)), axis=1) + np.cumsum(rng.integers(-30, 31, (nx, 1)), axis=0) + 600
    heights = (units / 1024.0).astype(np.float32)
    assert np.abs(heights - heights[:, ::-1]).max() > 0.1
    x0, y0 = -(nx - 1) * hs / 2, -(ny - 1) * hs / 2
    cfg = K.H12RoughEnvCfg_PLAY()
    n = 2
    cfg.scene.num_envs = n
    g = cfg.scene.terrain.terrain_generator
    g.num_rows, g.num_cols, g.border_width = 2, 2, 4.0
    assert not cfg.observations.policy.enable_corruption
    st = startup_state(cfg, n)

    def rows(h):
        O.set_terrain(h, hs, x0, y0, np.zeros((1, 1, 3), np.float32))
        env = O.OracleEnv(model, cfg.to_c(), n)
        apply_to_arrays(st, env.F, env.I)
        env.reset()
        p, q, c = FIELDS["POS"][0], FIELDS["QUAT"][0], FIELDS["CMD"][0]
        env.F[p:p + 3] = np.array([[0.25], [0.0], [1.3]], np.float32)
        env.F[q:q + 4] = np.array([[1.0], [0.0], [0.0], [0.0]], np.float32)
        env.F[c:c + 3] = np.array([[0.5], [0.0], [0.0]], np.float32)   # a command that is its own mirror image
        return env.observe(), env.observe()

    a, a_again = rows(heights)
    b, b_again = rows(np.ascontiguousarray(heights[:, ::-1]))
    tol = 4.0 * max(np.abs(a - a_again).max(), np.abs(b - b_again).max())
    scan = a[:, 48:]
    assert np.abs(scan).max() < 1.0 and scan.max() - scan.min() > 0.1     # unclipped relief under the rays
    m = S.mirror_table(cfg).mirror(torch.from_numpy(a)).numpy()
    print(f"\nobserve() repeat tolerance {tol}, mirrored difference {np.abs(m - b).max()}, "
          f"unmirrored {np.abs(a - b).max()}")
    assert tol == 0.0
    assert np.abs(m - b).max() <= tol
    assert np.abs(a - b).max() > 0.05


# ---------------------------------------------------------------------------------------------- 4. PPO semantics
OBS_T = S.MirrorTable([3, 4, 5, 0, 1, 2], [False, True, False, False, True, False])
ACT_T = S.MirrorTable([0, 2, 1], [True, False, False])
TOY_ENV = SimpleNamespace(mirror_tables={"policy": OBS_T, "actions": ACT_T})
HP = dict(num_learning_epochs=1, num_mini_batches=2, clip_param=0.2, value_loss_coef=0.7, entropy_coef=0.01,
          learning_rate=1e-3, max_grad_norm=1e9, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01,
          normalize_advantage_per_mini_batch=True, device="cpu")
MODES = {"augment": (True, False), "mirror_loss": (False, True), "both": (True, True), "logging": (False, False)}


def sym_cfg(mode, func="h12env.symmetry:augment", coeff=0.5):
    a, m = MODES[mode]
    return {"use_data_augmentation": a, "use_mirror_loss": m, "mirror_loss_coeff": coeff,
            "data_augmentation_func": func, "_env": TOY_ENV}


def matrix(t):
    p = torch.zeros(t.width, t.width)
    for j in range(t.width):
        p[int(t.src[j]), j] = -1.0 if bool(t.flip[j]) else 1.0
    return p


def toy_alg(symmetry_cfg, seed=0):
    torch.manual_seed(seed)
    pol = ActorCritic(6, 6, 3, [16], [16], init_noise_std=0.8)
    alg = PPO(pol, symmetry_cfg=symmetry_cfg, **HP)
    alg.init_storage(8, 6, [6], None, [3])
    g = torch.Generator().manual_seed(11)
    for k, v in alg.storage.t.items():
        v.copy_(torch.randn(v.shape, generator=g) * (0.1 if k == "sigma" else 1.0))
    alg.storage.t["sigma"].abs_().add_(0.7)
    alg.storage.t["mu"].mul_(0.1)
    return alg


def restated(policy, b, idx, mode, coeff, lr):
    """rsl_rl 2.3.3 PPO.update's loop body with symmetry, in plain torch: (loss, parts, new learning rate)."""
    aug, mirror = MODES[mode]
    po, pa = matrix(OBS_T), matrix(ACT_T)
    n = idx.shape[0]
    obs, actions = b["observations"][idx], b["actions"][idx]
    tv, adv, ret, olp = b["values"][idx], b["advantages"][idx], b["returns"][idx], b["actions_log_prob"][idx]
    omu, osig = b["mu"][idx], b["sigma"][idx]
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    if aug:
        obs, actions = torch.cat([obs, obs @ po]), torch.cat([actions, actions @ pa])
        tv, adv, ret, olp = (t.repeat(2, 1) for t in (tv, adv, ret, olp))
    mean = policy.actor(obs)
    dist = Normal(mean, policy.std.expand_as(mean))
    logp = dist.log_prob(actions).sum(-1)
    value = policy.critic(obs)
    mu, sig, ent = mean[:n], dist.stddev[:n], dist.entropy().sum(-1)[:n]
    with torch.no_grad():
        kl = torch.sum(torch.log(sig / osig + 1e-5) + (osig.square() + (omu - mu).square()) / (2.0 * sig.square()) - 0.5,
                       dim=-1).mean().item()
    if kl > HP["desired_kl"] * 2.0:
        lr = max(1e-5, lr / 1.5)
    elif 0.0 < kl < HP["desired_kl"] / 2.0:
        lr = min(1e-2, lr * 1.5)
    ratio = torch.exp(logp - olp.squeeze(-1))
    a = adv.squeeze(-1)
    surrogate = torch.max(-a * ratio, -a * ratio.clamp(1.0 - HP["clip_param"], 1.0 + HP["clip_param"])).mean()
    vc = tv + (value - tv).clamp(-HP["clip_param"], HP["clip_param"])
    vloss = torch.max((value - ret).square(), (vc - ret).square()).mean()
    loss = surrogate + HP["value_loss_coef"] * vloss - HP["entropy_coef"] * ent.mean()
    obs_m = obs if aug else torch.cat([obs, obs @ po])
    mean_all = policy.actor(obs_m.detach())
    target = (mean_all[:n] @ pa).detach()
    sloss = torch.nn.functional.mse_loss(mean_all[n:], target)
    if mirror:
        loss = loss + coeff * sloss
    return loss, (vloss, surrogate, ent.mean(), sloss), lr


@pytest.mark.parametrize("mode", ["augment", "mirror_loss", "both"])
def test_minibatch_equals_the_plain_torch_restatement(mode):
    alg = toy_alg(sym_cfg(mode))
    ref = copy.deepcopy(alg.policy)
    b = alg._batch()
    idx = torch.randperm(48, generator=torch.Generator().manual_seed(2))[:24]
    loss, parts, lr = restated(ref, b, idx, mode, 0.5, HP["learning_rate"])
    loss.backward()
    stats = torch.zeros(4)
    alg._minibatch(b, idx, stats)
    for got, want in zip(stats, parts):
        torch.testing.assert_close(got, want.detach())
    got_loss = stats[1] + HP["value_loss_coef"] * stats[0] - HP["entropy_coef"] * stats[2]
    if MODES[mode][1]:
        got_loss = got_loss + 0.5 * stats[3]
    torch.testing.assert_close(got_loss, loss.detach())
    assert alg.learning_rate == lr
    assert float(parts[3].detach()) > 1e-4                       # an untrained actor is not symmetric
    for (name, p), q in zip(alg.policy.named_parameters(), ref.parameters()):
        assert p.grad is not None and q.grad is not None, name
        torch.testing.assert_close(p.grad, q.grad, msg=lambda m: f"{name}: {m}")


def test_mirror_loss_changes_the_actor_gradient_only_when_switched_on():
    b_idx = torch.arange(24)
    grads = {}
    for mode in ("logging", "mirror_loss"):
        alg = toy_alg(sym_cfg(mode))
        alg._minibatch(alg._batch(), b_idx, torch.zeros(4))
        grads[mode] = [p.grad.clone() for p in alg.policy.actor.parameters()]
    none = toy_alg(None)
    none._minibatch(none._batch(), b_idx, torch.zeros(3))
    for g, h in zip(grads["logging"], none.policy.actor.parameters()):
        assert torch.equal(g, h.grad)
    assert any(not torch.equal(g, h) for g, h in zip(grads["logging"], grads["mirror_loss"]))


# ---------------------------------------------------------------------------------------------- 5. logging only
def test_logging_only_mode_updates_as_without_symmetry():
    a, b = toy_alg(sym_cfg("logging")), toy_alg(None)
    la, lb = a.update(), b.update()
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    assert "symmetry" in la and math.isfinite(la["symmetry"]) and la["symmetry"] > 0.0
    assert "symmetry" not in lb
    assert {k: v for k, v in la.items() if k != "symmetry"} == lb
    c = toy_alg(sym_cfg("both"))
    c.update()
    assert any(not torch.equal(p, q) for p, q in zip(c.policy.parameters(), b.policy.parameters()))


# ---------------------------------------------------------------------------------------------- 6. runner, train.py
def toy_augment(obs=None, actions=None, env=None, obs_type="policy"):
    """A user's data_augmentation_func with exactly rsl_rl's signature."""
    return S.augment(obs=obs, actions=actions, env=env, obs_type=obs_type)


@pytest.mark.parametrize("func", ["h12env.symmetry:augment", toy_augment], ids=["string", "callable"])
def test_runner_hands_symmetry_cfg_to_ppo_and_logs_it(tmp_path, func):
    from isaaclab_rl.rsl_rl import RslRlOnPolicyRunnerCfg, RslRlSymmetryCfg, RslRlVecEnvWrapper
    from toy_sym import ToyEnvCfg, ToySymEnv

    c = RslRlOnPolicyRunnerCfg(device="cpu", num_steps_per_env=8, save_interval=1000, experiment_name="toy")
    c.policy.actor_hidden_dims = c.policy.critic_hidden_dims = [16]
    assert c.algorithm.symmetry_cfg is None
    c.algorithm.symmetry_cfg = RslRlSymmetryCfg(use_data_augmentation=True, use_mirror_loss=True,
                                                mirror_loss_coeff=0.3, data_augmentation_func=func)
    env = RslRlVecEnvWrapper(ToySymEnv(ToyEnvCfg(scene=type(ToyEnvCfg().scene)(num_envs=16))))
    d = c.to_dict()
    if callable(func):  # class_to_dict names a callable "module:func", as IsaacLab's does; hand the object itself over
        assert d["algorithm"]["symmetry_cfg"]["data_augmentation_func"].endswith(":toy_augment")
        d["algorithm"]["symmetry_cfg"]["data_augmentation_func"] = func
    runner = OnPolicyRunner(env, d, log_dir=str(tmp_path), device="cpu")
    sym = runner.alg.symmetry
    assert sym["use_data_augmentation"] and sym["use_mirror_loss"] and sym["mirror_loss_coeff"] == 0.3
    assert sym["data_augmentation_func"] is (S.augment if isinstance(func, str) else func) and sym["_env"] is env
    runner.learn(2)
    lines = [json.loads(x) for x in (tmp_path / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2 and all(math.isfinite(x["Loss/symmetry"]) and x["Loss/symmetry"] > 0 for x in lines)
    plain = OnPolicyRunner(env, RslRlOnPolicyRunnerCfg(device="cpu").to_dict(), log_dir=None, device="cpu")
    assert plain.alg.symmetry is None


PRELUDE = r"""
import sys
sys.path[:0] = [{shims!r}, {pkg!r}, {helpers!r}, {scripts!r}]
import gymnasium as gym
from isaaclab_rl.rsl_rl import RslRlOnPolicyRunnerCfg
def toy_agent():
    c = RslRlOnPolicyRunnerCfg(device="cpu", num_steps_per_env=8, max_iterations=3, save_interval=1,
                               experiment_name="toy_sym")
    c.policy.actor_hidden_dims = [16]
    c.policy.critic_hidden_dims = [16]
    return c
gym.register(id="Toy-Sym-v0", entry_point="toy_sym:ToySymEnv",
             kwargs={{"env_cfg_entry_point": "toy_sym:ToyEnvCfg", "rsl_rl_cfg_entry_point": toy_agent}})
import train
sys.exit(train.main(sys.argv[1:]))
"""
OVERRIDE = ("agent.algorithm.symmetry_cfg={use_data_augmentation: true, use_mirror_loss: false, "
            "mirror_loss_coeff: 0.0, data_augmentation_func: 'h12env.symmetry:augment'}")


@pytest.mark.parametrize("extra", [("--symmetry", "both", "--mirror_loss_coeff", "0.25"), (OVERRIDE,)],
                         ids=["flag", "hydra"])
def test_train_script_with_symmetry(tmp_path, extra):
    train = ROOT / "h1v2-isaac_amd" / "scripts" / "train.py"
    prelude = PRELUDE.format(shims=str(ROOT / "h1v2-isaac_amd" / "shims"), pkg=str(ROOT / "h1v2-isaac_amd"),
                             helpers=str(ROOT / "tests" / "helpers"), scripts=str(train.parent))
    cmd = [sys.executable, "-c", prelude, "--task", "Toy-Sym-v0", "--headless", "--device", "cpu", "--num_envs", "16",
           "--seed", "3", "--max_iterations", "2", "env.episode_length=20", *extra]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Loss/symmetry" in r.stdout
    run_dir = next((tmp_path / "logs" / "rsl_rl" / "toy_sym").iterdir())
    lines = [json.loads(x) for x in (run_dir / "metrics.jsonl").read_text().splitlines()]
    assert [x["iter"] for x in lines] == [0, 1]
    assert all(math.isfinite(x["Loss/symmetry"]) for x in lines)
    agent = (run_dir / "params" / "agent.yaml").read_text()
    assert "h12env.symmetry:augment" in agent
    if extra[0] == "--symmetry":
        assert "mirror_loss_coeff: 0.25" in agent and "use_mirror_loss: true" in agent


def test_agent_cfg_defaults_stay_none():
    import biped_tasks.tasks  # noqa: F401
    import isaaclab_rl.rsl_rl as R
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    assert "RslRlSymmetryCfg" in R.__all__
    f = {x.name for x in __import__("dataclasses").fields(R.RslRlSymmetryCfg)}
    assert f == {"use_data_augmentation", "use_mirror_loss", "mirror_loss_coeff", "data_augmentation_func"}
    for task in ("Isaac-Velocity-Flat-H12_12dof-v0", "Isaac-Velocity-Rough-H12_12dof-v0",
                 "Isaac-Velocity-Rsl-H12_12dof-v0"):
        assert load_cfg_from_registry(task, "rsl_rl_cfg_entry_point").algorithm.symmetry_cfg is None


# ---------------------------------------------------------------------------------------------- 7. ABI
def test_mirror_rows_validates_before_any_hip_call():
    from h12env._learn import LEARN_SYMBOLS, learn_library

    assert "h12learn_mirror_rows" in LEARN_SYMBOLS
    lib = learn_library()
    assert "h12learn_mirror_rows" in (ROOT / "include" / "h12learn.h").read_text()
    buf = (C.c_float * 16)()
    tab = (C.c_int * 4)(0, 1, 2, 3)
    p, t = C.addressof(buf), C.addressof(tab)
    f = lib.h12learn_mirror_rows
    cases = [((p, 4, None, 2, 0, t, 0, p, None), b"d = 0"), ((p, 4, None, -1, 4, t, 0, p, None), b"n = -1"),
             ((None, 4, None, 2, 4, t, 0, p, None), b"x is null"), ((p, 4, None, 2, 4, None, 0, p, None), b"table is null"),
             ((p, 4, None, 2, 4, t, 0, None, None), b"out is null"), ((p, 0, None, 2, 4, t, 0, p, None), b"n_src_rows = 0"),
             ((p, 4, None, 5, 4, t, 0, p, None), b"without idx")]
    for args, msg in cases:
        assert f(*args) == -1, msg
        assert msg in lib.h12learn_last_error(), (msg, lib.h12learn_last_error())
    assert f(p, 4, None, 0, 4, t, 1, p, None) == 0  # nothing to do: no launch
