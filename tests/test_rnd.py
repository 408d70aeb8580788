"""Random Network Distillation (h12env.rnd, rsl_rl's rnd_cfg) on the CPU: the reward path against an fp64 restatement
written here from the formulas of DESIGN.md section 7t, the weight schedules, PPO's use of it on a toy env, the
checkpoint, the refusals, and that a run without rnd_cfg has none of it."""
import copy
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "shims"))
sys.path.insert(0, str(ROOT / "tests" / "helpers"))

from h12env import distributed as D  # noqa: E402
from h12env.ppo import PPO, ActorCritic, ActorCriticRecurrent, OnPolicyRunner  # noqa: E402
from h12env.rnd import (EmpiricalDiscountedVariationNormalization, RandomNetworkDistillation,  # noqa: E402
                        resolve_rnd_cfg, scheduled_weight)
from isaaclab_rl.rsl_rl import (RslRlOnPolicyRunnerCfg, RslRlPpoActorCriticCfg, RslRlPpoAlgorithmCfg,  # noqa: E402
                                RslRlRndCfg, RslRlVecEnvWrapper)
from toyenv import ToyEnv, ToyEnvCfg  # noqa: E402

STEP_DT = 0.02


class RndToyEnv(ToyEnv):
    """ToyEnv that also serves the observation group ``rnd_state`` (position and distance to the target: 4 floats)."""

    step_dt = STEP_DT

    def __init__(self, *a, serve_rnd_state=True, **kw):
        self._serve = serve_rnd_state
        super().__init__(*a, **kw)
        self.observation_manager.compute = self._obs

    def _obs(self):
        out = super()._obs()
        if self._serve:
            out["rnd_state"] = torch.cat([self.x, (self.target - self.x).norm(dim=1, keepdim=True)], dim=1)
        return out


def make_env(n=8, episode_length=50, serve=True):
    cfg = ToyEnvCfg()
    cfg.scene.num_envs = n
    cfg.episode_length = episode_length
    return RslRlVecEnvWrapper(RndToyEnv(cfg, serve_rnd_state=serve))


def train_cfg(rnd_cfg, seed=3, **algorithm):
    c = RslRlOnPolicyRunnerCfg(seed=seed, device="cpu", num_steps_per_env=4, max_iterations=2, save_interval=100,
                               policy=RslRlPpoActorCriticCfg(actor_hidden_dims=[8], critic_hidden_dims=[8]),
                               algorithm=RslRlPpoAlgorithmCfg(num_learning_epochs=2, num_mini_batches=2, rnd_cfg=rnd_cfg,
                                                              **algorithm))
    return c.to_dict()


RND = dict(weight=2.0, state_normalization=True, reward_normalization=True, learning_rate=1e-2, num_outputs=3,
           predictor_hidden_dims=[-1], target_hidden_dims=[6])


# ---------------------------------------------------------------------------------------------- 1: fp64 restatement
def np_net(seq, x):
    """An nn.Sequential of Linear / ELU in numpy fp64 on the module's fp32 weights."""
    for m in seq:
        if isinstance(m, torch.nn.Linear):
            x = x @ m.weight.detach().double().numpy().T + m.bias.detach().double().numpy()
        else:
            x = np.where(x > 0, x, np.expm1(x))
    return x


class Fp64Rnd:
    """get_intrinsic_reward restated: EmpiricalNormalization([d], eps=1e-2), the networks, the row norm, the discounted
    variation normaliser (gamma 0.99) and the weight."""

    def __init__(self, module, d, normalise):
        self.m, self.normalise = module, normalise
        self.s_mean, self.s_var, self.s_std, self.s_count = np.zeros(d), np.ones(d), np.ones(d), 0
        self.r_mean, self.r_var, self.r_std, self.r_count = 0.0, 1.0, 1.0, 0
        self.avg = None

    @staticmethod
    def fold(mean, var, count, x):
        n = x.shape[0]
        mean_x, var_x = x.mean(axis=0), x.var(axis=0)  # population variance
        count += n
        rate = n / count
        delta = mean_x - mean
        mean = mean + rate * delta
        var = var + rate * (var_x - var + delta * (mean_x - mean))
        return mean, var, np.sqrt(var), count

    def __call__(self, x, weight):
        x = x.double().numpy()
        if self.normalise:
            self.s_mean, self.s_var, self.s_std, self.s_count = self.fold(self.s_mean, self.s_var, self.s_count, x)
            x = (x - self.s_mean) / (self.s_std + 1e-2)
        e = np.sqrt(((np_net(self.m.target, x) - np_net(self.m.predictor, x)) ** 2).sum(axis=1))
        if self.normalise:
            self.avg = e.copy() if self.avg is None else self.avg * 0.99 + e
            self.r_mean, self.r_var, self.r_std, self.r_count = self.fold(self.r_mean, self.r_var, self.r_count, self.avg)
            e = e / self.r_std if self.r_std > 0 else e
        return e * weight, x


@pytest.mark.parametrize("normalise", [True, False])
def test_reward_path_against_fp64_restatement(normalise):
    torch.manual_seed(11)
    m = RandomNetworkDistillation(5, num_outputs=3, predictor_hidden_dims=[8], target_hidden_dims=[8], weight=0.7,
                                  state_normalization=normalise, reward_normalization=normalise).train()
    ref = Fp64Rnd(m, 5, normalise)
    g = torch.Generator().manual_seed(5)
    for call in range(5):
        x = torch.randn(7, 5, generator=g) * 2.0 + 0.5
        got, s = m.get_intrinsic_reward(x)
        want, s_ref = ref(x, 0.7)
        assert m.update_counter == call + 1
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-5)
        np.testing.assert_allclose(s.numpy(), s_ref, rtol=1e-5, atol=1e-6)
        if normalise:
            sn, rn = m.state_normalizer, m.reward_normalizer
            for have, exp in ((sn._mean[0], ref.s_mean), (sn._var[0], ref.s_var), (sn._std[0], ref.s_std),
                              (rn._mean, ref.r_mean), (rn._var, ref.r_var), (rn._std, ref.r_std), (rn.avg, ref.avg)):
                np.testing.assert_allclose(have.numpy(), exp, rtol=1e-5, atol=1e-7)
            assert int(sn.count) == ref.s_count and int(rn.count) == ref.r_count == 7 * (call + 1)
    assert not any(p.requires_grad for p in m.target.parameters()) and not m.target.training


def test_reward_normaliser_zero_std_and_until():
    """std == 0 passes x through (chosen on the device); statistics freeze once count >= until."""
    n = EmpiricalDiscountedVariationNormalization([], until=6).train()
    x = torch.full((4,), 2.0)
    # an all-equal first batch: rate = n / count = 1, so the running variance becomes the batch's, 0
    assert torch.equal(n(x), x) and float(n._std) == 0.0 and float(n._mean) == 2.0
    n = EmpiricalDiscountedVariationNormalization([], until=6).train()
    n(torch.tensor([1.0, 2.0, 3.0, 4.0]))
    n(torch.tensor([2.0, 1.0, 0.0, 5.0]))
    frozen = {k: v.clone() for k, v in n.state_dict().items() if k != "avg"}
    assert int(n.count) == 8
    n(torch.tensor([9.0, 9.0, 1.0, 1.0]))
    for k, v in frozen.items():
        if k != "first":
            assert torch.equal(n.state_dict()[k], v), k


# ---------------------------------------------------------------------------------------------- 2: schedules
def test_weight_schedules_at_the_boundaries():
    w0 = 0.5
    assert scheduled_weight(w0, None, 10 ** 6) == w0 and scheduled_weight(w0, {"mode": "constant"}, 7) == w0
    step = {"mode": "step", "final_step": 10, "final_value": 0.1}
    assert [scheduled_weight(w0, step, s) for s in (9, 10, 11)] == [w0, 0.1, 0.1]
    lin = {"mode": "linear", "initial_step": 10, "final_step": 20, "final_value": 0.1}
    got = [scheduled_weight(w0, lin, s) for s in (9, 10, 15, 20, 21)]
    assert got[0] == w0 and got[1] == w0 and got[3] == 0.1 and got[4] == 0.1
    assert got[2] == pytest.approx(0.3, rel=1e-12)
    m = RandomNetworkDistillation(3, weight=w0, weight_schedule=lin)
    m.update_counter = 15
    assert m.weight == pytest.approx(0.3, rel=1e-12)


def test_runner_scales_the_weight_by_step_dt_once_and_not_the_schedule():
    sched = {"mode": "step", "final_step": 3, "final_value": 0.25}
    r = OnPolicyRunner(make_env(), train_cfg({**RND, "weight_schedule": sched}), device="cpu")
    rnd = r.alg.rnd
    assert rnd.initial_weight == 2.0 * STEP_DT and rnd.num_states == 4
    assert rnd.predictor[0].out_features == 4 and rnd.target[0].out_features == 6  # -1 is num_states
    rnd.update_counter = 3
    assert rnd.weight == 0.25  # taken as given


# ---------------------------------------------------------------------------------------------- 3: PPO on CPU
def net(seq, x):
    for m in seq:
        x = F.linear(x, m.weight, m.bias) if isinstance(m, torch.nn.Linear) else F.elu(x)
    return x


def test_ppo_collects_and_trains_with_rnd(tmp_path):
    env = make_env(n=8, episode_length=3)
    r = OnPolicyRunner(env, train_cfg({**RND, "reward_normalization": False}), log_dir=str(tmp_path), device="cpu")
    alg, rnd = r.alg, r.alg.rnd
    assert alg.storage.t["rnd_state"].shape == (4, 8, 4)
    target0 = copy.deepcopy(rnd.target.state_dict())
    predictor0 = copy.deepcopy(rnd.predictor.state_dict())
    w = 2.0 * STEP_DT
    obs, extras = env.get_observations()
    r.train_mode()
    saw_time_out = False
    with torch.inference_mode():
        for t in range(4):
            actions = alg.act(obs, obs)
            obs, rewards, dones, infos = env.step(actions)
            # the test's own fp32 recomputation, from the state the modules have before the step
            norm = copy.deepcopy(rnd.state_normalizer)
            state = infos["observations"]["rnd_state"]
            s = norm(state)
            e = torch.linalg.norm(net(rnd.target, s) - net(rnd.predictor, s), dim=1)
            want = rewards.clone().float()
            want += e * w
            want += alg.gamma * (alg._values.squeeze(1) * infos["time_outs"].float())
            saw_time_out |= bool(infos["time_outs"].any())
            alg.process_env_step(rewards, dones, infos)
            assert torch.equal(alg.storage.t["rnd_state"][t], s)
            assert torch.equal(alg.storage.t["rewards"][t, :, 0], want)
            assert torch.equal(alg.intrinsic_rewards, e * w)
        alg.compute_returns(obs)
    assert saw_time_out and rnd.update_counter == 4
    loss = alg.update()
    assert math.isfinite(loss["rnd"]) and loss["rnd"] > 0
    for k, v in rnd.target.state_dict().items():
        assert torch.equal(v, target0[k]), k
    assert any(not torch.equal(v, predictor0[k]) for k, v in rnd.predictor.state_dict().items())
    r.learn(1)  # the second iteration, through the runner: the log keys
    stats = r.last_iteration_stats
    assert math.isfinite(stats["Loss/rnd"]) and stats["Rnd/weight"] == w
    assert math.isfinite(stats["Rnd/mean_extrinsic_reward"]) and stats["Rnd/mean_intrinsic_reward"] > 0
    assert stats["Train/mean_reward"] == pytest.approx(stats["Rnd/mean_extrinsic_reward"]
                                                       + stats["Rnd/mean_intrinsic_reward"], rel=1e-5)
    for k, v in rnd.target.state_dict().items():
        assert torch.equal(v, target0[k]), k


# ---------------------------------------------------------------------------------------------- 4: learning
def test_predictor_learns_a_fixed_batch():
    torch.manual_seed(2)
    policy = ActorCritic(6, 6, 3, actor_hidden_dims=(8,), critic_hidden_dims=(8,))
    alg = PPO(policy, device="cpu", rnd_cfg={"num_states": 5, "num_outputs": 4, "learning_rate": 1e-2,
                                             "predictor_hidden_dims": [16], "target_hidden_dims": [16]})
    x = torch.randn(64, 5)
    losses = []
    for _ in range(50):
        loss = F.mse_loss(alg.rnd.predictor(x), alg.rnd.target(x).detach())
        alg.rnd_optimizer.zero_grad()
        loss.backward()
        alg.rnd_optimizer.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0]


# ---------------------------------------------------------------------------------------------- 5: checkpoint
def test_checkpoint_round_trip(tmp_path):
    a = OnPolicyRunner(make_env(episode_length=3), train_cfg(RND, seed=3), log_dir=str(tmp_path / "a"), device="cpu")
    a.learn(2)
    path = str(tmp_path / "a" / "model_2.pt")
    d = torch.load(path, weights_only=True)
    assert "rnd_state_dict" in d and "rnd_optimizer_state_dict" in d
    b = OnPolicyRunner(make_env(episode_length=3), train_cfg(RND, seed=99), device="cpu")
    assert not torch.equal(a.alg.rnd.target[0].weight, b.alg.rnd.target[0].weight)
    b.load(path)
    sa, sb = a.alg.rnd.state_dict(), b.alg.rnd.state_dict()
    assert set(sa) == set(sb) and {"reward_normalizer.avg", "reward_normalizer.count", "state_normalizer.count",
                                    "reward_normalizer._std", "state_normalizer._mean"} <= set(sa)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert b.alg.rnd.update_counter == a.alg.rnd.update_counter == 8
    oa, ob = a.alg.rnd_optimizer.state_dict()["state"], b.alg.rnd_optimizer.state_dict()["state"]
    assert oa.keys() == ob.keys() and len(oa) > 0
    for i in oa:
        for k in oa[i]:
            assert torch.equal(torch.as_tensor(oa[i][k]), torch.as_tensor(ob[i][k])), (i, k)
    b.learn(1)  # and it goes on training


# ---------------------------------------------------------------------------------------------- 6: refusals
def test_checkpoint_without_rnd_is_refused_by_an_rnd_run(tmp_path):
    plain = OnPolicyRunner(make_env(), train_cfg(None), log_dir=str(tmp_path), device="cpu")
    plain.learn(1)
    with pytest.raises(ValueError, match="rnd_state_dict"):
        OnPolicyRunner(make_env(), train_cfg(RND), device="cpu").load(str(tmp_path / "model_1.pt"))
    # the other way round: a plain run reads an RND checkpoint's policy and ignores the rest
    rnd_run = OnPolicyRunner(make_env(), train_cfg(RND), log_dir=str(tmp_path / "r"), device="cpu")
    rnd_run.learn(1)
    plain.load(str(tmp_path / "r" / "model_1.pt"))


def test_missing_rnd_state_group_is_refused():
    with pytest.raises(ValueError, match="rnd_state"):
        OnPolicyRunner(make_env(serve=False), train_cfg(RND), device="cpu")


def small_policy(recurrent=False):
    if recurrent:
        return ActorCriticRecurrent(6, 6, 3, actor_hidden_dims=(8,), critic_hidden_dims=(8,), rnn_hidden_dim=8)
    return ActorCritic(6, 6, 3, actor_hidden_dims=(8,), critic_hidden_dims=(8,))


@pytest.mark.parametrize("what,kw,recurrent", [
    ("a recurrent policy", {}, True),
    ("symmetry_cfg data augmentation",
     {"symmetry_cfg": {"use_data_augmentation": True, "data_augmentation_func": "h12env.symmetry:augment"}}, False),
    ("more than one rank", {"shard": D.Shard(0, 2, 0, 0)}, False),
    ("precision='bf16'", {"precision": "bf16"}, False),
])
def test_refused_combinations(what, kw, recurrent):
    with pytest.raises(ValueError) as e:
        PPO(small_policy(recurrent), device="cpu", rnd_cfg={"num_states": 4}, **kw)
    assert "rnd_cfg" in str(e.value) and what in str(e.value)


def test_rnd_with_distillation_is_refused():
    from isaaclab_rl.rsl_rl import RslRlDistillationAlgorithmCfg, RslRlDistillationStudentTeacherCfg

    c = RslRlOnPolicyRunnerCfg(seed=1, device="cpu", num_steps_per_env=4, policy=RslRlDistillationStudentTeacherCfg(),
                               algorithm=RslRlDistillationAlgorithmCfg()).to_dict()
    c["algorithm"]["rnd_cfg"] = dict(RND)
    with pytest.raises(ValueError, match="rnd_cfg is not supported with Distillation"):
        OnPolicyRunner(make_env(), c, device="cpu")


@pytest.mark.parametrize("bad", [
    {"wieght": 1.0},
    {"weight_schedule": {"mode": "cosine"}},
    {"weight_schedule": {"mode": "step", "final_step": 3}},
    {"weight_schedule": {"mode": "linear", "initial_step": 5, "final_step": 5, "final_value": 0.0}},
])
def test_unknown_keys_and_schedule_modes_are_refused(bad):
    with pytest.raises(ValueError, match="rnd_cfg"):
        OnPolicyRunner(make_env(), train_cfg({**RND, **bad}), device="cpu")
    with pytest.raises(ValueError, match="rnd_cfg"):
        PPO(small_policy(), device="cpu", rnd_cfg={"num_states": 4, **bad})


def test_fused_rnd_refuses_what_the_kernels_cannot_run():
    from h12env.rnd import FusedRND

    with pytest.raises(ValueError, match="Linear/ELU"):
        FusedRND(RandomNetworkDistillation(4, activation="relu"))


def test_resolve_leaves_the_callers_cfg_alone():
    env = make_env()
    cfg = dict(RND)
    out = resolve_rnd_cfg(cfg, env, env.get_observations()[1]["observations"])
    assert cfg == RND and out["num_states"] == 4 and out["weight"] == 2.0 * STEP_DT


def test_shim_cfg_reaches_the_runner():
    c = train_cfg(RslRlRndCfg(weight=1.5, num_outputs=2))
    assert c["algorithm"]["rnd_cfg"]["weight"] == 1.5
    r = OnPolicyRunner(make_env(), c, device="cpu")
    assert r.alg.rnd.num_outputs == 2 and r.alg.rnd_fused is None


# ---------------------------------------------------------------------------------------------- 7: off means off
def test_off_means_off(tmp_path):
    r = OnPolicyRunner(make_env(episode_length=3), train_cfg(None), log_dir=str(tmp_path), device="cpu")
    assert r.alg.rnd is None and not hasattr(r.alg, "rnd_optimizer")
    assert "rnd_state" not in r.alg.storage.t and r.alg._n_stats == 3
    r.learn(1)
    assert not [k for k in r.last_iteration_stats if "rnd" in k.lower()]
    d = torch.load(str(tmp_path / "model_1.pt"), weights_only=True)
    assert not [k for k in d if "rnd" in k]
