"""CPU: the recurrent actor-critic of the PPO runner (h12env.recurrent, h12env.ppo.ActorCriticRecurrent, the recurrent
branch of RolloutStorage / PPO / OnPolicyRunner, the recurrent export and h12env.policy.RecurrentPolicy)."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "shims"))
sys.path.insert(0, str(ROOT / "tests" / "helpers"))

from h12env.ppo import PPO, ActorCritic, ActorCriticRecurrent, OnPolicyRunner  # noqa: E402
from h12env.recurrent import Memory, split_and_pad_trajectories, unpad_trajectories  # noqa: E402
from isaaclab_rl.rsl_rl import (RslRlOnPolicyRunnerCfg, RslRlPpoActorCriticRecurrentCfg,  # noqa: E402
                                RslRlVecEnvWrapper)
from toyenv import ToyEnv  # noqa: E402


# ---------------------------------------------------------------------------------------------- 1: split / pad
def test_split_and_pad_on_planted_dones_equals_literals_and_round_trips():
    T, N = 5, 3
    x = (10.0 * torch.arange(N)[None, :, None] + torch.arange(T)[:, None, None]
         + torch.tensor([0.0, 100.0])[None, None, :])  # x[t, e] = (10 e + t, 10 e + t + 100)
    dones = torch.zeros(T, N, 1)
    dones[0, 1] = dones[3, 1] = dones[4, 2] = 1  # env 0: none; env 1: t = 0 and t = 3; env 2: t = 4
    padded, masks = split_and_pad_trajectories(x, dones)
    # 1 + 3 + 1 trajectories, env-major; first feature, zero-padded to T
    first = torch.tensor([[0., 10., 11., 14., 20.],
                          [1., 0., 12., 0., 21.],
                          [2., 0., 13., 0., 22.],
                          [3., 0., 0., 0., 23.],
                          [4., 0., 0., 0., 24.]])
    want_masks = torch.tensor([[1, 1, 1, 1, 1],
                               [1, 0, 1, 0, 1],
                               [1, 0, 1, 0, 1],
                               [1, 0, 0, 0, 1],
                               [1, 0, 0, 0, 1]], dtype=torch.bool)
    assert padded.shape == (T, 5, 2) and masks.shape == (T, 5)
    assert torch.equal(masks, want_masks)
    assert torch.equal(padded[..., 0], first)
    assert torch.equal(padded[..., 1], torch.where(want_masks, first + 100.0, torch.zeros(())))
    assert torch.equal(unpad_trajectories(padded, masks), x)


def test_memory_modes():
    torch.manual_seed(0)
    m = Memory(4, type="lstm", hidden_size=6)
    assert m.hidden_states is None
    out = m(torch.randn(3, 4))
    assert out.shape == (1, 3, 6) and m.hidden_states[0].shape == (1, 3, 6)
    m.reset(torch.tensor([0, 1, 0]))
    assert all((s[:, 1] == 0).all() and (s[:, 0] != 0).any() for s in m.hidden_states)
    with pytest.raises(ValueError, match="Hidden states"):
        m(torch.randn(5, 2, 4), masks=torch.ones(5, 2, dtype=torch.bool))
    m.reset()
    assert m.hidden_states is None
    g = Memory(4, type="gru", hidden_size=6)
    g(torch.randn(3, 4))
    g.reset(torch.tensor([1, 0, 0]))
    assert (g.hidden_states[:, 0] == 0).all() and (g.hidden_states[:, 1] != 0).any()


# ---------------------------------------------------------------------------------------------- 2: update == collection
def planted_rollout(priv: bool):
    """T = 6, N = 8 through PPO.act / process_env_step, with consecutive dones, a done at T - 1 and one at t = 0."""
    torch.manual_seed(11)
    T, N, d, dc, A = 6, 8, 5, 7 if priv else 5, 3
    policy = ActorCriticRecurrent(d, dc, A, actor_hidden_dims=(12,), critic_hidden_dims=(10,), rnn_hidden_dim=9)
    alg = PPO(policy, num_learning_epochs=1, num_mini_batches=2, device="cpu", schedule="fixed")
    alg.init_storage(N, T, [d], [dc] if priv else None, [A])
    dones = torch.zeros(T, N)
    dones[1, 2] = dones[2, 2] = 1  # consecutive
    dones[T - 1, 3] = 1
    dones[0, 5] = dones[3, 5] = dones[4, 5] = 1
    dones[2, 7] = 1
    obs = torch.randn(T + 1, N, d)
    cobs = torch.randn(T + 1, N, dc) if priv else obs
    # a step of a previous iteration, so the t = 0 states are not zero
    with torch.no_grad():
        policy.act(torch.randn(N, d)), policy.evaluate(torch.randn(N, dc))
        for t in range(T):
            alg.act(obs[t], cobs[t] if priv else obs[t])
            alg.process_env_step(torch.randn(N), dones[t], {})
        alg.compute_returns(cobs[T])
    return alg, dones


@pytest.mark.parametrize("priv", [False, True])
def test_the_update_sees_what_the_collection_saw(priv):
    alg, dones = planted_rollout(priv)
    st, policy = alg.storage, alg.policy
    T, N = st.num_steps, st.num_envs
    seen = 0
    with torch.no_grad():
        for i, rec in enumerate(st.recurrent_mini_batch_generator(2, 1, (policy.memory_a, policy.memory_c))):
            e = slice(i * N // 2, (i + 1) * N // 2)
            n_traj = int(dones[:-1, e].sum()) + N // 2
            assert rec["masks"].shape == (T, n_traj) and rec["observations"].shape[:2] == (T, n_traj)
            assert rec["hidden_a"][0].shape == (1, n_traj, 9)
            policy.act(rec["observations"], masks=rec["masks"], hidden_states=rec["hidden_a"])
            value = policy.evaluate(rec["critic_observations"], masks=rec["masks"], hidden_states=rec["hidden_c"])
            log_prob = policy.get_actions_log_prob(rec["actions"])
            for got, want in ((policy.action_mean, st.mu[:, e]), (log_prob, st.actions_log_prob[:, e, 0]),
                              (value, st.values[:, e])):
                assert got.shape == want.shape
                err = (got - want).abs().max().item()
                print(f"minibatch {i}: max |batch mode - collection| = {err:.3e}")
                assert err <= 1e-6
            for k in ("returns", "advantages", "sigma"):
                assert torch.equal(rec[k], st.t[k][:, e])
            seen += 1
    assert seen == 2


def test_recurrent_update_runs_on_the_planted_rollout():
    alg, _ = planted_rollout(False)
    before = [p.detach().clone() for p in alg.policy.parameters()]
    out = alg.update()
    assert all(torch.isfinite(torch.tensor(v)) for v in out.values())
    assert any(not torch.equal(a, b) for a, b in zip(before, alg.policy.parameters()))
    assert alg.storage.step == 0


# ---------------------------------------------------------------------------------------------- 3: runner
def recurrent_cfg(**kw):
    c = RslRlOnPolicyRunnerCfg(device="cpu", num_steps_per_env=8, save_interval=1000, experiment_name="toy", **kw)
    c.policy = RslRlPpoActorCriticRecurrentCfg(actor_hidden_dims=[16, 16], critic_hidden_dims=[16], rnn_hidden_dim=12)
    c.algorithm.num_learning_epochs = 2
    return c


KEYS = ({f"memory_{m}.rnn.{p}_l0" for m in "ac" for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
        | {f"actor.{k}.{p}" for k in (0, 2, 4) for p in ("weight", "bias")}
        | {f"critic.{k}.{p}" for k in (0, 2) for p in ("weight", "bias")} | {"std"})


def test_runner_builds_trains_saves_and_loads_the_recurrent_class(tmp_path):
    cfg = recurrent_cfg().to_dict()
    assert cfg["policy"]["class_name"] == "ActorCriticRecurrent" and cfg["policy"]["rnn_type"] == "lstm"
    runner = OnPolicyRunner(RslRlVecEnvWrapper(ToyEnv()), cfg, log_dir=None, device="cpu")
    policy = runner.alg.policy
    assert isinstance(policy, ActorCriticRecurrent) and policy.is_recurrent
    assert set(policy.state_dict()) == KEYS
    before = {k: v.clone() for k, v in policy.state_dict().items()}
    runner.learn(2)
    stats = runner.last_iteration_stats
    assert all(torch.isfinite(torch.tensor(float(stats[k]))) for k in ("Loss/value_function", "Loss/surrogate"))
    after = policy.state_dict()
    for k in ("memory_a.rnn.weight_hh_l0", "memory_c.rnn.weight_ih_l0", "actor.0.weight", "critic.2.bias"):
        assert not torch.equal(before[k], after[k]), k
    path = str(tmp_path / "model.pt")
    runner.save(path)
    fresh = OnPolicyRunner(RslRlVecEnvWrapper(ToyEnv()), cfg, log_dir=None, device="cpu")
    fresh.load(path)
    obs = torch.randn(5, 64, 6)
    with torch.no_grad():
        a, b = runner.get_inference_policy(), fresh.get_inference_policy()
        seq_a, seq_b = [a(o) for o in obs], [b(o) for o in obs]
    assert all(torch.equal(x, y) for x, y in zip(seq_a, seq_b))
    assert not torch.equal(seq_a[0], a(obs[0]))  # stateful: the same observation later gives another action

    # an absent / feed-forward class_name is today's class; its checkpoint does not load into the recurrent runner
    ff = RslRlOnPolicyRunnerCfg(device="cpu", num_steps_per_env=8, save_interval=1000, experiment_name="toy").to_dict()
    ff["policy"]["actor_hidden_dims"] = ff["policy"]["critic_hidden_dims"] = [16]
    ff_runner = OnPolicyRunner(RslRlVecEnvWrapper(ToyEnv()), ff, log_dir=None, device="cpu")
    assert type(ff_runner.alg.policy) is ActorCritic
    del ff["policy"]["class_name"]
    assert type(OnPolicyRunner(RslRlVecEnvWrapper(ToyEnv()), ff, log_dir=None, device="cpu").alg.policy) is ActorCritic
    ff_path = str(tmp_path / "ff.pt")
    ff_runner.save(ff_path)
    with pytest.raises(RuntimeError, match="load_state_dict|state_dict"):
        fresh.load(ff_path)
    bad = dict(cfg, policy=dict(cfg["policy"], class_name="ActorCriticTransformer"))
    with pytest.raises(ValueError, match="class_name"):
        OnPolicyRunner(RslRlVecEnvWrapper(ToyEnv()), bad, log_dir=None, device="cpu")


def test_runner_trains_the_recurrent_class_with_empirical_normalization(tmp_path):
    cfg = recurrent_cfg(empirical_normalization=True).to_dict()
    runner = OnPolicyRunner(RslRlVecEnvWrapper(ToyEnv()), cfg, log_dir=None, device="cpu")
    norm = runner.obs_normalizer
    assert runner.empirical_normalization and int(norm.count) == 0 and (norm._std == 1).all()
    before = {k: v.clone() for k, v in runner.alg.policy.state_dict().items()}
    runner.learn(2)
    stats = runner.last_iteration_stats
    assert all(torch.isfinite(torch.tensor(float(stats[k]))) for k in ("Loss/value_function", "Loss/surrogate"))
    assert int(norm.count) > 0 and int(runner.critic_obs_normalizer.count) > 0
    assert not (norm._std == 1).all() and torch.equal(norm._std, torch.sqrt(norm._var))
    after = runner.alg.policy.state_dict()
    for k in ("memory_a.rnn.weight_ih_l0", "memory_c.rnn.weight_hh_l0", "actor.0.weight", "critic.2.bias"):
        assert not torch.equal(before[k], after[k]), k
    # the deployed policy reads the statistics and leaves them alone; a fresh runner gets them from the checkpoint
    count, std = int(norm.count), norm._std.clone()
    path = str(tmp_path / "model.pt")
    runner.save(path)
    fresh = OnPolicyRunner(RslRlVecEnvWrapper(ToyEnv()), cfg, log_dir=None, device="cpu")
    fresh.load(path)
    obs = torch.randn(3, 64, 6)
    with torch.no_grad():
        a, b = runner.get_inference_policy(), fresh.get_inference_policy()
        assert all(torch.equal(a(o), b(o)) for o in obs)
    assert int(norm.count) == count == int(fresh.obs_normalizer.count) and torch.equal(norm._std, std)
    assert torch.equal(fresh.obs_normalizer._std, std)


def test_recurrent_policy_reads_a_running_mean_std_without_updating_it():
    from h12env.cleanrl import RunningMeanStd
    from h12env.policy import RecurrentPolicy

    torch.manual_seed(2)
    pol = ActorCriticRecurrent(6, 6, 3, actor_hidden_dims=(8,), critic_hidden_dims=(8,), rnn_hidden_dim=8)
    norm = RunningMeanStd(shape=(6,))
    norm.running_mean.copy_(torch.randn(6)), norm.running_var.copy_(torch.rand(6) + 0.5)
    kept = {k: v.clone() for k, v in norm.state_dict().items()}
    p = RecurrentPolicy(pol.memory_a.rnn, pol.actor, norm)
    x = torch.randn(4, 6) * 3
    with torch.no_grad():
        y = p(x)
        out, _ = pol.memory_a.rnn(((x - kept["running_mean"]) / torch.sqrt(kept["running_var"] + norm.epsilon))[None])
        assert torch.equal(y, pol.actor(out[0]))
    assert all(torch.equal(v, kept[k]) for k, v in norm.state_dict().items())


def test_older_spelling_and_gru():
    p = ActorCriticRecurrent(6, 6, 3, rnn_hidden_size=20, rnn_type="gru", rnn_num_layers=2)
    assert p.memory_a.rnn.hidden_size == 20 and isinstance(p.memory_c.rnn, torch.nn.GRU)
    assert p.actor[0].in_features == 20 and p.critic[0].in_features == 20
    with torch.no_grad():
        assert p.act_inference(torch.randn(4, 6)).shape == (4, 3)
    ha, hc = p.get_hidden_states()
    assert ha.shape == (2, 4, 20) and hc is None


# ---------------------------------------------------------------------------------------------- 4: refused switches
@pytest.mark.parametrize("switch,kw", [
    ("fused_learner", {"fused_learner": True}),
    ("fused_loss", {"fused_loss": True}),
    ("symmetry_cfg", {"symmetry_cfg": {"use_data_augmentation": True, "data_augmentation_func": "h12env.symmetry:augment"}}),
    ("shard.world > 1", {"shard": "two"}),
])
def test_switches_refused_with_a_recurrent_policy(switch, kw):
    from h12env import distributed as D

    if kw.get("shard") == "two":
        kw = {"shard": D.Shard(0, 2, 0, 0)}
    policy = ActorCriticRecurrent(6, 6, 3, actor_hidden_dims=(8,), critic_hidden_dims=(8,), rnn_hidden_dim=8)
    with pytest.raises(ValueError) as e:
        PPO(policy, device="cpu", **kw)
    assert switch in str(e.value) and "recurrent" in str(e.value)


# ---------------------------------------------------------------------------------------------- 5: export
def test_recurrent_export_and_batched_recurrent_policy(tmp_path):
    from h12env.export import export_policy_as_jit, export_policy_as_onnx
    from h12env.policy import RecurrentPolicy, deploy_policy
    from h12env.ppo import EmpiricalNormalization

    torch.manual_seed(4)
    policy = ActorCriticRecurrent(10, 10, 4, actor_hidden_dims=(24, 16), critic_hidden_dims=(8,), rnn_hidden_dim=14)
    norm = EmpiricalNormalization([10]).train()
    norm(torch.randn(64, 10) * 3 + 1)
    norm.eval()
    path = export_policy_as_jit(policy, norm, str(tmp_path))
    m = torch.jit.load(path)
    assert m.hidden_state.shape == (1, 1, 14) and m.cell_state.shape == (1, 1, 14) and hasattr(m, "rnn")
    obs = torch.randn(5, 1, 10) * 3 + 1
    with torch.no_grad():
        want = [policy.act_inference(norm(o)) for o in obs]
        got = [m(o) for o in obs]
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        assert not torch.equal(m(obs[0]), got[0])
        m.reset()
        assert torch.equal(m(obs[0]), got[0])
    with pytest.raises(NotImplementedError, match="recurrent"):
        export_policy_as_onnx(policy, norm, str(tmp_path))

    # four robots on one RecurrentPolicy == four independent copies of the export
    batch = torch.randn(6, 4, 10) * 3 + 1
    p = RecurrentPolicy.from_exported(m, 4)
    assert isinstance(deploy_policy(m, 4, "cpu"), RecurrentPolicy)
    copies = [torch.jit.load(path) for _ in range(4)]
    with torch.no_grad():
        for t, x in enumerate(batch):
            if t == 3:  # robot 2 starts a new episode
                p.reset(torch.tensor([0, 0, 1, 0]))
                copies[2] = torch.jit.load(path)
            y = p(x)
            ref = torch.cat([c(x[i:i + 1]) for i, c in enumerate(copies)])
            assert y.shape == (4, 4) and torch.allclose(y, ref, rtol=0, atol=1e-6), t

    gru = ActorCriticRecurrent(10, 10, 4, rnn_type="gru", rnn_hidden_dim=8)
    with pytest.raises(ValueError, match="LSTM only"):
        RecurrentPolicy(gru.memory_a.rnn, gru.actor, fused=True)
    two = ActorCriticRecurrent(10, 10, 4, rnn_num_layers=2, rnn_hidden_dim=8)
    with pytest.raises(ValueError, match="num_layers = 2"):
        RecurrentPolicy(two.memory_a.rnn, two.actor, fused=True)
    wide = ActorCriticRecurrent(10, 10, 4, rnn_hidden_dim=257)
    with pytest.raises(ValueError, match="hidden size 257"):
        RecurrentPolicy(wide.memory_a.rnn, wide.actor, fused=True)
    with torch.no_grad():  # all three run on the torch path
        for pol in (gru, two, wide):
            assert RecurrentPolicy(pol.memory_a.rnn, pol.actor)(torch.randn(3, 10)).shape == (3, 4)
