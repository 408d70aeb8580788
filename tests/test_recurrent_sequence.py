"""CPU: the sequence form of the recurrent update (h12env.recurrent.lstm_sequence in its torch-loop form,
RolloutStorage.recurrent_env_mini_batch_generator, PPO(fused_rnn_update=True)).  DESIGN.md section 7r.  The kernels
themselves are tested in tests/test_gpu_recurrent_sequence.py."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "shims"))
sys.path.insert(0, str(ROOT / "tests" / "helpers"))

from h12env import recurrent as R  # noqa: E402
from h12env.ppo import PPO, ActorCritic, ActorCriticRecurrent, OnPolicyRunner  # noqa: E402
from isaaclab_rl.rsl_rl import (RslRlOnPolicyRunnerCfg, RslRlPpoActorCriticRecurrentCfg,  # noqa: E402
                                RslRlVecEnvWrapper)
from lstm_ref import U  # noqa: E402
from lstm_seq_ref import (MISTAKES, library_padded_grads, make_case, planted_dones, seq_grads,  # noqa: E402
                          worst_error)
from toyenv import ToyEnv  # noqa: E402


def batch_mode_dones(T=6, N=8):
    """The planted dones of tests/test_recurrent.py's batch-mode case: consecutive dones, a done at T - 1, a done at
    t = 0, envs without any."""
    dones = torch.zeros(T, N)
    dones[1, 2] = dones[2, 2] = 1
    dones[T - 1, 3] = 1
    dones[0, 5] = dones[3, 5] = dones[4, 5] = 1
    dones[2, 7] = 1
    return dones


def planted_rollout(priv: bool, **ppo_kw):
    """T = 6, N = 8 through PPO.act / process_env_step on those dones, from non-zero t = 0 states."""
    torch.manual_seed(11)
    T, N, d, dc, A = 6, 8, 5, 7 if priv else 5, 3
    policy = ActorCriticRecurrent(d, dc, A, actor_hidden_dims=(12,), critic_hidden_dims=(10,), rnn_hidden_dim=9)
    alg = PPO(policy, num_learning_epochs=1, num_mini_batches=2, device="cpu", schedule="fixed", **ppo_kw)
    alg.init_storage(N, T, [d], [dc] if priv else None, [A])
    dones = batch_mode_dones(T, N)
    obs = torch.randn(T + 1, N, d)
    cobs = torch.randn(T + 1, N, dc) if priv else obs
    with torch.no_grad():
        policy.act(torch.randn(N, d)), policy.evaluate(torch.randn(N, dc))  # a step of a previous iteration
        for t in range(T):
            alg.act(obs[t], cobs[t] if priv else obs[t])
            alg.process_env_step(torch.randn(N), dones[t], {})
        alg.compute_returns(cobs[T])
    return alg, dones


# ---------------------------------------------------------------------------------------------- 1: equivalence
@pytest.mark.parametrize("priv", [False, True])
def test_sequence_form_equals_the_padded_trajectories(priv):
    alg, dones = planted_rollout(priv)
    st, policy = alg.storage, alg.policy
    cobs = st.privileged_observations if priv else st.observations
    for mem, x, start in ((policy.memory_a, st.observations, st.start_states[0]),
                          (policy.memory_c, cobs, st.start_states[1])):
        assert all((s != 0).any() for s in start)
        w = torch.randn(st.num_steps, st.num_envs, 9)
        # the padded form: every env's first trajectory starts from the stored state, the others from zeros
        padded, masks = R.split_and_pad_trajectories(x, st.dones)
        starts = torch.cat([torch.ones(1, st.num_envs), dones[:-1]]) != 0
        per_env = starts.sum(0)
        at = torch.cat([per_env.new_zeros(1), per_env.cumsum(0)])[:-1]
        hidden = tuple(torch.zeros(1, masks.shape[1], 9).index_copy(1, at, s) for s in start)
        mem.rnn.zero_grad()
        want = mem(padded, masks=masks, hidden_states=hidden)
        (want * w).sum().backward()
        want_g = [p.grad.clone() for p in mem.rnn.parameters()]
        mem.rnn.zero_grad()
        got = mem(x, dones=st.dones, hidden_states=start)
        (got * w).sum().backward()
        assert got.shape == want.shape == (st.num_steps, st.num_envs, 9)
        err = float((got - want).detach().abs().max())
        print(f"priv {priv}: outputs {err:.3e}")
        assert err <= 1e-6
        for (name, p), g in zip(mem.rnn.named_parameters(), want_g):
            e = float((p.grad - g).abs().max())
            print(f"priv {priv}: {name} {e:.3e} (largest {float(g.abs().max()):.3e})")
            assert e <= 1e-6 * float(g.abs().max()), name  # of the gradient's largest element
        assert torch.equal(R.lstm_sequence(mem.rnn, x, st.dones, start), got)


def test_dones_of_the_last_step_are_not_read_and_t0_reads_the_start_state():
    rnn, x, h0, c0, _ = make_case(5, 4, 3, 6, seed=1)
    state = (h0[None], c0[None])
    d = planted_dones(5, 4)
    with torch.no_grad():
        a = R.lstm_sequence(rnn, x, d, state)
        d2 = d.clone()
        d2[-1] = 1 - d2[-1]
        assert torch.equal(R.lstm_sequence(rnn, x, d2, state), a)
        one, _ = rnn(x[:1], state)
        assert torch.equal(a[:1], one)  # env 0 has a done at t = 0: t = 0 itself still reads h0 / c0
        zero, _ = rnn(x[1:2, :1])
        assert torch.equal(a[1:2, :1], zero)  # and t = 1 reads zeros there


def test_memory_sequence_mode_arguments():
    m = R.Memory(4, hidden_size=6)
    x, d = torch.randn(5, 2, 4), torch.zeros(5, 2)
    state = (torch.zeros(1, 2, 6), torch.zeros(1, 2, 6))
    with pytest.raises(ValueError, match="mutually exclusive"):
        m(x, masks=torch.ones(5, 2, dtype=torch.bool), hidden_states=state, dones=d)
    with pytest.raises(ValueError, match="Hidden states"):
        m(x, dones=d)
    assert m(x, dones=d, hidden_states=state).shape == (5, 2, 6)
    g = R.Memory(4, type="gru", num_layers=2, hidden_size=6)  # what the kernels refuse runs through the torch loop
    assert g(x, dones=d, hidden_states=torch.zeros(2, 2, 6)).shape == (5, 2, 6)


# ---------------------------------------------------------------------------------------------- 2: generator
@pytest.mark.parametrize("priv", [False, True])
def test_env_generator_matches_the_padded_generator_without_host_reads(priv, monkeypatch):
    alg, dones = planted_rollout(priv)
    st, policy = alg.storage, alg.policy
    T, N = st.num_steps, st.num_envs
    memories = (policy.memory_a, policy.memory_c)
    old = list(st.recurrent_mini_batch_generator(2, 2, memories))

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"Tensor.{name} called: a host read of a device value")
        return f

    for name in ("tolist", "nonzero", "item"):
        monkeypatch.setattr(torch.Tensor, name, refuse(name))
    monkeypatch.setattr(torch, "split", refuse("split"))
    monkeypatch.setattr(nn.utils.rnn, "pad_sequence", refuse("pad_sequence"))
    new = list(st.recurrent_env_mini_batch_generator(2, 2, memories))
    monkeypatch.undo()
    assert len(new) == len(old) == 4
    dc = 7 if priv else 5
    for i, (a, b) in enumerate(zip(new, old)):
        e = slice((i % 2) * N // 2, (i % 2 + 1) * N // 2)
        assert "masks" not in a
        assert a["observations"].shape == (T, N // 2, 5) and a["critic_observations"].shape == (T, N // 2, dc)
        assert a["dones"].shape == (T, N // 2) and a["dones"].dtype == torch.uint8
        assert torch.equal(a["dones"].float(), dones[:, e])
        assert torch.equal(a["observations"], st.observations[:, e])
        assert torch.equal(a["critic_observations"], (st.privileged_observations if priv else st.observations)[:, e])
        for k, which in (("hidden_a", 0), ("hidden_c", 1)):
            assert len(a[k]) == 2
            for s, s0 in zip(a[k], st.start_states[which]):
                assert s.shape == (1, N // 2, 9) and torch.equal(s, s0[:, e])
        for k in ("actions", "values", "returns", "advantages", "actions_log_prob", "mu", "sigma"):
            assert torch.equal(a[k], b[k]), k
        # the padded observations, un-padded, are the slices
        assert torch.equal(R.unpad_trajectories(b["observations"], b["masks"]), a["observations"])
    # a memory that never stepped reads zeros
    st.start_states = [None, None]
    rec = next(st.recurrent_env_mini_batch_generator(2, 1, memories))
    assert all(s.shape == (1, N // 2, 9) and not s.any() for k in ("hidden_a", "hidden_c") for s in rec[k])


# ---------------------------------------------------------------------------------------------- 3: runner
def recurrent_cfg(**alg_kw):
    c = RslRlOnPolicyRunnerCfg(device="cpu", num_steps_per_env=8, save_interval=1000, experiment_name="toy")
    c.policy = RslRlPpoActorCriticRecurrentCfg(actor_hidden_dims=[16, 16], critic_hidden_dims=[16], rnn_hidden_dim=12)
    c.algorithm.num_learning_epochs = 2
    for k, v in alg_kw.items():
        setattr(c.algorithm, k, v)
    return c


def toy_run(monkeypatch, **alg_kw):
    """(the runner after 2 iterations, the loss of the first minibatch, the names of the generators that ran)."""
    runner = OnPolicyRunner(RslRlVecEnvWrapper(ToyEnv()), recurrent_cfg(**alg_kw).to_dict(), log_dir=None, device="cpu")
    losses, used = [], []
    backward = torch.Tensor.backward

    def spy(self, *a, **k):
        losses.append(float(self.detach()))
        return backward(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "backward", spy)
    st = runner.alg.storage
    for name in ("recurrent_mini_batch_generator", "recurrent_env_mini_batch_generator"):
        def wrap(*a, _f=getattr(st, name), _n=name, **k):
            used.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(st, name, wrap)
    runner.learn(2)
    monkeypatch.undo()
    return runner, losses[0], used


def learned(runner):
    """last_iteration_stats without the wall-clock entries."""
    return {k: v for k, v in runner.last_iteration_stats.items() if not k.startswith("Perf/")}


def test_runner_with_the_switch_on_and_off(monkeypatch):
    monkeypatch.delenv("H12_RNN_UPDATE_FUSED", raising=False)
    default, loss_d, used_d = toy_run(monkeypatch)
    off, loss_off, used_off = toy_run(monkeypatch, fused_rnn_update=False)
    on, loss_on, used_on = toy_run(monkeypatch, fused_rnn_update=True)
    monkeypatch.setenv("H12_RNN_UPDATE_FUSED", "1")
    env_on, loss_env, used_env = toy_run(monkeypatch)
    assert not default.alg.fused_rnn_update and not off.alg.fused_rnn_update
    assert on.alg.fused_rnn_update and env_on.alg.fused_rnn_update
    assert set(used_d) == set(used_off) == {"recurrent_mini_batch_generator"}
    assert set(used_on) == set(used_env) == {"recurrent_env_mini_batch_generator"}
    # off: the default path, bit for bit
    assert learned(default) == learned(off) and len(learned(off)) >= 3 and loss_d == loss_off
    for a, b in zip(default.alg.policy.parameters(), off.alg.policy.parameters()):
        assert torch.equal(a, b)
    # on: the same first minibatch (same seed, same rollout, same minibatch of envs), then a finite run
    print(f"first-minibatch loss: default {loss_d!r}, sequence form {loss_on!r}")
    assert abs(loss_on - loss_d) <= 1e-5 and loss_env == loss_on
    stats = on.last_iteration_stats
    assert all(torch.isfinite(torch.tensor(float(stats[k]))) for k in ("Loss/value_function", "Loss/surrogate"))
    assert learned(on) == learned(env_on)


@pytest.mark.parametrize("why,policy_kw,ppo_kw", [
    ("GRU", {"rnn_type": "gru"}, {}),
    ("num_layers = 2", {"rnn_num_layers": 2}, {}),
    ("hidden size 257", {"rnn_hidden_dim": 257}, {}),
    ("bf16", {}, {"precision": "bf16"}),
])
def test_refusals_name_the_limit(why, policy_kw, ppo_kw, monkeypatch):
    monkeypatch.delenv("H12_RNN_UPDATE_FUSED", raising=False)
    policy = ActorCriticRecurrent(6, 6, 3, actor_hidden_dims=(8,), critic_hidden_dims=(8,),
                                  **{"rnn_hidden_dim": 8, **policy_kw})
    with pytest.raises(ValueError) as e:
        PPO(policy, device="cpu", fused_rnn_update=True, **ppo_kw)
    assert why in str(e.value) and "fused_rnn_update" in str(e.value)
    PPO(policy, device="cpu", **ppo_kw)  # the default path takes all of them
    monkeypatch.setenv("H12_RNN_UPDATE_FUSED", "1")
    with pytest.raises(ValueError, match="fused_rnn_update"):
        PPO(policy, device="cpu", **ppo_kw)


def test_refused_with_a_feed_forward_policy():
    with pytest.raises(ValueError, match="fused_rnn_update needs a recurrent policy"):
        PPO(ActorCritic(6, 6, 3, actor_hidden_dims=(8,), critic_hidden_dims=(8,)), device="cpu", fused_rnn_update=True)


# ---------------------------------------------------------------------------------------------- 4: the GPU test's rule
@pytest.mark.parametrize("shape", [(8, 17, 5, 20), (8, 33, 45, 64), (4, 1, 1, 1)])
def test_backward_rule_separates_an_fp32_evaluation_from_three_mistakes(shape):
    """The rule of tests/test_gpu_recurrent_sequence.py (normalised error against fp64, measured in units of the CPU
    library LSTM's own error over the padded form) on an fp32 emulation: the right loop is within the cap of 64, each
    planted mistake is beyond 1e3."""
    T, N, d_in, H = shape
    rnn, x, h0, c0, dh = make_case(T, N, d_in, H, seed=sum(shape))
    dones = planted_dones(T, N)
    ref = seq_grads(rnn, x, dones, h0, c0, dh)
    yard, per = worst_error(library_padded_grads(rnn, x, dones, h0, c0, dh), ref)
    yard = max(yard, U)
    right, _ = worst_error(seq_grads(rnn, x, dones, h0, c0, dh, dtype=torch.float32), ref)
    print(f"{shape}: yardstick {yard:.3e} ({per}), fp32 loop {right:.3e} = {right / yard:.2f} x")
    assert right <= 64 * yard
    for m in MISTAKES:
        wrong, _ = worst_error(seq_grads(rnn, x, dones, h0, c0, dh, dtype=torch.float32, mistake=m), ref)
        print(f"{shape}: {m} {wrong:.3e} = {wrong / yard:.3e} x")
        assert wrong > 1e3 * yard, m
