"""GPU: the fused recurrent policy step (h12learn_lstm_pack / h12learn_lstm_step, h12env.policy.FusedLSTMStep and
RecurrentPolicy) and the recurrent actor-critic on the real env.  DESIGN.md section 7q.  U = 2^-24.

a  accuracy against an fp64 evaluation of the same fp32 parameters, inputs and state, elementwise inside an a-priori
   bound propagated in fp64 (``lstm_fp64_with_bound`` of tests/helpers/lstm_ref.py, shared with the tests of the
   normaliser and the shape edges in tests/test_gpu_recurrent_edges.py; the MLP part is the bound of
   tests/test_gpu_policy.py; e_x = 0 here, no test of this file hands the kernel a normaliser):
       e_z  = e_x |W_ih|^T + e_h |W_hh|^T + (K + 3) U (|x||W_ih|^T + |h||W_hh|^T + |b_ih| + |b_hh|),   K = d_in + H
              (a K + 1 term fmaf chain in any order, and the rounding of b_ih + b_hh at pack time)
       e_s  = e_z / 4 + 8 U s   for s = sigmoid(z)   (1/4-Lipschitz; expf within 2 ulp, one add, one true division)
       e_g  = e_z + 8 U |g|     for g = tanh(z)      (1-Lipschitz)
       e_c' = [f c] + [i g] + U |c'|,  [a b] = |a| e_b + |b| e_a + e_a e_b + U |a b|   (product rule, one rounding each)
       e_h' = [o tanh(c')],  e_tanh(c') = e_c' + 8 U |tanh(c')|
   and e_h' feeds the MLP's bound.  The function takes the incoming state's errors, so it chains over steps (d).
b  against torch.nn.LSTM + the MLP on the CPU in fp32 (same parameters): within bound + bound, torch obeying the same.
c  bitwise: run to run, row subsets, in place == out of place, reset mask == zeroed state, two networks == two calls,
   NaN containment.
d  eight free-running steps with planted dones against the fp64 recursion, inside the chained bound.
e  pack + step in place inside a captured graph; the first call over 64 KiB of LDS refused inside a capture.
f  PPO.act with H12_POLICY_FUSED=1 at 64 envs: graphed == eager bit for bit; inside b's bounds of the torch path.
g  training 64 envs x 8 steps with class_name=ActorCriticRecurrent; mean |ratio - 1| of the first minibatch < 1e-3.
h  play.py --fused and sim2sim.py --fused on a recurrent checkpoint, one subprocess each.
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
SHIMS = ROOT / "h1v2-isaac_amd" / "shims"
SCRIPTS = ROOT / "h1v2-isaac_amd" / "scripts"
for p in (str(SHIMS), str(ROOT / "tests" / "helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

from h12env.policy import FusedLSTMStep, RecurrentPolicy  # noqa: E402
from lstm_ref import clone_states, lstm_fp64_with_bound, make_inputs, make_pairs, torch_cpu  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 33)
REAL = [512, 256, 128]
# (d_in, H, MLP hidden widths, d_out); the last one needs more than 64 KiB of LDS
SHAPES = [(1, 16, [], 1), (3, 24, [24], 12), (45, 64, [40, 24], 12), (451, 256, REAL, 12)]
TASK = "Isaac-Velocity-Flat-H12_12dof-v0"


def fraction(got, ref, bound):
    return float(((got.double().cpu() - ref.double().cpu()).abs() / bound.cpu()).max())


# ---------------------------------------------------------------------------------------------- a, b
@pytest.mark.parametrize("n_nets", [1, 2])
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_accuracy_against_fp64_bound_and_torch_lstm(gpu, case, n_nets):
    shape = SHAPES[case]
    pairs = make_pairs(shape, n_nets, seed=case)
    f = FusedLSTMStep(pairs)
    worst = worst_t = 0.0
    for n in NS:
        x, states = make_inputs(shape, n, n_nets, seed=1000 * case + n)
        before = clone_states(states)
        ys = f(x, states)
        for k, (rnn, net) in enumerate(pairs):
            ref, bound = lstm_fp64_with_bound(rnn, net, x, *before[k])
            cpu = torch_cpu(rnn, net, x, *before[k])
            for name, got, r64, e, rt in zip(("y", "h", "c"), (ys[k], *states[k]), ref, bound, cpu):
                assert got.shape == r64.shape and torch.isfinite(got).all()
                fa, fb = fraction(got, r64, e), fraction(got, rt, 2 * e)
                ft = fraction(rt, r64, e)
                worst, worst_t = max(worst, fa), max(worst_t, ft)
                print(f"shape {shape} nets {n_nets} n {n} net {k} {name}: kernel {fa:.3e} of the bound, "
                      f"kernel - torch {fb:.3e} of twice the bound, torch {ft:.3e}")
                assert fa <= 1.0, (shape, n_nets, n, k, name, fa)
                assert fb <= 1.0, (shape, n_nets, n, k, name, fb)
    print(f"WORST shape {shape} nets {n_nets}: kernel {worst:.3e} torch {worst_t:.3e}")


# ---------------------------------------------------------------------------------------------- c
@pytest.fixture(scope="module")
def bitwise_setup(gpu):
    out = []
    for case in (2, 3):
        shape = SHAPES[case]
        pairs = make_pairs(shape, 2, seed=40 + case)
        x, states = make_inputs(shape, 33, 2, seed=60 + case)
        f = FusedLSTMStep(pairs)
        new = clone_states(states)
        ys = f(x, new)
        out.append((shape, pairs, f, x, states, ys, new))
    return out


def same(states_a, states_b):
    return all(torch.equal(a, b) for pa, pb in zip(states_a, states_b) for a, b in zip(pa, pb))


def test_bitwise_run_to_run_row_subset_and_in_place(bitwise_setup):
    for shape, pairs, f, x, states, ys, new in bitwise_setup:
        again = clone_states(states)
        y2 = f(x, again)
        assert all(torch.equal(a, b) for a, b in zip(y2, ys)) and same(again, new)
        part = [(h[5:20].clone(), c[5:20].clone()) for h, c in states]
        yp = f(x[5:20].contiguous(), part)
        assert all(torch.equal(a, b[5:20]) for a, b in zip(yp, ys))
        assert all(torch.equal(a, b[5:20]) for pa, pb in zip(part, new) for a, b in zip(pa, pb))
        # out of place: the inputs stay, the outputs are those of the in-place call
        keep = clone_states(states)
        outs = [(torch.empty_like(h), torch.empty_like(c)) for h, c in states]
        yo = f(x, keep, out_states=outs)
        assert same(keep, states) and same(outs, new) and all(torch.equal(a, b) for a, b in zip(yo, ys))


def test_bitwise_reset_mask_equals_zeroed_state(bitwise_setup):
    for shape, pairs, f, x, states, ys, new in bitwise_setup:
        mask = torch.zeros(33, dtype=torch.uint8, device="cuda")
        mask[[0, 7, 16, 32]] = 1
        masked = clone_states(states)
        ym = f(x, masked, reset=mask)
        zeroed = clone_states(states)
        for h, c in zeroed:
            h[mask.bool()] = 0
            c[mask.bool()] = 0
        yz = f(x, zeroed)
        assert all(torch.equal(a, b) for a, b in zip(ym, yz)) and same(masked, zeroed)
        assert not torch.equal(ym[0][7], ys[0][7]) and torch.equal(ym[0][8], ys[0][8])
        yb = f(x, clone_states(states), reset=mask.bool())  # a bool mask is the same bytes
        assert all(torch.equal(a, b) for a, b in zip(yb, ym))


def test_bitwise_two_networks_equal_two_calls(bitwise_setup):
    for shape, pairs, f, x, states, ys, new in bitwise_setup:
        for k, pair in enumerate(pairs):
            st = clone_states(states[k:k + 1])
            (y,) = FusedLSTMStep([pair])(x, st)
            assert torch.equal(y, ys[k]) and same(st, new[k:k + 1]), k


def test_bitwise_nan_row_stays_in_its_row(bitwise_setup):
    for shape, pairs, f, x, states, ys, new in bitwise_setup:
        keep = torch.arange(33, device="cuda") != 5
        for where in ("x", "h", "c"):
            xn, sn = x.clone(), clone_states(states)
            {"x": xn, "h": sn[0][0], "c": sn[0][1]}[where][5] = float("nan")
            yn = f(xn, sn)
            # every other row is untouched, bit for bit; a NaN in network 0's state does not reach network 1 at all
            assert torch.equal(yn[0][keep], ys[0][keep]) and torch.equal(yn[1][keep], ys[1][keep]), where
            assert not torch.equal(yn[0][5], ys[0][5]), where
            assert where == "x" or torch.equal(yn[1], ys[1]), where
            for (h, c), (hr, cr) in zip(sn, new):
                assert torch.equal(h[keep], hr[keep]) and torch.equal(c[keep], cr[keep]), where


# ---------------------------------------------------------------------------------------------- d
def test_eight_free_running_steps_stay_inside_the_chained_bound(gpu):
    shape = SHAPES[2]
    n, steps = 17, 8
    (rnn, net), = make_pairs(shape, 1, seed=7)
    f = FusedLSTMStep([(rnn, net)])
    g = torch.Generator().manual_seed(8)
    xs = torch.randn(steps, n, shape[0], generator=g).cuda()
    dones = torch.zeros(steps, n, dtype=torch.bool)
    dones[2, [0, 16]] = True
    dones[5, [3, 16]] = True
    state = [(torch.zeros(n, shape[1], device="cuda"), torch.zeros(n, shape[1], device="cuda"))]
    h64 = c64 = eh = ec = torch.zeros(n, shape[1], dtype=torch.float64, device="cuda")
    reset = None
    for t in range(steps):
        (y,) = f(xs[t], state, reset=reset)  # the rows that were done at t - 1 read zeros
        (y64, h64, c64), (ey, eh, ec) = lstm_fp64_with_bound(rnn, net, xs[t], h64, c64, eh, ec)
        for name, got, ref, e in (("y", y, y64, ey), ("h", state[0][0], h64, eh), ("c", state[0][1], c64, ec)):
            fr = fraction(got, ref, e)
            print(f"step {t} {name}: {fr:.3e} of the chained bound (largest bound {float(e.max()):.3e})")
            assert fr <= 1.0, (t, name, fr)
        d = dones[t].cuda()
        reset = d.to(torch.uint8)
        h64, c64, eh, ec = (torch.where(d[:, None], torch.zeros_like(v), v) for v in (h64, c64, eh, ec))


# ---------------------------------------------------------------------------------------------- e
def test_pack_and_step_in_place_inside_a_captured_graph(bitwise_setup):
    shape, pairs, f, x, states, ys, new = bitwise_setup[1]  # over 64 KiB of LDS: the fixture made the first call
    eager_state = clone_states(states)
    eager = []
    for _ in range(3):
        eager.append([y.clone() for y in f(x, eager_state, repack=True)])
    st = clone_states(states)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        f(x, st, repack=True)
    torch.cuda.current_stream().wait_stream(s)
    for (h, c), (h0, c0) in zip(st, states):
        h.copy_(h0), c.copy_(c0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = f(x, st, repack=True)
    for k in range(3):
        g.replay()
        assert all(torch.equal(a, b) for a, b in zip(out, eager[k])), k
    assert same(st, eager_state)


def test_first_call_over_64_kib_of_lds_is_refused_inside_a_capture(gpu):
    # the raised-limit flag is one per kernel and process: only a fresh process makes a first call
    child = ROOT / "tests" / "helpers" / "lstm_lds_limit_child.py"
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, str(child)], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ok lstm_step\n" in p.stdout


# ---------------------------------------------------------------------------------------------- f, g, h
def _make_env(task, n=64, seed=3):
    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    cfg.seed = seed
    return gym.make(task, cfg=cfg)


def _recurrent_runner(task, n=64, **agent_kw):
    import dataclasses

    import biped_tasks.tasks  # noqa: F401
    from isaaclab_rl.rsl_rl import RslRlPpoActorCriticRecurrentCfg, RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    agent.device = "cuda:0"
    for k, v in agent_kw.items():
        setattr(agent, k, v)
    kept = {fl.name: getattr(agent.policy, fl.name) for fl in dataclasses.fields(agent.policy) if fl.name != "class_name"}
    agent.policy = RslRlPpoActorCriticRecurrentCfg(**kept)
    env = RslRlVecEnvWrapper(_make_env(task, n))
    return agent, env, OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0")


def _collect(monkeypatch, graph: bool, steps=4):
    monkeypatch.setenv("H12_POLICY_FUSED", "1")
    monkeypatch.setenv("H12_PPO_GRAPH", "1" if graph else "0")
    _, env, runner = _recurrent_runner(TASK)
    alg = runner.alg
    torch.manual_seed(17)
    rec = []
    obs, _ = env.get_observations()
    with torch.inference_mode():
        for t in range(steps):
            a = alg.act(obs, obs)
            rec.append([v.clone() for v in (obs, a, alg._values, alg._log_prob, alg._mu)])
            if t == 1:  # an update in the middle of the rollout: the next step must see the new weights
                for p in alg.policy.parameters():
                    p.mul_(1.03125)
            obs, r, dones, infos = env.step(a)
            if t == 2:
                dones = dones.clone()
                dones[[1, 40]] = 1  # planted: reset(dones) zeroes these rows of the state the kernel updates in place
            alg.process_env_step(r, dones, infos)
            rec[-1] += [t_.clone() for pair in alg.policy.get_hidden_states() for t_ in pair]
    env.close()
    return runner, rec


def test_rsl_collection_fused_graphed_equals_eager_and_default(gpu, monkeypatch):
    rg, recg = _collect(monkeypatch, True)
    re_, rece = _collect(monkeypatch, False)
    assert rg.alg._ga is not None and getattr(re_.alg, "_ga", None) is None
    names = ("obs", "action", "value", "logprob", "mean", "h_a", "c_a", "h_c", "c_c")
    for t, (g, e) in enumerate(zip(recg, rece)):
        for name, a, b in zip(names, g, e):
            assert torch.equal(a, b), (t, name, float((a - b).abs().max()))
    assert (rece[2][5][0, [1, 40]] == 0).all() and (rece[2][5][0, 2] != 0).any()
    # the default torch path from the states the fused step started from (the weights of the last steps are the
    # runner's): one step each, inside b's bounds
    pol = re_.alg.policy
    with torch.no_grad():
        for t in (2, 3):
            obs, _, value, _, mean = rece[t][:5]
            ha, ca, hc, cc = (s[0] for s in rece[t - 1][5:])
            for what, mem, net, h, c, got in (("mean", pol.memory_a, pol.actor, ha, ca, mean),
                                              ("value", pol.memory_c, pol.critic, hc, cc, value)):
                (y64, _, _), (e, _, _) = lstm_fp64_with_bound(mem.rnn, net, obs, h, c)
                out, _ = mem.rnn(obs.unsqueeze(0), (h.unsqueeze(0).contiguous(), c.unsqueeze(0).contiguous()))
                default = net(out[0])
                fa, fd = fraction(got, y64, e), fraction(got, default, 2 * e)
                print(f"step {t} {what}: fused {fa:.4f} of the bound, fused - default {fd:.4f} of twice the bound")
                assert fa <= 1.0 and fd <= 1.0, (t, what, fa, fd)


def test_training_with_the_recurrent_class(gpu, monkeypatch):
    monkeypatch.delenv("H12_POLICY_FUSED", raising=False)
    agent, env, runner = _recurrent_runner(TASK, num_steps_per_env=8)
    alg, policy = runner.alg, runner.alg.policy
    assert policy.is_recurrent and policy.memory_a.rnn.hidden_size == 256
    seen = []
    inner = alg._minibatch

    def probe(b, idx, stats, rec=None):
        if not seen:
            with torch.no_grad():
                policy.act(rec["observations"], masks=rec["masks"], hidden_states=rec["hidden_a"])
                ratio = torch.exp(policy.get_actions_log_prob(rec["actions"]) - rec["actions_log_prob"].squeeze(-1))
                seen.append(float((ratio - 1).abs().mean()))
        return inner(b, idx, stats, rec=rec)

    monkeypatch.setattr(alg, "_minibatch", probe)
    before = {k: v.clone() for k, v in policy.state_dict().items()}
    runner.learn(2)
    env.close()
    stats = runner.last_iteration_stats
    for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"):
        assert torch.isfinite(torch.tensor(stats[k])), (k, stats[k])
    for k in ("memory_a.rnn.weight_hh_l0", "memory_c.rnn.weight_ih_l0", "actor.0.weight", "critic.0.weight"):
        assert not torch.equal(before[k], policy.state_dict()[k]), k
    print(f"first minibatch of the first epoch: mean |ratio - 1| = {seen[0]:.3e}")
    assert seen[0] < 1e-3


def test_play_and_sim2sim_fused_on_a_recurrent_checkpoint(gpu, tmp_path):
    task = "Isaac-Velocity-Flat-H12_12dof-Play-v0"
    agent, env, runner = _recurrent_runner(task, n=16)
    with torch.no_grad():
        for p in runner.alg.policy.actor.parameters():
            p.mul_(0.01)  # near-zero actions: the robot stands under the default-pose PD
    run = tmp_path / "logs" / "rsl_rl" / agent.experiment_name / "run0"
    runner.save(str(run / "model_0.pt"))
    env.close()
    envv = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT / "h1v2-isaac_amd"), os.environ.get("PYTHONPATH", "")]))
    envv.pop("H12_POLICY_FUSED", None)
    p = subprocess.run([sys.executable, str(SCRIPTS / "play.py"), "--task", task, "--num_envs", "16", "--load_run",
                        "run0", "--steps", "5", "--fused"], cwd=tmp_path, env=envv, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert (run / "exported" / "policy.pt").exists() and (run / "exported" / "env.yaml").exists()
    assert hasattr(torch.jit.load(str(run / "exported" / "policy.pt")), "rnn")
    p = subprocess.run([sys.executable, str(SCRIPTS / "sim2sim.py"), str(run / "exported"), "--num_envs", "16",
                        "--episode_length", "0.2", "--fused"], cwd=tmp_path, env=envv, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "[sim2sim] 16 envs" in p.stdout
    height = float(p.stdout.split("base height mean ")[1].split(" m")[0])
    assert 0.85 < height < 1.2


def test_recurrent_policy_fused_against_the_torch_modules(gpu):
    shape = SHAPES[2]
    (rnn, net), = make_pairs(shape, 1, seed=21)
    fused, plain = RecurrentPolicy(rnn, net, fused=True), RecurrentPolicy(rnn, net)
    g = torch.Generator().manual_seed(22)
    for t in range(4):
        x = torch.randn(9, shape[0], generator=g).cuda()
        if t == 2:
            d = torch.tensor([0, 1, 0, 0, 0, 0, 0, 0, 1], device="cuda")
            fused.reset(d), plain.reset(d)
        if fused.state is not None:  # both from the same fp32 state: one step apart, inside twice a's bound
            plain._ensure_state(9, x.device)
            for dst, src in zip(plain.state, fused.state):
                dst.copy_(src)
            h0, c0 = fused.state[0][0].clone(), fused.state[1][0].clone()
        else:
            h0 = c0 = torch.zeros(9, shape[1], device="cuda")
        a, b = fused(x), plain(x)
        _, (e, _, _) = lstm_fp64_with_bound(rnn, net, x, h0, c0)
        assert a.shape == (9, shape[3]) and fraction(a, b, 2 * e) <= 1.0, t
    assert (fused.state[0][0, 1] != 0).any()
    fused.reset()
    assert all((s == 0).all() for s in fused.state)
