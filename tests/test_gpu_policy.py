"""GPU: the fused policy MLP forward (h12learn_mlp_pack / h12learn_mlp_forward, h12env.policy.FusedMLP).

Gate 1  exact-integer layout: integer inputs and asymmetric integer weights with every partial sum below 2^24, so any
        summation order is exact and the output must equal the int64 reference exactly (a wrong lane map, a dropped k
        or a swapped index cannot hide in rounding).
Gate 2  accuracy against an fp64 evaluation of the same fp32 parameters and inputs, elementwise inside an a-priori
        forward bound propagated in fp64 with u = 2^-24:
            e_0 = 4u (|x| + |mean|) / scale                  (subtract, scale's add and sqrt, divide)
            e_z = |W| e_h + (K + 2) u (|W||h| + |b|)         (a K + 1 term fmaf chain in any order)
            e_h = e_z + 4u |h|                               (ELU is 1-Lipschitz; expm1f within a few ulp)
        measured on the MI355X (worst fraction of the bound over every shape below): fused 0.226, torch fp32 0.220
        (the single layer with 3 inputs; 4e-6 on 451-512-256-128-12, where the compounded bound is loose).
Gate 3  bitwise properties: run to run, row-subset invariance, two networks == two calls, NaN containment, re-pack;
        the first call over 64 KiB of LDS is refused inside a stream capture (inference and training kernels, in a
        fresh process: tests/helpers/lds_limit_child.py).
Gate 4  integration at 64 envs: both trainers' collection with H12_POLICY_FUSED=1 (graphed == eager bit for bit, inside
        gate 2 of the default path), play.py --fused and sim2sim.py --fused in a subprocess each,
        get_inference_policy(fused=True).
"""
import copy
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[1]
SHIMS = ROOT / "h1v2-isaac_amd" / "shims"
SCRIPTS = ROOT / "h1v2-isaac_amd" / "scripts"
for p in (str(SHIMS), str(ROOT / "tests" / "helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

from h12env.policy import FusedMLP  # noqa: E402
from lstm_ref import make_norm  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NS = (1, 31, 32, 33, 95)
REAL = [512, 256, 128]
# (d_in, hidden widths, output width per network): every listed d_in, hidden and d_out, one and two networks
SHAPES = [
    (1, [24], [1]),
    (3, [], [12]),
    (3, [24, 40, 64], [12]),
    (45, [40, 24], [33]),
    (45, [64, 40, 24], [33, 1]),
    (451, [64], [1, 12]),
    (451, REAL, [12]),
    (451, REAL, [12, 1]),
    (1024, [512], [33]),  # more than 64 KiB of LDS
]
NORMS = ("none", "var", "std")


def seq(dims):
    mods = []
    for i in range(len(dims) - 1):
        mods.append(nn.Linear(dims[i], dims[i + 1]))
        if i + 2 < len(dims):
            mods.append(nn.ELU())
    return nn.Sequential(*mods)


def make_nets(d_in, hidden, d_outs, seed):
    torch.manual_seed(seed)
    nets = [seq([d_in] + hidden + [d]) for d in d_outs]
    for net in nets:
        for m in net:
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.bias, std=0.3)
    return [n.cuda().requires_grad_(False) for n in nets]


def make_x(n, d_in, norm, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d_in, generator=g)
    if norm is not None:
        mean = (norm.running_mean if hasattr(norm, "running_mean") else norm._mean).cpu().reshape(-1)
        x = x * 2 + mean
    return x.cuda()


@torch.no_grad()
def fp64_with_bound(nets, norm, x):
    """(y64, e_L) per network: the fp64 evaluation of the fp32 parameters on the fp32 input and the a-priori bound."""
    h0 = x.double()
    e0 = torch.zeros_like(h0)
    if norm is not None:
        if hasattr(norm, "running_mean"):
            mean, scale = norm.running_mean.double(), torch.sqrt(norm.running_var.double() + norm.epsilon)
        else:
            mean, scale = norm._mean.double().reshape(-1), norm._std.double().reshape(-1) + norm.eps
        e0 = 4 * U * (h0.abs() + mean.abs()) / scale
        h0 = (h0 - mean) / scale
    out = []
    for net in nets:
        h, e = h0, e0
        lins = [m for m in net if isinstance(m, nn.Linear)]
        for i, lin in enumerate(lins):
            W, b = lin.weight.double(), lin.bias.double()
            K = W.shape[1]
            e = e @ W.abs().T + (K + 2) * U * (h.abs() @ W.abs().T + b.abs())
            h = h @ W.T + b
            if i + 1 < len(lins):
                h = torch.where(h > 0, h, torch.expm1(h))
                e = e + 4 * U * h.abs()
        out.append((h, e))
    return out


@torch.no_grad()
def torch_path(nets, norm, x):
    h = x
    if norm is not None:
        h = norm(x, update=False) if hasattr(norm, "running_mean") else norm(x)
    return [net(h) for net in nets]


# ---------------------------------------------------------------------------------------------- gate 1
def int_weights(out, k_in, lo, span):
    j = torch.arange(out)[:, None]
    k = torch.arange(k_in)[None, :]
    return (3 * j + 5 * k + (j * k) % 4 + (j // 3)) % span + lo  # asymmetric in (j, k)


def int_net(dims, wlo, wspan, blo, bspan):
    net = seq(dims)
    ints = []
    for m in net:
        if isinstance(m, nn.Linear):
            W = int_weights(m.out_features, m.in_features, wlo, wspan)
            b = (7 * torch.arange(m.out_features)) % bspan + blo
            m.weight.data.copy_(W.float()), m.bias.data.copy_(b.float())
            ints.append((W.long(), b.long()))
    return net.cuda().requires_grad_(False), ints


@pytest.mark.parametrize("d_in,d_out", [(1, 1), (3, 12), (45, 33), (451, 12), (451, 64), (1024, 40)])
def test_exact_integers_single_layer_signed(gpu, d_in, d_out):
    net, [(W, b)] = int_net([d_in, d_out], -4, 9, -5, 11)
    f = FusedMLP([net])
    for n in NS:
        g = torch.Generator().manual_seed(n)
        x = torch.randint(-8, 9, (n, d_in), generator=g)
        ref = x.long() @ W.T + b  # |sum| <= 1024 * 32 + 5 < 2^24
        (y,) = f(x.float().cuda())
        assert torch.equal(y.cpu().long(), ref) and torch.equal(y.cpu(), ref.float()), (n, d_in, d_out)


@pytest.mark.parametrize("dims,xmax", [([45, 40, 24, 33], 3), ([451, 24, 40, 12], 1), ([3, 33, 17, 1], 3)])
def test_exact_integers_three_layers_nonnegative(gpu, dims, xmax):
    # non-negative data: ELU is the identity.  The largest partial sum (45 * 6 + 2 = 272, then 40 * 2 * 272 + 2,
    # then 24 * 2 * 21762 + 2, about 1.05e6; less for the other shapes) is below 2^24
    net, ints = int_net(dims, 0, 3, 0, 3)
    f = FusedMLP([net])
    for n in NS:
        g = torch.Generator().manual_seed(n)
        x = torch.randint(0, xmax + 1, (n, dims[0]), generator=g)
        h = x.long()
        for W, b in ints:
            h = h @ W.T + b
        assert int(h.max()) < 2 ** 24
        (y,) = f(x.float().cuda())
        assert torch.equal(y.cpu(), h.float()), (n, dims)


# ---------------------------------------------------------------------------------------------- gate 2
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_accuracy_against_fp64_bound(gpu, case):
    d_in, hidden, d_outs = SHAPES[case]
    kind = NORMS[case % 3]
    nets = make_nets(d_in, hidden, d_outs, seed=case)
    norm = make_norm(kind, d_in, seed=100 + case)
    f = FusedMLP(nets, normalizer=norm)
    worst_fused = worst_torch = 0.0
    for n in NS:
        x = make_x(n, d_in, norm, seed=1000 * case + n)
        ys = f(x)
        yt = torch_path(nets, norm, x)
        for i, (y64, e) in enumerate(fp64_with_bound(nets, norm, x)):
            assert ys[i].shape == y64.shape
            ff = float(((ys[i].double() - y64).abs() / e).max())
            ft = float(((yt[i].double() - y64).abs() / e).max())
            worst_fused, worst_torch = max(worst_fused, ff), max(worst_torch, ft)
            print(f"shape {SHAPES[case]} norm {kind} n {n} net {i}: fused {ff:.3e} of the bound, torch {ft:.3e}")
            assert torch.isfinite(ys[i]).all() and ff <= 1.0, (SHAPES[case], kind, n, i, ff)
    print(f"WORST shape {SHAPES[case]} norm {kind}: fused {worst_fused:.3e} torch {worst_torch:.3e}")


# ---------------------------------------------------------------------------------------------- gate 3
@pytest.fixture(scope="module")
def bitwise_setup(gpu):
    out = []
    for case, (d_in, hidden, d_outs) in enumerate([(45, [40, 24], [33, 1]), (451, REAL, [12, 1])]):
        nets = make_nets(d_in, hidden, d_outs, seed=40 + case)
        norm = make_norm(NORMS[1 + case], d_in, seed=50 + case)
        x = make_x(128, d_in, norm, seed=60 + case)
        f = FusedMLP(nets, normalizer=norm)
        full = tuple(y.clone() for y in f(x))
        out.append((nets, norm, x, f, full))
    return out


def test_bitwise_run_to_run_and_row_subsets(bitwise_setup):
    for nets, norm, x, f, full in bitwise_setup:
        again = f(x)
        assert all(torch.equal(a, b) for a, b in zip(again, full))
        for n in NS:
            part = f(x[:n].contiguous())
            for a, b in zip(part, full):
                assert a.shape[0] == n and torch.equal(a, b[:n]), n


def test_bitwise_two_networks_equal_two_calls(bitwise_setup):
    for nets, norm, x, f, full in bitwise_setup:
        for i, net in enumerate(nets):
            (y,) = FusedMLP([net], normalizer=norm)(x)
            assert torch.equal(y, full[i]), i
        swapped = FusedMLP(nets[::-1], normalizer=norm)(x)
        assert torch.equal(swapped[0], full[1]) and torch.equal(swapped[1], full[0])


def test_bitwise_nan_row_stays_in_its_row(bitwise_setup):
    for nets, norm, x, f, full in bitwise_setup:
        xn = x[:95].clone()
        xn[5] = float("nan")
        keep = torch.arange(95, device=x.device) != 5
        for y, ref in zip(f(xn), full):
            assert torch.equal(y[keep], ref[:95][keep])
            assert torch.isnan(y[5]).all()


def test_repack_follows_in_place_weight_changes(bitwise_setup):
    nets, norm, x, _, full = bitwise_setup[0]
    nets = [copy.deepcopy(n) for n in nets]
    f = FusedMLP(nets, normalizer=norm)
    assert all(torch.equal(a, b) for a, b in zip(f(x), full))
    with torch.no_grad():
        nets[0][0].weight.mul_(1.5)
        nets[1][2].bias.add_(0.25)
    stale = f(x)
    assert all(torch.equal(a, b) for a, b in zip(stale, full))  # the packed copy is what the kernel reads
    fresh = f(x, repack=True)
    assert not torch.equal(fresh[0], full[0]) and not torch.equal(fresh[1], full[1])
    new = FusedMLP(nets, normalizer=norm)(x)
    assert all(torch.equal(a, b) for a, b in zip(fresh, new))
    f.refresh()
    assert all(torch.equal(a, b) for a, b in zip(f(x), new))


def test_forward_and_pack_inside_a_captured_graph(bitwise_setup):
    nets, norm, x, _, full = bitwise_setup[1]
    nets = [copy.deepcopy(n) for n in nets]
    f = FusedMLP(nets, normalizer=norm)
    inp = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        f(inp, repack=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = f(inp, repack=True)
    g.replay()
    assert all(torch.equal(a, b) for a, b in zip(out, full))
    with torch.no_grad():
        nets[0][0].weight.mul_(0.5)
    inp.copy_(x.flip(0))
    g.replay()  # the replay re-packs the changed weights and reads the new input
    new = FusedMLP(nets, normalizer=norm)(x.flip(0).contiguous())
    assert all(torch.equal(a, b) for a, b in zip(out, new))


def test_first_call_over_64_kib_of_lds_is_refused_inside_a_capture(gpu):
    # the raised-limit flags are one per kernel and process: only a fresh process makes a first call
    child = ROOT / "tests" / "helpers" / "lds_limit_child.py"
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, str(child)], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for kernel in ("mlp_forward", "mlp_forward_train", "mlp_backward"):
        assert f"ok {kernel}\n" in p.stdout, kernel


# ---------------------------------------------------------------------------------------------- gate 4
@torch.no_grad()
def _inside_gate2_of_default(nets, x, fused_out, what):
    """fused within e_L of fp64 (gate 2), and so within 2 e_L of the default torch path, which obeys the same bound."""
    default = [net(x) for net in nets]
    for i, (y64, e) in enumerate(fp64_with_bound(nets, None, x)):
        ff = float(((fused_out[i].double() - y64).abs() / e).max())
        fd = float(((fused_out[i].double() - default[i].double()).abs() / (2 * e)).max())
        print(f"{what} net {i}: fused {ff:.4f} of the bound, fused - default {fd:.4f} of twice the bound")
        assert ff <= 1.0 and fd <= 1.0, (what, i, ff, fd)


def _make_env(task, n=64, seed=3):
    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    cfg.seed = seed
    return gym.make(task, cfg=cfg)


def _rsl_collect(monkeypatch, graph: bool, steps=8):
    import biped_tasks.tasks  # noqa: F401
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    task = "Isaac-Velocity-Flat-H12_12dof-v0"
    monkeypatch.setenv("H12_POLICY_FUSED", "1")
    monkeypatch.setenv("H12_PPO_GRAPH", "1" if graph else "0")
    agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    agent.device = "cuda:0"
    env = RslRlVecEnvWrapper(_make_env(task))
    runner = OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0")
    torch.manual_seed(17)
    rec = []
    obs, _ = env.get_observations()
    with torch.inference_mode():
        for t in range(steps):
            a = runner.alg.act(obs, obs)
            rec.append([v.clone() for v in (obs, a, runner.alg._values, runner.alg._log_prob, runner.alg._mu)])
            if t == steps // 2:  # an update in the middle of the rollout: the next step must see the new weights
                for p in runner.alg.policy.parameters():
                    p.mul_(1.03125)
            obs, _, _, _ = env.step(a)
    env.close()
    return runner, rec


def test_rsl_collection_fused_graphed_equals_eager_and_default(gpu, monkeypatch):
    rg, recg = _rsl_collect(monkeypatch, True)
    re_, rece = _rsl_collect(monkeypatch, False)
    assert rg.alg._ga is not None and getattr(re_.alg, "_ga", None) is None
    for t, (g, e) in enumerate(zip(recg, rece)):
        for name, a, b in zip(("obs", "action", "value", "logprob", "mean"), g, e):
            assert torch.equal(a, b), (t, name, float((a - b).abs().max()))
    assert not torch.equal(rece[0][4], rece[-1][4])
    # the default path on the rollout's own observations; the weights of the last steps are the runner's
    pol = re_.alg.policy
    for obs, _, value, _, mean in rece[len(rece) // 2 + 1:]:
        _inside_gate2_of_default([pol.actor, pol.critic], obs, (mean, value), "rsl collection")


def _cleanrl_collect(monkeypatch, graph: bool, steps=8):
    from h12env import cleanrl

    monkeypatch.setenv("H12_POLICY_FUSED", "1")
    env = _make_env("Isaac-Velocity-CaT-Flat-H12_12dof-v0")
    torch.manual_seed(21)
    agent = cleanrl.Agent(env).to("cuda:0")
    col = cleanrl._Collector(agent, graph)
    rec = []
    raw = env.reset()[0]["policy"]
    with torch.no_grad():
        for t in range(steps):
            obs, action, logprob, value = col.normalise_act(raw)
            mean = col._fused(obs)[0]
            rec.append([v.clone() for v in (obs, action, logprob, value, mean)])
            if t == steps // 2:
                for p in agent.parameters():
                    p.mul_(1.03125)
            raw = env.step(action)[0]["policy"]
    env.close()
    return agent, col, rec


def test_cleanrl_collection_fused_graphed_equals_eager_and_default(gpu, monkeypatch):
    ag, cg, recg = _cleanrl_collect(monkeypatch, True)
    ae, ce, rece = _cleanrl_collect(monkeypatch, False)
    assert cg._graphs and not ce._graphs
    for t, (g, e) in enumerate(zip(recg, rece)):
        for name, a, b in zip(("obs", "action", "logprob", "value", "mean"), g, e):
            assert torch.equal(a, b), (t, name, float((a - b).abs().max()))
    for k in ("running_mean", "running_var", "count"):
        assert torch.equal(getattr(ag.obs_rms, k), getattr(ae.obs_rms, k)), k
    for obs, _, _, value, mean in rece[len(rece) // 2 + 1:]:
        _inside_gate2_of_default([ae.actor_mean, ae.critic], obs, (mean, value[:, None]), "cleanrl collection")


def test_inference_policy_fused_within_gate2_of_default(gpu):
    import biped_tasks.tasks  # noqa: F401
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    task = "Isaac-Velocity-Flat-H12_12dof-Play-v0"
    agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    agent.device = "cuda:0"
    env = RslRlVecEnvWrapper(_make_env(task))
    runner = OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0")
    fused = runner.get_inference_policy(device="cuda:0", fused=True)
    default = runner.get_inference_policy(device="cuda:0")
    obs, _ = env.get_observations()
    with torch.inference_mode():
        for _ in range(5):
            a = fused(obs)
            assert a.shape == default(obs).shape == (64, 12)
            norm = runner.obs_normalizer if runner.empirical_normalization else None
            (y64, e), = fp64_with_bound([runner.alg.policy.actor], norm, obs)
            assert float(((a.double() - y64).abs() / e).max()) <= 1.0
            assert float(((a.double() - default(obs).double()).abs() / (2 * e)).max()) <= 1.0
            obs, _, _, _ = env.step(a)
    env.close()


def test_play_and_sim2sim_fused_in_subprocesses(gpu, tmp_path):
    import biped_tasks.tasks  # noqa: F401
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    task = "Isaac-Velocity-Flat-H12_12dof-Play-v0"
    agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    agent.device = "cuda:0"
    env = RslRlVecEnvWrapper(_make_env(task, n=16))
    runner = OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0")
    with torch.no_grad():
        for p in runner.alg.policy.actor.parameters():
            p.mul_(0.01)  # near-zero actions: the robot stands under the default-pose PD
    run = tmp_path / "logs" / "rsl_rl" / agent.experiment_name / "run0"
    runner.save(str(run / "model_0.pt"))
    env.close()
    envv = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT / "h1v2-isaac_amd"), os.environ.get("PYTHONPATH", "")]))
    p = subprocess.run([sys.executable, str(SCRIPTS / "play.py"), "--task", task, "--num_envs", "16", "--load_run",
                        "run0", "--steps", "5", "--fused"], cwd=tmp_path, env=envv, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert (run / "exported" / "policy.pt").exists() and (run / "exported" / "env.yaml").exists()
    p = subprocess.run([sys.executable, str(SCRIPTS / "sim2sim.py"), str(run / "exported"), "--num_envs", "16",
                        "--episode_length", "0.2", "--fused"], cwd=tmp_path, env=envv, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "[sim2sim] 16 envs" in p.stdout
    height = float(p.stdout.split("base height mean ")[1].split(" m")[0])
    assert 0.85 < height < 1.2
