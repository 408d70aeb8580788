"""GPU: the trainable fused policy MLP (h12learn_mlp_pack_t / _forward_train / _backward, csrc/h12_policy_train.hip;
h12env.policy.TrainableFusedMLP; PPO(fused_learner=True)).  DESIGN.md section 7l.  u = 2^-24, R = the row tile.

Gate 1  exact integers: non-negative integer networks (ELU the identity, f' = 1, a unit with h = 0 exactly included),
        signed integer dY, every sum of absolute products below 2^24: y, every h_l, dZ_l, dX, db_l and dW_l equal the
        int64 reference exactly at n in {1, R-1, R, R+1, 2R+1}; a signed single layer, forward and dX.
Gate 2  against fp64 of the same fp32 parameters, elementwise inside the a-priori bounds of tests/helpers/mlp_bounds.py;
        the backward reference is teacher-forced on the kernel's own saved h_l.  The 1024-wide input of section 7g's
        shape list is wider than h12learn_mlp_train_max_width() and is refused (tests/test_policy_train_api.py).
Gate 3  bitwise: forward_train's y == h12learn_mlp_forward's; run to run (db included); row-subset invariance of dZ; a
        NaN row of dY stays in its row; forward + backward in a captured graph follow a later weight change.
Gate 4  the runner at 64 envs (minibatch 384 rows): captured update == eager update bit for bit, also with symmetry
        (augmentation + mirror loss) and with the privileged critic; one minibatch's gradients against the loss
        restated in fp64 (fused error <= 4 x the default path's error + u max|grad| per tensor); train.py
        --fused_learner in a subprocess, and its checkpoint in a default-path runner.
"""
import copy
import json
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn as nn
from torch.distributions import Normal

ROOT = Path(__file__).resolve().parents[1]
SHIMS = ROOT / "h1v2-isaac_amd" / "shims"
for p in (str(SHIMS), str(ROOT / "tests" / "helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mlp_bounds as B  # noqa: E402
from h12env import _learn  # noqa: E402
from h12env.policy import FusedMLP, TrainableFusedMLP, _wgrad  # noqa: E402

pytestmark = pytest.mark.gpu

U = B.U
REAL = [512, 256, 128]


def tile_ns():
    r = _learn.mlp_train_rows()
    return (1, r - 1, r, r + 1, 2 * r + 1)


def run_kernels(net, x, dy, need_dx=True):
    """The entry points called directly: y, [h_l], [dZ_l], [db_l], [dW_l], dX of one network."""
    lins = B.linears(net)
    pairs = [(m.weight.detach(), m.bias.detach()) for m in lins]
    desc = _learn.mlp_desc([pairs])
    packed = torch.empty(_learn.mlp_packed_bytes(desc) // 4, device=x.device)
    packed_t = torch.empty(_learn.mlp_packed_t_bytes(desc) // 4, device=x.device)
    _learn.mlp_pack(desc, packed)
    _learn.mlp_pack_t(desc, packed_t)
    y, hs = _learn.mlp_forward_train(desc, packed, x)
    dzs, dbs, dx = _learn.mlp_backward(desc, packed_t, dy, hs, need_dx=need_dx)
    acts = [x] + hs
    dWs = [_wgrad(dz, acts[l]) for l, dz in enumerate(dzs + [dy])]
    return {"y": y, "h": hs, "dz": dzs, "db": dbs, "dW": dWs, "dx": dx}


def run_autograd(net, x, dy):
    """The same through TrainableFusedMLP and torch.autograd: y, dX, [db_l], [dW_l]."""
    net = copy.deepcopy(net).requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    y = TrainableFusedMLP(net)(xg)
    y.backward(dy)
    lins = B.linears(net)
    return {"y": y.detach(), "dx": xg.grad, "db": [m.bias.grad for m in lins], "dW": [m.weight.grad for m in lins]}


# ---------------------------------------------------------------------------------------------- gate 1
@pytest.mark.parametrize("dims,xmax", [([45, 40, 24, 33], 3), ([451, 24, 40, 12], 1), ([3, 33, 17, 1], 3)])
def test_exact_integers_three_layers_nonnegative(gpu, dims, xmax):
    # unit 1 of layer 0 and unit 2 of layer 1 have zero weights and bias: h = 0 exactly, where f' must be 1
    net, ints = B.int_net(dims, 0, 3, 0, 3, zero_units=((0, 1), (1, 2)))
    net = net.cuda().requires_grad_(False)
    for n in tile_ns():
        g = torch.Generator().manual_seed(n)
        x = torch.randint(0, xmax + 1, (n, dims[0]), generator=g)
        dy = torch.randint(-2, 3, (n, dims[-1]), generator=g)
        ref = B.int_reference(ints, x, dy)
        assert ref["peak"] < 2 ** 24, ref["peak"]
        assert int(ref["h"][0][:, 1].abs().max()) == 0 and int(ref["h"][1][:, 2].abs().max()) == 0
        out = run_kernels(net, x.float().cuda(), dy.float().cuda())
        via = run_autograd(net, x.float().cuda(), dy.float().cuda())
        for key in ("y", "dx"):
            assert torch.equal(out[key].cpu(), ref[key].float()), (key, n, dims)
            assert torch.equal(via[key].cpu(), ref[key].float()), ("autograd", key, n, dims)
        for key in ("h", "dz", "db", "dW"):
            assert len(out[key]) == len(ref[key])
            for l, (a, b) in enumerate(zip(out[key], ref[key])):
                assert a.shape == b.shape and torch.equal(a.cpu(), b.float()), (key, l, n, dims)
        for key in ("db", "dW"):
            for l, (a, b) in enumerate(zip(via[key], ref[key])):
                assert a.shape == b.shape and torch.equal(a.cpu(), b.float()), ("autograd", key, l, n, dims)


@pytest.mark.parametrize("d_in,d_out", [(1, 1), (3, 12), (45, 33), (451, 12), (451, 64), (512, 40)])
def test_exact_integers_single_layer_signed(gpu, d_in, d_out):
    net, ints = B.int_net([d_in, d_out], -4, 9, -5, 11)
    net = net.cuda().requires_grad_(False)
    for n in tile_ns():
        g = torch.Generator().manual_seed(n)
        x = torch.randint(-8, 9, (n, d_in), generator=g)
        dy = torch.randint(-8, 9, (n, d_out), generator=g)
        ref = B.int_reference(ints, x, dy)  # |y| <= 512 * 32 + 5, |dX| <= 64 * 32, |dW| <= 65 * 64
        assert ref["peak"] < 2 ** 24
        out = run_kernels(net, x.float().cuda(), dy.float().cuda())
        assert out["h"] == [] and out["dz"] == []
        for key in ("y", "dx"):
            assert torch.equal(out[key].cpu(), ref[key].float()), (key, n, d_in, d_out)
        assert torch.equal(out["db"][0].cpu(), ref["db"][0].float()), (n, d_in, d_out)
        assert torch.equal(out["dW"][0].cpu(), ref["dW"][0].float()), (n, d_in, d_out)


# ---------------------------------------------------------------------------------------------- gate 2
# section 7g's shape list with one output per network; (1024, [512], 33) is wider than the training kernels' maximum
SHAPES = [
    [1, 24, 1],
    [3, 12],
    [3, 24, 40, 64, 12],
    [45, 40, 24, 33],
    [45, 64, 40, 24, 33],
    [45, 64, 40, 24, 1],
    [451, 64, 1],
    [451, 64, 12],
]
REAL_SHAPES = [[451] + REAL + [12], [451] + REAL + [1]]


def torch_autograd(net, x, dy):
    """torch's own forward and backward, layer by layer, keeping every h_l and dZ_l."""
    net = copy.deepcopy(net).requires_grad_(True)
    lins = B.linears(net)
    xg = x.clone().requires_grad_(True)
    h, hs, zs = xg, [], []
    for i, lin in enumerate(lins):
        z = lin(h)
        if i + 1 < len(lins):
            z.retain_grad()
            zs.append(z)
            h = nn.functional.elu(z)
            hs.append(h.detach())
        else:
            h = z
    h.backward(dy)
    return {"y": h.detach(), "h": hs, "dz": [z.grad for z in zs], "dx": xg.grad, "db": [m.bias.grad for m in lins],
            "dW": [m.weight.grad for m in lins]}


def fractions(lins, x, dy, out):
    """Worst fraction of the bound per quantity; the backward reference is teacher-forced on out's own h."""
    hs64, es, y64, ey = B.forward_fp64(lins, x)
    fr = {"y": B.fraction(out["y"], y64, ey)}
    fr["h"] = max([B.fraction(h, r, e) for h, r, e in zip(out["h"], hs64, es)], default=0.0)
    ref = B.backward_fp64(lins, x, out["h"], dy)
    for key in ("dz", "db", "dW"):
        assert len(out[key]) == len(ref[key])
        fr[key] = max([B.fraction(a, r, e) for a, (r, e) in zip(out[key], ref[key])], default=0.0)
    fr["dx"] = B.fraction(out["dx"], *ref["dx"])
    return fr


def check_against_fp64(dims, n, seed):
    net = B.random_net(dims, seed).cuda().requires_grad_(False)
    lins = B.linears(net)
    g = torch.Generator().manual_seed(1000 * seed + n)
    x = torch.randn(n, dims[0], generator=g).cuda()
    dy = torch.randn(n, dims[-1], generator=g).cuda()
    out = run_kernels(net, x, dy)
    for l, h in enumerate(out["h"]):  # a condition on the inputs: both branches of f' are exercised in every layer
        assert bool((h > 0).any()) and bool((h < 0).any()), (dims, n, l)
    ff = fractions(lins, x, dy, out)
    ft = fractions(lins, x, dy, torch_autograd(net, x, dy))
    print(f"shape {dims} n {n}: fused " + " ".join(f"{k} {v:.3e}" for k, v in ff.items()))
    print(f"shape {dims} n {n}: torch " + " ".join(f"{k} {v:.3e}" for k, v in ft.items()))
    for k, v in ff.items():
        assert v <= 1.0, (dims, n, k, v)
    # the autograd wrapper returns what the entry points computed
    via = run_autograd(net, x, dy)
    assert torch.equal(via["y"], out["y"]) and torch.equal(via["dx"], out["dx"])
    for key in ("db", "dW"):
        assert all(torch.equal(a, b) for a, b in zip(via[key], out[key])), key
    return ff, ft


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_accuracy_against_fp64_bound(gpu, case):
    r = _learn.mlp_train_rows()
    worst_f, worst_t = {}, {}
    for n in (1, r + 1, 3 * r - 1):
        ff, ft = check_against_fp64(SHAPES[case], n, seed=case)
        for k in ff:
            worst_f[k], worst_t[k] = max(worst_f.get(k, 0.0), ff[k]), max(worst_t.get(k, 0.0), ft[k])
    print(f"WORST shape {SHAPES[case]}: fused {max(worst_f.values()):.3e} torch {max(worst_t.values()):.3e}")


@pytest.mark.parametrize("case", range(len(REAL_SHAPES)))
def test_accuracy_against_fp64_bound_real_shapes(gpu, case):
    ff, ft = check_against_fp64(REAL_SHAPES[case], 3 * _learn.mlp_train_rows() - 1, seed=20 + case)
    print(f"WORST shape {REAL_SHAPES[case]}: fused {max(ff.values()):.3e} torch {max(ft.values()):.3e}")


# ---------------------------------------------------------------------------------------------- gate 3
@pytest.fixture(scope="module")
def bitwise_setup(gpu):
    out = []
    n = 4 * _learn.mlp_train_rows()
    for case, dims in enumerate([[45, 40, 24, 33], [451] + REAL + [12]]):
        net = B.random_net(dims, 40 + case).cuda().requires_grad_(False)
        g = torch.Generator().manual_seed(60 + case)
        x = torch.randn(n, dims[0], generator=g).cuda()
        dy = torch.randn(n, dims[-1], generator=g).cuda()
        full = run_kernels(net, x, dy)
        out.append((net, x, dy, full))
    return out


def flat(out):
    return [out["y"], out["dx"]] + out["h"] + out["dz"] + out["db"] + out["dW"]


def test_bitwise_forward_train_equals_the_inference_forward(bitwise_setup):
    for net, x, dy, full in bitwise_setup:
        (y,) = FusedMLP([net])(x)
        assert torch.equal(full["y"], y)
        for n in tile_ns():
            (y,) = FusedMLP([net])(x[:n].contiguous())
            assert torch.equal(run_kernels(net, x[:n].contiguous(), dy[:n].contiguous())["y"], y), n


def test_bitwise_run_to_run(bitwise_setup):
    for net, x, dy, full in bitwise_setup:
        for _ in range(2):
            again = run_kernels(net, x, dy)
            assert all(torch.equal(a, b) for a, b in zip(flat(again), flat(full)))


def test_bitwise_row_subsets(bitwise_setup):
    for net, x, dy, full in bitwise_setup:
        for m in tile_ns():
            part = run_kernels(net, x[:m].contiguous(), dy[:m].contiguous())
            for key in ("h", "dz"):
                for l, (a, b) in enumerate(zip(part[key], full[key])):
                    assert a.shape[0] == m and torch.equal(a, b[:m]), (key, l, m)
            assert torch.equal(part["dx"], full["dx"][:m]) and torch.equal(part["y"], full["y"][:m]), m


def test_bitwise_nan_row_of_dy_stays_in_its_row(bitwise_setup):
    for net, x, dy, full in bitwise_setup:
        n = 2 * _learn.mlp_train_rows() + 1
        bad = dy[:n].clone()
        bad[5] = float("nan")
        keep = torch.arange(n, device=x.device) != 5
        out = run_kernels(net, x[:n].contiguous(), bad)
        for l, (a, b) in enumerate(zip(out["dz"], full["dz"])):
            assert torch.equal(a[keep], b[:n][keep]), l
            assert torch.isnan(a[5]).all(), l
        assert torch.equal(out["dx"][keep], full["dx"][:n][keep]) and torch.isnan(out["dx"][5]).all()


def test_forward_and_backward_inside_a_captured_graph_follow_weight_changes(bitwise_setup):
    net, x, dy, full = bitwise_setup[1]
    net = copy.deepcopy(net).requires_grad_(True)
    params = list(net.parameters())
    f = TrainableFusedMLP(net)
    inp = x.clone().requires_grad_(True)

    def body():
        y = f(inp)
        return [y.detach()] + list(torch.autograd.grad(y, [inp] + params, dy))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = body()
    g.replay()
    lins = B.linears(net)
    assert torch.equal(out[0], full["y"]) and torch.equal(out[1], full["dx"])
    for l in range(len(lins)):
        assert torch.equal(out[2 + 2 * l], full["dW"][l]) and torch.equal(out[3 + 2 * l], full["db"][l]), l
    with torch.no_grad():
        lins[1].weight.mul_(0.5)
        lins[2].bias.add_(0.25)
        inp.copy_(x.flip(0))
    g.replay()  # the replay packs the changed weights, both layouts, and reads the new input
    new = run_kernels(net.requires_grad_(False), x.flip(0).contiguous(), dy)
    assert not torch.equal(new["y"], full["y"])
    assert torch.equal(out[0], new["y"]) and torch.equal(out[1], new["dx"])
    for l in range(len(lins)):
        assert torch.equal(out[2 + 2 * l], new["dW"][l]) and torch.equal(out[3 + 2 * l], new["db"][l]), l


def test_two_applications_in_one_graph_accumulate(gpu):
    net = B.random_net([45, 40, 24, 12], 77).cuda()
    f = TrainableFusedMLP(net)
    g = torch.Generator().manual_seed(5)
    xa, xb = (torch.randn(37, 45, generator=g).cuda() for _ in range(2))
    dya, dyb = (torch.randn(37, 12, generator=g).cuda() for _ in range(2))
    ((f(xa) * dya).sum() + (f(xb) * dyb).sum()).backward()
    a, b = run_kernels(net, xa, dya), run_kernels(net, xb, dyb)
    for l, lin in enumerate(B.linears(net)):
        assert torch.equal(lin.weight.grad, a["dW"][l] + b["dW"][l]), l
        assert torch.equal(lin.bias.grad, a["db"][l] + b["db"][l]), l
    with pytest.raises(RuntimeError, match="once_differentiable"):
        x = xa.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad(f(x).square().sum(), x, create_graph=True)
        gx.sum().backward()


# ---------------------------------------------------------------------------------------------- gate 4
def ppo_run(monkeypatch, graph, fused, mode=None, priv=False):
    from h12env import cfg as K
    from h12env.ppo import PPO, ActorCritic

    monkeypatch.setenv("H12_PPO_GRAPH", "1" if graph else "0")
    torch.manual_seed(7)
    pol = ActorCritic(270, 65 if priv else 270, 12, [128, 64], [128, 64])
    sym = None
    if mode is not None:
        sym = {"use_data_augmentation": True, "use_mirror_loss": mode == "both", "mirror_loss_coeff": 0.5,
               "data_augmentation_func": "h12env.symmetry:augment", "_env": K.H12RslEnvCfg()}
    alg = PPO(pol, num_learning_epochs=2, num_mini_batches=4, learning_rate=1e-3, schedule="adaptive", desired_kl=0.01,
              device="cuda:0", symmetry_cfg=sym, fused_learner=fused)
    alg.init_storage(64, 24, [270], [65] if priv else None, [12])  # 1536 rows, minibatches of 384
    out = []
    for u in range(2):
        g = torch.Generator(device="cuda:0").manual_seed(100 + u)
        for k, v in alg.storage.t.items():
            v.copy_(torch.randn(v.shape, generator=g, device="cuda:0") * (0.1 if k == "sigma" else 1.0))
        alg.storage.t["sigma"].abs_().add_(0.5)
        out.append(alg.update())
    return alg, out


@pytest.mark.parametrize("mode,priv", [(None, False), ("both", False), (None, True)])
def test_graph_captured_fused_update_equals_eager(gpu, monkeypatch, mode, priv):
    calls = []
    orig = _learn.mlp_backward
    monkeypatch.setattr(_learn, "mlp_backward", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    a, la = ppo_run(monkeypatch, True, True, mode, priv)
    in_graph = len(calls)
    b, lb = ppo_run(monkeypatch, False, True, mode, priv)
    # per minibatch: actor + critic, and the actor once more under the mirror loss
    per = 3 if mode == "both" else 2
    assert in_graph == 3 * per and len(calls) - in_graph == 2 * 8 * per  # warm-up x 2 + capture; 2 updates x 8
    assert a._graph is not None and b._graph is None and a.fused_learner and b.fused_learner
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.isfinite(p).all() and torch.equal(p, q), (p - q).abs().max()
    assert la == lb and a.learning_rate == b.learning_rate
    # the default path never reaches the kernels and keeps the same state dict
    n_before = len(calls)
    c, lc = ppo_run(monkeypatch, True, False, mode, priv)
    assert len(calls) == n_before and not c.fused_learner
    assert list(a.policy.state_dict()) == list(c.policy.state_dict())
    assert all(math.isfinite(v) for x in la + lc for v in x.values())


def loss_fp64(pol, alg, b, idx):
    """PPO._minibatch's loss (no symmetry, fixed schedule) restated on a double policy."""
    d = {k: v[idx].double() for k, v in b.items()}
    mean = pol.actor(d["observations"])
    dist = Normal(mean, pol.std.expand_as(mean))
    log_prob = dist.log_prob(d["actions"]).sum(dim=-1)
    entropy = dist.entropy().sum(dim=-1)
    value = pol.critic(d["observations"])
    ratio = torch.exp(log_prob - d["actions_log_prob"].squeeze(-1))
    adv = d["advantages"].squeeze(-1)
    surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - alg.clip_param, 1.0 + alg.clip_param)).mean()
    tv, ret = d["values"], d["returns"]
    v_clipped = tv + (value - tv).clamp(-alg.clip_param, alg.clip_param)
    value_loss = torch.max((value - ret).square(), (v_clipped - ret).square()).mean()
    return surrogate + alg.value_loss_coef * value_loss - alg.entropy_coef * entropy.mean()


def test_minibatch_gradients_against_fp64(gpu, monkeypatch):
    from h12env.ppo import PPO, ActorCritic

    monkeypatch.setenv("H12_PPO_GRAPH", "0")

    def make(fused):
        torch.manual_seed(11)
        pol = ActorCritic(270, 270, 12, REAL, REAL)
        alg = PPO(pol, num_mini_batches=4, schedule="fixed", max_grad_norm=float("inf"), entropy_coef=0.01,
                  device="cuda:0", fused_learner=fused)
        alg.init_storage(64, 24, [270], None, [12])
        g = torch.Generator(device="cuda:0").manual_seed(5)
        t = alg.storage.t
        rnd = lambda k, s=1.0: torch.randn(t[k].shape, generator=g, device="cuda:0") * s  # noqa: E731
        with torch.no_grad():  # a rollout the policy could have produced: ratios near 1, both clip branches live
            t["observations"].copy_(rnd("observations"))
            mu = alg.policy.actor(t["observations"])
            t["mu"].copy_(mu), t["sigma"].fill_(1.0)
            t["actions"].copy_(mu + rnd("actions"))
            t["actions_log_prob"].copy_(Normal(mu, 1.0).log_prob(t["actions"]).sum(-1, keepdim=True)
                                        + rnd("actions_log_prob", 0.15))
            t["values"].copy_(alg.policy.critic(t["observations"]) + rnd("values", 0.15))
            t["returns"].copy_(t["values"] + rnd("returns"))
            t["advantages"].copy_(rnd("advantages"))
        return alg

    fused, default = make(True), make(False)
    b = default._batch()
    idx = torch.randperm(1536, generator=torch.Generator().manual_seed(9))[:384].cuda()
    pol64 = copy.deepcopy(default.policy).double()
    pol64._fused_learner = None
    loss_fp64(pol64, default, b, idx).backward()
    ref = {k: p.grad for k, p in pol64.named_parameters()}
    grads = {}
    assert fused.fused_learner and not default.fused_learner
    assert all(torch.equal(p, q) for p, q in zip(fused.policy.parameters(), default.policy.parameters()))
    assert all(torch.equal(fused.storage.t[k], v) for k, v in default.storage.t.items())
    for name, alg in (("fused", fused), ("default", default)):
        alg._minibatch(alg._batch(), idx, torch.zeros(3, device="cuda:0"))
        grads[name] = {k: p.grad.clone() for k, p in alg.policy.named_parameters()}
    for k, r in ref.items():
        if k == "std":
            continue  # outside the networks: the same torch operations on either path
        ef = float((grads["fused"][k].double() - r).abs().max())
        ed = float((grads["default"][k].double() - r).abs().max())
        gmax = float(r.abs().max())
        print(f"{k}: max|grad| {gmax:.3e}  fused error {ef:.3e}  default error {ed:.3e}")
        assert gmax > 0 and ef <= 4 * ed + U * gmax, (k, ef, ed, gmax)


def test_train_script_with_fused_learner(gpu, tmp_path):
    train = ROOT / "h1v2-isaac_amd" / "scripts" / "train.py"
    task = "Isaac-Velocity-Flat-H12_12dof-v0"
    r = subprocess.run([sys.executable, str(train), "--task", task, "--headless", "--num_envs", "64",
                        "--max_iterations", "2", "--fused_learner", "agent.save_interval=1"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    run = next((tmp_path / "logs" / "rsl_rl" / "h12_12dof_flat").iterdir())
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2
    assert all(math.isfinite(v) for x in lines for v in x.values() if isinstance(v, float))
    assert "fused_learner: true" in (run / "params" / "agent.yaml").read_text()
    ck = run / "model_2.pt"
    assert ck.exists()

    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    cfg.scene.num_envs = 64
    cfg.sim.device = "cuda:0"
    agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    agent.device = "cuda:0"
    env = RslRlVecEnvWrapper(gym.make(task, cfg=cfg))
    runner = OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0")
    assert not runner.alg.fused_learner
    runner.load(str(ck))
    saved = torch.load(ck, map_location="cuda:0", weights_only=True)["model_state_dict"]
    assert list(saved) == list(runner.alg.policy.state_dict())
    for k, v in runner.alg.policy.state_dict().items():
        assert torch.equal(v, saved[k]) and torch.isfinite(v).all(), k
    runner.learn(1)  # the default path trains on from the fused run's parameters and optimizer state
    env.close()
