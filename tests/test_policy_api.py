"""CPU: the fused policy MLP's surface without a GPU.  The h12learn_mlp_* entry points are declared, bound and exported,
validate every argument before any HIP call, and h12env.policy.FusedMLP on CPU tensors evaluates the torch modules
(both normaliser kinds), rejects what the kernel cannot express, rebuilds an exported policy.pt, and serves the
``fused=True`` switches of both trainers on the CPU toy envs."""
import ctypes as C
import os
import re
import sys
from pathlib import Path

import pytest
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "shims"))
sys.path.insert(0, str(ROOT / "tests" / "helpers"))

from h12env import _learn, build  # noqa: E402
from h12env._abi import load_library  # noqa: E402
from h12env._learn import LEARN_SYMBOLS, MlpDesc, learn_library  # noqa: E402

MLP_NAMES = {"h12learn_mlp_max_width", "h12learn_mlp_packed_bytes", "h12learn_mlp_pack", "h12learn_mlp_forward"}


def seq(dims, act=nn.ELU):
    mods = []
    for i in range(len(dims) - 1):
        mods.append(nn.Linear(dims[i], dims[i + 1]))
        if i + 2 < len(dims):
            mods.append(act())
    return nn.Sequential(*mods)


def shape_desc(dims_per_net, ptr=0):
    """A descriptor with the given layer widths and every pointer set to ``ptr`` (never dereferenced on the host)."""
    d = MlpDesc()
    d.n_nets = len(dims_per_net)
    d.d_in = dims_per_net[0][0] if dims_per_net else 0
    for i, dims in enumerate(dims_per_net[:_learn.MLP_MAX_NETS]):
        d.nets[i].n_layers = len(dims) - 1
        for k, w in enumerate(dims[:_learn.MLP_MAX_LAYERS + 1]):
            d.nets[i].dims[k] = w
        for k in range(min(len(dims) - 1, _learn.MLP_MAX_LAYERS)):
            d.nets[i].W[k] = d.nets[i].b[k] = ptr or None
    return d


def test_header_symbols_and_exports_name_the_mlp_entry_points():
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "h12learn.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(h12learn_[a-z_]+)\s*\(", src))
    assert MLP_NAMES <= declared
    assert declared == set(LEARN_SYMBOLS)
    lib = load_library()
    for n in MLP_NAMES:
        assert hasattr(lib, n), n
    assert lib.h12env_abi_version() == 9
    assert "h12_policy.hip" in {p.name for p in build.sources()}
    assert C.sizeof(MlpDesc) == 32 + 4 * (40 + 2 * 8 * 8)  # the C struct's layout on LP64


def test_max_width_and_packed_bytes():
    lib = learn_library()
    assert lib.h12learn_mlp_max_width() >= 1024
    assert lib.h12learn_mlp_packed_bytes(C.byref(shape_desc([]))) == 0
    assert b"n_nets = 0" in lib.h12learn_last_error()
    assert lib.h12learn_mlp_packed_bytes(None) == 0 and b"desc" in lib.h12learn_last_error()
    prev = 0
    for w in (1, 15, 16, 17, 100, 256, 512):
        nbytes = lib.h12learn_mlp_packed_bytes(C.byref(shape_desc([[450, w, 12]])))
        assert nbytes >= 4 * (450 * w + w + w * 12 + 12) and nbytes % 16 == 0
        assert nbytes >= prev
        prev = nbytes
    one = lib.h12learn_mlp_packed_bytes(C.byref(shape_desc([[450, 512, 256, 128, 12]])))
    two = lib.h12learn_mlp_packed_bytes(C.byref(shape_desc([[450, 512, 256, 128, 12], [450, 512, 256, 128, 1]])))
    assert one < two < 2 * one + 1


def test_argument_validation_without_gpu():
    lib = learn_library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ys = (C.c_void_p * 4)(p, p, p, p)
    mx = lib.h12learn_mlp_max_width()

    def fwd(desc, packed=p, x=p, n=4, y=ys):
        return lib.h12learn_mlp_forward(C.byref(desc) if desc is not None else None, packed, x, n, y, None)

    def pack(desc, packed=p):
        return lib.h12learn_mlp_pack(C.byref(desc) if desc is not None else None, packed, None)

    def err():
        return lib.h12learn_last_error()

    good = [[6, 8, 3]]
    assert fwd(None) == -1 and b"desc" in err()
    assert pack(None) == -1 and b"desc" in err()
    assert fwd(shape_desc([], p)) == -1 and b"n_nets = 0" in err()
    five = shape_desc([[6, 3]] * 4, p)
    five.n_nets = 5
    assert fwd(five) == -1 and b"n_nets = 5" in err()
    assert pack(five) == -1 and b"n_nets = 5" in err()
    nine = shape_desc(good, p)
    nine.nets[0].n_layers = 9
    assert fwd(nine) == -1 and b"n_layers = 9" in err()
    assert pack(nine) == -1 and b"n_layers = 9" in err()
    zero_layers = shape_desc(good, p)
    zero_layers.nets[0].n_layers = 0
    assert fwd(zero_layers) == -1 and b"n_layers = 0" in err()
    assert fwd(shape_desc([[6, 0, 3]], p)) == -1 and b"dims[1] = 0" in err()
    assert fwd(shape_desc([[6, 8, mx + 1]], p)) == -1 and b"dims[2]" in err()
    assert fwd(shape_desc([[mx + 1, 8, 3]], p)) == -1 and b"d_in" in err()
    assert fwd(shape_desc([[0, 8, 3]], p)) == -1 and b"d_in = 0" in err()
    assert fwd(shape_desc([[6, 8, 3], [7, 8, 1]], p)) == -1 and b"dims[0]" in err()
    assert fwd(shape_desc(good, 0)) == -1 and b"W[0]" in err()
    assert pack(shape_desc(good, 0)) == -1 and b"W[0]" in err()
    no_bias = shape_desc(good, p)
    no_bias.nets[0].b[1] = None
    assert fwd(no_bias) == -1 and b"b[1]" in err()
    norm = shape_desc(good, p)
    norm.norm_kind = _learn.MLP_NORM_VAR
    assert fwd(norm) == -1 and b"norm_mean" in err()
    norm.norm_kind = 7
    assert fwd(norm) == -1 and b"norm_kind = 7" in err()
    ok = shape_desc(good, p)
    assert fwd(ok, packed=None) == -1 and b"packed" in err()
    assert pack(ok, packed=None) == -1 and b"packed" in err()
    assert fwd(ok, x=None) == -1 and b"x is null" in err()
    assert fwd(ok, n=0) == -1 and b"n = 0" in err()
    assert fwd(ok, y=None) == -1 and b"y is null" in err()
    assert fwd(ok, y=(C.c_void_p * 4)()) == -1 and b"y[0]" in err()


def test_fused_mlp_on_cpu_equals_the_modules_for_both_normalisers():
    from h12env.cleanrl import RunningMeanStd
    from h12env.policy import FusedMLP
    from h12env.ppo import EmpiricalNormalization, mlp

    torch.manual_seed(3)
    x = torch.randn(9, 7) * 3 + 1
    actor, critic = seq([7, 24, 40, 5]), mlp(7, [16, 8], 1, "elu")  # SplitKLinear layers qualify
    rms = RunningMeanStd(shape=(7,))
    rms.update(torch.randn(50, 7) * 2 + 0.5)
    emp = EmpiricalNormalization([7]).train()
    emp(torch.randn(50, 7) * 2 - 0.5)
    emp.eval()
    before = [t.clone() for t in (rms.running_mean, rms.running_var, rms.count, emp._mean, emp._std, emp.count)]
    for norm in (None, rms, emp):
        f = FusedMLP([actor, critic], normalizer=norm)
        h = x if norm is None else (norm(x, update=False) if norm is rms else norm(x))
        ya, yc = f(x)
        assert torch.equal(ya, actor(h)) and torch.equal(yc, critic(h))
        assert ya.shape == (9, 5) and yc.shape == (9, 1) and not ya.requires_grad
    after = (rms.running_mean, rms.running_var, rms.count, emp._mean, emp._std, emp.count)
    assert all(torch.equal(a, b) for a, b in zip(before, after))  # statistics are read only
    with pytest.raises(RuntimeError, match="autograd"):
        FusedMLP([actor])(x.clone().requires_grad_(True))


def test_fused_mlp_rejects_what_the_kernel_cannot_express():
    from h12env.policy import FusedMLP

    with pytest.raises(ValueError, match="ELU"):
        FusedMLP([seq([6, 8, 3], act=nn.Tanh)])
    with pytest.raises(ValueError, match="layers"):
        FusedMLP([seq([6] + [8] * 8 + [3])])  # 9 linear layers
    FusedMLP([seq([6] + [8] * 7 + [3])])  # 8 are fine
    with pytest.raises(ValueError, match="wider"):
        FusedMLP([seq([6, _learn.mlp_max_width() + 1, 3])])
    with pytest.raises(ValueError, match="networks"):
        FusedMLP([seq([6, 3]) for _ in range(5)])
    with pytest.raises(ValueError, match="inputs"):
        FusedMLP([seq([6, 3]), seq([7, 3])])
    with pytest.raises(ValueError, match="normalizer"):
        FusedMLP([seq([6, 3])], normalizer=nn.BatchNorm1d(6))
    with pytest.raises(ValueError, match="ELU"):
        FusedMLP([nn.Sequential(nn.Linear(6, 8), nn.ELU(alpha=0.5), nn.Linear(8, 3))])


@pytest.mark.parametrize("with_norm", [False, True])
def test_from_exported_round_trips_policy_pt(tmp_path, with_norm):
    from h12env.export import export_policy_as_jit
    from h12env.policy import FusedMLP
    from h12env.ppo import ActorCritic, EmpiricalNormalization

    torch.manual_seed(5)
    policy = ActorCritic(10, 10, 4, actor_hidden_dims=(24, 16), critic_hidden_dims=(8,))
    norm = None
    if with_norm:
        norm = EmpiricalNormalization([10]).train()
        norm(torch.randn(64, 10) * 4 + 2)
        norm.eval()
    path = export_policy_as_jit(policy, norm, str(tmp_path))
    jit = torch.jit.load(path)
    f = FusedMLP.from_exported(jit)
    x = torch.randn(6, 10) * 4 + 2
    (y,) = f(x)
    assert torch.equal(y, jit(x))
    assert [lin.out_features for lin in f._layers[0]] == [24, 16, 4]
    assert (f.normalizer is not None) == with_norm


def test_runner_inference_policy_fused_on_the_cpu_toy_env():
    from h12env.ppo import OnPolicyRunner
    from isaaclab_rl.rsl_rl import RslRlOnPolicyRunnerCfg, RslRlVecEnvWrapper
    from toyenv import ToyEnv

    for empirical in (False, True):
        c = RslRlOnPolicyRunnerCfg(device="cpu", num_steps_per_env=8, save_interval=1000, experiment_name="toy")
        c.policy.actor_hidden_dims = [32, 32]
        c.policy.critic_hidden_dims = [32, 32]
        c.empirical_normalization = empirical
        runner = OnPolicyRunner(RslRlVecEnvWrapper(ToyEnv()), c.to_dict(), log_dir=None, device="cpu")
        runner.learn(1)
        obs, _ = runner.env.get_observations()
        eager = runner.get_inference_policy()(obs)
        fused = runner.get_inference_policy(fused=True)(obs)
        assert fused.shape == (64, 3) and torch.equal(fused, eager)


def test_agent_inference_policy_fused_on_the_cpu_toy_cat_env():
    from h12env.cleanrl import Agent
    from toy_cat import ToyCaTEnv

    torch.manual_seed(2)
    env = ToyCaTEnv()
    agent = Agent(env)
    obs = env.reset()[0]["policy"]
    agent.obs_rms(torch.cat([obs, env.step(torch.zeros(8, 12))[0]["policy"]]))
    stats = [t.clone() for t in (agent.obs_rms.running_mean, agent.obs_rms.running_var, agent.obs_rms.count)]
    with torch.no_grad():
        eager = agent(obs)
    assert torch.equal(agent.inference_policy()(obs), eager)
    assert torch.equal(agent.inference_policy(fused=True)(obs), eager)
    assert all(torch.equal(a, b) for a, b in
               zip(stats, (agent.obs_rms.running_mean, agent.obs_rms.running_var, agent.obs_rms.count)))


def test_collection_switch_defaults_off(monkeypatch):
    from h12env.policy import fused_collection_enabled

    monkeypatch.delenv("H12_POLICY_FUSED", raising=False)
    assert not fused_collection_enabled()
    monkeypatch.setenv("H12_POLICY_FUSED", "1")
    assert fused_collection_enabled()
    assert os.environ["H12_POLICY_FUSED"] == "1"
