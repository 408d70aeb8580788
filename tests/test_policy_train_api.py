"""CPU: the trainable fused MLP's surface without a GPU.  The training entry points of include/h12learn.h are declared,
bound and exported and validate every argument before any HIP call; h12env.policy.TrainableFusedMLP on CPU tensors is
the torch modules bit for bit (outputs and gradients) and refuses a double backward; PPO(fused_learner=True) on the CPU
toy env trains exactly like the default, and refuses what the kernels cannot express."""
import copy
import ctypes as C
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
from mlp_bounds import seq  # noqa: E402

TRAIN_NAMES = {"h12learn_mlp_train_rows", "h12learn_mlp_train_max_width", "h12learn_mlp_packed_t_bytes",
               "h12learn_mlp_pack_t", "h12learn_mlp_forward_train", "h12learn_mlp_backward_workspace_bytes",
               "h12learn_mlp_backward"}


def shape_desc(dims, ptr=0):
    """A one-network descriptor with the given layer widths and every pointer ``ptr`` (never dereferenced on the host)."""
    d = MlpDesc()
    d.n_nets = 1
    d.d_in = dims[0]
    d.nets[0].n_layers = len(dims) - 1
    for k, w in enumerate(dims):
        d.nets[0].dims[k] = w
    for k in range(len(dims) - 1):
        d.nets[0].W[k] = d.nets[0].b[k] = ptr or None
    return d


def test_header_symbols_and_exports_name_the_training_entry_points():
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "h12learn.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(h12learn_[a-z_]+)\s*\(", src))
    assert TRAIN_NAMES <= declared and TRAIN_NAMES <= set(LEARN_SYMBOLS)
    lib = load_library()
    for n in TRAIN_NAMES:
        assert hasattr(lib, n), n
    assert "h12_policy_train.hip" in {p.name for p in build.sources()}
    assert _learn.mlp_train_max_width() >= 512
    r = _learn.mlp_train_rows()
    assert r >= 16 and r % 16 == 0


def test_sizes_follow_the_shapes():
    lib = learn_library()
    r = lib.h12learn_mlp_train_rows()
    d = shape_desc([451, 512, 256, 128, 12])
    nt = lib.h12learn_mlp_packed_t_bytes(C.byref(d))
    assert nt >= 4 * (451 * 512 + 512 * 256 + 256 * 128 + 128 * 12) and nt % 16 == 0
    assert nt < lib.h12learn_mlp_packed_bytes(C.byref(d))  # no biases in the transposed pack
    cols = 512 + 256 + 128 + 12
    for n, blocks in ((1, 1), (r, 1), (r + 1, 2), (24576, (24576 + r - 1) // r)):
        assert lib.h12learn_mlp_backward_workspace_bytes(C.byref(d), n) == 4 * cols * blocks
    assert lib.h12learn_mlp_backward_workspace_bytes(C.byref(d), 0) == 0 and b"n = 0" in lib.h12learn_last_error()


def test_argument_validation_without_gpu():
    lib = learn_library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    arr = (C.c_void_p * 8)(*([p] * 8))
    mx = lib.h12learn_mlp_train_max_width()

    def ref(desc):
        return C.byref(desc) if desc is not None else None

    def pack_t(desc, packed=p):
        return lib.h12learn_mlp_pack_t(ref(desc), packed, None)

    def fwd(desc, packed=p, x=p, n=4, y=p, h=arr):
        return lib.h12learn_mlp_forward_train(ref(desc), packed, x, n, y, h, None)

    def bwd(desc, packed_t=p, dy=p, h=arr, n=4, dz=arr, db=arr, dx=None, ws=p, ws_bytes=1 << 20):
        return lib.h12learn_mlp_backward(ref(desc), packed_t, dy, h, n, dz, db, dx, ws, ws_bytes, None)

    def nbytes_t(desc):
        return -1 if lib.h12learn_mlp_packed_t_bytes(ref(desc)) == 0 else 0

    def nbytes_ws(desc):
        return -1 if lib.h12learn_mlp_backward_workspace_bytes(ref(desc), 4) == 0 else 0

    def err():
        return lib.h12learn_last_error()

    good = [6, 8, 3]
    calls = (pack_t, fwd, bwd, nbytes_t, nbytes_ws)
    for f in calls:
        assert f(None) == -1 and b"desc is null" in err(), f.__name__
        two = shape_desc(good, p)
        two.n_nets = 2
        assert f(two) == -1 and b"n_nets = 2" in err(), f.__name__
        zero = shape_desc(good, p)
        zero.n_nets = 0
        assert f(zero) == -1 and b"n_nets = 0" in err(), f.__name__
        for kind in (_learn.MLP_NORM_VAR, _learn.MLP_NORM_STD, 7):
            norm = shape_desc(good, p)
            norm.norm_kind, norm.norm_mean, norm.norm_scale = kind, p, p
            assert f(norm) == -1 and b"norm_kind = %d" % kind in err(), f.__name__
        assert f(shape_desc([6, mx + 1, 3], p)) == -1 and b"dims[1] = %d" % (mx + 1) in err(), f.__name__
        assert f(shape_desc([6, 8, mx + 1], p)) == -1 and b"dims[2]" in err(), f.__name__
        assert f(shape_desc([mx + 1, 8, 3], p)) == -1 and b"d_in = %d" % (mx + 1) in err(), f.__name__
        assert f(shape_desc([6, 0, 3], p)) == -1 and b"dims[1] = 0" in err(), f.__name__
        nine = shape_desc(good, p)
        nine.nets[0].n_layers = 9
        assert f(nine) == -1 and b"n_layers = 9" in err(), f.__name__
    d = shape_desc(good, p)
    # null and misaligned buffers, rows
    assert pack_t(shape_desc(good, 0)) == -1 and b"W[0]" in err()
    assert pack_t(d, None) == -1 and b"packed_t is null" in err()
    assert pack_t(d, p + 4) == -1 and b"aligned" in err()
    assert fwd(d, packed=None) == -1 and b"packed is null" in err()
    assert fwd(d, packed=p + 4) == -1 and b"aligned" in err()
    assert fwd(d, x=None) == -1 and b"x is null" in err()
    assert fwd(d, n=0) == -1 and b"n = 0" in err()
    assert fwd(d, n=-3) == -1 and b"n = -3" in err()
    assert fwd(d, y=None) == -1 and b"y is null" in err()
    assert fwd(d, h=None) == -1 and b"h is null" in err()
    assert fwd(d, h=(C.c_void_p * 8)()) == -1 and b"h[0] is null" in err()
    assert bwd(d, packed_t=None) == -1 and b"packed_t is null" in err()
    assert bwd(d, dy=None) == -1 and b"dy is null" in err()
    assert bwd(d, n=0) == -1 and b"n = 0" in err()
    assert bwd(d, h=None) == -1 and b"h is null" in err()
    assert bwd(d, dz=None) == -1 and b"dz is null" in err()
    assert bwd(d, dz=(C.c_void_p * 8)()) == -1 and b"dz[0] is null" in err()
    assert bwd(d, db=None) == -1 and b"db is null" in err()
    assert bwd(d, db=(C.c_void_p * 8)(p)) == -1 and b"db[1] is null" in err()
    # workspace: null, and one byte short of what the query asks for
    need = lib.h12learn_mlp_backward_workspace_bytes(C.byref(d), 4)
    assert need == 4 * (8 + 3)
    assert bwd(d, ws=None) == -1 and b"workspace is null" in err()
    assert bwd(d, ws_bytes=need - 1) == -1 and b"workspace_bytes = %d" % (need - 1) in err()
    assert bwd(d, ws_bytes=0) == -1 and b"workspace_bytes = 0" in err()
    r = lib.h12learn_mlp_train_rows()
    assert bwd(d, n=r + 1, ws_bytes=need) == -1 and b"workspace_bytes" in err()  # two blocks need twice as much


def test_trainable_fused_mlp_on_cpu_is_the_torch_modules_bit_for_bit():
    from h12env.policy import TrainableFusedMLP
    from h12env.ppo import mlp

    torch.manual_seed(3)
    for net in (mlp(7, [9, 5], 3, "elu"), seq([4, 6]), seq([5, 33, 17, 8, 2])):
        ref = copy.deepcopy(net)
        f = TrainableFusedMLP(net)
        d_in = net[0].in_features
        x = torch.randn(11, d_in, requires_grad=True)
        xr = x.detach().clone().requires_grad_(True)
        # two applications on the same parameters in one graph: the gradients accumulate
        y = f(x) + 0.5 * f(2 * x)
        yr = ref(xr) + 0.5 * ref(2 * xr)
        assert torch.equal(y, yr)
        (y.square().sum() + y.sum()).backward()
        (yr.square().sum() + yr.sum()).backward()
        assert torch.equal(x.grad, xr.grad)
        for a, b in zip(net.parameters(), ref.parameters()):
            assert a.grad is not None and torch.equal(a.grad, b.grad)
        # no gradient for x unless it asks for one; none at all with grad disabled
        net.zero_grad()
        out = f(torch.randn(3, d_in))
        out.sum().backward()
        assert all(p.grad is not None for p in net.parameters())
        with torch.no_grad():
            assert not f(x).requires_grad and torch.equal(f(x), ref(x))


def test_double_backward_is_refused():
    from h12env.policy import TrainableFusedMLP

    torch.manual_seed(4)
    f = TrainableFusedMLP(seq([5, 8, 2]))
    x = torch.randn(6, 5, requires_grad=True)
    (g,) = torch.autograd.grad(f(x).square().sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_trainable_fused_mlp_validation():
    from h12env.policy import FusedMLP, TrainableFusedMLP

    mx = _learn.mlp_train_max_width()
    for bad, msg in ((nn.Linear(4, 3), "nn.Sequential"), (seq([4, 8, 3], act=nn.Tanh), "only nn.ELU"),
                     (nn.Sequential(nn.Linear(4, 8), nn.ELU(alpha=0.5), nn.Linear(8, 3)), "only nn.ELU"),
                     (nn.Sequential(nn.Linear(4, 8), nn.ELU()), "must be Linear"),
                     (nn.Sequential(nn.Linear(4, 8, bias=False)), "with bias"),
                     (seq([4, mx + 1, 3]), f"wider than {mx}"), (seq([mx + 1, 8, 3]), f"wider than {mx}"),
                     (seq([4, 8, 3]).double(), "not float32")):
        with pytest.raises(ValueError, match=msg):
            TrainableFusedMLP(bad)
    # the same networks, where FusedMLP supports the width, get the same message from FusedMLP
    with pytest.raises(ValueError, match="only nn.ELU"):
        FusedMLP([seq([4, 8, 3], act=nn.Tanh)])
    TrainableFusedMLP(seq([mx, mx, 1]))


def _toy_runner(fused, **alg):
    from h12env.ppo import OnPolicyRunner
    from isaaclab_rl.rsl_rl import RslRlOnPolicyRunnerCfg, RslRlVecEnvWrapper
    from toyenv import ToyEnv, ToyEnvCfg

    c = RslRlOnPolicyRunnerCfg(device="cpu", num_steps_per_env=16, save_interval=1000, experiment_name="toy")
    c.policy.actor_hidden_dims = [32, 32]
    c.policy.critic_hidden_dims = [32, 32]
    c.policy.init_noise_std = 0.5
    c.algorithm.num_mini_batches = 2
    c.algorithm.fused_learner = fused
    for k, v in alg.items():
        setattr(c.algorithm, k, v)
    torch.manual_seed(0)
    env = RslRlVecEnvWrapper(ToyEnv(ToyEnvCfg(scene=type(ToyEnvCfg().scene)(num_envs=64))))
    return OnPolicyRunner(env, c.to_dict(), log_dir=None, device="cpu")


def test_ppo_fused_learner_on_cpu_trains_like_the_default(monkeypatch):
    monkeypatch.delenv("H12_LEARNER_FUSED", raising=False)
    runs = []
    for fused in (True, None):
        r = _toy_runner(fused)
        assert r.alg.fused_learner is bool(fused)
        assert (r.alg.policy._fused_learner is not None) is bool(fused)
        r.learn(1)
        runs.append(r)
    a, b = runs
    assert list(a.alg.policy.state_dict()) == list(b.alg.policy.state_dict())
    for (k, p), q in zip(a.alg.policy.state_dict().items(), b.alg.policy.state_dict().values()):
        assert torch.equal(p, q), k
    assert a.last_iteration_stats["Loss/value_function"] == b.last_iteration_stats["Loss/value_function"]
    assert a.alg.learning_rate == b.alg.learning_rate
    # the environment variable is the default of the argument
    monkeypatch.setenv("H12_LEARNER_FUSED", "1")
    assert _toy_runner(None).alg.fused_learner is True
    assert _toy_runner(False).alg.fused_learner is False


def test_ppo_fused_learner_refusals():
    from h12env.ppo import PPO, ActorCritic

    mx = _learn.mlp_train_max_width()
    with pytest.raises(ValueError, match="fused_learner.*bf16"):
        PPO(ActorCritic(6, 6, 3, [8], [8]), fused_learner=True, precision="bf16")
    with pytest.raises(ValueError, match="fused_learner.*only nn.ELU"):
        PPO(ActorCritic(6, 6, 3, [8], [8], activation="tanh"), fused_learner=True)
    with pytest.raises(ValueError, match=f"fused_learner.*wider than {mx}"):
        PPO(ActorCritic(6, 6, 3, [8], [mx + 1, 8]), fused_learner=True)
    with pytest.raises(ValueError, match=f"fused_learner.*wider than {mx}"):
        PPO(ActorCritic(mx + 1, 6, 3, [8], [8]), fused_learner=True)
    PPO(ActorCritic(6, 6, 3, [8], [8], activation="tanh"))  # without the switch nothing is refused
    PPO(ActorCritic(6, 9, 3, [mx, 8], [8]), fused_learner=True)


def test_train_script_flag_and_override_set_the_switch():
    sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "scripts"))
    import train
    from isaaclab_rl.rsl_rl import RslRlOnPolicyRunnerCfg
    from isaaclab_tasks.utils.hydra import apply_overrides
    from toyenv import ToyEnvCfg

    args, _ = train.build_parser().parse_known_args(["--fused_learner"])
    agent, env = RslRlOnPolicyRunnerCfg(), ToyEnvCfg()
    assert agent.algorithm.fused_learner is None
    train.apply_cli(agent, env, args)
    assert agent.algorithm.fused_learner is True and agent.to_dict()["algorithm"]["fused_learner"] is True
    agent = RslRlOnPolicyRunnerCfg()
    train.apply_cli(agent, env, train.build_parser().parse_known_args([])[0])
    assert agent.algorithm.fused_learner is None
    apply_overrides(env, agent, ["agent.algorithm.fused_learner=true"])
    assert agent.algorithm.fused_learner is True
