"""CPU: the fused PPO loss head's surface without a GPU.  The entry points of include/h12learn.h
are declared, bound and exported and validate every argument before any HIP call; PPO(fused_loss=True) on CPU tensors
updates bit for bit like the default path (plain, with symmetry, with a privileged critic), refuses what the kernel does
not compute, and is reached by the environment variable, the train.py flag and the Hydra override."""
import ctypes as C
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "shims"))
sys.path.insert(0, str(ROOT / "tests" / "helpers"))

HEAD_NAMES = {"h12learn_ppo_head_rows", "h12learn_ppo_head_max_actions", "h12learn_ppo_head_workspace_bytes",
              "h12learn_ppo_head"}


def test_header_symbols_and_exports_name_the_head_entry_points():
    from h12env import _learn, build
    from h12env._abi import load_library

    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "h12learn.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(h12learn_[a-z_]+)\s*\(", src))
    assert HEAD_NAMES <= declared and HEAD_NAMES <= set(_learn.LEARN_SYMBOLS)
    lib = load_library()
    for n in HEAD_NAMES:
        assert hasattr(lib, n), n
    assert "h12_ppo_head.hip" in {p.name for p in build.sources()}
    assert _learn.ppo_head_max_actions() >= 32
    assert _learn.ppo_head_rows() >= 2 and _learn.ppo_head_rows() % 2 == 0


def host_args(**kw):
    """Arguments that pass every check; the pointers are host memory and are never dereferenced on the host."""
    from h12env._learn import PpoHeadArgs, learn_library

    lib = learn_library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    a = PpoHeadArgs()
    a._keep = buf
    a.m, a.B, a.n_src, a.A = 8, 8, 20, 12
    for name, kind in PpoHeadArgs._fields_:
        if kind is C.c_void_p:
            setattr(a, name, p)
    a.clip_param, a.value_loss_coef, a.entropy_coef, a.desired_kl = 0.2, 1.0, 0.01, 0.01
    a.use_clipped_value_loss = 1
    a.workspace_bytes = lib.h12learn_ppo_head_workspace_bytes(a.m, a.A)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_validation_without_gpu():
    from h12env._learn import PpoHeadArgs, learn_library

    lib = learn_library()
    mx = lib.h12learn_ppo_head_max_actions()

    def call(**kw):
        a = host_args(**kw)
        return lib.h12learn_ppo_head(C.byref(a), None), lib.h12learn_last_error()

    assert lib.h12learn_ppo_head(None, None) == -1 and b"args is null" in lib.h12learn_last_error()
    required = [n for n, kind in PpoHeadArgs._fields_ if kind is C.c_void_p and n not in ("idx", "lr", "stats_accum")]
    assert len(required) == 15
    for name in required:
        rc, err = call(**{name: None})
        assert rc == -1 and b"%s is null" % name.encode() in err, (name, err)
    rc, err = call(m=0)
    assert rc == -1 and b"m = 0" in err
    rc, err = call(m=-4)
    assert rc == -1 and b"m = -4" in err
    for m, b in ((8, 5), (10, 4), (8, 16), (8, 0)):
        rc, err = call(m=m, B=b)
        assert rc == -1 and b"m = %d is neither B nor 2 B" % m in err, (m, b, err)
    rc, err = call(A=mx + 1)
    assert rc == -1 and b"A = %d" % (mx + 1) in err
    rc, err = call(A=0)
    assert rc == -1 and b"A = 0" in err
    rc, err = call(n_src=0)
    assert rc == -1 and b"n_src = 0" in err
    rc, err = call(idx=None, n_src=7)  # without idx the first B source rows are read
    assert rc == -1 and b"n_src = 7" in err and b"without idx" in err
    rc, err = call(std_kind=2)
    assert rc == -1 and b"std_kind = 2" in err
    rc, err = call(clip_param=-0.1)
    assert rc == -1 and b"clip_param" in err
    rc, err = call(desired_kl=0.0)  # lr is set
    assert rc == -1 and b"desired_kl" in err
    need = lib.h12learn_ppo_head_workspace_bytes(8, 12)
    rc, err = call(workspace_bytes=need - 1)
    assert rc == -1 and b"workspace_bytes = %d" % (need - 1) in err
    r = lib.h12learn_ppo_head_rows()
    rc, err = call(m=r + 1, B=r + 1, workspace_bytes=need)  # two blocks need twice as much
    assert rc == -1 and b"workspace_bytes" in err
    rc, err = call(workspace=C.addressof(host_args()._keep) + 2)
    assert rc == -1 and b"aligned" in err


def test_workspace_size_is_monotone_and_steps_at_the_row_tile():
    from h12env._learn import learn_library

    lib = learn_library()
    r, mx = lib.h12learn_ppo_head_rows(), lib.h12learn_ppo_head_max_actions()
    ws = lib.h12learn_ppo_head_workspace_bytes
    for a in (1, 12, mx):
        one = ws(1, a)
        assert one >= 4 * a and one % 4 == 0  # at least d_param's partial sums
        assert ws(r - 1, a) == one and ws(r, a) == one
        assert ws(r + 1, a) == 2 * one and ws(2 * r, a) == 2 * one and ws(2 * r + 1, a) == 3 * one
        sizes = [ws(m, a) for m in range(1, 4 * r + 2)]
        assert sizes == sorted(sizes) and len(set(sizes)) == 5
        assert ws(24576, a) == one * ((24576 + r - 1) // r)
    assert ws(64, 12) < ws(64, 13)
    assert ws(0, 12) == 0 and b"m = 0" in lib.h12learn_last_error()
    assert ws(5, mx + 1) == 0 and b"A = %d" % (mx + 1) in lib.h12learn_last_error()


# ---------------------------------------------------------------------------------------------- PPO on CPU
HP = dict(num_learning_epochs=2, num_mini_batches=2, clip_param=0.2, value_loss_coef=0.7, entropy_coef=0.01,
          learning_rate=1e-3, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01,
          device="cpu")


def toy_alg(fused_loss, case, **kw):
    from h12env import symmetry as S
    from h12env.ppo import PPO, ActorCritic

    sym = None
    if case == "symmetry":
        env = SimpleNamespace(mirror_tables={
            "policy": S.MirrorTable([3, 4, 5, 0, 1, 2], [False, True, False, False, True, False]),
            "actions": S.MirrorTable([0, 2, 1], [True, False, False])})
        sym = {"use_data_augmentation": True, "use_mirror_loss": True, "mirror_loss_coeff": 0.5,
               "data_augmentation_func": "h12env.symmetry:augment", "_env": env}
    priv = case == "privileged"
    torch.manual_seed(0)
    pol = ActorCritic(6, 9 if priv else 6, 3, [16], [16], init_noise_std=0.8,
                      noise_std_type="log" if case == "log_std" else "scalar")
    alg = PPO(pol, symmetry_cfg=sym, fused_loss=fused_loss, **{**HP, **kw})
    alg.init_storage(8, 6, [6], [9] if priv else None, [3])
    return alg


def fill(alg, seed):
    g = torch.Generator().manual_seed(seed)
    for k, v in alg.storage.t.items():
        v.copy_(torch.randn(v.shape, generator=g) * (0.1 if k == "sigma" else 1.0))
    alg.storage.t["sigma"].abs_().add_(0.7)
    alg.storage.t["mu"].mul_(0.1)
    # log-probabilities near the policy's own, so ratios fall on both sides of the clip range
    alg.storage.t["actions_log_prob"].mul_(0.3).sub_(3.5)


@pytest.mark.parametrize("case", ["plain", "symmetry", "privileged", "log_std"])
def test_ppo_fused_loss_on_cpu_is_the_default_path_bit_for_bit(monkeypatch, case):
    monkeypatch.delenv("H12_PPO_HEAD_FUSED", raising=False)
    from h12env import ppo_head

    calls = []
    orig = ppo_head.torch_head  # what PPOHead evaluates on CPU tensors
    monkeypatch.setattr(ppo_head, "torch_head", lambda *a: (calls.append(1), orig(*a))[1])
    runs = []
    for fused in (True, False):
        alg = toy_alg(fused, case)
        assert alg.fused_loss is fused
        logs = []
        for u in range(2):
            fill(alg, 11 + u)
            logs.append(alg.update())
        runs.append((alg, logs))
        assert len(calls) == 8  # 2 updates x 2 epochs x 2 minibatches, all on the switched-on runner
    (a, la), (b, lb) = runs
    assert la == lb and a.learning_rate == b.learning_rate and a.learning_rate != HP["learning_rate"]
    assert ("symmetry" in la[0]) is (case == "symmetry")
    for (k, p), q in zip(a.policy.state_dict().items(), b.policy.state_dict().values()):
        assert torch.isfinite(p).all() and torch.equal(p, q), k
    sa, sb = a.optimizer.state_dict()["state"], b.optimizer.state_dict()["state"]
    for i in sa:
        assert torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"])


def test_ppo_head_on_cpu_returns_the_parts_and_refuses_a_double_backward():
    from h12env.ppo_head import HeadInputs, PPOHead, torch_head

    g = torch.Generator().manual_seed(3)
    n_src, n, a = 20, 7, 3
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    h = HeadInputs(idx=torch.randperm(n_src, generator=g)[:n], old_log_prob=r(n_src, 1) * 0.3 - 3.5,
                   advantages=r(n_src, 1), returns=r(n_src, 1), target_values=r(n_src, 1), old_mu=r(n_src, a) * 0.1,
                   old_sigma=r(n_src, a).abs() + 0.7, actions=r(n_src, a), actions_direct=False, std_kind="scalar",
                   clip_param=0.2, value_loss_coef=0.7, entropy_coef=0.01, use_clipped_value_loss=True)
    mean, value, std = r(n, a).requires_grad_(True), r(n, 1).requires_grad_(True), torch.full((a,), 0.8, requires_grad=True)
    loss, out = PPOHead.apply(mean, value, std, h)
    assert loss.requires_grad and not out.requires_grad and out.shape == (5,)
    ref = [t.detach().clone().requires_grad_(True) for t in (mean, value, std)]
    ref_loss, ref_out = torch_head(*ref, h)
    assert torch.equal(loss, ref_loss) and torch.equal(out, ref_out) and torch.equal(out[4], loss)
    assert torch.equal(out[4], out[0] + 0.7 * out[1] - 0.01 * out[2])
    loss.backward()
    ref_loss.backward()
    for t, q in zip((mean, value, std), ref):
        assert torch.equal(t.grad, q.grad)
    ones = [t.grad.clone() for t in (mean, value, std)]
    for t in (mean, value, std):
        t.grad = None
    (3.0 * PPOHead.apply(mean, value, std, h)[0]).backward()  # the saved gradients, scaled by the incoming one
    for t, q in zip((mean, value, std), ones):
        assert torch.equal(t.grad, 3.0 * q)
    mean.grad = None
    (gm,) = torch.autograd.grad(PPOHead.apply(mean, value, std, h)[0].square(), mean, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gm.sum().backward()


def test_ppo_fused_loss_refusals():
    from h12env import _learn
    from h12env.ppo import PPO, ActorCritic

    mx = _learn.ppo_head_max_actions()
    with pytest.raises(ValueError, match="fused_loss.*normalize_advantage_per_mini_batch.*two-pass"):
        PPO(ActorCritic(6, 6, 3, [8], [8]), fused_loss=True, normalize_advantage_per_mini_batch=True)
    with pytest.raises(ValueError, match=f"fused_loss.*{mx + 1} actions.*at most {mx}"):
        PPO(ActorCritic(6, 6, mx + 1, [8], [8]), fused_loss=True)
    # without the switch nothing is refused; at the maximum, and with everything else the issue lists, it is accepted
    PPO(ActorCritic(6, 6, mx + 1, [8], [8]), normalize_advantage_per_mini_batch=True)
    assert PPO(ActorCritic(6, 6, mx, [8], [8], noise_std_type="log"), fused_loss=True).fused_loss
    assert PPO(ActorCritic(6, 9, 3, [8], [8]), fused_loss=True, fused_learner=True, precision="fp32").fused_loss
    assert PPO(ActorCritic(6, 6, 3, [8], [8]), fused_loss=True, precision="bf16").fused_loss


def test_environment_variable_is_the_default_of_the_argument(monkeypatch):
    monkeypatch.delenv("H12_PPO_HEAD_FUSED", raising=False)
    assert toy_alg(None, "plain").fused_loss is False
    monkeypatch.setenv("H12_PPO_HEAD_FUSED", "1")
    assert toy_alg(None, "plain").fused_loss is True
    assert toy_alg(False, "plain").fused_loss is False
    monkeypatch.setenv("H12_PPO_HEAD_FUSED", "0")
    assert toy_alg(None, "plain").fused_loss is False and toy_alg(True, "plain").fused_loss is True


def test_train_script_flag_and_override_reach_ppo():
    sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "scripts"))
    import train
    from h12env.ppo import OnPolicyRunner
    from isaaclab_rl.rsl_rl import RslRlOnPolicyRunnerCfg, RslRlVecEnvWrapper
    from isaaclab_tasks.utils.hydra import apply_overrides
    from toyenv import ToyEnv, ToyEnvCfg

    def runner(agent):
        agent.device = "cpu"
        agent.policy.actor_hidden_dims = agent.policy.critic_hidden_dims = [16]
        env = RslRlVecEnvWrapper(ToyEnv(ToyEnvCfg(scene=type(ToyEnvCfg().scene)(num_envs=8))))
        return OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cpu")

    args, _ = train.build_parser().parse_known_args(["--fused_loss"])
    agent, env = RslRlOnPolicyRunnerCfg(), ToyEnvCfg()
    assert agent.algorithm.fused_loss is None
    train.apply_cli(agent, env, args)
    assert agent.algorithm.fused_loss is True and agent.to_dict()["algorithm"]["fused_loss"] is True
    assert agent.algorithm.fused_learner is None
    assert runner(agent).alg.fused_loss is True
    agent = RslRlOnPolicyRunnerCfg()
    train.apply_cli(agent, env, train.build_parser().parse_known_args([])[0])
    assert agent.algorithm.fused_loss is None
    apply_overrides(env, agent, ["agent.algorithm.fused_loss=true"])
    assert agent.algorithm.fused_loss is True
    r = runner(agent)
    assert r.alg.fused_loss is True
    r.learn(1)  # the runner trains with the switch on
    assert all(torch.isfinite(p).all() for p in r.alg.policy.parameters())
