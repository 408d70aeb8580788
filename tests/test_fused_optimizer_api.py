"""CPU: the fused optimiser step's surface without a GPU.  The entry points of include/h12learn.h
are declared, bound and exported and refuse every bad argument, naming it, before any HIP call; the workspace formula;
``FusedClipAdam`` / ``FusedClipRAdam`` on CPU tensors are clip_grad_norm_ + torch's classes bit for bit, state included, and
their state_dicts interchange with torch's both ways; the refusals; ``cleanrl.PPO(fused_optimizer=True)`` on the toy env is
the default run bit for bit; the environment variable and both train scripts' flags reach the switch."""
import ctypes as C
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
SHIMS = ROOT / "h1v2-isaac_amd" / "shims"
SCRIPTS = ROOT / "h1v2-isaac_amd" / "scripts"
for p in (str(SHIMS), str(ROOT / "tests" / "helpers"), str(SCRIPTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

import optim_ref as R  # noqa: E402
import toy_cat  # noqa: E402
from h12env import optim as O  # noqa: E402

NAMES = ["h12learn_optim_chunk", "h12learn_optim_max_tensors", "h12learn_optim_fold", "h12learn_optim_workspace_bytes",
         "h12learn_optim_step"]
GOLDEN = ROOT / "tests" / "golden"


def test_header_binding_export_and_build_agree():
    from h12env import _learn, build
    from h12env._abi import load_library

    text = (ROOT / "include" / "h12learn.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"\b(h12learn_[a-z_]+)\s*\(", src)
    assert [n for n in declared if "_optim_" in n] == NAMES and set(NAMES) <= set(_learn.LEARN_SYMBOLS)
    # ahead of the PPO loss-head section, after the RND section
    assert declared.index("h12learn_rnd_finish") < declared.index(NAMES[0])
    assert declared.index(NAMES[-1]) < declared.index("h12learn_ppo_head_rows")
    lib = load_library()
    for n in NAMES:
        assert hasattr(lib, n), n
    body = re.search(r"typedef struct h12learn_optim_args \{(.*?)\} h12learn_optim_args;", src, re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in _learn.OptimArgs._fields_]
    rules = dict(re.findall(r"#define (H12LEARN_OPTIM_[A-Z]+) (\d+)", src))
    assert rules == {"H12LEARN_OPTIM_ADAM": str(_learn.OPTIM_ADAM), "H12LEARN_OPTIM_RADAM": str(_learn.OPTIM_RADAM)}
    assert build.CSRC / "h12_optim.hip" in build.UNITS
    assert {"h12_optim.hip", "h12learn.h"} <= {p.name for p in build.sources()}
    assert lib.h12env_abi_version() == 9
    assert _learn.optim_chunk() >= 8 and _learn.optim_chunk() % 4 == 0
    assert _learn.optim_max_tensors() >= 17 and _learn.optim_fold() >= 1  # a trainer's 17 tensors take one launch


class HostArgs:
    """Arguments that pass every check; the pointers are host memory and are never dereferenced on the host."""

    def __init__(self, n=3, numel=(5, 4096, 1), **kw):
        from h12env._learn import OptimArgs, learn_library

        self.lib = learn_library()
        self.buf = (C.c_double * 64)()
        base = C.addressof(self.buf)
        a = self.a = OptimArgs()
        a.rule, a.n_tensors = 1, n
        a.beta1, a.beta2, a.eps, a.max_norm, a.lr = 0.9, 0.999, 1e-8, 1.0, 1e-3
        self.tables = {}
        for name in ("p", "g", "exp_avg", "exp_avg_sq", "step"):
            self.tables[name] = (C.c_void_p * max(n, 1))(*([base] * max(n, 1)))
            setattr(a, name, self.tables[name])
        self.numel = (C.c_longlong * max(n, 1))(*numel[:max(n, 1)])
        a.numel = self.numel
        a.grad_norm = a.workspace = base
        a.workspace_bytes = self.lib.h12learn_optim_workspace_bytes(self.numel, n) if n >= 1 else 64
        for k, v in kw.items():
            setattr(a, k, v)

    def call(self):
        return self.lib.h12learn_optim_step(C.byref(self.a), None), self.lib.h12learn_last_error()


def test_argument_validation_without_gpu():
    from h12env._learn import learn_library

    lib = learn_library()
    assert lib.h12learn_optim_step(None, None) == -1 and b"args is null" in lib.h12learn_last_error()

    def refused(what, **kw):
        rc, err = HostArgs(**kw).call()
        assert rc == -1 and what in err, (what, err)

    refused(b"rule = 2", rule=2)
    refused(b"rule = -1", rule=-1)
    for name in ("beta1", "beta2"):
        for bad in (1.0, -0.1, 1.5, float("nan")):
            refused(name.encode(), **{name: bad})
    for bad in (0.0, -1e-8, float("nan"), float("inf")):
        refused(b"eps", eps=bad)
    refused(b"max_norm", max_norm=float("nan"))
    refused(b"lr = -0.001", lr=-1e-3)
    refused(b"n_tensors = 0", n=0)
    refused(b"n_tensors = -2", n_tensors=-2)
    for name in ("p", "g", "exp_avg", "exp_avg_sq", "step", "numel"):
        h = HostArgs()
        setattr(h.a, name, None)
        rc, err = h.call()
        assert rc == -1 and b"optim_step: %s is null" % name.encode() in err, (name, err)
    for name in ("p", "g", "exp_avg", "exp_avg_sq", "step"):  # a null or misaligned table entry, named with its index
        h = HostArgs()
        h.tables[name][1] = None
        rc, err = h.call()
        assert rc == -1 and b"%s[1] is null" % name.encode() in err, (name, err)
        h = HostArgs()
        h.tables[name][2] = C.addressof(h.buf) + 2
        rc, err = h.call()
        assert rc == -1 and b"%s[2] not 4-byte aligned" % name.encode() in err, (name, err)
    refused(b"numel[1] = 0", numel=(5, 0, 1))
    refused(b"numel[2] = -3", numel=(5, 7, -3))
    refused(b"workspace is null", workspace=None)
    need = HostArgs().a.workspace_bytes
    refused(b"workspace_bytes = %d" % (need - 1), workspace_bytes=need - 1)
    h = HostArgs()
    h.a.workspace = C.addressof(h.buf) + 4
    rc, err = h.call()
    assert rc == -1 and b"workspace not 8-byte aligned" in err
    h = HostArgs()
    h.a.lr_dev = C.addressof(h.buf) + 1
    rc, err = h.call()
    assert rc == -1 and b"lr_dev" in err
    h = HostArgs()
    h.a.grad_norm = C.addressof(h.buf) + 2
    rc, err = h.call()
    assert rc == -1 and b"grad_norm" in err


def test_workspace_size_formula():
    from h12env import _learn

    c = _learn.optim_chunk()
    for sizes in ([1], [3], [c - 1, c, c + 1], [2 * c + 1, 1, 12, 5], [7] * (_learn.optim_max_tensors() + 1),
                  [c * _learn.optim_fold() + 1]):
        assert _learn.optim_workspace_bytes(sizes) == 8 * sum(-(-n // c) for n in sizes), sizes
    lib = _learn.learn_library()
    assert lib.h12learn_optim_workspace_bytes(None, 1) == 0 and b"numel is null" in lib.h12learn_last_error()
    arr = (C.c_longlong * 2)(4, 0)
    assert lib.h12learn_optim_workspace_bytes(arr, 2) == 0 and b"numel[1] = 0" in lib.h12learn_last_error()
    assert lib.h12learn_optim_workspace_bytes(arr, 0) == 0 and b"n_tensors = 0" in lib.h12learn_last_error()


# ---------------------------------------------------------------------------------------------- the classes on CPU
def fused_class(rule):
    return {"adam": O.FusedClipAdam, "radam": O.FusedClipRAdam}[rule]


def recurrent_policy():
    from h12env.ppo import ActorCriticRecurrent

    torch.manual_seed(3)
    return ActorCriticRecurrent(10, 10, 4, [16, 8], [16, 8], rnn_hidden_dim=8)


def train_both(rule, params, max_norm, steps=R.STEPS, lr=R.LR):
    """The same seeded gradients through the fused class and through clip_grad_norm_ + torch's class."""
    a = [torch.nn.Parameter(p.detach().clone()) for p in params]
    b = [torch.nn.Parameter(p.detach().clone()) for p in params]
    kw = R.rule_kwargs(rule)
    fused = fused_class(rule)(a, lr=lr, max_norm=max_norm, **kw)
    ref = R.torch_class(rule)(b, lr=lr, **kw)
    g = torch.Generator().manual_seed(17)
    for s in range(steps):
        for p, q in zip(a, b):
            p.grad = torch.randn(p.shape, generator=g) * R.SCALES[s % 2]
            q.grad = p.grad.clone()
        a[-1].grad = b[-1].grad = None  # a parameter without a gradient is left out, as torch leaves it out
        fused.step()
        if max_norm is not None:
            want = torch.nn.utils.clip_grad_norm_(b, max_norm)
            assert torch.equal(fused.last_grad_norm, want)
        ref.step()
    return a, b, fused, ref


@pytest.mark.parametrize("rule", ["adam", "radam"])
@pytest.mark.parametrize("max_norm", [1.0, None])
@pytest.mark.parametrize("net", ["tensors", "recurrent"])
def test_cpu_step_is_torchs_bit_for_bit(rule, max_norm, net):
    if net == "recurrent":
        params = list(recurrent_policy().parameters())
        assert any("LSTM" in type(m).__name__ for m in recurrent_policy().modules())
    else:
        params = R.make_case([5, 1, 33, 7], seed=2).params
    a, b, fused, ref = train_both(rule, params, max_norm)
    for p, q in zip(a, b):
        assert torch.equal(p, q) and torch.isfinite(p).all()
        sp, sq = fused.state[p], ref.state[q]
        assert set(sp) == set(sq)
        for k in sq:
            assert torch.equal(sp[k], sq[k]) and sp[k].dtype == sq[k].dtype and sp[k].shape == sq[k].shape, k
    assert not any(torch.equal(p, q) for p, q in zip(a[:-1], params[:-1]))  # they moved
    assert torch.equal(a[-1], params[-1]) and len(fused.state[a[-1]]) == 0   # no gradient: no state, no step
    assert float(fused.state[a[0]]["step"]) == R.STEPS


@pytest.mark.parametrize("rule", ["adam", "radam"])
def test_state_dict_round_trips_with_torchs_class_both_ways(rule):
    params = R.make_case([5, 9], seed=4).params
    a, b, fused, ref = train_both(rule, params + [torch.zeros(2)], 1.0, steps=3)
    # fused -> torch, torch -> fused: each continues the other's run bit for bit
    a2 = [torch.nn.Parameter(p.detach().clone()) for p in a]
    b2 = [torch.nn.Parameter(p.detach().clone()) for p in a]
    kw = R.rule_kwargs(rule)
    into_torch = R.torch_class(rule)(b2, lr=0.5, **kw)
    into_torch.load_state_dict(fused.state_dict())
    into_fused = fused_class(rule)(a2, lr=0.5, max_norm=1.0, **kw)
    into_fused.load_state_dict(ref.state_dict())
    assert into_fused.max_norm == 1.0 and into_fused.param_groups[0]["lr"] == R.LR == into_torch.param_groups[0]["lr"]
    assert set(into_fused.param_groups[0]) == set(into_torch.param_groups[0]) == set(ref.param_groups[0])
    g = torch.Generator().manual_seed(5)
    for s in range(3):
        for p, q in zip(a2, b2):
            p.grad = torch.randn(p.shape, generator=g) * R.SCALES[s % 2]
            q.grad = p.grad.clone()
        into_fused.step()
        torch.nn.utils.clip_grad_norm_(b2, 1.0)
        into_torch.step()
    for i, (p, q) in enumerate(zip(a2, b2)):
        assert torch.equal(p, q)
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(into_fused.state[p][k], into_torch.state[q][k])
        # the last parameter had no gradient before the hand-over: its state starts after it
        assert float(into_fused.state[p]["step"]) == (6 if i < 2 else 3)
        assert into_fused.state[p]["step"].dtype == torch.float32
    sd = into_fused.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and "max_norm" not in sd["param_groups"][0]


def test_every_refusal_names_the_offender():
    p = torch.nn.Parameter(torch.zeros(4))
    for cls in (O.FusedClipAdam, O.FusedClipRAdam):
        with pytest.raises(ValueError, match="weight_decay"):
            cls([p], weight_decay=0.1)
        with pytest.raises(ValueError, match="maximize"):
            cls([p], maximize=True)
        with pytest.raises(ValueError, match="max_norm"):
            cls([p], max_norm=0.0)
        with pytest.raises(ValueError, match="betas"):
            cls([p], betas=(0.9, 1.0))
        with pytest.raises(ValueError, match="eps"):
            cls([p], eps=0.0)
        q = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
        q.grad = torch.zeros(4, dtype=torch.float64)
        with pytest.raises(ValueError, match=r"parameter 0 of group 0 \(4,\) is torch.float64"):
            cls([q]).step()
        q = torch.nn.Parameter(torch.zeros(4, 6).t())
        q.grad = torch.zeros(6, 4)
        with pytest.raises(ValueError, match=r"parameter 0 of group 0 \(6, 4\) is not contiguous"):
            cls([q]).step()
        q = torch.nn.Parameter(torch.zeros(6, 4))
        q.grad = torch.zeros(4, 6).t()
        with pytest.raises(ValueError, match=r"the gradient of parameter 0 of group 0 \(6, 4\) is not contiguous"):
            cls([q]).step()
        opt = cls([{"params": [p]}, {"params": [torch.nn.Parameter(torch.zeros(2))], "lr": 0.5}])
        p.grad = torch.zeros(4)
        with pytest.raises(ValueError, match="param group 1"):
            opt.step()
    with pytest.raises(ValueError, match="amsgrad"):
        O.FusedClipAdam([p], amsgrad=True)
    opt = O.FusedClipAdam([p])
    opt.param_groups[0]["weight_decay"] = 0.01  # set after construction, as a loaded state_dict may
    with pytest.raises(ValueError, match="weight_decay"):
        opt.step()


# ---------------------------------------------------------------------------------------------- the trainers on CPU
def toy_run(tmp, fused_optimizer, monkeypatch, fused_loss=False, **cfg):
    from h12env import cleanrl

    z = np.load(GOLDEN / "ref_cleanrl_ppo.npz")
    env = toy_cat.ToyCaTEnv({k[6:]: z[k] for k in z.files if k.startswith("table_")})
    monkeypatch.setattr(cleanrl, "layer_init", toy_cat.SeededInit())
    c = toy_cat.toy_ppo_cfg(**cfg)
    torch.manual_seed(c.seed)
    agent = cleanrl.PPO(env, c, str(tmp), fused_loss=fused_loss, fused_optimizer=fused_optimizer)
    lines = [json.loads(x) for x in (Path(tmp) / "metrics.jsonl").read_text().splitlines()]
    return agent, lines, env


def count_steps(monkeypatch):
    calls = []
    orig = O.FusedClipRAdam.step
    monkeypatch.setattr(O.FusedClipRAdam, "step", lambda self, *a: (calls.append(self.max_norm), orig(self, *a))[1])
    return calls


@pytest.mark.parametrize("fused_loss", [False, True], ids=["default_path", "fused_loss"])
def test_cleanrl_ppo_fused_optimizer_on_cpu_is_the_default_run_bit_for_bit(tmp_path, monkeypatch, fused_loss):
    monkeypatch.delenv("H12_OPTIMIZER_FUSED", raising=False)
    calls = count_steps(monkeypatch)
    fa, la, ea = toy_run(tmp_path / "fused", True, monkeypatch, fused_loss)
    n_calls = len(calls)
    da, ld, ed = toy_run(tmp_path / "default", False, monkeypatch, fused_loss)
    assert n_calls == 2 * 2 * 2 and len(calls) == n_calls  # iterations x epochs x minibatches; never on the default run
    assert set(calls) == {toy_cat.toy_ppo_cfg().max_grad_norm}
    for x, y in zip(la, ld):
        assert {k: v for k, v in x.items() if not k.startswith("Perf/")} == {k: v for k, v in y.items()
                                                                            if not k.startswith("Perf/")}
    assert la[0]["Loss/learning_rate"] != la[1]["Loss/learning_rate"]  # the annealed host lr reaches the step
    assert all(torch.equal(a, b) for a, b in zip(ea.actions, ed.actions))
    for (k, v), w in zip(fa.state_dict().items(), da.state_dict().values()):
        assert torch.isfinite(v).all() and torch.equal(v, w), k


def test_environment_variable_is_the_default_of_both_arguments(tmp_path, monkeypatch):
    from h12env import ppo

    calls = count_steps(monkeypatch)
    seen = []
    orig = ppo.PPO._init_optimizer
    monkeypatch.setattr(ppo.PPO, "_init_optimizer", lambda self, lr, f=False: (seen.append(bool(f)), orig(self, lr, f))[1])
    for i, (env, arg, reached) in enumerate([(None, None, False), ("1", None, True), ("1", False, False),
                                             ("0", None, False), ("0", True, True)]):
        if env is None:
            monkeypatch.delenv("H12_OPTIMIZER_FUSED", raising=False)
        else:
            monkeypatch.setenv("H12_OPTIMIZER_FUSED", env)
        del calls[:], seen[:]
        toy_run(tmp_path / str(i), arg, monkeypatch, num_iterations=1)
        assert bool(calls) is reached, (env, arg)
        alg = ppo.PPO(ppo.ActorCritic(6, 6, 2, [8], [8]), device="cpu", fused_optimizer=arg)
        assert seen == [reached], (env, arg)
        # the HIP step is the GPU's: on CPU the runner keeps torch's clip and Adam
        assert alg.fused_optimizer is False and type(alg.optimizer) is torch.optim.Adam


def test_more_than_one_rank_is_refused():
    from h12env import distributed as D
    from h12env import ppo

    pol = ppo.ActorCritic(6, 6, 2, [8], [8])
    with pytest.raises(ValueError, match="fused_optimizer with more than one rank"):
        ppo.PPO(pol, device="cpu", fused_optimizer=True, shard=D.Shard(0, 2, 0, 0))
    ppo.PPO(pol, device="cpu", fused_optimizer=False, shard=D.Shard(0, 2, 0, 0))


def test_train_script_flag_and_override_reach_the_algorithm_cfg():
    import biped_tasks.tasks  # noqa: F401
    import train
    from isaaclab_tasks.utils.hydra import apply_overrides
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    task = "Isaac-Velocity-Flat-H12_12dof-v0"
    for argv, want in ((["--fused_optimizer"], True), (["agent.algorithm.fused_optimizer=true"], True), ([], None)):
        args, hydra_args = train.build_parser().parse_known_args(["--task", task, "--headless"] + argv)
        env_cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
        agent_cfg = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
        apply_overrides(env_cfg, agent_cfg, hydra_args)
        train.apply_cli(agent_cfg, env_cfg, args)
        assert agent_cfg.to_dict()["algorithm"]["fused_optimizer"] is want, argv
    args, _ = train.build_parser().parse_known_args(["--task", task, "--distill", "--fused_optimizer",
                                                     "--teacher_checkpoint", "x.pt"])
    with pytest.raises(SystemExit, match="--distill does not take --fused_optimizer"):
        train.make_distillation(agent_cfg, env_cfg, args)


def test_train_cleanrl_script_flag_reaches_ppo(tmp_path, monkeypatch):
    import biped_tasks.utils.cleanrl.ppo as shim
    import gymnasium as gym
    import train_cleanrl

    def toy_agent():
        from biped_tasks.tasks.agents import H12_12dof_FlatCleanRlPPOCfg
        return H12_12dof_FlatCleanRlPPOCfg(num_steps=4, num_iterations=1, minibatch_size=16, updates_epochs=1,
                                           save_interval=2, experiment_name="toy_cat_optim")

    gym.register(id="Toy-CaT-Optim-v0", entry_point="toy_cat:ToyCaTEnv",
                 kwargs={"env_cfg_entry_point": "h12env.cfg:H12CaTEnvCfg", "clean_rl_cfg_entry_point": toy_agent})
    seen = []
    monkeypatch.setattr(shim, "PPO", lambda *a, **k: seen.append(k))
    monkeypatch.chdir(tmp_path)
    base = ["--task", "Toy-CaT-Optim-v0", "--headless", "--device", "cpu", "--num_envs", "8"]
    assert train_cleanrl.main(base + ["--fused_optimizer"]) == 0
    assert train_cleanrl.main(base) == 0
    assert [k["fused_optimizer"] for k in seen] == [True, None] and [k["fused_loss"] for k in seen] == [None, None]
