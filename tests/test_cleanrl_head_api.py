"""CPU: the fused CleanRL loss head's surface without a GPU.  The entry points of
include/h12learn.h are declared, bound and exported and refuse every bad argument, naming it, before any HIP call; the
workspace formula; ``torch_cleanrl_head`` is the default path's expressions bit for bit; ``CleanRLHead`` on CPU returns
autograd's gradients; ``cleanrl.PPO(fused_loss=True)`` on the toy env is the default run bit for bit (and so the reference
fixture of tests/test_cleanrl.py at its gate); the environment variable and the train_cleanrl.py flag reach it."""
import ctypes as C
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from torch.distributions.normal import Normal

ROOT = Path(__file__).resolve().parents[1]
SHIMS = ROOT / "h1v2-isaac_amd" / "shims"
for p in (str(SHIMS), str(ROOT / "tests" / "helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

import toy_cat  # noqa: E402

HEAD_NAMES = {"h12learn_cleanrl_head_rows", "h12learn_cleanrl_head_workspace_bytes", "h12learn_cleanrl_head"}
GOLDEN = ROOT / "tests" / "golden"


def test_header_symbols_and_exports_name_the_entry_points():
    from h12env import _learn
    from h12env._abi import load_library

    text = (ROOT / "include" / "h12learn.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"\b(h12learn_[a-z_]+)\s*\(", src)
    assert HEAD_NAMES <= set(declared) and HEAD_NAMES <= set(_learn.LEARN_SYMBOLS)
    assert declared[-1] == "h12learn_cleanrl_head"  # at the end of the header
    lib = load_library()
    for n in HEAD_NAMES:
        assert hasattr(lib, n), n
    # the struct of the binding has the header's fields, in the header's order
    body = re.search(r"typedef struct h12learn_cleanrl_head_args \{(.*?)\} h12learn_cleanrl_head_args;", src, re.S).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [n for n, _ in _learn.CleanRlHeadArgs._fields_]
    assert _learn.cleanrl_head_rows() >= 2


def host_args(**kw):
    """Arguments that pass every check; the pointers are host memory and are never dereferenced on the host."""
    from h12env._learn import CleanRlHeadArgs, learn_library

    lib = learn_library()
    buf = (C.c_double * 64)()
    a = CleanRlHeadArgs()
    a._keep = buf
    a.m, a.n_src, a.A, a.norm_adv, a.clip_vloss = 8, 20, 12, 1, 1
    for name, kind in CleanRlHeadArgs._fields_:
        if kind is C.c_void_p:
            setattr(a, name, C.addressof(buf))
    a.clip_coef, a.ent_coef, a.vf_coef, a.value_eps = 0.2, 0.01, 2.0, 1e-8
    a.workspace_bytes = lib.h12learn_cleanrl_head_workspace_bytes(a.m, a.A)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_validation_without_gpu():
    from h12env._learn import CleanRlHeadArgs, learn_library

    lib = learn_library()
    mx = lib.h12learn_ppo_head_max_actions()

    def call(**kw):
        a = host_args(**kw)
        return lib.h12learn_cleanrl_head(C.byref(a), None), lib.h12learn_last_error()

    assert lib.h12learn_cleanrl_head(None, None) == -1 and b"args is null" in lib.h12learn_last_error()
    required = [n for n, kind in CleanRlHeadArgs._fields_ if kind is C.c_void_p and n not in ("idx", "stats_accum")]
    assert len(required) == 15
    for name in required:
        rc, err = call(**{name: None})
        assert rc == -1 and b"cleanrl_head: %s is null" % name.encode() in err, (name, err)
    rc, err = call(m=0)
    assert rc == -1 and b"m = 0" in err
    rc, err = call(m=-4)
    assert rc == -1 and b"m = -4" in err
    rc, err = call(m=1)
    assert rc == -1 and b"m = 1 with norm_adv" in err
    rc, err = call(A=mx + 1)
    assert rc == -1 and b"A = %d" % (mx + 1) in err
    rc, err = call(A=0)
    assert rc == -1 and b"A = 0" in err
    rc, err = call(n_src=0)
    assert rc == -1 and b"n_src = 0" in err
    rc, err = call(idx=None, n_src=7)  # without idx the first m source rows are read
    assert rc == -1 and b"n_src = 7" in err and b"without idx" in err
    need = lib.h12learn_cleanrl_head_workspace_bytes(8, 12)
    rc, err = call(workspace_bytes=need - 1)
    assert rc == -1 and b"workspace_bytes = %d" % (need - 1) in err
    r = lib.h12learn_cleanrl_head_rows()
    rc, err = call(m=r + 1, n_src=r + 1, workspace_bytes=need)  # two blocks need twice as much
    assert rc == -1 and b"workspace_bytes" in err
    rc, err = call(workspace=C.addressof(host_args()._keep) + 4)
    assert rc == -1 and b"workspace is not 8-byte aligned" in err
    rc, err = call(value_eps=-1e-8)
    assert rc == -1 and b"value_eps" in err
    rc, err = call(clip_coef=-0.1)
    assert rc == -1 and b"clip_coef" in err


def test_workspace_size_formula():
    from h12env._learn import learn_library

    lib = learn_library()
    r, mx = lib.h12learn_cleanrl_head_rows(), lib.h12learn_ppo_head_max_actions()
    ws = lib.h12learn_cleanrl_head_workspace_bytes
    for a in (1, 12, 13, mx):
        for m in (1, 2, r - 1, r, r + 1, 2 * r, 2 * r + 1, 16384, 128 * r + 1):
            # per block of R rows: (count, mean, M2) of the advantages, three summed scalars, A columns of d_logstd
            assert ws(m, a) == ((m + r - 1) // r) * (3 + 3 + a) * 8, (m, a)
    assert ws(0, 12) == 0 and b"m = 0" in lib.h12learn_last_error()
    assert ws(5, mx + 1) == 0 and b"A = %d" % (mx + 1) in lib.h12learn_last_error()


def test_depth_shapes_are_one_block_past_the_chunks():
    """The GPU test's depth shapes are computed from these two figures and the row-tile query: a change of the fold's
    chunk, of the merge's chunk or of R shows here."""
    from cleanrl_head_ref import FOLD_CHUNK, MERGE_CHUNK
    from h12env._learn import learn_library

    src = (ROOT / "h1v2-isaac_amd" / "csrc" / "h12_ppo_head.hip").read_text()
    const = lambda n: re.search(r"constexpr int %s = ([^;]+);" % n, src).group(1)  # noqa: E731
    waves = int(const("HEAD_WAVES"))
    assert int(const("FOLD_CHUNK")) == FOLD_CHUNK == 128
    assert const("MERGE_CHUNK") == "HEAD_WAVES * 64" and waves * 64 == MERGE_CHUNK
    assert int(const("HEAD_ROWS")) == learn_library().h12learn_cleanrl_head_rows() == 64
    lib = learn_library()
    r = lib.h12learn_cleanrl_head_rows()
    for chunk in (FOLD_CHUNK, MERGE_CHUNK):
        assert lib.h12learn_cleanrl_head_workspace_bytes(chunk * r + 1, 12) == (chunk + 1) * (6 + 12) * 8
        assert lib.h12learn_cleanrl_head_workspace_bytes(chunk * r, 12) == chunk * (6 + 12) * 8
    assert FOLD_CHUNK * r + 1 == 8193 and MERGE_CHUNK * r + 1 == 16385


# ---------------------------------------------------------------------------------------------- the torch expressions
def seeded_inputs(norm_adv=True, clip_vloss=True, seed=3):
    from h12env import cleanrl
    from h12env.ppo_head import CleanRLInputs

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    n_src, n, a = 40, 16, 5
    rms = cleanrl.RunningMeanStd(shape=())
    rms.running_mean.fill_(1.7), rms.running_var.fill_(2.3)
    h = CleanRLInputs(idx=torch.randperm(n_src, generator=g)[:n], old_log_prob=r(n_src) * 0.3 - 1.4 * a,
                      advantages=r(n_src) + 0.3, returns_n=r(n_src), values_n=r(n_src), actions=r(n_src, a),
                      value_rms=rms, clip_coef=0.2, ent_coef=0.0081, vf_coef=2.0, norm_adv=norm_adv,
                      clip_vloss=clip_vloss)
    mean, value, logstd = r(n, a) * 0.3, r(n, 1) * 2 + 1.7, r(1, a) * 0.1
    return h, mean, value, logstd


def inline_default_path(mean, value, logstd, h):
    """The statements of cleanrl.PPO's minibatch (and of Agent.get_action_and_value) as the default path runs them."""
    mb_inds = h.idx
    CLIP_COEF, ENT_COEF, VF_COEF = h.clip_coef, h.ent_coef, h.vf_coef
    action_logstd = logstd.expand_as(mean)
    action_std = torch.exp(action_logstd)
    probs = Normal(mean, action_std)
    newlogprob, entropy, newvalue = probs.log_prob(h.actions[mb_inds]).sum(1), probs.entropy().sum(1), value
    logratio = newlogprob - h.old_log_prob[mb_inds]
    ratio = logratio.exp()
    with torch.no_grad():
        clipfrac = ((ratio - 1.0).abs() > CLIP_COEF).float().mean()
    mb_advantages = h.advantages[mb_inds]
    if h.norm_adv:
        mb_advantages = (mb_advantages - mb_advantages.mean()) / (mb_advantages.std() + 1e-8)
    pg_loss1 = -mb_advantages * ratio
    pg_loss2 = -mb_advantages * torch.clamp(ratio, 1 - CLIP_COEF, 1 + CLIP_COEF)
    pg_loss = torch.max(pg_loss1, pg_loss2).mean()
    newvalue = h.value_rms(newvalue.view(-1), update=False)
    if h.clip_vloss:
        v_loss_unclipped = (newvalue - h.returns_n[mb_inds]) ** 2
        v_clipped = h.values_n[mb_inds] + torch.clamp(newvalue - h.values_n[mb_inds], -CLIP_COEF, CLIP_COEF)
        v_loss_clipped = (v_clipped - h.returns_n[mb_inds]) ** 2
        v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
    else:
        v_loss = 0.5 * ((newvalue - h.returns_n[mb_inds]) ** 2).mean()
    entropy_loss = entropy.mean()
    loss = pg_loss - ENT_COEF * entropy_loss + v_loss * VF_COEF
    return loss, torch.stack([pg_loss.detach(), entropy_loss.detach(), v_loss.detach(), loss.detach(), clipfrac])


@pytest.mark.parametrize("norm_adv,clip_vloss", [(True, True), (False, True), (True, False), (False, False)])
def test_torch_cleanrl_head_is_the_default_paths_expressions_bit_for_bit(norm_adv, clip_vloss):
    from h12env.ppo_head import torch_cleanrl_head

    h, *leaves = seeded_inputs(norm_adv, clip_vloss)
    a = [t.clone().requires_grad_(True) for t in leaves]
    b = [t.clone().requires_grad_(True) for t in leaves]
    la, oa = torch_cleanrl_head(*a, h)
    lb, ob = inline_default_path(*b, h)
    assert torch.equal(la, lb) and torch.equal(oa, ob) and oa.shape == (5,) and not oa.requires_grad
    assert 0.0 < float(oa[4]) < 1.0  # rows on both sides of the clip range
    la.backward()
    lb.backward()
    for x, y in zip(a, b):
        assert torch.equal(x.grad, y.grad) and bool((x.grad != 0).any())


def test_cleanrl_head_on_cpu_returns_autograds_gradients():
    from h12env.ppo_head import CleanRLHead, torch_cleanrl_head

    h, *leaves = seeded_inputs()
    mean, value, logstd = (t.clone().requires_grad_(True) for t in leaves)
    loss, out = CleanRLHead.apply(mean, value, logstd, h)
    assert loss.requires_grad and not out.requires_grad and out.shape == (5,)
    ref = [t.clone().requires_grad_(True) for t in leaves]
    ref_loss, ref_out = torch_cleanrl_head(*ref, h)
    assert torch.equal(loss, ref_loss) and torch.equal(out, ref_out) and torch.equal(out[3], loss)
    loss.backward()
    ref_loss.backward()
    for t, q in zip((mean, value, logstd), ref):
        assert t.grad.shape == t.shape and torch.equal(t.grad, q.grad)
    ones = [t.grad.clone() for t in (mean, value, logstd)]
    for t in (mean, value, logstd):
        t.grad = None
    (3.0 * CleanRLHead.apply(mean, value, logstd, h)[0]).backward()  # the saved gradients, scaled by the incoming one
    for t, q in zip((mean, value, logstd), ones):
        assert torch.equal(t.grad, 3.0 * q)
    mean.grad = None
    (gm,) = torch.autograd.grad(CleanRLHead.apply(mean, value, logstd, h)[0].square(), mean, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gm.sum().backward()


# ---------------------------------------------------------------------------------------------- the trainer on CPU
def toy_run(tmp, fused_loss, monkeypatch, **cfg):
    from h12env import cleanrl

    z = np.load(GOLDEN / "ref_cleanrl_ppo.npz")
    env = toy_cat.ToyCaTEnv({k[6:]: z[k] for k in z.files if k.startswith("table_")})
    monkeypatch.setattr(cleanrl, "layer_init", toy_cat.SeededInit())
    c = toy_cat.toy_ppo_cfg(**cfg)
    torch.manual_seed(c.seed)
    agent = cleanrl.PPO(env, c, str(tmp), fused_loss=fused_loss)
    lines = [json.loads(x) for x in (Path(tmp) / "metrics.jsonl").read_text().splitlines()]
    return agent, lines, env, z


@pytest.mark.parametrize("cfg", [{}, {"minibatch_size": 12, "norm_adv": False}, {"clip_vloss": False, "anneal_lr": False}],
                         ids=["fixture", "ragged-no_norm", "no_clip-no_anneal"])
def test_ppo_fused_loss_on_cpu_is_the_default_run_bit_for_bit(tmp_path, monkeypatch, cfg):
    monkeypatch.delenv("H12_CLEANRL_HEAD_FUSED", raising=False)
    from h12env import ppo_head

    calls = []
    orig = ppo_head.torch_cleanrl_head  # what CleanRLHead evaluates on CPU tensors
    monkeypatch.setattr(ppo_head, "torch_cleanrl_head", lambda *a: (calls.append(a[0].shape[0]), orig(*a))[1])
    fa, la, ea, z = toy_run(tmp_path / "fused", True, monkeypatch, **cfg)
    n_calls = len(calls)
    da, ld, ed, _ = toy_run(tmp_path / "default", False, monkeypatch, **cfg)
    mb = cfg.get("minibatch_size", 16)
    per_epoch = -(-32 // mb)
    assert n_calls == 2 * 2 * per_epoch and len(calls) == n_calls  # the default path never reaches the node
    assert set(calls) == ({mb, 32 % mb} - {0})
    skip = ("Perf/",)
    for x, y in zip(la, ld):
        assert {k: v for k, v in x.items() if not k.startswith(skip)} == {k: v for k, v in y.items()
                                                                        if not k.startswith(skip)}
    assert all(torch.equal(a, b) for a, b in zip(ea.actions, ed.actions))
    for (k, v), w in zip(fa.state_dict().items(), da.state_dict().values()):
        assert torch.isfinite(v).all() and torch.equal(v, w), k
    if not cfg:
        # and therefore the reference's run, at the gate of tests/test_cleanrl.py
        gate = 1e-6
        for tag, ref in zip(z["scalar_tags"], z["scalars"]):
            got = np.asarray([x[str(tag)] for x in la], dtype=np.float64)
            assert np.abs(got - ref).max() <= gate * max(np.abs(ref).max(), 1e-300), tag
        sd = {k: v.detach().numpy() for k, v in fa.state_dict().items()}
        for k in z.files:
            kind, _, name = k.partition("/")
            if kind == "sd":
                assert np.abs(sd[name] - z[k]).max() <= gate * np.abs(z[k]).max(), k


def test_environment_variable_is_the_default_of_the_argument(tmp_path, monkeypatch):
    from h12env import ppo_head

    calls = []
    orig = ppo_head.torch_cleanrl_head
    monkeypatch.setattr(ppo_head, "torch_cleanrl_head", lambda *a: (calls.append(1), orig(*a))[1])
    for i, (env, arg, reached) in enumerate([(None, None, False), ("1", None, True), ("1", False, False),
                                             ("0", None, False), ("0", True, True)]):
        if env is None:
            monkeypatch.delenv("H12_CLEANRL_HEAD_FUSED", raising=False)
        else:
            monkeypatch.setenv("H12_CLEANRL_HEAD_FUSED", env)
        del calls[:]
        toy_run(tmp_path / str(i), arg, monkeypatch, num_iterations=1)
        assert bool(calls) is reached, (env, arg)


def test_the_cfg_of_the_reference_has_no_new_field():
    from h12env import cleanrl

    assert "fused_loss" not in {f.name for f in cleanrl.dataclasses.fields(cleanrl.CleanRlPpoActorCriticCfg)}


PRELUDE = r"""
import sys
sys.path[:0] = [{shims!r}, {pkg!r}, {helpers!r}, {scripts!r}]
import gymnasium as gym
import toy_cat
from h12env import ppo_head
orig = ppo_head.torch_cleanrl_head
def counted(*a):
    print("HEAD", a[0].shape[0], flush=True)
    return orig(*a)
ppo_head.torch_cleanrl_head = counted
def toy_agent():
    from biped_tasks.tasks.agents import H12_12dof_FlatCleanRlPPOCfg
    return H12_12dof_FlatCleanRlPPOCfg(num_steps=4, num_iterations=3, minibatch_size=16, updates_epochs=2,
                                       save_interval=2, experiment_name="toy_cat")
gym.register(id="Toy-CaT-v0", entry_point="toy_cat:ToyCaTEnv",
             kwargs={{"env_cfg_entry_point": "h12env.cfg:H12CaTEnvCfg", "clean_rl_cfg_entry_point": toy_agent}})
import train_cleanrl
sys.exit(train_cleanrl.main(sys.argv[1:]))
"""


def test_train_script_flag_reaches_ppo(tmp_path):
    scripts = ROOT / "h1v2-isaac_amd" / "scripts"
    prelude = PRELUDE.format(shims=str(SHIMS), pkg=str(ROOT / "h1v2-isaac_amd"), helpers=str(ROOT / "tests" / "helpers"),
                             scripts=str(scripts))
    cmd = [sys.executable, "-c", prelude, "--task", "Toy-CaT-v0", "--headless", "--device", "cpu", "--num_envs", "8",
           "--seed", "5", "--num_iterations", "2", "--fused_loss"]
    env = {k: v for k, v in __import__("os").environ.items() if k != "H12_CLEANRL_HEAD_FUSED"}
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("HEAD 16") == 2 * 2 * 2  # iterations x epochs x minibatches
    run = next((tmp_path / "logs" / "clean_rl" / "toy_cat").iterdir())
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    assert [x["iter"] for x in lines] == [1, 2]
    assert all(np.isfinite(v) for x in lines for v in x.values())
    sd = torch.load(run / "model_1.pt", weights_only=True)
    assert "actor_logstd" in sd and "value_rms.running_var" in sd
