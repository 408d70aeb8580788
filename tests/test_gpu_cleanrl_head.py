"""GPU: the fused CleanRL loss head (h12learn_cleanrl_head, csrc/h12_ppo_head.hip; h12env.ppo_head.CleanRLHead;
cleanrl.PPO(fused_loss=True)).  DESIGN.md section 7o.  u = 2^-24, R = the row tile.

Gate 1  against fp64: the header's expressions restated in float64 on a double copy of the fp32 inputs and differentiated
        by torch autograd (tests/helpers/cleanrl_head_ref.py).  Per output tensor (out, d_mean, d_value, d_logstd) the
        kernel's worst elementwise error is at most FACTOR x the worst error of the same restatement evaluated by torch in
        fp32 on the device + u max|ref|.  Exact ties and boundaries are kept out of these data and tested on their own
        against torch autograd on the same fp32 inputs.
Gate 2  bitwise: run to run; index clamping; the statistics accumulator; a captured call follows in-place changes of mean,
        idx and the value statistics; one workspace for several m, never zeroed; the autograd node.
Gate 3  the trainer on the CaT task at 64 envs x 24 steps (minibatches of 384 rows, and of 500 for the ragged capture):
        graphed == eager bit for bit with the switch on; the kernel is reached the expected number of times; the default
        path never reaches it; one minibatch's gradients against the loss restated in fp64; the two paths' first logged
        losses; a fused run's checkpoint in a default run.
"""
import copy
import json
import math
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
SHIMS = ROOT / "h1v2-isaac_amd" / "shims"
for p in (str(SHIMS), str(ROOT / "tests" / "helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

from cleanrl_head_ref import FOLD_CHUNK, MERGE_CHUNK, make_case, restated  # noqa: E402
from h12env import _learn, cleanrl  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FACTOR = 2.0  # the smallest power of two above the worst measured ratio (1.78, d_logstd of a 63-row case)
DEV = "cuda:0"
PER_ROW = ("old_log_prob", "advantages", "returns_n", "values_n", "actions")
NAMES = ("out", "d_mean", "d_value", "d_logstd")


def tile():
    return _learn.cleanrl_head_rows()


def run_kernel(c, t=None, idx="case", stats=None, ws=None):
    """The entry point called directly on c's tensors (or the device copies ``t``)."""
    t = t or {n: v.to(DEV) for n, v in c.t.items()}
    if isinstance(idx, str):
        idx = None if c.idx is None else c.idx.to(DEV)
    d_mean, d_value, d_logstd, out = _learn.cleanrl_head(
        t["mean"], t["value"], t["logstd"], idx, *(t[n] for n in PER_ROW), t["value_mean"], t["value_var"], c.veps,
        c.clip, c.ecoef, c.vcoef, c.norm_adv, c.clip_vloss, stats_accum=stats, workspace=ws)
    return SimpleNamespace(out=out, d_mean=d_mean, d_value=d_value, d_logstd=d_logstd)


def flat(o):
    return [getattr(o, n) for n in NAMES]


def assert_every_branch_is_populated(c, ref):
    lo, hi = 1.0 - c.clip, 1.0 + c.clip
    for side in (ref.ratio < lo, (ref.ratio > lo) & (ref.ratio < hi), ref.ratio > hi):
        assert bool((side & (ref.adv > 0)).any()) and bool((side & (ref.adv < 0)).any()), (c.m, c.A)
    assert bool((ref.dv < -c.clip).any()) and bool((ref.dv.abs() < c.clip).any()) and bool((ref.dv > c.clip).any())
    assert bool((ref.q1 > ref.q2).any()) and bool((ref.q2 > ref.q1).any())
    assert 0.0 < float(ref.clip_rows.mean()) < 1.0
    # no planted tie or boundary here: those have a test of their own
    assert not bool((ref.ratio == lo).any() | (ref.ratio == hi).any() | (ref.dv.abs() == c.clip).any())
    assert not bool((ref.adv == 0).any())


# ---------------------------------------------------------------------------------------------- gate 1
def gate1_cases():
    """Shapes as expressions of the row tile R and the two staging chunks (resolved when the test runs)."""
    cases = [dict(m=m, A=12) for m in ("2", "R-1", "R", "R+1", "2R+1")]
    cases += [dict(m="R+1", A=a) for a in (1, 13, 32)]
    cases += [dict(m="2R+1", A=32, use_idx=False), dict(m="R+1", A=12, use_idx=False), dict(m="2", A=1, use_idx=False)]
    cases += [dict(m="2R+1", A=12, norm_adv=False), dict(m="R-1", A=13, norm_adv=False, use_idx=False),
              dict(m="R+1", A=12, clip_vloss=False), dict(m="R", A=1, clip_vloss=False, norm_adv=False),
              dict(m="2", A=12, norm_adv=False, clip_vloss=False)]
    cases += [dict(m="2R+1", A=12, adv_shift=100.0), dict(m="R+1", A=13, adv_shift=100.0, use_idx=False)]
    # the depth shapes: one block more than the fold stages at a time, and than a row block merges at a time
    cases += [dict(m="FOLD+1", A=12), dict(m="MERGE+1", A=12, adv_shift=100.0)]
    return cases


def resolve(spec):
    r = tile()
    rows = {"2": 2, "R-1": r - 1, "R": r, "R+1": r + 1, "2R+1": 2 * r + 1, "FOLD+1": FOLD_CHUNK * r + 1,
            "MERGE+1": MERGE_CHUNK * r + 1}[spec["m"]]
    return dict(spec, m=rows)


def case_id(spec):
    return "-".join(f"{k}={v}" for k, v in spec.items())


def errors(c):
    """Per output tensor: (kernel's worst error, fp32 torch's worst error, max|ref|) against the fp64 restatement."""
    ref = restated(c, torch.float64, DEV)
    t32 = restated(c, torch.float32, DEV)
    got = run_kernel(c)
    rows = {}
    for name in NAMES:
        r = getattr(ref, name)
        rows[name] = (float((getattr(got, name).double() - r).abs().max()),
                      float((getattr(t32, name).double() - r).abs().max()), float(r.abs().max()))
    for i, name in enumerate(("pg", "entropy", "v", "loss", "clipfrac")):  # printed, not gated one by one
        r = ref.out[i]
        print(f"OUT {name}: kernel {float((got.out[i].double() - r).abs()):.3e} "
              f"torch32 {float((t32.out[i].double() - r).abs()):.3e} ref {float(r):.6e}")
    return ref, rows


@pytest.mark.parametrize("spec", gate1_cases(), ids=case_id)
def test_outputs_and_gradients_against_fp64(gpu, spec):
    c = make_case(seed=3, **resolve(spec))
    ref, rows = errors(c)
    if c.m >= tile() - 1 and c.clip_vloss:
        assert_every_branch_is_populated(c, ref)
    if spec["m"] in ("FOLD+1", "MERGE+1"):
        n_blocks = (c.m + tile() - 1) // tile()
        assert n_blocks == {"FOLD+1": FOLD_CHUNK, "MERGE+1": MERGE_CHUNK}[spec["m"]] + 1
        assert _learn.learn_library().h12learn_cleanrl_head_workspace_bytes(c.m, c.A) == n_blocks * (6 + c.A) * 8
    for name, (ek, et, scale) in rows.items():
        ratio = max(0.0, ek - U * scale) / et if et > 0 else (0.0 if ek <= U * scale else math.inf)
        print(f"GATE1 {case_id(spec)} {name}: kernel {ek:.3e} torch32 {et:.3e} max|ref| {scale:.3e} ratio {ratio:.2f}")
    for name, (ek, et, scale) in rows.items():
        assert ek <= FACTOR * et + U * scale, (name, ek, et, scale)


def test_a_one_pass_variance_could_not_hide(gpu):
    """The advantages 100 + N(0, 1): E[x^2] - mean^2 in fp32 loses about 1e4 u = 6e-4 of the variance, 3e-4 of the
    standard deviation, which every normalised advantage, and d_mean through it, would carry.  What the expression itself
    costs is the mean narrowed to fp32, at most ulp(100) / 2 = 3.8e-6 on a normalised advantage of order 1.  The bound
    lies between the two: 5e-5 of d_mean's largest element."""
    c = make_case(m=2 * tile() + 1, A=12, adv_shift=100.0, seed=4)
    ref, got = restated(c, torch.float64, DEV), run_kernel(c)
    k = c.k.to(DEV)
    assert 99.0 < float(c.t["advantages"].to(DEV)[k].mean()) < 101.0
    err = float((got.d_mean.double() - ref.d_mean).abs().max() / ref.d_mean.abs().max())
    print(f"shifted advantages: d_mean's error relative to its largest element {err:.3e}")
    assert err <= 5e-5


# ---------------------------------------------------------------------------------------------- ties and boundaries
def tie_case(clip):
    """A = 1, sigma = 1 (logstd = 0): a row's log-probability is the same single rounded expression in torch and in the
    kernel, so old_log_prob = log_prob plants ratio == 1 exactly.  value_rms has mean 0.5, variance 4 and epsilon 0, so
    nv = (value - 0.5) / 2 is exact for the planted values.  clip = 0: ratio == 1 sits on both ends of the clip range (and
    is no clip row: the comparison is strict) and nv == values_n on both ends of the value clip.  clip = 0.25: nv - values_n
    == +-clip, a tie of the two value operands outside the range, and advantages of exactly zero (norm_adv off)."""
    n = 12
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    mean, actions = rn(n, 1), rn(n, 1)
    lp = -((actions - mean) ** 2) / 2.0 - 0.0 - math.log(math.sqrt(2 * math.pi))
    old_log_prob = lp.squeeze(-1).clone()
    adv = rn(n)
    vn = rn(n)
    nv = vn + 0.5 * rn(n)
    ret = vn + 0.5 * rn(n)
    special = torch.zeros(n, dtype=torch.bool)
    if clip == 0.0:
        old_log_prob[6:9] += 0.3     # ratio below 1
        old_log_prob[9:] -= 0.3      # ratio above 1; rows 0..5 have ratio == 1 exactly
        vn[0:3] = torch.tensor([0.25, -0.5, 1.0])
        nv[0:3] = vn[0:3]            # nv - values_n == 0 == +-clip
        special[:6] = True
    else:
        old_log_prob[0:6] += torch.tensor([0.1, -0.1, 0.5, -0.5, 0.5, -0.5])
        adv[4:6] = 0.0               # outside the range with s1 == s2 == 0
        vn[0:4] = torch.tensor([0.0, 0.0, 0.5, -2.0])
        nv[0:4] = vn[0:4] + torch.tensor([0.25, -0.25, 0.25, -0.25])   # on the value clip's ends
        vn[6], nv[6], ret[6] = 0.0, 1.0, 0.625                         # e1 = 0.375 = -e2 outside the range
        vn[7], nv[7], ret[7] = 1.0, 0.0, 0.375                         # the same from below
        special[:8] = True
    value = 2.0 * nv + 0.5
    t = dict(mean=mean, value=value, logstd=torch.zeros(1), old_log_prob=old_log_prob, advantages=adv, returns_n=ret,
             values_n=vn, actions=actions, value_mean=torch.tensor(0.5), value_var=torch.tensor(4.0))
    c = SimpleNamespace(m=n, A=1, n_src=n, idx=None, k=torch.arange(n), norm_adv=False, clip_vloss=True, clip=clip,
                        ecoef=0.0081, vcoef=2.0, veps=0.0, t=t)
    return c, special


@pytest.mark.parametrize("clip", [0.0, 0.25])
def test_ties_and_boundaries_get_the_gradient_torch_autograd_gives(gpu, clip):
    c, special = tie_case(clip)
    t32 = restated(c, torch.float32, DEV)
    got = run_kernel(c)
    n = c.m
    adv, d = c.t["advantages"].to(DEV), (c.t["actions"] - c.t["mean"]).to(DEV).squeeze(-1)
    e1 = ((c.t["value"] - 0.5) / 2.0 - c.t["returns_n"]).to(DEV)
    half = c.vcoef * 0.5 / 2.0  # vf_coef x the 0.5 of the value loss / sqrt(value_var)
    if clip == 0.0:
        assert bool((t32.ratio[:6] == 1.0).all()) and bool((t32.ratio[6:] != 1.0).all())
        # strict: ratio == 1 with clip_coef == 0 is no clip row; the six other rows are
        assert float(t32.out[4]) == 0.5 and float(got.out[4]) == 0.5
        # on the boundary the full gradient, ratio = 1: d loss / d mean = -adv (actions - mean) / m
        torch.testing.assert_close(t32.d_mean[:6, 0], -adv[:6] * d[:6] / n, rtol=1e-6, atol=0)
        assert bool((t32.dv[:3] == 0).all()) and bool((t32.q1[:3] == t32.q2[:3]).all())
        torch.testing.assert_close(t32.d_value[:3], half * 2 * e1[:3] / n, rtol=1e-6, atol=0)
    else:
        assert bool((t32.dv[:4].abs() == 0.25).all()) and bool((t32.q1[:4] == t32.q2[:4]).all())
        torch.testing.assert_close(t32.d_value[:4], half * 2 * e1[:4] / n, rtol=1e-6, atol=0)
        assert bool((t32.q1[6:8] == t32.q2[6:8]).all()) and bool((t32.dv[6:8].abs() > 0.25).all())
        torch.testing.assert_close(t32.d_value[6:8], half * e1[6:8] / n, rtol=1e-6, atol=0)  # half: the clamp is flat
        assert bool((adv[4:6] == 0).all()) and bool((t32.d_mean[4:6] == 0).all())
    # every row, the tie and boundary rows among them, within 8 u of torch's own fp32 gradient
    for name in ("d_mean", "d_value"):
        a, b = getattr(got, name).reshape(n), getattr(t32, name).reshape(n)
        assert bool(((a - b).abs() <= 8 * U * b.abs()).all()), (name, a, b)
        assert bool((b[special] != 0).any())
    # d_logstd sums n rows of about d_mean's size, and the entropy term of size ent_coef
    assert abs(float(got.d_logstd - t32.d_logstd)) <= 8 * U * float(t32.d_logstd.abs() + t32.d_mean.abs().sum() + 1.0)
    torch.testing.assert_close(got.out, t32.out, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------- gate 2
@pytest.fixture(scope="module")
def big(gpu):
    r = tile()
    cases = (make_case(m=2 * r + 1, A=12, seed=21), make_case(m=r + 1, A=13, seed=22, norm_adv=False, clip_vloss=False))
    return [(c, {n: v.to(DEV) for n, v in c.t.items()}, run_kernel(c)) for c in cases]


def test_bitwise_run_to_run(big):
    for c, t, first in big:
        for _ in range(2):
            again = run_kernel(c, t)
            assert all(torch.equal(a, b) for a, b in zip(flat(again), flat(first)))
        assert bool(torch.isfinite(torch.cat([x.reshape(-1) for x in flat(first)])).all())
        assert bool((first.d_logstd != 0).all()) and bool((first.out != 0).all())


def test_out_of_range_indices_are_clamped(big):
    c, t, first = big[0]
    idx = c.idx.to(DEV).clone()
    wild = idx.clone()
    wild[idx == 0] = -7
    wild[idx == c.n_src - 1] = c.n_src + 3
    wild[5] = 2 ** 40
    idx[5] = c.n_src - 1
    a, b = run_kernel(c, t, idx=wild), run_kernel(c, t, idx=idx)
    assert all(torch.equal(x, y) for x, y in zip(flat(a), flat(b)))
    assert not torch.equal(a.d_mean, first.d_mean)  # row 5 moved, and with it the minibatch's advantage statistics


def test_statistics_accumulate_over_two_calls(big):
    for c, t, first in big:
        stats = torch.zeros(5, device=DEV)
        want = torch.zeros(5, device=DEV)
        for _ in range(2):
            got = run_kernel(c, t, stats=stats)
            want += got.out
            assert torch.equal(stats, want)
        assert torch.equal(got.out, first.out) and bool((stats != 0).all())


def test_captured_graph_follows_changes_of_mean_idx_and_value_statistics(big):
    c, t, first = big[0]
    t = dict(t, mean=t["mean"].clone(), value_mean=t["value_mean"].clone(), value_var=t["value_var"].clone())
    idx = c.idx.to(DEV).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run_kernel(c, t, idx=idx)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run_kernel(c, t, idx=idx)
    g.replay()
    assert all(torch.equal(a, b) for a, b in zip(flat(out), flat(first)))
    seen = [first]
    for change in (lambda: t["mean"].add_(0.05), lambda: idx.copy_(idx.flip(0)),
                   lambda: (t["value_mean"].fill_(1.2), t["value_var"].fill_(3.1))):
        change()
        g.replay()
        new = run_kernel(c, t, idx=idx)
        assert not torch.equal(new.out, seen[-1].out)
        assert all(torch.equal(a, b) for a, b in zip(flat(out), flat(new)))
        seen.append(new)


def test_one_workspace_serves_every_smaller_m_without_zeroing(gpu):
    r = tile()
    nbytes = _learn.learn_library().h12learn_cleanrl_head_workspace_bytes(2 * r + 1, 12)
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=DEV)  # poison, never cleared
    for m in (2 * r + 1, r + 1, r - 1, 2, 2 * r + 1):
        c = make_case(m=m, A=12, seed=30 + m)
        own = run_kernel(c)
        shared = run_kernel(c, ws=ws)
        assert all(torch.equal(a, b) for a, b in zip(flat(own), flat(shared))), m
        assert bool(torch.isfinite(torch.cat([x.reshape(-1) for x in flat(shared)])).all())
    with pytest.raises(Exception, match="workspace_bytes"):
        run_kernel(make_case(m=3 * r + 1, A=12), ws=ws)
    assert _learn.cleanrl_head_workspace(r + 1, 12, DEV) is _learn.cleanrl_head_workspace(r + 1, 12, DEV)


def rms_module(c, t):
    rms = cleanrl.RunningMeanStd(shape=(), epsilon=c.veps).to(DEV)
    rms.running_mean.copy_(t["value_mean"]), rms.running_var.copy_(t["value_var"])
    return rms


def test_autograd_node_returns_the_kernels_gradients(big):
    from h12env.ppo_head import CleanRLHead, CleanRLInputs

    for c, t, first in big:
        mean, value, logstd = (t[n].clone().requires_grad_(True) for n in ("mean", "value", "logstd"))
        h = CleanRLInputs(idx=c.idx.to(DEV), old_log_prob=t["old_log_prob"], advantages=t["advantages"],
                          returns_n=t["returns_n"], values_n=t["values_n"], actions=t["actions"],
                          value_rms=rms_module(c, t), clip_coef=c.clip, ent_coef=c.ecoef, vf_coef=c.vcoef,
                          norm_adv=c.norm_adv, clip_vloss=c.clip_vloss)
        v2, l2 = value.view(-1, 1), logstd.view(1, -1)  # the critic's [m][1] output, the agent's [1][A] parameter
        loss, out = CleanRLHead.apply(mean, v2, l2, h)
        assert torch.equal(out, first.out) and torch.equal(loss, first.out[3]) and not out.requires_grad
        (2.0 * loss).backward()
        assert torch.equal(mean.grad, 2.0 * first.d_mean) and torch.equal(value.grad, 2.0 * first.d_value)
        assert torch.equal(logstd.grad, 2.0 * first.d_logstd)


# ---------------------------------------------------------------------------------------------- gate 3
TASK = "Isaac-Velocity-CaT-Flat-H12_12dof-v0"
LOSS_KEYS = ("Loss/mean_pg_loss", "Loss/mean_entropy_loss", "Loss/mean_v_loss", "Loss/mean_surrogate_loss",
             "Loss/clipfrac", "Loss/learning_rate")


def trainer_run(tmp, graph, fused_loss, minibatch_size=384, resume=None, iterations=2):
    """cleanrl.PPO on the CaT task at 64 envs x 24 steps; returns the agent, the logged lines and the number of calls
    of the kernel's binding."""
    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from biped_tasks.tasks.agents import H12_12dof_FlatCleanRlPPOCfg
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    calls = []
    orig = _learn.cleanrl_head
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("H12_PPO_GRAPH", "1" if graph else "0")
        mp.delenv("H12_CLEANRL_HEAD_FUSED", raising=False)
        mp.setattr(_learn, "cleanrl_head", lambda *a, **k: (calls.append(a[0].shape[0]), orig(*a, **k))[1])
        cfg = load_cfg_from_registry(TASK, "env_cfg_entry_point")
        cfg.scene.num_envs = 64
        cfg.sim.device = DEV
        cfg.seed = 3
        env = gym.make(TASK, cfg=cfg)
        ppo_cfg = H12_12dof_FlatCleanRlPPOCfg(num_steps=24, num_iterations=iterations, minibatch_size=minibatch_size,
                                              updates_epochs=2, save_interval=2)
        torch.manual_seed(21)
        run = tmp / f"g{int(graph)}_f{int(fused_loss)}_{minibatch_size}_{'r' if resume else 'n'}"
        agent = cleanrl.PPO(env, ppo_cfg, str(run), resume_path=resume, fused_loss=fused_loss)
        env.close()
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    return SimpleNamespace(agent=agent, lines=lines, calls=calls, run=run)


@pytest.fixture(scope="module")
def trainer_runs(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cleanrl_head")
    return SimpleNamespace(graphed=trainer_run(tmp, True, True), eager=trainer_run(tmp, False, True),
                           default=trainer_run(tmp, True, False), tmp=tmp)


def assert_same_training(a, b):
    for (k, p), q in zip(a.agent.state_dict().items(), b.agent.state_dict().values()):
        assert torch.isfinite(p).all() and torch.equal(p, q), (k, float((p - q).abs().max()))
    assert [k for k in a.agent.state_dict() if "rms" in k] == [f"{m}.{n}" for m in ("obs_rms", "value_rms")
                                                               for n in ("running_mean", "running_var", "count")]
    for x, y in zip(a.lines, b.lines):
        assert all(math.isfinite(x[k]) for k in LOSS_KEYS)
        assert {k: x[k] for k in LOSS_KEYS} == {k: y[k] for k in LOSS_KEYS}
    assert len(a.lines) == len(b.lines) == 2


def test_graphed_update_equals_eager_bit_for_bit(trainer_runs):
    g, e = trainer_runs.graphed, trainer_runs.eager
    assert_same_training(g, e)
    # graphed: two warm-up calls and the capture; eager: 2 iterations x 2 epochs x 4 minibatches
    assert g.calls == [384] * 3 and e.calls == [384] * 16
    assert g.lines[0]["Loss/learning_rate"] != g.lines[1]["Loss/learning_rate"]  # annealed through the device scalar
    assert g.lines[0]["Loss/clipfrac"] >= 0.0 and g.lines[0]["Loss/mean_v_loss"] > 0.0


def test_default_path_never_reaches_the_kernel_and_agrees_to_rounding(trainer_runs):
    f, d = trainer_runs.graphed, trainer_runs.default
    assert d.calls == [] and len(d.lines) == 2
    assert list(f.agent.state_dict()) == list(d.agent.state_dict())
    x, y = f.lines[0], d.lines[0]
    for key in LOSS_KEYS:
        print(f"FIRST {key}: fused {x[key]!r} default {y[key]!r}")
    for key in LOSS_KEYS:
        assert abs(x[key] - y[key]) <= 1e-3 * max(1.0, abs(y[key])), (key, x[key], y[key])


def test_ragged_last_minibatch_gets_its_own_capture(trainer_runs):
    g = trainer_run(trainer_runs.tmp, True, True, minibatch_size=500)
    e = trainer_run(trainer_runs.tmp, False, True, minibatch_size=500)
    assert_same_training(g, e)
    assert 1536 % 500 == 36
    assert g.calls == [500] * 3 + [36] * 3 and e.calls == ([500] * 3 + [36]) * 4


def test_fused_checkpoint_trains_on_in_a_default_run(trainer_runs):
    ck = trainer_runs.graphed.run / "model_1.pt"
    saved = torch.load(ck, map_location=DEV, weights_only=True)
    fresh = cleanrl.Agent(SimpleNamespace(unwrapped=SimpleNamespace(
        single_observation_space={"policy": SimpleNamespace(shape=(saved["obs_rms.running_mean"].shape[0],))},
        single_action_space=SimpleNamespace(shape=(12,)))))
    fresh.load_state_dict(saved)  # strict: the default run's keys and shapes
    d = trainer_run(trainer_runs.tmp, True, False, resume=str(ck), iterations=1)
    assert d.calls == [] and len(d.lines) == 1 and all(math.isfinite(d.lines[0][k]) for k in LOSS_KEYS)
    assert all(torch.isfinite(v).all() for v in d.agent.state_dict().values())
    assert not torch.equal(d.agent.state_dict()["actor_mean.0.weight"], saved["actor_mean.0.weight"])


def test_minibatch_gradients_against_fp64(gpu):
    """One minibatch from identical state on either path, before the optimiser step, against the loss restated in fp64
    on a double copy of the agent."""
    from h12env.ppo_head import CleanRLHead, CleanRLInputs, torch_cleanrl_head

    n_obs, n_act, n_src, m = 270, 12, 1536, 384
    envs = SimpleNamespace(unwrapped=SimpleNamespace(single_observation_space={"policy": SimpleNamespace(shape=(n_obs,))},
                                                     single_action_space=SimpleNamespace(shape=(n_act,))))
    torch.manual_seed(11)
    agent = cleanrl.Agent(envs).to(DEV)
    with torch.no_grad():
        agent.actor_logstd.copy_(0.1 * torch.randn(1, n_act))
        agent.value_rms.running_mean.fill_(1.7), agent.value_rms.running_var.fill_(2.3)
    g = torch.Generator(device=DEV).manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)  # noqa: E731
    with torch.no_grad():  # a rollout the policy could have produced: ratios near 1, both clip branches live
        obs = rnd(n_src, n_obs)
        mu, std = agent.actor_mean(obs), agent.actor_logstd.exp()
        actions = mu + std * rnd(n_src, n_act)
        logprobs = torch.distributions.Normal(mu, std).log_prob(actions).sum(1) + 0.15 * rnd(n_src)
        values_n = agent.value_rms(agent.critic(obs).view(-1), update=False) + 0.15 * rnd(n_src)
        returns_n = values_n + rnd(n_src)
        advantages = 0.3 + rnd(n_src)
    idx = torch.randperm(n_src, generator=torch.Generator().manual_seed(9))[:m].to(DEV)

    def inputs(a, dtype):
        c = lambda t: t.to(dtype)  # noqa: E731
        return CleanRLInputs(idx=idx, old_log_prob=c(logprobs), advantages=c(advantages), returns_n=c(returns_n),
                             values_n=c(values_n), actions=c(actions), value_rms=a.value_rms, clip_coef=0.2,
                             ent_coef=0.0081, vf_coef=2.0, norm_adv=True, clip_vloss=True)

    def grads(a, head, dtype=torch.float32):
        a.zero_grad()
        x = obs.to(dtype)[idx]
        head(a.actor_mean(x), a.critic(x), a.actor_logstd, inputs(a, dtype))[0].backward()
        return {k: p.grad.clone() for k, p in a.named_parameters()}

    ref = grads(copy.deepcopy(agent).double(), torch_cleanrl_head, torch.float64)
    fused = grads(agent, CleanRLHead.apply)
    default = grads(agent, torch_cleanrl_head)  # the default path's statements on the device
    rows = []
    for k, r in ref.items():
        rows.append((k, float((fused[k].double() - r).abs().max()), float((default[k].double() - r).abs().max()),
                     float(r.abs().max())))
        print(f"GRAD {k}: max|grad| {rows[-1][3]:.3e}  fused error {rows[-1][1]:.3e}  default error {rows[-1][2]:.3e}")
    assert len(rows) == 17
    for k, ef, ed, gmax in rows:
        assert gmax > 0 and ef <= FACTOR * ed + U * gmax, (k, ef, ed, gmax)
