"""GPU: the fused PPO loss head (h12learn_ppo_head, csrc/h12_ppo_head.hip; h12env.ppo_head.PPOHead;
PPO(fused_loss=True)).  DESIGN.md section 7n.  u = 2^-24, R = the row tile.

Gate 1  against fp64: PPO._minibatch's expression restated in float64 on a double copy of the fp32 inputs and
        differentiated by torch autograd.  Per output tensor (out, d_mean, d_value, d_param) the kernel's worst
        elementwise error is at most FACTOR x the worst error of the same restatement evaluated by torch in fp32 on the
        device (the default path's arithmetic) + u max|ref|.  Exact ties and boundaries are kept out of these data and
        tested on their own against torch autograd on the same fp32 inputs.
Gate 2  bitwise: run to run; row permutations; equal halves under augmentation; a captured graph follows in-place
        changes of mean and idx; the learning-rate rule; the statistics accumulator; index clamping.
Gate 3  the runner at 64 envs x 24 steps (minibatches of 384 rows): captured update == eager update bit for bit with the
        switch on (plain, symmetry, privileged critic, fused learner, bf16, log_std); one minibatch's gradients against the
        loss restated in fp64; train.py --fused_loss in a subprocess and its checkpoint in a default-path runner.
"""
import copy
import json
import math
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch
from torch.distributions import Normal

ROOT = Path(__file__).resolve().parents[1]
SHIMS = ROOT / "h1v2-isaac_amd" / "shims"
for p in (str(SHIMS), str(ROOT / "tests" / "helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

from h12env import _learn  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FACTOR = 8.0  # the smallest power of two above the worst measured ratio (4.92, two rows), table there
DEV = "cuda:0"
PER_ROW = ("old_log_prob", "advantages", "returns", "target_values", "old_mu", "old_sigma")


def tile():
    return _learn.ppo_head_rows()


# ---------------------------------------------------------------------------------------------- data
def make_case(m, B, A, kind="scalar", clipped=True, use_idx=True, direct=False, seed=0, clip=0.2):
    """A minibatch on the CPU (fp32) whose rows fall on every side of both clip ranges.  The rollout has
    n_src = 3 B + 5 rows; idx holds 0, n_src - 1 and a duplicate where B allows."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * m + A)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    n_src = 3 * B + 5
    sigma = 0.5 + 0.7 * torch.rand(A, generator=g)
    std_param = sigma.log() if kind == "log" else sigma.clone()
    sigma = std_param.exp() if kind == "log" else std_param
    idx = None
    if use_idx:
        idx = torch.randint(0, n_src, (B,), generator=g)
        idx[0] = 0
        if B >= 2:
            idx[B - 1] = n_src - 1
        if B >= 4:
            idx[2] = idx[1]
    base = idx if use_idx else torch.arange(B)
    k = torch.cat([base, base]) if m == 2 * B else base
    z = rn(m, A)
    if m == 2 * B:  # the mirrored rows: log-probabilities near their originals'
        z[B:] = z[:B].roll(1, dims=1) + 0.05 * rn(B, A)
    if direct:
        mean = 0.5 * rn(m, A)
        actions = mean + sigma * z
        act_rows = actions
    else:
        actions = rn(n_src, A)
        act_rows = actions[k]
        mean = act_rows - sigma * z
    s64 = sigma.double()
    lp = (-(act_rows.double() - mean.double()).square() / (2 * s64.square()) - s64.log()
          - math.log(math.sqrt(2 * math.pi))).sum(-1)
    old_log_prob = rn(n_src) * 0.5 - 1.4 * A
    old_log_prob[k] = (lp + 0.25 * rn(m).double()).float()
    target = rn(n_src)
    value = target[k] + 0.3 * rn(m)
    old_mu = 0.5 * rn(n_src, A)
    old_mu[k[:B]] = mean[:B] + 0.1 * rn(B, A)
    old_sigma = sigma * (1.0 + 0.1 * rn(n_src, A)).abs() + 0.05
    t = dict(mean=mean.contiguous(), value=value, std_param=std_param, old_log_prob=old_log_prob, advantages=rn(n_src),
             returns=target + 0.5 * rn(n_src), target_values=target, old_mu=old_mu, old_sigma=old_sigma,
             actions=actions.contiguous())
    return SimpleNamespace(m=m, B=B, A=A, n_src=n_src, kind=kind, clipped=clipped, direct=direct, clip=clip, idx=idx,
                           k=k, vcoef=0.7, ecoef=0.01, t=t)


def restated(c, dtype, device):
    """PPO._minibatch's loss head on copies of c's tensors in ``dtype``: out [5], the three gradients, and the
    quantities the branches turn on."""
    t = {n: v.to(device=device, dtype=dtype) for n, v in c.t.items()}
    mean, value, prm = (t[n].requires_grad_(True) for n in ("mean", "value", "std_param"))
    k, B = c.k.to(device), c.B
    actions = t["actions"] if c.direct else t["actions"][k]
    old_log_prob, adv, returns, target = (t[n][k] for n in ("old_log_prob", "advantages", "returns", "target_values"))
    old_mu, old_sigma = t["old_mu"][k[:B]], t["old_sigma"][k[:B]]
    s = prm if c.kind == "scalar" else torch.exp(prm)
    dist = Normal(mean, s.expand_as(mean))
    log_prob = dist.log_prob(actions).sum(dim=-1)
    mu, sigma, entropy = dist.mean[:B], dist.stddev[:B], dist.entropy().sum(dim=-1)[:B]
    with torch.no_grad():
        kl = torch.sum(torch.log(sigma / old_sigma + 1e-5)
                       + (old_sigma.square() + (old_mu - mu).square()) / (2.0 * sigma.square()) - 0.5, dim=-1)
        kl_mean = kl.mean()
    ratio = torch.exp(log_prob - old_log_prob)
    surrogate = -adv * ratio
    surrogate_clipped = -adv * torch.clamp(ratio, 1.0 - c.clip, 1.0 + c.clip)
    surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
    q1 = (value - returns).square()
    v_clipped = target + (value - target).clamp(-c.clip, c.clip)
    q2 = (v_clipped - returns).square()
    if c.clipped:
        value_loss = torch.max(q1, q2).mean()
    else:
        value_loss = (returns - value).square().mean()
    loss = surrogate_loss + c.vcoef * value_loss - c.ecoef * entropy.mean()
    loss.backward()
    out = torch.stack([surrogate_loss, value_loss, entropy.mean(), kl_mean, loss]).detach()
    return SimpleNamespace(out=out, d_mean=mean.grad, d_value=value.grad, d_param=prm.grad, ratio=ratio.detach(),
                           adv=adv, dv=(value - target).detach(), q1=q1.detach(), q2=q2.detach())


def run_kernel(c, t=None, idx="case", lr=None, desired_kl=None, stats=None):
    """The entry point called directly on c's tensors (or the device copies ``t``)."""
    t = t or {n: v.to(DEV) for n, v in c.t.items()}
    if isinstance(idx, str):
        idx = None if c.idx is None else c.idx.to(DEV)
    d_mean, d_value, d_param, out = _learn.ppo_head(
        t["mean"], t["value"], t["std_param"], _learn.PPO_STD_LOG if c.kind == "log" else _learn.PPO_STD_SCALAR, idx, c.B,
        *(t[n] for n in PER_ROW), t["actions"], c.direct, c.clip, c.vcoef, c.ecoef, c.clipped, lr=lr,
        desired_kl=desired_kl, stats_accum=stats)
    return SimpleNamespace(out=out, d_mean=d_mean, d_value=d_value, d_param=d_param)


def assert_every_branch_is_populated(c, ref):
    lo, hi = 1.0 - c.clip, 1.0 + c.clip
    for side in (ref.ratio < lo, (ref.ratio > lo) & (ref.ratio < hi), ref.ratio > hi):
        assert bool((side & (ref.adv > 0)).any()) and bool((side & (ref.adv < 0)).any()), (c.m, c.A)
    assert bool((ref.dv < -c.clip).any()) and bool((ref.dv.abs() < c.clip).any()) and bool((ref.dv > c.clip).any())
    assert bool((ref.q1 > ref.q2).any()) and bool((ref.q2 > ref.q1).any())
    # no planted tie or boundary here: those have a test of their own
    assert not bool((ref.ratio == lo).any() | (ref.ratio == hi).any() | (ref.dv.abs() == c.clip).any())
    assert not bool((ref.adv == 0).any())


# ---------------------------------------------------------------------------------------------- gate 1
def gate1_cases():
    """Shapes as expressions of the row tile R and the kernel's maximum A (resolved when the test runs)."""
    cases = []
    for m in ("1", "R-1", "R", "R+1", "2R+1"):
        cases.append(dict(m=m, aug=False, A=12))
    for b in ("1", "R/2", "R/2+1", "R+1"):
        cases.append(dict(m=b, aug=True, A=12, direct=True))
    cases.append(dict(m="R/2+1", aug=True, A=12, direct=False))
    for a in (1, 13, "max"):
        cases.append(dict(m="R+1", aug=False, A=a))
    cases.append(dict(m="R/2+1", aug=True, A="max", direct=True))
    cases.append(dict(m="R+1", aug=False, A=12, use_idx=False))
    cases.append(dict(m="R/2+1", aug=True, A=12, direct=True, use_idx=False))
    cases.append(dict(m="2R+1", aug=False, A=12, kind="log"))
    cases.append(dict(m="R/2+1", aug=True, A=13, kind="log", direct=True))
    cases.append(dict(m="R+1", aug=False, A=12, clipped=False))
    cases.append(dict(m="R/2", aug=True, A=1, clipped=False, kind="log", direct=True))
    return cases


def resolve(spec):
    r = tile()
    rows = {"1": 1, "R-1": r - 1, "R": r, "R+1": r + 1, "2R+1": 2 * r + 1, "R/2": r // 2, "R/2+1": r // 2 + 1}[spec["m"]]
    a = _learn.ppo_head_max_actions() if spec["A"] == "max" else spec["A"]
    kw = {k: v for k, v in spec.items() if k not in ("m", "aug", "A")}
    return dict(m=2 * rows if spec["aug"] else rows, B=rows, A=a, **kw)


def case_id(spec):
    return "-".join(f"{k}={v}" for k, v in spec.items())


def errors(c):
    """Per output tensor: (kernel's worst error, fp32 torch's worst error, max|ref|) against the fp64 restatement."""
    ref = restated(c, torch.float64, DEV)
    t32 = restated(c, torch.float32, DEV)
    got = run_kernel(c)
    rows = {}
    for name in ("out", "d_mean", "d_value", "d_param"):
        r = getattr(ref, name)
        rows[name] = (float((getattr(got, name).double() - r).abs().max()),
                      float((getattr(t32, name).double() - r).abs().max()), float(r.abs().max()))
    for i, name in enumerate(("surrogate", "value_loss", "entropy", "kl", "loss")):  # printed, not gated one by one
        r = ref.out[i]
        print(f"OUT {name}: kernel {float((got.out[i].double() - r).abs()):.3e} "
              f"torch32 {float((t32.out[i].double() - r).abs()):.3e} ref {float(r):.6e}")
    return ref, rows


@pytest.mark.parametrize("spec", gate1_cases(), ids=case_id)
def test_outputs_and_gradients_against_fp64(gpu, spec):
    kw = resolve(spec)
    c = make_case(seed=3, **kw)
    ref, rows = errors(c)
    if c.B >= tile() // 2 and c.clipped:
        assert_every_branch_is_populated(c, ref)
    for name, (ek, et, scale) in rows.items():
        ratio = max(0.0, ek - U * scale) / et if et > 0 else (0.0 if ek <= U * scale else math.inf)
        print(f"GATE1 {case_id(spec)} {name}: kernel {ek:.3e} torch32 {et:.3e} max|ref| {scale:.3e} ratio {ratio:.2f}")
    for name, (ek, et, scale) in rows.items():
        assert ek <= FACTOR * et + U * scale, (name, ek, et, scale)


# ---------------------------------------------------------------------------------------------- ties and boundaries
def tie_case(clip):
    """A = 1, sigma = 1: a row's log-probability is the same single rounded expression in torch and in the kernel, so
    old_log_prob = log_prob plants ratio == 1 exactly.  clip = 0: ratio == 1 sits on both ends of the clip range and
    value == target on both ends of the value clip.  clip = 0.25 (exact in binary): value - target == +-clip, a tie of
    the two value operands outside the range, and advantages of exactly zero."""
    n = 12
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    mean, actions = rn(n, 1), rn(n, 1)
    lp = -((actions - mean) ** 2) / 2.0 - 0.0 - math.log(math.sqrt(2 * math.pi))  # torch's Normal.log_prob, sigma = 1
    old_log_prob = lp.squeeze(-1).clone()
    adv = rn(n)
    target = rn(n)
    value = target + 0.5 * rn(n)
    returns = target + 0.5 * rn(n)
    special = torch.zeros(n, dtype=torch.bool)
    if clip == 0.0:
        old_log_prob[6:9] += 0.3     # ratio below 1
        old_log_prob[9:] -= 0.3      # ratio above 1; rows 0..5 have ratio == 1 exactly
        value[0:3] = target[0:3]     # value - target == 0 == +-clip
        special[:6] = True
    else:
        old_log_prob[0:6] += torch.tensor([0.1, -0.1, 0.5, -0.5, 0.5, -0.5])
        adv[4:6] = 0.0               # outside the range with s1 == s2 == 0
        target[0:4] = torch.tensor([0.0, 0.0, 0.5, -2.0])
        value[0:4] = target[0:4] + torch.tensor([0.25, -0.25, 0.25, -0.25])   # on the value clip's ends
        target[6], value[6], returns[6] = 0.0, 1.0, 0.625                   # e1 = 0.375 = -e2 outside the range
        target[7], value[7], returns[7] = 1.0, 0.0, 0.375                   # the same from below
        special[:8] = True
    t = dict(mean=mean, value=value, std_param=torch.ones(1), old_log_prob=old_log_prob, advantages=adv,
             returns=returns, target_values=target, old_mu=mean + 0.1, old_sigma=torch.ones(n, 1), actions=actions)
    c = SimpleNamespace(m=n, B=n, A=1, n_src=n, kind="scalar", clipped=True, direct=False, clip=clip, idx=None,
                        k=torch.arange(n), vcoef=0.7, ecoef=0.01, t=t)
    return c, special


@pytest.mark.parametrize("clip", [0.0, 0.25])
def test_ties_and_boundaries_get_the_gradient_torch_autograd_gives(gpu, clip):
    c, special = tie_case(clip)
    t32 = restated(c, torch.float32, DEV)
    got = run_kernel(c)
    n = c.m
    adv, d = c.t["advantages"].to(DEV), (c.t["actions"] - c.t["mean"]).to(DEV).squeeze(-1)
    e1 = (c.t["value"] - c.t["returns"]).to(DEV)
    if clip == 0.0:
        assert bool((t32.ratio[:6] == 1.0).all()) and bool((t32.ratio[6:] != 1.0).all())
        # on the boundary the full gradient, ratio = 1: d loss / d mean = -adv (actions - mean) / m
        torch.testing.assert_close(t32.d_mean[:6, 0], -adv[:6] * d[:6] / n, rtol=1e-6, atol=0)
        assert bool((t32.dv[:3] == 0).all()) and bool((t32.q1[:3] == t32.q2[:3]).all())
        torch.testing.assert_close(t32.d_value[:3], c.vcoef * 2 * e1[:3] / n, rtol=1e-6, atol=0)
    else:
        assert bool((t32.dv[:4].abs() == 0.25).all()) and bool((t32.q1[:4] == t32.q2[:4]).all())
        torch.testing.assert_close(t32.d_value[:4], c.vcoef * 2 * e1[:4] / n, rtol=1e-6, atol=0)
        assert bool((t32.q1[6:8] == t32.q2[6:8]).all()) and bool((t32.dv[6:8].abs() > 0.25).all())
        torch.testing.assert_close(t32.d_value[6:8], c.vcoef * e1[6:8] / n, rtol=1e-6, atol=0)  # half: the clamp is flat
        assert bool((t32.d_mean[4:6] == 0).all())
    # every row, the tie and boundary rows among them, within 8 u of torch's own fp32 gradient
    for name in ("d_mean", "d_value"):
        a, b = getattr(got, name).reshape(n), getattr(t32, name).reshape(n)
        assert bool(((a - b).abs() <= 8 * U * b.abs()).all()), (name, a, b)
        assert bool((b[special] != 0).any())
    # d_param sums n rows of about d_mean's size, and the entropy term of size entropy_coef
    assert abs(float(got.d_param - t32.d_param)) <= 8 * U * float(t32.d_param.abs() + t32.d_mean.abs().sum() + 1.0)
    torch.testing.assert_close(got.out, t32.out, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------- gate 2
@pytest.fixture(scope="module")
def big(gpu):
    r = tile()
    plain = make_case(m=2 * r + 1, B=2 * r + 1, A=12, seed=21)
    aug = make_case(m=2 * (r + 1), B=r + 1, A=12, direct=True, seed=22)
    return [(c, {n: v.to(DEV) for n, v in c.t.items()}, run_kernel(c)) for c in (plain, aug)]


def flat(o):
    return [o.out, o.d_mean, o.d_value, o.d_param]


def test_bitwise_run_to_run(big):
    for c, t, first in big:
        for _ in range(2):
            again = run_kernel(c, t)
            assert all(torch.equal(a, b) for a, b in zip(flat(again), flat(first)))
        assert bool(torch.isfinite(torch.cat([x.reshape(-1) for x in flat(first)])).all())


def test_bitwise_permuting_the_minibatch_permutes_the_gradient_rows(big):
    c, t, first = big[0]
    perm = torch.randperm(c.m, generator=torch.Generator().manual_seed(1)).to(DEV)
    tp = dict(t, mean=t["mean"][perm].contiguous(), value=t["value"][perm].contiguous())
    got = run_kernel(c, tp, idx=c.idx.to(DEV)[perm].contiguous())
    assert torch.equal(got.d_mean, first.d_mean[perm]) and torch.equal(got.d_value, first.d_value[perm])
    assert not torch.equal(got.d_mean, first.d_mean)
    torch.testing.assert_close(got.d_param, first.d_param, rtol=1e-4, atol=1e-6)  # another summation order
    torch.testing.assert_close(got.out, first.out, rtol=1e-5, atol=1e-6)


def test_bitwise_equal_halves_under_augmentation(big):
    c, t, _ = big[1]
    B = c.B
    same = dict(t, mean=torch.cat([t["mean"][:B]] * 2), value=torch.cat([t["value"][:B]] * 2),
                actions=torch.cat([t["actions"][:B]] * 2))
    got = run_kernel(c, same)
    assert torch.equal(got.d_mean[:B], got.d_mean[B:]) and torch.equal(got.d_value[:B], got.d_value[B:])
    assert bool((got.d_mean[:B] != 0).any())
    # and the per-sample scalars of a mirrored row are its original's: rows [B, 2B) of the plain run differ from a
    # run whose mirrored half is shifted by one sample
    shifted = run_kernel(c, dict(same, mean=torch.cat([t["mean"][:B], t["mean"][:B].roll(1, 0)]),
                                 value=torch.cat([t["value"][:B], t["value"][:B].roll(1, 0)]),
                                 actions=torch.cat([t["actions"][:B], t["actions"][:B].roll(1, 0)])))
    assert torch.equal(shifted.d_mean[:B], got.d_mean[:B]) and not torch.equal(shifted.d_mean[B:], got.d_mean[B:])


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


def test_captured_graph_follows_changes_of_mean_and_idx(big):
    c, t, first = big[0]
    t = dict(t, mean=t["mean"].clone())
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
    t["mean"].add_(0.05)
    idx.copy_(idx.flip(0))
    g.replay()
    new = run_kernel(c, t, idx=idx)
    assert not torch.equal(new.d_mean, first.d_mean) and not torch.equal(new.out, first.out)
    assert all(torch.equal(a, b) for a, b in zip(flat(out), flat(new)))


def torch_lr_rule(lr, kl_mean, desired_kl):
    """PPO._minibatch's schedule on the device tensor, verbatim."""
    up = kl_mean > desired_kl * 2.0
    down = (kl_mean > 0.0) & (kl_mean < desired_kl / 2.0)
    return torch.where(up, torch.clamp(lr / 1.5, min=1e-5), torch.where(down, torch.clamp(lr * 1.5, max=1e-2), lr))


def test_learning_rate_rule_bit_for_bit(gpu):
    """A KL mean of exactly 0 cannot be planted through finite inputs: every element of the KL expression is at least
    about log(1 + 1e-5) > 0.  The smallest reachable KL (identical distributions) takes the branch next to
    it, 0 < kl < desired_kl / 2."""
    c = make_case(m=tile() + 1, B=tile() + 1, A=12, use_idx=False, seed=23)
    t = {n: v.to(DEV) for n, v in c.t.items()}
    first = run_kernel(c, t)
    kl = first.out[3]
    k = float(kl)
    assert k > 0
    same = dict(t, old_mu=t["old_mu"].clone(), old_sigma=t["old_sigma"].clone())
    same["old_mu"][:c.B] = t["mean"]
    same["old_sigma"][:c.B] = t["std_param"]
    tiny = run_kernel(c, same).out[3]
    assert 0 < float(tiny) < 2e-5 * c.A
    seen = set()
    for tt, kl_t, desired, start in [(t, kl, k / 4, 1e-3), (t, kl, k / 4, 3e-4), (t, kl, k, 1e-3), (t, kl, 4 * k, 1e-3),
                                     (t, kl, 4 * k, 7e-3), (t, kl, k / 4, 1e-5), (t, kl, k / 4, 1.2e-5),
                                     (t, kl, 4 * k, 1e-2), (t, kl, 4 * k, 9e-3), (t, kl, k / 2, 1e-3), (t, kl, 2 * k, 1e-3),
                                     (same, tiny, 0.01, 1e-3), (same, tiny, 1e-5 * c.A, 1e-3)]:
        lr = torch.tensor(start, device=DEV)
        want = torch_lr_rule(lr.clone(), kl_t, desired)
        got = run_kernel(c, tt, lr=lr, desired_kl=desired)
        assert torch.equal(got.out[3], kl_t)
        assert torch.equal(lr, want), (desired, start, float(lr), float(want))
        s32 = float(torch.tensor(start, dtype=torch.float32))
        seen.add("up" if float(want) < s32 else ("down" if float(want) > s32 else "stay"))
        if start in (1e-5, 1e-2):
            assert float(lr) == s32  # at a bound it stays put
        assert all(torch.equal(a, b) for a, b in zip(flat(got)[1:], flat(first if tt is t else run_kernel(c, same))[1:]))
    assert seen == {"up", "down", "stay"}
    # no lr given: nothing is written anywhere else
    lr = torch.tensor(1e-3, device=DEV)
    run_kernel(c, t)
    assert float(lr) == float(torch.tensor(1e-3, dtype=torch.float32))


def test_statistics_accumulate_over_two_calls(big):
    for c, t, first in big:
        stats = torch.zeros(3, device=DEV)
        want = torch.zeros(3, device=DEV)
        for _ in range(2):
            got = run_kernel(c, t, stats=stats)
            want += torch.stack([got.out[1], got.out[0], got.out[2]])
            assert torch.equal(stats, want)
        assert torch.equal(got.out, first.out) and bool((stats != 0).all())


def test_autograd_node_returns_the_kernels_gradients(big):
    from h12env.ppo_head import HeadInputs, PPOHead

    for c, t, first in big:
        mean, value, prm = (t[n].clone().requires_grad_(True) for n in ("mean", "value", "std_param"))
        col = lambda n: t[n].view(-1, 1)  # noqa: E731  the storage's [n_src][1] columns
        h = HeadInputs(idx=c.idx.to(DEV), old_log_prob=col("old_log_prob"), advantages=col("advantages"),
                       returns=col("returns"), target_values=col("target_values"), old_mu=t["old_mu"],
                       old_sigma=t["old_sigma"], actions=t["actions"], actions_direct=c.direct, std_kind=c.kind,
                       clip_param=c.clip, value_loss_coef=c.vcoef, entropy_coef=c.ecoef, use_clipped_value_loss=True)
        loss, out = PPOHead.apply(mean, value.view(-1, 1), prm, h)
        assert torch.equal(out, first.out) and torch.equal(loss, first.out[4]) and not out.requires_grad
        (2.0 * loss).backward()
        assert torch.equal(mean.grad, 2.0 * first.d_mean) and torch.equal(value.grad, 2.0 * first.d_value)
        assert torch.equal(prm.grad, 2.0 * first.d_param)


# ---------------------------------------------------------------------------------------------- gate 3
def ppo_run(monkeypatch, graph, fused_loss, mode=None, priv=False, fused_learner=False, precision="fp32",
            std_type="scalar"):
    from h12env import cfg as K
    from h12env.ppo import PPO, ActorCritic

    monkeypatch.setenv("H12_PPO_GRAPH", "1" if graph else "0")
    torch.manual_seed(7)
    pol = ActorCritic(270, 65 if priv else 270, 12, [128, 64], [128, 64], noise_std_type=std_type)
    sym = None
    if mode is not None:
        sym = {"use_data_augmentation": True, "use_mirror_loss": mode == "both", "mirror_loss_coeff": 0.5,
               "data_augmentation_func": "h12env.symmetry:augment", "_env": K.H12RslEnvCfg()}
    alg = PPO(pol, num_learning_epochs=2, num_mini_batches=4, learning_rate=1e-3, schedule="adaptive", desired_kl=0.01,
              device=DEV, symmetry_cfg=sym, fused_learner=fused_learner, fused_loss=fused_loss, precision=precision)
    alg.init_storage(64, 24, [270], [65] if priv else None, [12])  # 1536 rows, minibatches of 384
    out = []
    for u in range(2):
        g = torch.Generator(device=DEV).manual_seed(100 + u)
        for k, v in alg.storage.t.items():
            v.copy_(torch.randn(v.shape, generator=g, device=DEV) * (0.1 if k == "sigma" else 1.0))
        alg.storage.t["sigma"].abs_().add_(0.5)
        out.append(alg.update())
    return alg, out


@pytest.mark.parametrize("mode,priv,learner", [(None, False, False), ("both", False, False), (None, True, False),
                                               (None, False, True)])
def test_graph_captured_fused_loss_update_equals_eager(gpu, monkeypatch, mode, priv, learner):
    calls = []
    orig = _learn.ppo_head
    monkeypatch.setattr(_learn, "ppo_head", lambda *a, **k: (calls.append(k), orig(*a, **k))[1])
    a, la = ppo_run(monkeypatch, True, True, mode, priv, learner)
    in_graph = len(calls)
    b, lb = ppo_run(monkeypatch, False, True, mode, priv, learner)
    assert in_graph == 3 and len(calls) - in_graph == 2 * 8  # warm-up x 2 + capture; 2 updates x 8 minibatches
    # one rank on the device: the fold runs the schedule; it adds the statistics where torch adds no fourth one
    assert all(k["lr"] is x._lr_t for k, x in zip((calls[0], calls[-1]), (a, b)))
    assert all((k["stats_accum"] is None) is (mode is not None) for k in calls)
    assert a._graph is not None and b._graph is None and a.fused_loss and b.fused_loss
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.isfinite(p).all() and torch.equal(p, q), (p - q).abs().max()
    assert la == lb and a.learning_rate == b.learning_rate and a.learning_rate != 1e-3
    assert all(math.isfinite(v) for x in la for v in x.values())
    if mode is None and not priv and not learner:
        # the default path never reaches the kernel, and the two paths agree to rounding over two updates
        n_before = len(calls)
        d, ld = ppo_run(monkeypatch, True, False)
        assert len(calls) == n_before and not d.fused_loss
        assert list(a.policy.state_dict()) == list(d.policy.state_dict())
        for x, y in zip(la, ld):
            for key in x:
                assert abs(x[key] - y[key]) <= 1e-3 * max(1.0, abs(y[key])), (key, x, y)


@pytest.mark.parametrize("precision,std_type,mode", [("bf16", "scalar", None), ("fp32", "log", "augment")])
def test_bf16_learner_and_log_std_with_the_switch_on(gpu, monkeypatch, precision, std_type, mode):
    """The head receives the .float() outputs of the bf16 learner; log_std goes through the kernel's other std kind
    (here with augmentation without the mirror loss).  Captured == eager bit for bit, as on the other paths."""
    calls = []
    orig = _learn.ppo_head
    monkeypatch.setattr(_learn, "ppo_head", lambda *a, **k: (calls.append(a[3]), orig(*a, **k))[1])
    a, la = ppo_run(monkeypatch, True, True, mode, precision=precision, std_type=std_type)
    b, lb = ppo_run(monkeypatch, False, True, mode, precision=precision, std_type=std_type)
    assert len(calls) == 3 + 16 and set(calls) == {_learn.PPO_STD_LOG if std_type == "log" else _learn.PPO_STD_SCALAR}
    assert a.fused_loss and b.fused_loss and a._graph is not None and a.precision == precision
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.isfinite(p).all() and torch.equal(p, q)
    assert la == lb and a.learning_rate == b.learning_rate and a.learning_rate != 1e-3
    assert all(math.isfinite(v) for x in la for v in x.values())


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

    def make(fused_loss):
        torch.manual_seed(11)
        pol = ActorCritic(270, 270, 12, [512, 256, 128], [512, 256, 128])
        alg = PPO(pol, num_mini_batches=4, schedule="fixed", max_grad_norm=float("inf"), entropy_coef=0.01,
                  device=DEV, fused_loss=fused_loss)
        alg.init_storage(64, 24, [270], None, [12])
        g = torch.Generator(device=DEV).manual_seed(5)
        t = alg.storage.t
        rnd = lambda k, s=1.0: torch.randn(t[k].shape, generator=g, device=DEV) * s  # noqa: E731
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
    idx = torch.randperm(1536, generator=torch.Generator().manual_seed(9))[:384].to(DEV)
    pol64 = copy.deepcopy(default.policy).double()
    loss_fp64(pol64, default, b, idx).backward()
    ref = {k: p.grad for k, p in pol64.named_parameters()}
    grads = {}
    assert fused.fused_loss and not default.fused_loss
    assert all(torch.equal(p, q) for p, q in zip(fused.policy.parameters(), default.policy.parameters()))
    for name, alg in (("fused", fused), ("default", default)):
        alg._minibatch(alg._batch(), idx, torch.zeros(3, device=DEV))
        grads[name] = {k: p.grad.clone() for k, p in alg.policy.named_parameters()}
    for k, r in ref.items():
        ef = float((grads["fused"][k].double() - r).abs().max())
        ed = float((grads["default"][k].double() - r).abs().max())
        gmax = float(r.abs().max())
        print(f"GRAD {k}: max|grad| {gmax:.3e}  fused-loss error {ef:.3e}  default error {ed:.3e}")
    for k, r in ref.items():
        ef = float((grads["fused"][k].double() - r).abs().max())
        ed = float((grads["default"][k].double() - r).abs().max())
        gmax = float(r.abs().max())
        assert gmax > 0 and ef <= FACTOR * ed + U * gmax, (k, ef, ed, gmax)


def test_train_script_with_fused_loss(gpu, tmp_path):
    train = ROOT / "h1v2-isaac_amd" / "scripts" / "train.py"
    task = "Isaac-Velocity-Flat-H12_12dof-v0"
    r = subprocess.run([sys.executable, str(train), "--task", task, "--headless", "--num_envs", "64",
                        "--max_iterations", "2", "--fused_loss", "agent.save_interval=1"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    run = next((tmp_path / "logs" / "rsl_rl" / "h12_12dof_flat").iterdir())
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2
    assert all(math.isfinite(v) for x in lines for v in x.values() if isinstance(v, float))
    assert "fused_loss: true" in (run / "params" / "agent.yaml").read_text()
    ck = run / "model_2.pt"
    assert ck.exists()

    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    cfg.scene.num_envs = 64
    cfg.sim.device = DEV
    agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    agent.device = DEV
    env = RslRlVecEnvWrapper(gym.make(task, cfg=cfg))
    runner = OnPolicyRunner(env, agent.to_dict(), log_dir=None, device=DEV)
    assert not runner.alg.fused_loss
    runner.load(str(ck))
    saved = torch.load(ck, map_location=DEV, weights_only=True)["model_state_dict"]
    assert list(saved) == list(runner.alg.policy.state_dict())
    for k, v in runner.alg.policy.state_dict().items():
        assert torch.equal(v, saved[k]) and torch.isfinite(v).all(), k
    runner.learn(1)  # the default path trains on from the fused-loss run's parameters and optimizer state
    env.close()
