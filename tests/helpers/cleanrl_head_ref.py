"""The CleanRL loss head restated (include/h12learn.h, h12learn_cleanrl_head): the data of the GPU
tests and ``restated(case, dtype, device)``, which evaluates the header's expressions with torch in ``dtype`` on copies of
the case's fp32 tensors and differentiates them with autograd.  float64 is the reference, float32 on the device the
yardstick (the default path's arithmetic)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

VALUE_MEAN, VALUE_VAR, VALUE_EPS = 1.7, 2.3, 1e-8
# csrc/h12_ppo_head.hip: the blocks the fold stages at a time, and the advantage partials a row block stages at a time;
# the depth shapes of the GPU test lie one block past each (tests/test_cleanrl_head_api.py pins both to the source)
FOLD_CHUNK, MERGE_CHUNK = 128, 256


def make_case(m, A, use_idx=True, norm_adv=True, clip_vloss=True, adv_shift=0.3, seed=0, clip=0.2):
    """A minibatch on the CPU (fp32) whose rows fall on every side of both clip ranges.  With ``use_idx`` the rollout has
    n_src = 3 m + 5 rows and idx holds 0, n_src - 1 and a duplicate where m allows; without it n_src = m."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * m + A)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    n_src = 3 * m + 5 if use_idx else m
    logstd = (0.5 + 0.7 * torch.rand(A, generator=g)).log()
    sigma = logstd.exp()
    idx = None
    if use_idx:
        idx = torch.randint(0, n_src, (m,), generator=g)
        idx[0] = 0
        idx[m - 1] = n_src - 1
        if m >= 4:
            idx[2] = idx[1]
    k = idx if use_idx else torch.arange(m)
    actions = rn(n_src, A)
    mean = actions[k] - sigma * rn(m, A)
    s64 = sigma.double()
    lp = (-(actions[k].double() - mean.double()).square() / (2 * s64.square()) - logstd.double()
          - math.log(math.sqrt(2 * math.pi))).sum(-1)
    old_log_prob = rn(n_src) * 0.5 - 1.4 * A
    old_log_prob[k] = (lp + 0.25 * rn(m).double()).float()
    values_n = rn(n_src)
    sd = math.sqrt(VALUE_VAR + VALUE_EPS)
    value = (values_n[k] + 0.3 * rn(m)) * sd + VALUE_MEAN  # the critic's raw output: normalised, it is near values_n
    t = dict(mean=mean.contiguous(), value=value, logstd=logstd, old_log_prob=old_log_prob,
             advantages=adv_shift + rn(n_src), returns_n=values_n + 0.5 * rn(n_src), values_n=values_n,
             actions=actions.contiguous(), value_mean=torch.tensor(VALUE_MEAN), value_var=torch.tensor(VALUE_VAR))
    return SimpleNamespace(m=m, A=A, n_src=n_src, idx=idx, k=k, norm_adv=norm_adv, clip_vloss=clip_vloss, clip=clip,
                           ecoef=0.0081, vcoef=2.0, veps=VALUE_EPS, t=t)


def restated(c, dtype, device):
    """out [5] = (pg loss, entropy, v loss, total, clip fraction), the three gradients, and what the branches turn on."""
    t = {n: v.to(device=device, dtype=dtype) for n, v in c.t.items()}
    mean, value, logstd = (t[n].requires_grad_(True) for n in ("mean", "value", "logstd"))
    k = c.k.to(device)
    sigma = torch.exp(logstd)
    log_prob = (-(t["actions"][k] - mean).square() / (2 * sigma.square()) - logstd
                - math.log(math.sqrt(2 * math.pi))).sum(-1)
    ratio = torch.exp(log_prob - t["old_log_prob"][k])
    clip_rows = ((ratio - 1.0).abs() > c.clip).to(dtype)
    adv = t["advantages"][k]
    if c.norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)  # torch.std: correction 1
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - c.clip, 1 + c.clip)).mean()
    nv = (value - t["value_mean"]) / torch.sqrt(t["value_var"] + c.veps)
    ret, vn = t["returns_n"][k], t["values_n"][k]
    q1 = (nv - ret).square()
    q2 = (vn + torch.clamp(nv - vn, -c.clip, c.clip) - ret).square()
    v = 0.5 * (torch.max(q1, q2) if c.clip_vloss else q1).mean()
    entropy = (0.5 + 0.5 * math.log(2 * math.pi) + logstd).sum()
    loss = pg - c.ecoef * entropy + c.vcoef * v
    loss.backward()
    out = torch.stack([pg, entropy, v, loss, clip_rows.mean()]).detach()
    return SimpleNamespace(out=out, d_mean=mean.grad, d_value=value.grad, d_logstd=logstd.grad, ratio=ratio.detach(),
                           adv=adv.detach(), dv=(nv - vn).detach(), q1=q1.detach(), q2=q2.detach(),
                           clip_rows=clip_rows.detach())
