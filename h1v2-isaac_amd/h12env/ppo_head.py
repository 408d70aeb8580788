"""The PPO loss head as one autograd node.

``PPOHead`` takes the networks' outputs of a minibatch -- the actor's mean, the critic's value, the std parameter -- and
returns the scalar loss ``surrogate + value_loss_coef * value_loss - entropy_coef * entropy`` of ``PPO._minibatch``
together with ``out`` = (surrogate loss, value loss, entropy mean, KL mean, total loss).  On CUDA tensors the forward is
one ``h12learn_ppo_head`` call (csrc/h12_ppo_head.hip: two launches), which gathers the rollout's per-sample tensors
itself, applies the adaptive learning-rate rule and accumulates the statistics when asked to, and leaves the three
gradients for the backward.  On CPU tensors the same node evaluates ``_minibatch``'s torch expressions and
differentiates them with autograd, so it is bit-identical to the default path there.

``CleanRLHead`` is the same construction for the CleanRL trainer (h12env/cleanrl.py): the block of
``cleanrl.PPO`` from ``logratio`` to ``loss`` over (mean, value, actor_logstd), ``out`` = (pg loss, entropy, v loss, total
loss, clip fraction), one ``h12learn_cleanrl_head`` call on CUDA tensors and ``torch_cleanrl_head`` on CPU tensors."""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch.autograd.function import once_differentiable
from torch.distributions import Normal

from . import _learn

STD_KINDS = {"scalar": _learn.PPO_STD_SCALAR, "log": _learn.PPO_STD_LOG}


def fused_loss_enabled() -> bool:
    """H12_PPO_HEAD_FUSED=1: ppo.PPO computes the loss head with PPOHead."""
    import os

    return os.environ.get("H12_PPO_HEAD_FUSED", "0") == "1"


@dataclass
class HeadInputs:
    """What the head reads besides the networks' outputs.  The rollout tensors are the storage's flattened tensors
    (n_src rows) and ``idx`` the minibatch's rows of them; ``actions`` is such a tensor too, or, with ``actions_direct``,
    the [m][A] actions already gathered (and mirrored).  m is idx.shape[0], or twice that under data augmentation."""
    idx: torch.Tensor
    old_log_prob: torch.Tensor
    advantages: torch.Tensor
    returns: torch.Tensor
    target_values: torch.Tensor
    old_mu: torch.Tensor
    old_sigma: torch.Tensor
    actions: torch.Tensor
    actions_direct: bool
    std_kind: str
    clip_param: float
    value_loss_coef: float
    entropy_coef: float
    use_clipped_value_loss: bool
    lr: torch.Tensor | None = None  # CUDA only: the device scalar the fold's schedule rewrites
    desired_kl: float | None = None
    stats_accum: torch.Tensor | None = None  # CUDA only: value loss, surrogate, entropy are added to its first three


def torch_head(mean, value, std_param, h: HeadInputs):
    """``PPO._minibatch``'s expressions, operation for operation: (loss, out)."""
    idx = h.idx
    n_orig = idx.shape[0]
    aug = mean.shape[0] != n_orig
    actions = h.actions if h.actions_direct else h.actions[idx]
    target_values = h.target_values[idx]
    advantages = h.advantages[idx]
    returns = h.returns[idx]
    old_log_prob = h.old_log_prob[idx]
    old_mu, old_sigma = h.old_mu[idx], h.old_sigma[idx]
    if aug:
        old_log_prob, target_values, advantages, returns = (torch.cat([t, t]) for t in
                                                            (old_log_prob, target_values, advantages, returns))
    s = std_param if h.std_kind == "scalar" else torch.exp(std_param)
    dist = Normal(mean, s.expand_as(mean))
    log_prob = dist.log_prob(actions).sum(dim=-1)
    mu, sigma, entropy = dist.mean, dist.stddev, dist.entropy().sum(dim=-1)
    if aug:
        mu, sigma, entropy = mu[:n_orig], sigma[:n_orig], entropy[:n_orig]
    with torch.no_grad():
        kl = torch.sum(torch.log(sigma / old_sigma + 1e-5)
                       + (old_sigma.square() + (old_mu - mu).square()) / (2.0 * sigma.square()) - 0.5, dim=-1)
        kl_mean = kl.mean()
    ratio = torch.exp(log_prob - old_log_prob.squeeze(-1))
    adv = advantages.squeeze(-1)
    surrogate = -adv * ratio
    surrogate_clipped = -adv * torch.clamp(ratio, 1.0 - h.clip_param, 1.0 + h.clip_param)
    surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
    if h.use_clipped_value_loss:
        v_clipped = target_values + (value - target_values).clamp(-h.clip_param, h.clip_param)
        value_loss = torch.max((value - returns).square(), (v_clipped - returns).square()).mean()
    else:
        value_loss = (returns - value).square().mean()
    entropy_mean = entropy.mean()
    loss = surrogate_loss + h.value_loss_coef * value_loss - h.entropy_coef * entropy_mean
    out = torch.stack([surrogate_loss.detach(), value_loss.detach(), entropy_mean.detach(), kl_mean, loss.detach()])
    return loss, out


class _Head(torch.autograd.Function):
    """The autograd node both heads are.  A head supplies ``device(mean, value, param, h)``, the HIP call, returning
    (d_mean, d_value, d_param, out, index of the loss in out), and ``restated(mean, value, param, h)``, its torch
    restatement looked up on this module when called, returning (loss, out).  The forward runs ``device`` on CUDA tensors
    and ``restated``, differentiated under enable_grad, on CPU tensors; it saves the three gradients and returns
    (loss, out) with ``out`` non-differentiable.  The backward scales the saved gradients by the incoming one."""

    @classmethod
    def forward(cls, ctx, mean, value, param, h):
        if mean.is_cuda:
            d_mean, d_value, d_param, out, i_loss = cls.device(mean, value, param, h)
            loss = out[i_loss].clone()
            d_value, d_param = d_value.view_as(value), d_param.view_as(param)
        else:
            leaves = [t.detach().requires_grad_(True) for t in (mean, value, param)]
            with torch.enable_grad():
                loss, out = cls.restated(*leaves, h)
                d_mean, d_value, d_param = torch.autograd.grad(loss, leaves)
            loss = loss.detach()
        ctx.save_for_backward(d_mean, d_value, d_param)
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_out):
        d_mean, d_value, d_param = ctx.saved_tensors
        return g * d_mean, g * d_value, g * d_param, None


class PPOHead(_Head):
    """(loss, out) = PPOHead.apply(mean [m][A], value [m][1], std_param [A], HeadInputs).  ``out`` carries no
    gradient; the backward returns the three gradients the forward computed, scaled by the incoming gradient."""

    @staticmethod
    def device(mean, value, std_param, h: HeadInputs):
        flat = lambda t: t.reshape(-1)  # noqa: E731  ([n_src][1] storage columns; contiguous views)
        return (*_learn.ppo_head(
            mean, value, std_param, STD_KINDS[h.std_kind], h.idx, h.idx.shape[0], flat(h.old_log_prob),
            flat(h.advantages), flat(h.returns), flat(h.target_values), h.old_mu, h.old_sigma, h.actions,
            h.actions_direct, h.clip_param, h.value_loss_coef, h.entropy_coef, h.use_clipped_value_loss, lr=h.lr,
            desired_kl=h.desired_kl, stats_accum=h.stats_accum), 4)

    @staticmethod
    def restated(mean, value, std_param, h: HeadInputs):
        return torch_head(mean, value, std_param, h)


# ---------------------------------------------------------------------------------------------- CleanRL
def cleanrl_fused_loss_enabled() -> bool:
    """H12_CLEANRL_HEAD_FUSED=1: cleanrl.PPO computes the loss head with CleanRLHead."""
    import os

    return os.environ.get("H12_CLEANRL_HEAD_FUSED", "0") == "1"


@dataclass
class CleanRLInputs:
    """What the CleanRL head reads besides the networks' outputs: the minibatch's rows ``idx`` of the flattened rollout
    tensors (n_src rows each; returns_n and values_n are normalised by value_rms), the agent's ``value_rms`` module
    (read, never updated) and the trainer's coefficients."""
    idx: torch.Tensor
    old_log_prob: torch.Tensor
    advantages: torch.Tensor
    returns_n: torch.Tensor
    values_n: torch.Tensor
    actions: torch.Tensor
    value_rms: torch.nn.Module
    clip_coef: float
    ent_coef: float
    vf_coef: float
    norm_adv: bool
    clip_vloss: bool
    stats_accum: torch.Tensor | None = None  # CUDA only: ``out`` is added to its five elements


def torch_cleanrl_head(mean, value, logstd, h: CleanRLInputs):
    """``cleanrl.PPO``'s minibatch from the networks' outputs to the loss, operation for operation (the Normal of
    ``Agent.get_action_and_value`` included): (loss, out)."""
    mb_inds = h.idx
    action_logstd = logstd.expand_as(mean)
    action_std = torch.exp(action_logstd)
    probs = Normal(mean, action_std, validate_args=None if not mean.is_cuda else False)
    newlogprob, entropy = probs.log_prob(h.actions[mb_inds]).sum(1), probs.entropy().sum(1)
    logratio = newlogprob - h.old_log_prob[mb_inds]
    ratio = logratio.exp()
    with torch.no_grad():
        clipfrac = ((ratio - 1.0).abs() > h.clip_coef).float().mean()

    mb_advantages = h.advantages[mb_inds]
    if h.norm_adv:
        mb_advantages = (mb_advantages - mb_advantages.mean()) / (mb_advantages.std() + 1e-8)

    pg_loss1 = -mb_advantages * ratio
    pg_loss2 = -mb_advantages * torch.clamp(ratio, 1 - h.clip_coef, 1 + h.clip_coef)
    pg_loss = torch.max(pg_loss1, pg_loss2).mean()

    newvalue = h.value_rms(value.view(-1), update=False)
    if h.clip_vloss:
        v_loss_unclipped = (newvalue - h.returns_n[mb_inds]) ** 2
        v_clipped = h.values_n[mb_inds] + torch.clamp(newvalue - h.values_n[mb_inds], -h.clip_coef, h.clip_coef)
        v_loss_clipped = (v_clipped - h.returns_n[mb_inds]) ** 2
        v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
    else:
        v_loss = 0.5 * ((newvalue - h.returns_n[mb_inds]) ** 2).mean()

    entropy_loss = entropy.mean()
    loss = pg_loss - h.ent_coef * entropy_loss + v_loss * h.vf_coef
    out = torch.stack([pg_loss.detach(), entropy_loss.detach(), v_loss.detach(), loss.detach(), clipfrac])
    return loss, out


class CleanRLHead(_Head):
    """(loss, out) = CleanRLHead.apply(mean [m][A], value [m][1], actor_logstd [1][A], CleanRLInputs).  ``out`` carries
    no gradient; the backward returns the three gradients the forward computed, scaled by the incoming gradient."""

    @staticmethod
    def device(mean, value, logstd, h: CleanRLInputs):
        rms = h.value_rms
        return (*_learn.cleanrl_head(
            mean, value, logstd, h.idx, h.old_log_prob, h.advantages, h.returns_n, h.values_n, h.actions,
            rms.running_mean, rms.running_var, rms.epsilon, h.clip_coef, h.ent_coef, h.vf_coef, h.norm_adv,
            h.clip_vloss, stats_accum=h.stats_accum), 3)

    @staticmethod
    def restated(mean, value, logstd, h: CleanRLInputs):
        return torch_cleanrl_head(mean, value, logstd, h)
