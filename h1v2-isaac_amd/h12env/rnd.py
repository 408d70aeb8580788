"""Random Network Distillation (rsl_rl 2.3 ``rnd_cfg``): curiosity-driven exploration.  A fixed,
randomly initialised ``target`` network embeds the ``rnd_state`` observation group; a ``predictor`` is trained to match
it; the norm of their difference is an intrinsic reward that is large where the predictor has seen little data.

rsl-rl-lib 2.3.3 (modules/rnd.py, modules/normalizer.py) is restated here -- the package is not importable offline.
Deviations are listed in DESIGN.md section 9: schedule values are taken as given (only the initial ``weight`` is
multiplied by the env's step_dt, by the runner), and the reward normaliser's per-env discounted average is never reset
on a done.

``RandomNetworkDistillation`` is the torch path (and the CPU path).  ``FusedRND`` runs the per-env-step work of
``get_intrinsic_reward`` and the reward sum of ``PPO.process_env_step`` in two HIP launches (csrc/h12_rnd.hip); it is
opt-in: ``rnd_cfg["fused"] = True``, ``train.py --rnd_fused`` or ``H12_RND_FUSED=1``.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

RND_KEYS = ("weight", "weight_schedule", "reward_normalization", "state_normalization", "learning_rate", "num_outputs",
            "predictor_hidden_dims", "target_hidden_dims", "activation", "num_states", "fused")
SCHEDULE_KEYS = {"constant": (), "step": ("final_step", "final_value"),
                 "linear": ("initial_step", "final_step", "final_value")}


def rnd_fused_enabled() -> bool:
    """H12_RND_FUSED=1: the intrinsic-reward step of the collection loop runs on the h12learn_rnd_* kernels."""
    return os.environ.get("H12_RND_FUSED", "0") == "1"


def check_schedule(schedule):
    """ValueError for a weight_schedule that is not None or a dict with a known mode and exactly that mode's keys."""
    if schedule is None:
        return
    if not isinstance(schedule, dict) or "mode" not in schedule:
        raise ValueError(f"rnd_cfg.weight_schedule must be None or a dict with a 'mode', got {schedule!r}")
    mode = schedule["mode"]
    if mode not in SCHEDULE_KEYS:
        raise ValueError(f"rnd_cfg.weight_schedule: unknown mode {mode!r} (one of {sorted(SCHEDULE_KEYS)})")
    keys = set(schedule) - {"mode"}
    if keys != set(SCHEDULE_KEYS[mode]):
        raise ValueError(f"rnd_cfg.weight_schedule mode {mode!r} takes the keys {SCHEDULE_KEYS[mode]}, got "
                         f"{sorted(keys)}")
    if mode == "linear" and not schedule["final_step"] > schedule["initial_step"]:
        raise ValueError("rnd_cfg.weight_schedule: linear needs final_step > initial_step")


def scheduled_weight(initial: float, schedule, step: int) -> float:
    """The intrinsic-reward weight at ``step`` (the module's update_counter).  None / constant: ``initial``.  step:
    ``initial`` while step < final_step, then final_value.  linear: ``initial`` up to initial_step, final_value from
    final_step on, a straight line in between.  The schedule's values are taken as given: only ``initial`` carries the
    runner's step_dt factor."""
    if schedule is None or schedule["mode"] == "constant":
        return float(initial)
    if schedule["mode"] == "step":
        return float(initial) if step < schedule["final_step"] else float(schedule["final_value"])
    s0, s1, final = schedule["initial_step"], schedule["final_step"], float(schedule["final_value"])
    if step <= s0:
        return float(initial)
    if step >= s1:
        return final
    return float(initial) + (final - float(initial)) * (step - s0) / (s1 - s0)


def check_rnd_cfg(rnd_cfg: dict):
    unknown = sorted(set(rnd_cfg) - set(RND_KEYS))
    if unknown:
        raise ValueError(f"rnd_cfg: unknown keys {unknown} (known: {RND_KEYS})")
    check_schedule(rnd_cfg.get("weight_schedule"))


def resolve_rnd_cfg(rnd_cfg: dict, env, observations: dict) -> dict:
    """What rsl_rl's runner does to ``rnd_cfg``: num_states from the width of the env's ``rnd_state`` observation group
    and ``weight`` multiplied by the env's step_dt, once.  ValueError without the group."""
    check_rnd_cfg(rnd_cfg)
    state = observations.get("rnd_state")
    if state is None:
        raise ValueError("rnd_cfg needs the observation group 'rnd_state' (extras['observations']['rnd_state']); "
                         "set env_cfg.observations.rnd_state = RndStateObsCfg() (train.py --rnd)")
    out = dict(rnd_cfg)
    out["num_states"] = int(state.shape[1])
    out["weight"] = float(out.get("weight", 0.0)) * float(env.unwrapped.step_dt)
    return out


class EmpiricalDiscountedVariationNormalization(nn.Module):
    """rsl_rl's reward normaliser of RND: x / std of a discounted per-env sum of x.  In training mode a call first sets
    ``avg = x`` (the first call) or ``avg = avg * gamma + x`` per env -- never reset on a done --, then folds the
    batch mean and population variance of ``avg`` (batch axis: the envs) into the scalar running statistics by
    ppo.EmpiricalNormalization's rule while ``count < until``.  The result is ``x / std`` where ``std > 0``, else x:
    no mean is subtracted and ``eps`` is unused.  Every decision is taken on the device (no host sync)."""

    def __init__(self, shape=(), eps=1e-2, gamma=0.99, until=None):
        super().__init__()
        if list(shape):
            raise ValueError("EmpiricalDiscountedVariationNormalization: scalar statistics only (shape=[])")
        self.eps, self.gamma, self.until = eps, gamma, until
        self.register_buffer("_mean", torch.zeros(1))
        self.register_buffer("_var", torch.ones(1))
        self.register_buffer("_std", torch.ones(1))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))
        self.register_buffer("avg", torch.zeros(0))
        self.register_buffer("first", torch.ones(1, dtype=torch.int32))

    def ensure(self, n: int, device):
        """The per-env average as an ordinary [n] tensor (the collection loop runs in inference mode)."""
        if self.avg.numel() != n or self.avg.device != torch.device(device):
            with torch.inference_mode(False):
                self.avg = torch.zeros(n, device=device, dtype=self._mean.dtype)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        v = state_dict.get(prefix + "avg")
        if v is not None and v.shape != self.avg.shape:
            with torch.inference_mode(False):
                self.avg = torch.zeros(v.shape, device=self.avg.device, dtype=self._mean.dtype)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    @torch.no_grad()
    def update(self, x):
        n = x.shape[0]
        self.ensure(n, x.device)
        self.avg.copy_(torch.where(self.first != 0, x, self.avg * self.gamma + x))
        self.first.zero_()
        live = self.count < self.until if self.until is not None else torch.ones((), dtype=torch.bool, device=x.device)
        var_x = torch.var(self.avg, dim=0, unbiased=False, keepdim=True)
        mean_x = torch.mean(self.avg, dim=0, keepdim=True)
        count = self.count + n
        rate = n / count
        delta = mean_x - self._mean
        mean = self._mean + rate * delta
        var = self._var + rate * (var_x - self._var + delta * (mean_x - mean))
        self.count.copy_(torch.where(live, count, self.count))
        self._mean.copy_(torch.where(live, mean, self._mean))
        self._var.copy_(torch.where(live, var, self._var))
        self._std.copy_(torch.where(live, torch.sqrt(var), self._std))

    def forward(self, x):
        if self.training:
            self.update(x)
        return torch.where(self._std > 0, x / self._std, x)


class RandomNetworkDistillation(nn.Module):
    """rsl_rl's RandomNetworkDistillation.  ``predictor`` and ``target`` are nn.Sequential of Linear and activation
    layers (state-dict keys predictor.{0,2,..}.weight|bias, target....); the target is never trained and stays in eval
    mode.  ``get_intrinsic_reward(rnd_state)`` is called once per env step."""

    def __init__(self, num_states: int, num_outputs: int = 1, predictor_hidden_dims=(-1,), target_hidden_dims=(-1,),
                 activation: str = "elu", weight: float = 0.0, state_normalization: bool = False,
                 reward_normalization: bool = False, weight_schedule: dict | None = None, device="cpu", **kwargs):
        super().__init__()
        from .ppo import EmpiricalNormalization, mlp

        if kwargs:
            raise ValueError(f"RandomNetworkDistillation: unknown arguments {sorted(kwargs)}")
        check_schedule(weight_schedule)
        self.num_states, self.num_outputs = int(num_states), int(num_outputs)
        self.initial_weight = float(weight)
        self.weight_schedule = None if weight_schedule is None else dict(weight_schedule)
        self.state_normalization, self.reward_normalization = bool(state_normalization), bool(reward_normalization)
        dims = lambda hs: [self.num_states if h == -1 else int(h) for h in hs]  # noqa: E731
        self.predictor = mlp(self.num_states, dims(predictor_hidden_dims), self.num_outputs, activation)
        self.target = mlp(self.num_states, dims(target_hidden_dims), self.num_outputs, activation)
        self.target.requires_grad_(False)
        self.state_normalizer = (EmpiricalNormalization([self.num_states], until=1.0e8) if self.state_normalization
                                 else nn.Identity())
        self.reward_normalizer = (EmpiricalDiscountedVariationNormalization([], until=1.0e8)
                                  if self.reward_normalization else nn.Identity())
        self.update_counter = 0
        self.to(device)
        self.target.eval()

    @property
    def weight(self) -> float:
        """The weight the last get_intrinsic_reward applied (the initial one before the first)."""
        return scheduled_weight(self.initial_weight, self.weight_schedule, self.update_counter)

    def train(self, mode: bool = True):
        super().train(mode)
        self.target.eval()
        return self

    def forward(self, *args, **kwargs):
        raise RuntimeError("RandomNetworkDistillation: call get_intrinsic_reward()")

    @torch.no_grad()
    def get_intrinsic_reward(self, rnd_state):
        """(intrinsic reward [n], normalised state [n][num_states]); the rollout stores the normalised state."""
        self.update_counter += 1
        s = self.state_normalizer(rnd_state)
        e = torch.linalg.norm(self.target(s) - self.predictor(s), dim=1)
        e = self.reward_normalizer(e)
        return e * self.weight, s

    def rnd_state_dict(self) -> dict:
        """Checkpoint entry: both networks, both normalisers with their counts and the per-env average, and the
        update counter."""
        return {"module": self.state_dict(), "update_counter": int(self.update_counter)}

    def load_rnd_state_dict(self, d: dict):
        self.load_state_dict(d["module"])
        self.update_counter = int(d["update_counter"])
        self.target.eval()


class FusedRND:
    """The per-env-step work of RND on the device in two launches: h12learn_rnd_reward (state normaliser applied,
    target, predictor, row norm) and h12learn_rnd_finish (reward normaliser, weight, extrinsic + intrinsic).  It shares
    the module's parameters and buffers: the torch path can take over at any step.  The state normaliser's running update
    stays the torch ``update()``; only its application is fused.  Linear/ELU networks within the kernel's width limit
    only (ValueError otherwise).  On CPU tensors the module's torch path runs."""

    def __init__(self, rnd: RandomNetworkDistillation):
        from .policy import FusedMLP

        self.rnd = rnd
        try:
            self._mlp = FusedMLP([rnd.predictor, rnd.target], rnd.state_normalizer if rnd.state_normalization else None)
        except ValueError as e:
            raise ValueError(f"rnd_cfg fused: the RND networks cannot run on the fused kernels (Linear/ELU only, every "
                             f"width at most the kernels' maximum): {e}") from e
        self._weight = None
        self._weight_value = None
        self._args = None
        self._args_key = None
        self.dirty = True  # the predictor changed since the last pack

    def __call__(self, rnd_state: torch.Tensor, ext_reward: torch.Tensor):
        """(intrinsic [n], extrinsic + intrinsic [n], normalised state [n][num_states])."""
        from . import _learn

        rnd = self.rnd
        # CPU tensors, or a reward normaliser in eval mode (it then leaves its per-env average alone, which the finish
        # kernel does not): the module's own path
        if not rnd_state.is_cuda or (rnd.reward_normalization and not rnd.reward_normalizer.training):
            intrinsic, s = rnd.get_intrinsic_reward(rnd_state)
            return intrinsic, ext_reward + intrinsic, s
        rnd.update_counter += 1
        x = rnd_state.detach().contiguous()
        ext = ext_reward.detach().contiguous()
        n, dev = x.shape[0], x.device
        if rnd.state_normalization and rnd.state_normalizer.training:
            rnd.state_normalizer.update(x)
        m = self._mlp
        before = m._desc
        desc = m._describe()
        if self.dirty or desc is not before:
            _learn.mlp_pack(desc, m._packed)
            self.dirty = False
        with torch.inference_mode(False):
            if self._weight is None or self._weight.device != dev:
                self._weight = torch.zeros(1, device=dev)
                self._weight_value = None
            if getattr(self, "_n", None) != n:
                self._err, self._xn = torch.empty(n, device=dev), torch.empty(n, rnd.num_states, device=dev)
                self._intrinsic, self._total = torch.empty(n, device=dev), torch.empty(n, device=dev)
                self._n = n
        w = rnd.weight
        if w != self._weight_value:  # a launch only when the schedule moved it
            self._weight.fill_(w)
            self._weight_value = w
        _learn.rnd_reward(desc, m._packed, x, err=self._err, xn=self._xn)
        a = _learn.RndFinishArgs()
        a.n, a.err, a.ext_reward, a.weight = n, self._err.data_ptr(), ext.data_ptr(), self._weight.data_ptr()
        a.intrinsic, a.total = self._intrinsic.data_ptr(), self._total.data_ptr()
        if rnd.reward_normalization:
            rn = rnd.reward_normalizer
            rn.ensure(n, dev)
            a.normalize = 1
            a.gamma = float(rn.gamma)
            a.until = int(rn.until) if rn.until is not None else 2 ** 62
            a.avg, a.mean, a.var, a.std = (t.data_ptr() for t in (rn.avg, rn._mean, rn._var, rn._std))
            a.count, a.first = rn.count.data_ptr(), rn.first.data_ptr()
        _learn.rnd_finish(a, dev)
        return self._intrinsic, self._total, self._xn
