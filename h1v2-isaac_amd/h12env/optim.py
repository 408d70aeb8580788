"""Gradient clip and optimiser step as two HIP launches: ``FusedClipAdam`` and ``FusedClipRAdam``.

    opt = FusedClipRAdam(agent.parameters(), lr=lr_t, eps=1e-5, max_norm=0.5)
    loss.backward();  opt.step()            # no clip_grad_norm_ call: the clip is part of the step

Both are ``torch.optim.Optimizer`` subclasses over h12learn_optim_step (csrc/h12_optim.hip): launch 1 sums the squares of
every gradient in fp64 and counts the step, launch 2 forms the clip coefficient and the step's scalars (bias corrections,
RAdam's rho_t and rectification) in double and updates every parameter tensor and its moments.  include/h12learn.h has
the formulae: those of torch's ``Adam`` / ``RAdam`` with Python-float scalars, that is of the default, non-capturable
path; a captured step therefore takes the rectification branch that the eager default takes.

``optimizer.state[p]`` holds ``step`` (a float32 scalar tensor on the parameter's device), ``exp_avg`` and
``exp_avg_sq``, and the param groups carry the keys of torch's classes, so ``state_dict()`` / ``load_state_dict()``
interchange with ``torch.optim.Adam`` / ``torch.optim.RAdam`` in both directions and graphs.TrainingState restores the
state unchanged.  ``max_norm`` (None: no clip) is an attribute of the optimiser, not of a group: the norm is over every
parameter with a gradient.  ``p.grad`` is not rescaled in memory (a deviation from clip_grad_norm_: nothing reads it after
the step).  ``last_grad_norm`` is the norm of the last step as a scalar tensor on the parameters' device.

On CPU tensors ``step()`` runs ``clip_grad_norm_`` and torch's own functional single-tensor rule: bit for bit what
``clip_grad_norm_`` followed by ``torch.optim.Adam.step()`` / ``RAdam.step()`` does there.  A missing kernel is an
error; there is no fall-back from the HIP path."""
from __future__ import annotations

import os

import torch
from torch.optim import Optimizer


def fused_optimizer_enabled() -> bool:
    """H12_OPTIMIZER_FUSED=1: both trainers' ``fused_optimizer=None`` reads it."""
    return os.environ.get("H12_OPTIMIZER_FUSED", "0") == "1"


def _on_cuda(params) -> bool:
    for p in params:
        if torch.is_tensor(p):
            return p.is_cuda
        if isinstance(p, dict):
            return _on_cuda(p["params"] if not torch.is_tensor(p["params"]) else [p["params"]])
    return False


class _FusedClipBase(Optimizer):
    RULE = None  # _learn.OPTIM_*
    NAME = ""

    def __init__(self, params, defaults: dict, max_norm):
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError(f"{self.NAME}: max_norm = {max_norm} (a positive number, or None for no clip)")
        lr, (beta1, beta2), eps = defaults["lr"], defaults["betas"], defaults["eps"]
        if torch.is_tensor(lr):
            if lr.numel() != 1:
                raise ValueError(f"{self.NAME}: a tensor lr must have one element")
        elif not 0.0 <= lr:
            raise ValueError(f"{self.NAME}: lr = {lr} (must be >= 0)")
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"{self.NAME}: betas = {(beta1, beta2)} (each in [0, 1))")
        if not 0.0 < eps:
            raise ValueError(f"{self.NAME}: eps = {eps} (must be > 0)")
        super().__init__(params, defaults)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.last_grad_norm = None
        self._ws: dict = {}  # tensor sizes -> the kernels' workspace
        for g in self.param_groups:
            self._check_group(g)

    def _check_group(self, g: dict):
        for key in ("weight_decay", "amsgrad", "maximize", "differentiable", "decoupled_weight_decay"):
            if g.get(key):
                raise ValueError(f"{self.NAME}: {key} = {g[key]!r} is not supported")

    def load_state_dict(self, state_dict):
        """torch's, then every ``step`` as a float32 scalar on its parameter's device (torch's non-capturable optimisers
        keep theirs on the host)."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            self._check_group(g)
            for p in g["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).to(p.device).reshape(())

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _gather(self):
        """(params with a gradient, grads, exp_avgs, exp_avg_sqs, steps, the group they share the scalars of)."""
        params, grads, ms, vs, steps = [], [], [], [], []
        first = None
        for gi, g in enumerate(self.param_groups):
            self._check_group(g)
            if first is None:
                first = g
            elif any(g[k] is not first[k] and g[k] != first[k] for k in ("lr", "betas", "eps")):
                raise ValueError(f"{self.NAME}: param group {gi} differs from group 0 in lr, betas or eps; one step "
                                 "takes one set of scalars")
            for i, p in enumerate(g["params"]):
                if p.grad is None:
                    continue
                what = f"parameter {i} of group {gi} {tuple(p.shape)}"
                for name, t in (("", p), ("the gradient of ", p.grad)):
                    if t.is_sparse or t.dtype != torch.float32:
                        raise ValueError(f"{self.NAME}: {name}{what} is {t.dtype}{' sparse' if t.is_sparse else ''}; "
                                         "dense float32 is required")
                    if not t.is_contiguous():
                        raise ValueError(f"{self.NAME}: {name}{what} is not contiguous")
                if p.numel() < 1:
                    raise ValueError(f"{self.NAME}: {what} is empty")
                st = self._init_state(p)
                params.append(p), grads.append(p.grad), ms.append(st["exp_avg"]), vs.append(st["exp_avg_sq"])
                steps.append(st["step"])
        return params, grads, ms, vs, steps, first

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params, grads, ms, vs, steps, g = self._gather()
        if not params:
            return loss
        if any(p.is_cuda for p in params):
            if not all(p.is_cuda and p.device == params[0].device for p in params):
                raise ValueError(f"{self.NAME}: the parameters lie on more than one device")
            self._step_hip(params, grads, ms, vs, steps, g)
        else:
            self._step_cpu(params, grads, ms, vs, steps, g)
        return loss

    def _step_hip(self, params, grads, ms, vs, steps, g):
        from . import _learn

        dev = params[0].device
        key = (dev, tuple(p.numel() for p in params))
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty(_learn.optim_workspace_bytes(key[1]) // 8, dtype=torch.float64, device=dev)
        if self.last_grad_norm is None or self.last_grad_norm.device != dev:
            self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        lr = g["lr"]
        if torch.is_tensor(lr) and not (lr.is_cuda and lr.dtype == torch.float32):
            lr = float(lr)
        _learn.optim_step(self.RULE, params, grads, ms, vs, steps, g["betas"][0], g["betas"][1], g["eps"], self.max_norm,
                          lr, ws, self.last_grad_norm)

    def _step_cpu(self, params, grads, ms, vs, steps, g):
        if self.max_norm is not None:
            self.last_grad_norm = torch.nn.utils.clip_grad_norm_(params, self.max_norm)
        else:
            self.last_grad_norm = torch.nn.utils.get_total_norm(grads)
        self._rule_cpu(params, grads, ms, vs, steps, g)


class FusedClipAdam(_FusedClipBase):
    """``clip_grad_norm_(params, max_norm)`` and ``torch.optim.Adam.step()`` in two HIP launches."""
    NAME = "FusedClipAdam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 max_norm=None, maximize=False):
        from ._learn import OPTIM_ADAM

        self.RULE = OPTIM_ADAM
        params = list(params)
        cuda = _on_cuda(params)
        # torch.optim.Adam's keys, so that a state_dict loads there: on the device this step is a fused, capturable one
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                        maximize=maximize, foreach=None, capturable=cuda, differentiable=False,
                        fused=True if cuda else None, decoupled_weight_decay=False)
        super().__init__(params, defaults, max_norm)

    def _rule_cpu(self, params, grads, ms, vs, steps, g):
        from torch.optim.adam import adam

        adam(params, grads, ms, vs, [], steps, foreach=False, capturable=False, differentiable=False, fused=False,
             grad_scale=None, found_inf=None, has_complex=False, decoupled_weight_decay=False, amsgrad=False,
             beta1=g["betas"][0], beta2=g["betas"][1], lr=g["lr"], weight_decay=0, eps=g["eps"], maximize=False)


class FusedClipRAdam(_FusedClipBase):
    """``clip_grad_norm_(params, max_norm)`` and ``torch.optim.RAdam.step()`` in two HIP launches."""
    NAME = "FusedClipRAdam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, max_norm=None,
                 maximize=False):
        from ._learn import OPTIM_RADAM

        self.RULE = OPTIM_RADAM
        params = list(params)
        cuda = _on_cuda(params)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, maximize=maximize, foreach=None,
                        capturable=cuda, decoupled_weight_decay=False, differentiable=False)
        super().__init__(params, defaults, max_norm)

    def _rule_cpu(self, params, grads, ms, vs, steps, g):
        from torch.optim.radam import radam

        radam(params, grads, ms, vs, steps, decoupled_weight_decay=False, foreach=False, differentiable=False,
              capturable=False, has_complex=False, maximize=False, beta1=g["betas"][0], beta2=g["betas"][1], lr=g["lr"],
              weight_decay=0, eps=g["eps"])
