"""``FusedMLP``: the inference forward of small Linear/ELU networks over one shared input as ONE HIP launch
(h12learn_mlp_forward, csrc/h12_policy.hip): observation normaliser, every layer and the output, in exact fp32 on the
f32-input MFMA, with the activations held in LDS.  It serves play, sim2sim and the trainers' collection; the default
everywhere stays the torch path (``fused=False`` / ``--fused`` absent / ``H12_POLICY_FUSED`` unset).

    f = FusedMLP([agent.actor_mean, agent.critic])           # two networks, one input
    mean, value = f(obs, repack=True)                        # re-pack from the live parameters, then one launch
    act = FusedMLP([policy.actor], normalizer=obs_norm)      # statistics read, never updated
    (actions,) = act(obs)

The packed copy of the weights is what the kernel reads: ``refresh()`` (one launch, capturable) re-packs it from the
live parameters, so call it, or pass ``repack=True``, after the parameters changed.  No autograd.  On CPU tensors the
torch modules are evaluated, so the surface is testable without a GPU; on CUDA a missing kernel is an error.

Inside a captured graph: networks wider than 512 need more than 64 KiB of LDS, and the first such call of a process
raises the kernel's limit, which cannot be done while the stream is capturing: that call raises "must be made outside
a stream capture (warm up first)".  Call once eagerly before capturing, as any graph warm-up does.

``TrainableFusedMLP`` (further down) is the learner's counterpart: one network with autograd, forward and backward on
the training kernels of csrc/h12_policy_train.hip; ``FusedMLP`` itself stays forward only."""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _learn


def fused_collection_enabled() -> bool:
    """H12_POLICY_FUSED=1: both trainers' collection computes actor mean and critic value with FusedMLP."""
    return os.environ.get("H12_POLICY_FUSED", "0") == "1"


def _linears(net: nn.Module, index: int) -> list[nn.Linear]:
    if not isinstance(net, nn.Sequential):
        raise ValueError(f"FusedMLP: network {index} is {type(net).__name__}, an nn.Sequential of Linear/ELU is required")
    mods = list(net)
    if not mods or len(mods) % 2 == 0:
        raise ValueError(f"FusedMLP: network {index} must be Linear (ELU Linear)*, got {len(mods)} modules")
    out = []
    for k, m in enumerate(mods):
        if k % 2 == 0:
            if not isinstance(m, nn.Linear) or m.bias is None:
                raise ValueError(f"FusedMLP: network {index} module {k} is {type(m).__name__}, nn.Linear with bias expected")
            out.append(m)
        elif not isinstance(m, nn.ELU) or m.alpha != 1.0:
            raise ValueError(f"FusedMLP: network {index} module {k} is {m}, only nn.ELU(alpha=1) is supported")
    return out


class FusedMLP:
    def __init__(self, nets, normalizer: nn.Module | None = None):
        from .cleanrl import RunningMeanStd
        from .ppo import EmpiricalNormalization

        self.nets = list(nets)
        if not 1 <= len(self.nets) <= _learn.MLP_MAX_NETS:
            raise ValueError(f"FusedMLP: {len(self.nets)} networks (1..{_learn.MLP_MAX_NETS})")
        self._layers = [_linears(net, i) for i, net in enumerate(self.nets)]
        max_width = _learn.mlp_max_width()
        d_in = self._layers[0][0].in_features
        for i, layers in enumerate(self._layers):
            if len(layers) > _learn.MLP_MAX_LAYERS:
                raise ValueError(f"FusedMLP: network {i} has {len(layers)} linear layers (at most {_learn.MLP_MAX_LAYERS})")
            if layers[0].in_features != d_in:
                raise ValueError(f"FusedMLP: network {i} reads {layers[0].in_features} inputs, network 0 reads {d_in}")
            for lin in layers:
                if max(lin.in_features, lin.out_features) > max_width or lin.weight.dtype != torch.float32:
                    raise ValueError(f"FusedMLP: network {i}: {lin} is wider than {max_width} or not float32")
        if isinstance(normalizer, nn.Identity):
            normalizer = None
        self.normalizer = normalizer
        if normalizer is None:
            self._norm = (_learn.MLP_NORM_NONE, None, None, 0.0)
        elif isinstance(normalizer, RunningMeanStd):
            self._norm = (_learn.MLP_NORM_VAR, normalizer.running_mean, normalizer.running_var, normalizer.epsilon)
        elif isinstance(normalizer, EmpiricalNormalization):
            self._norm = (_learn.MLP_NORM_STD, normalizer._mean, normalizer._std, normalizer.eps)
        else:
            raise ValueError(f"FusedMLP: normalizer {type(normalizer).__name__} is neither cleanrl.RunningMeanStd nor "
                             "ppo.EmpiricalNormalization")
        if normalizer is not None and self._norm[1].numel() != d_in:
            raise ValueError(f"FusedMLP: normalizer of {self._norm[1].numel()} columns on {d_in} inputs")
        self.d_in = d_in
        self._desc = None
        self._packed = None
        self._keep = None
        if self._layers[0][0].weight.is_cuda:
            self.refresh()

    # ---- device side
    def _describe(self):
        """The descriptor over the parameters' present storage (rebuilt when a parameter or a statistic moved)."""
        tensors = [(lin.weight, lin.bias) for layers in self._layers for lin in layers]
        kind, mean, scale, eps = self._norm
        if kind == _learn.MLP_NORM_STD:  # EmpiricalNormalization.update rebinds _std
            mean, scale = self.normalizer._mean, self.normalizer._std
        ptrs = tuple(t.data_ptr() for pair in tensors for t in pair) + (
            (mean.data_ptr(), scale.data_ptr()) if kind != _learn.MLP_NORM_NONE else ())
        if self._desc is not None and ptrs == self._ptrs:
            return self._desc
        dev = tensors[0][0].device
        for w, b in tensors:
            if not (w.is_cuda and w.device == dev and b.device == dev and w.is_contiguous() and b.is_contiguous()):
                raise ValueError("FusedMLP: every parameter must be a contiguous tensor on one CUDA device")
        nm = ns = None
        if kind != _learn.MLP_NORM_NONE:
            nm, ns = mean.detach().reshape(-1), scale.detach().reshape(-1)
            if not (nm.device == dev and nm.dtype == torch.float32 and ns.dtype == torch.float32
                    and nm.is_contiguous() and ns.is_contiguous()):
                raise ValueError("FusedMLP: the normalizer's statistics must be float32 on the networks' device")
        nets = [[(lin.weight.detach(), lin.bias.detach()) for lin in layers] for layers in self._layers]
        self._desc = _learn.mlp_desc(nets, kind, nm, ns, eps)
        self._keep = (nets, nm, ns)
        self._ptrs = ptrs
        nfloat = _learn.mlp_packed_bytes(self._desc) // 4
        if self._packed is None or self._packed.numel() != nfloat or self._packed.device != dev:
            self._packed = torch.empty(nfloat, dtype=torch.float32, device=dev)
        return self._desc

    def refresh(self):
        """Re-pack from the live parameters: one launch on the current stream, capturable."""
        desc = self._describe()
        _learn.mlp_pack(desc, self._packed)
        return self

    def __call__(self, x: torch.Tensor, repack: bool = False) -> tuple:
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("FusedMLP does no autograd: call it under torch.no_grad() or on a detached input")
        if not x.is_cuda:
            with torch.no_grad():
                h = x if self.normalizer is None else self._normalise_torch(x)
                return tuple(net(h) for net in self.nets)
        if x.dim() != 2 or x.shape[1] != self.d_in:
            raise ValueError(f"FusedMLP: x {tuple(x.shape)} is not (n, {self.d_in})")
        before = self._desc
        desc = self._describe()
        if repack or desc is not before:  # a parameter that moved is re-packed from its new storage
            _learn.mlp_pack(desc, self._packed)
        return _learn.mlp_forward(desc, self._packed, x.detach().contiguous())

    def _normalise_torch(self, x):
        kind, mean, scale, eps = self._norm
        if kind == _learn.MLP_NORM_VAR:
            return (x - mean) / torch.sqrt(scale + eps)
        return (x - self.normalizer._mean) / (self.normalizer._std + eps)

    # ---- from an exported policy.pt
    @classmethod
    def from_exported(cls, jit_module, device=None) -> "FusedMLP":
        """Actor and normaliser of a ``policy.pt`` written by export_policy_as_jit (h12env.export._ExportedPolicy:
        ``actor.<k>.weight/bias`` with ELU between, ``normalizer._mean/_var/_std/count`` when one was exported)."""
        from .ppo import EmpiricalNormalization

        sd = jit_module.state_dict()
        idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith("actor.") and k.endswith(".weight")})
        if not idx:
            raise ValueError("FusedMLP.from_exported: no actor.<k>.weight in the module's state_dict")
        kinds = [getattr(m, "original_name", type(m).__name__) for m in jit_module.actor.children()]
        mods: list[nn.Module] = []
        for k, name in enumerate(kinds):
            if name == "Linear" and k in idx:
                w = sd[f"actor.{k}.weight"]
                lin = nn.Linear(w.shape[1], w.shape[0])
                lin.load_state_dict({"weight": w, "bias": sd[f"actor.{k}.bias"]})
                mods.append(lin)
            elif name == "ELU":
                mods.append(nn.ELU())
            else:
                raise ValueError(f"FusedMLP.from_exported: actor.{k} is {name}; only Linear and ELU are supported")
        actor = nn.Sequential(*mods)
        norm = None
        if "normalizer._mean" in sd:
            norm = EmpiricalNormalization([sd["normalizer._mean"].shape[-1]],
                                          eps=float(getattr(jit_module.normalizer, "eps", 1e-2)))
            norm.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("normalizer.")})
            norm.eval()
        if device is None:
            device = next(iter(sd.values())).device
        actor = actor.to(device).eval()
        for p in actor.parameters():
            p.requires_grad_(False)
        return cls([actor], norm.to(device) if norm is not None else None)


def learner_fused_enabled() -> bool:
    """H12_LEARNER_FUSED=1: ppo.PPO routes the learning-phase actor and critic through TrainableFusedMLP."""
    return os.environ.get("H12_LEARNER_FUSED", "0") == "1"


def _wgrad(dz: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """dW = dZ^T H on the GEMM library, with ppo.SplitKLinear's rule: a 16-way split-K bmm for large batches."""
    from .ppo import SplitKLinear

    n, s = dz.shape[0], SplitKLinear.SPLIT_K
    if n >= SplitKLinear.MIN_BATCH and n % s == 0:
        return torch.bmm(dz.view(s, n // s, -1).transpose(1, 2), h.view(s, n // s, -1)).sum(0)
    return dz.t() @ h


class _FusedMLPFn(torch.autograd.Function):
    """y = net(x) of one Linear/ELU network: pack W and W^T from the live parameters, h12learn_mlp_forward_train; the
    backward is h12learn_mlp_backward (dgrad chain, ELU', bias gradients) and one library GEMM per weight gradient.
    First derivatives only (once_differentiable).  CPU tensors: the same node over the torch operations."""

    @staticmethod
    def forward(ctx, x, *params):
        ctx.on_device = x.is_cuda
        if not x.is_cuda:  # the torch modules' own operations, recorded here and differentiated once in backward
            with torch.enable_grad():
                xd = x.detach().requires_grad_(ctx.needs_input_grad[0])
                ps = [p.detach().requires_grad_(ctx.needs_input_grad[1 + i]) for i, p in enumerate(params)]
                h = xd
                for i in range(0, len(ps), 2):
                    h = nn.functional.linear(h, ps[i], ps[i + 1])
                    if i + 2 < len(ps):
                        h = nn.functional.elu(h)
            ctx.torch_graph = (xd, ps, h)
            return h.detach()
        with torch.autocast(device_type="cuda", enabled=False):
            pairs = [(params[i].detach(), params[i + 1].detach()) for i in range(0, len(params), 2)]
            for w, b in pairs:
                if not (w.is_cuda and w.device == x.device and b.device == x.device and w.dtype == torch.float32
                        and b.dtype == torch.float32 and w.is_contiguous() and b.is_contiguous()):
                    raise ValueError("TrainableFusedMLP: every parameter must be a contiguous float32 tensor on x's device")
            xc = x.detach().float().contiguous()
            desc = _learn.mlp_desc([pairs])
            packed = torch.empty(_learn.mlp_packed_bytes(desc) // 4, dtype=torch.float32, device=x.device)
            packed_t = torch.empty(_learn.mlp_packed_t_bytes(desc) // 4, dtype=torch.float32, device=x.device)
            _learn.mlp_pack(desc, packed)
            _learn.mlp_pack_t(desc, packed_t)
            y, hs = _learn.mlp_forward_train(desc, packed, xc)
            ctx.desc, ctx.x_dtype = desc, x.dtype
            ctx.save_for_backward(xc, packed_t, *hs)
            return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        if not ctx.on_device:
            xd, ps, y = ctx.torch_graph
            ctx.torch_graph = None
            wanted = [t for t in [xd] + ps if t.requires_grad]
            with torch.enable_grad():
                got = iter(torch.autograd.grad(y, wanted, dy) if wanted else ())
            return tuple(next(got) if t.requires_grad else None for t in [xd] + ps)
        xc, packed_t, *hs = ctx.saved_tensors
        with torch.autocast(device_type="cuda", enabled=False):
            dy = dy.float().contiguous()
            # the descriptor's shapes only: the backward reads the transposed pack and the saved activations
            dzs, dbs, dx = _learn.mlp_backward(ctx.desc, packed_t, dy, hs, need_dx=ctx.needs_input_grad[0])
            dzs = dzs + [dy]
            acts = [xc] + list(hs)
            grads = []
            for l, (dz, db) in enumerate(zip(dzs, dbs)):
                gw = _wgrad(dz, acts[l]) if ctx.needs_input_grad[1 + 2 * l] else None
                grads += [gw, db if ctx.needs_input_grad[2 + 2 * l] else None]
            return (None if dx is None else dx.to(ctx.x_dtype), *grads)


class TrainableFusedMLP:
    """``TrainableFusedMLP(net)(x)`` is ``net(x)`` with autograd, computed by the fused kernels: the forward and the
    whole backward except the weight-gradient GEMMs are one HIP launch each (csrc/h12_policy_train.hip).  ``net``: an
    ``nn.Sequential`` of nn.Linear / ELU(alpha=1) as for FusedMLP, every width at most ``mlp_train_max_width()``.  The
    parameters are read live at every call (packed inside the autograd function, so also inside a captured graph).
    First derivatives only: a double backward is refused.  On CPU tensors, or with grad disabled, the torch modules'
    operations are evaluated (bit-identical to ``net``)."""

    def __init__(self, net: nn.Module):
        self.net = net
        self._layers = _linears(net, 0)
        if len(self._layers) > _learn.MLP_MAX_LAYERS:
            raise ValueError(f"FusedMLP: network 0 has {len(self._layers)} linear layers (at most {_learn.MLP_MAX_LAYERS})")
        max_width = _learn.mlp_train_max_width()
        for lin in self._layers:
            if max(lin.in_features, lin.out_features) > max_width or lin.weight.dtype != torch.float32:
                raise ValueError(f"FusedMLP: network 0: {lin} is wider than {max_width} or not float32")
        self.d_in = self._layers[0].in_features

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if not torch.is_grad_enabled():
            return self.net(x)
        if x.is_cuda and (x.dim() != 2 or x.shape[1] != self.d_in or x.shape[0] < 1):
            raise ValueError(f"TrainableFusedMLP: x {tuple(x.shape)} is not (n >= 1, {self.d_in})")
        params = [p for lin in self._layers for p in (lin.weight, lin.bias)]
        return _FusedMLPFn.apply(x, *params)
