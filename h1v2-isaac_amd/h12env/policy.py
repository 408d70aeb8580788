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


def fused_collection_on(obs: torch.Tensor) -> bool:
    """Fused collection on this tensor, for both trainers: the flag, a CUDA tensor, grad disabled (no autograd)."""
    return fused_collection_enabled() and obs.is_cuda and not torch.is_grad_enabled()


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
        self.normalizer, self._norm = _norm_of(normalizer, d_in, "FusedMLP")
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
        sd = jit_module.state_dict()
        actor, norm = _exported_actor(jit_module, sd), _exported_normalizer(jit_module, sd)
        if device is None:
            device = next(iter(sd.values())).device
        return cls([actor.to(device)], norm.to(device) if norm is not None else None)


def _exported_actor(jit_module, sd) -> nn.Sequential:
    """The ``actor`` of an exported policy.pt as a frozen nn.Sequential in eval mode: ``actor.<k>.weight/bias`` with ELU
    between.  Any other child, or a Linear whose weight the state dict does not hold, is refused."""
    if not any(k.startswith("actor.") and k.endswith(".weight") for k in sd):
        raise ValueError("from_exported: no actor.<k>.weight in the module's state_dict")
    mods: list[nn.Module] = []
    for k, m in enumerate(jit_module.actor.children()):
        name = getattr(m, "original_name", type(m).__name__)
        if name == "Linear" and f"actor.{k}.weight" in sd:
            w = sd[f"actor.{k}.weight"]
            lin = nn.Linear(w.shape[1], w.shape[0])
            lin.load_state_dict({"weight": w, "bias": sd[f"actor.{k}.bias"]})
            mods.append(lin)
        elif name == "ELU":
            mods.append(nn.ELU())
        else:
            raise ValueError(f"from_exported: actor.{k} is {name}; only Linear and ELU are supported")
    return nn.Sequential(*mods).eval().requires_grad_(False)


def _exported_normalizer(jit_module, sd):
    """The ``normalizer`` of an exported policy.pt as an EmpiricalNormalization in eval mode; None without one."""
    from .ppo import EmpiricalNormalization

    if "normalizer._mean" not in sd:
        return None
    norm = EmpiricalNormalization([sd["normalizer._mean"].shape[-1]],
                                  eps=float(getattr(jit_module.normalizer, "eps", 1e-2)))
    norm.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("normalizer.")})
    return norm.eval()


def _norm_of(normalizer, d_in: int, who: str):
    """(normalizer or None, (kind, mean, scale, eps)) as FusedMLP reads a normaliser."""
    from .cleanrl import RunningMeanStd
    from .ppo import EmpiricalNormalization

    if normalizer is None or isinstance(normalizer, nn.Identity):
        return None, (_learn.MLP_NORM_NONE, None, None, 0.0)
    if isinstance(normalizer, RunningMeanStd):
        norm = (_learn.MLP_NORM_VAR, normalizer.running_mean, normalizer.running_var, normalizer.epsilon)
    elif isinstance(normalizer, EmpiricalNormalization):
        norm = (_learn.MLP_NORM_STD, normalizer._mean, normalizer._std, normalizer.eps)
    else:
        raise ValueError(f"{who}: normalizer {type(normalizer).__name__} is neither cleanrl.RunningMeanStd nor "
                         "ppo.EmpiricalNormalization")
    if norm[1].numel() != d_in:
        raise ValueError(f"{who}: normalizer of {norm[1].numel()} columns on {d_in} inputs")
    return normalizer, norm


def lstm_step_limit(rnn: nn.Module) -> str | None:
    """Why h12learn_lstm_step cannot run ``rnn`` (None: it can): one-layer fp32 nn.LSTM of at most lstm_max_hidden()."""
    if not isinstance(rnn, nn.LSTM):
        return f"{type(rnn).__name__}: the fused step is LSTM only"
    if rnn.num_layers != 1 or rnn.bidirectional or rnn.proj_size != 0 or not rnn.bias:
        return f"num_layers = {rnn.num_layers}: the fused step is one unidirectional layer with biases, no projection"
    if rnn.hidden_size > _learn.lstm_max_hidden():
        return f"hidden size {rnn.hidden_size}: the fused step supports at most {_learn.lstm_max_hidden()}"
    if rnn.input_size > _learn.mlp_max_width() or rnn.weight_ih_l0.dtype != torch.float32:
        return f"input size {rnn.input_size} is wider than {_learn.mlp_max_width()} or the weights are not float32"
    return None


class FusedLSTMStep:
    """One step of up to two (nn.LSTM, Linear/ELU nn.Sequential) pairs over one shared input as ONE HIP launch
    (h12learn_lstm_step, csrc/h12_policy_rnn.hip).  ``step(x, states)`` with ``states`` a list of (h, c) [n][H] tensors
    per pair, updated in place; returns the MLPs' outputs.  ``refresh()`` / ``repack=True`` re-pack the weights (one
    launch, capturable) as for FusedMLP; the first call at more than 64 KiB of LDS must be made outside a capture."""

    def __init__(self, pairs, normalizer: nn.Module | None = None):
        self.pairs = list(pairs)
        if not 1 <= len(self.pairs) <= _learn.LSTM_MAX_NETS:
            raise ValueError(f"FusedLSTMStep: {len(self.pairs)} networks (1..{_learn.LSTM_MAX_NETS})")
        for rnn, _ in self.pairs:
            why = lstm_step_limit(rnn)
            if why:
                raise ValueError(f"FusedLSTMStep: {why}")
        r0 = self.pairs[0][0]
        self.d_in, self.hidden = r0.input_size, r0.hidden_size
        self._layers = [_linears(net, i) for i, (_, net) in enumerate(self.pairs)]
        for i, ((rnn, _), layers) in enumerate(zip(self.pairs, self._layers)):
            if (rnn.input_size, rnn.hidden_size) != (self.d_in, self.hidden) or layers[0].in_features != self.hidden:
                raise ValueError(f"FusedLSTMStep: network {i} is {rnn.input_size} -> {rnn.hidden_size} -> "
                                 f"{layers[0].in_features}, network 0 is {self.d_in} -> {self.hidden}")
            if len(layers) > _learn.MLP_MAX_LAYERS or any(
                    max(lin.in_features, lin.out_features) > _learn.mlp_max_width() for lin in layers):
                raise ValueError(f"FusedLSTMStep: network {i} has more than {_learn.MLP_MAX_LAYERS} layers or one wider "
                                 f"than {_learn.mlp_max_width()}")
        self.normalizer, self._norm = _norm_of(normalizer, self.d_in, "FusedLSTMStep")
        self._desc = self._packed = self._keep = self._ptrs = None

    def _describe(self):
        kind, mean, scale, eps = self._norm
        if kind == _learn.MLP_NORM_STD:  # EmpiricalNormalization.update rebinds _std
            mean, scale = self.normalizer._mean, self.normalizer._std
        cells = [tuple(p.detach() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0))
                 for rnn, _ in self.pairs]
        nets = [[(lin.weight.detach(), lin.bias.detach()) for lin in layers] for layers in self._layers]
        tensors = [t for c in cells for t in c] + [t for net in nets for pair in net for t in pair]
        nm = ns = None
        if kind != _learn.MLP_NORM_NONE:
            nm, ns = mean.detach().reshape(-1), scale.detach().reshape(-1)
            tensors += [nm, ns]
        ptrs = tuple(t.data_ptr() for t in tensors)
        if self._desc is not None and ptrs == self._ptrs:
            return self._desc
        dev = tensors[0].device
        for t in tensors:
            if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("FusedLSTMStep: every parameter and statistic must be a contiguous float32 tensor on "
                                 "one CUDA device")
        self._desc = _learn.lstm_desc(cells, nets, kind, nm, ns, eps)
        self._keep, self._ptrs = tensors, ptrs
        nfloat = _learn.lstm_packed_bytes(self._desc) // 4
        if self._packed is None or self._packed.numel() != nfloat or self._packed.device != dev:
            self._packed = torch.empty(nfloat, dtype=torch.float32, device=dev)
        return self._desc

    def refresh(self):
        _learn.lstm_pack(self._describe(), self._packed)
        return self

    def __call__(self, x: torch.Tensor, states, repack: bool = False, reset: torch.Tensor | None = None,
                 out_states=None) -> tuple:
        before = self._desc
        desc = self._describe()
        if repack or desc is not before:
            _learn.lstm_pack(desc, self._packed)
        return _learn.lstm_step(desc, self._packed, x.detach().contiguous(), states, reset=reset, out_states=out_states)


class FusedActorCritic:
    """The trainers' collection forward: ``(mean, value) = f(obs, cobs)`` from FusedMLP, or with ``memories`` (the
    actor's and the critic's nn.LSTM) from FusedLSTMStep, which steps ``states = [(h_a, c_a), (h_c, c_c)]`` in place.
    One two-network launch when actor and critic read the same observation (``cobs`` is ``obs`` or None), else one
    launch each.  The weights are re-packed at every call, in the same body and so inside a captured graph: they can
    never be stale after an update."""

    def __init__(self, actor: nn.Module, critic: nn.Module, memories=None):
        nets = [actor, critic]
        self._nets = nets if memories is None else list(zip(memories, nets))
        self._make = FusedMLP if memories is None else FusedLSTMStep
        self._shared = self._fused = None

    def __call__(self, obs: torch.Tensor, cobs: torch.Tensor | None = None, states=None) -> tuple:
        shared = cobs is None or cobs is obs
        if self._shared != shared:
            groups = [self._nets] if shared else [self._nets[:1], self._nets[1:]]
            self._fused = [self._make(g) for g in groups]
            self._shared = shared

        def run(f, x, st):
            return f(x, repack=True) if states is None else f(x, st, repack=True)

        if shared:
            return run(self._fused[0], obs, states)
        sa, sc = states if states is not None else (None, None)
        return run(self._fused[0], obs, [sa])[0], run(self._fused[1], cobs, [sc])[0]


class RecurrentPolicy:
    """The stateful inference policy of a recurrent actor: ``obs [n][d_in] -> actions``, keeping its own (n, H) memory.

        p = RecurrentPolicy(policy.memory_a.rnn, policy.actor, obs_normalizer, fused=True)
        actions = p(obs);  p.reset(dones)          # zero the rows of finished episodes;  p.reset(): all of them

    ``fused=True`` on CUDA tensors: one h12learn_lstm_step launch per call, in place on the state; it raises ValueError
    when the kernel cannot run the memory (GRU, more than one layer, hidden size above lstm_max_hidden()), naming the
    limit.  Otherwise, and on CPU tensors, the torch modules run.  The weights are packed at construction; call
    ``refresh()`` after they change.  No autograd."""

    def __init__(self, rnn: nn.Module, mlp: nn.Module, normalizer: nn.Module | None = None, fused: bool = False):
        self.rnn, self.mlp = rnn, mlp
        self.normalizer = None if isinstance(normalizer, nn.Identity) else normalizer
        self.fused = bool(fused)
        self._step = None
        if self.fused:
            why = lstm_step_limit(rnn)
            if why:
                raise ValueError(f"RecurrentPolicy(fused=True): {why}; the torch path (fused=False) runs it")
            self._step = FusedLSTMStep([(rnn, mlp)], self.normalizer)
        self.state = None  # LSTM: (h, c), GRU: (h,); [layers][n][H] each

    def refresh(self):
        if self._step is not None and self._step._packed is not None:
            self._step.refresh()
        return self

    def _ensure_state(self, n: int, device):
        if self.state is None or self.state[0].shape[1] != n or self.state[0].device != device:
            k = 2 if isinstance(self.rnn, nn.LSTM) else 1
            with torch.inference_mode(False):
                self.state = tuple(torch.zeros(self.rnn.num_layers, n, self.rnn.hidden_size, device=device)
                                   for _ in range(k))

    def reset(self, dones=None):
        if self.state is None:
            return
        for s in self.state:
            if dones is None:
                s.zero_()
            else:
                s[:, dones.to(s.device).reshape(-1) != 0] = 0.0

    @torch.no_grad()
    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        self._ensure_state(obs.shape[0], obs.device)
        if self._step is not None and obs.is_cuda:
            (y,) = self._step(obs.float(), [(self.state[0][0], self.state[1][0])])
            return y
        x = obs if self.normalizer is None else self._normalise_torch(obs)
        hx = self.state if len(self.state) > 1 else self.state[0]
        out, new = self.rnn(x.unsqueeze(0), hx)
        for dst, src in zip(self.state, new if len(self.state) > 1 else (new,)):
            dst.copy_(src)
        return self.mlp(out.squeeze(0))

    def _normalise_torch(self, obs):
        """The normaliser module with its statistics read, never updated, as the kernel reads them:
        cleanrl.RunningMeanStd has no eval mode and updates on a plain call."""
        from .cleanrl import RunningMeanStd

        if isinstance(self.normalizer, RunningMeanStd):
            return self.normalizer(obs, update=False)
        return self.normalizer(obs)

    @classmethod
    def from_exported(cls, jit_module, num_envs: int, device=None, fused: bool = False) -> "RecurrentPolicy":
        """The memory, actor and normaliser of a recurrent ``policy.pt`` (h12env.export: ``rnn.*``, ``actor.<k>.*``,
        ``normalizer.*``), with a state of ``num_envs`` rows: the export's own (1, 1, H) buffers serve one robot."""
        sd = jit_module.state_dict()
        if "rnn.weight_ih_l0" not in sd:
            raise ValueError("RecurrentPolicy.from_exported: no rnn.weight_ih_l0 in the module's state_dict")
        w_ih, w_hh = sd["rnn.weight_ih_l0"], sd["rnn.weight_hh_l0"]
        hidden = w_hh.shape[1]
        gates = w_ih.shape[0] // hidden
        if gates not in (3, 4):
            raise ValueError(f"RecurrentPolicy.from_exported: {gates} gates per unit (LSTM has 4, GRU 3)")
        layers = len([k for k in sd if k.startswith("rnn.weight_ih_l")])
        rnn = (nn.LSTM if gates == 4 else nn.GRU)(w_ih.shape[1], hidden, num_layers=layers)
        rnn.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("rnn.")})
        actor, norm = _exported_actor(jit_module, sd), _exported_normalizer(jit_module, sd)
        if device is None:
            device = w_ih.device
        rnn = rnn.to(device).eval().requires_grad_(False)
        p = cls(rnn, actor.to(device), norm.to(device) if norm is not None else None, fused=fused)
        p._ensure_state(num_envs, torch.device(device))
        return p


def deploy_policy(jit_module, num_envs: int, device, fused: bool = False):
    """The callable obs [num_envs][d] -> actions of an exported ``policy.pt`` for the batched deploy loops (sim2sim.py,
    eval_policy.py).  A recurrent export (it has an ``rnn``) keeps (1, 1, H) state buffers that cannot serve num_envs
    robots: it is rebuilt as a RecurrentPolicy with a state of num_envs rows.  ``fused``: the HIP kernels."""
    if hasattr(jit_module, "rnn"):
        return RecurrentPolicy.from_exported(jit_module, num_envs, device=device, fused=fused)
    if fused:
        f = FusedMLP.from_exported(jit_module, device=device)
        return lambda x: f(x)[0]
    return jit_module


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
