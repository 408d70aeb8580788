"""PPO runner for the H1-2 env: the rsl_rl 2.3 OnPolicyRunner surface that scripts/rsl_rl/train.py drives
(reference: scripts/rsl_rl/train.py:123-141; agent cfg biped_tasks/.../h12_12dof/agents/rsl_rl_ppo_cfg.py:10-47;
algorithm: rsl-rl-lib 2.3.3 as pinned in uv.lock, restated here -- the package is not importable offline).

Design for one process per MI355X:
  * the rollout lives in HBM as (T, N, ...) tensors filled in place; the env's observation buffer is
    copied into it once per step (the env keeps a ping-pong buffer);
  * multi-GPU (torchrun, one rank per GPU): each rank collects its env shard, the rollout is
    all-gathered over RCCL/xGMI in one collective per dtype bucket (h12env.distributed.allgather_rollout,
    the north_star's exchange), every rank draws the same minibatch permutation of the GLOBAL batch,
    computes gradients on its 1/world share of each minibatch, and the gradients are averaged with one
    flat all-reduce -- so all ranks apply bit-identical updates (parameters are also broadcast from rank 0
    at start and on load);
  * checkpoints use rsl_rl's layout ({"model_state_dict", "optimizer_state_dict", "iter", "infos"});
  * rsl_rl's symmetry_cfg (mirror-image data augmentation, mirror loss) with the env's own mirror map
    (h12env.symmetry): gather + mirror + concatenation of a minibatch are one launch inside the update graph.
"""
from __future__ import annotations

import json
import math
import os
import statistics
import subprocess
import time
from collections import deque
from dataclasses import dataclass

import torch
import torch.distributed as dist
import torch.nn as nn
from torch.distributions import Normal

from . import distributed as D
from .graphs import TrainingState, capture, graph_enabled
from .policy import FusedActorCritic, fused_collection_on
from .recurrent import Memory, split_and_pad_trajectories, state_tensors


# ---------------------------------------------------------------------------------------------- modules
def activation(name: str) -> nn.Module:
    table = {"elu": nn.ELU, "selu": nn.SELU, "relu": nn.ReLU, "lrelu": nn.LeakyReLU, "tanh": nn.Tanh,
             "sigmoid": nn.Sigmoid, "gelu": nn.GELU}
    if name not in table:
        raise ValueError(f"unknown activation {name!r}")
    return table[name]()


class _SplitKLinearFn(torch.autograd.Function):
    """y = x W^T + b whose weight gradient dW = dY^T X is computed as SPLIT_K batched GEMMs over slices of the
    minibatch and summed: a (out x in) GEMM with K = 24576 gives hipBLASLt only ~17 output tiles for the 256
    CUs (measured 20 TFLOP/s); split 16 ways it runs 1.5x faster end to end (exp: fwd+bwd of both MLPs
    2.19 -> 1.48 ms per minibatch).  Same math, fp32 summation order differs.  dt: the GEMM operand type
    (float32, or bfloat16 under the bf16 learner's autocast: the partial products are summed in fp32 and the
    gradients of the fp32 master weights are fp32)."""

    @staticmethod
    def forward(ctx, x, w, b, split, dt):
        with torch.autocast(device_type="cuda", enabled=False):
            xc, wc = x.to(dt), w.to(dt)
            ctx.save_for_backward(xc, wc)
            ctx.split, ctx.x_dtype = split, x.dtype
            return torch.addmm(b.to(dt), xc, wc.t())

    @staticmethod
    def backward(ctx, gy):
        xc, wc = ctx.saved_tensors
        s, n = ctx.split, xc.shape[0]
        with torch.autocast(device_type="cuda", enabled=False):
            gy = gy.to(wc.dtype)
            gx = (gy @ wc).to(ctx.x_dtype) if ctx.needs_input_grad[0] else None
            gw = torch.bmm(gy.view(s, n // s, -1).transpose(1, 2), xc.view(s, n // s, -1))
            gw = gw.sum(0) if gw.dtype == torch.float32 else gw.float().sum(0)
            return gx, gw, gy.float().sum(0), None, None


class SplitKLinear(nn.Linear):
    """nn.Linear (same parameters / state dict) with the split-K weight gradient for large GPU batches
    (fp32, or bf16 operands under autocast)."""

    SPLIT_K = 16
    MIN_BATCH = 8192

    def forward(self, x):
        if (x.is_cuda and x.dim() == 2 and self.weight.dtype == torch.float32 and torch.is_grad_enabled()
                and x.shape[0] >= self.MIN_BATCH and x.shape[0] % self.SPLIT_K == 0):
            dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.float32
            if x.dtype in (torch.float32, dt):
                return _SplitKLinearFn.apply(x, self.weight, self.bias, self.SPLIT_K, dt)
        return nn.functional.linear(x, self.weight, self.bias)


def mlp(n_in: int, hidden: list[int], n_out: int, act: str) -> nn.Sequential:
    layers: list[nn.Module] = []
    d = n_in
    for h in hidden:
        layers += [SplitKLinear(d, h), activation(act)]
        d = h
    layers.append(SplitKLinear(d, n_out))
    return nn.Sequential(*layers)


def plain_linear(module: nn.Module) -> nn.Module:
    """A copy of `module` with every SplitKLinear replaced by an nn.Linear holding the same parameters
    (for TorchScript / ONNX export)."""
    import copy

    m = copy.deepcopy(module)
    for name, child in list(m.named_children()):
        if isinstance(child, SplitKLinear):
            lin = nn.Linear(child.in_features, child.out_features, device=child.weight.device, dtype=child.weight.dtype)
            lin.load_state_dict(child.state_dict())
            setattr(m, name, lin)
        else:
            setattr(m, name, plain_linear(child))
    return m


class ActorCritic(nn.Module):
    """Gaussian policy with a state-independent std (rsl_rl ActorCritic, noise_std_type "scalar"/"log")."""

    is_recurrent = False

    def __init__(self, num_actor_obs: int, num_critic_obs: int, num_actions: int, actor_hidden_dims=(256, 256, 256),
                 critic_hidden_dims=(256, 256, 256), activation="elu", init_noise_std=1.0, noise_std_type="scalar",
                 **kwargs):
        super().__init__()
        self.actor = mlp(num_actor_obs, list(actor_hidden_dims), num_actions, activation)
        self.critic = mlp(num_critic_obs, list(critic_hidden_dims), 1, activation)
        self.noise_std_type = noise_std_type
        if noise_std_type == "scalar":
            self.std = nn.Parameter(init_noise_std * torch.ones(num_actions))
        elif noise_std_type == "log":
            self.log_std = nn.Parameter(torch.log(init_noise_std * torch.ones(num_actions)))
        else:
            raise ValueError(f"unknown noise_std_type {noise_std_type!r}")
        self.distribution: Normal | None = None
        self._fused_learner: dict | None = None
        Normal.set_default_validate_args(False)

    def enable_fused_learner(self):
        """Route actor and critic through h12env.policy.TrainableFusedMLP (fused HIP forward and backward) whenever
        grad is enabled on CUDA tensors.  Same parameters, same state dict.  ValueError when a network is not
        Linear/ELU or is wider than the training kernels support."""
        from .policy import TrainableFusedMLP

        self._fused_learner = {"actor": TrainableFusedMLP(self.actor), "critic": TrainableFusedMLP(self.critic)}

    def _net(self, name: str, obs):
        f = self.__dict__.get("_fused_learner")
        if f is not None and obs.is_cuda and torch.is_grad_enabled():
            return f[name](obs)
        return getattr(self, name)(obs)

    def _std(self, mean):
        s = self.std if self.noise_std_type == "scalar" else torch.exp(self.log_std)
        return s.expand_as(mean)

    def update_distribution(self, obs):
        mean = self._net("actor", obs)
        self.distribution = Normal(mean, self._std(mean))

    def act(self, obs, **kw):
        self.update_distribution(obs)
        return self.distribution.sample()

    def act_inference(self, obs):
        return self._net("actor", obs)

    def evaluate(self, critic_obs, **kw):
        return self._net("critic", critic_obs)

    def get_actions_log_prob(self, actions):
        return self.distribution.log_prob(actions).sum(dim=-1)

    @property
    def action_mean(self):
        return self.distribution.mean

    @property
    def action_std(self):
        return self.distribution.stddev

    @property
    def entropy(self):
        return self.distribution.entropy().sum(dim=-1)

    def reset(self, dones=None):
        pass


class ActorCriticRecurrent(ActorCritic):
    """rsl_rl's ActorCriticRecurrent: ``memory_a`` reads the actor observation, ``memory_c`` the critic observation,
    and the actor and critic MLPs read the memories' hidden state.  Collection steps the memories (``masks is None``);
    the update runs them over padded trajectories from ``hidden_states`` (h12env.recurrent.Memory).  State-dict keys are
    rsl_rl's (memory_a.rnn.*, memory_c.rnn.*, actor.N.*, critic.N.*, std / log_std)."""

    is_recurrent = True

    def __init__(self, num_actor_obs: int, num_critic_obs: int, num_actions: int, actor_hidden_dims=(256, 256, 256),
                 critic_hidden_dims=(256, 256, 256), activation="elu", rnn_type="lstm", rnn_hidden_dim=256,
                 rnn_num_layers=1, init_noise_std=1.0, noise_std_type="scalar", **kwargs):
        if "rnn_hidden_size" in kwargs:  # the spelling of rsl_rl before 2.3
            rnn_hidden_dim = kwargs.pop("rnn_hidden_size")
        super().__init__(rnn_hidden_dim, rnn_hidden_dim, num_actions, actor_hidden_dims=actor_hidden_dims,
                         critic_hidden_dims=critic_hidden_dims, activation=activation, init_noise_std=init_noise_std,
                         noise_std_type=noise_std_type)
        self.memory_a = Memory(num_actor_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_dim)
        self.memory_c = Memory(num_critic_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_dim)

    def enable_fused_learner(self):
        raise ValueError("a recurrent policy's update runs through the library LSTM")

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def act(self, obs, masks=None, hidden_states=None, dones=None):
        return super().act(self.memory_a(obs, masks, hidden_states, dones=dones).squeeze(0))

    def act_inference(self, obs):
        return super().act_inference(self.memory_a(obs).squeeze(0))

    def evaluate(self, critic_obs, masks=None, hidden_states=None, dones=None):
        return super().evaluate(self.memory_c(critic_obs, masks, hidden_states, dones=dones).squeeze(0))

    def act_and_evaluate_sequence(self, obs, critic_obs, dones, hidden_a, hidden_c):
        """act(obs, dones=, hidden_states=hidden_a) and evaluate(critic_obs, dones=, hidden_states=hidden_c) with both
        memories in one two-network call of the sequence kernels (h12env.recurrent.lstm_sequence_pair).  Returns the
        value."""
        from .recurrent import lstm_sequence_pair

        ha, hc = lstm_sequence_pair((self.memory_a.rnn, self.memory_c.rnn), (obs, critic_obs), dones,
                                    (hidden_a, hidden_c))
        ActorCritic.act(self, ha)
        return ActorCritic.evaluate(self, hc)

    def get_hidden_states(self):
        return self.memory_a.hidden_states, self.memory_c.hidden_states


class EmpiricalNormalization(nn.Module):
    """Running mean / variance normaliser (rsl_rl EmpiricalNormalization); statistics frozen in eval."""

    def __init__(self, shape, eps=1e-2, until=None):
        super().__init__()
        self.eps = eps
        self.until = until
        self.register_buffer("_mean", torch.zeros(shape).unsqueeze(0))
        self.register_buffer("_var", torch.ones(shape).unsqueeze(0))
        self.register_buffer("_std", torch.ones(shape).unsqueeze(0))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))

    def forward(self, x):
        if self.training:
            self.update(x)
        return (x - self._mean) / (self._std + self.eps)

    @torch.jit.unused
    def update(self, x):
        """Running update from one batch; under torch.distributed (world > 1) the batch is the union of
        every rank's shard, so all ranks keep identical statistics.  The shards' statistics are merged with
        Chan's parallel formula (global mean from sum n_r mean_r, then M2 = sum n_r (var_r + (mean_r - mean)^2)):
        no E[x^2] - mean^2 cancellation, so the merged variance is never negative.  Every call issues exactly two
        all-reduces on every rank: the union size rides in the first one (with the shards' weighted means), so
        ranks never disagree on which collectives run, whatever their local batch sizes.  The merge and the sample count
        use the device-side union size (no host sync per update)."""
        if self.until is not None and self.count >= self.until:
            return
        n = x.shape[0]
        var_x = torch.var(x, dim=0, unbiased=False, keepdim=True)
        mean_x = torch.mean(x, dim=0, keepdim=True)
        if torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1:
            s1 = torch.cat([mean_x * n, torch.full((1, 1), float(n), device=x.device, dtype=mean_x.dtype)], 1)
            D.all_reduce(s1)
            n_dev = s1[:, -1:]
            g_mean = s1[:, :-1] / n_dev
            m2 = (var_x + (mean_x - g_mean) ** 2) * n
            D.all_reduce(m2)
            m2 = m2 / n_dev
            # the union size stays on the device (no host sync, and no cache that a rank whose own batch size is
            # unchanged could keep while another rank's changes)
            self.count += n_dev.reshape(()).round().long()
            rate = n_dev / self.count
            mean_x, var_x = g_mean, m2
        else:
            self.count += n
            rate = n / self.count
        delta = mean_x - self._mean
        self._mean += rate * delta
        self._var += rate * (var_x - self._var + delta * (mean_x - self._mean))
        self._std = torch.sqrt(self._var)


# ---------------------------------------------------------------------------------------------- storage
class RolloutStorage:
    """(T, N, ...) device tensors of one PPO iteration (rsl_rl RolloutStorage).

    Recurrent policies: ``save_start_states`` takes the memories' states as they were BEFORE the act / evaluate of
    t = 0 and those only (rsl_rl keeps every step's).  PPO.process_env_step zeroes the state right after a done, so every
    trajectory that starts later than t = 0 starts from zeros, and recurrent_mini_batch_generator needs no more."""

    def __init__(self, num_envs, num_steps, obs_dim, critic_obs_dim, num_actions, device, rnd_state_dim=None):
        T, N = num_steps, num_envs
        self.num_envs, self.num_steps, self.device = N, T, device
        z = lambda *s: torch.zeros(*s, device=device)  # noqa: E731
        self.t = {
            "observations": z(T, N, obs_dim),
            "actions": z(T, N, num_actions),
            "rewards": z(T, N, 1),
            "dones": z(T, N, 1),
            "values": z(T, N, 1),
            "actions_log_prob": z(T, N, 1),
            "mu": z(T, N, num_actions),
            "sigma": z(T, N, num_actions),
            "returns": z(T, N, 1),
            "advantages": z(T, N, 1),
        }
        if critic_obs_dim is not None:
            self.t["privileged_observations"] = z(T, N, critic_obs_dim)
        if rnd_state_dim is not None:  # Random Network Distillation: the normalised rnd_state rows
            self.t["rnd_state"] = z(T, N, rnd_state_dim)
        self.step = 0

    def __getattr__(self, k):
        t = self.__dict__.get("t")
        if t is not None and k in t:
            return t[k]
        raise AttributeError(k)

    def add(self, obs, critic_obs, actions, rewards, dones, values, log_prob, mu, sigma, rnd_state=None):
        if self.step >= self.num_steps:
            raise OverflowError("rollout buffer overflow; call clear() before adding new transitions")
        s = self.step
        t = self.t
        t["observations"][s].copy_(obs)
        if "privileged_observations" in t and critic_obs is not None:
            t["privileged_observations"][s].copy_(critic_obs)
        t["actions"][s].copy_(actions)
        t["rewards"][s].copy_(rewards.view(-1, 1))
        t["dones"][s].copy_(dones.view(-1, 1))
        t["values"][s].copy_(values)
        t["actions_log_prob"][s].copy_(log_prob.view(-1, 1))
        t["mu"][s].copy_(mu)
        t["sigma"][s].copy_(sigma)
        if rnd_state is not None:
            t["rnd_state"][s].copy_(rnd_state)
        self.step += 1

    def clear(self):
        self.step = 0

    def save_start_states(self, hidden_states):
        """Copies of (actor memory state, critic memory state) at t = 0; a memory that has not stepped yet (None) is
        recorded as None and read as zeros.  The copies are ordinary tensors also when collection runs in inference
        mode: the update's LSTM saves them for its backward."""
        with torch.inference_mode(False):
            self.start_states = [None if h is None else tuple(torch.empty(x.shape, dtype=x.dtype, device=self.device)
                                                              for x in state_tensors(h)) for h in hidden_states]
        for dst, h in zip(self.start_states, hidden_states):
            if dst is not None:
                for d, x in zip(dst, state_tensors(h)):
                    d.copy_(x)

    def recurrent_mini_batch_generator(self, num_mini_batches: int, num_epochs: int = 8, memories=None):
        """rsl_rl's recurrent generator.  Minibatches split over ENVS (mini_batch_size = num_envs // num_mini_batches),
        in env order.  Yields, per epoch and minibatch, a dict: the padded observation trajectories of those envs
        ("observations", "critic_observations": [T, n_traj, ...]) with their "masks" [T, n_traj], the trajectories'
        start states ("hidden_a", "hidden_c": per state tensor [layers, n_traj, H]; the stored t = 0 state for an env's
        first trajectory, zeros for the others), and the [T, envs, ...] slices of actions, values, returns,
        advantages, actions_log_prob, mu and sigma.  ``memories``: the (actor, critic) Memory modules, read for the state
        shapes when a memory had not stepped before t = 0."""
        t = self.t
        T, N = self.num_steps, self.num_envs
        obs_traj, masks = split_and_pad_trajectories(t["observations"], t["dones"])
        cobs_traj = (split_and_pad_trajectories(t["privileged_observations"], t["dones"])[0] if "privileged_observations" in t
                     else obs_traj)
        starts = torch.zeros(T, N, dtype=torch.bool, device=self.device)  # a trajectory starts at (t, env)
        starts[0] = True
        starts[1:] = t["dones"][:-1, :, 0] != 0
        per_env = starts.sum(0)
        first = torch.cat([per_env.new_zeros(1), per_env.cumsum(0)]).tolist()  # env e's first trajectory
        mb = N // num_mini_batches
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                e0, e1 = i * mb, (i + 1) * mb
                k0, k1 = first[e0], first[e1]
                at = torch.tensor(first[e0:e1], device=self.device) - k0
                hidden = []
                for which in (0, 1):
                    saved = self.start_states[which] if getattr(self, "start_states", None) else None
                    if saved is None:
                        rnn = memories[which].rnn
                        n_state = 2 if isinstance(rnn, nn.LSTM) else 1
                        saved = tuple(torch.zeros(rnn.num_layers, N, rnn.hidden_size, device=self.device)
                                      for _ in range(n_state))
                    states = []
                    for s0 in saved:
                        h = torch.zeros(s0.shape[0], k1 - k0, s0.shape[2], device=self.device, dtype=s0.dtype)
                        h[:, at] = s0[:, e0:e1]
                        states.append(h)
                    hidden.append(tuple(states) if len(states) > 1 else states[0])
                out = {"observations": obs_traj[:, k0:k1], "critic_observations": cobs_traj[:, k0:k1],
                       "masks": masks[:, k0:k1], "hidden_a": hidden[0], "hidden_c": hidden[1]}
                for k in ("actions", "values", "returns", "advantages", "actions_log_prob", "mu", "sigma"):
                    out[k] = t[k][:, e0:e1]
                yield out

    def recurrent_env_mini_batch_generator(self, num_mini_batches: int, num_epochs: int = 8, memories=None):
        """The sequence form of recurrent_mini_batch_generator: the same env split and order, nothing cut or padded, so
        every yield has fixed shapes and nothing here reads a device value on the host.  Yields a dict: the
        [T, e0:e1, ...] slices "observations", "critic_observations" and "dones" ([T, envs] bytes), the envs' t = 0
        states "hidden_a" / "hidden_c" (per state tensor [layers, envs, H]; zeros for a memory that had not stepped), and
        the same per-sample slices as recurrent_mini_batch_generator.  The networks read them through
        h12env.recurrent.lstm_sequence, which zeroes the state after a done."""
        t = self.t
        N = self.num_envs
        cobs = t["privileged_observations"] if "privileged_observations" in t else t["observations"]
        dones = (t["dones"][:, :, 0] != 0).to(torch.uint8)
        saved_states = []
        for which in (0, 1):
            saved = self.start_states[which] if getattr(self, "start_states", None) else None
            if saved is None:
                rnn = memories[which].rnn
                n_state = 2 if isinstance(rnn, nn.LSTM) else 1
                saved = tuple(torch.zeros(rnn.num_layers, N, rnn.hidden_size, device=self.device)
                              for _ in range(n_state))
            saved_states.append(saved)
        mb = N // num_mini_batches
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                e0, e1 = i * mb, (i + 1) * mb
                hidden = [tuple(s0[:, e0:e1] for s0 in saved) for saved in saved_states]
                hidden = [h if len(h) > 1 else h[0] for h in hidden]
                out = {"observations": t["observations"][:, e0:e1], "critic_observations": cobs[:, e0:e1],
                       "dones": dones[:, e0:e1], "hidden_a": hidden[0], "hidden_c": hidden[1]}
                for k in ("actions", "values", "returns", "advantages", "actions_log_prob", "mu", "sigma"):
                    out[k] = t[k][:, e0:e1]
                yield out

    def compute_returns(self, last_values, gamma, lam, normalize_advantage=True):
        """GAE(gamma, lambda) backwards over the T steps, bootstrapped by last_values."""
        t = self.t
        adv = 0
        for s in reversed(range(self.num_steps)):
            nxt = last_values if s == self.num_steps - 1 else t["values"][s + 1]
            not_done = 1.0 - t["dones"][s]
            delta = t["rewards"][s] + not_done * gamma * nxt - t["values"][s]
            adv = delta + not_done * gamma * lam * adv
            t["returns"][s] = adv + t["values"][s]
        t["advantages"].copy_(t["returns"] - t["values"])
        if normalize_advantage:
            a = t["advantages"]
            t["advantages"].copy_((a - a.mean()) / (a.std() + 1e-8))


# ---------------------------------------------------------------------------------------------- PPO
def enable_tunable_gemm():
    """PyTorch's TunableOp for the learner's GEMMs: the first call of each GEMM shape times the available
    hipBLASLt / rocBLAS solutions and keeps the fastest for the process (the minibatch shapes are fixed, so a few
    seconds once per run).  Round 4, C3 at 4096 envs, 2 runs each: learning 38.6 / 38.5 ms per iteration against 41.3
    / 40.8 ms with the default heuristics (profiles/r4/r4t_blas_tunableop_ab.txt).

    OPT-IN (H12_TUNABLEOP=1, or bench.py --mode train --tunableop): the selection is the fastest solution of a timing
    run, so it can differ between runs and between ranks -- two runs with the same seed are then not bit-reproducible
    (each rank's GEMMs may round differently), and the switch is process-wide (every GEMM in the process is tuned).
    With PYTORCH_TUNABLEOP_FILENAME set to an existing tuning table the recorded selections are reused with tuning
    off (reproducible); otherwise the table is written to the temp directory."""
    import tempfile

    t = torch.cuda.tunable
    if not t.is_enabled():
        fixed = os.environ.get("PYTORCH_TUNABLEOP_FILENAME")
        if fixed and os.path.exists(fixed):
            t.enable(True)
            t.tuning_enable(False)  # a checked tuning table: its selections, no timing runs
            t.read_file(fixed)
            return
        if not fixed:
            t.set_filename(os.path.join(tempfile.gettempdir(), f"h12env_tunableop_{os.getpid()}_%d.csv"))
        t.enable(True)
        t.tuning_enable(True)


class _DeviceLrAdam:
    """The optimizer of PPO and of h12env.distill.Distillation: Adam over ``self.policy``'s parameters."""

    def _init_optimizer(self, learning_rate, fused_optimizer: bool = False) -> bool:
        """fused Adam (one kernel for all parameters) on the GPU with the learning rate as a device tensor, so
        the KL-adaptive schedule runs on the device (no host sync per minibatch); plain Adam on CPU.  Returns whether
        it is the fused one.  ``fused_optimizer``: on the GPU, h12env.optim.FusedClipAdam instead, which clips to
        ``self.max_grad_norm`` inside its step; ``self.fused_optimizer`` says whether it is in use."""
        fused = str(self.device).startswith("cuda")
        self._lr_t = torch.tensor(float(learning_rate), device=self.device) if fused else None
        self.fused_optimizer = bool(fused_optimizer) and fused
        if self.fused_optimizer:
            from .optim import FusedClipAdam

            self.optimizer = FusedClipAdam(self.policy.parameters(), lr=self._lr_t, max_norm=self.max_grad_norm)
        else:
            self.optimizer = torch.optim.Adam(self.policy.parameters(), lr=self._lr_t if fused else learning_rate,
                                              fused=fused, capturable=fused)
        self.learning_rate = learning_rate
        return fused

    def optimizer_state_dict(self) -> dict:
        """The optimizer state with a plain-float learning rate (rsl_rl's checkpoint layout)."""
        sd = self.optimizer.state_dict()
        for g in sd["param_groups"]:
            if torch.is_tensor(g["lr"]):
                g["lr"] = float(g["lr"])
        return sd

    def load_optimizer_state_dict(self, sd: dict):
        self.optimizer.load_state_dict(sd)
        lr = float(self.optimizer.param_groups[0]["lr"])
        self.learning_rate = lr
        if self._lr_t is not None:  # keep the device tensor the schedule updates in the param groups
            self._lr_t.fill_(lr)
            for g in self.optimizer.param_groups:
                g["lr"] = self._lr_t


class PPO(_DeviceLrAdam):
    """Clipped-surrogate PPO with clipped value loss, entropy bonus and KL-adaptive learning rate
    (rsl_rl 2.3 algorithms/ppo.py semantics)."""

    def __init__(self, policy, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, gamma=0.998, lam=0.95,
                 value_loss_coef=1.0, entropy_coef=0.0, learning_rate=1e-3, max_grad_norm=1.0,
                 use_clipped_value_loss=True, schedule="fixed", desired_kl=0.01, device="cpu",
                 normalize_advantage_per_mini_batch=False, shard: D.Shard | None = None, precision: str = "fp32",
                 symmetry_cfg: dict | None = None, fused_learner: bool | None = None, fused_loss: bool | None = None,
                 fused_rnn_update: bool | None = None, rnd_cfg: dict | None = None,
                 fused_optimizer: bool | None = None, **kwargs):
        self.policy = policy.to(device)
        self.actor_critic = self.policy  # rsl_rl < 2.3 name
        self.device = device
        if str(device).startswith("cuda") and os.environ.get("H12_TUNABLEOP", "0") == "1":
            enable_tunable_gemm()
        # opt-in: gradient clip and Adam step as two HIP launches (h12env.optim.FusedClipAdam) on the GPU;
        # _minibatch then leaves its clip_grad_norm_ call out.  None reads H12_OPTIMIZER_FUSED=1.  The default stays
        # torch's clip and fused Adam.  Distillation and the RND predictor keep torch's Adam.
        if fused_optimizer is None:
            from .optim import fused_optimizer_enabled

            fused_optimizer = fused_optimizer_enabled()
        if fused_optimizer and shard is not None and shard.world > 1:
            raise ValueError("fused_optimizer with more than one rank is not supported (the gradients are averaged "
                             "across ranks between backward and the clip)")
        self.max_grad_norm = max_grad_norm
        fused = self._init_optimizer(learning_rate, fused_optimizer)
        self._graph = None
        self._fused = None
        self.num_learning_epochs = num_learning_epochs
        self.num_mini_batches = num_mini_batches
        self.clip_param = clip_param
        self.gamma, self.lam = gamma, lam
        self.value_loss_coef, self.entropy_coef = value_loss_coef, entropy_coef
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.schedule, self.desired_kl = schedule, desired_kl
        self.normalize_advantage_per_mini_batch = normalize_advantage_per_mini_batch
        self.shard = shard or D.Shard(0, 1, 0, 0)
        self.storage: RolloutStorage | None = None
        self._update_count = 0
        # "bf16": autocast the learning-phase forward/backward GEMMs to bf16 MFMA (the reference trains with
        # TF32 matmuls enabled on NVIDIA, train.py:70-71; gfx950 has no TF32); "fp32": exact fp32
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be fp32 or bf16, got {precision!r}")
        self.precision = precision
        # opt-in: the update's actor and critic on the fused HIP forward / backward (h12env.policy.TrainableFusedMLP,
        # DESIGN 7l).  None reads H12_LEARNER_FUSED=1.  The collection (_act_body) is untouched; on CPU the torch
        # modules run.  The default stays the torch path.
        if fused_learner is None:
            from .policy import learner_fused_enabled

            fused_learner = learner_fused_enabled()
        self.fused_learner = bool(fused_learner)
        self.recurrent = bool(getattr(policy, "is_recurrent", False))
        if self.recurrent:  # the update of a recurrent policy is the eager library-LSTM path only
            for name, on in (("fused_learner", fused_learner), ("fused_loss", fused_loss), ("symmetry_cfg", symmetry_cfg),
                             ("shard.world > 1", self.shard.world > 1)):
                if name == "fused_loss" and on is None:
                    from .ppo_head import fused_loss_enabled

                    on = fused_loss_enabled()
                if on:
                    raise ValueError(f"{name} is not supported with a recurrent policy ({type(policy).__name__})")
        # opt-in: a recurrent policy's update in the sequence form (h12env.recurrent.lstm_sequence): the
        # memories run over [T, envs of the minibatch] with the state zeroed after a done, on the h12learn_lstm_seq_*
        # kernels on the GPU; no trajectories are cut or padded.  None reads H12_RNN_UPDATE_FUSED=1.  The default stays
        # the library LSTM over padded trajectories.
        if fused_rnn_update is None:
            fused_rnn_update = os.environ.get("H12_RNN_UPDATE_FUSED", "0") == "1"
        self.fused_rnn_update = bool(fused_rnn_update)
        if self.fused_rnn_update:
            from .recurrent import lstm_sequence_limit

            if not self.recurrent:
                raise ValueError(f"fused_rnn_update needs a recurrent policy, {type(policy).__name__} has no memory")
            if precision == "bf16":
                raise ValueError("fused_rnn_update: the sequence kernels are exact fp32, precision='bf16' is not "
                                 "supported")
            for name in ("memory_a", "memory_c"):
                why = lstm_sequence_limit(getattr(self.policy, name).rnn)
                if why:
                    raise ValueError(f"fused_rnn_update: {name}: {why}")
        if self.fused_learner:
            if precision == "bf16":
                raise ValueError("fused_learner: the fused kernels are exact fp32, precision='bf16' is not supported")
            if not hasattr(self.policy, "enable_fused_learner"):
                raise ValueError(f"fused_learner: {type(self.policy).__name__} has no enable_fused_learner()")
            try:
                self.policy.enable_fused_learner()
            except ValueError as e:
                raise ValueError(f"fused_learner: the policy's networks cannot run on the fused kernels "
                                 f"(Linear/ELU only, every width at most the kernels' maximum): {e}") from e
        # opt-in: everything between the networks' outputs and loss.backward() as one autograd node on one HIP call
        # (h12env.ppo_head.PPOHead).  None reads H12_PPO_HEAD_FUSED=1.  On CPU the node evaluates the torch
        # expressions.  The default stays the torch path.
        if fused_loss is None:
            from .ppo_head import fused_loss_enabled

            fused_loss = fused_loss_enabled()
        self.fused_loss = bool(fused_loss)
        if self.fused_loss:
            from . import _learn

            if normalize_advantage_per_mini_batch:
                raise ValueError("fused_loss: normalize_advantage_per_mini_batch=True needs a two-pass mean / std over "
                                 "the minibatch's advantages, which the fused loss head does not compute")
            std_param = getattr(self.policy, "std", None) if getattr(self.policy, "noise_std_type", None) == "scalar" \
                else getattr(self.policy, "log_std", None)
            if std_param is None:
                raise ValueError(f"fused_loss: {type(self.policy).__name__} has no state-independent std / log_std "
                                 "parameter")
            if std_param.numel() > _learn.ppo_head_max_actions():
                raise ValueError(f"fused_loss: {std_param.numel()} actions, the fused loss head supports at most "
                                 f"{_learn.ppo_head_max_actions()}")
        # rsl_rl 2.3 symmetry: mirror-image data augmentation and / or mirror loss; with both switches off the
        # symmetry loss is computed for logging only.  None: the update is untouched.
        self.symmetry = None
        if symmetry_cfg is not None:
            from .symmetry import resolve_func

            s = dict(symmetry_cfg)
            self.symmetry = {"use_data_augmentation": bool(s.get("use_data_augmentation", False)),
                             "use_mirror_loss": bool(s.get("use_mirror_loss", False)),
                             "mirror_loss_coeff": float(s.get("mirror_loss_coeff", 0.0)),
                             "data_augmentation_func": resolve_func(s.get("data_augmentation_func")),
                             "_env": s.get("_env")}
        self._n_stats = 3 if self.symmetry is None else 4
        # rsl_rl 2.3 rnd_cfg: Random Network Distillation (h12env.rnd).  None: nothing changes.  The cfg
        # arrives resolved (num_states set, weight scaled by step_dt: rnd.resolve_rnd_cfg, the runner's part).
        self.rnd = None
        if rnd_cfg is not None:
            self._init_rnd(dict(rnd_cfg), symmetry_cfg, fused)

    def _init_rnd(self, cfg: dict, symmetry_cfg, fused_adam: bool):
        from . import rnd as R

        R.check_rnd_cfg(cfg)
        for what, on in (("a recurrent policy", self.recurrent),
                         ("symmetry_cfg data augmentation", self.symmetry is not None
                          and self.symmetry["use_data_augmentation"]),
                         ("more than one rank", self.shard.world > 1), ("precision='bf16'", self.precision == "bf16")):
            if on:
                raise ValueError(f"rnd_cfg with {what} is not supported")
        if "num_states" not in cfg:
            raise ValueError("rnd_cfg: num_states is missing (the runner sets it from the rnd_state observation group)")
        lr = float(cfg.pop("learning_rate", 1e-3))
        fused_rnd = cfg.pop("fused", None)
        if fused_rnd is None:
            fused_rnd = R.rnd_fused_enabled()
        cfg.setdefault("activation", "elu")
        self.rnd = R.RandomNetworkDistillation(device=self.device, **cfg)
        self.rnd_optimizer = torch.optim.Adam(self.rnd.predictor.parameters(), lr=lr, fused=fused_adam,
                                              capturable=fused_adam)
        # opt-in: the intrinsic-reward step of process_env_step on the h12learn_rnd_* kernels (rnd.FusedRND)
        self.rnd_fused = R.FusedRND(self.rnd) if fused_rnd else None
        self._n_stats += 1  # the rnd loss: the last column

    def init_storage(self, num_envs, num_steps, obs_shape, critic_obs_shape, action_shape):
        self.storage = RolloutStorage(num_envs, num_steps, obs_shape[0],
                                      None if critic_obs_shape is None else critic_obs_shape[0], action_shape[0],
                                      self.device, None if self.rnd is None else self.rnd.num_states)

    # ---- collection
    def act(self, obs, critic_obs):
        if self.recurrent:
            self._obs_rows = obs.shape[0]
            if self.storage is not None and self.storage.step == 0:  # the states as they are before this step
                self.storage.save_start_states(self.policy.get_hidden_states())
        if self._act_graph_ok(obs, critic_obs):
            return self._act_graphed(obs, critic_obs)
        self._obs, self._critic_obs = obs, critic_obs
        if fused_collection_on(obs):  # eager collection on the fused forward: the graphed body, run directly
            with torch.no_grad():
                out = self._act_compute(obs, critic_obs)
            self._actions, self._values, self._log_prob, self._mu, self._sigma = out
            return self._actions
        self._actions = self.policy.act(obs).detach()
        self._values = self.policy.evaluate(critic_obs).detach()
        self._log_prob = self.policy.get_actions_log_prob(self._actions).detach()
        self._mu = self.policy.action_mean.detach()
        self._sigma = self.policy.action_std.detach()
        return self._actions

    # ---- collection as a HIP graph: actor + critic forward, Gaussian sample, log-probability in one launch
    def _act_graph_ok(self, obs, critic_obs) -> bool:
        # a recurrent policy's collection is captured on the fused step only: it updates the state in place
        return (obs.is_cuda and not torch.is_grad_enabled() and graph_enabled()
                and (not self.recurrent or fused_collection_on(obs)))

    def _fused_states(self):
        """The (h, c) [N][H] views of the two memories' states for h12learn_lstm_step, which updates them in place.  A
        memory that has not stepped gets zeros; the memories keep their storage from here on (Memory.keep_storage), so
        the torch step of compute_returns and reset(dones) write into the same tensors the captured graph points to."""
        from .policy import lstm_step_limit

        out = []
        n = self._obs_rows
        for mem in (self.policy.memory_a, self.policy.memory_c):
            why = lstm_step_limit(mem.rnn)
            if why:
                raise ValueError(f"H12_POLICY_FUSED=1: {why}; unset it to collect on the torch path")
            hs = mem.hidden_states
            if hs is None or any(t.is_inference() for t in hs):
                with torch.inference_mode(False):
                    new = tuple(torch.zeros(1, n, mem.rnn.hidden_size, device=self.device) for _ in range(2))
                if hs is not None:
                    for d, t in zip(new, hs):
                        d.copy_(t)
                hs = mem.hidden_states = new
            mem.keep_storage = True
            out.append((hs[0][0], hs[1][0]))
        return out

    def _act_fused(self, obs, cobs):
        """H12_POLICY_FUSED=1: actor mean and critic value from policy.FusedActorCritic; a recurrent policy's memories
        are stepped in place on their own storage."""
        if self._fused is None:
            p = self.policy
            self._fused = FusedActorCritic(p.actor, p.critic,
                                           (p.memory_a.rnn, p.memory_c.rnn) if self.recurrent else None)
        return self._fused(obs, cobs, self._fused_states() if self.recurrent else None)

    def _act_compute(self, obs, cobs):
        fused = fused_collection_on(obs)
        if fused:
            mean, values = self._act_fused(obs, cobs)
        else:
            mean = self.policy.actor(obs)
        std = self.policy._std(mean)
        # mean + std * N(0, 1): the same Normal(mean, std) sample as distribution.sample(), from randn (capturable)
        actions = mean + std * torch.randn_like(mean)
        if not fused:
            values = self.policy.critic(cobs)
        log_prob = Normal(mean, std).log_prob(actions).sum(dim=-1)
        return actions, values, log_prob, mean, std

    def _act_graphed(self, obs, critic_obs):
        key = (tuple(obs.shape), tuple(critic_obs.shape), critic_obs is obs, obs.dtype)
        states = [t for pair in self._fused_states() for t in pair] if self.recurrent else []
        key += tuple(t.data_ptr() for t in states)
        if getattr(self, "_ga", None) is None or self._ga_key != key:
            # normal (not inference) tensors throughout: the graph's RNG state is updated outside inference mode.
            # The warm-up steps a recurrent policy's state and consumes exploration-noise draws: capture() puts both
            # back, so the replays draw the same noise sequence as the eager path (graph-safe philox offsets)
            with torch.inference_mode(False), torch.no_grad():
                self._ga_obs = torch.zeros(obs.shape, dtype=obs.dtype, device=obs.device)
                self._ga_cobs = (self._ga_obs if critic_obs is obs else
                                 torch.zeros(critic_obs.shape, dtype=critic_obs.dtype, device=obs.device))
                self._ga, self._ga_out = capture(lambda: self._act_compute(self._ga_obs, self._ga_cobs), obs.device,
                                                 undo=states, rng=True)
            self._ga_key = key
        self._ga_obs.copy_(obs)
        if critic_obs is not obs:
            self._ga_cobs.copy_(critic_obs)
        self._ga.replay()
        self._obs, self._critic_obs = obs, critic_obs
        self._actions, self._values, self._log_prob, self._mu, self._sigma = self._ga_out
        return self._actions

    def process_env_step(self, rewards, dones, infos):
        r = rewards.clone().float()
        rnd_state = None
        if self.rnd is not None:  # r += intrinsic, before the bootstrap (rsl_rl ppo.py)
            state = infos.get("observations", {}).get("rnd_state")
            if state is None:
                raise ValueError("rnd_cfg: the env step returned no 'rnd_state' observation group")
            state = state.to(self.device)
            if self.rnd_fused is not None:
                self.intrinsic_rewards, r, rnd_state = self.rnd_fused(state, r)
            else:
                self.intrinsic_rewards, rnd_state = self.rnd.get_intrinsic_reward(state)
                r += self.intrinsic_rewards
        if "time_outs" in infos:  # bootstrap on time-outs (rsl_rl ppo.py)
            r += self.gamma * (self._values.squeeze(1) * infos["time_outs"].to(self.device).float())
        self.storage.add(self._obs, self._critic_obs if self.storage.t.get("privileged_observations") is not None else None,
                         self._actions, r, dones.float(), self._values, self._log_prob, self._mu, self._sigma,
                         rnd_state)
        self.policy.reset(dones)

    def compute_returns(self, last_critic_obs):
        last_values = self.policy.evaluate(last_critic_obs).detach()
        # multi-GPU: advantages are normalised over the all-gathered global batch in _batch()
        self.storage.compute_returns(last_values, self.gamma, self.lam,
                                     normalize_advantage=not self.normalize_advantage_per_mini_batch
                                     and self.shard.world == 1)

    # ---- learning
    def _batch(self):
        """Flattened (T*N_global, ...) views of the (all-gathered) rollout."""
        st = self.storage.t
        if self.shard.world > 1:
            keys = [k for k in st if k not in ("rewards", "dones")]
            g = D.allgather_rollout({k: st[k] for k in keys}, self.shard, env_dim=1)
            if not self.normalize_advantage_per_mini_batch:
                a = g["advantages"]
                g["advantages"] = (a - a.mean()) / (a.std() + 1e-8)
        else:
            g = st
        return {k: v.reshape(-1, *v.shape[2:]) for k, v in g.items() if k not in ("rewards", "dones")}

    def _allreduce_grads(self):
        if self.shard.world == 1:
            return
        grads = [p.grad for p in self.policy.parameters() if p.grad is not None]
        flat = torch.cat([g.reshape(-1) for g in grads])
        D.all_reduce(flat, op=dist.ReduceOp.SUM)
        flat /= self.shard.world
        off = 0
        for g in grads:
            n = g.numel()
            g.copy_(flat[off:off + n].view_as(g))
            off += n

    def _adapt_lr(self, kl_mean: torch.Tensor):
        """rsl_rl's KL-adaptive schedule on a minibatch's mean KL (averaged over the ranks first): on the device tensor
        the fused optimizer reads, without a host sync, or on the host learning rate."""
        with torch.no_grad():
            if self.shard.world > 1:
                D.all_reduce(kl_mean, op=dist.ReduceOp.SUM)
                kl_mean /= self.shard.world
            if self._lr_t is not None:
                lr = self._lr_t
                up = kl_mean > self.desired_kl * 2.0
                down = (kl_mean > 0.0) & (kl_mean < self.desired_kl / 2.0)
                self._lr_t.copy_(torch.where(up, torch.clamp(lr / 1.5, min=1e-5),
                                             torch.where(down, torch.clamp(lr * 1.5, max=1e-2), lr)))
            else:
                k = kl_mean.item()
                if k > self.desired_kl * 2.0:
                    self.learning_rate = max(1e-5, self.learning_rate / 1.5)
                elif 0.0 < k < self.desired_kl / 2.0:
                    self.learning_rate = min(1e-2, self.learning_rate * 1.5)
                for g in self.optimizer.param_groups:
                    g["lr"] = self.learning_rate

    def _minibatch(self, b: dict, idx: torch.Tensor | None, stats: torch.Tensor, rec: dict | None = None):
        """One PPO minibatch update (rsl_rl ppo.py update loop body): gather, forward, KL-adaptive learning
        rate, clipped surrogate + clipped value loss, backward, (all-reduce), grad clip, Adam, statistics.
        Host-sync free on the fused path, so it is also the body of the captured HIP graph.

        With fused_loss only the observations are gathered here (and the actions where they are mirrored); everything
        from get_actions_log_prob to loss is one PPOHead node, which on a single CUDA rank also applies the adaptive
        schedule to _lr_t and, without symmetry, adds the statistics.

        ``rec`` (a recurrent policy; b and idx are then None): one yield of recurrent_mini_batch_generator.  The networks
        run in batch mode over its padded trajectories; the per-sample tensors are its [T, envs, ...] slices.  With
        fused_rnn_update it is one yield of recurrent_env_mini_batch_generator (no "masks") and the memories run in
        sequence mode."""
        sym = self.symmetry
        fused = self.fused_loss
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        aug = sym is not None and sym["use_data_augmentation"]
        n_orig = 0 if rec is not None else idx.shape[0]
        if rec is not None:
            obs, critic_obs, actions = rec["observations"], rec["critic_observations"], rec["actions"]
        elif aug:  # rows [0, B) the minibatch, rows [B, 2B) its mirror image
            obs, actions = self._augment(b["observations"], b["actions"], idx, "policy")
            critic_obs = (self._augment(b["privileged_observations"], None, idx, "critic")[0]
                          if "privileged_observations" in b else obs)
        else:
            obs = b["observations"][idx]
            critic_obs = b["privileged_observations"][idx] if "privileged_observations" in b else obs
            actions = b["actions"] if fused else b["actions"][idx]  # the head gathers its rows itself
        if rec is not None:
            target_values, advantages, returns = rec["values"], rec["advantages"], rec["returns"]
            old_log_prob, old_mu, old_sigma = rec["actions_log_prob"], rec["mu"], rec["sigma"]
            if self.normalize_advantage_per_mini_batch:
                advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
        elif not fused:
            target_values = b["values"][idx]
            advantages = b["advantages"][idx]
            returns = b["returns"][idx]
            old_log_prob = b["actions_log_prob"][idx]
            old_mu, old_sigma = b["mu"][idx], b["sigma"][idx]
            if self.normalize_advantage_per_mini_batch:
                advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
            if aug:  # the mirrored samples keep their originals' statistics (normalised above on the original batch)
                old_log_prob, target_values, advantages, returns = (torch.cat([t, t]) for t in
                                                                    (old_log_prob, target_values, advantages, returns))
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16, cache_enabled=False,
                            enabled=self.precision == "bf16" and str(self.device).startswith("cuda")):
            if rec is not None and "masks" not in rec:  # sequence mode (fused_rnn_update): [T, envs], reset after a done
                if obs.is_cuda:  # both memories in one two-network call
                    value = self.policy.act_and_evaluate_sequence(obs, critic_obs, rec["dones"], rec["hidden_a"],
                                                                  rec["hidden_c"]).float()
                else:
                    self.policy.act(obs, dones=rec["dones"], hidden_states=rec["hidden_a"])
                    value = self.policy.evaluate(critic_obs, dones=rec["dones"], hidden_states=rec["hidden_c"]).float()
            elif rec is not None:  # batch mode: the library LSTM over the padded trajectories, from their start states
                self.policy.act(obs, masks=rec["masks"], hidden_states=rec["hidden_a"])
                value = self.policy.evaluate(critic_obs, masks=rec["masks"], hidden_states=rec["hidden_c"]).float()
            else:
                self.policy.update_distribution(obs)  # rsl_rl calls act(); the sample itself is unused
                value = self.policy.evaluate(critic_obs).float()
        if self.precision == "bf16":  # distribution statistics in fp32
            self.policy.distribution = Normal(self.policy.distribution.mean.float(),
                                              self.policy.distribution.stddev.float())
        if fused:
            from .ppo_head import HeadInputs, PPOHead

            mean = self.policy.action_mean
            kind = self.policy.noise_std_type
            head = HeadInputs(idx=idx, old_log_prob=b["actions_log_prob"], advantages=b["advantages"],
                              returns=b["returns"], target_values=b["values"], old_mu=b["mu"], old_sigma=b["sigma"],
                              actions=actions, actions_direct=aug, std_kind=kind, clip_param=self.clip_param,
                              value_loss_coef=self.value_loss_coef, entropy_coef=self.entropy_coef,
                              use_clipped_value_loss=self.use_clipped_value_loss,
                              lr=self._lr_t if mean.is_cuda and adaptive and self.shard.world == 1 else None,
                              desired_kl=self.desired_kl,
                              stats_accum=stats[:3] if mean.is_cuda and sym is None else None)
            loss, out = PPOHead.apply(mean, value, self.policy.std if kind == "scalar" else self.policy.log_std, head)
            if adaptive and head.lr is None:  # CPU, or several ranks: the KL from the head
                self._adapt_lr(out[3].clone())
        else:
            log_prob = self.policy.get_actions_log_prob(actions)
            mu, sigma, entropy = self.policy.action_mean, self.policy.action_std, self.policy.entropy
            if aug:  # the KL of the schedule and the entropy bonus are those of the original samples
                mu, sigma, entropy = mu[:n_orig], sigma[:n_orig], entropy[:n_orig]
            if adaptive:
                with torch.no_grad():
                    kl = torch.sum(torch.log(sigma / old_sigma + 1e-5)
                                   + (old_sigma.square() + (old_mu - mu).square()) / (2.0 * sigma.square()) - 0.5,
                                   dim=-1)
                    self._adapt_lr(kl.mean())
            ratio = torch.exp(log_prob - old_log_prob.squeeze(-1))
            adv = advantages.squeeze(-1)
            surrogate = -adv * ratio
            surrogate_clipped = -adv * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)
            surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
            if self.use_clipped_value_loss:
                v_clipped = target_values + (value - target_values).clamp(-self.clip_param, self.clip_param)
                value_loss = torch.max((value - returns).square(), (v_clipped - returns).square()).mean()
            else:
                value_loss = (returns - value).square().mean()
            loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * entropy.mean()
        if sym is not None:
            symmetry_loss = self._symmetry_loss(obs, aug, n_orig)
            if sym["use_mirror_loss"]:
                loss = loss + sym["mirror_loss_coeff"] * symmetry_loss
        self.optimizer.zero_grad(set_to_none=True)  # backward writes the grads (no fill + add)
        loss.backward()
        self._allreduce_grads()
        if not self.fused_optimizer:  # FusedClipAdam clips inside its step
            nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
        self.optimizer.step()
        if self.rnd is not None:  # the predictor's own loss, backward and Adam, after the policy's
            s_b = b["rnd_state"][idx]
            with torch.no_grad():
                embedding = self.rnd.target(s_b)
            rnd_loss = nn.functional.mse_loss(self.rnd.predictor(s_b), embedding)
            self.rnd_optimizer.zero_grad(set_to_none=True)
            rnd_loss.backward()
            self.rnd_optimizer.step()
            stats[-1:] += rnd_loss.detach()
        if fused:  # value loss, surrogate, entropy: from the head, unless it has added them to stats itself
            parts = [out[1], out[0], out[2]] if head.stats_accum is None else None
        else:
            parts = [value_loss.detach(), surrogate_loss.detach(), entropy.mean().detach()]
        if parts is not None:
            parts = torch.stack(parts + ([symmetry_loss.detach()] if sym is not None else []))
            stats[:parts.shape[0]] += parts

    def _augment(self, obs, actions, idx, obs_type):
        """data_augmentation_func on the rows ``idx``.  h12env.symmetry.augment takes the index itself: gather, mirror
        and concatenation are then one h12learn_mirror_rows launch per tensor on the device."""
        from . import symmetry as S

        f, env = self.symmetry["data_augmentation_func"], self.symmetry["_env"]
        if f is S.augment:
            return f(obs=obs, actions=actions, env=env, obs_type=obs_type, idx=idx)
        return f(obs=None if obs is None else obs[idx], actions=None if actions is None else actions[idx], env=env,
                 obs_type=obs_type)

    def _symmetry_loss(self, obs, aug: bool, n_orig: int):
        """rsl_rl's mirror loss: the actor's mean on the mirrored observations against the mirror image of its mean
        on the originals (the target carries no gradient).  Without use_mirror_loss it is a logged number only."""
        sym = self.symmetry
        f, env = sym["data_augmentation_func"], sym["_env"]
        with torch.set_grad_enabled(sym["use_mirror_loss"] and torch.is_grad_enabled()):
            if not aug:
                obs = f(obs=obs, actions=None, env=env, obs_type="policy")[0]
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16, cache_enabled=False,
                                enabled=self.precision == "bf16" and str(self.device).startswith("cuda")):
                mean_all = self.policy.act_inference(obs.detach()).float()
            target = f(obs=None, actions=mean_all[:n_orig], env=env, obs_type="policy")[1].detach()
            return nn.functional.mse_loss(mean_all[n_orig:], target[n_orig:])

    def _graph_ok(self) -> bool:
        return (self._lr_t is not None and self.shard.world == 1 and str(self.device).startswith("cuda")
                and graph_enabled())

    def _capture(self, b: dict, mb: int):
        """Capture one minibatch update as a HIP graph (replayed num_epochs x num_mini_batches times per
        update): the ~300 kernel launches of a minibatch cost one graph launch.  The warm-up runs on the real
        parameters; they, the optimiser state, the learning rate and the statistics are restored bit-exactly before
        the capture."""
        self._g_idx = torch.zeros(mb, dtype=torch.long, device=self.device)
        self._g_stats = torch.zeros(self._n_stats, device=self.device)
        self.policy.distribution = None  # drop autograd graphs built on the default stream

        def drop_graphs_and_grads():
            self.policy.distribution = None
            self.optimizer.zero_grad(set_to_none=True)
            if self.rnd is not None:
                self.rnd_optimizer.zero_grad(set_to_none=True)

        undo = [TrainingState(self.policy.parameters(), self.optimizer, [self._lr_t, self._g_stats])]
        if self.rnd is not None:
            undo.append(TrainingState(self.rnd.predictor.parameters(), self.rnd_optimizer))
        self._graph, _ = capture(lambda: self._minibatch(b, self._g_idx, self._g_stats), self.device, undo=undo,
                                 before_capture=drop_graphs_and_grads)
        self._graph_key = (mb, tuple((k, v.data_ptr(), tuple(v.shape)) for k, v in sorted(b.items())))

    def _update_recurrent(self):
        """The update of a recurrent policy: eager, minibatches over envs.  From recurrent_mini_batch_generator the
        number of trajectories changes every iteration, so there is no graph to capture; with fused_rnn_update the
        shapes are fixed (recurrent_env_mini_batch_generator), and capturing it is left for later."""
        stats = torch.zeros(self._n_stats, device=self.device)
        n_updates = 0
        memories = (self.policy.memory_a, self.policy.memory_c)
        generator = (self.storage.recurrent_env_mini_batch_generator if self.fused_rnn_update
                     else self.storage.recurrent_mini_batch_generator)
        for rec in generator(self.num_mini_batches, self.num_learning_epochs, memories):
            self._minibatch(None, None, stats, rec=rec)
            n_updates += 1
        return stats, n_updates

    def update(self):
        if self.recurrent:
            stats, n_updates = self._update_recurrent()
            return self._finish_update(stats, n_updates)
        b = self._batch()
        n_total = b["observations"].shape[0]
        mb = n_total // self.num_mini_batches
        world, rank = self.shard.world, self.shard.rank
        gen = torch.Generator(device=self.device)
        use_graph = self._graph_ok()
        if use_graph:
            key = (mb, tuple((k, v.data_ptr(), tuple(v.shape)) for k, v in sorted(b.items())))
            if getattr(self, "_graph", None) is None or self._graph_key != key:
                self._capture(b, mb)
            stats = self._g_stats
            stats.zero_()
        else:
            stats = torch.zeros(self._n_stats, device=self.device)
        n_updates = 0
        for epoch in range(self.num_learning_epochs):
            # identical permutation on every rank (shared seed per epoch); each rank takes its share
            gen.manual_seed(1_000_003 * self._update_count + epoch)
            perm = torch.randperm(n_total, generator=gen, device=self.device)
            for i in range(self.num_mini_batches):
                idx = perm[i * mb:(i + 1) * mb]
                if world > 1:
                    share = mb // world
                    idx = idx[rank * share:(rank + 1) * share]
                if use_graph:
                    self._g_idx.copy_(idx)
                    self._graph.replay()
                else:
                    self._minibatch(b, idx, stats)
                n_updates += 1
        return self._finish_update(stats, n_updates)

    def _finish_update(self, stats, n_updates):
        self._update_count += 1
        self.storage.clear()
        if self._lr_t is not None:
            self.learning_rate = float(self._lr_t)
        v, sl, en, *rest = (stats / n_updates).tolist()
        out = {"value_function": v, "surrogate": sl, "entropy": en}
        if self.symmetry is not None:
            out["symmetry"] = rest[0]
        if self.rnd is not None:
            out["rnd"] = rest[-1]
            if self.rnd_fused is not None:
                self.rnd_fused.dirty = True  # the predictor moved: re-pack before the next collection step
        return out

    def load_optimizer_state_dict(self, sd: dict):
        super().load_optimizer_state_dict(sd)
        self._graph = None  # the captured graph holds the old state tensors

    def broadcast_parameters(self):
        if self.shard.world > 1:
            for p in self.policy.state_dict().values():
                D.broadcast(p, src=0)


# ---------------------------------------------------------------------------------------------- runner
@dataclass
class _Logger:
    log_dir: str | None
    rank: int

    def __post_init__(self):
        self._fh = None

    def write(self, it: int, scalars: dict):
        # the run directory is created lazily (a resume looks up the previous run before this one exists)
        if self._fh is None and self.log_dir and self.rank == 0:
            os.makedirs(self.log_dir, exist_ok=True)
            self._fh = open(os.path.join(self.log_dir, "metrics.jsonl"), "a")
        if self._fh:
            self._fh.write(json.dumps({"iter": it, **scalars}) + "\n")
            self._fh.flush()

    def close(self):
        if self._fh:
            self._fh.close()
            self._fh = None


class EpisodeStats:
    """rsl_rl's rewbuffer / lenbuffer: the reward sums and the lengths of the last 100 finished episodes, as
    ``buffers[stream]`` and ``buffers["length"]``, one deque per named reward stream.

    rsl_rl extends the deques at every step (a host sync per step); here ``step`` records the finished episodes on
    the device and ``flush`` moves them once per iteration, in the same order (step-major, env index within a
    step)."""

    def __init__(self, num_envs: int, device, streams=("reward",)):
        self.running = {k: torch.zeros(num_envs, device=device) for k in (*streams, "length")}
        self.buffers = {k: deque(maxlen=100) for k in self.running}
        self._done: list = []
        self._at_done = {k: [] for k in self.running}

    def step(self, dones, **rewards):
        """One env step: ``rewards[stream]`` [num_envs] for every stream, ``dones`` [num_envs].  Device work only."""
        for k, r in rewards.items():
            self.running[k] += r
        self.running["length"] += 1
        done = dones > 0
        self._done.append(done)
        for k, cur in self.running.items():
            self._at_done[k].append(torch.where(done, cur, 0.0))
            cur.masked_fill_(done, 0.0)

    def flush(self):
        """The episodes finished since the last flush go into the deques: one mask, then one indexed transfer per
        stream."""
        if not self._done:
            return
        m = torch.stack(self._done)
        self._done.clear()
        for k, rows in self._at_done.items():
            self.buffers[k].extend(torch.stack(rows)[m].cpu().tolist())
            rows.clear()


class OnPolicyRunner:
    """rsl_rl 2.3 OnPolicyRunner: collect num_steps_per_env transitions from every env, PPO update,
    log, checkpoint every save_interval iterations.

    h12env.distill.DistillationRunner is this runner around another algorithm.  What differs is in the methods after
    ``__init__``: ``_build_algorithm``, the four steps of ``learn`` (``_check_ready``, ``_first_inputs``,
    ``_step_inputs``, ``_end_collection``), ``_checkpoint_extras``, ``load``, ``_loss_scalars`` and the module names
    below."""

    _inference_modules = ("memory_a", "actor")  # of alg.policy: what get_inference_policy serves (memory: if recurrent)

    def __new__(cls, env=None, train_cfg: dict | None = None, *args, **kwargs):
        # algorithm.class_name = "Distillation" (with a StudentTeacher* policy) is served by h12env.distill's runner:
        # the same surface around another algorithm.  One of the two names without the other is refused there.
        if cls is OnPolicyRunner and train_cfg is not None:
            from .distill import DistillationRunner, wants_distillation

            if wants_distillation(train_cfg):
                return object.__new__(DistillationRunner)
        return object.__new__(cls)

    def __init__(self, env, train_cfg: dict, log_dir: str | None = None, device="cpu"):
        self.cfg = train_cfg
        self.alg_cfg = dict(train_cfg["algorithm"])
        self.policy_cfg = dict(train_cfg["policy"])
        self.device = device
        self.env = env
        self.shard = getattr(env, "shard", None) or _shard_from_env()
        # learner RNG per rank (IsaacLab's distributed train.py: seed + local rank), so the exploration noise
        # and init_at_random_ep_len draws differ between shards; parameters are broadcast from rank 0 below.
        # The env's own streams stay keyed by the global env id (shard-invariant trajectories).
        seed = int(train_cfg.get("seed", 1))
        torch.manual_seed(seed + self.shard.rank)
        self.num_steps_per_env = int(train_cfg["num_steps_per_env"])
        self.save_interval = int(train_cfg.get("save_interval", 50))
        self.empirical_normalization = bool(train_cfg.get("empirical_normalization", False))
        self._build_algorithm()
        self.log_dir = log_dir
        self.logger = _Logger(log_dir, self.shard.rank)
        self.tot_timesteps = 0
        self.tot_time = 0.0
        self.current_learning_iteration = 0
        self.git_status_repos: list[str] = []
        self.last_iteration_stats: dict = {}
        self.env.reset()

    def _normalizer(self, width: int) -> nn.Module:
        if self.empirical_normalization:
            return EmpiricalNormalization([width], until=1.0e8).to(self.device)
        return nn.Identity().to(self.device)

    def _build_algorithm(self):
        """self.alg with its storage, and the two observation normalisers."""
        env, device = self.env, self.device
        obs, extras = env.get_observations()
        num_obs = obs.shape[1]
        critic_obs = extras["observations"].get("critic")
        num_critic_obs = critic_obs.shape[1] if critic_obs is not None else num_obs
        class_name = self.policy_cfg.pop("class_name", None) or "ActorCritic"
        classes = {"ActorCritic": ActorCritic, "ActorCriticRecurrent": ActorCriticRecurrent}
        if class_name not in classes:
            raise ValueError(f"policy.class_name = {class_name!r}; this runner builds {sorted(classes)}")
        policy = classes[class_name](num_obs, num_critic_obs, env.num_actions, **self.policy_cfg).to(device)
        self.alg_cfg.pop("class_name", None)
        if self.alg_cfg.get("rnd_cfg") is not None:  # rsl_rl's runner: num_states and the step_dt factor
            from .rnd import resolve_rnd_cfg

            self.alg_cfg["rnd_cfg"] = resolve_rnd_cfg(self.alg_cfg["rnd_cfg"], env, extras["observations"])
        else:
            self.alg_cfg.pop("rnd_cfg", None)
        if self.alg_cfg.get("symmetry_cfg") is not None:  # rsl_rl hands the env to the augmentation function
            self.alg_cfg["symmetry_cfg"] = {**self.alg_cfg["symmetry_cfg"], "_env": env}
        self.alg = PPO(policy, device=device, shard=self.shard, **self.alg_cfg)
        self.alg.broadcast_parameters()
        self.obs_normalizer = self._normalizer(num_obs)
        self.critic_obs_normalizer = self._normalizer(num_critic_obs)
        self.alg.init_storage(env.num_envs, self.num_steps_per_env, [num_obs],
                              None if critic_obs is None else [num_critic_obs], [env.num_actions])

    # ---- the steps of learn() that depend on the algorithm
    def _check_ready(self):
        pass

    def _first_inputs(self):
        """alg.act's two inputs at the first step of learn(): the env's observations as they are (not normalised)."""
        obs, extras = self.env.get_observations()
        critic_obs = extras["observations"].get("critic", obs)
        return obs.to(self.device), critic_obs.to(self.device)

    def _step_inputs(self, obs, infos):
        """alg.act's two inputs for the next step, from env.step's (obs, infos)."""
        obs = self.obs_normalizer(obs.to(self.device))
        critic_obs = infos["observations"].get("critic", obs)
        return obs, self.critic_obs_normalizer(critic_obs.to(self.device))

    def _end_collection(self, critic_obs):
        """Between the last env step and alg.update(); counted as learning time."""
        self.alg.compute_returns(critic_obs)

    # ---- API used by train.py / play.py
    def learn(self, num_learning_iterations: int, init_at_random_ep_len: bool = False):
        self._check_ready()
        if init_at_random_ep_len:
            self.env.episode_length_buf = torch.randint_like(self.env.episode_length_buf,
                                                             high=int(self.env.max_episode_length))
        obs, critic_obs = self._first_inputs()
        self.train_mode()
        self._store_git_state()
        ep_infos: list[dict] = []
        rnd = self.alg.rnd is not None  # extrinsic / intrinsic episode sums, collected as the reward's are
        episodes = EpisodeStats(self.env.num_envs, self.device,
                                ("reward", "extrinsic", "intrinsic") if rnd else ("reward",))
        start_iter = self.current_learning_iteration
        tot_iter = start_iter + num_learning_iterations
        for it in range(start_iter, tot_iter):
            start = time.time()
            with torch.inference_mode():
                for _ in range(self.num_steps_per_env):
                    actions = self.alg.act(obs, critic_obs)
                    obs, rewards, dones, infos = self.env.step(actions.to(self.env.device))
                    rewards, dones = rewards.to(self.device), dones.to(self.device)
                    obs, critic_obs = self._step_inputs(obs, infos)
                    self.alg.process_env_step(rewards, dones, infos)
                    if self.log_dir is not None:
                        if "episode" in infos:
                            ep_infos.append(infos["episode"])
                        elif "log" in infos:
                            ep_infos.append(infos["log"])
                        if rnd:  # rsl_rl: the logged reward is extrinsic + intrinsic
                            intrinsic = self.alg.intrinsic_rewards
                            episodes.step(dones, reward=rewards + intrinsic, extrinsic=rewards, intrinsic=intrinsic)
                        else:
                            episodes.step(dones, reward=rewards)
                if self.log_dir is not None:
                    episodes.flush()
                stop = time.time()
                collection_time = stop - start
                start = stop
                self._end_collection(critic_obs)
            loss = self.alg.update()
            stop = time.time()
            learn_time = stop - start
            self.current_learning_iteration = it
            self._log(it, start_iter, tot_iter, collection_time, learn_time, loss, ep_infos, episodes.buffers)
            if self.log_dir is not None and it % self.save_interval == 0:
                self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
            ep_infos.clear()
        self.current_learning_iteration = tot_iter
        if self.log_dir is not None:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))

    def _log(self, it, start_iter, tot_iter, collection_time, learn_time, loss, ep_infos, episodes):
        steps = self.num_steps_per_env * self.env.num_envs * self.shard.world
        self.tot_timesteps += steps
        it_time = collection_time + learn_time
        self.tot_time += it_time
        fps = int(steps / it_time) if it_time > 0 else 0
        scalars = {**self._loss_scalars(loss),
                   "Loss/learning_rate": self.alg.learning_rate,
                   "Policy/mean_noise_std": self.alg.policy.action_std.mean().item()
                   if self.alg.policy.distribution is not None else 0.0,
                   "Perf/total_fps": fps, "Perf/collection_time": collection_time, "Perf/learning_time": learn_time,
                   "Perf/collection_env_steps_per_s": self.env.num_envs * self.shard.world * self.num_steps_per_env
                   / max(collection_time, 1e-9)}
        for key in (ep_infos[0].keys() if ep_infos else []):
            vals = [float(torch.as_tensor(e[key]).float().mean()) for e in ep_infos if key in e]
            if vals:
                scalars[key if "/" in key else "Episode/" + key] = sum(vals) / len(vals)
        if episodes["reward"]:
            scalars["Train/mean_reward"] = statistics.mean(episodes["reward"])
            scalars["Train/mean_episode_length"] = statistics.mean(episodes["length"])
        if self.alg.rnd is not None:
            scalars["Rnd/weight"] = self.alg.rnd.weight
            if episodes["extrinsic"]:
                scalars["Rnd/mean_extrinsic_reward"] = statistics.mean(episodes["extrinsic"])
                scalars["Rnd/mean_intrinsic_reward"] = statistics.mean(episodes["intrinsic"])
        self.last_iteration_stats = scalars
        if self.shard.rank != 0:
            return
        self.logger.write(it, scalars)
        width = 80
        lines = [f"{'#' * width}", f" \033[1m Learning iteration {it}/{tot_iter} \033[0m ".center(width, " "),
                 f"{'Computation:':>35} {fps:.0f} steps/s (collection: {collection_time:.3f}s, learning {learn_time:.3f}s)"]
        for k, v in scalars.items():
            if not k.startswith("Perf/"):
                lines.append(f"{k + ':':>35} {v:.4f}")
        eta = self.tot_time / max(1, it + 1 - start_iter) * (tot_iter - it - 1)
        lines += [f"{'-' * width}", f"{'Total timesteps:':>35} {self.tot_timesteps}",
                  f"{'Iteration time:':>35} {it_time:.2f}s", f"{'Total time:':>35} {self.tot_time:.2f}s",
                  f"{'ETA:':>35} {eta:.1f}s"]
        print("\n".join(lines), flush=True)

    def _loss_scalars(self, loss: dict) -> dict:
        return {"Loss/value_function": loss["value_function"], "Loss/surrogate": loss["surrogate"],
                "Loss/entropy": loss["entropy"], **({"Loss/symmetry": loss["symmetry"]} if "symmetry" in loss else {}),
                **({"Loss/rnd": loss["rnd"]} if "rnd" in loss else {})}

    def save(self, path: str, infos=None):
        if self.shard.rank != 0:
            return
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        d = {"model_state_dict": self.alg.policy.state_dict(), "optimizer_state_dict": self.alg.optimizer_state_dict(),
             "iter": self.current_learning_iteration, "infos": infos}
        if self.empirical_normalization:
            d["obs_norm_state_dict"] = self.obs_normalizer.state_dict()
        d.update(self._checkpoint_extras())
        torch.save(d, path)

    def _checkpoint_extras(self) -> dict:
        """The checkpoint's keys beyond the model, the optimizer and the observation normaliser."""
        d = {}
        if self.empirical_normalization:
            d["critic_obs_norm_state_dict"] = self.critic_obs_normalizer.state_dict()
        if self.alg.rnd is not None:
            d["rnd_state_dict"] = self.alg.rnd.rnd_state_dict()
            d["rnd_optimizer_state_dict"] = self.alg.rnd_optimizer.state_dict()
        return d

    def load(self, path: str, load_optimizer: bool = True):
        d = torch.load(path, map_location=self.device, weights_only=True)
        if self.alg.policy.is_recurrent:  # the critic's memory reads the observation
            w = d["model_state_dict"].get("memory_c.rnn.weight_ih_l0")
            mine = self.alg.policy.memory_c.rnn.input_size
        else:
            w = d["model_state_dict"].get("critic.0.weight")
            mine = self.alg.policy.critic[0].weight.shape[1]
        if w is not None and w.shape[1] != mine:
            raise ValueError(f"{path}: the checkpoint's critic reads {w.shape[1]}-wide observations, this env's "
                             f"critic observation is {mine} wide -- the two were built with different "
                             "--privileged_critic settings (env.observations.critic)")
        if self.alg.rnd is not None and "rnd_state_dict" not in d:
            raise ValueError(f"{path}: the checkpoint holds no rnd_state_dict, this run trains with rnd_cfg -- resume it "
                             "without rnd_cfg, or start the RND run afresh")
        self.alg.policy.load_state_dict(d["model_state_dict"])
        if self.alg.rnd is not None:
            self.alg.rnd.load_rnd_state_dict(d["rnd_state_dict"])
            if load_optimizer and "rnd_optimizer_state_dict" in d:
                self.alg.rnd_optimizer.load_state_dict(d["rnd_optimizer_state_dict"])
            self.alg._graph = None  # the captured graph holds the old optimizer state tensors
            if self.alg.rnd_fused is not None:
                self.alg.rnd_fused.dirty = True
        if self.empirical_normalization and "obs_norm_state_dict" in d:
            self.obs_normalizer.load_state_dict(d["obs_norm_state_dict"])
            self.critic_obs_normalizer.load_state_dict(d["critic_obs_norm_state_dict"])
        if load_optimizer and "optimizer_state_dict" in d:
            self.alg.load_optimizer_state_dict(d["optimizer_state_dict"])
        self.current_learning_iteration = int(d.get("iter", 0))
        self.alg.broadcast_parameters()
        return d.get("infos")

    def get_inference_policy(self, device=None, fused: bool = False):
        """The deterministic policy obs -> action mean (DistillationRunner: the student's, from the student
        observation).  ``fused=True``: one h12learn_mlp_forward launch (normaliser +
        actor, h12env.policy.FusedMLP) packed from the parameters as they are now; the default is the torch path.

        A recurrent policy's is stateful: it starts from an empty memory, and the caller resets the rows of finished
        episodes (``policy.reset(dones)``: the returned callable's own ``reset`` with ``fused``, the policy module's
        otherwise).  ``fused=True``: h12env.policy.RecurrentPolicy on h12learn_lstm_step."""
        self.eval_mode()
        p = self.alg.policy
        memory, net = (getattr(p, name, None) for name in self._inference_modules)
        norm = self.obs_normalizer if self.empirical_normalization else None
        if device is not None:
            p.to(device)
            if norm is not None:
                norm.to(device)
        if p.is_recurrent:
            if fused:
                from .policy import RecurrentPolicy

                return RecurrentPolicy(memory.rnn, net, norm, fused=True)
            p.reset()
        elif fused:
            from .policy import FusedMLP

            f = FusedMLP([net], norm)
            return lambda x: f(x)[0]
        if norm is not None:
            return lambda x: p.act_inference(norm(x))
        return p.act_inference

    def _mode_modules(self) -> list:
        """What train_mode() / eval_mode() switch."""
        return [self.alg.policy, self.obs_normalizer, self.critic_obs_normalizer,
                *([] if self.alg.rnd is None else [self.alg.rnd])]

    def train_mode(self):
        for m in self._mode_modules():
            m.train()

    def eval_mode(self):
        for m in self._mode_modules():
            m.eval()

    def add_git_repo_to_log(self, repo_file_path):
        self.git_status_repos.append(repo_file_path)

    def _store_git_state(self):
        if self.log_dir is None or self.shard.rank != 0:
            return
        for p in self.git_status_repos:
            self._store_git_diff(p)
        self.git_status_repos = []

    def _store_git_diff(self, repo_file_path):
        try:
            d = os.path.dirname(os.path.abspath(repo_file_path))
            diff = subprocess.run(["git", "-C", d, "diff", "HEAD"], capture_output=True, text=True, timeout=10).stdout
            os.makedirs(self.log_dir, exist_ok=True)
            with open(os.path.join(self.log_dir, "git.diff"), "a") as f:
                f.write(f"--- {repo_file_path}\n{diff}\n")
        except Exception:  # not a git checkout: nothing to record
            pass


def _shard_from_env() -> D.Shard:
    if dist.is_available() and dist.is_initialized():
        return D.Shard(dist.get_rank(), dist.get_world_size(), int(os.environ.get("LOCAL_RANK", "0")), 0)
    return D.Shard(0, 1, 0, 0)
