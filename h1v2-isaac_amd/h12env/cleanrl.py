"""CleanRL-style PPO of the Constraints-as-Terminations tasks (biped_tasks/utils/cleanrl/ppo.py restated on
this stack): ``RunningMeanStd``, ``Agent`` and ``PPO(envs, ppo_cfg, run_path)``.

What differs from h12env.ppo (rsl_rl's PPO): GAE over *soft* terminations (the env's termination probabilities are
the dones, and (1 - done)(1 - true_done) multiplies the bootstrap term and the running advantage), a running
mean/variance normaliser over every observation that updates on every step, a second one over values and returns,
RAdam with a linearly annealed learning rate and no KL schedule, advantage normalisation per minibatch, vf_coef 2.

Module, parameter and buffer names, and therefore the ``state_dict`` keys and shapes, are the reference's
(critic.{0,2,4,6}.*, actor_mean.{0,2,4,6}.*, actor_logstd, obs_rms.{running_mean,running_var,count}, value_rms.*):
a checkpoint of either side loads on the other.

Device path: on CUDA tensors ``RunningMeanStd.forward`` is one call of h12learn_rms_forward (statistics update
fused with the normalisation, buffers updated in place, bitwise reproducible) and the GAE is h12learn_gae_soft
(bit-identical to the fp32 torch loop); ``H12_CLEANRL_FUSED=0`` selects the torch restatement of both, which is
also what runs on CPU and wherever autograd has to see through the normaliser (the value loss).

Deviations from the reference, all deliberate:
  * logging goes to <run_path>/metrics.jsonl (h12env.ppo._Logger): tensorboard and wandb are not part of this
    stack; ``logger="wandb"`` raises;
  * no ``exit(0)`` on ``info["time_outs"]`` (ppo.py:226-229 is a debug stop; this env always reports time_outs);
  * no host synchronisation per minibatch or per step: clipfracs and the loss sums stay on the device until the
    iteration ends, and on CUDA ``Normal`` is built without its argument check (a device-to-host read);
  * graphed collection: on CUDA the per-step agent work (normaliser launches, actor and critic forward,
    mean + std * randn, log-probability) replays as one HIP graph; the generator state is restored after the
    warm-up, so graphed and eager collection draw the same noise.  ``H12_PPO_GRAPH=0`` selects eager, and so does
    ``H12_CLEANRL_FUSED=0``: the graph is built on the HIP normaliser only (replaying the torch restatement of
    it at 4096 envs turned finite observations non-finite on the MI355X, which eager it never does).  On CUDA the
    sample is ``mean + std * randn_like(mean)`` in both modes; on CPU it is ``Normal(mean, std).sample()`` and one
    ``torch.randperm(BATCH)`` per epoch, the reference's calls in the reference's order;
  * the update stays eager, unless ``fused_loss`` is on (``PPO(..., fused_loss=True)``, ``H12_CLEANRL_HEAD_FUSED=1``,
    ``train_cleanrl.py --fused_loss``): everything from ``logratio`` to ``loss`` is then one
    ``CleanRLHead`` node (h12learn_cleanrl_head on CUDA, the same torch expressions on CPU), the optimiser is the
    capturable RAdam with the learning rate as a device scalar, and on CUDA a whole minibatch (gather, forwards, head,
    backward, gradient clip, RAdam step) replays as one HIP graph per minibatch size; ``H12_PPO_GRAPH=0`` runs the
    same minibatch eagerly, bit for bit;
  * with ``fused_optimizer`` (``PPO(..., fused_optimizer=True)``, ``H12_OPTIMIZER_FUSED=1``, ``train_cleanrl.py
    --fused_optimizer``) the gradient clip and the RAdam step of either update path are
    ``h12env.optim.FusedClipRAdam``: two HIP launches on CUDA, ``clip_grad_norm_`` and torch's own rule on CPU;
  * the storage, the agent and the rollout live on the env's device (the reference picks cuda when available);
  * the running statistics are updated in place (the reference rebinds the buffers), so a graph can hold them;
  * ``PPO`` returns the trained agent (the reference returns None) and takes ``resume_path`` / ``on_step``.
Single GPU only, as in the reference.
"""
from __future__ import annotations

import dataclasses
import os
import time
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim
from torch.distributions.normal import Normal

from .graphs import TrainingState, capture, graph_enabled
from .policy import FusedActorCritic, fused_collection_on


# ---------------------------------------------------------------------------------------------- cfg
class _Missing:
    """dataclasses.MISSING of the reference cfg: a field the task's agent cfg has to set."""

    def __repr__(self):
        return "MISSING"


MISSING = _Missing()


@dataclass
class CleanRlPpoActorCriticCfg:
    """biped_tasks/utils/cleanrl/rl_cfg.py."""
    seed: int = 42
    save_interval: int = MISSING
    learning_rate: float = MISSING
    num_steps: int = MISSING
    num_iterations: int = MISSING
    gamma: float = MISSING
    gae_lambda: float = MISSING
    updates_epochs: int = MISSING
    minibatch_size: int = MISSING
    clip_coef: float = MISSING
    ent_coef: float = MISSING
    vf_coef: float = MISSING
    max_grad_norm: float = MISSING
    norm_adv: bool = MISSING
    clip_vloss: bool = MISSING
    anneal_lr: bool = MISSING
    experiment_name: str = MISSING
    logger: str = "tensorboard"
    wandb_project: str = MISSING
    load_run: str = MISSING
    load_checkpoint: str = MISSING

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


# ---------------------------------------------------------------------------------------------- normaliser
def fused_enabled() -> bool:
    return os.environ.get("H12_CLEANRL_FUSED", "1") != "0"


def update_mean_var_count_from_moments(mean, var, count, batch_mean, batch_var, batch_count):
    delta = batch_mean - mean
    tot_count = count + batch_count
    new_mean = mean + delta * batch_count / tot_count
    m_a = var * count
    m_b = batch_var * batch_count
    M2 = m_a + m_b + torch.square(delta) * count * batch_count / tot_count
    new_var = M2 / tot_count
    return new_mean, new_var, tot_count


class RunningMeanStd(nn.Module):
    def __init__(self, shape=(), epsilon=1e-08):
        super().__init__()
        self.register_buffer("running_mean", torch.zeros(shape))
        self.register_buffer("running_var", torch.ones(shape))
        self.register_buffer("count", torch.ones(()))
        self.epsilon = epsilon
        self._ws = {}  # (device, n) -> workspace of the fused kernel (not module state)

    def _fused_ok(self, obs) -> bool:
        return (obs.is_cuda and obs.dtype == torch.float32 and self.running_mean.dtype == torch.float32
                and self.running_mean.is_cuda and fused_enabled() and obs.dim() >= 1 and obs.shape[0] >= 1
                and obs.shape[1:].numel() == self.running_mean.numel()
                and not (torch.is_grad_enabled() and obs.requires_grad) and not torch.jit.is_tracing())

    def forward(self, obs, update=True):
        if self._fused_ok(obs):
            return self._forward_fused(obs, update)
        if update:
            self.update(obs)
        return (obs - self.running_mean) / torch.sqrt(self.running_var + self.epsilon)

    def _forward_fused(self, obs, update):
        from . import _learn

        x = obs.detach().contiguous()
        ws = None
        if update:
            key = (x.device, x.shape[0])
            ws = self._ws.get(key)
            if ws is None:
                ws = self._ws[key] = _learn.rms_workspace(x.shape[0], self.running_mean.numel(), x.device)
        return _learn.rms_forward(x, self.running_mean, self.running_var, self.count, self.epsilon, bool(update), ws)

    def update(self, x):
        """Updates the mean, var and count from a batch of samples."""
        batch_mean = torch.mean(x, dim=0)
        batch_var = torch.var(x, correction=0, dim=0)
        self.update_from_moments(batch_mean, batch_var, x.shape[0])

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        m, v, c = update_mean_var_count_from_moments(self.running_mean, self.running_var, self.count, batch_mean,
                                                     batch_var, batch_count)
        with torch.no_grad():
            self.running_mean.copy_(m)
            self.running_var.copy_(v)
            self.count.copy_(c)


# ---------------------------------------------------------------------------------------------- agent
def layer_init(layer, std=np.sqrt(2), bias_const=0.0):
    torch.nn.init.orthogonal_(layer.weight, std)
    torch.nn.init.constant_(layer.bias, bias_const)
    return layer


class Agent(nn.Module):
    def __init__(self, envs):
        super().__init__()
        obs_shape = tuple(envs.unwrapped.single_observation_space["policy"].shape)
        act_shape = tuple(envs.unwrapped.single_action_space.shape)
        n_obs, n_act = int(np.prod(obs_shape)), int(np.prod(act_shape))
        self.critic = nn.Sequential(
            layer_init(nn.Linear(n_obs, 512)), nn.ELU(),
            layer_init(nn.Linear(512, 256)), nn.ELU(),
            layer_init(nn.Linear(256, 128)), nn.ELU(),
            layer_init(nn.Linear(128, 1), std=1.0),
        )
        self.actor_mean = nn.Sequential(
            layer_init(nn.Linear(n_obs, 512)), nn.ELU(),
            layer_init(nn.Linear(512, 256)), nn.ELU(),
            layer_init(nn.Linear(256, 128)), nn.ELU(),
            layer_init(nn.Linear(128, n_act), std=0.01),
        )
        self.actor_logstd = nn.Parameter(torch.zeros(1, n_act))
        self.obs_rms = RunningMeanStd(shape=obs_shape)
        self.value_rms = RunningMeanStd(shape=())

    def get_value(self, x):
        return self.critic(x)

    def get_action_and_value(self, x, action=None, deterministic=False):
        action_mean = self.actor_mean(x)
        action_logstd = self.actor_logstd.expand_as(action_mean)
        action_std = torch.exp(action_logstd)
        # the argument check of Normal is a host synchronisation (and cannot be captured): CPU only
        probs = Normal(action_mean, action_std, validate_args=None if not action_mean.is_cuda else False)
        if action is None:
            if deterministic:
                action = action_mean
            elif action_mean.is_cuda:  # the same Normal(mean, std) sample from randn: capturable into a graph
                action = action_mean + action_std * torch.randn_like(action_mean)
            else:
                action = probs.sample()
        return action, probs.log_prob(action).sum(1), probs.entropy().sum(1), self.critic(x)

    def forward(self, x, deterministic: bool = True):
        action, _, _, _ = self.get_action_and_value(self.obs_rms(x, update=False), deterministic=deterministic)
        return action

    def inference_policy(self, fused: bool = False):
        """The deterministic policy raw obs -> action mean (obs_rms read, not updated).  ``fused=True``: one
        h12learn_mlp_forward launch (normaliser + actor_mean, h12env.policy.FusedMLP) packed from the parameters as
        they are now; the default is the torch path."""
        if fused:
            from .policy import FusedMLP

            f = FusedMLP([self.actor_mean], self.obs_rms)
            return lambda x: f(x)[0]

        def policy(x):
            with torch.no_grad():
                return self.actor_mean(self.obs_rms(x, update=False))

        return policy


# ---------------------------------------------------------------------------------------------- GAE
def gae_soft_torch(rewards, values, dones, true_dones, next_value, next_done, next_true_done, gamma, gae_lambda):
    """ppo.py:250-267, operation for operation."""
    num_steps = rewards.shape[0]
    next_value = next_value.reshape(1, -1)
    advantages = torch.zeros_like(rewards)
    lastgaelam = 0
    for t in reversed(range(num_steps)):
        if t == num_steps - 1:
            nextnonterminal = 1.0 - next_done
            true_nextnonterminal = 1 - next_true_done
            nextvalues = next_value
        else:
            nextnonterminal = 1.0 - dones[t + 1]
            true_nextnonterminal = 1 - true_dones[t + 1]
            nextvalues = values[t + 1]
        delta = rewards[t] + gamma * nextvalues * nextnonterminal * true_nextnonterminal - values[t]
        advantages[t] = lastgaelam = delta + gamma * gae_lambda * nextnonterminal * true_nextnonterminal * lastgaelam
    return advantages, advantages + values


def gae_soft(rewards, values, dones, true_dones, next_value, next_done, next_true_done, gamma, gae_lambda):
    if rewards.is_cuda and fused_enabled():
        from . import _learn

        return _learn.gae_soft(rewards, values, dones, true_dones, next_value.reshape(-1).contiguous(),
                               next_done.contiguous(), next_true_done.contiguous(), gamma, gae_lambda)
    return gae_soft_torch(rewards, values, dones, true_dones, next_value, next_done, next_true_done, gamma, gae_lambda)


# ---------------------------------------------------------------------------------------------- collection
class _Collector:
    """The per-step agent work: ``normalise`` (obs_rms with update), ``act`` (actor + critic forward, sample,
    log-probability) and the two in one, ``normalise_act``.  Graphed, ``act`` and ``normalise_act`` each replay
    one captured HIP graph on static buffers; the returned tensors are the graph's outputs and are overwritten by
    the next replay, so the caller copies them into its storage first."""

    def __init__(self, agent: Agent, graphed: bool):
        self.agent = agent
        self.graphed = graphed
        self._graphs: dict = {}
        self._fused = FusedActorCritic(agent.actor_mean, agent.critic)

    def normalise(self, raw):
        with torch.no_grad():
            return self.agent.obs_rms(raw)

    def _act_body(self, obs):
        if fused_collection_on(obs):
            return self._act_body_fused(obs)
        action, logprob, _, value = self.agent.get_action_and_value(obs)
        return action, logprob, value.flatten()

    def _act_body_fused(self, obs):
        """H12_POLICY_FUSED=1: actor mean and critic value from policy.FusedActorCritic (one two-network launch); the
        sample and the log-probability are get_action_and_value's."""
        mean, value = self._fused(obs)
        std = torch.exp(self.agent.actor_logstd.expand_as(mean))
        action = mean + std * torch.randn_like(mean)
        return action, Normal(mean, std, validate_args=False).log_prob(action).sum(1), value.flatten()

    def act(self, obs):
        if self.graphed:
            return self._replay("act", obs)[1:]
        with torch.no_grad():
            return self._act_body(obs)

    def normalise_act(self, raw):
        if self.graphed:
            return self._replay("normalise_act", raw)
        with torch.no_grad():
            obs = self.agent.obs_rms(raw)
            return (obs, *self._act_body(obs))

    def _body(self, kind, x):
        obs = self.agent.obs_rms(x) if kind == "normalise_act" else x
        return (obs, *self._act_body(obs))

    def _replay(self, kind, x):
        key = (kind, tuple(x.shape))
        ent = self._graphs.get(key)
        if ent is None:
            ent = self._graphs[key] = self._capture(kind, x)
        g, inp, out = ent
        inp.copy_(x)
        g.replay()
        return out

    def _capture(self, kind, x):
        rms = self.agent.obs_rms
        # the warm-up consumes noise draws and (normalise_act) updates the statistics: both are put back, so the
        # replays continue exactly where eager collection would
        with torch.no_grad():
            inp = x.detach().clone()
            g, out = capture(lambda: self._body(kind, inp), x.device,
                             undo=(rms.running_mean, rms.running_var, rms.count), rng=True)
        return g, inp, out


def _graph_enabled(device) -> bool:
    # the graph is built on the HIP normaliser; the torch restatement (H12_CLEANRL_FUSED=0) collects eagerly
    return device.type == "cuda" and graph_enabled() and fused_enabled()


def _episode_scalars(ep_infos, device) -> dict:
    """Mean over the iteration's info dicts per key (ppo.py:231-247), one host transfer for all keys."""
    if not ep_infos:
        return {}
    names, vals = [], []
    for key in ep_infos[0]:
        parts = [torch.as_tensor(e[key], dtype=torch.float32, device=device).reshape(-1) for e in ep_infos if key in e]
        if parts:
            names.append(key if "/" in key else "Episode/" + key)
            vals.append(torch.cat(parts).mean())
    return dict(zip(names, torch.stack(vals).tolist())) if vals else {}


# ---------------------------------------------------------------------------------------------- fused update
class _FusedUpdate:
    """The minibatch of ``PPO(fused_loss=True)``: gather the observations, actor and critic forward, ``CleanRLHead``,
    backward, gradient clip, optimiser step.  On CUDA the loss statistics accumulate on the device in ``stats``
    (pg, entropy, v, total, clip fraction) and, graphed, each minibatch size replays a graph of its own, captured at its
    first use (graphs.capture: the warm-up's changes to parameters, optimiser state and statistics are put back bit for
    bit).  On CPU the node evaluates the default path's expressions."""

    def __init__(self, agent, optimizer, cfg, batch_size: int, device, graphed: bool, clip: bool = True):
        self.agent, self.optimizer, self.cfg, self.device = agent, optimizer, cfg, device
        self.clip = clip  # False: the optimiser clips inside its step (optim.FusedClipRAdam)
        self.cuda = device.type == "cuda"
        self.graphed = graphed and self.cuda
        self._graphs: dict = {}  # minibatch size -> (graph, static index buffer)
        self.stats = torch.zeros(5, device=device)
        self.n_minibatches = 0
        self.clipfracs: list = []  # CPU: the default path's list
        # static copies of what an iteration computes anew (advantages, normalised values and returns)
        self.adv, self.values_n, self.returns_n = (torch.zeros(batch_size, device=device) for _ in range(3))
        self.obs = self.logprobs = self.actions = None

    def begin(self, b_obs, b_logprobs, b_actions, b_advantages, b_values, b_returns):
        """An iteration's rollout: the storage's flattened tensors (static) and the three computed after collection."""
        self.obs, self.logprobs, self.actions = b_obs, b_logprobs, b_actions
        self.adv.copy_(b_advantages)
        self.values_n.copy_(b_values)
        self.returns_n.copy_(b_returns)
        self.stats.zero_()
        self.n_minibatches = 0
        self.clipfracs = []

    def _minibatch(self, idx):
        from .ppo_head import CleanRLHead, CleanRLInputs

        agent, c = self.agent, self.cfg
        x = self.obs[idx]
        h = CleanRLInputs(idx=idx, old_log_prob=self.logprobs, advantages=self.adv, returns_n=self.returns_n,
                          values_n=self.values_n, actions=self.actions, value_rms=agent.value_rms,
                          clip_coef=c.clip_coef, ent_coef=c.ent_coef, vf_coef=c.vf_coef, norm_adv=c.norm_adv,
                          clip_vloss=c.clip_vloss, stats_accum=self.stats if self.cuda else None)
        loss, out = CleanRLHead.apply(agent.actor_mean(x), agent.critic(x), agent.actor_logstd, h)
        self.optimizer.zero_grad()
        loss.backward()
        if self.clip:
            nn.utils.clip_grad_norm_(agent.parameters(), c.max_grad_norm)
        self.optimizer.step()
        return out

    def step(self, mb_inds):
        self.n_minibatches += 1
        if self.graphed:
            ent = self._graphs.get(mb_inds.shape[0])
            if ent is None:
                ent = self._graphs[mb_inds.shape[0]] = self._capture(mb_inds.shape[0])
            g, idx = ent
            idx.copy_(mb_inds)
            g.replay()
            return
        out = self._minibatch(mb_inds)
        if not self.cuda:
            self.stats[:4] += out[:4]
            self.clipfracs.append(out[4])

    def _capture(self, mb: int):
        idx = torch.arange(mb, dtype=torch.long, device=self.device)
        state = TrainingState(self.agent.parameters(), self.optimizer, [self.stats])
        g, _ = capture(lambda: self._minibatch(idx), self.device, undo=[state],
                       before_capture=lambda: self.optimizer.zero_grad(set_to_none=True))
        return g, idx

    def means(self, num_updates: float):
        """(pg, entropy, v, total, clip fraction) of the iteration, on the device."""
        if self.cuda:
            return torch.cat([self.stats[:4] / num_updates, self.stats[4:] / max(self.n_minibatches, 1)])
        return torch.cat([self.stats[:4] / num_updates, torch.stack(self.clipfracs).mean().reshape(1)])


# ---------------------------------------------------------------------------------------------- PPO
def PPO(envs, ppo_cfg, run_path, resume_path: str | None = None, on_step=None, fused_loss: bool | None = None,
        fused_optimizer: bool | None = None):
    """biped_tasks/utils/cleanrl/ppo.py:121-369 (the module docstring lists the deviations).  ``on_step(step_index,
    obs, action, logprob, value)`` is a read-only observer of each stored transition (tests, probes).  ``fused_loss``
    (None: ``H12_CLEANRL_HEAD_FUSED=1``) selects the fused loss head and, on CUDA, the captured update;
    ``fused_optimizer`` (None: ``H12_OPTIMIZER_FUSED=1``) selects optim.FusedClipRAdam, clip included, on both."""
    from .optim import FusedClipRAdam, fused_optimizer_enabled
    from .ppo import _Logger
    from .ppo_head import cleanrl_fused_loss_enabled

    fused_loss = cleanrl_fused_loss_enabled() if fused_loss is None else bool(fused_loss)
    fused_optimizer = fused_optimizer_enabled() if fused_optimizer is None else bool(fused_optimizer)

    if ppo_cfg.logger == "wandb":
        raise RuntimeError("logger='wandb' is not available on this stack (no wandb package); use 'tensorboard', "
                           "which logs to <run>/metrics.jsonl")
    if ppo_cfg.logger != "tensorboard":
        raise AssertionError("logger type not found")
    os.makedirs(run_path, exist_ok=True)
    writer = _Logger(run_path, 0)

    LEARNING_RATE = ppo_cfg.learning_rate
    NUM_STEPS = ppo_cfg.num_steps
    NUM_ITERATIONS = ppo_cfg.num_iterations
    GAMMA = ppo_cfg.gamma
    GAE_LAMBDA = ppo_cfg.gae_lambda
    UPDATES_EPOCHS = ppo_cfg.updates_epochs
    MINIBATCH_SIZE = ppo_cfg.minibatch_size
    CLIP_COEF = ppo_cfg.clip_coef
    ENT_COEF = ppo_cfg.ent_coef
    VF_COEF = ppo_cfg.vf_coef
    MAX_GRAD_NORM = ppo_cfg.max_grad_norm
    NORM_ADV = ppo_cfg.norm_adv
    CLIP_VLOSS = ppo_cfg.clip_vloss
    ANNEAL_LR = ppo_cfg.anneal_lr

    NUM_ENVS = envs.unwrapped.num_envs
    obs_shape = tuple(envs.unwrapped.single_observation_space["policy"].shape)
    act_shape = tuple(envs.unwrapped.single_action_space.shape)
    device = torch.device(envs.unwrapped.device)
    BATCH_SIZE = int(NUM_ENVS * NUM_STEPS)

    agent = Agent(envs).to(device)
    if resume_path is not None:
        agent.load_state_dict(torch.load(resume_path, map_location=device, weights_only=True))
    lr_t = updater = None
    if fused_loss:
        if device.type == "cuda":
            from . import _learn

            if int(np.prod(act_shape)) > _learn.ppo_head_max_actions():
                raise ValueError(f"fused_loss: {int(np.prod(act_shape))} actions, the loss head takes at most "
                                 f"{_learn.ppo_head_max_actions()}")
            # the learning rate as a device scalar: the annealing rewrites it under a captured step
            lr_t = torch.tensor(LEARNING_RATE, dtype=torch.float32, device=device)
            if fused_optimizer:  # in place of the capturable RAdam inside the graph
                optimizer = FusedClipRAdam(agent.parameters(), lr=lr_t, eps=1e-5, max_norm=MAX_GRAD_NORM)
            else:
                optimizer = optim.RAdam(agent.parameters(), lr=lr_t, eps=1e-5, capturable=True)
        elif fused_optimizer:
            optimizer = FusedClipRAdam(agent.parameters(), lr=LEARNING_RATE, eps=1e-5, max_norm=MAX_GRAD_NORM)
        else:
            optimizer = optim.RAdam(agent.parameters(), lr=LEARNING_RATE, eps=1e-5)
        updater = _FusedUpdate(agent, optimizer, ppo_cfg, BATCH_SIZE, device, _graph_enabled(device),
                               clip=not fused_optimizer)
    elif fused_optimizer:
        optimizer = FusedClipRAdam(agent.parameters(), lr=LEARNING_RATE, eps=1e-5, max_norm=MAX_GRAD_NORM)
    else:
        optimizer = optim.RAdam(agent.parameters(), lr=LEARNING_RATE, eps=1e-5)
    lr_host = LEARNING_RATE
    collector = _Collector(agent, _graph_enabled(device))

    obs = torch.zeros((NUM_STEPS, NUM_ENVS, *obs_shape), dtype=torch.float, device=device)
    actions = torch.zeros((NUM_STEPS, NUM_ENVS, *act_shape), dtype=torch.float, device=device)
    logprobs = torch.zeros((NUM_STEPS, NUM_ENVS), dtype=torch.float, device=device)
    rewards = torch.zeros((NUM_STEPS, NUM_ENVS), dtype=torch.float, device=device)
    dones = torch.zeros((NUM_STEPS, NUM_ENVS), dtype=torch.float, device=device)
    true_dones = torch.zeros((NUM_STEPS, NUM_ENVS), dtype=torch.float, device=device)
    values = torch.zeros((NUM_STEPS, NUM_ENVS), dtype=torch.float, device=device)

    global_step = 0
    next_obs = collector.normalise(envs.reset()[0]["policy"])
    next_done = torch.zeros(NUM_ENVS, dtype=torch.float, device=device)
    next_true_done = torch.zeros(NUM_ENVS, dtype=torch.float, device=device)

    print(f"Starting training for {NUM_ITERATIONS} steps")
    for iteration in range(1, NUM_ITERATIONS + 1):
        t_start = time.time()
        ep_infos = []
        if ANNEAL_LR:
            frac = 1.0 - (iteration - 1.0) / NUM_ITERATIONS
            if lr_t is not None:
                lr_host = frac * LEARNING_RATE
                lr_t.fill_(lr_host)
            else:
                optimizer.param_groups[0]["lr"] = frac * LEARNING_RATE

        # the first action of an iteration comes from the freshly updated weights; within the iteration the
        # normalisation of the new observation and the next action are one piece of work (one graph replay)
        action, logprob, value = collector.act(next_obs)
        for step in range(NUM_STEPS):
            global_step += NUM_ENVS
            obs[step] = next_obs
            dones[step] = next_done
            true_dones[step] = next_true_done
            values[step] = value
            actions[step] = action
            logprobs[step] = logprob
            if on_step is not None:
                on_step(global_step // NUM_ENVS - 1, obs[step], actions[step], logprobs[step], values[step])

            raw_obs, rewards[step], next_done, timeouts, info = envs.step(action)
            next_done = next_done.to(torch.float)
            if "episode" in info:
                ep_infos.append(info["episode"])
            elif "log" in info:
                ep_infos.append(info["log"])
            next_true_done = timeouts.float()
            if step + 1 < NUM_STEPS:
                next_obs, action, logprob, value = collector.normalise_act(raw_obs["policy"])
            else:
                next_obs = collector.normalise(raw_obs["policy"])
        scalars = _episode_scalars(ep_infos, device)
        t_collect = time.time()

        # bootstrap value if not done; soft GAE
        with torch.no_grad():
            next_value = agent.get_value(next_obs).reshape(-1)
            advantages, returns = gae_soft(rewards, values, dones, true_dones, next_value, next_done, next_true_done,
                                           GAMMA, GAE_LAMBDA)
            b_obs = obs.reshape((-1, *obs_shape))
            b_logprobs = logprobs.reshape(-1)
            b_actions = actions.reshape((-1, *act_shape))
            b_advantages = advantages.reshape(-1)
            b_values = agent.value_rms(values.reshape(-1))
            b_returns = agent.value_rms(returns.reshape(-1))

        sums = torch.zeros(4, device=device)  # pg, entropy, v, surrogate
        clipfracs = []
        if updater is not None:
            updater.begin(b_obs, b_logprobs, b_actions, b_advantages, b_values, b_returns)
        for _epoch in range(UPDATES_EPOCHS):
            b_inds = torch.randperm(BATCH_SIZE, device=device)
            for start in range(0, BATCH_SIZE, MINIBATCH_SIZE):
                mb_inds = b_inds[start:start + MINIBATCH_SIZE]
                if updater is not None:
                    updater.step(mb_inds)
                    continue
                _, newlogprob, entropy, newvalue = agent.get_action_and_value(b_obs[mb_inds], b_actions[mb_inds])
                logratio = newlogprob - b_logprobs[mb_inds]
                ratio = logratio.exp()
                with torch.no_grad():
                    clipfracs.append(((ratio - 1.0).abs() > CLIP_COEF).float().mean())

                mb_advantages = b_advantages[mb_inds]
                if NORM_ADV:
                    mb_advantages = (mb_advantages - mb_advantages.mean()) / (mb_advantages.std() + 1e-8)

                pg_loss1 = -mb_advantages * ratio
                pg_loss2 = -mb_advantages * torch.clamp(ratio, 1 - CLIP_COEF, 1 + CLIP_COEF)
                pg_loss = torch.max(pg_loss1, pg_loss2).mean()

                newvalue = agent.value_rms(newvalue.view(-1), update=False)
                if CLIP_VLOSS:
                    v_loss_unclipped = (newvalue - b_returns[mb_inds]) ** 2
                    v_clipped = b_values[mb_inds] + torch.clamp(newvalue - b_values[mb_inds], -CLIP_COEF, CLIP_COEF)
                    v_loss_clipped = (v_clipped - b_returns[mb_inds]) ** 2
                    v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
                else:
                    v_loss = 0.5 * ((newvalue - b_returns[mb_inds]) ** 2).mean()

                entropy_loss = entropy.mean()
                loss = pg_loss - ENT_COEF * entropy_loss + v_loss * VF_COEF
                sums += torch.stack([pg_loss.detach(), entropy_loss.detach(), v_loss.detach(), loss.detach()])

                optimizer.zero_grad()
                loss.backward()
                if not fused_optimizer:
                    nn.utils.clip_grad_norm_(agent.parameters(), MAX_GRAD_NORM)
                optimizer.step()

        num_updates = UPDATES_EPOCHS * BATCH_SIZE / MINIBATCH_SIZE
        if updater is not None:
            pg, ent, vl, sur, cf = updater.means(num_updates).tolist()
        else:
            pg, ent, vl, sur, cf = torch.cat([sums / num_updates, torch.stack(clipfracs).mean().reshape(1)]).tolist()
        t_end = time.time()
        scalars.update({"Loss/mean_pg_loss": pg, "Loss/mean_entropy_loss": ent, "Loss/mean_v_loss": vl,
                        "Loss/mean_surrogate_loss": sur,
                        "Loss/learning_rate": lr_host if lr_t is not None else optimizer.param_groups[0]["lr"],
                        "Loss/clipfrac": cf, "Perf/collection_time": t_collect - t_start,
                        "Perf/learning_time": t_end - t_collect,
                        "Perf/total_fps": BATCH_SIZE / max(t_end - t_start, 1e-9)})
        writer.write(iteration, scalars)
        print(f"iteration {iteration}/{NUM_ITERATIONS}: pg {pg:.5f} v {vl:.5f} entropy {ent:.4f} "
              f"lr {scalars['Loss/learning_rate']:.3e} ({scalars['Perf/total_fps']:.0f} steps/s)", flush=True)

        if (iteration + 1) % ppo_cfg.save_interval == 0:
            torch.save(agent.state_dict(), f"{run_path}/model_{iteration}.pt")
            print("Saved model")
    writer.close()
    return agent
