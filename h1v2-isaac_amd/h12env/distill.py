"""Teacher-student distillation for the PPO runner (rsl_rl 2.3 modules/student_teacher*.py, algorithms/distillation.py,
restated -- the package is not importable offline).

A teacher that was trained with PPO on everything the simulator knows (the Rough task's 235-wide row: base linear
velocity, height scan) labels the states a student visits; the student reads the deployable observation group
(h12env.student: what the robot measures, with noise) and regresses on the teacher's action (DAgger: the env executes
the student's own sampled action).  ``StudentTeacher`` / ``StudentTeacherRecurrent`` hold both networks,
``Distillation`` is the algorithm, ``DistillationRunner`` is what ``OnPolicyRunner(env, cfg)`` builds when the cfg's
algorithm is ``Distillation``.

The update is rsl_rl's truncated BPTT: over epochs x T steps in time order the per-step behaviour losses are summed, and
every ``gradient_length`` steps (counted across the epochs of one update) the sum is backpropagated, the optimizer
steps and the student's memory is detached; a trailing remainder is evaluated but never backpropagated.  Here a chunk of
``gradient_length`` steps is one call, not a Python loop over steps: ``recurrent.lstm_sequence_state`` over [L, N] for a
recurrent student (the h12learn_lstm_seq_* kernels with ``fused_rnn_update``), the MLP over L * N rows for a plain one;
a chunk that spans an epoch boundary is two such calls, since every epoch restarts from the carried state.
"""
from __future__ import annotations

import os
import warnings

import torch
import torch.nn as nn
from torch.distributions import Normal

from . import distributed as D
from .policy import fused_collection_on
from .ppo import OnPolicyRunner, _DeviceLrAdam, mlp
from .recurrent import Memory, lstm_sequence_state, state_tensors

POLICY_CLASSES = ("StudentTeacher", "StudentTeacherRecurrent")
DEFAULT_OBS_GROUPS = {"student": "student", "teacher": "policy"}


# ---------------------------------------------------------------------------------------------- policies
class StudentTeacher(nn.Module):
    """rsl_rl's StudentTeacher: ``student`` (trained) and ``teacher`` (loaded from a PPO checkpoint's actor, kept in
    eval mode, never differentiated), and the student's state-independent exploration std."""

    is_recurrent = False

    def __init__(self, num_student_obs: int, num_teacher_obs: int, num_actions: int,
                 student_hidden_dims=(256, 256, 256), teacher_hidden_dims=(256, 256, 256), activation="elu",
                 init_noise_std=0.1, noise_std_type="scalar", **kwargs):
        super().__init__()
        self.loaded_teacher = False
        self.student = mlp(num_student_obs, list(student_hidden_dims), num_actions, activation)
        self.teacher = mlp(num_teacher_obs, list(teacher_hidden_dims), num_actions, activation)
        self.teacher.eval()
        self.noise_std_type = noise_std_type
        if noise_std_type == "scalar":
            self.std = nn.Parameter(init_noise_std * torch.ones(num_actions))
        elif noise_std_type == "log":
            self.log_std = nn.Parameter(torch.log(init_noise_std * torch.ones(num_actions)))
        else:
            raise ValueError(f"unknown noise_std_type {noise_std_type!r}")
        self.distribution: Normal | None = None
        Normal.set_default_validate_args(False)

    def train(self, mode: bool = True):
        super().train(mode)
        self.teacher.eval()  # the teacher is a fixed labeller whatever the mode
        return self

    def _std(self, mean):
        s = self.std if self.noise_std_type == "scalar" else torch.exp(self.log_std)
        return s.expand_as(mean)

    # the features the two MLPs read: the observation itself, or a memory's output in the recurrent subclass
    def _student_in(self, obs):
        return obs

    def _teacher_in(self, obs):
        return obs

    def update_distribution(self, obs):
        mean = self.student(self._student_in(obs))
        self.distribution = Normal(mean, self._std(mean))

    def act(self, obs):
        self.update_distribution(obs)
        return self.distribution.sample()

    def act_inference(self, obs):
        return self.student(self._student_in(obs))

    def evaluate(self, teacher_obs):
        with torch.no_grad():
            return self.teacher(self._teacher_in(teacher_obs))

    @property
    def action_mean(self):
        return self.distribution.mean

    @property
    def action_std(self):
        return self.distribution.stddev

    @property
    def entropy(self):
        return self.distribution.entropy().sum(dim=-1)

    def reset(self, dones=None, hidden_states=None):
        pass

    def get_hidden_states(self):
        return None, None

    def detach_hidden_states(self, dones=None):
        pass

    # checkpoint key prefixes of a PPO policy -> this module's
    _TEACHER_KEYS = {"actor.": "teacher."}

    def load_state_dict(self, state_dict, strict: bool = True):
        """Three cases, by the keys (rsl_rl): a PPO checkpoint (some key contains ``actor``) loads its actor into the
        teacher and returns False -- training starts, nothing is resumed; a distillation checkpoint (some key contains
        ``student``) loads everything and returns True; anything else raises ValueError."""
        keys = list(state_dict)
        if any("actor" in k for k in keys):
            mine = {}
            for k, v in state_dict.items():
                for src, dst in self._TEACHER_KEYS.items():
                    if k.startswith(src):
                        mine[dst + k[len(src):]] = v
            extra = [k for k in keys if k.startswith("memory_a.")] if "memory_a." not in self._TEACHER_KEYS else []
            if extra:
                raise ValueError("the teacher checkpoint is a recurrent policy (memory_a.*): build the policy with "
                                 "teacher_recurrent=True (StudentTeacherRecurrent)")
            want = {k for k in self.state_dict() if k.startswith(tuple(self._TEACHER_KEYS.values()))}
            if strict and set(mine) != want:
                raise ValueError(f"the teacher checkpoint's actor does not match the teacher network: missing "
                                 f"{sorted(want - set(mine))}, unexpected {sorted(set(mine) - want)}")
            super().load_state_dict(mine, strict=False)
            self.loaded_teacher = True
            self.teacher.eval()
            return False
        if any("student" in k for k in keys):
            super().load_state_dict(state_dict, strict=strict)
            self.loaded_teacher = True
            self.teacher.eval()
            return True
        raise ValueError("state_dict contains neither actor.* (a PPO checkpoint, the teacher) nor student.* (a "
                         "distillation checkpoint) parameters")


class StudentTeacherRecurrent(StudentTeacher):
    """rsl_rl's StudentTeacherRecurrent: ``memory_s`` (h12env.recurrent.Memory) in front of the student; with
    ``teacher_recurrent`` the teacher is a recurrent PPO actor and ``memory_t`` takes its ``memory_a``."""

    is_recurrent = True

    def __init__(self, num_student_obs: int, num_teacher_obs: int, num_actions: int,
                 student_hidden_dims=(256, 256, 256), teacher_hidden_dims=(256, 256, 256), activation="elu",
                 rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1, init_noise_std=0.1, noise_std_type="scalar",
                 teacher_recurrent=False, **kwargs):
        if "rnn_hidden_size" in kwargs:  # the spelling of rsl_rl before 2.3
            rnn_hidden_dim = kwargs.pop("rnn_hidden_size")
        self.teacher_recurrent = bool(teacher_recurrent)
        super().__init__(rnn_hidden_dim, rnn_hidden_dim if teacher_recurrent else num_teacher_obs, num_actions,
                         student_hidden_dims=student_hidden_dims, teacher_hidden_dims=teacher_hidden_dims,
                         activation=activation, init_noise_std=init_noise_std, noise_std_type=noise_std_type)
        self.memory_s = Memory(num_student_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_dim)
        if self.teacher_recurrent:
            self.memory_t = Memory(num_teacher_obs, type=rnn_type, num_layers=rnn_num_layers,
                                   hidden_size=rnn_hidden_dim)
            self.memory_t.eval()
            self._TEACHER_KEYS = {"actor.": "teacher.", "memory_a.": "memory_t."}

    def train(self, mode: bool = True):
        super().train(mode)
        if self.teacher_recurrent:
            self.memory_t.eval()
        return self

    def _student_in(self, obs):
        return self.memory_s(obs).squeeze(0)

    def _teacher_in(self, obs):
        return self.memory_t(obs).squeeze(0) if self.teacher_recurrent else obs

    def reset(self, dones=None, hidden_states=None):
        hs, ht = hidden_states if hidden_states is not None else (None, None)
        self.memory_s.reset(dones, hs)
        if self.teacher_recurrent:
            self.memory_t.reset(dones, ht)

    def get_hidden_states(self):
        return self.memory_s.hidden_states, (self.memory_t.hidden_states if self.teacher_recurrent else None)

    def detach_hidden_states(self, dones=None):
        """Cut the autograd history of the memories' states (all rows; ``dones`` is accepted for rsl_rl's signature:
        a row that was just zeroed carries no history either way)."""
        for mem in (self.memory_s,) + ((self.memory_t,) if self.teacher_recurrent else ()):
            if mem.hidden_states is not None:
                hs = tuple(s.detach() for s in state_tensors(mem.hidden_states))
                mem.hidden_states = hs if isinstance(mem.hidden_states, (tuple, list)) else hs[0]


class StudentView:
    """The student as the exporters and the deploy wrappers see a PPO policy (h12env.export.export_policy_as_jit /
    _onnx): ``actor`` is the student MLP, ``memory_a`` the student's memory."""

    def __init__(self, policy: StudentTeacher):
        self.actor = policy.student
        self.is_recurrent = bool(policy.is_recurrent)
        if self.is_recurrent:
            self.memory_a = policy.memory_s


def is_student_checkpoint(model_state_dict) -> bool:
    """A distillation checkpoint says so itself: it has student.* parameters (and no actor.*)."""
    return any(k.startswith("student.") for k in model_state_dict) and not any("actor" in k for k in model_state_dict)


def cfg_from_checkpoint(sd, activation: str = "elu"):
    """(policy section of the train cfg, student history length) read from a distillation checkpoint's parameters: the
    two MLPs' hidden widths, the memories' type and size, and H = the student's input width / 45."""
    def hidden(prefix):
        ws = sorted((int(k.split(".")[1]), v.shape[0]) for k, v in sd.items()
                    if k.startswith(prefix) and k.endswith(".weight"))
        return [w for _, w in ws[:-1]]

    policy = {"class_name": "StudentTeacher", "student_hidden_dims": hidden("student."),
              "teacher_hidden_dims": hidden("teacher."), "activation": activation,
              "noise_std_type": "log" if "log_std" in sd else "scalar"}
    width = sd["student.0.weight"].shape[1]
    if "memory_s.rnn.weight_ih_l0" in sd:
        w_ih, w_hh = sd["memory_s.rnn.weight_ih_l0"], sd["memory_s.rnn.weight_hh_l0"]
        policy.update(class_name="StudentTeacherRecurrent", rnn_hidden_dim=w_hh.shape[1],
                      rnn_type="lstm" if w_ih.shape[0] == 4 * w_hh.shape[1] else "gru",
                      rnn_num_layers=len([k for k in sd if k.startswith("memory_s.rnn.weight_ih_l")]),
                      teacher_recurrent="memory_t.rnn.weight_ih_l0" in sd)
        width = w_ih.shape[1]
    from .student import FRAME

    if width % FRAME:
        raise ValueError(f"the checkpoint's student reads {width} inputs: no multiple of the {FRAME}-wide student frame")
    return policy, width // FRAME


def student_group_from_run(run_dir, history: int):
    """The StudentObsCfg a student run was trained on, read from the run's params/env.yaml (what train.py dumps): its
    history, per-term scales and noise.  Without that file: the defaults with ``history`` (the checkpoint's input
    width says that much).  The history must agree with the checkpoint's."""
    import yaml

    from .cfg import StudentObsCfg, Unoise
    from .student import TERMS

    path = os.path.join(str(run_dir), "params", "env.yaml")
    group = StudentObsCfg(history_length=history)
    if not os.path.exists(path):
        return group
    with open(path) as f:
        d = ((yaml.safe_load(f) or {}).get("observations") or {}).get("student")
    if not d:
        return group
    if int(d.get("history_length", history)) != history:
        raise ValueError(f"{path}: student history_length {d.get('history_length')} but the checkpoint's student reads "
                         f"{history} frames")
    group.enable_corruption = bool(d.get("enable_corruption", True))
    group.scales = {k: float(v) for k, v in (d.get("scales") or {}).items()}
    for t in TERMS:
        u = d.get(t)
        setattr(group, t, None if u is None else Unoise(float(u["n_min"]), float(u["n_max"])))
    return group


# ---------------------------------------------------------------------------------------------- algorithm
class DistillationStorage:
    """(T, N, ...) device tensors of one distillation iteration."""

    def __init__(self, num_envs, num_steps, student_obs_dim, teacher_obs_dim, num_actions, device):
        T, N = num_steps, num_envs
        self.num_envs, self.num_steps, self.device = N, T, device
        z = lambda *s: torch.zeros(*s, device=device)  # noqa: E731
        self.observations = z(T, N, student_obs_dim)
        self.privileged_observations = z(T, N, teacher_obs_dim)
        self.actions = z(T, N, num_actions)
        self.privileged_actions = z(T, N, num_actions)
        self.rewards = z(T, N, 1)
        self.dones = torch.zeros(T, N, dtype=torch.uint8, device=device)
        self.step = 0

    def add(self, obs, teacher_obs, actions, teacher_actions, rewards, dones):
        if self.step >= self.num_steps:
            raise OverflowError("rollout storage overflow: call update() / clear() first")
        t = self.step
        self.observations[t].copy_(obs)
        self.privileged_observations[t].copy_(teacher_obs)
        self.actions[t].copy_(actions)
        self.privileged_actions[t].copy_(teacher_actions)
        self.rewards[t].copy_(rewards.view(-1, 1))
        self.dones[t].copy_(dones.view(-1) != 0)
        self.step += 1

    def clear(self):
        self.step = 0


def _loss_rows(loss_type: str):
    """The unreduced loss: rsl_rl's mse_loss / huber_loss (delta 1) before their mean."""
    if loss_type == "mse":
        return lambda a, b: nn.functional.mse_loss(a, b, reduction="none")
    if loss_type == "huber":
        return lambda a, b: nn.functional.huber_loss(a, b, reduction="none")
    raise ValueError(f"unknown loss type {loss_type!r} (mse or huber)")


def update_segments(num_steps: int, epochs: int, gradient_length: int):
    """The update's schedule: a list of chunks, each (segments, backprop) with segments = [(epoch, t0, t1)] -- runs of
    consecutive steps inside one epoch.  Steps are counted across the epochs; every full chunk of gradient_length
    steps is backpropagated, the trailing remainder (backprop False) is only evaluated."""
    total = epochs * num_steps
    chunks = []
    for g0 in range(0, total, gradient_length):
        g1 = min(g0 + gradient_length, total)
        segs, g = [], g0
        while g < g1:
            e, t0 = divmod(g, num_steps)
            t1 = min(num_steps, t0 + (g1 - g))
            segs.append((e, t0, t1))
            g += t1 - t0
        chunks.append((segs, g1 - g0 == gradient_length))
    return chunks


class Distillation(_DeviceLrAdam):
    """rsl_rl 2.3's Distillation: behaviour cloning of the teacher's action on the student's own rollouts, truncated
    BPTT every ``gradient_length`` steps, Adam over the policy's parameters, no gradient clipping."""

    rnd = None  # no reward to add an exploration bonus to (the runner refuses rnd_cfg)

    def __init__(self, policy, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, loss_type="mse",
                 device="cpu", fused_rnn_update: bool | None = None, shard: D.Shard | None = None, **kwargs):
        if kwargs.get("symmetry_cfg") is not None:
            raise ValueError("symmetry_cfg is not supported with Distillation (the student copies the teacher's action; "
                             "train the teacher with symmetry instead)")
        self.shard = shard or D.Shard(0, 1, 0, 0)
        if self.shard.world > 1:
            raise ValueError("Distillation runs on one GPU (the update is a sequence over every env of the rollout)")
        self.policy = policy.to(device)
        self.device = device
        self._init_optimizer(learning_rate)
        self.num_learning_epochs = int(num_learning_epochs)
        self.gradient_length = int(gradient_length)
        if self.gradient_length < 1 or self.num_learning_epochs < 1:
            raise ValueError("gradient_length and num_learning_epochs must be at least 1")
        self.loss_type = loss_type
        self._loss_rows = _loss_rows(loss_type)
        self.recurrent = bool(getattr(policy, "is_recurrent", False))
        # a recurrent student's chunks on the h12learn_lstm_seq_* kernels; None reads H12_RNN_UPDATE_FUSED=1
        if fused_rnn_update is None:
            fused_rnn_update = os.environ.get("H12_RNN_UPDATE_FUSED", "0") == "1"
        self.fused_rnn_update = bool(fused_rnn_update)
        if self.fused_rnn_update:
            from .recurrent import lstm_sequence_limit

            if not self.recurrent:
                raise ValueError(f"fused_rnn_update needs a recurrent student, {type(policy).__name__} has no memory")
            why = lstm_sequence_limit(self.policy.memory_s.rnn)
            if why:
                raise ValueError(f"fused_rnn_update: memory_s: {why}")
        self.storage: DistillationStorage | None = None
        self.last_hidden_states = None  # the student's state the last update ended with: where this rollout began
        self.num_updates = 0
        self._fused = None  # H12_POLICY_FUSED=1: (teacher wrapper, student wrapper)
        self._student_stale = False  # the plain student's packed weights are older than its parameters

    def init_storage(self, num_envs, num_steps, student_obs_shape, teacher_obs_shape, action_shape):
        self.storage = DistillationStorage(num_envs, num_steps, student_obs_shape[0], teacher_obs_shape[0],
                                           action_shape[0], self.device)
        total = self.num_learning_epochs * num_steps
        if total % self.gradient_length != 0:
            warnings.warn(f"Distillation: num_learning_epochs x num_steps_per_env = {total} is no multiple of "
                          f"gradient_length = {self.gradient_length}: the last {total % self.gradient_length} steps of "
                          "every update are evaluated but never backpropagated (as in rsl_rl)", stacklevel=2)

    # ---- collection
    def _fused_wrappers(self):
        """H12_POLICY_FUSED=1: the teacher's labels and the student's mean on the fused forward kernels
        (policy.FusedMLP / policy.RecurrentPolicy).  The student's is re-packed after every update."""
        if self._fused is None:
            from .policy import FusedMLP, RecurrentPolicy

            p = self.policy
            if self.recurrent and p.teacher_recurrent:
                teacher = RecurrentPolicy(p.memory_t.rnn, p.teacher, None, fused=True)
            else:
                f = FusedMLP([p.teacher])
                teacher = lambda x: f(x)[0]  # noqa: E731
            if self.recurrent:
                student = RecurrentPolicy(p.memory_s.rnn, p.student, None, fused=True)
                self._load_wrapper_state(student)
            else:
                g = FusedMLP([p.student])
                student = lambda x: g(x, repack=self._student_stale)[0]  # noqa: E731
            self._student_stale = False
            self._fused = (teacher, student)
        return self._fused

    def _load_wrapper_state(self, wrapper):
        """The student wrapper's own (h, c) <- the memory's state (what the last update ended with)."""
        hs = self.policy.memory_s.hidden_states
        if hs is not None:
            with torch.inference_mode(False):
                wrapper.state = tuple(s.detach().clone() for s in state_tensors(hs))

    def act(self, obs, teacher_obs):
        self._obs, self._teacher_obs = obs, teacher_obs
        if fused_collection_on(obs):
            teacher, student = self._fused_wrappers()
            with torch.no_grad():
                mean = student(obs)
                self._student_stale = False
                self._actions = mean + self.policy._std(mean) * torch.randn_like(mean)  # as PPO._act_compute
                self._teacher_actions = teacher(teacher_obs)
            return self._actions
        self._actions = self.policy.act(obs).detach()
        self._teacher_actions = self.policy.evaluate(teacher_obs).detach()
        return self._actions

    def process_env_step(self, rewards, dones, infos):
        self.storage.add(self._obs, self._teacher_obs, self._actions, self._teacher_actions, rewards, dones)
        self.policy.reset(dones)
        if self._fused is not None:
            for w in self._fused:
                if hasattr(w, "reset"):
                    w.reset(dones)

    # ---- learning
    def _start_state(self, n: int):
        """The detached state an epoch starts from: the one the last update ended with, zeros before the first."""
        rnn = self.policy.memory_s.rnn
        hs = self.last_hidden_states[0] if self.last_hidden_states is not None else None
        if hs is None:
            k = 2 if isinstance(rnn, nn.LSTM) else 1
            hs = tuple(torch.zeros(rnn.num_layers, n, rnn.hidden_size, device=self.device,
                                   dtype=rnn.weight_hh_l0.dtype) for _ in range(k))
        return tuple(s.detach() for s in state_tensors(hs))

    def _segment(self, t0: int, t1: int, state):
        """sum over t0 <= t < t1 of mean_{envs, actions} loss(act_inference(obs_t), teacher_action_t) as ONE call over
        the [t1 - t0, N] block, and the student's state after step t1 - 1 (zeroed where that step was a done)."""
        st = self.storage
        dt = self.policy.student[0].weight.dtype  # the rollout is float32; a float64 policy reads it widened
        obs, target, dones = st.observations[t0:t1].to(dt), st.privileged_actions[t0:t1].to(dt), st.dones[t0:t1]
        L, N = obs.shape[:2]
        if self.recurrent:
            rnn = self.policy.memory_s.rnn
            hx = state if len(state) > 1 else state[0]
            feats, new = lstm_sequence_state(rnn, obs, dones, hx, kernels=self.fused_rnn_update)
            keep = (dones[-1] == 0).to(obs.dtype).view(1, N, 1)
            state = tuple(s * keep for s in state_tensors(new))
        else:
            feats = obs
        mean = self.policy.student(feats.reshape(L * N, -1)).view(L, N, -1)
        return self._loss_rows(mean, target).mean(dim=(1, 2)).sum(), state

    def update(self):
        st = self.storage
        T, N = st.num_steps, st.num_envs
        if st.step != T:
            raise RuntimeError(f"update() after {st.step} of {T} collected steps")
        self.num_updates += 1
        total = self.num_learning_epochs * T
        mean_loss = torch.zeros((), device=self.device)
        state = None
        for segs, backprop in update_segments(T, self.num_learning_epochs, self.gradient_length):
            loss = 0.0
            for _, t0, t1 in segs:
                if t0 == 0 and self.recurrent:  # every epoch restarts where the rollout began
                    state = self._start_state(N)
                seg_loss, state = self._segment(t0, t1, state)
                loss = loss + seg_loss
            mean_loss += loss.detach()
            if backprop:
                self.optimizer.zero_grad()
                loss.backward()
                self.optimizer.step()
            if state is not None:
                state = tuple(s.detach() for s in state)
        st.clear()
        if self.recurrent:  # the memory goes on from here: the next rollout's first step, and the next update's start
            rnn = self.policy.memory_s.rnn
            self.policy.memory_s.hidden_states = state if isinstance(rnn, nn.LSTM) else state[0]
            # a copy of its own: reset(dones) zeroes the memory's rows in place during the next rollout (with the fused
            # collection nothing rebinds them first), and the next update starts from this state as it is now
            self.last_hidden_states = tuple(None if hs is None else tuple(t.detach().clone() for t in state_tensors(hs))
                                            for hs in self.policy.get_hidden_states())
            if self._fused is not None:
                self._fused[1].refresh()
                self._load_wrapper_state(self._fused[1])
        self._student_stale = True
        return {"behavior": mean_loss / total}

    def broadcast_parameters(self):
        pass  # one GPU


# ---------------------------------------------------------------------------------------------- runner
def wants_distillation(train_cfg: dict) -> bool:
    """Whether the cfg names the Distillation algorithm or a StudentTeacher* policy.  One without the other is refused
    here, with a message."""
    alg = (train_cfg.get("algorithm") or {}).get("class_name") or "PPO"
    pol = (train_cfg.get("policy") or {}).get("class_name") or "ActorCritic"
    if alg == "Distillation" and pol not in POLICY_CLASSES:
        raise ValueError(f"algorithm.class_name = 'Distillation' needs a StudentTeacher or StudentTeacherRecurrent "
                         f"policy, not policy.class_name = {pol!r}")
    if pol in POLICY_CLASSES and alg != "Distillation":
        raise ValueError(f"policy.class_name = {pol!r} is trained by algorithm.class_name = 'Distillation', not {alg!r}")
    return alg == "Distillation"


class DistillationRunner(OnPolicyRunner):
    """What OnPolicyRunner(env, train_cfg) builds for ``algorithm.class_name = "Distillation"``: the same surface
    (learn / save / load / get_inference_policy), serving the student.  ``train_cfg["obs_groups"]`` names the env's
    observation groups the two networks read; the default is {"student": "student", "teacher": "policy"} -- the teacher
    reads the group it was trained on (rsl_rl 2.3 calls that group "teacher")."""

    _inference_modules = ("memory_s", "student")

    def _build_algorithm(self):
        env, device = self.env, self.device
        if self.shard.world > 1:
            raise ValueError("Distillation runs on one GPU: start it without torchrun (several GPUs are not supported)")
        if self.alg_cfg.get("symmetry_cfg") is not None:
            raise ValueError("symmetry_cfg is not supported with Distillation (the student copies the teacher's action; "
                             "train the teacher with symmetry instead)")
        if self.alg_cfg.get("rnd_cfg") is not None:
            raise ValueError("rnd_cfg is not supported with Distillation (there is no reward to add an exploration "
                             "bonus to)")
        class_name = self.policy_cfg.pop("class_name")
        if self.empirical_normalization and class_name == "StudentTeacherRecurrent":
            raise ValueError("empirical_normalization is not supported with a recurrent student: the update's sequence "
                             "form reads the stored observations as they are")
        self.obs_groups = {**DEFAULT_OBS_GROUPS, **(self.cfg.get("obs_groups") or {})}
        s_obs, t_obs = self._split(env.get_observations()[1])
        cls = {"StudentTeacher": StudentTeacher, "StudentTeacherRecurrent": StudentTeacherRecurrent}[class_name]
        policy = cls(s_obs.shape[1], t_obs.shape[1], env.num_actions, **self.policy_cfg).to(device)
        for k in ("class_name", "rnd_cfg", "symmetry_cfg"):
            self.alg_cfg.pop(k, None)
        self.alg = Distillation(policy, device=device, shard=self.shard, **self.alg_cfg)
        self.obs_normalizer = self._normalizer(s_obs.shape[1])
        self.teacher_obs_normalizer = self._normalizer(t_obs.shape[1])
        self.teacher_obs_normalizer.eval()  # the teacher's statistics come with its checkpoint and stay
        self.alg.init_storage(env.num_envs, self.num_steps_per_env, [s_obs.shape[1]], [t_obs.shape[1]],
                              [env.num_actions])

    def _split(self, extras):
        """(student observation, teacher observation) of a step's extras["observations"]."""
        groups = extras["observations"]
        out = []
        for role in ("student", "teacher"):
            name = self.obs_groups[role]
            if name not in groups:
                hint = " (set env_cfg.observations.student, e.g. train.py --distill)" if name == "student" else ""
                raise ValueError(f"obs_groups[{role!r}] = {name!r}: the env has no such observation group, only "
                                 f"{sorted(groups)}{hint}")
            out.append(groups[name])
        return out

    def _check_ready(self):
        if not self.alg.policy.loaded_teacher:
            raise ValueError("Distillation needs a trained teacher: load a PPO checkpoint first "
                             "(runner.load(path), train.py --teacher_checkpoint PATH)")

    def _first_inputs(self):
        """The first (student, teacher) observations go through the normalisers, as every later pair."""
        return self._step_inputs(*self.env.get_observations())

    def _step_inputs(self, obs, infos):
        s_obs, t_obs = (x.to(self.device) for x in self._split(infos))
        return self.obs_normalizer(s_obs), self.teacher_obs_normalizer(t_obs)

    def _end_collection(self, teacher_obs):
        pass  # no returns to compute: the update reads the stored teacher actions

    def _loss_scalars(self, loss: dict) -> dict:
        return {"Loss/behavior": float(loss["behavior"])}  # the device scalar is read here, at the iteration's log line

    def _checkpoint_extras(self) -> dict:
        if not self.empirical_normalization:
            return {}
        return {"privileged_obs_norm_state_dict": self.teacher_obs_normalizer.state_dict()}

    def load(self, path: str, load_optimizer: bool = True):
        """A PPO checkpoint: its actor becomes the teacher (and its observation normaliser the teacher's), the student
        starts fresh at iteration 0.  A distillation checkpoint: everything is restored, training resumes."""
        d = torch.load(path, map_location=self.device, weights_only=True)
        sd = d["model_state_dict"]
        teacher_only = any("actor" in k for k in sd)
        has_norm = "obs_norm_state_dict" in d
        if not teacher_only and has_norm != self.empirical_normalization:
            raise ValueError(f"{path}: the student was trained {'with' if has_norm else 'without'} "
                             f"empirical_normalization, this run is set up {'with' if self.empirical_normalization else 'without'} "
                             "it: the student would read observations it was not trained on")
        if teacher_only and has_norm != self.empirical_normalization:
            raise ValueError(f"{path}: the teacher was trained {'with' if has_norm else 'without'} "
                             f"empirical_normalization, this run is set up {'with' if self.empirical_normalization else 'without'} "
                             "it: the teacher would read observations it was not trained on")
        resumed = self.alg.policy.load_state_dict(sd)
        if self.empirical_normalization:
            if teacher_only:
                self.teacher_obs_normalizer.load_state_dict(d["obs_norm_state_dict"])
            else:
                self.obs_normalizer.load_state_dict(d["obs_norm_state_dict"])
                self.teacher_obs_normalizer.load_state_dict(d["privileged_obs_norm_state_dict"])
        if resumed:
            if load_optimizer and "optimizer_state_dict" in d:
                self.alg.load_optimizer_state_dict(d["optimizer_state_dict"])
            self.current_learning_iteration = int(d.get("iter", 0))
        self.alg._fused = None  # the fused wrappers are packed from the parameters: rebuilt on the next act()
        return d.get("infos")

    def _mode_modules(self) -> list:
        return [self.alg.policy, self.obs_normalizer]  # not the teacher's normaliser: it stays in eval mode
