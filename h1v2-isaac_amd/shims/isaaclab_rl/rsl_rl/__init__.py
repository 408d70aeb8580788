"""isaaclab_rl.rsl_rl: runner / policy / algorithm cfgs and RslRlVecEnvWrapper (IsaacLab 2.1 surface)."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field

import torch

from isaaclab.utils.dict import class_to_dict


@dataclass
class RslRlPpoActorCriticCfg:
    class_name: str = "ActorCritic"
    init_noise_std: float = 1.0
    noise_std_type: str = "scalar"
    actor_hidden_dims: list = field(default_factory=lambda: [256, 256, 256])
    critic_hidden_dims: list = field(default_factory=lambda: [256, 256, 256])
    activation: str = "elu"


@dataclass
class RslRlPpoActorCriticRecurrentCfg(RslRlPpoActorCriticCfg):
    """rsl_rl's ActorCriticRecurrent (h12env.ppo.ActorCriticRecurrent): a memory in front of the actor and critic MLPs."""
    class_name: str = "ActorCriticRecurrent"
    rnn_type: str = "lstm"
    rnn_hidden_dim: int = 256
    rnn_num_layers: int = 1


@dataclass
class RslRlSymmetryCfg:
    """rsl_rl 2.3 symmetry options (isaaclab_rl.rsl_rl.symmetry_cfg.RslRlSymmetryCfg).  data_augmentation_func is
    a callable or a "module:func" string with rsl_rl's signature (obs, actions, env, obs_type) -> (obs, actions);
    the H1-2 tasks ship theirs as "h12env.symmetry:augment"."""
    use_data_augmentation: bool = False
    use_mirror_loss: bool = False
    data_augmentation_func: object = None
    mirror_loss_coeff: float = 0.0


@dataclass
class RslRlRndCfg:
    """rsl_rl 2.3 Random Network Distillation options (isaaclab_rl.rsl_rl.rnd_cfg.RslRlRndCfg; h12env.rnd).  The env
    must serve the observation group "rnd_state" (env_cfg.observations.rnd_state).  weight_schedule is None or a dict
    {"mode": "constant" | "step" | "linear", ...}; -1 in the hidden dims means the width of rnd_state."""
    weight: float = 0.0
    weight_schedule: dict | None = None
    reward_normalization: bool = False
    state_normalization: bool = False
    learning_rate: float = 1.0e-3
    num_outputs: int = 1
    predictor_hidden_dims: list = field(default_factory=lambda: [-1])
    target_hidden_dims: list = field(default_factory=lambda: [-1])
    # h12env.rnd extension: the per-env-step reward work on the h12learn_rnd_* kernels (None: H12_RND_FUSED)
    fused: bool | None = None


@dataclass
class RslRlPpoAlgorithmCfg:
    class_name: str = "PPO"
    num_learning_epochs: int = 5
    num_mini_batches: int = 4
    learning_rate: float = 1.0e-3
    schedule: str = "adaptive"
    gamma: float = 0.99
    lam: float = 0.95
    entropy_coef: float = 0.01
    desired_kl: float = 0.01
    max_grad_norm: float = 1.0
    value_loss_coef: float = 1.0
    use_clipped_value_loss: bool = True
    clip_param: float = 0.2
    normalize_advantage_per_mini_batch: bool = False
    symmetry_cfg: RslRlSymmetryCfg | dict | None = None
    rnd_cfg: RslRlRndCfg | dict | None = None
    # h12env.ppo extension: actor and critic of the update on the fused HIP forward / backward (None: H12_LEARNER_FUSED)
    fused_learner: bool | None = None
    # h12env.ppo extension: the update's loss head as one HIP call, h12env.ppo_head.PPOHead (None: H12_PPO_HEAD_FUSED)
    fused_loss: bool | None = None
    # h12env.ppo extension: a recurrent policy's update in the sequence form on the h12learn_lstm_seq_* kernels
    # (None: H12_RNN_UPDATE_FUSED)
    fused_rnn_update: bool | None = None
    # h12env.ppo extension: gradient clip and Adam step as two HIP launches, h12env.optim.FusedClipAdam
    # (None: H12_OPTIMIZER_FUSED)
    fused_optimizer: bool | None = None


@dataclass
class RslRlDistillationStudentTeacherCfg:
    """rsl_rl's StudentTeacher (h12env.distill.StudentTeacher): the student MLP that is trained and the teacher MLP that
    a PPO checkpoint's actor is loaded into."""
    class_name: str = "StudentTeacher"
    init_noise_std: float = 0.1
    noise_std_type: str = "scalar"
    student_hidden_dims: list = field(default_factory=lambda: [256, 256, 256])
    teacher_hidden_dims: list = field(default_factory=lambda: [256, 256, 256])
    activation: str = "elu"


@dataclass
class RslRlDistillationStudentTeacherRecurrentCfg(RslRlDistillationStudentTeacherCfg):
    """rsl_rl's StudentTeacherRecurrent (h12env.distill.StudentTeacherRecurrent): a memory in front of the student, and
    in front of the teacher when the teacher is a recurrent PPO policy."""
    class_name: str = "StudentTeacherRecurrent"
    rnn_type: str = "lstm"
    rnn_hidden_dim: int = 256
    rnn_num_layers: int = 1
    teacher_recurrent: bool = False


@dataclass
class RslRlDistillationAlgorithmCfg:
    """rsl_rl's Distillation (h12env.distill.Distillation)."""
    class_name: str = "Distillation"
    num_learning_epochs: int = 1
    learning_rate: float = 1.0e-3
    gradient_length: int = 15
    loss_type: str = "mse"
    # h12env.distill extension: a recurrent student's chunks on the h12learn_lstm_seq_* kernels (None:
    # H12_RNN_UPDATE_FUSED)
    fused_rnn_update: bool | None = None


@dataclass
class RslRlOnPolicyRunnerCfg:
    seed: int = 42
    device: str = "cuda:0"
    num_steps_per_env: int = 24
    max_iterations: int = 1500
    empirical_normalization: bool = False
    policy: "RslRlPpoActorCriticCfg | RslRlDistillationStudentTeacherCfg" = field(default_factory=RslRlPpoActorCriticCfg)
    algorithm: "RslRlPpoAlgorithmCfg | RslRlDistillationAlgorithmCfg" = field(default_factory=RslRlPpoAlgorithmCfg)
    clip_actions: float | None = None
    save_interval: int = 50
    experiment_name: str = "default"
    run_name: str = ""
    logger: str = "tensorboard"
    neptune_project: str = "isaaclab"
    wandb_project: str = "isaaclab"
    resume: bool = False
    load_run: str = ".*"
    load_checkpoint: str = "model_.*.pt"

    def to_dict(self) -> dict:
        return class_to_dict(self)

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


class RslRlVecEnvWrapper:
    """Wraps the env for rsl_rl: obs tensor + {"observations": obs_dict} extras, long dones, time-outs."""

    def __init__(self, env, clip_actions: float | None = None):
        self.env = env
        self.clip_actions = clip_actions
        u = env.unwrapped
        self.num_envs = u.num_envs
        self.device = u.device
        self.max_episode_length = u.max_episode_length
        self.num_actions = u.action_manager.total_action_dim
        self.num_obs = u.observation_manager.group_obs_dim["policy"][0]
        crit = u.observation_manager.group_obs_dim.get("critic")
        self.num_privileged_obs = crit[0] if crit is not None else None
        self.shard = getattr(u, "shard", None)
        self.env.reset()

    def __str__(self):
        return f"<{type(self).__name__}{self.env}>"

    @property
    def cfg(self):
        return self.unwrapped.cfg

    @property
    def render_mode(self):
        return getattr(self.env, "render_mode", None)

    @property
    def observation_space(self):
        return getattr(self.env, "observation_space", None)

    @property
    def action_space(self):
        return getattr(self.env, "action_space", None)

    @classmethod
    def class_name(cls) -> str:
        return cls.__name__

    @property
    def unwrapped(self):
        return self.env.unwrapped

    @property
    def episode_length_buf(self) -> torch.Tensor:
        return self.unwrapped.episode_length_buf

    @episode_length_buf.setter
    def episode_length_buf(self, value: torch.Tensor):
        self.unwrapped.episode_length_buf = value

    def seed(self, seed: int = -1) -> int:
        return self.unwrapped.seed(seed)

    def get_observations(self):
        obs_dict = self.unwrapped.observation_manager.compute()
        return obs_dict["policy"], {"observations": obs_dict}

    def reset(self):
        obs_dict, _ = self.env.reset()
        return obs_dict["policy"], {"observations": obs_dict}

    def step(self, actions: torch.Tensor):
        if self.clip_actions is not None:
            actions = torch.clamp(actions, -self.clip_actions, self.clip_actions)
        obs_dict, rew, terminated, truncated, extras = self.env.step(actions)
        dones = (terminated | truncated).to(dtype=torch.long)
        extras["observations"] = obs_dict
        if not getattr(self.unwrapped.cfg, "is_finite_horizon", False):
            extras["time_outs"] = truncated
        return obs_dict["policy"], rew, dones, extras

    def close(self):
        return self.env.close()


def export_policy_as_jit(policy, normalizer, path: str, filename="policy.pt"):
    from h12env.export import export_policy_as_jit as f

    return f(policy, normalizer, path, filename)


def export_policy_as_onnx(policy, normalizer, path: str, filename="policy.onnx", verbose=False):
    from h12env.export import export_policy_as_onnx as f

    return f(policy, normalizer, path, filename, verbose)


__all__ = ["RslRlDistillationAlgorithmCfg", "RslRlDistillationStudentTeacherCfg",
           "RslRlDistillationStudentTeacherRecurrentCfg", "RslRlOnPolicyRunnerCfg", "RslRlPpoActorCriticCfg",
           "RslRlPpoAlgorithmCfg", "RslRlRndCfg", "RslRlSymmetryCfg", "RslRlVecEnvWrapper", "export_policy_as_jit",
           "export_policy_as_onnx"]
