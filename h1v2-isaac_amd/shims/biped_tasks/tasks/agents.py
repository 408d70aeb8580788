"""PPO runner cfgs of the H1-2 12-DoF tasks (values of biped_tasks/.../h12_12dof/agents/rsl_rl_ppo_cfg.py:10-47
and, for the CaT tasks, agents/clean_rl_ppo_cfg.py)."""
from dataclasses import dataclass, field

from biped_tasks.utils.cleanrl.rl_cfg import CleanRlPpoActorCriticCfg
from isaaclab_rl.rsl_rl import RslRlOnPolicyRunnerCfg, RslRlPpoActorCriticCfg, RslRlPpoAlgorithmCfg


@dataclass
class H12_12dof_RoughPPORunnerCfg(RslRlOnPolicyRunnerCfg):
    num_steps_per_env: int = 24
    max_iterations: int = 3000
    save_interval: int = 100
    experiment_name: str = "h12_12dof_rough"
    empirical_normalization: bool = False
    policy: RslRlPpoActorCriticCfg = field(default_factory=lambda: RslRlPpoActorCriticCfg(
        init_noise_std=1.0, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu"))
    algorithm: RslRlPpoAlgorithmCfg = field(default_factory=lambda: RslRlPpoAlgorithmCfg(
        value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.0081, num_learning_epochs=5,
        num_mini_batches=4, learning_rate=1.0e-3, schedule="adaptive", gamma=0.99, lam=0.95, desired_kl=0.01,
        max_grad_norm=1.0))


@dataclass
class H12_12dof_FlatPPORunnerCfg(H12_12dof_RoughPPORunnerCfg):
    max_iterations: int = 3000
    experiment_name: str = "h12_12dof_flat"


@dataclass
class H12_12dof_FlatCleanRlPPOCfg(CleanRlPpoActorCriticCfg):
    """The CaT tasks' CleanRL PPO cfg (values of .../h12_12dof/agents/clean_rl_ppo_cfg.py:11-32)."""
    save_interval: int = 200
    learning_rate: float = 3.0e-4
    num_steps: int = 24
    num_iterations: int = 50000
    gamma: float = 0.99
    gae_lambda: float = 0.95
    updates_epochs: int = 5
    minibatch_size: int = 16384
    clip_coef: float = 0.2
    ent_coef: float = 0.0081
    vf_coef: float = 2.0
    max_grad_norm: float = 1.0
    norm_adv: bool = True
    clip_vloss: bool = True
    anneal_lr: bool = True
    experiment_name: str = "h12_12dof_flat"
    logger: str = "tensorboard"
    wandb_project: str = "h12_12dof_flat"
    load_run: str = ".*"
    load_checkpoint: str = "model_.*.pt"
