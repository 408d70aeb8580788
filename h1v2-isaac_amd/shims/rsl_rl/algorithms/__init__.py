from h12env.distill import Distillation
from h12env.ppo import PPO

__all__ = ["PPO", "Distillation"]
