"""biped_tasks.utils.cleanrl.rl_cfg: the CleanRL PPO cfg base class (h12env.cleanrl)."""
from h12env.cleanrl import MISSING, CleanRlPpoActorCriticCfg

__all__ = ["MISSING", "CleanRlPpoActorCriticCfg"]
