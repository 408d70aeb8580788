"""biped_tasks.utils.cleanrl.ppo: the CleanRL PPO of the CaT tasks on this stack (h12env.cleanrl)."""
from h12env.cleanrl import PPO, Agent, RunningMeanStd, layer_init, update_mean_var_count_from_moments

__all__ = ["PPO", "Agent", "RunningMeanStd", "layer_init", "update_mean_var_count_from_moments"]
