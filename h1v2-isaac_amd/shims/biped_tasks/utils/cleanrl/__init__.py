"""biped_tasks.utils.cleanrl: ppo (PPO, Agent, RunningMeanStd) and rl_cfg (CleanRlPpoActorCriticCfg)."""
