"""biped_tasks.utils: the CleanRL PPO surface of the CaT tasks."""
