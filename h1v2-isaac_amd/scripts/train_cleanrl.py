#!/usr/bin/env python3
"""CleanRL PPO training of a Constraints-as-Terminations task on the MI355X env.

Command line, configuration sources and log artefacts follow the reference's scripts/clean_rl/train.py
(+ cli_args.py): task / num_envs / seed / num_iterations / experiment_name / resume / load_run / checkpoint /
logger / log_project_name flags, AppLauncher flags, Hydra-style ``env.*=`` / ``agent.*=`` overrides; a run lands
in logs/clean_rl/<experiment>/<timestamp>/ with params/{env,agent}.{yaml,pkl}, params/deploy_config.yaml,
metrics.jsonl and model_<it>.pt (the agent's state_dict).  ``--resume`` starts from the checkpoint that
``--load_run`` / ``--checkpoint`` select (the reference parses the flags and never loads).

    python train_cleanrl.py --task Isaac-Velocity-CaT-Flat-H12_12dof-v0 --num_envs 4096 --headless
"""
from __future__ import annotations

import argparse
import os
import sys
from datetime import datetime
from pathlib import Path

HERE = Path(__file__).resolve().parent
PKG = HERE.parent
for p in (PKG / "shims", PKG):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

from isaaclab.app import AppLauncher  # noqa: E402


def add_clean_rl_args(ap: argparse.ArgumentParser):
    g = ap.add_argument_group("clean_rl", description="Arguments for CleanRL agent.")
    g.add_argument("--experiment_name", type=str, default=None)
    g.add_argument("--resume", type=bool, default=None)
    g.add_argument("--load_run", type=str, default=None)
    g.add_argument("--checkpoint", type=str, default=None)
    g.add_argument("--logger", type=str, default=None, choices={"wandb", "tensorboard"})
    g.add_argument("--log_project_name", type=str, default=None)


def update_clean_rl_cfg(agent_cfg, args):
    """cli_args.update_clean_rl_cfg."""
    if getattr(args, "seed", None) is not None:
        agent_cfg.seed = args.seed
    if args.resume is not None:
        agent_cfg.resume = args.resume
    if args.experiment_name is not None:
        agent_cfg.experiment_name = args.experiment_name
    if args.load_run is not None:
        agent_cfg.load_run = args.load_run
    if args.checkpoint is not None:
        agent_cfg.load_checkpoint = args.checkpoint
    if args.logger is not None:
        agent_cfg.logger = args.logger
    if agent_cfg.logger in {"wandb"} and args.log_project_name:
        agent_cfg.wandb_project = args.log_project_name
    return agent_cfg


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Train an RL agent with CleanRL.")
    ap.add_argument("--video", action="store_true", default=False)
    ap.add_argument("--video_length", type=int, default=200)
    ap.add_argument("--video_interval", type=int, default=2000)
    ap.add_argument("--num_envs", type=int, default=None)
    ap.add_argument("--task", type=str, default="Isaac-Velocity-CaT-Flat-H12_12dof-v0")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--num_iterations", type=int, default=None)
    ap.add_argument("--fused_loss", action="store_true", default=False,
                    help="fused loss head (h12learn_cleanrl_head) and, on the GPU, the update as a captured graph")
    ap.add_argument("--fused_optimizer", action="store_true", default=False,
                    help="gradient clip and RAdam step as two fused HIP launches (h12env.optim.FusedClipRAdam)")
    add_clean_rl_args(ap)
    AppLauncher.add_app_launcher_args(ap)
    return ap


def main(argv=None) -> int:
    args, hydra_args = build_parser().parse_known_args(argv)
    if args.video:
        args.enable_cameras = True
    launcher = AppLauncher(args)

    import gymnasium as gym
    import torch

    import biped_tasks.tasks  # noqa: F401  (task registry)
    from biped_tasks.utils.cleanrl.ppo import PPO
    from h12env.export import deploy_config as get_deploy_config
    from isaaclab.utils.dict import print_dict
    from isaaclab.utils.io import dump_pickle, dump_yaml
    from isaaclab_tasks.utils import get_checkpoint_path
    from isaaclab_tasks.utils.hydra import apply_overrides
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    env_cfg = load_cfg_from_registry(args.task, "env_cfg_entry_point")
    agent_cfg = load_cfg_from_registry(args.task, "clean_rl_cfg_entry_point")
    apply_overrides(env_cfg, agent_cfg, hydra_args)
    agent_cfg = update_clean_rl_cfg(agent_cfg, args)
    if args.num_envs is not None:
        env_cfg.scene.num_envs = args.num_envs
    if args.num_iterations is not None:
        agent_cfg.num_iterations = args.num_iterations
    env_cfg.seed = agent_cfg.seed
    if args.device is not None:
        env_cfg.sim.device = args.device
    torch.manual_seed(agent_cfg.seed)

    log_root_path = os.path.abspath(os.path.join("logs", "clean_rl", agent_cfg.experiment_name))
    print(f"[INFO] Logging experiment in directory: {log_root_path}")
    resume_path = None
    if getattr(agent_cfg, "resume", False):  # looked up before this run's directory exists
        resume_path = get_checkpoint_path(log_root_path, agent_cfg.load_run, agent_cfg.load_checkpoint)
        print(f"[INFO]: Loading model checkpoint from: {resume_path}")
    log_dir = os.path.join(log_root_path, datetime.now().strftime("%Y-%m-%d_%H-%M-%S"))

    dump_yaml(os.path.join(log_dir, "params", "env.yaml"), env_cfg)
    dump_yaml(os.path.join(log_dir, "params", "agent.yaml"), agent_cfg)
    dump_pickle(os.path.join(log_dir, "params", "env.pkl"), env_cfg)
    dump_pickle(os.path.join(log_dir, "params", "agent.pkl"), agent_cfg)
    dump_yaml(os.path.join(log_dir, "params", "deploy_config.yaml"), get_deploy_config(env_cfg))

    env = gym.make(args.task, cfg=env_cfg, render_mode="rgb_array" if args.video else None)
    if args.video:
        vk = {"video_folder": os.path.join(log_dir, "videos_train"),
              "step_trigger": lambda s: s % args.video_interval == 0, "video_length": args.video_length,
              "disable_logger": True}
        print("[INFO] Recording videos during training.")
        print_dict(vk, nesting=4)
        env = gym.wrappers.RecordVideo(env, **vk)

    PPO(env, agent_cfg, log_dir, resume_path=resume_path, fused_loss=True if args.fused_loss else None,
        fused_optimizer=True if args.fused_optimizer else None)
    env.close()
    launcher.app.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
