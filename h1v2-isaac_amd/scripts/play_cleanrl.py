#!/usr/bin/env python3
"""Play a CleanRL PPO checkpoint on a CaT *-Play-v0 task and export it (the reference's scripts/clean_rl/play.py
flow): load model_*.pt (the agent's state_dict) through get_checkpoint_path, write <run>/exported/policy.pt
(TorchScript of Agent.forward: observation normaliser + deterministic actor; ONNX is skipped with a message when
the onnx package is absent), then step the task with deterministic actions for --video_length steps.

    python play_cleanrl.py --task Isaac-Velocity-CaT-Flat-H12_12dof-Play-v0 [--load_run <run>] [--checkpoint model_.*.pt]
"""
from __future__ import annotations

import argparse
import copy
import os
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
PKG = HERE.parent
for p in (PKG / "shims", PKG, HERE):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

from isaaclab.app import AppLauncher  # noqa: E402
from train_cleanrl import add_clean_rl_args, update_clean_rl_cfg  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Play an RL agent with CleanRL.")
    ap.add_argument("--video", action="store_true", default=False)
    ap.add_argument("--video_length", type=int, default=200, help="env steps to play")
    ap.add_argument("--disable_fabric", action="store_true", default=False)
    ap.add_argument("--num_envs", type=int, default=None)
    ap.add_argument("--task", type=str, default="Isaac-Velocity-CaT-Flat-H12_12dof-Play-v0")
    ap.add_argument("--fused", action="store_true", default=False,
                    help="run the policy as one fused HIP launch (h12env.policy.FusedMLP) instead of torch modules")
    add_clean_rl_args(ap)
    AppLauncher.add_app_launcher_args(ap)
    return ap


def export_agent(agent, n_obs: int, out_dir: str) -> str:
    """<out_dir>/policy.pt: TorchScript trace of Agent.forward on CPU (+ policy.onnx when onnx is installed)."""
    import torch

    os.makedirs(out_dir, exist_ok=True)
    actor = copy.deepcopy(agent).cpu().eval()
    dummy = torch.randn(1, n_obs)
    pt_path = os.path.join(out_dir, "policy.pt")
    with torch.no_grad():
        torch.jit.trace(actor, dummy).save(pt_path)
    print(f"[INFO] Exported .pt model to {pt_path}")
    try:
        import onnx  # noqa: F401  (torch's exporter serialises through it)
    except ImportError as e:
        print(f"[INFO]: skipping ONNX export ({e})")
    else:
        onnx_path = os.path.join(out_dir, "policy.onnx")
        torch.onnx.export(actor, dummy, onnx_path, export_params=True, opset_version=16, do_constant_folding=True,
                          input_names=["input"], output_names=["output"], dynamo=False)
        print(f"[INFO] Exported ONNX model to {onnx_path}")
    return pt_path


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    launcher = AppLauncher(args)

    import gymnasium as gym
    import torch

    import biped_tasks.tasks  # noqa: F401
    from biped_tasks.utils.cleanrl.ppo import Agent
    from isaaclab_tasks.utils import get_checkpoint_path, parse_env_cfg
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    kw = {"num_envs": args.num_envs}
    if args.device is not None:
        kw["device"] = args.device
    env_cfg = parse_env_cfg(args.task, **kw)
    agent_cfg = update_clean_rl_cfg(load_cfg_from_registry(args.task, "clean_rl_cfg_entry_point"), args)

    log_root_path = os.path.abspath(os.path.join("logs", "clean_rl", agent_cfg.experiment_name))
    print(f"[INFO] Loading experiment from directory: {log_root_path}")
    resume_path = get_checkpoint_path(log_root_path, agent_cfg.load_run, agent_cfg.load_checkpoint)
    print(f"[INFO] Loading model: {resume_path}")
    log_dir = os.path.dirname(resume_path)

    env = gym.make(args.task, cfg=env_cfg, render_mode="rgb_array" if args.video else None)
    if args.video:
        env = gym.wrappers.RecordVideo(env, video_folder=os.path.join(log_dir, "videos_play"),
                                       step_trigger=lambda s: s == 0, video_length=args.video_length,
                                       disable_logger=True)
    device = torch.device(env.unwrapped.device)
    actor = Agent(env).to(device)
    actor.load_state_dict(torch.load(resume_path, map_location=device, weights_only=True))
    actor.eval()

    obs = env.reset()[0]["policy"]
    export_agent(actor, obs.shape[-1], os.path.join(log_dir, "exported"))

    fused = actor.inference_policy(fused=True) if args.fused else None
    for _ in range(args.video_length):
        with torch.no_grad():
            if fused is not None:
                actions = fused(obs)
            else:
                actions, _, _, _ = actor.get_action_and_value(actor.obs_rms(obs, update=False), deterministic=True)
        next_obs, rewards, next_done, timeouts, info = env.step(actions)
        obs = next_obs["policy"]
    env.close()
    launcher.app.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
