#!/usr/bin/env python3
"""Play a trained checkpoint on the *-Play-v0 task and export it for deployment (the reference's
scripts/rsl_rl/play.py flow): <run>/exported/{policy.pt, env.yaml} (+ policy.onnx when the onnx package
is installed), then roll the policy out for --steps env steps.

    python play.py --task Isaac-Velocity-Flat-H12_12dof-Play-v0 --load_run <run dir name> [--checkpoint model_.*.pt]
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
PKG = HERE.parent
for p in (PKG / "shims", PKG):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="Isaac-Velocity-Flat-H12_12dof-Play-v0")
    ap.add_argument("--num_envs", type=int, default=None)
    ap.add_argument("--experiment_name", default=None)
    ap.add_argument("--load_run", default=".*")
    ap.add_argument("--checkpoint", default="model_.*.pt")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--fused", action="store_true",
                    help="run the policy as one fused HIP launch (h12env.policy.FusedMLP, or RecurrentPolicy for a "
                         "recurrent checkpoint) instead of torch modules")
    ap.add_argument("--privileged_critic", action="store_true", default=False,
                    help="the checkpoint was trained with train.py --privileged_critic (its critic reads the "
                         "privileged observation group)")
    ap.add_argument("--terrain", default="project", choices=["project", "isaaclab_rough"],
                    help="terrain of a terrain task for a run whose params/env.yaml does not say: a run trained with "
                         "train.py --terrain isaaclab_rough plays on that mix without this flag; refused on plane tasks")
    ap.add_argument("--video", action="store_true", default=False, help="Record a video of the rollout.")
    ap.add_argument("--video_length", type=int, default=200, help="Length of the recorded video (in steps).")
    args = ap.parse_args(argv)

    import gymnasium as gym
    import torch

    import biped_tasks.tasks  # noqa: F401
    from h12env.export import export_policy_as_jit, export_policy_as_onnx, write_env_yaml
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from isaaclab_tasks.utils import get_checkpoint_path
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    env_cfg = load_cfg_from_registry(args.task, "env_cfg_entry_point")
    agent_cfg = load_cfg_from_registry(args.task, "rsl_rl_cfg_entry_point")
    if args.num_envs:
        env_cfg.scene.num_envs = args.num_envs
    if args.privileged_critic:
        from h12env.cfg import enable_privileged_critic

        enable_privileged_critic(env_cfg)
    env_cfg.sim.device = agent_cfg.device = args.device
    from h12env.cfg import apply_terrain_choice, terrain_from_run

    apply_terrain_choice(env_cfg, args.terrain)
    root = os.path.abspath(os.path.join("logs", "rsl_rl", args.experiment_name or agent_cfg.experiment_name))
    path = get_checkpoint_path(root, args.load_run, args.checkpoint)
    print(f"[INFO]: Loading model checkpoint from: {path}")
    if terrain_from_run(env_cfg, os.path.dirname(path)):  # the run's own sub-terrain mix, read from its cfg
        print("[INFO]: playing on the run's sub-terrain mix: "
              + ", ".join(env_cfg.scene.terrain.terrain_generator.sub_terrains))
    # a recurrent checkpoint (train.py --recurrent) says so itself: the memory's type and size are read from it
    keys = torch.load(path, map_location="cpu", weights_only=True)["model_state_dict"]
    # a distilled student (train.py --distill) says so too: it has student.* parameters.  The env then returns the
    # student observation group with the history the student was trained on, and the student is what plays
    from h12env.distill import StudentView, cfg_from_checkpoint, is_student_checkpoint, student_group_from_run

    student = is_student_checkpoint(keys)
    student_policy = None
    if student:
        from isaaclab_rl.rsl_rl import RslRlDistillationAlgorithmCfg

        student_policy, history = cfg_from_checkpoint(keys, agent_cfg.policy.activation)
        # the group as the run trained on it (history, per-term scales: params/env.yaml of the run), and, as the Play
        # tasks do for their policy group, without corruption
        env_cfg.observations.student = student_group_from_run(os.path.dirname(path), history)
        env_cfg.observations.student.enable_corruption = False
        agent_cfg.algorithm = RslRlDistillationAlgorithmCfg()
    recurrent = "memory_a.rnn.weight_ih_l0" in keys or (student and student_policy["class_name"].endswith("Recurrent"))
    if recurrent and not student:
        w_ih, w_hh = keys["memory_a.rnn.weight_ih_l0"], keys["memory_a.rnn.weight_hh_l0"]
        agent_cfg.policy.class_name = "ActorCriticRecurrent"
        rnn = {"rnn_type": "lstm" if w_ih.shape[0] == 4 * w_hh.shape[1] else "gru", "rnn_hidden_dim": w_hh.shape[1],
               "rnn_num_layers": len([k for k in keys if k.startswith("memory_a.rnn.weight_ih_l")])}
    env = gym.make(args.task, cfg=env_cfg, render_mode="rgb_array" if args.video else None)
    if args.video:  # the reference's play.py: one video from step 0 under <run>/videos/play
        vk = {"video_folder": os.path.join(os.path.dirname(path), "videos", "play"),
              "step_trigger": lambda step: step == 0, "video_length": args.video_length, "disable_logger": True}
        print("[INFO] Recording videos during training.")
        env = gym.wrappers.RecordVideo(env, **vk)
    env = RslRlVecEnvWrapper(env)
    train_cfg = agent_cfg.to_dict()
    if student:
        train_cfg["policy"] = student_policy
    elif recurrent:
        train_cfg["policy"].update(rnn)
    runner = OnPolicyRunner(env, train_cfg, log_dir=None, device=args.device)
    runner.load(path)
    policy = runner.get_inference_policy(device=args.device, fused=args.fused)
    out = os.path.join(os.path.dirname(path), "exported")
    exported = StudentView(runner.alg.policy) if student else runner.alg.policy
    export_policy_as_jit(exported, runner.obs_normalizer, out, "policy.pt")
    write_env_yaml(env_cfg, os.path.join(out, "env.yaml"), group="student" if student else "policy")
    try:
        export_policy_as_onnx(exported, runner.obs_normalizer, out, "policy.onnx")
    except (ImportError, NotImplementedError) as e:
        print(f"[INFO]: skipping ONNX export ({e})")
    print(f"[INFO]: exported to {out}")
    # what the policy reads: the actor's row, or for a student its own observation group
    pick = (lambda obs, extras: extras["observations"]["student"]) if student else (lambda obs, extras: obs)
    obs = pick(*env.get_observations())
    with torch.inference_mode():
        for timestep in range(1, args.steps + 1):
            obs, _, dones, extras = env.step(policy(obs))
            obs = pick(obs, extras)
            if recurrent:  # forget the episodes that ended
                (policy if args.fused else runner.alg.policy).reset(dones)
            if args.video and timestep == args.video_length:  # exit the play loop after recording one video
                break
    env.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
