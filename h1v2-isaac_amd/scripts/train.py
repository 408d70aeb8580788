#!/usr/bin/env python3
"""PPO training of an H1-2 velocity task on the MI355X env, and (--distill) distillation of a trained policy into a
student that reads only what the robot measures.

Command line, configuration sources and log artefacts follow the reference's scripts/rsl_rl/train.py
(+ cli_args.py): task / num_envs / seed / max_iterations / experiment_name / run_name / resume /
load_run / checkpoint / logger flags, AppLauncher flags, Hydra-style ``env.*=`` / ``agent.*=``
overrides; runs land in logs/rsl_rl/<experiment>/<timestamp>[_<run>]/ with params/{env,agent}.{yaml,pkl},
metrics.jsonl and model_<it>.pt.  Everything is resolved through the same import surface the reference
script uses (h1v2-isaac_amd/shims), i.e. this is that call sequence exercised on this stack.

Multi-GPU (one rank per GPU):
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py --distributed ...
Each rank steps its own env shard (global env ids rank*num_envs ...), the rollout is all-gathered over
RCCL and every rank applies the identical PPO update (h12env.ppo).
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


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Train an RL agent with RSL-RL-style PPO on the MI355X env.")
    ap.add_argument("--video", action="store_true", default=False)
    ap.add_argument("--video_length", type=int, default=200)
    ap.add_argument("--video_interval", type=int, default=2000)
    ap.add_argument("--num_envs", type=int, default=None, help="envs per rank")
    ap.add_argument("--task", type=str, default="Isaac-Velocity-Flat-H12_12dof-v0")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--max_iterations", type=int, default=None)
    ap.add_argument("--terrain", type=str, default="project", choices=["project", "isaaclab_rough"],
                    help="terrain of a terrain task: its own (project: one noise type, 0-2 cm) or the reference's Rough mix "
                         "(isaaclab_rough: upstream ROUGH_TERRAINS_CFG, h12env.cfg.isaaclab_rough_terrains_cfg); "
                         "env.scene.terrain.terrain_generator.* overrides reach either; refused on plane tasks")
    rl = ap.add_argument_group("rsl_rl")
    rl.add_argument("--experiment_name", type=str, default=None)
    rl.add_argument("--run_name", type=str, default=None)
    rl.add_argument("--resume", type=bool, default=None)
    rl.add_argument("--load_run", type=str, default=None)
    rl.add_argument("--checkpoint", type=str, default=None)
    rl.add_argument("--logger", type=str, default=None, choices={"wandb", "tensorboard", "neptune"})
    rl.add_argument("--log_project_name", type=str, default=None)
    sym = ap.add_argument_group("symmetry", "rsl_rl's symmetry_cfg with the env's own mirror map (h12env.symmetry)")
    sym.add_argument("--symmetry", type=str, default=None, choices=["augment", "mirror_loss", "both"],
                     help="mirror-image data augmentation, the mirror loss, or both "
                          "(fills agent.algorithm.symmetry_cfg; an agent.algorithm.symmetry_cfg=... override works too)")
    sym.add_argument("--mirror_loss_coeff", type=float, default=None, help="weight of the mirror loss (default 1.0)")
    ap.add_argument("--privileged_critic", action="store_true", default=False,
                    help="asymmetric actor-critic: the env also returns the noise-free privileged observation group "
                         "\"critic\" (env.observations.critic = CriticObsCfg(), h12env.priv) and the critic reads it")
    ap.add_argument("--recurrent", action="store_true", default=False,
                    help="train rsl_rl's ActorCriticRecurrent (an LSTM memory in front of the actor and critic MLPs, whose "
                         "hidden dims stay the task's); agent.policy.class_name=ActorCriticRecurrent works too, and with "
                         "this flag agent.policy.rnn_type / rnn_hidden_dim / rnn_num_layers can be overridden")
    ap.add_argument("--fused_learner", action="store_true", default=False,
                    help="the PPO update's actor and critic on the fused HIP forward / backward "
                         "(h12env.policy.TrainableFusedMLP; agent.algorithm.fused_learner=true works too)")
    ap.add_argument("--fused_rnn_update", action="store_true", default=False,
                    help="with --recurrent: the update's memories in the sequence form on the h12learn_lstm_seq_* kernels "
                         "(h12env.recurrent.lstm_sequence; agent.algorithm.fused_rnn_update=true works too)")
    ap.add_argument("--fused_loss", action="store_true", default=False,
                    help="the PPO update's loss head (gathers, losses, gradients, KL schedule) as one fused HIP call "
                         "(h12env.ppo_head.PPOHead; agent.algorithm.fused_loss=true works too)")
    ap.add_argument("--fused_optimizer", action="store_true", default=False,
                    help="the PPO update's gradient clip and Adam step as two fused HIP launches "
                         "(h12env.optim.FusedClipAdam; agent.algorithm.fused_optimizer=true works too)")
    rnd = ap.add_argument_group("rnd", "rsl_rl's rnd_cfg: Random Network Distillation, an exploration bonus (h12env.rnd)")
    rnd.add_argument("--rnd", action="store_true", default=False,
                     help="add RND's intrinsic reward: sets env.observations.rnd_state (the defaults of RndStateObsCfg) and "
                          "agent.algorithm.rnd_cfg (RslRlRndCfg defaults; agent.algorithm.rnd_cfg.* can be overridden)")
    rnd.add_argument("--rnd_weight", type=float, default=None,
                     help="rnd_cfg.weight before the runner's step_dt factor (default 1.0 with --rnd)")
    rnd.add_argument("--rnd_fused", action="store_true", default=False,
                     help="with --rnd: the per-env-step reward work on the h12learn_rnd_* kernels (h12env.rnd.FusedRND; "
                          "agent.algorithm.rnd_cfg.fused=true works too)")
    ds = ap.add_argument_group("distillation", "rsl_rl's Distillation: a student on the deployable observation group "
                               "(h12env.student) copies a PPO-trained teacher (h12env.distill)")
    ds.add_argument("--distill", action="store_true", default=False,
                    help="train a student by distillation: sets env.observations.student, swaps the agent's policy / "
                         "algorithm sections for StudentTeacher / Distillation and loads --teacher_checkpoint; with "
                         "--resume it continues a student run instead")
    ds.add_argument("--teacher_checkpoint", type=str, default=None,
                    help="model_<it>.pt of the PPO run whose actor is the teacher (same task, same policy sizes)")
    ds.add_argument("--student_recurrent", action="store_true", default=False,
                    help="StudentTeacherRecurrent: an LSTM memory in front of the student (agent.policy.rnn_* can be "
                         "overridden); --fused_rnn_update runs its update on the h12learn_lstm_seq_* kernels")
    ds.add_argument("--student_history", type=int, default=None,
                    help="frames of history in the student's observation row (1 .. 10, default 1)")
    AppLauncher.add_app_launcher_args(ap)
    return ap


def make_distillation(agent_cfg, env_cfg, args):
    """--distill: the student observation group on the env cfg; the task's agent cfg with its policy section as a
    StudentTeacher(Recurrent) cfg (teacher and student take the task's actor sizes and activation) and its algorithm
    section as a Distillation cfg (the task's learning rate).  A recurrent teacher checkpoint says so itself: the
    memory's type and size are read from it.  With --resume and no teacher checkpoint the student checkpoint that will
    be resumed describes the run: network sizes, memories (a recurrent teacher's too) and the history length are read
    from it (distill.cfg_from_checkpoint), and the observation group from the run's params/env.yaml."""
    from h12env.cfg import enable_student_observations
    from isaaclab_rl.rsl_rl import (RslRlDistillationAlgorithmCfg, RslRlDistillationStudentTeacherCfg,
                                    RslRlDistillationStudentTeacherRecurrentCfg)

    for flag in ("symmetry", "fused_learner", "fused_loss", "fused_optimizer", "recurrent", "rnd", "rnd_fused"):
        if getattr(args, flag, None):
            raise SystemExit(f"--distill does not take --{flag} (a PPO option; the student's memory is --student_recurrent)")
    if not args.teacher_checkpoint and not args.resume:
        raise SystemExit("--distill needs --teacher_checkpoint PATH (or --resume of a student run)")
    old = agent_cfg.policy
    if args.resume and not args.teacher_checkpoint:
        import torch

        from h12env.distill import cfg_from_checkpoint, is_student_checkpoint, student_group_from_run
        from isaaclab_tasks.utils import get_checkpoint_path

        root = os.path.abspath(os.path.join("logs", "rsl_rl", args.experiment_name or agent_cfg.experiment_name))
        path = get_checkpoint_path(root, args.load_run or agent_cfg.load_run, args.checkpoint or agent_cfg.load_checkpoint)
        keys = torch.load(path, map_location="cpu", weights_only=True)["model_state_dict"]
        if not is_student_checkpoint(keys):
            raise SystemExit(f"--distill --resume: {path} is not a student checkpoint (pass a PPO checkpoint as "
                             "--teacher_checkpoint instead)")
        policy, history = cfg_from_checkpoint(keys, old.activation)
        if args.student_history not in (None, history):
            raise SystemExit(f"--student_history {args.student_history}: the run being resumed has {history}")
        env_cfg.observations.student = student_group_from_run(os.path.dirname(path), history)
        recurrent = policy.pop("class_name") == "StudentTeacherRecurrent"
        cls = RslRlDistillationStudentTeacherRecurrentCfg if recurrent else RslRlDistillationStudentTeacherCfg
        agent_cfg.policy = cls(**policy)
        agent_cfg.algorithm = RslRlDistillationAlgorithmCfg(learning_rate=agent_cfg.algorithm.learning_rate)
        return
    enable_student_observations(env_cfg, args.student_history)
    kw = {"student_hidden_dims": list(old.actor_hidden_dims), "teacher_hidden_dims": list(old.actor_hidden_dims),
          "activation": old.activation, "noise_std_type": old.noise_std_type}
    if args.teacher_checkpoint:
        import torch

        keys = torch.load(args.teacher_checkpoint, map_location="cpu", weights_only=True)["model_state_dict"]
        if "memory_a.rnn.weight_ih_l0" in keys:
            if not args.student_recurrent:
                raise SystemExit("--teacher_checkpoint is a recurrent policy: distil it with --student_recurrent")
            w_ih, w_hh = keys["memory_a.rnn.weight_ih_l0"], keys["memory_a.rnn.weight_hh_l0"]
            kw.update(teacher_recurrent=True, rnn_hidden_dim=w_hh.shape[1],
                      rnn_type="lstm" if w_ih.shape[0] == 4 * w_hh.shape[1] else "gru",
                      rnn_num_layers=len([k for k in keys if k.startswith("memory_a.rnn.weight_ih_l")]))
    cls = RslRlDistillationStudentTeacherRecurrentCfg if args.student_recurrent else RslRlDistillationStudentTeacherCfg
    agent_cfg.policy = cls(**kw)
    agent_cfg.algorithm = RslRlDistillationAlgorithmCfg(learning_rate=agent_cfg.algorithm.learning_rate)


def make_recurrent(agent_cfg):
    """--recurrent: the task's policy cfg as an RslRlPpoActorCriticRecurrentCfg, its other fields kept."""
    import dataclasses

    from isaaclab_rl.rsl_rl import RslRlPpoActorCriticRecurrentCfg

    if not isinstance(agent_cfg.policy, RslRlPpoActorCriticRecurrentCfg):
        kept = {f.name: getattr(agent_cfg.policy, f.name) for f in dataclasses.fields(agent_cfg.policy)
                if f.name != "class_name"}
        agent_cfg.policy = RslRlPpoActorCriticRecurrentCfg(**kept)


def make_rnd(agent_cfg, args):
    """--rnd: agent.algorithm.rnd_cfg as an RslRlRndCfg with --rnd_weight, unless the task's cfg already has one."""
    from isaaclab_rl.rsl_rl import RslRlRndCfg

    if agent_cfg.algorithm.rnd_cfg is None:
        agent_cfg.algorithm.rnd_cfg = RslRlRndCfg(weight=1.0 if args.rnd_weight is None else args.rnd_weight)
    elif args.rnd_weight is not None:
        r = agent_cfg.algorithm.rnd_cfg
        if isinstance(r, dict):
            r["weight"] = args.rnd_weight
        else:
            r.weight = args.rnd_weight


def apply_cli(agent_cfg, env_cfg, args):
    """cli_args.update_rsl_rl_cfg + the num_envs / seed / device / max_iterations overrides."""
    for flag, attr in (("seed", "seed"), ("resume", "resume"), ("load_run", "load_run"),
                       ("checkpoint", "load_checkpoint"), ("run_name", "run_name"), ("logger", "logger"),
                       ("experiment_name", "experiment_name"), ("max_iterations", "max_iterations")):
        v = getattr(args, flag, None)
        if v is not None:
            setattr(agent_cfg, attr, v)
    if agent_cfg.logger in {"wandb", "neptune"} and args.log_project_name:
        agent_cfg.wandb_project = agent_cfg.neptune_project = args.log_project_name
    if getattr(args, "symmetry", None) is not None:
        from isaaclab_rl.rsl_rl import RslRlSymmetryCfg

        agent_cfg.algorithm.symmetry_cfg = RslRlSymmetryCfg(
            use_data_augmentation=args.symmetry in ("augment", "both"),
            use_mirror_loss=args.symmetry in ("mirror_loss", "both"),
            mirror_loss_coeff=1.0 if args.mirror_loss_coeff is None else args.mirror_loss_coeff,
            data_augmentation_func="h12env.symmetry:augment")
    elif getattr(args, "mirror_loss_coeff", None) is not None:
        if agent_cfg.algorithm.symmetry_cfg is None:
            raise SystemExit("--mirror_loss_coeff needs --symmetry (or an agent.algorithm.symmetry_cfg override)")
        s = agent_cfg.algorithm.symmetry_cfg
        if isinstance(s, dict):
            s["mirror_loss_coeff"] = args.mirror_loss_coeff
        else:
            s.mirror_loss_coeff = args.mirror_loss_coeff
    if getattr(args, "fused_learner", False):
        agent_cfg.algorithm.fused_learner = True
    if getattr(args, "fused_loss", False):
        agent_cfg.algorithm.fused_loss = True
    if getattr(args, "fused_rnn_update", False):
        agent_cfg.algorithm.fused_rnn_update = True
    if getattr(args, "fused_optimizer", False):
        agent_cfg.algorithm.fused_optimizer = True
    r = getattr(agent_cfg.algorithm, "rnd_cfg", None)
    if getattr(args, "rnd_fused", False):
        if r is None:
            raise SystemExit("--rnd_fused needs --rnd (or an agent.algorithm.rnd_cfg override)")
        if isinstance(r, dict):
            r["fused"] = True
        else:
            r.fused = True
    elif getattr(args, "rnd_weight", None) is not None and r is None:
        raise SystemExit("--rnd_weight needs --rnd (or an agent.algorithm.rnd_cfg override)")
    if r is not None:  # the group RND reads; an env cfg that has set it keeps its terms
        from h12env.cfg import enable_rnd_state

        enable_rnd_state(env_cfg)
    if getattr(args, "privileged_critic", False):
        from h12env.cfg import enable_privileged_critic

        enable_privileged_critic(env_cfg)
    if args.num_envs is not None:
        env_cfg.scene.num_envs = args.num_envs
    env_cfg.seed = agent_cfg.seed
    if args.device is not None:
        env_cfg.sim.device = args.device
        agent_cfg.device = args.device


def run_dir(agent_cfg) -> tuple[str, str]:
    root = os.path.abspath(os.path.join("logs", "rsl_rl", agent_cfg.experiment_name))
    name = datetime.now().strftime("%Y-%m-%d_%H-%M-%S") + (f"_{agent_cfg.run_name}" if agent_cfg.run_name else "")
    return root, os.path.join(root, name)


def main(argv=None) -> int:
    args, hydra_args = build_parser().parse_known_args(argv)
    if args.video:
        args.enable_cameras = True
    launcher = AppLauncher(args)

    import gymnasium as gym
    import torch
    import torch.distributed as dist

    import biped_tasks.tasks  # noqa: F401  (task registry)
    from isaaclab.utils.dict import print_dict
    from isaaclab.utils.io import dump_pickle, dump_yaml
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from isaaclab_tasks.utils import get_checkpoint_path
    from isaaclab_tasks.utils.hydra import apply_overrides
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    env_cfg = load_cfg_from_registry(args.task, "env_cfg_entry_point")
    agent_cfg = load_cfg_from_registry(args.task, "rsl_rl_cfg_entry_point")
    from h12env.cfg import apply_terrain_choice

    apply_terrain_choice(env_cfg, args.terrain)  # before the overrides, so that ...terrain_generator.sub_terrains.* exist
    if args.distill:  # before the overrides, so that agent.algorithm.gradient_length etc. exist for them
        make_distillation(agent_cfg, env_cfg, args)
    elif args.recurrent:  # before the overrides, so that agent.policy.rnn_* exist for them
        make_recurrent(agent_cfg)
    if args.rnd and not args.distill:  # before the overrides, so that agent.algorithm.rnd_cfg.* exist for them
        make_rnd(agent_cfg, args)
    apply_overrides(env_cfg, agent_cfg, hydra_args)
    apply_cli(agent_cfg, env_cfg, args)
    rank = dist.get_rank() if dist.is_initialized() else 0

    root, log_dir = run_dir(agent_cfg)
    if rank == 0:
        print(f"[INFO] Logging experiment in directory: {root}")
    make_kw = {"cfg": env_cfg, "render_mode": "rgb_array" if args.video else None}
    if dist.is_initialized():
        make_kw["env_offset"] = rank * int(env_cfg.scene.num_envs)
    env = gym.make(args.task, **make_kw)
    if args.video:
        vk = {"video_folder": os.path.join(log_dir, "videos", "train"),
              "step_trigger": lambda s: s % args.video_interval == 0, "video_length": args.video_length}
        print_dict(vk, nesting=4)
        env = gym.wrappers.RecordVideo(env, **vk)
    env = RslRlVecEnvWrapper(env)
    runner = OnPolicyRunner(env, agent_cfg.to_dict(), log_dir=log_dir if rank == 0 else None, device=agent_cfg.device)
    runner.add_git_repo_to_log(__file__)
    if agent_cfg.resume:
        path = get_checkpoint_path(root, agent_cfg.load_run, agent_cfg.load_checkpoint)
        print(f"[INFO]: Loading model checkpoint from: {path}")
        runner.load(path)
    elif args.distill:  # a PPO checkpoint: its actor becomes the teacher, the student starts at iteration 0
        print(f"[INFO]: Loading the teacher from: {args.teacher_checkpoint}")
        runner.load(args.teacher_checkpoint)
    if rank == 0:
        for name, obj in (("env", env_cfg), ("agent", agent_cfg)):
            dump_yaml(os.path.join(log_dir, "params", f"{name}.yaml"), obj)
            dump_pickle(os.path.join(log_dir, "params", f"{name}.pkl"), obj)
    runner.learn(num_learning_iterations=agent_cfg.max_iterations, init_at_random_ep_len=True)
    env.close()
    launcher.app.close()
    del torch
    return 0


if __name__ == "__main__":
    sys.exit(main())
