#!/usr/bin/env python3
"""Batched policy evaluation with the on-device safety monitor: the sim2sim loop (scripts/sim2sim.py) for N envs with
every 1 kHz physics substep of every env recorded by h12env.safety.SafetyMonitor, then the three tables of the
reference's biped_deploy/eval/eval_policy.py over the whole batch -- average action rate per joint, average / maximum
foot force, position violations per joint -- and the share of envs with any violation.

    python eval_policy.py <policy_dir> [--num_envs 4096] [--episode_length 5] [--command 0.5 0 0 | --command_grid]
                          [--trace_envs k] [--fused] [--log_dir out]

--command_grid spreads a 3 x 3 x 3 grid of deploy-convention commands ({-1, 0, 1} per axis) over the envs.  --log_dir
receives eval.json and, for each traced env i < k, env_<i>/metrics.json (MJLogger schema at physics rate, with the real
torques and foot forces) and env_<i>/safety_check.json (SafetyChecker's violations of that file).
"""
from __future__ import annotations

import argparse
import itertools
import json
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))


def _grid(rows: list, headers: list) -> str:
    """A plain grid table (the reference prints tabulate's "grid" format)."""
    cells = [[str(c) for c in headers]] + [[str(c) for c in r] for r in rows]
    width = [max(len(r[i]) for r in cells) for i in range(len(headers))]
    bar = "+" + "+".join("-" * (w + 2) for w in width) + "+"
    line = lambda r: "| " + " | ".join(c.ljust(w) for c, w in zip(r, width)) + " |"  # noqa: E731
    out = [bar, line(cells[0]), bar.replace("-", "=")]
    for r in cells[1:]:
        out += [line(r), bar]
    return "\n".join(out)


def format_tables(summary: dict, label: str = "batch") -> str:
    """The reference's three tables for one experiment column, from SafetyMonitor.summary()."""
    joints = summary["joints"]
    rate = _grid([[n, f"{d['tau_rate_avg']:.3f}"] for n, d in joints.items()], ["Joint Name", label])
    feet = summary["feet"]
    force_rows = [["Avg Force", f"{summary['force_pair_avg']:.0f}"], ["Max Force", f"{summary['force_pair_max']:.0f}"]]
    force_rows += [[f"Max Force {n}", f"{d['force_max']:.0f}"] for n, d in feet.items()]
    force = _grid(force_rows, ["Metric", label])
    viol = _grid([[n, d["pos_viol_count"]] for n, d in sorted(joints.items()) if d["pos_viol_count"] > 0],
                 ["Joint Name", label])
    share = (f"envs with any violation: {summary['envs_any_viol']} of {summary['num_envs']} "
             f"({100.0 * summary['share_any_viol']:.2f} %; position {summary['envs_pos_viol']}, "
             f"foot force {summary['envs_force_viol']}, velocity {summary['envs_vel_viol']}) "
             f"over {summary['substeps']} env-substeps")
    return (f"Avg Action Rate:\n{rate}\n\nAvg Force and Max Force:\n{force}\n\nPosition Violations:\n{viol}\n\n{share}")


def write_eval(log_dir, summary: dict, run: dict) -> Path:
    """eval.json: the run's arguments and the batch summary."""
    log_dir = Path(log_dir)
    log_dir.mkdir(parents=True, exist_ok=True)
    p = log_dir / "eval.json"
    p.write_text(json.dumps({"run": run, "summary": summary}, indent=2) + "\n")
    return p


def command_grid(num_envs: int):
    import torch

    combos = torch.tensor(list(itertools.product((-1.0, 0.0, 1.0), repeat=3)))
    return combos[torch.arange(num_envs) % combos.shape[0]]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("policy_dir", type=Path)
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--episode_length", type=float, default=5.0, help="seconds")
    ap.add_argument("--command", type=float, nargs=3, default=[0.0, 0.0, 0.0])
    ap.add_argument("--command_grid", action="store_true", help="a 3 x 3 x 3 grid of commands spread over the envs")
    ap.add_argument("--trace_envs", type=int, default=0, help="envs [0, k) also write metrics.json / safety_check.json")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--log_dir", type=Path, default=None)
    ap.add_argument("--fused", action="store_true",
                    help="run policy.pt's actor and normaliser (and memory, when recurrent) as one fused HIP launch "
                         "(h12env.policy.FusedMLP / RecurrentPolicy)")
    ap.add_argument("--privileged_critic", action="store_true", default=False,
                    help="build the env with the privileged critic observation group, as train.py / play.py do with "
                         "this flag (the exported policy is the actor alone: the evaluation itself does not change)")
    ap.add_argument("--terrain", default="project", choices=["project", "isaaclab_rough"],
                    help="as train.py / play.py; the evaluation runs on the plane, which refuses isaaclab_rough")
    args = ap.parse_args(argv)
    if not 0 <= args.trace_envs <= args.num_envs:
        ap.error("--trace_envs must be in 0..num_envs")

    import torch
    import yaml

    from h12env import mujoco_cfg
    from h12env.env import H12VelocityEnv
    from h12env.export import DeployController, env_state
    from h12env.safety import SafetyMonitor, write_env_logs

    pcfg = yaml.safe_load((args.policy_dir / "env.yaml").read_text())
    policy = torch.jit.load(str(args.policy_dir / "policy.pt"), map_location=args.device).eval()
    from h12env.policy import deploy_policy

    policy = deploy_policy(policy, args.num_envs, args.device, fused=args.fused)  # a recurrent export: batched state
    cfg = mujoco_cfg()
    cfg.scene.num_envs = args.num_envs
    cfg.sim.device = args.device
    cfg.decimation = int(round(pcfg["control_dt"] / cfg.sim.dt))
    from h12env.cfg import apply_terrain_choice

    apply_terrain_choice(cfg, args.terrain)
    if args.privileged_critic:
        from h12env.cfg import enable_privileged_critic

        enable_privileged_critic(cfg)
    env = H12VelocityEnv(cfg)
    env.reset()
    mon = SafetyMonitor(env, trace_envs=args.trace_envs)
    ctrl = DeployController(policy, pcfg, args.num_envs, args.device)
    if args.command_grid:
        cmd = command_grid(args.num_envs).to(args.device)
    else:
        cmd = torch.tensor(args.command, device=args.device).expand(args.num_envs, 3)
    steps = int(round(args.episode_length / pcfg["control_dt"]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        q_ref = ctrl(env_state(env), cmd)
        env.step_physics(q_ref, cfg.decimation, monitor=mon)
    summary = mon.summary()  # synchronises
    wall = time.perf_counter() - t0
    rate = args.num_envs * steps * cfg.decimation / wall
    print(f"[eval_policy] {args.num_envs} envs x {steps} control steps x {cfg.decimation} substeps in {wall:.2f} s "
          f"({rate:.3e} env-substeps/s)")
    print(format_tables(summary))
    if args.log_dir:
        run = {"policy_dir": str(args.policy_dir), "num_envs": args.num_envs, "control_steps": steps,
               "substeps_per_step": cfg.decimation, "command": "grid" if args.command_grid else list(args.command),
               "trace_envs": args.trace_envs, "fused": bool(args.fused), "wall_s": wall, "env_substeps_per_s": rate}
        print(f"[eval_policy] wrote {write_eval(args.log_dir, summary, run)}")
        for i, metrics in enumerate(mon.trace_metrics()):
            mf, sf = write_env_logs(args.log_dir, i, metrics)
            print(f"[eval_policy] env {i}: {mf}, {sf}")
    env.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
