#!/usr/bin/env python3
"""Measure the CleanRL PPO collection on the CaT task: fused HIP normaliser + GAE against H12_CLEANRL_FUSED=0.

    python tools/probe/cleanrl_collect.py [--num_envs 4096] [--steps 24] [--rounds 4] [--iters 5] [--out FILE]
    python tools/probe/cleanrl_collect.py --mode rocprof [--out FILE]

time (default): the two arms alternate in one process on one env (arm A fused, arm B torch, A, B, ...); each
turn is one PPO() call of 1 + iters iterations whose first iteration (graph capture, allocator warm-up) is
dropped.  PPO's own per-iteration figures are used: Perf/collection_time ends on a host transfer of the episode
statistics and the iteration ends on the transfer of the loss sums, so both are synchronised.  Reported:
collection ms / iteration and whole-iteration ms, median and min per arm.
rocprof: starts `rocprofv3 --kernel-trace --stats -- python <this file> --mode short` as a child process (this
process never opens the GPU) and reports calls / average / min / max of the new kernels from its stats CSV.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
PKG = ROOT / "h1v2-isaac_amd"
TASK = "Isaac-Velocity-CaT-Flat-H12_12dof-v0"
KERNELS = ("rms_stats_kernel", "rms_normalise_kernel", "gae_soft_kernel")


def _paths():
    for p in (PKG / "shims", PKG):
        if str(p) not in sys.path:
            sys.path.insert(0, str(p))


def make_env(num_envs: int):
    _paths()
    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    cfg = load_cfg_from_registry(TASK, "env_cfg_entry_point")
    cfg.scene.num_envs = num_envs
    cfg.sim.device = "cuda:0"
    cfg.seed = 1
    return gym.make(TASK, cfg=cfg)


def run_arm(env, fused: bool, steps: int, iters: int, tmp: str):
    import torch
    from biped_tasks.tasks.agents import H12_12dof_FlatCleanRlPPOCfg
    from h12env import cleanrl

    os.environ["H12_CLEANRL_FUSED"] = "1" if fused else "0"
    cfg = H12_12dof_FlatCleanRlPPOCfg(num_steps=steps, num_iterations=1 + iters, save_interval=10 ** 9)
    cfg.minibatch_size = min(cfg.minibatch_size, steps * env.unwrapped.num_envs)
    run = tempfile.mkdtemp(dir=tmp)
    torch.manual_seed(1)
    cleanrl.PPO(env, cfg, run)
    torch.cuda.synchronize()
    lines = [json.loads(x) for x in open(os.path.join(run, "metrics.jsonl"))][1:]
    return ([1e3 * x["Perf/collection_time"] for x in lines],
            [1e3 * (x["Perf/collection_time"] + x["Perf/learning_time"]) for x in lines])


def mode_time(a):
    env = make_env(a.num_envs)
    res = {"fused": ([], []), "torch": ([], [])}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(a.rounds):
            for arm in ("fused", "torch"):
                c, w = run_arm(env, arm == "fused", a.steps, a.iters, tmp)
                res[arm][0].extend(c)
                res[arm][1].extend(w)
    env.close()
    out = {"task": TASK, "num_envs": a.num_envs, "steps": a.steps, "iterations_per_arm": a.rounds * a.iters,
           "graph": os.environ.get("H12_PPO_GRAPH", "1")}
    for arm, (c, w) in res.items():
        out[arm] = {"collection_ms_median": statistics.median(c), "collection_ms_min": min(c),
                    "iteration_ms_median": statistics.median(w), "iteration_ms_min": min(w),
                    "timed_s": sum(w) / 1e3}
    return out


def mode_short(a):
    env = make_env(a.num_envs)
    with tempfile.TemporaryDirectory() as tmp:
        run_arm(env, True, a.steps, 3, tmp)
    env.close()
    return {"ok": True}


def mode_rocprof(a):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
               str(Path(__file__).resolve()), "--mode", "short", "--num_envs", str(a.num_envs), "--steps", str(a.steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(files[0])))
    out = {"command": "rocprofv3 --kernel-trace --stats -- python tools/probe/cleanrl_collect.py --mode short",
           "num_envs": a.num_envs, "steps": a.steps, "kernels": {}}
    for row in rows:
        for k in KERNELS:
            if k in row["Name"]:
                out["kernels"][k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                     "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("time", "short", "rocprof"), default="time")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    out = {"time": mode_time, "short": mode_short, "rocprof": mode_rocprof}[a.mode](a)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
