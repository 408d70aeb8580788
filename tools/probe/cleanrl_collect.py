#!/usr/bin/env python3
"""Measure the CleanRL PPO collection on the CaT task: fused HIP normaliser + GAE against H12_CLEANRL_FUSED=0.

    python tools/probe/cleanrl_collect.py [--num_envs 4096] [--steps 24] [--rounds 4] [--iters 5] [--out FILE]
    python tools/probe/cleanrl_collect.py --mode rocprof [--out FILE]
    python tools/probe/cleanrl_collect.py --mode head [--rounds 4] [--iters 6] [--out FILE]
    python tools/probe/cleanrl_collect.py --mode head_trace --arm default|fused_eager|fused_graphed [--out FILE]
    python tools/probe/cleanrl_collect.py --mode head --arms fused_graphed,fused_graphed+optim [--out FILE]

time (default): the two arms alternate in one process on one env (arm A fused, arm B torch, A, B, ...); each
turn is one PPO() call of 1 + iters iterations whose first iteration (graph capture, allocator warm-up) is
dropped.  PPO's own per-iteration figures are used: Perf/collection_time ends on a host transfer of the episode
statistics and the iteration ends on the transfer of the loss sums, so both are synchronised.  Reported:
collection ms / iteration and whole-iteration ms, median and min per arm.
rocprof: starts `rocprofv3 --kernel-trace --stats -- python <this file> --mode short` as a child process (this
process never opens the GPU) and reports calls / average / min / max of the new kernels from its stats CSV.
head: the update's three arms alternate in one process on one env: ``default`` (the switch off), ``fused_eager``
(fused_loss with H12_PPO_GRAPH=0, which also collects eagerly: compare its learning time, not its iteration) and
``fused_graphed``.  Learning ms and whole-iteration ms per arm: median and minimum over all turns, and the median of
every turn on its own, which is the spread between repeats of one arm.  Every logged loss and every parameter of every
arm is asserted finite.
head_trace: one arm under `rocprofv3 --kernel-trace --stats` in a child process; the update's dispatches (from an
iteration's GAE kernel to the next env step) per minibatch, split into GEMMs, ELU, optimiser and gradient clip (the
multi-tensor kernels and the capturable optimiser's scalar kernels on 0-dim tensors are in the rest), the head's
kernels, the fused optimiser step's two kernels and the rest.
The arms ``default+optim`` and ``fused_graphed+optim`` are ``default`` and ``fused_graphed`` with ``fused_optimizer`` on
(h12env.optim.FusedClipRAdam); ``--arms`` picks the arms ``head`` alternates.
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


# arm -> (fused_loss, H12_PPO_GRAPH, fused_optimizer)
HEAD_ARMS = {"default": (False, "1", False), "fused_eager": (True, "0", False), "fused_graphed": (True, "1", False),
             "default+optim": (False, "1", True), "fused_graphed+optim": (True, "1", True)}
HEAD_DEFAULT_ARMS = ("default", "fused_eager", "fused_graphed")


def run_head_arm(env, arm: str, steps: int, iters: int, tmp: str):
    import math

    import torch
    from biped_tasks.tasks.agents import H12_12dof_FlatCleanRlPPOCfg
    from h12env import cleanrl

    fused_loss, graph, fused_optimizer = HEAD_ARMS[arm]
    os.environ["H12_CLEANRL_FUSED"] = "1"
    os.environ["H12_PPO_GRAPH"] = graph
    cfg = H12_12dof_FlatCleanRlPPOCfg(num_steps=steps, num_iterations=1 + iters, save_interval=10 ** 9)
    cfg.minibatch_size = min(cfg.minibatch_size, steps * env.unwrapped.num_envs)
    run = tempfile.mkdtemp(dir=tmp)
    torch.manual_seed(1)
    agent = cleanrl.PPO(env, cfg, run, fused_loss=fused_loss, fused_optimizer=fused_optimizer)
    torch.cuda.synchronize()
    all_lines = [json.loads(x) for x in open(os.path.join(run, "metrics.jsonl"))]
    for x in all_lines:
        bad = {k: v for k, v in x.items() if k.startswith("Loss/") and not math.isfinite(v)}
        assert not bad, (arm, x["iter"], bad)
    for k, v in agent.state_dict().items():
        assert bool(torch.isfinite(v).all()), (arm, k)
    lines = all_lines[1:]
    return ([1e3 * x["Perf/learning_time"] for x in lines],
            [1e3 * (x["Perf/collection_time"] + x["Perf/learning_time"]) for x in lines],
            {"minibatch_size": cfg.minibatch_size, "updates_epochs": cfg.updates_epochs})


def mode_head(a):
    env = make_env(a.num_envs)
    arms = tuple(a.arms.split(",")) if a.arms else HEAD_DEFAULT_ARMS
    res = {arm: ([], [], []) for arm in arms}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(a.rounds):
            for arm in arms:
                learn, whole, shape = run_head_arm(env, arm, a.steps, a.iters, tmp)
                res[arm][0].extend(learn)
                res[arm][1].extend(whole)
                res[arm][2].append(statistics.median(learn))
    env.close()
    out = {"task": TASK, "num_envs": a.num_envs, "steps": a.steps, "iterations_per_arm": a.rounds * a.iters,
           "finite": "every logged loss and every parameter, every arm", **shape}
    for arm, (learn, whole, turns) in res.items():
        out[arm] = {"learning_ms_median": statistics.median(learn), "learning_ms_min": min(learn),
                    "iteration_ms_median": statistics.median(whole), "iteration_ms_min": min(whole),
                    "learning_ms_median_per_turn": turns}
    return out


def mode_head_short(a):
    env = make_env(a.num_envs)
    with tempfile.TemporaryDirectory() as tmp:
        _, _, shape = run_head_arm(env, a.arm, a.steps, 2, tmp)
    env.close()
    return {"ok": True, **shape}


def _category(name: str) -> str:
    low = name.lower()
    if "cleanrl_" in low:
        return "head"
    if "optim_norm_kernel" in low or "optim_apply_kernel" in low:
        return "fused_optimiser"
    if "cijk" in low or "gemm" in low:
        return "gemm"
    if "elu" in low:
        return "elu"
    if "multi_tensor" in low:
        return "optimiser_and_clip"
    return "rest"


def mode_head_trace(a):
    iters = 3  # of head_short: 1 + 2
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
               str(Path(__file__).resolve()), "--mode", "head_short", "--arm", a.arm, "--num_envs", str(a.num_envs),
               "--steps", str(a.steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
        shape = json.loads(r.stdout[r.stdout.rindex('{\n "ok"'):])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_trace.csv")
        rows = sorted(csv.DictReader(open(files[0])), key=lambda x: int(x["Start_Timestamp"]))
    # an iteration's update: after its GAE kernel, until the env steps again (the last update runs to the end)
    cats, names, in_update, updates = {}, {}, False, 0
    for row in rows:
        name = row["Kernel_Name"]
        if "gae_soft_kernel" in name:
            in_update, updates = True, updates + 1
            continue
        if "step_kernel" in name:
            in_update = False
        if not in_update:
            continue
        ns = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
        c = cats.setdefault(_category(name), [0, 0])
        c[0] += 1
        c[1] += ns
        n = names.setdefault(name[:96], [0, 0])
        n[0] += 1
        n[1] += ns
    assert updates == iters, updates
    n_mb = updates * shape["updates_epochs"] * -(-a.num_envs * a.steps // shape["minibatch_size"])
    total = sum(c[1] for c in cats.values())
    out = {"command": f"rocprofv3 --kernel-trace --stats -- python tools/probe/cleanrl_collect.py --mode head_short "
                      f"--arm {a.arm}", "arm": a.arm, "num_envs": a.num_envs, "steps": a.steps, **shape,
           "minibatches_traced": n_mb, "launches_per_minibatch": sum(c[0] for c in cats.values()) / n_mb,
           "gpu_us_per_minibatch": total / n_mb / 1e3, "split": {}}
    for k, (calls, ns) in sorted(cats.items()):
        out["split"][k] = {"launches_per_minibatch": calls / n_mb, "gpu_us_per_minibatch": ns / n_mb / 1e3,
                           "share": ns / total}
    by_time = sorted(names.items(), key=lambda kv: -kv[1][1])
    top = by_time[:25] + [kv for kv in by_time[25:] if "optim_" in kv[0]]  # the fused optimiser's two, wherever they rank
    out["kernels"] = {k: {"calls_per_minibatch": c / n_mb, "avg_us": ns / c / 1e3} for k, (c, ns) in top}
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
    ap.add_argument("--mode", choices=("time", "short", "rocprof", "head", "head_short", "head_trace"), default="time")
    ap.add_argument("--arm", choices=tuple(HEAD_ARMS), default="default")
    ap.add_argument("--arms", default=None, help="head: comma-separated arms to alternate (default: the three without "
                                                "+optim)")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    out = {"time": mode_time, "short": mode_short, "rocprof": mode_rocprof, "head": mode_head,
           "head_short": mode_head_short, "head_trace": mode_head_trace}[a.mode](a)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
