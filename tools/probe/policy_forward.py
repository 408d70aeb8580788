#!/usr/bin/env python3
"""Measure the fused policy MLP forward (h12learn_mlp_forward, h12env.policy.FusedMLP) against the torch path.

    python tools/probe/policy_forward.py [--rows 4096 8192] [--rounds 6] [--reps 40] [--out FILE]
    python tools/probe/policy_forward.py --mode rocprof [--out FILE]

time (default): per row count, at the Flat task's observation width, with both arms in one process, alternating
(fused, torch, fused, ...); the first iteration of every turn is dropped; median and minimum per arm, in us:
  (a) actor  actor-only inference, each arm one torch.cuda.graph replay (fused: one launch; torch: the module chain);
  (b) act    actor + critic as collection runs them: the CleanRL collector's graphed act body (forward of both
             networks, sample, log-probability) with H12_POLICY_FUSED=1 (pack + one two-network launch) and without;
  (c) loop   a closed loop of env.step(policy(obs)) over 200 steps, as play.py runs it, per step;
  (d) ppo    the collection time of one CleanRL PPO iteration (24 steps) with and without H12_POLICY_FUSED=1, in ms.
The FLOP floors next to them: 2 * rows * parameters / 157.3 TF/s (the fp32 matrix peak).
rocprof: starts `rocprofv3 --kernel-trace --stats -- python <this file> --mode short` as a child process (this
process never opens the GPU) and reports calls / average / min / max of mlp_pack_kernel and mlp_forward_kernel.
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
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[2]
PKG = ROOT / "h1v2-isaac_amd"
TASK = "Isaac-Velocity-CaT-Flat-H12_12dof-v0"
KERNELS = ("mlp_pack_kernel", "mlp_forward_kernel")
PEAK_FP32_MATRIX = 157.3e12


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


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "samples": len(v)}


def timed_us(fn, reps: int) -> float:
    """Mean us per call of fn over reps calls after one dropped call, between two events on the current stream."""
    import torch

    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def graphed(body):
    import torch

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(2):
            body()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = body()
    return g, out


def alternate(arms: dict, rounds: int, reps: int) -> dict:
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            res[k].append(timed_us(fn, reps))
    return {k: summary(v) for k, v in res.items()}


def measure_rows(env, n: int, a) -> dict:
    import torch
    from h12env import cleanrl
    from h12env.policy import FusedMLP

    base = env.unwrapped
    d_in = int(base.single_observation_space["policy"].shape[0])
    torch.manual_seed(1)
    agent = cleanrl.Agent(env).to("cuda:0")
    params = {name: sum(p.numel() for p in net.parameters())
              for name, net in (("actor", agent.actor_mean), ("critic", agent.critic))}
    x = torch.randn(n, d_in, device="cuda:0")
    out = {"rows": n, "d_in": d_in,
           "floor_us": {"actor": 2e6 * n * params["actor"] / PEAK_FP32_MATRIX,
                        "actor_critic": 2e6 * n * (params["actor"] + params["critic"]) / PEAK_FP32_MATRIX}}

    # (a) actor-only inference
    f = FusedMLP([agent.actor_mean], agent.obs_rms)
    gf, _ = graphed(lambda: f(x))
    gt, _ = graphed(lambda: agent.actor_mean(agent.obs_rms(x, update=False)))
    out["actor_us"] = alternate({"fused": gf.replay, "torch": gt.replay}, a.rounds, a.reps)

    # (b) the collector's act body
    arms = {}
    for arm, flag in (("fused", "1"), ("torch", "0")):
        os.environ["H12_POLICY_FUSED"] = flag
        col = cleanrl._Collector(agent, True)
        col.act(x)  # capture under this arm's setting
        arms[arm] = (lambda c=col: c._graphs[("act", tuple(x.shape))][0].replay())
    out["act_us"] = alternate(arms, a.rounds, a.reps)
    os.environ.pop("H12_POLICY_FUSED")
    return out


def measure_loop(env, a, steps=200) -> dict:
    import torch
    from h12env import cleanrl

    torch.manual_seed(1)
    agent = cleanrl.Agent(env).to("cuda:0")
    with torch.no_grad():
        for p in agent.actor_mean.parameters():
            p.mul_(0.1)
    arms = {"fused": agent.inference_policy(fused=True), "torch": agent.inference_policy()}
    res = {k: [] for k in arms}
    for _ in range(max(2, a.rounds // 2)):
        for k, policy in arms.items():
            obs = env.reset()[0]["policy"]
            with torch.no_grad():
                obs = env.step(policy(obs))[0]["policy"]  # dropped
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(steps):
                    obs = env.step(policy(obs))[0]["policy"]
                t1.record()
                t1.synchronize()
            res[k].append(1e3 * t0.elapsed_time(t1) / steps)
    return {"steps": steps, "us_per_step": {k: summary(v) for k, v in res.items()}}


def run_ppo(env, fused: bool, steps: int, iters: int, tmp: str):
    import torch
    from biped_tasks.tasks.agents import H12_12dof_FlatCleanRlPPOCfg
    from h12env import cleanrl

    os.environ["H12_POLICY_FUSED"] = "1" if fused else "0"
    cfg = H12_12dof_FlatCleanRlPPOCfg(num_steps=steps, num_iterations=1 + iters, save_interval=10 ** 9)
    cfg.minibatch_size = min(cfg.minibatch_size, steps * env.unwrapped.num_envs)
    run = tempfile.mkdtemp(dir=tmp)
    torch.manual_seed(1)
    cleanrl.PPO(env, cfg, run)
    torch.cuda.synchronize()
    os.environ.pop("H12_POLICY_FUSED")
    lines = [json.loads(x) for x in open(os.path.join(run, "metrics.jsonl"))][1:]
    return [1e3 * x["Perf/collection_time"] for x in lines]


def measure_ppo(env, a, steps=24, iters=3) -> dict:
    res = {"fused": [], "torch": []}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(max(2, a.rounds // 2)):
            for arm in res:
                res[arm].extend(run_ppo(env, arm == "fused", steps, iters, tmp))
    return {"steps": steps, "collection_ms": {k: summary(v) for k, v in res.items()}}


def mode_time(a):
    out = {"task": TASK, "rounds": a.rounds, "reps": a.reps, "rows": []}
    for n in a.rows:
        env = make_env(n)
        r = measure_rows(env, n, a)
        r["loop"] = measure_loop(env, a)
        r["ppo"] = measure_ppo(env, a)
        env.close()
        out["rows"].append(r)
    return out


def mode_short(a):
    import torch
    from h12env import cleanrl
    from h12env.policy import FusedMLP

    _paths()
    n, d_in = a.rows[0], a.d_in
    torch.manual_seed(1)
    stub = SimpleNamespace(single_observation_space={"policy": SimpleNamespace(shape=(d_in,))},
                           single_action_space=SimpleNamespace(shape=(12,)))
    stub.unwrapped = stub
    agent = cleanrl.Agent(stub).to("cuda:0")
    x = torch.randn(n, d_in, device="cuda:0")
    one, two = FusedMLP([agent.actor_mean], agent.obs_rms), FusedMLP([agent.actor_mean, agent.critic])
    for _ in range(50):
        one(x)
        two(x, repack=True)
    torch.cuda.synchronize()
    return {"ok": True}


def mode_rocprof(a):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
               str(Path(__file__).resolve()), "--mode", "short", "--rows", str(a.rows[0]), "--d_in", str(a.d_in)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(files[0])))
    out = {"command": "rocprofv3 --kernel-trace --stats -- python tools/probe/policy_forward.py --mode short",
           "rows": a.rows[0], "d_in": a.d_in,
           "note": "mlp_forward_kernel: 50 one-network (actor + normaliser) and 50 two-network (actor + critic) calls",
           "kernels": {}}
    for row in rows:
        for k in KERNELS:
            if k in row["Name"]:
                out["kernels"][k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                     "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("time", "short", "rocprof"), default="time")
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--d_in", type=int, default=450, help="observation width of the short / rocprof modes")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    _paths()
    out = {"time": mode_time, "short": mode_short, "rocprof": mode_rocprof}[a.mode](a)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
