#!/usr/bin/env python3
"""Measurements of DESIGN.md section 7s: the student observation launch and one distillation iteration.

    python tools/probe/student_obs.py launch  --out DIR   # h12student_observe back to back, device events
    python tools/probe/student_obs.py trace   --out DIR   # the same launches, few of them: run it under
                                                           # rocprofv3 --kernel-trace --stats for the kernel time
    python tools/probe/student_obs.py env     --out DIR   # Rough env.step() without the group, with H = 1 and H = 6
    python tools/probe/student_obs.py distill --out DIR   # 4096 envs x 24 steps, LSTM 256: collection and update,
                                                           # library path and fused (H12_POLICY_FUSED=1 is read at start)

Every mode needs the GPU and writes DIR/student_<mode>.json.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "h1v2-isaac_amd" / "shims"), str(ROOT / "h1v2-isaac_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = [(4096, 1), (4096, 6), (8192, 1), (8192, 6)]


def planted(n: int, seed: int = 0):
    from h12env._abi import NF_FLOAT, NF_INT, I

    r = np.random.default_rng(seed)
    Fh = r.normal(size=(NF_FLOAT, n)).astype(np.float32)
    Ih = r.integers(0, 1 << 20, size=(NF_INT, n)).astype(np.int32)
    pk = I["PACK"][0]
    Ih[pk] = (Ih[pk] & ~(3 << 9)) | (2 << 9)
    Ih[pk, ::50] &= ~(3 << 9)  # 2 % of the rows fill
    buf = torch.empty((NF_FLOAT + NF_INT) * n, dtype=torch.int32, device="cuda")
    buf[:Fh.size] = torch.from_numpy(Fh.reshape(-1).view(np.int32)).cuda()
    buf[Fh.size:] = torch.from_numpy(Ih.reshape(-1)).cuda()
    return buf


def launcher(n: int, h: int):
    from h12env import student

    lib = student.student_library()
    c = student.StudentConfig()
    c.history, c.enable_corruption, c.seed_lo = h, 1, 42
    for i, nz in enumerate((0.2, 0.05, 0.0, 0.01, 1.5, 0.0)):
        c.noise[i], c.scale[i] = nz, 1.0
    ws = planted(n)
    bufs = [torch.zeros(n, 45 * h, device="cuda") for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    ref = C.byref(c)

    def run(k: int):
        rc = lib.h12student_observe(ws.data_ptr(), n, ref, bufs[k & 1].data_ptr(), bufs[(k + 1) & 1].data_ptr(), k + 1,
                                    stream)
        if rc:
            student.check(lib, rc, "h12student_observe")

    run.keep = (ws, bufs, c)
    return run


def mode_launch(reps: int):
    out = {}
    for n, h in SIZES:
        run = launcher(n, h)
        for k in range(200):
            run(k)
        torch.cuda.synchronize()
        windows = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(reps):
                run(k)
            e1.record()
            torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) * 1e3 / reps)
        out[f"n{n}_H{h}"] = {"us_per_launch_windows": windows, "bytes_written": n * 45 * h * 4,
                             "bytes_prev_read": n * 45 * (h - 1) * 4}
        print(f"n = {n} H = {h}: {min(windows):.2f} .. {max(windows):.2f} us per back-to-back launch", flush=True)
    return out


def mode_trace():
    for n, h in SIZES:
        run = launcher(n, h)
        for k in range(500):
            run(k)
        torch.cuda.synchronize()
    return {"launches_per_size": 500, "order": [f"n{n}_H{h}" for n, h in SIZES]}


def rough_env(n: int, h: int | None):
    from h12env import cfg as K
    from h12env.env import H12VelocityEnv

    c = K.H12RoughEnvCfg()
    c.scene.num_envs = n
    c.sim.device = "cuda:0"
    if h is not None:
        c.observations.student = K.StudentObsCfg(history_length=h)
    return H12VelocityEnv(c)


def mode_env(steps: int):
    out = {}
    for n in (4096, 8192):
        for h in (None, 1, 6):
            env = rough_env(n, h)
            env.reset()
            g = torch.Generator(device="cuda").manual_seed(1)
            acts = [torch.randn(n, 12, device="cuda", generator=g) for _ in range(16)]
            for k in range(100):
                env.step(acts[k & 15])
            torch.cuda.synchronize()
            windows = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(steps):
                    env.step(acts[k & 15])
                e1.record()
                torch.cuda.synchronize()
                windows.append(e0.elapsed_time(e1) * 1e3 / steps)
            env.close()
            out[f"n{n}_H{h}"] = windows
            print(f"Rough n = {n} student H = {h}: {min(windows):.2f} .. {max(windows):.2f} us per env.step()", flush=True)
    return out


def mode_distill(iters: int):
    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from h12env import cfg as K
    from h12env.ppo import ActorCritic
    from isaaclab_rl.rsl_rl import (RslRlDistillationAlgorithmCfg, RslRlDistillationStudentTeacherRecurrentCfg,
                                    RslRlVecEnvWrapper)
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    task = "Isaac-Velocity-Rough-H12_12dof-v0"
    fused = os.environ.get("H12_POLICY_FUSED", "0") == "1"
    env_cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    env_cfg.scene.num_envs = 4096
    K.enable_student_observations(env_cfg, 1)
    dims = list(agent.policy.actor_hidden_dims)
    agent.policy = RslRlDistillationStudentTeacherRecurrentCfg(student_hidden_dims=dims, teacher_hidden_dims=dims,
                                                               rnn_hidden_dim=256)
    agent.algorithm = RslRlDistillationAlgorithmCfg(gradient_length=12, fused_rnn_update=fused)
    env = RslRlVecEnvWrapper(gym.make(task, cfg=env_cfg))
    runner = OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0")
    torch.manual_seed(0)
    teacher = ActorCritic(235, 235, 12, actor_hidden_dims=dims, critic_hidden_dims=dims)
    with torch.no_grad():
        for p in teacher.actor[-1].parameters():
            p.mul_(0.1)  # a random teacher with small actions: robots that stand for a while
    runner.alg.policy.load_state_dict(teacher.state_dict())
    # the runner's own Perf/* times are host clocks around enqueues (the update never synchronises): here the update
    # is bracketed by device synchronises, and the collection is the rest of the iteration
    alg, inner, spent = runner.alg, runner.alg.update, []

    def timed_update():
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = inner()
        torch.cuda.synchronize()
        spent.append(time.perf_counter() - t)
        return out

    alg.update = timed_update
    rows = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        runner.learn(1)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        rows.append({"iteration_s": wall, "update_s": spent[-1], "collection_s": wall - spent[-1],
                     "behavior": runner.last_iteration_stats["Loss/behavior"]})
    env.close()
    return {"fused_collection_and_update": fused, "envs": 4096, "steps": 24, "gradient_length": 12, "iterations": rows}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["launch", "trace", "env", "distill"])
    ap.add_argument("--out", type=Path, required=True)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--tag", default="")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("student_obs.py measures on the GPU: no device found")
    t0 = time.time()
    res = {"launch": lambda: mode_launch(args.reps), "trace": mode_trace, "env": lambda: mode_env(args.steps),
           "distill": lambda: mode_distill(args.iters)}[args.mode]()
    args.out.mkdir(parents=True, exist_ok=True)
    name = f"student_{args.mode}{('_' + args.tag) if args.tag else ''}.json"
    (args.out / name).write_text(json.dumps({"mode": args.mode, "wall_s": time.time() - t0, "result": res}, indent=1))
    print(f"wrote {args.out / name}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
