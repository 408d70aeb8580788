#!/usr/bin/env python3
"""Measurements of DESIGN.md section 7t: Random Network Distillation's per-env-step work.

    python tools/probe/rnd_step.py reward --out DIR   # the RND part of PPO.process_env_step, torch path and fused,
                                                       # interleaved pairs, device events; launches per step
    python tools/probe/rnd_step.py env    --out DIR   # Flat env.step() without the rnd_state group and with it
    python tools/probe/rnd_step.py train  --out DIR   # one runner, collection + update, plain PPO / --rnd / fused

Every mode needs the GPU and writes DIR/rnd_<mode>.json.  4096 envs, the default 36-float rnd_state, predictor and
target [256, 256] -> 16 (and -> 1), both normalisers on.
"""
from __future__ import annotations

import argparse
import copy
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "h1v2-isaac_amd" / "shims"), str(ROOT / "h1v2-isaac_amd")]

import torch  # noqa: E402

N = 4096
DEV = "cuda:0"


def window(fn, reps: int) -> float:
    """Microseconds per call over one window of reps calls (device events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def launches(fn) -> int | None:
    """Kernel launches of one call, from the profiler's device events; None where the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return n or None
    except Exception:  # noqa: BLE001
        return None


def mode_reward(reps: int):
    from h12env.rnd import FusedRND, RandomNetworkDistillation

    out = {}
    for d_out in (16, 1):
        torch.manual_seed(0)
        base = RandomNetworkDistillation(36, num_outputs=d_out, predictor_hidden_dims=[256, 256],
                                         target_hidden_dims=[256, 256], weight=0.02, state_normalization=True,
                                         reward_normalization=True, device=DEV).train()
        torch_mod, fused_mod = copy.deepcopy(base), copy.deepcopy(base)
        fused = FusedRND(fused_mod)
        x = torch.randn(N, 36, device=DEV)
        rew = torch.randn(N, device=DEV)

        def torch_path():
            with torch.inference_mode():
                r = rew.clone()
                intrinsic, s = torch_mod.get_intrinsic_reward(x)
                r += intrinsic
            return r

        def fused_path():
            with torch.inference_mode():
                return fused(x, rew.clone())

        for f in (torch_path, fused_path):
            for _ in range(50):
                f()
        torch.cuda.synchronize()
        pairs = []
        for _ in range(7):  # interleaved pairs
            pairs.append((window(torch_path, reps), window(fused_path, reps)))
        t, f = sorted(p[0] for p in pairs), sorted(p[1] for p in pairs)
        out[f"d_out_{d_out}"] = {"torch_us": t[len(t) // 2], "fused_us": f[len(f) // 2], "pairs_us": pairs,
                                 "torch_launches": launches(torch_path), "fused_launches": launches(fused_path)}
    return out


def make_env(rnd_state: bool):
    from h12env import cfg as K
    from h12env.env import H12VelocityEnv

    cfg = K.H12FlatEnvCfg()
    cfg.scene.num_envs = N
    cfg.sim.device = DEV
    if rnd_state:
        cfg.observations.rnd_state = K.RndStateObsCfg()
    return H12VelocityEnv(cfg)


def mode_env(reps: int):
    envs = {"off": make_env(False), "rnd_state": make_env(True)}
    a = torch.zeros(N, 12, device=DEV)
    for e in envs.values():
        e.reset()
        for _ in range(100):
            e.step(a)
    torch.cuda.synchronize()
    pairs = []
    for _ in range(7):
        pairs.append(tuple(window(lambda e=e: e.step(a), reps) for e in envs.values()))
    off, on = sorted(p[0] for p in pairs), sorted(p[1] for p in pairs)
    return {"step_us_off": off[len(off) // 2], "step_us_rnd_state": on[len(on) // 2], "pairs_us": pairs}


def mode_train(iters: int):
    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from h12env.cfg import enable_rnd_state
    from h12env.ppo import OnPolicyRunner
    from isaaclab_rl.rsl_rl import RslRlRndCfg, RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    task = "Isaac-Velocity-Flat-H12_12dof-v0"
    out = {}
    for name in ("plain", "rnd", "rnd_fused", "plain_again"):
        env_cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
        agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
        env_cfg.scene.num_envs = N
        if name.startswith("rnd"):
            enable_rnd_state(env_cfg)
            agent.algorithm.rnd_cfg = RslRlRndCfg(weight=1.0, state_normalization=True, reward_normalization=True,
                                                  num_outputs=16, predictor_hidden_dims=[256, 256],
                                                  target_hidden_dims=[256, 256], fused=name == "rnd_fused")
        env = RslRlVecEnvWrapper(gym.make(task, cfg=env_cfg))
        runner = OnPolicyRunner(env, agent.to_dict(), log_dir=None, device=DEV)
        runner.learn(3)  # builds the graphs, warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.learn(iters)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[name] = {"env_steps_per_s": N * runner.num_steps_per_env * iters / dt, "seconds": dt, "iterations": iters}
        env.close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["reward", "env", "train"])
    ap.add_argument("--out", default="out")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnd_step.py measures on the GPU; none is visible")
    modes = {"reward": lambda: mode_reward(a.reps), "env": lambda: mode_env(a.reps), "train": lambda: mode_train(a.iters)}
    res = modes[a.mode]()
    Path(a.out).mkdir(parents=True, exist_ok=True)
    (Path(a.out) / f"rnd_{a.mode}.json").write_text(json.dumps(res, indent=1))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
