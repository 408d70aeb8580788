#!/usr/bin/env python3
"""Measure the safety monitor's cost on the physics-only path (h12env_step_physics_monitored against
h12env_step_physics), with the method of tools/probe/policy_forward.py.

    python tools/probe/safety_monitor.py [--envs 4096] [--substeps 20] [--rounds 6] [--reps 20] [--out FILE]

Three arms alternate in one process at --envs envs x --substeps substeps per call, robots held at the default pose by
the PD alone (without a policy they fall within the first seconds and lie on the floor: sole, knee and torso contacts
are active; base_height_mean in the output says where they ended): plain (h12env_step_physics, the unchanged physics_kernel: the baseline), monitored, and
monitored with one traced env.  The first call of every turn is dropped; median and minimum per arm, in us per call.
That process runs once per accumulator placement (child processes; H12_MON_REGS=1: registers over the call, 0:
read-modify-write per substep), so both placements are on record next to the default.  Then scripts/eval_policy.py runs
end to end in a child process (a near-zero policy exported here, 2 s episodes) and its env-substeps/s is recorded.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
PKG = ROOT / "h1v2-isaac_amd"
sys.path.insert(0, str(PKG))


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "samples": len(v)}


def timed_us(fn, reps: int) -> float:
    import torch

    fn()  # dropped
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def mode_arms(a) -> dict:
    import torch

    from h12env import mujoco_cfg
    from h12env.env import H12VelocityEnv
    from h12env.safety import SafetyMonitor

    cfg = mujoco_cfg()
    cfg.scene.num_envs = a.envs
    cfg.sim.device = "cuda:0"
    env = H12VelocityEnv(cfg)
    env.reset()
    q_ref = torch.tensor(list(env._model.q_default), device="cuda:0").expand(a.envs, 12).contiguous()
    mon, mon_t = SafetyMonitor(env), SafetyMonitor(env, trace_envs=1)

    def traced():
        env.step_physics(q_ref, a.substeps, monitor=mon_t)
        mon_t._trace.clear()  # keep one call's records, as a consumer that drains them would

    arms = {"plain": lambda: env.step_physics(q_ref, a.substeps),
            "monitored": lambda: env.step_physics(q_ref, a.substeps, monitor=mon),
            "monitored_trace1": traced}
    for _ in range(10):  # drop onto the floor
        env.step_physics(q_ref, a.substeps)
    res = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            res[k].append(timed_us(fn, a.reps))
    out = {k: summary(v) for k, v in res.items()}
    out["overhead_monitored"] = out["monitored"]["median"] / out["plain"]["median"] - 1.0
    out["overhead_monitored_trace1"] = out["monitored_trace1"]["median"] / out["plain"]["median"] - 1.0
    out["base_height_mean"] = float(env._field("POS")[2].mean())
    env.close()
    return out


def child(args: list, env: dict | None = None, timeout=280) -> subprocess.CompletedProcess:
    r = subprocess.run([sys.executable, *args], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise RuntimeError(f"{args[0]} failed ({r.returncode}): {r.stdout[-1000:]}{r.stderr[-2000:]}")
    return r


def mode_all(a) -> dict:
    me = str(Path(__file__).resolve())
    common = ["--envs", str(a.envs), "--substeps", str(a.substeps), "--rounds", str(a.rounds), "--reps", str(a.reps)]
    out = {"command": "python tools/probe/safety_monitor.py", "device": "1x MI355X", "envs": a.envs,
           "substeps_per_call": a.substeps, "rounds": a.rounds, "reps": a.reps, "unit": "us per call",
           "note": "plain: h12env_step_physics (the unchanged physics_kernel); monitored: "
                   "h12env_step_physics_monitored; monitored_trace1: the same with one traced env.  One process per "
                   "accumulator placement, the three arms alternating in it; the first call of every turn dropped."}
    for name, flag in (("registers", "1"), ("read_modify_write", "0")):
        r = child([me, "--mode", "arms", *common], {"H12_MON_REGS": flag})
        out[name] = json.loads(r.stdout[r.stdout.index("{"):])
    # end to end: scripts/eval_policy.py on a policy exported here (CPU only in this process)
    import torch

    from h12env.cfg import H12FlatEnvCfg
    from h12env.export import export_policy_as_jit, write_env_yaml
    from h12env.ppo import ActorCritic

    with tempfile.TemporaryDirectory() as tmp:
        torch.manual_seed(0)
        pol = ActorCritic(450, 450, 12, [512, 256, 128], [512, 256, 128])
        for p in pol.actor.parameters():
            p.data.mul_(0.01)
        export_policy_as_jit(pol, None, tmp)
        write_env_yaml(H12FlatEnvCfg(), str(Path(tmp) / "env.yaml"))
        args = [str(PKG / "scripts" / "eval_policy.py"), tmp, "--num_envs", str(a.envs), "--episode_length", "2.0",
                "--fused", "--log_dir", str(Path(tmp) / "log")]
        child(args)
        ev = json.loads((Path(tmp) / "log" / "eval.json").read_text())
    out["eval_policy"] = {"command": "python scripts/eval_policy.py <policy_dir> --num_envs %d --episode_length 2.0 --fused"
                                     % a.envs,
                          "wall_s": ev["run"]["wall_s"], "env_substeps_per_s": ev["run"]["env_substeps_per_s"],
                          "env_substeps": ev["summary"]["substeps"], "share_any_viol": ev["summary"]["share_any_viol"]}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("all", "arms"), default="all")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    out = {"all": mode_all, "arms": mode_arms}[a.mode](a)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
