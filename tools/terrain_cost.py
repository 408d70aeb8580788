"""GPU: what the reference's Rough terrain mix costs per env step, against the project's terrain on the same build.

Two Rough envs of --envs robots live side by side: one on the task's own terrain (1201 x 2001 cells of 0.1 m), one on
isaaclab_rough_terrains_cfg (2401 x 4001 cells of 0.05 m).  Both run the same kernels; what differs is the size of the
field the contacts and the 187-ray scan gather from, and what the robots stand on.  Windows of --steps env steps are
timed with device events in interleaved pairs (A B, B A, A B, ...), after a warm-up of both, so that a drift of the
machine falls on both arms alike.  Two cases: "curriculum" is the task as it is (under these random actions nobody walks,
so the curriculum takes every env down to row 0 and the footprint is one row of sub-terrains); "all_rows" switches the
curriculum off and spreads the initial levels over all ten rows, the widest footprint the gathers can have.  Measured,
not gated: the figures go into profiles/terrain_mix/cost.json.

    python tools/terrain_cost.py [--envs 4096] [--steps 5000] [--pairs 8] [--out profiles/terrain_mix]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd"))


def make_env(n: int, terrain: str, all_rows: bool):
    from h12env.cfg import H12RoughEnvCfg, apply_terrain_choice
    from h12env.env import H12VelocityEnv

    cfg = H12RoughEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    apply_terrain_choice(cfg, terrain)
    if all_rows:
        cfg.curriculum.terrain_levels = False
        cfg.scene.terrain.max_init_terrain_level = None
    return H12VelocityEnv(cfg)


def measure(a, all_rows: bool) -> dict:
    import torch

    arms = {k: make_env(a.envs, k, all_rows) for k in ("project", "isaaclab_rough")}
    g = torch.Generator(device="cuda").manual_seed(1)
    acts = [0.5 * torch.randn(a.envs, 12, device="cuda", generator=g) for _ in range(16)]
    field = {}
    for name, env in arms.items():
        env.reset()
        for k in range(a.warmup):
            env.step(acts[k & 15])
        t = env.terrain
        field[name] = {"cells": list(t.shape), "cell_m": t.hscale, "bytes": int(t.heights.nbytes)}
    torch.cuda.synchronize()

    def window(env):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.steps):
            env.step(acts[k & 15])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.steps

    us = {k: [] for k in arms}
    for p in range(a.pairs):
        order = list(arms) if p % 2 == 0 else list(arms)[::-1]
        for name in order:
            us[name].append(window(arms[name]))
        print(f"{'all_rows' if all_rows else 'curriculum'} pair {p}: " + ", ".join(f"{k} {us[k][-1]:.2f} us" for k in arms),
              flush=True)
    levels = {k: [float(v) for v in torch.bincount(env.terrain_levels().long(), minlength=10) / a.envs]
              for k, env in arms.items()}
    for env in arms.values():
        env.close()
    ratio = [m / q for m, q in zip(us["isaaclab_rough"], us["project"])]
    return {"field": field, "us_per_step": us, "median_us": {k: statistics.median(v) for k, v in us.items()},
            "ratio_mix_over_project": {"per_pair": ratio, "median": statistics.median(ratio), "min": min(ratio),
                                       "max": max(ratio)},
            "share_of_envs_per_level_after": levels}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "terrain_mix")
    a = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("terrain_cost.py measures on the GPU: no device found")
    t0 = time.time()
    cases = {"curriculum": measure(a, False), "all_rows": measure(a, True)}
    out = {"command": "python tools/terrain_cost.py", "device": "1x MI355X", "task": "Isaac-Velocity-Rough-H12_12dof-v0",
           "envs": a.envs, "steps_per_window": a.steps, "pairs": a.pairs, "warmup_steps": a.warmup,
           "unit": "us per env.step(), device events, interleaved pairs", "cases": cases, "wall_s": time.time() - t0}
    a.out.mkdir(parents=True, exist_ok=True)
    (a.out / "cost.json").write_text(json.dumps(out, indent=1) + "\n")
    for name, c in cases.items():
        r = c["ratio_mix_over_project"]
        print(f"{name}: median {c['median_us']}; mix / project {r['median']:.4f} ({r['min']:.4f} .. {r['max']:.4f})")
    print(f"wrote {a.out / 'cost.json'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
