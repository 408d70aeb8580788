#!/usr/bin/env python3
"""Measure the ray-cast renderer (h12render_render: render_setup_kernel + render_kernel), with the method of
tools/probe/policy_forward.py.

    python tools/probe/render.py [--rounds 6] [--reps 20] [--out FILE]

Cases: one 1280 x 720 view, 16 views of 320 x 180, 4096 views of 64 x 36, on a Flat env of 4096 robots after 50
random-action steps.  Per case two arms alternate in one process -- the per-tile culling on and off (the image is the
same either way) -- the first call of every turn dropped; median and minimum in us per call, next to the
output-bytes floor (rgb bytes / HBM write rate).  Then the cost a recorded step adds to play: env.step alone against
env.step + env.render() (device render, copy to the host) at the default 640 x 360 view.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd"))

CASES = (("1x1280x720", 1, (1280, 720)), ("16x320x180", 16, (320, 180)), ("4096x64x36", 4096, (64, 36)))
HBM_BYTES_PER_S = 8.0e12  # MI355X peak, for the output-bytes floor


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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    import torch

    from h12env import H12FlatEnvCfg
    from h12env.env import H12VelocityEnv
    from h12env.render import Renderer, ViewerCfg

    cfg = H12FlatEnvCfg()
    cfg.scene.num_envs = a.envs
    cfg.sim.device = "cuda:0"
    env = H12VelocityEnv(cfg, render_mode="rgb_array")
    env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    act = 0.3 * torch.randn(a.envs, 12, device="cuda:0", generator=g)
    for _ in range(50):
        env.step(act)
    out = {"command": "python tools/probe/render.py", "device": "1x MI355X", "envs": a.envs, "rounds": a.rounds,
           "reps": a.reps, "unit": "us per call", "cases": {}}
    for name, m, res in CASES:
        m = min(m, a.envs)
        ids = list(range(m))
        arms = {}
        for label, cull in (("cull", True), ("no_cull", False)):
            r = Renderer(env, viewer=ViewerCfg(resolution=res), cull=cull)
            arms[label] = (lambda r=r: r.render(ids))
        samples = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                samples[k].append(timed_us(fn, a.reps))
        c = {k: summary(v) for k, v in samples.items()}
        nbytes = m * res[0] * res[1] * 3
        c["rgb_bytes"] = nbytes
        c["output_floor_us"] = 1e6 * nbytes / HBM_BYTES_PER_S
        c["cull_speedup"] = c["no_cull"]["median"] / c["cull"]["median"]
        out["cases"][name] = c
    # the cost of recording a step
    step = lambda: env.step(act)  # noqa: E731

    def step_render():
        env.step(act)
        env.render()

    samples = {"step": [], "step_render": []}
    for _ in range(a.rounds):
        samples["step"].append(timed_us(step, a.reps))
        samples["step_render"].append(timed_us(step_render, a.reps))
    out["play_video"] = {k: summary(v) for k, v in samples.items()}
    out["play_video"]["added_us_per_step"] = (out["play_video"]["step_render"]["median"]
                                              - out["play_video"]["step"]["median"])
    env.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
