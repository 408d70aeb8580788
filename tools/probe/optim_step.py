#!/usr/bin/env python3
"""Measure the fused optimiser step (h12env.optim) against torch's clip + optimiser.

    python tools/probe/optim_step.py --mode step [--rounds 4] [--calls 200] [--out FILE]
    python tools/probe/optim_step.py --mode runner [--rounds 4] [--updates 3] [--out FILE]

step: the optimiser step alone on the 17 parameter tensors of a cleanrl.Agent (270 observations, 12 actions) with fixed
gradients.  Per rule two arms, torch (clip_grad_norm_ + the class the trainer uses when its update is captured: Adam
fused / capturable, RAdam capturable) and fused (FusedClipAdam / FusedClipRAdam), each run eagerly and as a replayed HIP
graph; the arms alternate, ``calls`` steps per turn between two events, microseconds per step: median and minimum over
the turns.
runner: ppo.PPO.update at C3's learner shapes (4096 envs x 24 steps, 4 minibatches of 24 576 rows x 5 epochs, MLP
450-512-256-128) on a random rollout, no env in the process; the arms default and fused_optimizer alternate, the update
captured (H12_PPO_GRAPH=1), milliseconds per update between two events, the first update of every turn dropped.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd"))
DEV = "cuda:0"


def timed(fn, calls):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def make_step(rule: str, fused: bool, graphed: bool):
    import torch
    from h12env import cleanrl, optim
    from h12env.graphs import capture

    envs = SimpleNamespace(unwrapped=SimpleNamespace(single_observation_space={"policy": SimpleNamespace(shape=(270,))},
                                                     single_action_space=SimpleNamespace(shape=(12,))))
    torch.manual_seed(1)
    ps = list(cleanrl.Agent(envs).to(DEV).parameters())
    for p in ps:
        p.grad = torch.randn_like(p) * 1e-2
    lr = torch.tensor(1e-3, device=DEV)
    if fused:
        cls = optim.FusedClipAdam if rule == "adam" else optim.FusedClipRAdam
        opt = cls(ps, lr=lr, eps=1e-8 if rule == "adam" else 1e-5, max_norm=0.5)
        body = opt.step
    else:
        opt = (torch.optim.Adam(ps, lr=lr, fused=True, capturable=True) if rule == "adam"
               else torch.optim.RAdam(ps, lr=lr, eps=1e-5, capturable=True))

        def body():
            torch.nn.utils.clip_grad_norm_(ps, 0.5)
            opt.step()
    if not graphed:
        return body
    g, _ = capture(body, torch.device(DEV))
    return g.replay


def mode_step(a):
    arms = [(rule, fused, graphed) for rule in ("adam", "radam") for graphed in (False, True) for fused in (False, True)]
    fns = {arm: make_step(*arm) for arm in arms}
    for fn in fns.values():
        timed(fn, 20)
    res = {arm: [] for arm in arms}
    for _ in range(a.rounds):
        for arm in arms:
            res[arm].append(1e3 * timed(fns[arm], a.calls))
    out = {"tensors": 17, "calls_per_turn": a.calls, "turns": a.rounds, "unit": "us per step"}
    for (rule, fused, graphed), v in res.items():
        out[f"{rule} {'fused' if fused else 'torch'} {'graphed' if graphed else 'eager'}"] = {
            "median": statistics.median(v), "min": min(v), "turns": v}
    return out


def make_runner(fused_optimizer: bool):
    import torch
    from h12env.ppo import PPO, ActorCritic

    torch.manual_seed(7)
    pol = ActorCritic(450, 450, 12, [512, 256, 128], [512, 256, 128])
    alg = PPO(pol, num_learning_epochs=5, num_mini_batches=4, learning_rate=1e-3, schedule="adaptive", desired_kl=0.01,
              device=DEV, fused_optimizer=fused_optimizer)
    alg.init_storage(4096, 24, [450], None, [12])

    def update():
        g = torch.Generator(device=DEV).manual_seed(100)
        for k, v in alg.storage.t.items():
            v.copy_(torch.randn(v.shape, generator=g, device=DEV) * (0.1 if k == "sigma" else 1.0))
        alg.storage.t["sigma"].abs_().add_(0.5)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        alg.update()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    return update


def mode_runner(a):
    arms = {"default": make_runner(False), "fused_optimizer": make_runner(True)}
    res = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            res[k].extend([fn() for _ in range(1 + a.updates)][1:])
    out = {"shapes": "4096 envs x 24 steps, 4 minibatches x 5 epochs, MLP 450-512-256-128", "unit": "ms per update",
           "updates_per_arm": a.rounds * a.updates}
    for k, v in res.items():
        out[k] = {"median": statistics.median(v), "min": min(v), "all": v}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "runner"), default="step")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    out = {"step": mode_step, "runner": mode_runner}[a.mode](a)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
