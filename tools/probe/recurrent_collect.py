#!/usr/bin/env python3
"""Time the collection step of the recurrent policy (PPO.act of an ActorCriticRecurrent: both memories, both MLPs, the
sample and its log-probability) at the Flat task's shape: 450 observations, LSTM of 256, MLPs 512-256-128.

    python tools/probe/recurrent_collect.py [--envs 4096] [--rounds 6] [--reps 50] [--out FILE]

Four arms in one process, alternating (the first call of every turn is dropped), each timed between two device events
over --reps calls; median and minimum over the rounds, in us per step:
  torch_eager    the default path: nn.LSTM step + the module chain
  fused_eager    H12_POLICY_FUSED=1, H12_PPO_GRAPH=0: pack + one two-network h12learn_lstm_step launch
  fused_graphed  H12_POLICY_FUSED=1: the same body as PPO captures it
  torch_graphed  the default path's body captured here (PPO does not capture it); measured last, and reported as not
                 measured when the library LSTM cannot be captured
The observations are random: the time does not depend on them.  The FLOP floor next to the numbers is
2 * rows * parameters / 157.3 TF/s (the fp32 matrix peak)."""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd"))
PEAK_FP32_MATRIX = 157.3e12


def timed_us(fn, reps: int) -> float:
    import torch

    fn()
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import torch

    from h12env.graphs import capture
    from h12env.ppo import PPO, ActorCriticRecurrent

    if not torch.cuda.is_available():
        raise SystemExit("recurrent_collect: no GPU (a timing needs the MI355X)")
    dev = "cuda:0"
    torch.manual_seed(0)
    base = ActorCriticRecurrent(450, 450, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128],
                                rnn_hidden_dim=256)
    obs = torch.randn(args.envs, 450, device=dev)
    params = sum(p.numel() for n, p in base.named_parameters() if n != "std")
    switches = {"torch_eager": ("0", "0"), "fused_eager": ("1", "0"), "fused_graphed": ("1", "1")}
    algs = {name: PPO(copy.deepcopy(base), device=dev) for name in switches}

    def arm(name):
        fused, graph = switches[name]

        def call():
            os.environ["H12_POLICY_FUSED"], os.environ["H12_PPO_GRAPH"] = fused, graph
            with torch.inference_mode():
                algs[name].act(obs, obs)
        return call

    arms = {name: arm(name) for name in switches}
    for call in arms.values():  # every shape and path once before any timed window
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    samples = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, call in arms.items():
            samples[name].append(timed_us(call, args.reps))
    assert algs["fused_graphed"]._ga is not None and getattr(algs["torch_eager"], "_ga", None) is None
    result = {name: {"median_us": statistics.median(v), "min_us": min(v), "samples": len(v)} for name, v in samples.items()}

    # the default path's body in a graph of this tool's own; last, so that a refused capture costs nothing above
    os.environ["H12_POLICY_FUSED"] = "0"
    try:
        policy = copy.deepcopy(base).to(dev)
        with torch.no_grad():
            for mem in (policy.memory_a, policy.memory_c):
                mem.hidden_states = tuple(torch.zeros(1, args.envs, 256, device=dev) for _ in range(2))
                mem.keep_storage = True

            def body():
                a = policy.act(obs)
                return a, policy.evaluate(obs), policy.get_actions_log_prob(a)

            g, _ = capture(body, dev)
            v = [timed_us(g.replay, args.reps) for _ in range(args.rounds)]
        result["torch_graphed"] = {"median_us": statistics.median(v), "min_us": min(v), "samples": len(v)}
    except Exception as e:  # noqa: BLE001  (whatever the capture raises is the finding)
        result["torch_graphed"] = {"not_measured": f"{type(e).__name__}: {e}"[:300]}
    result["envs"] = args.envs
    result["flop_floor_us"] = 1e6 * 2 * args.envs * params / PEAK_FP32_MATRIX
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
