#!/usr/bin/env python3
"""Measure h12learn_mirror_rows (gather + mirror + concatenation in one launch) against the torch path it replaces,
and the learner's time per iteration with the mirror augmentation on and off.

    python tools/probe/mirror_rows.py [--rows 24576] [--widths 450 270] [--rounds 8] [--reps 200] [--out FILE]
    python tools/probe/mirror_rows.py --learner [--envs 4096] [--iterations 8] [--out FILE]

kernel (default): per width, both arms in one process, alternating (kernel, torch, kernel, ...); the first iteration
of every turn is dropped; median and minimum per arm, in us, from device events.  The source is a rollout of
4 x rows rows and the index a random permutation's first `rows` entries, as the learner's minibatch gather is:
  kernel  one h12learn_mirror_rows launch, both = 1;
  torch   index_select (rows) + index_select (columns) + mul (signs) + cat: four launches.
Next to them: the time of a plain copy moving the same number of bytes (n d floats read + 2 n d written) on the same
device, which is the traffic floor of the operation at the copy rate this device reaches.
learner: the loop bench.py --mode train times (OnPolicyRunner.learn(1) on the Flat task, after a warm-up), once
without symmetry and once each with --symmetry augment / both; Perf/learning_time per iteration, median / min, in ms.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
PKG = ROOT / "h1v2-isaac_amd"
for p in (PKG / "shims", PKG):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "samples": len(v)}


def timed(torch, fn, reps):
    """us per call of reps calls between two device events; the first (dropped) call is outside the window."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def kernel_mode(args):
    import torch

    from h12env import cfg as K
    from h12env import symmetry as S
    from h12env._learn import mirror_rows

    if not torch.cuda.is_available():
        raise SystemExit("mirror_rows probe: no GPU visible (a measurement path never falls back)")
    dev = torch.device("cuda:0")
    cfgs = {450: K.H12FlatEnvCfg, 270: K.H12RslEnvCfg, 235: K.H12RoughEnvCfg}
    res = {"rows": args.rows, "rounds": args.rounds, "reps": args.reps, "unit": "us", "widths": {}}
    for d in args.widths:
        t = S.mirror_table(cfgs[d]())
        n = args.rows
        x = torch.randn(4 * n, d, device=dev)
        idx = torch.randperm(4 * n, device=dev)[:n].contiguous()
        packed = t.packed(dev)
        src = t.src.long().to(dev)
        sign = torch.where(t.flip, -1.0, 1.0).to(dev)
        out = torch.empty(2 * n, d, device=dev)
        c_in, c_out = torch.randn(3 * n * d // 2, device=dev), torch.empty(3 * n * d // 2, device=dev)

        def arm_kernel():
            mirror_rows(x, packed, idx, True, out=out)

        def arm_torch():
            rows = x.index_select(0, idx)
            return torch.cat([rows, rows.index_select(1, src) * sign])

        def arm_copy():  # the same 3 n d floats of traffic as a plain copy: 1.5 n d read, 1.5 n d written
            c_out.copy_(c_in)

        arm_kernel()
        same = torch.equal(arm_torch(), out)
        arms = {"kernel": arm_kernel, "torch": arm_torch, "copy_floor": arm_copy}
        samples = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                samples[k].append(timed(torch, fn, args.reps))
        nbytes = 3 * n * d * 4
        r = {k: summary(v) for k, v in samples.items()}
        r["bytes"] = nbytes
        r["copy_rate_TBps"] = nbytes / (r["copy_floor"]["median"] * 1e-6) / 1e12
        r["kernel_rate_TBps"] = nbytes / (r["kernel"]["median"] * 1e-6) / 1e12
        r["torch_over_kernel"] = r["torch"]["median"] / r["kernel"]["median"]
        r["kernel_equals_torch"] = same
        res["widths"][str(d)] = r
    return res


def learner_mode(args):
    import torch

    from biped_tasks.tasks.agents import H12_12dof_FlatPPORunnerCfg
    from h12env import H12FlatEnvCfg
    from h12env.env import H12VelocityEnv
    from h12env.ppo import OnPolicyRunner
    from isaaclab_rl.rsl_rl import RslRlSymmetryCfg, RslRlVecEnvWrapper

    if not torch.cuda.is_available():
        raise SystemExit("mirror_rows probe: no GPU visible (a measurement path never falls back)")
    res = {"envs": args.envs, "iterations": args.iterations, "unit": "ms", "arms": {}}
    for arm in ("off", "augment", "both"):
        cfg = H12FlatEnvCfg()
        cfg.scene.num_envs = args.envs
        cfg.sim.device = "cuda:0"
        env = RslRlVecEnvWrapper(H12VelocityEnv(cfg))
        agent = H12_12dof_FlatPPORunnerCfg(device="cuda:0")
        if arm != "off":
            agent.algorithm.symmetry_cfg = RslRlSymmetryCfg(
                use_data_augmentation=True, use_mirror_loss=arm == "both", mirror_loss_coeff=1.0,
                data_augmentation_func="h12env.symmetry:augment")
        runner = OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0")
        with contextlib.redirect_stdout(io.StringIO()):
            runner.learn(2, init_at_random_ep_len=True)
        learn, coll = [], []
        for _ in range(args.iterations):
            with contextlib.redirect_stdout(io.StringIO()):
                runner.learn(1)
            st = runner.last_iteration_stats
            learn.append(1e3 * st["Perf/learning_time"])
            coll.append(1e3 * st["Perf/collection_time"])
        res["arms"][arm] = {"learning": summary(learn), "collection": summary(coll)}
        env.close()
        del runner
    off = res["arms"]["off"]["learning"]["median"]
    for arm in ("augment", "both"):
        res["arms"][arm]["learning_over_off"] = res["arms"][arm]["learning"]["median"] / off
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=24576)
    ap.add_argument("--widths", type=int, nargs="+", default=[450, 270], choices=[450, 270, 235])
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--learner", action="store_true")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = learner_mode(args) if args.learner else kernel_mode(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
