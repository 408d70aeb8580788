#!/usr/bin/env python3
"""Generate tests/golden/ref_cleanrl_* from the reference's CleanRL PPO (build container only).

The reference's utils/cleanrl/ppo.py and its cfg files are imported by file path from /root/reference (they need
only numpy and torch; ``isaaclab.utils.configclass`` is stubbed as the identity) and driven on CPU; only arrays,
names and settings are written -- no reference source enters the repository.

  ref_cleanrl_rms.npz    RunningMeanStd in float64 over a seeded sequence of fp32-valued batches (shape (5,) and
                         shape ()), update on and off: the inputs, and mean / var / count / output after every call
  ref_cleanrl_agent.json Agent state_dict key names and shapes at the CaT task's dimensions (450 obs, 12 actions),
                         and the values of agents/clean_rl_ppo_cfg.py
  ref_cleanrl_ppo.npz    PPO() for 2 iterations on tests/helpers/toy_cat.py (table-driven env, 8 envs): the tables,
                         the actions the env received, the logged scalars, and the final agent (small tensors in
                         full; of the large layers the first 4 rows plus fp64 sum and sum of squares).
                         torch.utils.tensorboard.SummaryWriter is stubbed with a recorder and the module's
                         layer_init is replaced by toy_cat.SeededInit, so the initial weights are a RandomState rule.

    python tools/gen_golden_cleanrl.py
"""
from __future__ import annotations

import importlib.util
import json
import sys
import tempfile
import types
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
REF = Path("/root/reference/packages/biped_tasks/biped_tasks")
OUT = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT / "tests" / "helpers"))

import toy_cat  # noqa: E402


def _load(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


class Recorder:
    """SummaryWriter stand-in: add_scalar(tag, value, step) -> scalars[tag] = [values by step]."""
    scalars: dict = {}

    def __init__(self, log_dir=None, **kw):
        type(self).scalars = {}

    def add_scalar(self, tag, value, step):
        type(self).scalars.setdefault(tag, []).append(float(value))


def install_stubs():
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = Recorder
    sys.modules["torch.utils.tensorboard"] = tb
    for name in ("isaaclab", "isaaclab.utils", "biped_tasks", "biped_tasks.utils", "biped_tasks.utils.cleanrl"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["isaaclab.utils"].configclass = lambda cls: cls


def gen_rms(ref):
    rs = np.random.RandomState(3)
    out = {}
    for tag, shape in (("vec", (5,)), ("scalar", ())):
        m = ref.RunningMeanStd(shape=shape).double()
        ns = [7, 1, 4, 16, 3, 9]
        updates = [1, 1, 0, 1, 0, 1]
        offs = np.array([0.0, 1e3, -7e4, 0.5, 2.0])[: (shape[0] if shape else 1)]
        scl = np.array([1.0, 1e-2, 1.0, 0.0, 3.0])[: (shape[0] if shape else 1)]
        for i, (n, u) in enumerate(zip(ns, updates)):
            x = (offs + scl * rs.standard_normal((n, len(offs)))).astype(np.float32)
            if not shape:
                x = x[:, 0]
            y = m(torch.from_numpy(x).double(), update=bool(u))
            out[f"{tag}_x{i}"] = x
            out[f"{tag}_y{i}"] = y.numpy().copy()
            out[f"{tag}_mean{i}"] = m.running_mean.numpy().copy()
            out[f"{tag}_var{i}"] = m.running_var.numpy().copy()
            out[f"{tag}_count{i}"] = m.count.numpy().copy()
        out[f"{tag}_update"] = np.array(updates)
    np.savez_compressed(OUT / "ref_cleanrl_rms.npz", **out)


def gen_agent(ref):
    env = SimpleNamespace(single_observation_space={"policy": SimpleNamespace(shape=(450,))},
                          single_action_space=SimpleNamespace(shape=(12,)))
    env.unwrapped = env
    sd = ref.Agent(env).state_dict()
    rl_cfg = _load("biped_tasks.utils.cleanrl.rl_cfg", REF / "utils/cleanrl/rl_cfg.py")
    cfg = _load("_ref_clean_rl_ppo_cfg",
                REF / "tasks/locomotion/velocity/config/h12_12dof/agents/clean_rl_ppo_cfg.py")
    cls = cfg.H12_12dof_FlatPPORunnerCfg
    names = list(rl_cfg.CleanRlPpoActorCriticCfg.__annotations__)
    values = {n: getattr(cls, n) for n in names}
    with open(OUT / "ref_cleanrl_agent.json", "w") as f:
        json.dump({"state_dict": {k: list(v.shape) for k, v in sd.items()}, "cfg": values}, f, indent=1)


def gen_ppo(ref):
    cfg = toy_cat.toy_ppo_cfg()
    tables = toy_cat.make_tables(cfg.num_steps * cfg.num_iterations)
    env = toy_cat.ToyCaTEnv(tables)
    agents = []
    real_agent = ref.Agent

    def recording_agent(envs):
        a = real_agent(envs)
        agents.append(a)
        return a

    ref.layer_init = toy_cat.SeededInit()
    ref.Agent = recording_agent
    torch.manual_seed(cfg.seed)
    with tempfile.TemporaryDirectory() as d:
        ref.PPO(env, cfg, d)
        saved = sorted(p.name for p in Path(d).iterdir())
    ref.Agent = real_agent
    sd = {k: v.detach().cpu().numpy() for k, v in agents[0].state_dict().items()}
    out = {f"table_{k}": v for k, v in tables.items()}
    out["actions"] = torch.stack(env.actions).numpy()
    out["scalar_tags"] = np.array(sorted(Recorder.scalars))
    out["scalars"] = np.array([Recorder.scalars[t] for t in sorted(Recorder.scalars)], dtype=np.float64)
    out["saved_files"] = np.array(saved)
    out["torch_version"] = np.array(torch.__version__)
    for k, v in sd.items():
        if v.size <= 2048:
            out["sd/" + k] = v
        else:
            out["head/" + k] = v[:4]
            out["sum/" + k] = np.array([v.astype(np.float64).sum(), np.square(v.astype(np.float64)).sum()])
    np.savez_compressed(OUT / "ref_cleanrl_ppo.npz", **out)


def main():
    install_stubs()
    ref = _load("biped_tasks.utils.cleanrl.ppo", REF / "utils/cleanrl/ppo.py")
    gen_rms(ref)
    gen_agent(ref)
    gen_ppo(ref)
    for f in ("ref_cleanrl_rms.npz", "ref_cleanrl_agent.json", "ref_cleanrl_ppo.npz"):
        print(f, (OUT / f).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
