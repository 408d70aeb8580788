"""Table-driven CPU stand-in for a CaT env with the surface the CleanRL PPO uses (test double; the H1-2 env itself
needs the MI355X): observations, rewards, soft dones (fractional termination probabilities) and time-outs are read
from fixed tables, step after step, whatever the actions are; the actions received are recorded.  Also the seeded
``layer_init`` replacement the CleanRL fixture was generated with, so initial weights can be rebuilt anywhere."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

NUM_ENVS, OBS_DIM, ACT_DIM = 8, 6, 12


def make_tables(steps: int, seed: int = 7, num_envs: int = NUM_ENVS, obs_dim: int = OBS_DIM) -> dict:
    rs = np.random.RandomState(seed)
    offs = np.array([0.0, 3.0, -20.0, 0.5, 100.0, -1.0])[:obs_dim]
    scale = np.array([1.0, 0.1, 5.0, 2.0, 0.5, 1.0])[:obs_dim]
    obs = (offs + scale * rs.standard_normal((steps + 1, num_envs, obs_dim))).astype(np.float32)
    rew = (0.5 + 0.5 * rs.standard_normal((steps, num_envs))).astype(np.float32)
    dones = (0.3 * rs.uniform(size=(steps, num_envs)) ** 2).astype(np.float32)
    dones[rs.uniform(size=dones.shape) < 0.1] = 1.0
    timeouts = rs.uniform(size=(steps, num_envs)) < 0.15
    return {"obs": obs, "rew": rew, "dones": dones, "timeouts": timeouts}


class ToyCaTEnv:
    def __init__(self, tables: dict | None = None, cfg=None, render_mode=None, **kw):
        self.cfg = cfg
        n = int(cfg.scene.num_envs) if cfg is not None else NUM_ENVS
        t = tables if tables is not None else make_tables(64, num_envs=n)
        self.t = {k: torch.from_numpy(np.asarray(v)) for k, v in t.items()}
        self.steps = self.t["rew"].shape[0]
        self.num_envs = self.t["rew"].shape[1]
        self.device = torch.device("cpu")
        self.single_observation_space = {"policy": SimpleNamespace(shape=(self.t["obs"].shape[2],))}
        self.single_action_space = SimpleNamespace(shape=(ACT_DIM,))
        self.k = 0
        self.actions: list = []
        self.closed = False

    @property
    def unwrapped(self):
        return self

    def reset(self, seed=None, options=None):
        self.k = 0
        return {"policy": self.t["obs"][0].clone()}, {}

    def step(self, action):
        assert action.shape == (self.num_envs, ACT_DIM)
        self.actions.append(action.detach().clone())
        k = self.k % self.steps
        self.k += 1
        rew = self.t["rew"][k].clone()
        info = {"log": {"Episode_Reward/toy": rew.mean(), "Metrics/k": float(k)}}
        return ({"policy": self.t["obs"][k + 1].clone()}, rew, self.t["dones"][k].clone(),
                self.t["timeouts"][k].clone(), info)

    def close(self):
        self.closed = True


class SeededInit:
    """layer_init(layer, std, bias_const) with weights from numpy.random.RandomState(k), k the call index:
    N(0, 1) * std / sqrt(fan_in), bias = bias_const."""

    def __init__(self):
        self.k = 0

    def __call__(self, layer, std=np.sqrt(2), bias_const=0.0):
        rs = np.random.RandomState(self.k)
        self.k += 1
        shape = tuple(layer.weight.shape)
        w = rs.standard_normal(shape).astype(np.float32) * np.float32(std / np.sqrt(shape[1]))
        with torch.no_grad():
            layer.weight.copy_(torch.from_numpy(w))
            layer.bias.fill_(bias_const)
        return layer


def toy_ppo_cfg(**kw):
    """The PPO settings of tests/golden/ref_cleanrl_ppo.npz."""
    c = dict(seed=11, logger="tensorboard", learning_rate=1.0e-3, num_steps=4, num_iterations=2, gamma=0.99,
             gae_lambda=0.95, updates_epochs=2, minibatch_size=16, clip_coef=0.2, ent_coef=0.0081, vf_coef=2.0,
             max_grad_norm=1.0, norm_adv=True, clip_vloss=True, anneal_lr=True, save_interval=2)
    c.update(kw)
    return SimpleNamespace(**c)
