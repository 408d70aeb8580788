"""The mirror map checked against the physics (tests/test_symmetry.py on the CPU oracle, tests/test_gpu_symmetry.py on
the HIP env): envs in pairs (A, B) that start in one mirror-symmetric state, B's command the mirror image of A's, B's
actions the mirror image of A's.  Then obs_B is the mirror image of obs_A up to the model's own asymmetry (the welded
upper body), and for every column j of the newest frame the table's (source column, sign) must be, among all the
(column of the same term, sign) candidates, the one that reproduces obs_B[j] from obs_A -- by a wide margin."""
from __future__ import annotations

import numpy as np
import torch

from h12env import symmetry as S
from h12env.cfg import H12FlatEnvCfg, H12RoughEnvCfg

N_ENVS = 16
K_STEPS = 2          # the pairs drift apart with every contact: 0.0053 at K = 2, 0.046 at K = 4 on the oracle
ACTION_STD = 0.3
SEED = 1
MARGIN = 0.1         # the table's entry against the best other candidate
WIDTHS = {"base_lin_vel": 3, "base_ang_vel": 3, "projected_gravity": 3, "velocity_commands": 3, "joint_pos": 12,
          "joint_vel": 12, "actions": 12, "height_scan": 187}
CMD_MIRROR = np.array([[1.0], [-1.0], [-1.0]], np.float32)  # (vx, -vy, -wz)


def pair_cfg(layout: str, device: str | None = None):
    """Flat, or the Rough layout on the plane (its flat fallback: base_lin_vel in the row, a constant scan)."""
    cfg = H12FlatEnvCfg() if layout == "flat" else H12RoughEnvCfg()
    if layout != "flat":
        cfg.scene.terrain.terrain_type = "plane"
        cfg.curriculum.terrain_levels = False
        # the Rough task commands vy = 0, and a column that is zero in every env cannot show its sign
        cfg.commands.base_velocity.ranges.lin_vel_y = (-0.5, 0.5)
    cfg.scene.num_envs = N_ENVS
    if device is not None:
        cfg.sim.device = device
    cfg.observations.policy.enable_corruption = False
    cfg.events.reset_base_pose_range = {"x": (0.0, 0.0), "y": (0.0, 0.0), "yaw": (0.0, 0.0)}
    cfg.events.push_robot = None
    for g in cfg.robot.actuators.values():
        g.min_delay = g.max_delay = 2
    cfg.commands.base_velocity.heading_command = False
    cfg.commands.base_velocity.rel_standing_envs = 0.0
    return cfg


def mirror_commands(cmd):
    """In place on the (3, n) command rows of the workspace (numpy or torch): odd envs get the even envs' mirror."""
    m = CMD_MIRROR if isinstance(cmd, np.ndarray) else torch.from_numpy(CMD_MIRROR).to(cmd.device)
    cmd[:, 1::2] = cmd[:, 0::2] * m


def paired_actions():
    """K_STEPS x (N_ENVS, 12): N(0, 0.3) in the even envs, mirror_actions of them in the odd ones."""
    rng = np.random.default_rng(SEED)
    out = []
    for _ in range(K_STEPS):
        a = rng.normal(0.0, ACTION_STD, (N_ENVS // 2, 12)).astype(np.float32)
        act = np.empty((N_ENVS, 12), np.float32)
        act[0::2] = a
        act[1::2] = S.mirror_actions(torch.from_numpy(a)).numpy()
        out.append(act)
    return out


def identify(table: S.MirrorTable, terms, history: int, obs_a: np.ndarray, obs_b: np.ndarray, skip=("height_scan",)):
    """(misidentified columns, worst ratio) over the newest-slot columns of ``terms``: for column j every (source
    column s of the same term's newest slot, sign) is scored by sum |sign * obs_a[:, s] - obs_b[:, j]|; the table's
    entry must score lowest, and at most MARGIN x the best other score."""
    h = max(1, int(history or 0))
    off, bad, worst, seen = 0, [], 0.0, 0
    for name in terms:
        w = WIDTHS[name]
        new = off + (h - 1) * w
        off += h * w
        if name in skip:
            continue
        for j in range(new, new + w):
            score = {}
            for s in range(new, new + w):
                for neg in (False, True):
                    score[(s, neg)] = float(np.abs((-1.0 if neg else 1.0) * obs_a[:, s] - obs_b[:, j]).sum())
            mine = (int(table.src[j]), bool(table.flip[j]))
            other = min(v for k, v in score.items() if k != mine)
            ok = mine in score and other > 0 and score[mine] <= MARGIN * other  # a constant column identifies nothing
            worst = max(worst, score.get(mine, np.inf) / other if other > 0 else np.inf)
            if not ok:
                bad.append((name, j - new, mine, score.get(mine), other))
            seen += 1
    assert off == table.width
    return bad, worst, seen
