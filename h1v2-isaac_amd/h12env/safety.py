"""Deployment safety report of the batched sim2sim run.

Device side: SafetyMonitor binds the per-substep monitor of the MuJoCo-mode physics loop
(h12env_step_physics_monitored, h12env_monitor_reduce) -- for every env and every 1 kHz substep the joint-limit,
torque, velocity and foot-force statistics the reference gathers for one robot with its MJLogger
(biped_deploy/utils/mj_logger.py) and evaluates with biped_deploy/eval/{safety_checker,eval_policy}.py.

Host side: check_safety / extract_data / check_position_limits restate those two evaluators for a metrics.json
(ours or the reference's), record for record and number for number; metrics_from_trace writes the monitor's trace in
MJLogger's schema; fold_monitor_host / summary_from_words restate the reduce kernel for canned data.

Two deviations of the recorded foot force from MuJoCo's: it is the norm of the foot's NET
contact force (MJLogger sums the norms of the individual contacts), and it is the force of the substep just
integrated (MJLogger reads the contacts of the previous mj_step's constraint solve, one substep older).
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from pathlib import Path

import numpy as np

from . import _abi
from ._abi import MON, MON_COUNTS, MON_PREV, MON_SUMS, MON_WORDS, SUM_EXTRA, SUM_WORDS, TRACE, TRACE_WORDS

FOOT_NAMES = ["left_ankle_roll_link", "right_ankle_roll_link"]
JOINT_FIELDS = ("POS_VIOL_COUNT", "POS_EXCESS_MAX", "TAU_ABS_MAX", "TAU_SAT_COUNT", "QD_ABS_MAX", "QD_VIOL_COUNT",
                "TAU_RATE_SUM", "TAU_RATE_MAX", "Q_RATE_SUM", "Q_RATE_MAX")
FOOT_FIELDS = ("FORCE_MAX", "FORCE_SUM", "FORCE_VIOL_COUNT")


def _joint_names():
    from .model import joint_names

    return joint_names()


def model_limits() -> dict:
    """MJLogger.record_limits: the joint ranges and the robot's weight (total mass x g)."""
    from .model import build_model

    m = build_model()
    names = _joint_names()
    return {"joint_pos_limits": {n: [float(m.q_lower[j]), float(m.q_upper[j])] for j, n in enumerate(names)},
            "total_mass_force": float((m.base_mass + sum(m.link_mass)) * m.gravity)}


# ------------------------------------------------------------------------------------------------ host evaluators
def _load(metrics):
    if isinstance(metrics, (str, os.PathLike)):
        with open(metrics) as f:
            return json.load(f)
    return metrics


def check_safety(metrics) -> list[dict]:
    """SafetyChecker.check_safety on a metrics.json (path or loaded list): record 0 holds the limits; every later
    record yields one "position" violation per joint outside its inclusive range and one "contact_force" violation per
    foot whose force exceeds total_mass_force, in record order, joints before feet, each in the record's key order.
    Returns the violations as the dicts SafetyChecker.save_data writes."""
    data = _load(metrics)
    pos_limits = data[0]["joint_pos_limits"]
    weight = data[0]["total_mass_force"]
    out = []
    for rec in data[1:]:
        t = rec["timestamp"]
        for joint, q in rec["joint_pos"].items():
            lo, hi = pos_limits[joint][0], pos_limits[joint][1]
            if not (lo <= q <= hi):
                out.append({"timestamp": t, "joint_name": joint, "check_type": "position", "value": q,
                            "limit": pos_limits[joint], "additional_info": {"lower_limit": lo, "upper_limit": hi}})
        for foot, force in rec["foot_contact_forces"].items():
            if force > weight:
                out.append({"timestamp": t, "joint_name": foot, "check_type": "contact_force", "value": force,
                            "limit": weight, "additional_info": {}})
    return out


def _rates(records, key):
    peak, total = {}, {}
    for rec in records:
        for joint, r in rec[key].items():
            a = abs(r)
            total[joint] = total.get(joint, 0) + a
            if joint not in peak:
                peak[joint] = 0
            if a > peak[joint]:
                peak[joint] = a
    for joint in total:
        total[joint] /= len(records)  # over all records, also those that lack the joint (as the reference)
    return peak, total


def extract_data(metrics) -> dict:
    """eval_policy.extract_data on a metrics.json: max / average foot force (left + right, over the records where
    either is non-zero) and the per-joint max / average |action_rate| and |joint_pos_rate|.

    "max_force" is the reference's number, not a maximum: when a record's left + right exceeds the value kept so far,
    the reference assigns it the RUNNING TOTAL of the forces (`max_force = total_force`).  That assignment is the
    reference's behaviour and is reproduced here so that both tools print the same table for the same file; the true
    maximum is what the batch summary reports (SafetyMonitor.summary()["force_pair_max"])."""
    records = _load(metrics)[1:]
    ref_max, total, count = 0, 0, 0
    for rec in records:
        left = rec["foot_contact_forces"].get(FOOT_NAMES[0], 0)
        right = rec["foot_contact_forces"].get(FOOT_NAMES[1], 0)
        if left == 0 and right == 0:
            continue
        both = left + right
        total += both
        if both > ref_max:
            ref_max = total  # the reference's behaviour (see the docstring)
        count += 1
    max_ar, avg_ar = _rates(records, "action_rate")
    max_pr, avg_pr = _rates(records, "joint_pos_rate")
    return {"max_force": ref_max, "avg_force": total / count if count > 0 else 0, "max_action_rate": max_ar,
            "avg_action_rate": avg_ar, "max_pos_rate": max_pr, "avg_pos_rate": avg_pr}


def check_position_limits(violations) -> dict:
    """eval_policy.check_position_limits on a safety_check.json (path or list): position violations per joint."""
    counts = {}
    for v in _load(violations):
        if v["check_type"] == "position":
            counts[v["joint_name"]] = counts.get(v["joint_name"], 0) + 1
    return counts


# ------------------------------------------------------------------------------------------------ trace -> MJLogger
def metrics_from_trace(trace: np.ndarray, dt: float, limits: dict | None = None, names=None, t0: float = 0.0) -> list:
    """The MJLogger metrics.json records (Limits, then one Metrics per substep) of one env's trace
    ([substeps][TRACE_WORDS] fp32, the monitor's records): real torques and foot forces; action_rate / joint_pos_rate
    are the signed differences to the previous record (0 on the first), as MJLogger.record_metrics computes them."""
    names = list(names) if names is not None else _joint_names()
    trace = np.asarray(trace, np.float32).reshape(-1, TRACE_WORDS)
    out = [dict(limits if limits is not None else model_limits())]
    f = lambda name: trace[:, TRACE[name][0]:TRACE[name][0] + TRACE[name][1]].astype(np.float64)  # noqa: E731
    pos, quat, vlin, wang, q, qd, tau, force = (f(k) for k in ("POS", "QUAT", "VLIN", "WANG", "Q", "QD", "TAU", "FORCE"))
    for k in range(trace.shape[0]):
        p = max(k - 1, 0)
        out.append({
            "timestamp": float(t0 + (k + 1) * dt),
            "base_lin_pos": pos[k].tolist(), "base_quat_pos": quat[k].tolist(),
            "joint_pos": {n: float(q[k, j]) for j, n in enumerate(names)},
            "base_lin_vel": vlin[k].tolist(), "base_quat_vel": wang[k].tolist(),
            "joint_vel": {n: float(qd[k, j]) for j, n in enumerate(names)},
            "applied_torques": {n: float(tau[k, j]) for j, n in enumerate(names)},
            "foot_contact_forces": {n: float(force[k, i]) for i, n in enumerate(FOOT_NAMES)},
            "action_rate": {n: float(tau[k, j] - tau[p, j]) for j, n in enumerate(names)},
            "joint_pos_rate": {n: float(q[k, j] - q[p, j]) for j, n in enumerate(names)},
        })
    return out


# ------------------------------------------------------------------------------------------------ summary
def _kind(name: str) -> str:
    return "count" if name in MON_COUNTS else "sum" if name in MON_SUMS else "zero" if name in MON_PREV else "max"


def fold_monitor_host(mon: np.ndarray) -> np.ndarray:
    """Host restatement of h12env_monitor_reduce: [MON_WORDS][n] 32-bit words -> SUM_WORDS 8-byte words (int64 view;
    maxima / sums hold a double's bits).  Sums use math.fsum (the kernel's blocked fp64 sum agrees to ~1e-13)."""
    mon = np.ascontiguousarray(mon).view(np.int32).reshape(MON_WORDS, -1)
    out = np.zeros(SUM_WORDS, np.int64)
    dbl = out.view(np.float64)
    for name, (off, cnt) in MON.items():
        kind = _kind(name)
        for w in range(off, off + cnt):
            if kind == "count":
                out[w] = int(mon[w].astype(np.int64).sum())
            elif kind == "max":
                dbl[w] = float(mon[w].view(np.float32).max())
            elif kind == "sum":
                dbl[w] = math.fsum(mon[w].view(np.float32).astype(np.float64).tolist())
    any_of = lambda name: (mon[MON[name][0]:MON[name][0] + MON[name][1]] != 0).any(axis=0)  # noqa: E731
    pv, fv, vv = any_of("POS_VIOL_COUNT"), any_of("FORCE_VIOL_COUNT"), any_of("QD_VIOL_COUNT")
    out[SUM_EXTRA["ENVS_POS_VIOL"]] = int(pv.sum())
    out[SUM_EXTRA["ENVS_FORCE_VIOL"]] = int(fv.sum())
    out[SUM_EXTRA["ENVS_VEL_VIOL"]] = int(vv.sum())
    out[SUM_EXTRA["ENVS_ANY_VIOL"]] = int((pv | fv | vv).sum())
    out[SUM_EXTRA["ENVS"]] = mon.shape[1]
    return out


def summary_from_words(words: np.ndarray, names=None) -> dict:
    """The report dict of a summary record (SUM_WORDS 8-byte words), keyed by joint and foot name.  Rates are averaged
    over all recorded substeps (eval_policy.extract_rate), foot forces over all substeps, the left + right force over
    the substeps with contact (eval_policy.extract_contact_force); force_pair_max is the true maximum."""
    names = list(names) if names is not None else _joint_names()
    words = np.ascontiguousarray(words, np.int64).reshape(SUM_WORDS)
    dbl = words.view(np.float64)

    def val(name, i):
        w = MON[name][0] + i
        return int(words[w]) if _kind(name) == "count" else float(dbl[w])

    sub = val("SUBSTEPS", 0)
    con = val("CONTACT_SUBSTEPS", 0)
    envs = int(words[SUM_EXTRA["ENVS"]])
    div = lambda a, b: a / b if b > 0 else 0.0  # noqa: E731
    joints = {}
    for j, n in enumerate(names):
        d = {f.lower(): val(f, j) for f in JOINT_FIELDS}
        d["tau_rate_avg"] = div(d.pop("tau_rate_sum"), sub)
        d["q_rate_avg"] = div(d.pop("q_rate_sum"), sub)
        joints[n] = d
    feet = {}
    for i, n in enumerate(FOOT_NAMES):
        d = {f.lower(): val(f, i) for f in FOOT_FIELDS}
        d["force_avg"] = div(d.pop("force_sum"), sub)
        feet[n] = d
    out = {"num_envs": envs, "substeps": sub, "contact_substeps": con, "joints": joints, "feet": feet,
           "force_pair_avg": div(val("FORCE_PAIR_SUM", 0), con), "force_pair_max": val("FORCE_PAIR_MAX", 0)}
    for k, w in SUM_EXTRA.items():
        if k != "ENVS":
            out[k.lower()] = int(words[w])
    out["share_any_viol"] = div(out["envs_any_viol"], envs)
    return out


# ------------------------------------------------------------------------------------------------ device monitor
class SafetyMonitor:
    """Per-env safety accumulators of env.step_physics(q_ref, n, monitor=self), kept on the device.

    trace_envs: the first k envs also keep every substep's raw record (for metrics.json).  force_limit: foot-force
    violation threshold [N], default total mass x g (MJLogger.record_limits).  vel_limit: |qd| violation threshold, a
    scalar or 12 values [rad/s]; None / 0 = not counted."""

    def __init__(self, env, trace_envs: int = 0, force_limit: float | None = None, vel_limit=None):
        import torch

        self.env = env
        self.n = env.num_envs
        self.n_trace = int(trace_envs)
        self.names = _joint_names()
        self.limits = model_limits()
        self.force_limit = float(self.limits["total_mass_force"] if force_limit is None else force_limit)
        vel = np.zeros(12, np.float32) if vel_limit is None else np.broadcast_to(np.asarray(vel_limit, np.float32), (12,))
        lib = env._lib
        sz = [C.c_size_t() for _ in range(3)]
        _abi.check(lib, lib.h12env_monitor_layout(self.n, self.n_trace, 0, *(C.byref(s) for s in sz)),
                   "h12env_monitor_layout")
        assert sz[0].value == MON_WORDS * self.n * 4
        self._mon = torch.zeros(MON_WORDS, self.n, dtype=torch.int32, device=env.device)
        self._limits = torch.from_numpy(np.concatenate([vel, [self.force_limit]]).astype(np.float32)).to(env.device)
        self._summary = torch.zeros(sz[2].value // 8, dtype=torch.int64, device=env.device)
        self._trace: list = []   # one [n_substeps][n_trace][TRACE_WORDS] tensor per monitored call
        self.dt = float(env.cfg.sim.dt)

    # called by H12VelocityEnv.step_physics
    def _step(self, env, q, n_substeps: int):
        import torch

        if env is not self.env:
            raise ValueError("this SafetyMonitor belongs to another env")
        tr = None
        if self.n_trace > 0 and n_substeps > 0:
            tr = torch.empty(n_substeps, self.n_trace, TRACE_WORDS, dtype=torch.float32, device=env.device)
            self._trace.append(tr)
        lib = env._lib
        _abi.check(lib, lib.h12env_step_physics_monitored(
            env._h, C.c_void_p(q.data_ptr()), n_substeps, C.c_void_p(self._mon.data_ptr()),
            C.c_void_p(self._limits.data_ptr()), C.c_void_p(tr.data_ptr()) if tr is not None else None, 0,
            self.n_trace if tr is not None else 0, env._stream()), "h12env_step_physics_monitored")

    def reset(self, mask=None):
        """Zero the accumulators (and the "previous record": the next record has rate 0) of the envs flagged in mask
        (bool, N), or of all envs -- which also drops the trace."""
        if mask is None:
            self._mon.zero_()
            self._trace.clear()
        else:
            self._mon[:, mask.to(device=self._mon.device, dtype=bool)] = 0

    def per_env(self) -> dict:
        """Named zero-copy views of the accumulators: (12, N) per joint field, (2, N) per foot field, (N,) per env
        field; counts int32, everything else float32."""
        import torch

        out = {}
        for name, (off, cnt) in MON.items():
            v = self._mon[off:off + cnt]
            v = v if name in MON_COUNTS else v.view(torch.float32)
            out[name.lower()] = v[0] if cnt == 1 else v
        return out

    def summary_words(self):
        """Run the reduce kernel; the summary record as a device int64 tensor (SUM_WORDS)."""
        lib = self.env._lib
        _abi.check(lib, lib.h12env_monitor_reduce(self.env._h, C.c_void_p(self._mon.data_ptr()),
                                                  C.c_void_p(self._summary.data_ptr()), self.env._stream()),
                   "h12env_monitor_reduce")
        return self._summary[:SUM_WORDS]

    def summary(self) -> dict:
        d = summary_from_words(self.summary_words().cpu().numpy(), self.names)
        d["force_limit"] = self.force_limit
        return d

    def trace(self) -> np.ndarray:
        """[substeps][n_trace][TRACE_WORDS] fp32: the traced envs' records since the last reset()."""
        import torch

        if not self._trace:
            return np.zeros((0, self.n_trace, TRACE_WORDS), np.float32)
        return torch.cat(self._trace, dim=0).cpu().numpy()

    def trace_metrics(self) -> list:
        """Per traced env the MJLogger metrics.json records (Limits, then one Metrics per 1 kHz substep)."""
        tr = self.trace()
        return [metrics_from_trace(tr[:, i], self.dt, self.limits, self.names) for i in range(self.n_trace)]


def write_env_logs(log_dir, index: int, metrics: list) -> tuple[Path, Path]:
    """env_<i>/metrics.json and env_<i>/safety_check.json (the reference's two files) for one traced env."""
    d = Path(log_dir) / f"env_{index}"
    d.mkdir(parents=True, exist_ok=True)
    (d / "metrics.json").write_text(json.dumps(metrics, indent=2))
    (d / "safety_check.json").write_text(json.dumps(check_safety(metrics), indent=2))
    return d / "metrics.json", d / "safety_check.json"
