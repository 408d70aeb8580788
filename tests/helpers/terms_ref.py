"""Plain numpy restatement of the 20 reward terms of REWARD_FUNCS, `terminated` and `time_out`, one env at a time,
written from the formulas (the Rsl table of rsl_env_cfg.py:279-441 and the IsaacLab
definitions it names); it shares no code with csrc/h12env.hip or oracle/h12_oracle.c.  `dtype` switches every
operation between float64 (the reference) and float32 (the definition's own rounding sensitivity, from which the
GPU gates are derived).  The planted rows the CPU and GPU tests evaluate are built here too (`planted_rows`).

Conventions: the state is 37 numbers (pos, quat wxyz, world linear velocity of the base origin, BODY-frame angular
velocity, q, qd); the root linear velocity is the pelvis body's COM velocity v + (R w) x (R root_com); joint ranges,
defaults, link COMs and root_com are the float32 values of the model struct; thresholds come from cfg.to_c().

    terms, terminated, time_out, info = evaluate(K, row, dtype=np.float64, slide="fd", mut=None)

`mut` names one planted misreading (MUTATIONS): the discrimination test applies each and requires the row set to
catch it at the GPU gate."""
from __future__ import annotations

import re
from dataclasses import dataclass, replace
from pathlib import Path

import numpy as np

from h12env._abi import NJ, NREW, NREW_FLAT, REWARD_FUNCS
from h12env.model import build_model, model_dict
from render_reference import fk

RID = {f: i for i, f in enumerate(REWARD_FUNCS)}
KERNEL_SRC = Path(__file__).resolve().parents[2] / "h1v2-isaac_amd" / "csrc" / "h12env.hip"
FD_STEP = 1e-5          # central-difference step (s) of the foot COM velocity, method (a)
EPS64, EPS32, TINY32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps), float(np.finfo(np.float32).tiny)

# joint groups by name, as the reward tables give them (rough_env_cfg.py:52-62, rsl_env_cfg.py:343-386)
GROUPS = {
    "joint_pos_limits:ankle": [r".*_ankle_roll_joint", r".*_ankle_pitch_joint"],
    "joint_pos_limits:hip": [r".*_hip_yaw_joint", r".*_hip_roll_joint"],
    "joint_deviation_l1:hip": [r".*_hip_yaw_joint", r".*_hip_roll_joint"],
    "joint_deviation_l1:ankle": [r".*_ankle_roll_joint", r".*_ankle_pitch_joint"],
}
PAIR_SUMS = ["joint_torques_l2", "joint_acc_l2", "action_rate_l2", "joint_pos_limits:ankle", "feet_slide",
             "joint_deviation_l1:hip", "joint_vel_l2", "joint_deviation_l1:ankle", "joint_pos_limits:hip",
             "contact_forces"]
# single misreadings a shared reading of the table could hide (ISSUE list).  `>=` for `>` is listed for the switches
# whose value jumps; contact_forces and the soft limits are continuous at their thresholds (max(x - t, 0)), where the
# two comparisons give the same value and no test can tell them apart.
MUTATIONS = (["base_frame_for_yaw_frame", "origin_velocity", "body_wz_for_world_wz", "world_wz_for_body_wz",
              "soft_factor_one", "hip_roll_from_index_1", "clip_of_summed_force"]
             + ["drop_right:" + f for f in PAIR_SUMS]
             + ["ge:feet_slide", "ge:knee", "ge:torso", "ge:div_w", "ge:div_v", "ge:in_contact", "gt:time_out"])


@dataclass(frozen=True)
class Consts:
    model: dict
    names: tuple
    q_lower: np.ndarray
    q_upper: np.ndarray
    q_default: np.ndarray
    link_com: np.ndarray
    root_com: np.ndarray
    track_std: float
    air_time_threshold: float
    soft_limit_factor: float
    contact_threshold: float
    contact_force_threshold: float
    base_height_target: float
    max_episode_length: int
    illegal_contact_knees: bool
    illegal_contact_torso: bool
    div_w: float
    div_v: float
    rsl_on: bool      # a weight on any of the terms 12-19: the table that holds them is in use


def divergence_limits():
    m = re.search(r"H12_DIV_W\s*=\s*([0-9.]+)f?\s*,\s*H12_DIV_V\s*=\s*([0-9.]+)f?", KERNEL_SRC.read_text())
    return float(m.group(1)), float(m.group(2))


def consts(cfg) -> Consts:
    c, m, d = cfg.to_c(), build_model(), model_dict()
    f32 = lambda a: np.array([float(x) for x in a], dtype=np.float32)  # noqa: E731
    dw, dv = divergence_limits()
    return Consts(
        model=d, names=tuple(d["joint_names"]), q_lower=f32(m.q_lower), q_upper=f32(m.q_upper),
        q_default=f32(m.q_default), link_com=np.array([[float(x) for x in r] for r in m.link_com], dtype=np.float32),
        root_com=f32(m.root_com), track_std=float(c.track_std), air_time_threshold=float(c.air_time_threshold),
        soft_limit_factor=float(c.soft_limit_factor), contact_threshold=float(c.contact_threshold),
        contact_force_threshold=float(c.contact_force_threshold), base_height_target=float(c.base_height_target),
        max_episode_length=int(c.max_episode_length), illegal_contact_knees=bool(c.illegal_contact_knees),
        illegal_contact_torso=bool(c.illegal_contact_torso), div_w=dw, div_v=dv,
        rsl_on=any(float(c.rew_w[t]) != 0.0 for t in range(NREW_FLAT, NREW)))


def group(K: Consts, func: str):
    return [j for j, n in enumerate(K.names) if any(re.fullmatch(p, n) for p in GROUPS[func])]


def chain(f: int):
    return range(6 * f, 6 * f + 6)   # the six joints from the pelvis to foot f (0 left, 1 right)


# ------------------------------------------------------------------ foot COM velocity
def _foot_com(K, pos, quat, q, T):
    R, p = fk(K.model, pos, quat, q, dtype=T)
    return [p[6 * f + 6] + R[6 * f + 6] @ K.link_com[6 * f + 5].astype(T) for f in range(2)]


def _advance(state, h):
    """The state after time h under its own constant twist and joint rates: the base origin moves along v, the
    attitude is right-multiplied by the body-frame increment, the joints move along qd."""
    s = np.asarray(state, np.float64)
    pos, qt, v, w, q, qd = s[0:3], s[3:7] / np.linalg.norm(s[3:7]), s[7:10], s[10:13], s[13:25], s[25:37]
    th = np.linalg.norm(w) * h
    ax = w / np.linalg.norm(w) if th != 0 else np.zeros(3)
    dq = np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * ax])
    a, b = qt, dq
    qn = np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])
    return pos + h * v, qn, q + h * qd


def foot_vel_fd(K, state, h=FD_STEP):
    """(a) central finite difference of the foot-link COM position, float64: (2, 3)."""
    cp = _foot_com(K, *_advance(state, h), np.float64)
    cm = _foot_com(K, *_advance(state, -h), np.float64)
    return np.array([(cp[f] - cm[f]) / (2 * h) for f in range(2)])


def fd_error_bound(K, state, h=FD_STEP):
    """Bound on |foot_vel_fd - truth| per foot.  The COM position is pos(t) + R0(t)(a0 + R1(t)(a1 + ...)) with every
    rotation turning at a constant rate about a fixed axis, so each time derivative multiplies the chain by at most
    W = |w| + sum |qd| of the leg and |p'''| <= W^3 L with L the summed offsets; the central difference truncates
    h^2/6 p'''.  Rounding: each of the two positions carries C eps64 (|pos| + L) (C = 32 covers the eight chained
    3x3 products and the quaternion normalisation), divided by 2h each."""
    s = np.asarray(state, np.float64)
    out = []
    for f in range(2):
        L = sum(np.linalg.norm(np.asarray(K.model["joints"][j]["pos"])) for j in chain(f)) + \
            np.linalg.norm(K.link_com[6 * f + 5])
        W = np.linalg.norm(s[10:13]) + np.abs(s[25 + 6 * f:31 + 6 * f]).sum()
        out.append(h * h * W ** 3 * L / 6 + 32 * EPS64 * (np.linalg.norm(s[0:3]) + h * np.linalg.norm(s[7:10]) + L) / h)
    return np.array(out)


def foot_vel_jac(K, state, T=np.float64):
    """(b) the same velocity from FK positions and joint axes (geometric Jacobian), in dtype T: (2, 3)."""
    s = np.asarray(state).astype(T)
    R, p = fk(K.model, s[0:3], s[3:7], s[13:25], dtype=T)
    ww = R[0] @ s[10:13]
    out = []
    for f in range(2):
        c = p[6 * f + 6] + R[6 * f + 6] @ K.link_com[6 * f + 5].astype(T)
        v = s[7:10] + np.cross(ww, c - p[0])
        for j in chain(f):
            axis_w = R[j + 1][:, int(K.model["joints"][j]["axis"])]
            v = v + s[25 + j] * np.cross(axis_w, c - p[j + 1])
        out.append(v)
    return np.array(out, dtype=T)


# ------------------------------------------------------------------ the terms
def evaluate(K: Consts, row: dict, dtype=np.float64, slide="fd", mut=None):
    T = dtype
    A = lambda k: np.asarray(row[k], np.float64).astype(T)  # noqa: E731
    s = A("state")
    pos, quat, v, wb, q, qd = s[0:3], s[3:7], s[7:10], s[10:13], s[13:25], s[25:37]
    act, act_prev, cmd, air, con, tau, jacc, fmax = (A(k) for k in
                                                     ("act", "act_prev", "cmd", "air", "con", "tau", "jacc", "fmax"))
    ffoot, fknee, ftorso = fmax[0:2], fmax[2:4], fmax[4]
    branch = []

    def gt(x, y, name=None):   # every switch goes through here: `>` unless the mutation says otherwise
        r = bool(x >= y) if (name is not None and mut == "ge:" + name) else bool(x > y)
        branch.append(r)
        return r

    right = lambda func: 0.0 if mut == "drop_right:" + func else 1.0  # noqa: E731
    legw = lambda func: np.array([1.0] * 6 + [right(func)] * 6).astype(T)  # noqa: E731

    # terminations: illegal contact on max_h |F| (threshold from the cfg), divergence guard, time-out
    ill = False
    if K.illegal_contact_knees:
        ill |= any([gt(fknee[f], T(K.contact_threshold), "knee") for f in range(2)])
    if K.illegal_contact_torso:
        ill |= gt(ftorso, T(K.contact_threshold), "torso")
    for a in range(3):
        ill |= (not np.isfinite(wb[a])) or gt(abs(wb[a]), T(K.div_w), "div_w")
        ill |= (not np.isfinite(v[a])) or gt(abs(v[a]), T(K.div_v), "div_v")
    terminated = bool(ill)
    eplen = int(row["eplen"])
    time_out = eplen > K.max_episode_length if mut == "gt:time_out" else eplen >= K.max_episode_length
    branch.append(time_out)

    # base kinematics
    R = fk(K.model, pos, quat, q, dtype=T)[0][0]
    ww = R @ wb
    vcom = v + np.cross(ww, R @ K.root_com.astype(T))
    if mut == "origin_velocity":
        vcom = v
    vb = R.T @ vcom
    yaw = np.arctan2(R[1, 0], R[0, 0])
    cy, sy = np.cos(yaw), np.sin(yaw)
    vyaw = np.array([cy * vcom[0] + sy * vcom[1], -sy * vcom[0] + cy * vcom[1], vcom[2]], dtype=T)
    gb = R.T @ np.array([0, 0, -1], dtype=T)
    std2 = T(K.track_std) * T(K.track_std)

    t = np.zeros(NREW, dtype=T)
    vt = vb if mut == "base_frame_for_yaw_frame" else vyaw
    t[RID["track_lin_vel_xy_yaw_frame_exp"]] = np.exp(-((cmd[0] - vt[0]) ** 2 + (cmd[1] - vt[1]) ** 2) / std2)
    wz = wb[2] if mut == "body_wz_for_world_wz" else ww[2]
    t[RID["track_ang_vel_z_world_exp"]] = np.exp(-((cmd[2] - wz) ** 2) / std2)
    t[RID["ang_vel_xy_l2"]] = wb[0] ** 2 + wb[1] ** 2
    t[RID["joint_torques_l2"]] = (legw("joint_torques_l2") * tau ** 2).sum()
    t[RID["joint_acc_l2"]] = (legw("joint_acc_l2") * jacc ** 2).sum()
    t[RID["action_rate_l2"]] = (legw("action_rate_l2") * (act - act_prev) ** 2).sum()

    # feet_air_time_positive_biped
    inc = [gt(con[f], T(0), "in_contact") for f in range(2)]
    mode_t = [con[f] if inc[f] else air[f] for f in range(2)]
    r = min(mode_t) if (inc[0] + inc[1]) == 1 else T(0)
    r = min(r, T(K.air_time_threshold))
    moving = bool(np.sqrt(cmd[0] ** 2 + cmd[1] ** 2) > T(0.1))
    branch.append(moving)
    t[RID["feet_air_time_positive_biped"]] = r if moving else T(0)

    t[RID["flat_orientation_l2"]] = gb[0] ** 2 + gb[1] ** 2

    factor = T(1.0) if mut == "soft_factor_one" else T(K.soft_limit_factor)
    lo, hi, q0 = K.q_lower.astype(T), K.q_upper.astype(T), K.q_default.astype(T)
    mean, rng_ = (lo + hi) / 2, hi - lo
    soft_lo, soft_hi = mean - T(0.5) * rng_ * factor, mean + T(0.5) * rng_ * factor

    def pick(j):   # the joint a term reads for joint j of its group
        return 6 * (j // 6) + 1 if (mut == "hip_roll_from_index_1" and K.names[j].endswith("_hip_roll_joint")) else j

    def limits(func):
        tot = T(0)
        for j0 in group(K, func):
            j = pick(j0)
            below, above = gt(soft_lo[j], q[j]), gt(q[j], soft_hi[j])
            wgt = T(right(func)) if j0 >= 6 else T(1)
            tot = tot + wgt * ((soft_lo[j] - q[j] if below else T(0)) + (q[j] - soft_hi[j] if above else T(0)))
        return tot

    def deviation(func):
        return sum(((T(right(func)) if j0 >= 6 else T(1)) * abs(q[pick(j0)] - q0[pick(j0)]) for j0 in group(K, func)),
                   T(0))

    t[RID["joint_pos_limits:ankle"]] = limits("joint_pos_limits:ankle")
    t[RID["is_terminated"]] = T(1) if terminated else T(0)

    # feet_slide: |v_xy| of the foot-link COM where the history maximum of |F| exceeds 1 N
    if slide == "fd":
        assert T is np.float64, "the finite difference is the float64 reference"
        fv = foot_vel_fd(K, s)
    else:
        fv = foot_vel_jac(K, s, T)
    sl = T(0)
    for f in range(2):
        if gt(ffoot[f], T(1.0), "feet_slide"):
            sl = sl + (T(right("feet_slide")) if f else T(1)) * np.sqrt(fv[f][0] ** 2 + fv[f][1] ** 2)
    t[RID["feet_slide"]] = sl
    t[RID["joint_deviation_l1:hip"]] = deviation("joint_deviation_l1:hip")

    if K.rsl_on:
        t[RID["track_lin_vel_xy_exp"]] = np.exp(-((cmd[0] - vb[0]) ** 2 + (cmd[1] - vb[1]) ** 2) / std2)
        wzb = ww[2] if mut == "world_wz_for_body_wz" else wb[2]
        t[RID["track_ang_vel_z_exp"]] = np.exp(-((cmd[2] - wzb) ** 2) / std2)
        t[RID["base_height_l2"]] = (pos[2] - T(K.base_height_target)) ** 2
        t[RID["joint_vel_l2"]] = (legw("joint_vel_l2") * qd ** 2).sum()
        t[RID["joint_deviation_l1:ankle"]] = deviation("joint_deviation_l1:ankle")
        t[RID["joint_pos_limits:hip"]] = limits("joint_pos_limits:hip")
        thr = T(K.contact_force_threshold)
        if mut == "clip_of_summed_force":   # one clip of the summed force where each foot is clipped on its own
            cf = max(ffoot[0] + ffoot[1] - thr, T(0))
        else:
            cf = sum(((T(right("contact_forces")) if f else T(1)) * (ffoot[f] - thr if gt(ffoot[f], thr) else T(0))
                      for f in range(2)), T(0))
        t[RID["contact_forces"]] = cf
        t[RID["lin_vel_z_l2"]] = vb[2] ** 2
    info = dict(branch=tuple(branch), vyaw=vyaw, vb=vb, ww=ww, soft_lo=soft_lo, soft_hi=soft_hi)
    return t, terminated, bool(time_out), info


# ------------------------------------------------------------------ symmetries (the restatement's own checks)
def mirror_row(row: dict) -> dict:
    """The row reflected through the pelvis xz-plane (y -> -y): legs swapped, yaw / roll joints negated."""
    s = np.asarray(row["state"], np.float64)
    js = np.array([-1, 1, -1, 1, 1, -1] * 2, dtype=np.float64)   # yaw (z) and roll (x) axes flip, pitch (y) does not
    sw = lambda a: (js * np.asarray(a, np.float64))[np.r_[6:12, 0:6]]  # noqa: E731
    pos, qt, v, w = s[0:3], s[3:7], s[7:10], s[10:13]
    st = np.concatenate([[pos[0], -pos[1], pos[2]], [qt[0], -qt[1], qt[2], -qt[3]], [v[0], -v[1], v[2]],
                         [-w[0], w[1], -w[2]], sw(s[13:25]), sw(s[25:37])])
    c, f = np.asarray(row["cmd"], np.float64), np.asarray(row["fmax"], np.float64)
    return dict(row, state=st, act=sw(row["act"]), act_prev=sw(row["act_prev"]), tau=sw(row["tau"]),
                jacc=sw(row["jacc"]), cmd=np.array([c[0], -c[1], -c[2]]), air=np.asarray(row["air"])[::-1].copy(),
                con=np.asarray(row["con"])[::-1].copy(), fmax=np.array([f[1], f[0], f[3], f[2], f[4]]))


def mirror_consts(K: Consts) -> Consts:
    """The reflected robot: the model is its own mirror image except for the pelvis COM's y offset."""
    return replace(K, root_com=K.root_com * np.array([1, -1, 1], dtype=np.float32))


def rotate_row(row: dict, angle: float) -> dict:
    """The same env with the world turned about z: position, attitude and world velocity turn, nothing else."""
    s = np.asarray(row["state"], np.float64).copy()
    c, sn = np.cos(angle), np.sin(angle)
    Rz = np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]])
    a, b = np.array([np.cos(angle / 2), 0, 0, np.sin(angle / 2)]), s[3:7]
    s[3:7] = np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])
    s[0:3], s[7:10] = Rz @ s[0:3], Rz @ s[7:10]
    return dict(row, state=s)


# ------------------------------------------------------------------ planted rows
def quat_rpy(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = (f(a / 2) for a in (yaw, pitch, roll) for f in (np.cos, np.sin))
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy])


def _rot(qt):
    return fk({"joints": []}, np.zeros(3), qt, [], dtype=np.float64)[0][0]


def up32(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def planted_rows(K: Consts):
    """Labelled rows, every input rounded to float32 (what the workspace holds).  Smooth rows keep 1e-3 from every
    switch; the rows that sit on a switch use inputs float32 holds exactly (1, the cfg's thresholds, the divergence
    limits and their float32 successors)."""
    rows = []
    q0 = K.q_default.astype(np.float64)

    def add(label, *, pos=(0.3, -0.2, 1.0), quat=(1, 0, 0, 0), v=(0, 0, 0), w=(0, 0, 0), q=None, qd=None, act=None,
            act_prev=None, cmd=(0, 0, 0), air=(0, 0), con=(0, 0), tau=None, jacc=None, fmax=(0, 0, 0, 0, 0), eplen=10):
        z = np.zeros(NJ)
        f = lambda a, d=None: np.asarray(d if a is None else a, np.float64).astype(np.float32).astype(np.float64)  # noqa: E731
        st = np.concatenate([f(pos), f(quat), f(v), f(w), f(q, q0), f(qd, z)])
        rows.append(dict(label=label, state=st, act=f(act, z), act_prev=f(act_prev, z), cmd=f(cmd), air=f(air),
                         con=f(con), tau=f(tau, z), jacc=f(jacc, z), fmax=f(fmax), eplen=int(eplen)))
        return rows[-1]

    def onehot(j, val):
        a = np.zeros(NJ)
        a[j] = val
        return a

    tilts = [(0.0, 0.0), (0.4, -0.6), (-1.0, 0.9)]   # (roll, pitch)
    # --- tracking frames
    for yaw in (0.0, np.pi / 2, -np.pi / 2, np.pi, 0.7):
        for roll, pitch in tilts:
            qt = quat_rpy(yaw, pitch, roll)
            R = _rot(qt)
            Rz = _rot(quat_rpy(yaw, 0, 0))
            for name, vel in (("world_x", np.array([0.8, 0, 0])), ("base_x", 0.8 * R[:, 0]), ("yaw_y", 0.6 * Rz[:, 1])):
                add(f"track/{name}/yaw{yaw:.2f}/r{roll}p{pitch}", quat=qt, v=vel, cmd=(0.5, -0.2, 0.3))
    for roll, pitch, w in ((0, 0, (0, 0, 2.0)), (0.5, -0.7, (0, 0, 2.0)), (0.5, -0.7, (1.5, -1.0, 2.0))):
        add(f"track/pure_spin/r{roll}p{pitch}/w{w}", quat=quat_rpy(0.3, pitch, roll), w=w)
    r = add("track/cmd_equals_measured", quat=quat_rpy(-2.1, 0.5, -0.3), v=(0.6, -0.5, 0.2), w=(0.4, -0.3, 0.9))
    info = evaluate(K, r)[3]
    r["cmd"] = np.array([info["vyaw"][0], info["vyaw"][1], info["ww"][2]]).astype(np.float32).astype(np.float64)
    add("track/underflow_subnormal", quat=quat_rpy(0.2, 0.3, -0.2), v=(3.2, -3.6, 0.0), w=(0, 0, 5.2))
    add("track/underflow_far", quat=quat_rpy(0.2, 0.3, -0.2), v=(6.0, 0.0, 0.0), w=(0, 0, 6.0), cmd=(0, 0, -1.0))
    add("track/vertical_x_axis", quat=(0.5, 0.5, 0.5, -0.5), v=(0.3, -0.4, 0.2), w=(0.5, -0.3, 0.7),
        cmd=(0.2, 0.1, -0.3))
    # --- world against body w_z
    for roll, pitch, yaw, w in ((0.8, 0, 0, (1.2, 0, 0)), (0, 0.7, 0, (0, -1.5, 0)), (0.6, -0.5, 1.0, (0, 1.0, 0)),
                                (0.6, -0.5, 1.0, (1.0, 0, 0))):
        add(f"wz/r{roll}p{pitch}/w{w}", quat=quat_rpy(yaw, pitch, roll), w=w, cmd=(0, 0, 0.4))
    # --- one-hot sums
    for j in range(NJ):
        sgn = -1.0 if j % 2 else 1.0
        add(f"onehot/tau/{j}", tau=onehot(j, sgn * (10 + 3 * j)))
        add(f"onehot/jacc/{j}", jacc=onehot(j, -sgn * (50 + 7 * j)))
        add(f"onehot/qd/{j}", qd=onehot(j, sgn * (0.5 + 0.25 * j)))
        add(f"onehot/act/{j}", act=onehot(j, 0.3 + 0.1 * j), act_prev=onehot(j, -0.1 * (j % 3)))
    jj = np.arange(NJ)
    sg = np.where(jj % 3 == 0, -1.0, 1.0)
    add("onehot/all", tau=sg * (5 + 2 * jj), jacc=-sg * (20 + 5 * jj), qd=sg * (0.2 + 0.1 * jj),
        act=sg * (0.1 + 0.05 * jj), act_prev=-0.3 * sg)
    # --- soft limits and deviations
    slo, shi = info["soft_lo"], info["soft_hi"]
    limited = group(K, "joint_pos_limits:ankle") + group(K, "joint_pos_limits:hip")
    pitch_knee = [j for j, n in enumerate(K.names) if n.endswith("_hip_pitch_joint") or n.endswith("_knee_joint")]
    for j in limited:
        for side, lim, out in (("lo", slo[j], -1.0), ("hi", shi[j], 1.0)):
            qq = q0.copy()
            for k in pitch_knee:    # joints no limit term reads sit outside their own soft limits
                qq[k] = shi[k] + 0.05
            qq[j] = lim - out * 1e-3
            add(f"limit/{K.names[j]}/{side}/inside", q=qq)
            for d in (1e-3, 0.1, 0.3):
                qq = q0.copy()
                qq[j] = lim + out * d
                add(f"limit/{K.names[j]}/{side}/outside{d}", q=qq)
    for i, j in enumerate(limited):
        qq = q0.copy()
        qq[j] += (-1.0 if i % 2 else 1.0) * (0.05 + 0.02 * i)
        add(f"deviation/{K.names[j]}", q=qq)
    # --- feet_slide
    bent = q0 + np.array([0.1, -0.3, 0.05, 0.5, -0.15, 0.04, -0.12, 0.2, -0.08, 0.3, 0.1, -0.06])
    tq = quat_rpy(0.9, -0.35, 0.25)
    jr = np.array([0.6, -0.7, 0.8, -0.9, 1.0, -1.1, -0.65, 0.75, -0.85, 0.95, -1.05, 1.15])
    motions = dict(translation=dict(v=(0.4, -0.3, 0.1)), spin=dict(w=(0.3, -0.2, 1.1)),
                   combined=dict(v=(0.4, -0.3, 0.1), w=(0.3, -0.2, 1.1), qd=jr, quat=tq, q=bent))
    feet = dict(left=(5.0, 0), right=(0, 5.0), both=(5.0, 7.0))
    for mn, mk in motions.items():
        for fn, ff in feet.items():
            add(f"slide/{mn}/{fn}", fmax=(*ff, 0, 0, 0), **{"q": bent, **mk})
    for j in range(NJ):
        add(f"slide/joint/{j}", q=bent, qd=onehot(j, jr[j]), fmax=(5.0, 5.0, 0, 0, 0))
    one, one_up = 1.0, up32(1.0)
    for fn, ff in (("left_at", (one, 0)), ("left_past", (one_up, 0)), ("right_at", (0, one)), ("right_past", (0, one_up)),
                   ("both_at", (one, one)), ("left_at_right_past", (one, one_up))):
        add(f"slide/threshold/{fn}", fmax=(*ff, 0, 0, 0), **motions["combined"])
    # --- contact_forces
    cf, cf_up = K.contact_force_threshold, up32(K.contact_force_threshold)
    for fn, ff in (("left_at", (cf, 0)), ("left_past", (cf_up, 0)), ("left_far", (2000.0, 0)), ("right_at", (0, cf)),
                   ("right_past", (0, cf_up)), ("right_far", (0, 2400.0)), ("both_at", (cf, cf)),
                   ("both_past", (cf_up, cf_up)), ("both_far", (1500.0, 2400.0)), ("both_below", (500.0, 600.0))):
        add(f"contact_forces/{fn}", fmax=(*ff, 0, 0, 0))
    # --- terminations
    ct, ct_up = K.contact_threshold, up32(K.contact_threshold)
    for fn, ff in (("left_knee_at", (ct, 0, 0)), ("left_knee_past", (ct_up, 0, 0)), ("right_knee_at", (0, ct, 0)),
                   ("right_knee_past", (0, ct_up, 0)), ("torso_at", (0, 0, ct)), ("torso_past", (0, 0, ct_up)),
                   ("all_at", (ct, ct, ct))):
        add(f"term/{fn}", fmax=(0, 0, *ff))
    add("term/timeout_before", eplen=K.max_episode_length - 1)
    add("term/timeout_at", eplen=K.max_episode_length)
    add("term/timeout_and_right_knee", eplen=K.max_episode_length, fmax=(0, 0, 0, 50.0, 0))
    for a in range(3):
        sgn = -1.0 if a == 1 else 1.0
        for name, key, lim in (("v", "v", K.div_v), ("w", "w", K.div_w)):
            add(f"term/div_{name}{a}_at", **{key: onehot(a, sgn * lim)[:3]})
            add(f"term/div_{name}{a}_past", **{key: onehot(a, sgn * up32(lim))[:3]})
    # --- feet_air_time switches (contact time exactly 0 is "in the air")
    for fn, con, air in (("left_air", (0, 0.3), (0.2, 0)), ("right_air", (0.25, 0), (0, 0.55)), ("both_contact", (0.2, 0.3), (0, 0)),
                         ("both_air", (0, 0), (0.2, 0.3)), ("clamped", (0.9, 0), (0, 0.7))):
        add(f"air_time/{fn}", con=con, air=air, cmd=(0.5, 0, 0))
    # --- remaining base terms: identity at rest, then tilted moving bases at three heights
    add("base/identity_rest", pos=(0, 0, K.base_height_target))
    for i, (z, roll, pitch, yaw) in enumerate(((0.7, 0.3, 0.2, -1.2), (1.0, -0.6, 0.5, 2.6), (1.25, 0.9, -0.8, 0.4))):
        add(f"base/tilted_moving/{i}", pos=(1.0 + i, -2.0, z), quat=quat_rpy(yaw, pitch, roll),
            v=(0.5 - 0.4 * i, 0.3, -0.6 + 0.5 * i), w=(0.7, -0.4 * i, 0.5), cmd=(0.3, 0.1, -0.2))
    # --- everything at once
    rng = np.random.default_rng(20)
    for i in range(6):
        qt = rng.normal(size=4)
        add(f"random/{i}", pos=(*rng.uniform(-3, 3, 2), rng.uniform(0.6, 1.2)), quat=qt / np.linalg.norm(qt),
            v=rng.normal(size=3), w=rng.normal(size=3), q=q0 + 0.4 * rng.normal(size=NJ), qd=2 * rng.normal(size=NJ),
            act=rng.normal(size=NJ), act_prev=rng.normal(size=NJ), cmd=rng.uniform(-1, 1, 3),
            air=(0, rng.uniform(0.05, 0.6)), con=(rng.uniform(0.05, 0.6), 0), tau=30 * rng.normal(size=NJ),
            jacc=100 * rng.normal(size=NJ), fmax=(rng.uniform(2, 1500), rng.uniform(2, 1500), 0, 0, 0), eplen=100 + i)
    while len(rows) % 2 == 0 or len(rows) % 32 == 0:   # an odd env count that fills no block
        add(f"pad/{len(rows)}", cmd=(0.4, 0.3, 0.1))
    return rows


def subset_rows(rows, n):
    """n rows spread over the families whose last one -- alone in its block when n = 33 -- loads the right leg only."""
    last = {1: "slide/combined/right", 33: "term/right_knee_past"}[n]
    keep = ["track/vertical_x_axis"] if n > 1 else []
    pool = [r for r in rows if r["label"] != last and r["label"] not in keep]
    m = n - 1 - len(keep)
    step = max(1, len(pool) // max(1, m))
    return [r for r in rows if r["label"] in keep] + pool[::step][:m] + [r for r in rows if r["label"] == last]


# ------------------------------------------------------------------ reference table and gates
MARGIN = 8.0        # what float32 numpy does not model: the kernel's summation order, FMA contraction and the
#                     hardware's approximate exp, reciprocal and rsqrt -- a few float32 roundings each
FLOOR = 4 * EPS32   # a float32 result is never asked to be better than a few ulps
SCALE = 1.0         # term scale: every term is O(1) in SI units at the states of interest (exponentials and squared
#                     direction cosines <= 1, joint angles ~1 rad, velocities ~1 m/s), so an absolute error is
#                     measured against max(|ref|, 1)
EXACT = ("is_terminated", "feet_air_time_positive_biped")


def reference(K: Consts, rows, mut=None):
    """(terms (NREW, n) float64, terminated (n,), time_out (n,)) of the float64 restatement."""
    out = [evaluate(K, r, mut=mut) for r in rows]
    return (np.array([o[0] for o in out]).T, np.array([o[1] for o in out]), np.array([o[2] for o in out]))


def gates(K: Consts, rows, ref_terms):
    """Per term, the relative gate: MARGIN x the largest deviation of the float32 restatement from the float64 one
    over the rows (feet_slide: method (b) in float32 against the reference), relative to max(|ref|, SCALE)."""
    t32 = np.array([evaluate(K, r, dtype=np.float32, slide="jac")[0].astype(np.float64) for r in rows]).T
    with np.errstate(invalid="ignore"):
        rel = np.abs(t32 - ref_terms) / np.maximum(np.abs(ref_terms), SCALE)
    return MARGIN * np.maximum(rel.max(axis=1), FLOOR)


def mismatches(K, rows, ref, got, gate):
    """Every (label, what, got, want) where `got` = (terms (NREW, n), terminated, truncated) leaves the reference:
    exact for the flags, the EXACT terms and every value the reference gives as exactly 0; an absolute gate of
    float32's smallest normal where the reference lies below it (the result may be flushed); else the term's gate."""
    rt, rterm, rtout = ref
    gt_, gterm, gtout = (np.asarray(x) for x in got)
    bad = []
    for i, r in enumerate(rows):
        if bool(gterm[i]) != bool(rterm[i]):
            bad.append((r["label"], "terminated", bool(gterm[i]), bool(rterm[i])))
        if bool(gtout[i]) != bool(rtout[i]):
            bad.append((r["label"], "truncated", bool(gtout[i]), bool(rtout[i])))
        for t in range(NREW):
            g, w = float(gt_[t, i]), float(rt[t, i])
            if not np.isfinite(g):
                ok = False
            elif REWARD_FUNCS[t] in EXACT or w == 0.0:
                ok = g == w
            elif abs(w) < TINY32:
                ok = abs(g - w) <= TINY32
            else:
                ok = abs(g - w) <= gate[t] * max(abs(w), SCALE)
            if not ok:
                bad.append((r["label"], REWARD_FUNCS[t], g, w))
    return bad
