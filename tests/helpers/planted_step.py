"""Planted states for the step kernel's switching paths (test infrastructure): joint-limit projection on every joint
and side, the implicit torso-corner and knee contact reports, a foot in the air, a fixed base.

plant() rewrites the physics rows of the field-major float state Fm [H12_NF_FLOAT, n] (and the sole contact flags of
the packed int row) in place, from a fixed seed, and returns the per-env class masks the states were planted for, each
re-derived from the planted floats with the oracle's kinematics (so a class that a later edit of the recipe empties
is seen).  Env i gets recipe i % 32:

   0..11  joint k = i: beyond QHI + lproj by EXCESS (+ up to 20 %), velocity outward; in the air
  12..23  joint k = i - 12: beyond QLO - lproj, velocity outward; in the air
  24, 25  lying on the torso box (chest / back down), the lowest corner 0-4 mm deep
  26, 27  kneeling: both knee capsules 1-3 mm deep, feet and torso clear of the floor
  28      both feet flat on the floor (every joint inside its range, torso and knees clear)
  29, 30  standing on the left / right foot, the other foot ~6 cm up
  31      in the air, every joint inside its range

The limit penalty is a stiff spring integrated implicitly, so most of a joint's excess is pulled back within one inner
step, and only a heavy joint planted far beyond its limit is still beyond QHI + lproj after the integration, where the
projection acts: with EXCESS the oracle's projection acts on hip and knee joints, beyond both sides of the range and
in both legs (projection_acts re-checks it with the oracle, limit projection on against off); the light ankle joints
are back inside after one inner step from any excess tried (up to 2 rad), so their planted envs exercise the selects
with both conditions false.

run_case() plants a handle, takes STEPS teacher-forced env steps (tests/helpers/forced.py) and returns every output
of each step; tools/gen_step_planted_golden.py records them, tests/test_gpu_step_planted.py compares."""
from __future__ import annotations

import copy

import numpy as np

import oracle as O
import scenarios as S
from h12env._abi import F as FIELDS

RECIPES = 32
EXCESS = (0.7, 0.3, 0.3, 0.7, 0.3, 0.3)  # rad beyond the projection surface, per joint of a leg
QD_OUT = 3.0          # rad/s, outward
KNEE_BODY = (4, 10)   # knee links of the left / right leg in the oracle's body order
KNEEL = dict(hip_pitch=0.2, knee=1.9, ankle_pitch=0.5, base_pitch=0.6)
SEED = 20251
STEPS = 2
CASES = ((33, False), (64, False), (33, True))  # (envs, fixed base): 33 = a partial second block
OUTPUTS = ("F", "I", "obs", "rew", "term", "trunc", "applied_torque", "foot_force")


def _state(Fm, i):
    s = np.zeros(37)
    s[0:37] = Fm[0:37, i]
    return s


def _write(Fm, i, s):
    for name, a, b in (("POS", 0, 3), ("QUAT", 3, 7), ("VLIN", 7, 10), ("WANG", 10, 13), ("Q", 13, 25), ("QD", 25, 37)):
        S._set(Fm, name, i, s[a:b])


def _air(model, rng, q):
    s = np.zeros(37)
    s[0:3] = [rng.uniform(-1, 1), rng.uniform(-1, 1), 1.5 + rng.uniform(0, 0.2)]
    s[3:7] = S._quat(rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(-np.pi, np.pi))
    s[7:10] = rng.normal(size=3) * 0.2
    s[10:13] = rng.normal(size=3) * 0.3
    s[13:25] = q
    s[25:37] = rng.normal(size=12) * 0.2
    return s


def lowest_points(model, s):
    """Heights above the floor of the lowest torso-box corner, of each knee capsule's surface and of each foot's
    lowest sole sphere surface, for the 37-float physics state s."""
    R, p = O.body_poses(model, s)
    ch, hh = np.array(model.torso_center, dtype=np.float64), np.array(model.torso_half, dtype=np.float64)
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    torso = float(((R[0] @ (ch[None] + signs * hh[None]).T)[2] + p[0][2]).min())
    k0, k1 = np.array(model.knee_p0, dtype=np.float64), np.array(model.knee_p1, dtype=np.float64)
    knee = [min((R[b] @ k0)[2], (R[b] @ k1)[2]) + p[b][2] - float(model.knee_radius) for b in KNEE_BODY]
    pts = np.asarray(model.foot_pts, dtype=np.float64)
    foot = [float(((R[b] @ pts.T).T + p[b])[:, 2].min()) - float(model.foot_radius) for b in S.FOOT_BODY]
    return torso, knee, foot


def plant(model, Fm, Im, lproj, seed=SEED):
    n = Fm.shape[1]
    rng = np.random.default_rng(seed)
    q0 = np.asarray(model.q_default, dtype=np.float64)[:12]
    qlo, qhi = np.asarray(model.q_lower, dtype=np.float64)[:12], np.asarray(model.q_upper, dtype=np.float64)[:12]
    for i in range(n):
        r = i % RECIPES
        if r < 24:
            k, up = r % 12, r < 12
            s = _air(model, rng, q0 + rng.normal(size=12) * 0.05)
            ex = EXCESS[k % 6] * rng.uniform(1.0, 1.2)
            s[13 + k] = qhi[k] + lproj + ex if up else qlo[k] - lproj - ex
            s[25 + k] = QD_OUT if up else -QD_OUT
            _write(Fm, i, s)
        elif r < 26:
            one = Fm[:, i:i + 1].copy()
            S.lying(model, one, rng)
            if (r == 24) != (one[FIELDS["QUAT"][0] + 2, 0] * one[FIELDS["QUAT"][0], 0] > 0):  # 24: chest down
                one[FIELDS["QUAT"][0] + 2, 0] *= -1.0
                s = _state(one, 0)
                s[2] -= lowest_points(model, s)[0] + rng.uniform(0.0, 0.004)
                _write(one, 0, s)
            Fm[:, i] = one[:, 0]
        elif r < 28:
            q = q0 + rng.normal(size=12) * 0.01
            for leg in (0, 1):
                q[6 * leg + 1], q[6 * leg + 3], q[6 * leg + 4] = KNEEL["hip_pitch"], KNEEL["knee"], KNEEL["ankle_pitch"]
            s = np.zeros(37)
            s[0:2] = rng.uniform(-1, 1, 2)
            s[3:7] = S._quat(0.0, KNEEL["base_pitch"], rng.uniform(-np.pi, np.pi))
            s[13:25] = q
            s[7:13] = rng.normal(size=6) * 0.05
            s[2] -= max(lowest_points(model, s)[1]) + rng.uniform(0.001, 0.003)
            _write(Fm, i, s)
        elif r == 28:
            one, ione = Fm[:, i:i + 1].copy(), Im[:, i:i + 1].copy()
            S.stance(model, one, rng, ione)
            Fm[:, i], Im[:, i] = one[:, 0], ione[:, 0]
        elif r < 31:
            # scenarios.single_stance stands env j on foot j % 2: a two-env batch, of which the wanted one is kept
            two, itwo = np.repeat(Fm[:, i:i + 1], 2, axis=1), np.repeat(Im[:, i:i + 1], 2, axis=1)
            S.single_stance(model, two, rng, itwo)
            Fm[:, i], Im[:, i] = two[:, r - 29], itwo[:, r - 29]
        else:
            _write(Fm, i, _air(model, rng, q0 + rng.normal(size=12) * 0.05))
    return classes(model, Fm, lproj)


def classes(model, Fm, lproj) -> dict:
    """{class name: bool mask over envs} of the planted float state (Fm as the kernel reads it, fp32)."""
    n = Fm.shape[1]
    qlo, qhi = np.asarray(model.q_lower, dtype=np.float64)[:12], np.asarray(model.q_upper, dtype=np.float64)[:12]
    q = Fm[FIELDS["Q"][0]:FIELDS["Q"][0] + 12].astype(np.float64)
    qd = Fm[FIELDS["QD"][0]:FIELDS["QD"][0] + 12].astype(np.float64)
    out = {}
    for k in range(12):
        out[f"joint{k}_over"] = (q[k] > qhi[k] + lproj) & (qd[k] > 0)
        out[f"joint{k}_under"] = (q[k] < qlo[k] - lproj) & (qd[k] < 0)
        out[f"joint{k}_inside"] = (q[k] > qlo[k]) & (q[k] < qhi[k])
    low = [lowest_points(model, _state(Fm, i)) for i in range(n)]
    torso = np.array([l[0] for l in low])
    knee = np.array([min(l[1]) for l in low])
    foot = np.array([l[2] for l in low])
    out["torso_contact"], out["torso_clear"] = torso < 0.0, torso > 0.01
    out["knee_contact"], out["knee_clear"] = knee < 0.0, knee > 0.01
    out["one_foot_in_air"] = (foot.min(axis=1) < 0.0) & (foot.max(axis=1) > 0.01)
    return out


def projection_acts(model, ccfg, F0, I0, obs0, actions, step_index) -> np.ndarray:
    """Per-env bool: the oracle's step from (F0, I0, obs0) with the limit projection off ends with another joint state
    than with it on -- the projection acted in that env's step."""
    res = []
    for on in (True, False):
        c = copy.copy(ccfg)
        if not on:
            c.limit_projection = 0.0
        ref = O.OracleEnv(model, c, F0.shape[1])
        ref.F[:], ref.I[:], ref.obs[:] = F0, I0, obs0
        ref.step(actions, step_index)
        res.append(ref.F[FIELDS["Q"][0]:FIELDS["Q"][0] + 12 + 12].copy())
    return (res[0] != res[1]).any(axis=0)


def case_key(n, fix_base) -> str:
    return f"n{n}_{'fixed' if fix_base else 'free'}"


def run_case(n, fix_base):
    """Flat with self-collision, n envs planted after reset, STEPS forced env steps.  Returns (gpu, ref, classes,
    acts, fp): gpu / ref = {output name: array stacked over the steps} of the kernel / the fp64 oracle, acts the
    per-env projection_acts of the first step, fp the ForcedParity (its check() is criterion iii)."""
    import torch

    from forced import ForcedParity
    from h12env import H12FlatEnvCfg
    from h12env.env import H12VelocityEnv

    cfg = H12FlatEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    cfg.sim.self_collision = True
    cfg.fix_base = fix_base
    env = H12VelocityEnv(cfg)
    try:
        env.reset()
        Fm, Im = env._fstate.cpu().numpy().copy(), env._istate.cpu().numpy().copy()
        cl = plant(env._model, Fm, Im, float(env._ccfg.limit_projection))
        env._fstate.copy_(torch.from_numpy(Fm))
        env._istate.copy_(torch.from_numpy(Im))
        obs0 = env._obs[env._k].cpu().numpy().copy()
        fp = ForcedParity(env, seed=SEED)
        rng = np.random.default_rng(SEED + 1)
        gpu, ref = {k: [] for k in OUTPUTS}, {k: [] for k in OUTPUTS}
        acts = None
        for t in range(STEPS):
            a = (rng.normal(size=(n, 12)) * 0.3).astype(np.float32)
            if t == 0:
                acts = projection_acts(env._model, env._ccfg, Fm, Im, obs0, a, env.common_step_counter + 1)
            g, o, _, _ = fp.step(a)
            torch.cuda.synchronize()
            g = tuple(np.array(x) for x in g) + (env._applied_torque.cpu().numpy().copy(),
                                                 env.foot_contact_force.cpu().numpy().copy())
            o = tuple(np.array(x) for x in o[:6]) + (o[6]["applied_torque"], o[6]["foot_force"])
            for k, x, y in zip(OUTPUTS, g, o):
                gpu[k].append(x)
                ref[k].append(y)
        return ({k: np.stack(v) for k, v in gpu.items()}, {k: np.stack(v) for k, v in ref.items()}, cl, acts, fp)
    finally:
        env.close()
