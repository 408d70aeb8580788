"""Shared pieces of the safety-monitor GPU tests: the drop-and-random-targets scenario of test_gpu_mujoco_contact.py and
the oracle's per-substep record (torques, foot-force norms) of one control step from a workspace snapshot."""
import numpy as np

import oracle as O
from h12env._abi import F as FIELDS, I as IFIELDS

N_SUB = 20
# the trace-vs-oracle scenario: chosen with the oracle alone (the oracle against its own fp32-perturbed re-run stays under
# half the 2 % cap on these inputs: 11 of 51200 env-substeps, 0.02 %, with 0.90 of them in sole contact; DESIGN.md
# section 7h)
TRACE_N, TRACE_STEPS, TRACE_SEED, TRACE_SCALE = 64, 40, 11, 0.25 * 0.6


def targets(rng, q0, n, scale):
    return (q0[None] + scale * rng.normal(size=(n, 12))).astype(np.float32)


def contact_envs(I):
    return ((I[IFIELDS["PACK"][0]] >> 13) & 0xFF) != 0


def phys_states(F, I):
    """[n][54] float64: the oracle's Phys vector (pose, velocities, q, qd, anchors, contact mask) of every env."""
    n = F.shape[1]
    rows = [F[FIELDS[k][0]:FIELDS[k][0] + FIELDS[k][1]] for k in ("POS", "QUAT", "VLIN", "WANG", "Q", "QD", "ANCHOR")]
    cm = ((I[IFIELDS["PACK"][0]] >> 13) & 0xFF).astype(np.float64)[None]
    return np.concatenate(rows + [cm], axis=0).astype(np.float64).T.reshape(n, 54)


def oracle_records(model, ccfg, F, I, q_ref, n_sub=N_SUB):
    """The oracle's substep records of one control step from workspace (F, I): [n][n_sub][14] = 12 clamped PD torques
    (computed in fp64 from the oracle's own pre-step state, the law of orc_env_step_physics) and the two feet's
    |net contact force| (mean over the inner steps)."""
    kp, kd = np.array(ccfg.kp, np.float64), np.array(ccfg.kd, np.float64)
    lim = np.array(model.mj_frc_limit, np.float64)
    S = phys_states(F, I)
    n = S.shape[0]
    out = np.zeros((n, n_sub, 14))
    qr = np.asarray(q_ref, np.float32).astype(np.float64)
    for i in range(n):
        s = S[i]
        for k in range(n_sub):
            tau = np.clip(kp * (qr[i] - s[13:25]) - kd * s[25:37], -lim, lim)
            s, rep = O.physics_step(model, ccfg, s, tau, contact=True, algo=1)
            out[i, k, :12] = tau
            out[i, k, 12] = np.linalg.norm(np.array(rep.foot_force[0]))
            out[i, k, 13] = np.linalg.norm(np.array(rep.foot_force[1]))
    return out


def record_err(x, b):
    """[n][n_sub] error of records x against b in units of the gates of test_contact_force_and_torque_parity: feet
    1e-2 of max(10 N, |F|), torques 2e-3 of max(1, |tau|)."""
    et = np.abs(x[..., :12] - b[..., :12]) / (2e-3 * np.maximum(1.0, np.abs(b[..., :12])))
    ef = np.abs(x[..., 12:] - b[..., 12:]) / (1e-2 * np.maximum(10.0, np.abs(b[..., 12:])))
    return np.maximum(et.max(axis=-1), ef.max(axis=-1))
