"""numpy float32 restatement of the safety monitor's accumulators (include/h12env.h, H12_MON_*), computed from a trace.

emulate(trace, ...) replays the records of a trace ([substeps][n][TRACE_WORDS] fp32, real joint signs) in substep order
with one separately rounded float32 operation per step of every sum, which is what physics_monitor_kernel does (its
accumulator lines are compiled without contraction): applied to the GPU's own trace it must reproduce every monitor
word bit for bit.  Pass the previous monitor as `mon` to continue it (persistence across calls)."""
import numpy as np

from h12env._abi import MON, MON_COUNTS, MON_WORDS, TRACE

f32 = np.float32


def _tr(trace, name):
    off, cnt = TRACE[name]
    return trace[..., off:off + cnt]


def emulate(trace, q_lower, q_upper, tau_clamp, vel_limit, force_limit, mon=None):
    """-> int32 [MON_WORDS][n] (float words hold float32 bits)."""
    trace = np.asarray(trace, f32)
    S, n = trace.shape[:2]
    out = np.zeros((MON_WORDS, n), np.int32) if mon is None else np.array(mon, np.int32).reshape(MON_WORDS, n).copy()
    fl = out.view(f32)
    lo, hi = np.asarray(q_lower, f32)[:, None], np.asarray(q_upper, f32)[:, None]
    clamp, vl = np.asarray(tau_clamp, f32)[:, None], np.asarray(vel_limit, f32)[:, None]
    flim = f32(force_limit)
    I = lambda name: out[MON[name][0]:MON[name][0] + MON[name][1]]  # noqa: E731
    F = lambda name: fl[MON[name][0]:MON[name][0] + MON[name][1]]  # noqa: E731
    assert all(name in MON for name in MON_COUNTS)
    zero = f32(0)
    for k in range(S):
        q, qd, tau, force = (_tr(trace[k], x).T for x in ("Q", "QD", "TAU", "FORCE"))  # [12][n], [2][n]
        first = (I("SUBSTEPS")[0] == 0)[None, :]
        I("POS_VIOL_COUNT")[:] += ((q < lo) | (q > hi)).astype(np.int32)
        F("POS_EXCESS_MAX")[:] = np.maximum(F("POS_EXCESS_MAX"), np.maximum(np.maximum(lo - q, q - hi), zero))
        ta, va = np.abs(tau), np.abs(qd)
        F("TAU_ABS_MAX")[:] = np.maximum(F("TAU_ABS_MAX"), ta)
        I("TAU_SAT_COUNT")[:] += (ta >= clamp).astype(np.int32)
        F("QD_ABS_MAX")[:] = np.maximum(F("QD_ABS_MAX"), va)
        I("QD_VIOL_COUNT")[:] += ((vl > zero) & (va > vl)).astype(np.int32)
        dtau = np.where(first, zero, np.abs(tau - F("TAU_PREV")))
        dq = np.where(first, zero, np.abs(q - F("Q_PREV")))
        F("TAU_RATE_SUM")[:] = F("TAU_RATE_SUM") + dtau
        F("TAU_RATE_MAX")[:] = np.maximum(F("TAU_RATE_MAX"), dtau)
        F("Q_RATE_SUM")[:] = F("Q_RATE_SUM") + dq
        F("Q_RATE_MAX")[:] = np.maximum(F("Q_RATE_MAX"), dq)
        F("TAU_PREV")[:] = tau
        F("Q_PREV")[:] = q
        F("FORCE_MAX")[:] = np.maximum(F("FORCE_MAX"), force)
        F("FORCE_SUM")[:] = F("FORCE_SUM") + force
        I("FORCE_VIOL_COUNT")[:] += (force > flim).astype(np.int32)
        con = (force[0] != zero) | (force[1] != zero)
        pair = force[0] + force[1]
        I("CONTACT_SUBSTEPS")[0] += con.astype(np.int32)
        F("FORCE_PAIR_SUM")[0] = np.where(con, F("FORCE_PAIR_SUM")[0] + pair, F("FORCE_PAIR_SUM")[0])
        F("FORCE_PAIR_MAX")[0] = np.where(con, np.maximum(F("FORCE_PAIR_MAX")[0], pair), F("FORCE_PAIR_MAX")[0])
        I("SUBSTEPS")[0] += 1
    return out
