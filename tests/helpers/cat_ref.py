"""CaT's cross-env pass restated in float64 (constraint_manager.py:23-123, constraints.py:202-238, cat_env.py:148-166).

cat_pass_numpy is the restatement the oracle's pass is checked against (tests/test_oracle_cat.py).  cat_step_ref is the
teacher-forced restatement of one pass of the HIP env from the kernel's own float32 rows (H12VelocityEnv.cat_snapshot):
the still set, the remap, the column maxima and their clamp, the running maxima, the probabilities, the constraint sums
and the episode statistics of the resetting envs.  Fed with the kernel's rows, the previous snapshot's running maxima
and the pre-step CSTR_SUM / CSTR_P fields, it isolates the pass from the fp32 contact decisions of the physics, so
tests/test_gpu_cat_fold.py can gate it exactly or at a few ulp.  plant() writes the scenarios of that test (which envs
are still, where the column maxima sit, which envs reset) through a setter, so the same scenario can be put into the
HIP env's tensors or the oracle's arrays."""
import numpy as np

from h12env._abi import NCSTR

COL0 = [0, 1, 13, 25, 37, 39, 51, 52, 53, 54, 56]
NCOLS = COL0[-1]
ROW_NOMOVE, ROW_EPLEN = NCOLS, NCOLS + 1
NM = slice(COL0[5], COL0[6])               # no_move's columns
COL_TERM = np.repeat(np.arange(NCSTR), np.diff(COL0))
U = 2.0 ** -24                              # float32 unit roundoff
TAU32 = float(np.float32(0.95))             # h12env_config.cat_tau as the kernel holds it
CLAMP32 = np.float32(1e-6)                  # constraint.max(dim=0).clamp(min=1e-6), as the kernel's float constant
ENVS_PER_BLOCK = 32


def cat_pass_numpy(cs, run_prev, max_p, tau=float(np.float32(0.95)), min_p=0.0, mask=(1 << NCSTR) - 1):
    """constraint_manager.py:42-78 (CaT.add / get_probs) + no_move's row remap (constraints.py:202-238)."""
    n = cs.shape[1]
    still = np.nonzero(cs[56] != 0)[0]
    rows = cs[:56].copy()
    nm = slice(COL0[5], COL0[6])
    if len(still):
        rows[nm] = cs[nm][:, still[np.arange(n) % len(still)]]
    else:
        rows[nm] = 0.0
    cmax = np.maximum(rows.max(axis=1), 1e-6)
    run = cmax if run_prev is None else tau * run_prev + (1 - tau) * cmax
    pt = np.zeros((NCSTR, n))
    for t in range(NCSTR):
        if not (mask >> t) & 1:
            continue
        r = rows[COL0[t]:COL0[t + 1]]
        p = np.where(r > 0, min_p + np.clip(r / run[COL0[t]:COL0[t + 1], None], 0, 1) * (max_p[t] - min_p), 0.0)
        pt[t] = p.max(axis=0)
    return run, pt, pt.max(axis=0)


def still_envs(rows):
    return np.nonzero(rows[ROW_NOMOVE] != 0)[0]


def still_masks(still, n):
    """The still set as one 32-bit mask per block of 32 envs (bit j of word b: env 32 b + j)."""
    mk = np.zeros((n + ENVS_PER_BLOCK - 1) // ENVS_PER_BLOCK, np.uint64)
    np.bitwise_or.at(mk, np.asarray(still) // ENVS_PER_BLOCK,
                     np.uint64(1) << (np.asarray(still, np.uint64) % np.uint64(ENVS_PER_BLOCK)))
    return mk.astype(np.uint32)


def column_maxima(rows):
    """(maxima of the 56 columns in the rows' own type -- no_move's over the still envs only, 0 with none --, the env
    holding each maximum, or -1 where it is not unique or no env counts).  max is exact, so on the kernel's float32
    rows these are the kernel's own values."""
    still = still_envs(rows)
    cm = np.zeros(NCOLS, rows.dtype)
    arg = np.full(NCOLS, -1)
    for c in range(NCOLS):
        nm = NM.start <= c < NM.stop
        envs = still if nm else np.arange(rows.shape[1])
        if len(envs) == 0:
            continue
        v = rows[c, envs]
        cm[c] = v.max()
        at = envs[v == cm[c]]
        if len(at) == 1:
            arg[c] = at[0]
    return cm, arg


def cat_step_ref(rows, run_prev, max_p, sums, psums, reset, tau=TAU32, min_p=0.0, mask=(1 << NCSTR) - 1,
                 clamp=CLAMP32):
    """One CaT pass in float64 from float32 inputs: rows (58, n) of the snapshot, run_prev (56,) the previous snapshot's
    running maxima (None: the first fold), max_p (NCSTR,), sums / psums (NCSTR, n) the pre-step CSTR_SUM / CSTR_P
    fields, reset (n,) bool the envs this step resets; clamp: the floor of the column maxima (the kernel's float32
    constant; the fp64 oracle's is the double 1e-6).  Returns a dict (see the keys at the end)."""
    n = rows.shape[1]
    still = still_envs(rows)
    m = len(still)
    src = still[np.arange(n) % m] if m else np.full(n, -1)
    r64 = rows[:NCOLS].astype(np.float64)
    if m:
        r64[NM] = r64[NM][:, src]
    else:
        r64[NM] = 0.0
    colmax, arg = column_maxima(rows)
    clamped = np.maximum(colmax, clamp)
    cm = clamped.astype(np.float64)
    run = cm if run_prev is None else tau * np.asarray(run_prev, np.float64) + (1.0 - tau) * cm
    mp = np.asarray(max_p, np.float64)
    on = np.array([(mask >> t) & 1 for t in range(NCSTR)], bool)
    ratio = r64 / run[:, None]
    p = np.where(r64 > 0, min_p + np.clip(ratio, 0, 1) * (mp[COL_TERM, None] - min_p), 0.0)
    p[~on[COL_TERM]] = 0.0
    pt = np.stack([p[COL0[t]:COL0[t + 1]].max(axis=0) for t in range(NCSTR)])
    pmax = pt.max(axis=0)
    s1 = np.asarray(sums, np.float64) + np.where(on[:, None], pt > 0, 0)
    p1 = np.asarray(psums, np.float64) + pt
    p1[~on] = np.asarray(psums, np.float64)[~on]
    ln = rows[ROW_EPLEN].astype(np.float64)
    k = int(reset.sum())
    out = dict(still=still, m=m, src=src, colmax=colmax, colarg=arg, clamped=clamped, run=run, pt=pt, pmax=pmax, k=k,
               # coverage: a violated value above its running maximum (clamped to 1), a probability inside (0, max_p)
               over=bool(((r64 > 0) & (ratio > 1) & on[COL_TERM, None]).any()),
               inside=bool(((pt > 0) & (pt < mp[:, None])).any()))
    if k:
        # ConstraintManager.reset: Episode_Constraint_violation = 100 mean(sum / len), _probability = mean(psum / len)
        v = 100.0 * s1[:, reset] / ln[reset] / k
        q = p1[:, reset] / ln[reset] / k
        out.update(log_violation=v.sum(axis=1), log_probability=q.sum(axis=1),
                   log_violation_abs=np.abs(v).sum(axis=1), log_probability_abs=np.abs(q).sum(axis=1))
    s1[:, reset] = np.where(on[:, None], 0.0, s1[:, reset])
    p1[:, reset] = np.where(on[:, None], 0.0, p1[:, reset])
    out.update(sums=s1, psums=p1, on=on)
    return out


def check_step(snap, run_prev, sums0, psums0, sums1, psums1, dones, rew, rew_twin, reset, log, inline, tau=TAU32,
               min_p=0.0, mask=(1 << NCSTR) - 1):
    """One step of the HIP env against cat_step_ref.  snap: H12VelocityEnv.cat_snapshot() after the step; run_prev: the
    previous snapshot's running maxima (None: the first fold); sums0 / psums0, sums1 / psums1: the CSTR_SUM / CSTR_P
    fields before and after; dones, rew: the step's outputs; rew_twin: the reward of the twin env whose probabilities
    are all zero; reset: the envs the step reset; log: {term id: (violation, probability)} of extras["log"] on a step
    with resets (else None); inline: the path (the still list exists on the two-kernel path only).

    Returns (restatement, fractions, failures): `fractions` is the measured worst fraction of each a-priori gate,
    `failures` the list of broken assertions (exact ones and gates over 1)."""
    rows, running = snap["rows"], snap["running"]
    n = rows.shape[1]
    max_p = snap["max_p"]
    R = cat_step_ref(rows, run_prev, max_p, sums0, psums0, reset, tau, min_p, mask)
    fails, frac = [], {}
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    # ---- exact: the still set, m, the masks, the list
    if snap["m"] != R["m"]:
        fails.append(f"m {snap['m']} != {R['m']}")
    if not np.array_equal(snap["still_mask"], still_masks(R["still"], n)):
        fails.append("still_mask differs from the snapshot's no_move flags")
    if not inline and not np.array_equal(snap["still_list"][:R["m"]], R["still"]):
        fails.append("still_list is not the ascending still set")
    if not snap["initialised"]:
        fails.append("running maxima not marked initialised after a fold")
    # ---- the running maxima: the first fold exact, later ones within 3 u (two products and a sum, all terms
    # positive, either contraction), the reciprocal exact (a correctly rounded division)
    if run_prev is None:
        if not np.array_equal(bits(running[0]), bits(R["clamped"])):
            fails.append(f"first fold: running maxima differ in columns {np.nonzero(running[0] != R['clamped'])[0]}")
        frac["fold"] = 0.0
    else:
        f = np.abs(running[0].astype(np.float64) - R["run"]) / (3 * U * R["run"])
        frac["fold"] = float(f.max())
        if f.max() > 1:
            fails.append(f"fold: column {int(f.argmax())} at {f.max():.2f} of the 3 u gate")
    if not np.array_equal(bits(running[1]), bits(np.float32(1) / running[0])):
        fails.append("running[1] is not fp32 1 / running[0]")
    # ---- the constraint sums: exact counts; zeroed with the probability sums where the env reset; a masked term's
    # sums are left as they were
    if not np.array_equal(sums1.astype(np.float64), R["sums"]):
        t, e = np.nonzero(sums1 != R["sums"])
        fails.append(f"CSTR_SUM differs in {len(e)} places, first (term {t[0]}, env {e[0]}): {sums1[t[0], e[0]]} != "
                     f"{R['sums'][t[0], e[0]]}")
    on = R["on"]
    if reset.any() and np.abs(psums1[on][:, reset]).max() != 0:
        fails.append("CSTR_P of a reset env is not zero")
    if (~on).any() and not np.array_equal(bits(psums1[~on]), bits(psums0[~on])):
        fails.append("a masked term's CSTR_P changed")
    if reset.any() and not (dones[reset] == 1).all():
        fails.append("dones of a reset env is not 1")
    # ---- probabilities: 5 u max(max_p, min_p) (the reciprocal, the product, the scale, the add), per term on the
    # CSTR_P increment (+ u |CSTR_P| for the accumulate), and on dones (a max over the terms) for the envs not reset
    mp = np.maximum(max_p.astype(np.float64), min_p)
    live = ~reset
    gate_t = 5 * U * mp[:, None] + U * np.abs(psums1.astype(np.float64))
    err_t = np.abs(psums1.astype(np.float64) - (psums0.astype(np.float64) + R["pt"]))
    sel = on[:, None] & live[None, :] & (gate_t > 0)
    # (a term whose max_p and sum are both 0 has a zero gate: it must be exact)
    if (err_t[on[:, None] & live[None, :] & (gate_t == 0)] != 0).any():
        fails.append("CSTR_P moved under a zero max_p")
    frac["cstr_p"] = float((err_t[sel] / gate_t[sel]).max()) if sel.any() else 0.0
    # (dones is a max over the terms, so its error is at most the largest of the terms'; a term without a violated
    # column is exactly 0 on both sides and adds none: the gate takes the max_p of the env's violated terms only)
    gate_d = 5 * U * np.where(R["pt"] > 0, mp[:, None], 0.0).max(axis=0)
    err_d = np.abs(dones.astype(np.float64) - R["pmax"])
    if (err_d[live & (gate_d == 0)] != 0).any():
        fails.append("dones of an env without a violated constraint is not 0")
    sel_d = live & (gate_d > 0)
    frac["dones"] = float((err_d[sel_d] / gate_d[sel_d]).max()) if sel_d.any() else 0.0
    # ---- the reward: rew_twin (1 - dones), both roundings pinned, for the envs not reset; for the reset ones
    # (dones = 1 there) the restatement's p_max under the probability gate, + u for 1 - p and the product
    want = rew_twin.astype(np.float32) * (np.float32(1) - dones.astype(np.float32))
    if not np.array_equal(rew[live], want[live]):
        e = np.nonzero(live & (rew != want))[0]
        fails.append(f"rew != fl(rew_twin fl(1 - dones)) in {len(e)} envs, first {e[0]}: {rew[e[0]]} vs {want[e[0]]}")
    if reset.any():
        err_r = np.abs(rew[reset].astype(np.float64) - rew_twin[reset].astype(np.float64) * (1 - R["pmax"][reset]))
        gate_r = (gate_d[reset] + U) * np.abs(rew_twin[reset].astype(np.float64))
        ok0 = (err_r[gate_r == 0] == 0).all()
        frac["rew_reset"] = float((err_r[gate_r > 0] / gate_r[gate_r > 0]).max()) if (gate_r > 0).any() else 0.0
        if not ok0:
            fails.append("reward of a reset env with a zero twin reward is not zero")
    # ---- the episode log of the resetting envs: (k + 3) u sum|terms| (k - 1 additions, the reciprocal of the length,
    # its product, the division by k and the scale; k <= 64)
    if R["k"]:
        if R["k"] > 64:
            fails.append(f"{R['k']} envs reset: the scenario keeps to 64")
        if log is None:
            fails.append("no episode log on a step with resets")
        else:
            worst = 0.0
            for t in range(NCSTR):
                if not on[t]:
                    if t in log:
                        fails.append(f"masked term {t} is logged")
                    continue
                for got, ref, ab in ((log[t][0], R["log_violation"][t], R["log_violation_abs"][t]),
                                     (log[t][1], R["log_probability"][t], R["log_probability_abs"][t])):
                    g = (R["k"] + 3) * U * ab
                    if g == 0:
                        if got != ref:
                            fails.append(f"log of term {t}: {got} != {ref} (exact: all terms zero)")
                    else:
                        worst = max(worst, abs(got - ref) / g)
            frac["log"] = worst
    for k, v in frac.items():
        if v > 1 and k != "fold":
            fails.append(f"{k}: {v:.2f} of its gate")
    return R, frac, fails


class Coverage:
    """The coverage conditions of a planted case, gathered from the steps' rows and restatements themselves, so a case
    cannot pass without having run the branches it is there for."""

    def __init__(self, n, scenario):
        self.n, self.scenario = n, scenario
        self.nb = (n + ENVS_PER_BLOCK - 1) // ENVS_PER_BLOCK
        self.seen = dict(resets=0, pmax=False, neg=False, over=False, inside=False, chunks=set(), remap=False,
                         cross=False, gap=False)

    def step(self, rows, still_mask, R, reset):
        s, n = self.seen, self.n
        planted = still_set(n, self.scenario)
        assert np.array_equal(R["still"], planted), (R["still"], planted)  # the commands held: the planted scenario
        s["resets"] += int(reset.sum())
        s["pmax"] |= bool((R["pmax"] > 0).any())
        s["neg"] |= bool((R["colmax"] < 0).any())
        s["over"] |= R["over"]
        s["inside"] |= R["inside"]
        s["chunks"] |= {int(e) // ENVS_PER_BLOCK for e in R["colarg"] if e >= 0}
        nm = rows[NM][:, R["still"]]
        pos = nm[:, (nm > 0).any(axis=0)]
        s["remap"] |= len({c.tobytes() for c in pos.T}) >= 3
        s["cross"] |= bool(R["m"] and (R["src"] // ENVS_PER_BLOCK != np.arange(n) // ENVS_PER_BLOCK).any())
        mk = np.nonzero(still_mask)[0]
        s["gap"] |= bool(len(mk) >= 2 and (still_mask[mk[0]:mk[-1]] == 0).any())

    def check(self):
        s, n = self.seen, self.n
        assert s["resets"] >= 1, "no env reset"
        assert s["pmax"], "no env with p_max > 0"
        assert s["neg"], "no column with a negative maximum (the clamp)"
        if n > 1:
            assert s["over"], "no violated value above its running maximum (the clamp to 1)"
            assert s["inside"], "no probability strictly inside (0, max_p)"
        m = len(still_set(n, self.scenario))
        if m >= 3:  # the remap scenarios
            assert s["remap"], "fewer than 3 still envs with a positive no_move column and pairwise different rows"
            if n > ENVS_PER_BLOCK and m < n:  # (with every env still, env i reads its own row)
                assert s["cross"], "no env reads a row of another block"
        if self.scenario == "sparse":
            assert s["gap"], "no empty still mask between two non-empty ones"
        if n >= 257:  # column maxima in blocks of every maxima set (hardware block mod 8) and in the last block
            assert {hw_block(c, self.nb) % 8 for c in s["chunks"]} == set(range(8)), s["chunks"]
            assert self.nb - 1 in s["chunks"], s["chunks"]


# ---- the planted scenarios of tests/test_gpu_cat_fold.py: (envs, still scenario, masked term, steps)
SIZES = [(n, "mixed", None, 4) for n in (1, 31, 33, 65, 257, 2085, 8224)]
STILL = [(n, s, None, 4) for n in (65, 257) for s in ("none", "one", "all", "sparse")]
OTHER = [(65, "mixed", "base_orientation", 4), (65, "mixed", None, 12)]
assert 257 % 32 == 1 and 2085 % 32 == 5 and 8224 == 257 * 32  # partial last blocks of 1 and 5 envs; 257 full blocks
CASES = SIZES + STILL + OTHER


def fold_cfg(n, masked=None, twin=False, device=None):
    """The CaT task with commands the test controls: the command deadzone's own re-drawing off (velocity_deadzone 0:
    a planted zero command stays zero, cmd_z is never re-drawn) and yaw commands of a reset env drawn outside no_move's
    deadzone.  masked: a constraint term switched off.  twin: every max_p held at 0 with the max_p curriculum off --
    all probabilities are zero, so its rewards are the unscaled ones."""
    from h12env.cfg import H12CaTEnvCfg

    cfg = H12CaTEnvCfg()
    cfg.scene.num_envs = n
    if device is not None:
        cfg.sim.device = device
    cfg.commands.base_velocity.velocity_deadzone = 0.0
    cfg.commands.base_velocity.ranges.ang_vel_z = (0.5, 1.0)
    if masked is not None:
        setattr(cfg.constraints, masked, None)
        cfg.curriculum.constraint_p = [t for t in cfg.curriculum.constraint_p if t.term_name != masked]
    if twin:
        for name, term in cfg.constraints.items():
            if term is not None:
                term.max_p = 0.0
        cfg.curriculum.constraint_p = []
    return cfg


def xcd_block(b, nb):
    """step_kernel's env chunk of hardware block b (the kernel's XCD-aware order; a bijection on [0, nb))."""
    x, k, q, r = b & 7, b >> 3, nb >> 3, nb & 7
    return x * q + min(x, r) + k


def hw_block(chunk, nb):
    return next(b for b in range(nb) if xcd_block(b, nb) == chunk)


def still_set(n, scenario):
    """The envs whose command sits inside no_move's deadzone."""
    nb = (n + ENVS_PER_BLOCK - 1) // ENVS_PER_BLOCK
    if scenario == "none":
        return np.zeros(0, int)
    if scenario == "one":           # a single still env, in the (partial) last block
        return np.array([n - 1])
    if scenario == "all":
        return np.arange(n)
    if scenario == "sparse":        # whole blocks without a still env between blocks that hold some
        blocks = [b for b in range(nb) if b in (0, nb - 1) or (nb > 4 and b in (3, 4))]
        pick = lambda b: [e for e in (32 * b + 1, 32 * b + 5, 32 * b + 6, 32 * b + 31) if e < n] or [32 * b]  # noqa: E731
        return np.array(sorted({e for b in blocks for e in pick(b)}))
    assert scenario == "mixed"
    return np.array(sorted(set(range(0, n, 3)) | {n - 1}))


def max_chunks(n):
    """The env chunks that get a planted column maximum: one per maxima set (hardware block mod 8), one past the
    first eight hardware blocks (the sets wrap), and the last chunk."""
    nb = (n + ENVS_PER_BLOCK - 1) // ENVS_PER_BLOCK
    ch = [xcd_block(b, nb) for b in range(min(nb, 9))]
    if nb - 1 not in ch:
        ch.append(nb - 1)
    return ch


def reset_envs(n, step):
    """The envs whose episode ends in 0-based step `step` (a handful: the log gate counts on <= 64)."""
    if step == 0:
        return sorted({n // 2, n - 1})
    if step == 2:
        return sorted({0, n // 3, (2 * n) // 3})
    return []


def plant(setf, seti, n, scenario, step, q_upper, max_len):
    """Write 0-based step `step`'s plants: setf(field, component, envs, values) / seti(field, envs, values)."""
    still = still_set(n, scenario)
    grow = step % 4  # (a longer run's maxima rise and fall: the running maxima drift both ways)
    allv = np.arange(n)
    isst = np.zeros(n, bool)
    isst[still] = True
    # commands: still envs (0, 0, 0), the others well outside the deadzone; no resampling within the test
    for k, v in enumerate((0.9, -0.4, 0.9)):
        setf("CMD", k, allv, np.where(isst, 0.0, v))
    setf("CMD_TIME", 0, allv, np.full(n, 1.0e6))
    # still envs: large, pairwise different joint velocities (no_move's columns |qd| - limit positive and distinguishable)
    if len(still):
        for j0 in (0, 5):
            for j in range(12):
                e = still[(still + j0) % 12 == j]
                if len(e):
                    sg = np.where(e % 2 == 0, 1.0, -1.0)
                    setf("QD", j, e, sg * (9.0 + ((e * 7919 + 131 * j0) % 1000) * 0.012 + 1.5 * grow))
    # column maxima in chosen chunks: joint k's velocity far over its limit in chunk k's env, growing per step so
    # that a violated value exceeds the lagging running maximum; joint positions past their limits in the same envs
    for k, c in enumerate(max_chunks(n)):
        e = np.array([min(32 * c + 7, n - 1)])
        setf("QD", k % 12, e, np.array([(45.0 + 3.0 * k) * (1.0 + 0.4 * grow)]))
        if step == 0:
            setf("Q", (k + 3) % 12, e, np.array([q_upper[(k + 3) % 12] + 0.3 + 0.02 * k]))
    # a few bases lifted out of the height band (base_height's flag)
    if step == 0:
        e = allv[allv % 11 == 4]
        if len(e):
            setf("POS", 2, e, np.full(len(e), 1.25))
    r = np.array(reset_envs(n, step), int)
    if len(r):
        seti("EPLEN", r, np.full(len(r), max_len - 1))
    return still
