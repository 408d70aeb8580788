"""CPU: the float64 restatement of CaT's cross-env pass (tests/helpers/cat_ref.py) that tests/test_gpu_cat_fold.py holds
the kernels to -- checked here without a GPU, three ways:

  * against the oracle's pass on the planted scenarios (running maxima to fp64 rounding; probabilities, constraint
    sums and the episode log to the oracle's float32 outputs), and the scenarios' coverage conditions hold there;
  * a float32 numpy emulation of the kernels' formulas (unfused and with either fused multiply-add) passes every exact
    assertion and a-priori gate of check_step, with the measured fractions printed;
  * the same emulation with one planted fault each -- no remap, a remap off by one, a block's maxima dropped, the
    Polyak weights swapped, a reset env missing from the log, a stale still mask -- fails it."""
import numpy as np
import pytest

import cat_ref as CR
import oracle as O
from h12env._abi import F, I, NCSTR, NREW
from h12env.startup import apply_to_arrays, startup_state

f32 = np.float32


def test_block_order_and_masks():
    for nb in (1, 2, 3, 9, 66, 257):
        assert sorted(CR.xcd_block(b, nb) for b in range(nb)) == list(range(nb))
        assert all(CR.xcd_block(CR.hw_block(c, nb), nb) == c for c in range(nb))
    mk = CR.still_masks(np.array([0, 31, 32, 64]), 65)
    assert mk.dtype == np.uint32 and mk.tolist() == [0x80000001, 1, 1]
    assert CR.still_masks(np.zeros(0, int), 33).tolist() == [0, 0]
    for n in (257, 2085, 8224):
        nb = (n + 31) // 32
        ch = CR.max_chunks(n)
        assert {CR.hw_block(c, nb) % 8 for c in ch} == set(range(8)) and nb - 1 in ch
    s = CR.still_set(257, "sparse")
    blocks = sorted(set(s // 32))
    assert blocks == [0, 3, 4, 8] and CR.still_set(65, "one").tolist() == [64]
    assert all(len(CR.reset_envs(n, st)) <= 3 for n in (1, 65, 8224) for st in range(12))


def oracle_run(model, n, scenario, masked=None, steps=4):
    """The planted scenario stepped by the oracle: per step (rows fp64, running maxima, reset, info, sums0, psums0,
    sums1, psums1, reward)."""
    cfg = CR.fold_cfg(n, masked)
    c = cfg.to_c()
    env = O.OracleEnv(model, c, n)
    apply_to_arrays(startup_state(cfg, n), env.F, env.I)
    O.set_dz_count(0)
    O.cat_reset()
    env.reset()
    max_len = int(np.ceil(cfg.episode_length_s / (cfg.sim.dt * cfg.decimation)))

    def setf(name, k, envs, vals):
        env.F[F[name][0] + k, envs] = vals

    def seti(name, envs, vals):
        env.I[I[name][0], envs] = vals

    fld = lambda k: env.F[F[k][0]:F[k][0] + F[k][1]].copy()  # noqa: E731
    rng = np.random.default_rng(n)
    out = []
    for s in range(steps):
        still = CR.plant(setf, seti, n, scenario, s, np.asarray(model.q_upper), max_len)
        s0, p0 = fld("CSTR_SUM"), fld("CSTR_P")
        _, rew, term, trunc, info = env.step((0.3 * rng.normal(size=(n, 12))).astype(np.float32), s + 1)
        rows = O.cat_last_constraints(n)
        assert np.array_equal(CR.still_envs(rows), still)
        out.append(dict(rows=rows, run=O.cat_running_max(), reset=(term | trunc).astype(bool), info=info, sums0=s0,
                        psums0=p0, sums1=fld("CSTR_SUM"), psums1=fld("CSTR_P"), rew=rew))
    return c, out


@pytest.fixture(scope="module")
def runs(model):
    return {k: oracle_run(model, *k) for k in ((65, "sparse", None), (257, "mixed", None), (65, "none", None),
                                               (65, "mixed", "base_orientation"))}


@pytest.mark.parametrize("key", [(65, "sparse", None), (257, "mixed", None), (65, "none", None),
                                 (65, "mixed", "base_orientation")], ids=str)
def test_restatement_matches_the_oracle_pass(runs, key):
    c, steps = runs[key]
    max_p = np.array(c.cstr_max_p, np.float64)
    run_prev = None
    for st in steps:
        R = CR.cat_step_ref(st["rows"], run_prev, max_p, st["sums0"], st["psums0"], st["reset"], mask=c.cstr_mask,
                            clamp=1e-6)
        np.testing.assert_allclose(R["run"], st["run"], rtol=1e-12)
        np.testing.assert_allclose(st["info"]["cstr_prob"], np.where(st["reset"], 1.0, R["pmax"]), rtol=1e-6, atol=1e-7)
        np.testing.assert_array_equal(st["sums1"], R["sums"])
        np.testing.assert_allclose(st["psums1"], R["psums"], rtol=1e-6, atol=1e-7)
        if R["k"]:
            lg = st["info"]["log"]
            assert lg[NREW] == R["k"]
            np.testing.assert_allclose(lg[NREW + 4:NREW + 4 + NCSTR] / R["k"] * 100, R["log_violation"], rtol=2e-6,
                                       atol=1e-6)
            np.testing.assert_allclose(lg[NREW + 4 + NCSTR:NREW + 4 + 2 * NCSTR] / R["k"], R["log_probability"],
                                       rtol=2e-6, atol=1e-8)
        run_prev = st["run"]


@pytest.mark.parametrize("case", CR.CASES, ids=str)
def test_every_case_meets_its_coverage_conditions_on_the_oracle(model, case):
    """The GPU test's cases on the oracle's physics: the plants hold the still sets, put the column maxima into blocks of
    every maxima set and the last block, make envs reset, and reach the clamps."""
    n, scenario, masked, steps = case
    c, out = oracle_run(model, n, scenario, masked, steps)
    max_p = np.array(c.cstr_max_p, np.float64)
    cover = CR.Coverage(n, scenario)
    run_prev = None
    for st in out:
        rows = st["rows"].astype(f32)
        R = CR.cat_step_ref(rows, run_prev, max_p, st["sums0"], st["psums0"], st["reset"], mask=c.cstr_mask)
        assert R["k"] <= 64
        cover.step(rows, CR.still_masks(R["still"], n), R, st["reset"])
        run_prev = st["run"]
    cover.check()


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def emulate(st, run_prev, max_p, mask, rew_twin, fused=0, fault=None):
    """cat_handoff / cat_fold / cat_prob_* in float32 numpy on float32 rows: (snapshot, sums1, psums1, dones, rew, log).
    fused: 0 none, 1 / 2 the two fused multiply-add placements of the Polyak step and the probability's scale."""
    rows = st["rows"].astype(f32)
    n = rows.shape[1]
    reset = st["reset"]
    still = CR.still_envs(rows)
    m = len(still)
    src = still[(np.arange(n) + (fault == "remap+1")) % m] if m else np.full(n, -1)
    if fault == "no-remap":
        src = np.where(rows[CR.ROW_NOMOVE] != 0, np.arange(n), src)
    cols = rows[:CR.NCOLS].copy()
    cols[CR.NM] = rows[CR.NM][:, src] if m else 0
    use = rows.copy()
    if fault == "block-dropped" and n > 32:   # the second block's maxima never arrive
        use[:CR.NCOLS, 32:64] = -3.0e38
    cm = np.maximum(CR.column_maxima(use)[0], CR.CLAMP32)
    tau = f32(0.95)
    w_old, w_new = (f32(1) - tau, tau) if fault == "polyak-swapped" else (tau, f32(1) - tau)
    if run_prev is None:
        run = cm
    elif fused == 1:
        run = fma32(w_old, run_prev, w_new * cm)
    elif fused == 2:
        run = fma32(w_new, cm, w_old * run_prev)
    else:
        run = w_old * run_prev + w_new * cm
    rinv = f32(1) / run
    on = np.array([(mask >> t) & 1 for t in range(NCSTR)], bool)
    clip = np.clip(cols * rinv[:, None], f32(0), f32(1))
    scale = max_p[CR.COL_TERM, None] - f32(0)
    p = fma32(clip, np.broadcast_to(scale, clip.shape), np.zeros_like(clip)) if fused else f32(0) + clip * scale
    p = np.where((cols > 0) & on[CR.COL_TERM, None], p, f32(0))
    pt = np.stack([p[CR.COL0[t]:CR.COL0[t + 1]].max(axis=0) for t in range(NCSTR)])
    pmax = pt.max(axis=0)
    a = st["sums0"].astype(f32) + np.where(on[:, None], pt > 0, 0).astype(f32)
    b = np.where(on[:, None], st["psums0"].astype(f32) + pt, st["psums0"].astype(f32))
    inv_len = f32(1) / rows[CR.ROW_EPLEN]
    log = None
    k = int(reset.sum())
    if k:
        who = np.nonzero(reset)[0][1:] if fault == "log-drops-env" and k > 1 else np.nonzero(reset)[0]
        log = {}
        for t in range(NCSTR):
            if on[t]:
                sv = sp = f32(0)
                for e in who:
                    sv = f32(sv + a[t, e] * inv_len[e])
                    sp = f32(sp + b[t, e] * inv_len[e])
                log[t] = (float(f32(sv / f32(k)) * f32(100)), float(f32(sp / f32(k))))
    a[:, reset] = np.where(on[:, None], 0, a[:, reset])
    b[:, reset] = np.where(on[:, None], 0, b[:, reset])
    keep = f32(1) - pmax
    mk = CR.still_masks(still, n)
    if fault == "stale-mask" and m:
        mk[still[0] // 32] ^= np.uint32(1) << np.uint32(still[0] % 32)
    snap = dict(rows=rows, running=np.stack([run, rinv]), still_mask=mk, m=m, initialised=True,
                still_list=np.concatenate([still, np.zeros(n - m, int)]), max_p=max_p)
    return snap, a, b, np.where(reset, f32(1), pmax), rew_twin * keep, log


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("key", [(65, "sparse", None), (257, "mixed", None), (65, "none", None),
                                 (65, "mixed", "base_orientation")], ids=str)
def test_fp32_emulation_passes_every_gate(runs, key, fused):
    c, steps = runs[key]
    max_p = np.array(c.cstr_max_p, f32)
    run_prev = None
    worst = {}
    for st in steps:
        snap, a, b, dones, rew, log = emulate(st, run_prev, max_p, c.cstr_mask, st["rew"].astype(f32), fused)
        _, frac, fails = CR.check_step(snap, run_prev, st["sums0"].astype(f32), st["psums0"].astype(f32), a, b, dones,
                                       rew, st["rew"].astype(f32), st["reset"], log, False, mask=c.cstr_mask)
        assert not fails, fails
        for k, v in frac.items():
            worst[k] = max(worst.get(k, 0.0), v)
        run_prev = snap["running"][0]
    print(f"{key} fused={fused}: worst gate fractions " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1


@pytest.mark.parametrize("fault", ["no-remap", "remap+1", "block-dropped", "polyak-swapped", "log-drops-env",
                                   "stale-mask"])
def test_a_planted_fault_fails_the_check(runs, fault):
    c, steps = runs[(257, "mixed", None)]
    max_p = np.array(c.cstr_max_p, f32)
    run_prev = None
    caught = []
    for st in steps:
        good = emulate(st, run_prev, max_p, c.cstr_mask, st["rew"].astype(f32))
        snap, a, b, dones, rew, log = emulate(st, run_prev, max_p, c.cstr_mask, st["rew"].astype(f32), fault=fault)
        _, _, fails = CR.check_step(snap, run_prev, st["sums0"].astype(f32), st["psums0"].astype(f32), a, b, dones, rew,
                                    st["rew"].astype(f32), st["reset"], log, False, mask=c.cstr_mask)
        caught += fails
        run_prev = good[0]["running"][0]
    assert caught, fault
