"""CPU: the reward / termination restatement (tests/helpers/terms_ref.py) and its planted rows.

* the oracle (orc_mdp_terms) against the restatement on every row, Flat and Rsl configs: analytic terms to 1e-12
  relative, feet_slide to the finite-difference error bounded from the step size;
* the restatement against itself: the Jacobian foot velocity equals the finite-difference one, a reflection through
  the pelvis xz-plane and a turn of the world about z leave every term unchanged, and the float32 evaluation takes
  the float64 one's branch on every row (so no row needs excusing on the GPU);
* discrimination: every single misreading of terms_ref.MUTATIONS moves at least one row past the gate the GPU test
  (tests/test_gpu_terms_planted.py) applies, so a row set that could not catch it fails here."""
import numpy as np
import pytest

import oracle as O
import terms_ref as TR
from h12env._abi import NREW, NREW_FLAT, REWARD_FUNCS
from h12env.cfg import H12FlatEnvCfg, H12RslEnvCfg

CFGS = {"flat": H12FlatEnvCfg, "rsl": H12RslEnvCfg}
SLIDE = TR.RID["feet_slide"]
_cache = {}


def table(name):
    """(cfg, consts, rows, float64 reference) of a config, computed once."""
    if name not in _cache:
        cfg = CFGS[name]()
        K = TR.consts(cfg)
        rows = TR.planted_rows(K)
        _cache[name] = (cfg, K, rows, TR.reference(K, rows))
    return _cache[name]


def close(a, b, rel=1e-12):
    """1e-12 relative; a value far below 1 is a difference of O(1) inputs (a residual velocity component, an excess
    over a limit) and carries their rounding, so the error is measured against max(|value|, term scale)."""
    return abs(a - b) <= rel * max(abs(b), TR.SCALE)


def test_rows_are_float32_exact_and_fill_no_block():
    _, K, rows, _ = table("rsl")
    assert len(rows) % 2 == 1 and len(rows) % 32 != 0
    assert len({r["label"] for r in rows}) == len(rows)
    for r in rows:
        for k in ("state", "act", "act_prev", "cmd", "air", "con", "tau", "jacc", "fmax"):
            a = np.asarray(r[k], np.float64)
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a), (r["label"], k)
    for n in (1, 33):
        sub = TR.subset_rows(rows, n)
        assert len(sub) == n
        f = sub[-1]["fmax"]
        assert (f[0] <= 1 and f[1] > 1 and f[2] == 0) or (f[2] == 0 and f[3] > K.contact_threshold), sub[-1]["label"]


@pytest.mark.parametrize("name", list(CFGS))
def test_float32_takes_the_float64_branch_on_every_row(name):
    _, K, rows, _ = table(name)
    for r in rows:
        t64, term64, out64, i64 = TR.evaluate(K, r, slide="jac")
        t32, term32, out32, i32 = TR.evaluate(K, r, dtype=np.float32, slide="jac")
        assert i32["branch"] == i64["branch"] and (term32, out32) == (term64, out64), r["label"]
        assert np.isfinite(t64).all() and np.isfinite(t32).all(), r["label"]
        # the values the GPU test asks to be exactly 0 are exactly 0 in float32 too (an exponential may underflow)
        alg = [t for t in range(NREW) if not REWARD_FUNCS[t].endswith("_exp")]
        assert ((t64 == 0) == (t32 == 0))[alg].all(), r["label"]


@pytest.mark.parametrize("name", list(CFGS))
def test_oracle_matches_restatement_on_every_row(name, model):
    cfg, K, rows, (rt, rterm, rtout) = table(name)
    c = cfg.to_c()
    nt = NREW if K.rsl_on else NREW_FLAT      # the oracle always fills rows 12-19; the Flat table does not weigh them
    worst = np.zeros(NREW)
    for i, r in enumerate(rows):
        f = r["fmax"]
        ti = O.term_in(r["state"], r["act"], r["act_prev"], r["cmd"], r["air"], r["con"], r["tau"], r["jacc"],
                       f[0:2], f[2:4], f[4], r["eplen"])
        ot, oterm, otout = O.mdp_terms(model, c, ti)
        assert (oterm, otout) == (bool(rterm[i]), bool(rtout[i])), r["label"]
        for t in range(nt):
            want = rt[t, i]
            if t == SLIDE:
                bound = (TR.fd_error_bound(K, r["state"]) * (f[0:2] > 1)).sum()
                assert abs(ot[t] - want) <= bound, (r["label"], ot[t], want, bound)
            else:
                assert close(ot[t], want), (r["label"], REWARD_FUNCS[t], ot[t], want)
            if want != 0:
                worst[t] = max(worst[t], abs(ot[t] - want) / max(abs(want), TR.SCALE))
    print("largest oracle error relative to max(|ref|, 1):", dict(zip(REWARD_FUNCS, worst)))


def test_jacobian_foot_velocity_equals_the_finite_difference():
    _, K, rows, _ = table("rsl")
    moving = 0
    for r in rows:
        a, b = TR.foot_vel_fd(K, r["state"]), TR.foot_vel_jac(K, r["state"])
        bound = TR.fd_error_bound(K, r["state"])
        assert (np.linalg.norm(a - b, axis=1) <= bound).all(), (r["label"], a, b, bound)
        # the bound is worth something: far below the speeds on the rows where feet_slide is on
        if (r["fmax"][0:2] > 1).any() and np.linalg.norm(b) > 0.1:
            moving += 1
            assert bound.max() < 1e-7 * np.linalg.norm(b, axis=1).max(), (r["label"], bound)
    assert moving >= 20


@pytest.mark.parametrize("what", ["mirror", "rotation"])
def test_symmetry_leaves_every_term_unchanged(what):
    _, K, rows, _ = table("rsl")
    for r in rows:
        if what == "mirror":
            K2, r2 = TR.mirror_consts(K), TR.mirror_row(r)
        else:
            K2, r2 = K, TR.rotate_row(r, 1.234)
        if r["label"] == "track/vertical_x_axis":
            continue   # the heading of a vertical x axis is a convention (atan2(0, 0)), not a geometric quantity
        if what == "rotation" and r["label"].startswith("term/div_v"):
            continue   # the divergence guard bounds the world-axis components of v: a rule of this port, not a norm
        t1, term1, out1, _ = TR.evaluate(K, r, slide="jac")
        t2, term2, out2, _ = TR.evaluate(K2, r2, slide="jac")
        assert (term1, out1) == (term2, out2), r["label"]
        # 1e-12 of the larger of the value and the term scale: the transformed inputs are rounded once more
        assert (np.abs(t1 - t2) <= 1e-12 * np.maximum(np.abs(t1), TR.SCALE)).all(), (r["label"], t1 - t2)


def test_reference_passes_its_own_gate_and_the_gate_is_tight():
    _, K, rows, ref = table("rsl")
    gate = TR.gates(K, rows, ref[0])
    print("gates:", dict(zip(REWARD_FUNCS, gate)))
    assert TR.mismatches(K, rows, ref, ref, gate) == []
    t32 = np.array([TR.evaluate(K, r, dtype=np.float32, slide="jac")[0].astype(np.float64) for r in rows]).T
    assert TR.mismatches(K, rows, ref, (t32, ref[1], ref[2]), gate) == []
    # float32 carries 7 digits: a gate wider than 1e-4 would mean a row sits where the definition itself loses four
    assert gate.max() < 1e-4 and gate.min() >= TR.MARGIN * TR.FLOOR


@pytest.mark.parametrize("mut", TR.MUTATIONS)
def test_planted_rows_catch_every_single_misreading(mut):
    _, K, rows, ref = table("rsl")
    gate = TR.gates(K, rows, ref[0]) if "gate" not in _cache else _cache["gate"]
    _cache["gate"] = gate
    got = [TR.evaluate(K, r, slide="jac", mut=mut) for r in rows]
    got = (np.array([g[0] for g in got]).T, np.array([g[1] for g in got]), np.array([g[2] for g in got]))
    bad = TR.mismatches(K, rows, ref, got, gate)
    assert bad, f"no planted row notices {mut}"
