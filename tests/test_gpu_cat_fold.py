"""GPU: CaT's cross-env pass -- cat_handoff's column maxima and still masks, cat_fold's prefix sums, running maxima and
still list, cat_prob_inline's / cat_prob_kernel's remap, probabilities, constraint sums and episode statistics --
against the float64 restatement of one pass (tests/helpers/cat_ref.py), teacher-forced: the restatement reads the
kernel's own float32 rows, the previous step's running maxima (H12VelocityEnv.cat_snapshot) and the pre-step CSTR_SUM /
CSTR_P fields, so no fp32 contact decision of the physics enters and the gates are exact or a few u (u = 2^-24):

  exact    m, the still masks, the still list (two-kernel path), the first fold's running maxima, the reciprocals,
           CSTR_SUM, the zeroed sums and dones = 1 of reset envs, rew = fl(rew_twin fl(1 - dones)) of the others
  3 u      later folds: tau run + (1 - tau) max, two products and a sum of positive terms
  5 u max(max_p, min_p)   dones and the CSTR_P increments (+ u |CSTR_P|): reciprocal, product, scale, add
  (k + 3) u sum|terms|    the episode log of the k <= 64 resetting envs

The twin env has the same cfg, seed, plants and actions with every max_p at 0: its rewards are the unscaled ones, and
its state must equal the CaT env's bit for bit (the probabilities feed nothing but the reward, dones and the
constraint sums).  test_gpu_cat_inline.py pins the two paths to each other and test_gpu_cat.py pins them to the oracle
statistically; a fold wrong in both paths alike passes the first, and the second's gates are loose by nature.

Shapes: every size at which cat_fold / cat_prob_* take another branch -- n = 1, 31 (< 32), 33 (a last block of one
env), 65 (three step blocks: cat_prob_kernel's second block has an empty half), 257 (9 blocks: the eight maxima sets
wrap), 2085 (66 blocks: two chunks per fold lane, a partial last block), 8224 (257 blocks: the fold's reload loop; the
inline path must refuse it) -- and the still sets none (m = 0), one (in the last block), all, sparse (blocks without a
still env between blocks with some).  The measured fractions of every gate are printed per case (CaT)."""
import os

import numpy as np
import pytest
import torch

import cat_ref as CR
from h12env._abi import CONSTRAINT_TERMS, NCSTR, F, I
from h12env.env import H12VelocityEnv

pytestmark = pytest.mark.gpu

CASES = [(c, inline) for c in CR.CASES for inline in (True, False) if not (c[0] == 8224 and not inline)]


def case_id(p):
    (n, scenario, masked, steps), inline = p
    tag = f"{n}-{scenario}" + (f"-no_{masked}" if masked else "") + (f"-{steps}steps" if steps != 4 else "")
    return tag + ("-inline" if inline else "-two-kernel")


def make(cfg, inline):
    old = os.environ.get("H12_CAT_INLINE")
    os.environ["H12_CAT_INLINE"] = "1" if inline else "0"
    try:
        env = H12VelocityEnv(cfg)
    finally:
        if old is None:
            del os.environ["H12_CAT_INLINE"]
        else:
            os.environ["H12_CAT_INLINE"] = old
    env.reset()
    return env


def fields(env, name):
    o, k = F[name]
    return env._fstate[o:o + k].cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cat_pass_matches_the_restatement(gpu, model, case):
    (n, scenario, masked, steps), inline = case
    env = make(CR.fold_cfg(n, masked, device="cuda:0"), inline)
    twin = make(CR.fold_cfg(n, masked, twin=True, device="cuda:0"), inline)
    nb = (n + 31) // 32
    if nb > 256:  # 257 blocks: more than the waiting wave's four prefixes per lane -- the request is refused
        assert inline and not env.cat_inline and not twin.cat_inline
        inline = False
    else:
        assert env.cat_inline == inline and twin.cat_inline == inline
    mask, tau, min_p = env._ccfg.cstr_mask, float(env._ccfg.cat_tau), float(env._ccfg.cat_min_p)
    active = dict(env.cfg.constraints.active())
    assert (masked is None) == (mask == (1 << NCSTR) - 1)
    q_upper = np.asarray(model.q_upper, np.float64)

    def setter(e):
        def setf(name, k, envs, vals):
            e._fstate[F[name][0] + k, torch.as_tensor(envs, device=gpu)] = torch.as_tensor(vals, dtype=torch.float32,
                                                                                           device=gpu)

        def seti(name, envs, vals):
            e._istate[I[name][0], torch.as_tensor(envs, device=gpu)] = torch.as_tensor(vals, dtype=torch.int32,
                                                                                       device=gpu)
        return setf, seti

    gen = torch.Generator(device="cpu").manual_seed(n)
    run_prev = None
    worst = {}
    cover = CR.Coverage(n, scenario)
    skip = (F["CSTR_SUM"][0], F["CSTR_SUM"][0] + 2 * NCSTR)
    assert F["CSTR_P"][0] == F["CSTR_SUM"][0] + NCSTR
    for s in range(steps):
        for e in (env, twin):
            CR.plant(*setter(e), n, scenario, s, q_upper, env.max_episode_length)
        sums0, psums0 = fields(env, "CSTR_SUM"), fields(env, "CSTR_P")
        act = (0.3 * torch.randn(n, 12, generator=gen)).to(gpu)
        _, rew, dones, _, ext = env.step(act)
        _, rew_t, dones_t, _, _ = twin.step(act)
        snap = env.cat_snapshot()
        # the probabilities feed back into nothing: the twin's state (all but the constraint sums), bit for bit
        fa, fb = env._fstate.view(torch.int32), twin._fstate.view(torch.int32)
        assert torch.equal(fa[:skip[0]], fb[:skip[0]]) and torch.equal(fa[skip[1]:], fb[skip[1]:]), s
        assert torch.equal(env._istate, twin._istate), s
        assert torch.equal(env.reset_terminated, twin.reset_terminated), s
        assert torch.equal(env.reset_time_outs, twin.reset_time_outs), s
        reset = (env.reset_terminated.bool() | env.reset_time_outs.bool()).cpu().numpy()
        assert (dones_t.cpu().numpy()[~reset] == 0).all() and (fields(twin, "CSTR_SUM") == 0).all()
        log = None
        if reset.any():
            lg = ext["log"]
            log = {cid: (float(lg[f"Episode_Constraint_violation/{name}"]),
                         float(lg[f"Episode_Constraint_probability/{name}"])) for name, cid in active.items()}
            if masked:
                assert f"Episode_Constraint_violation/{masked}" not in lg
                assert f"Episode_Constraint_probability/{masked}" not in lg
        R, frac, fails = CR.check_step(snap, run_prev, sums0, psums0, fields(env, "CSTR_SUM"), fields(env, "CSTR_P"),
                                       dones.cpu().numpy(), rew.cpu().numpy(), rew_t.cpu().numpy(), reset, log, inline,
                                       tau, min_p, mask)
        print(f"{case_id(case)} step {s}: m {R['m']}, {int(reset.sum())} resets, gate fractions "
              + ", ".join(f"{k} {v:.3f}" for k, v in frac.items()))
        assert not fails, (s, fails)
        for k, v in frac.items():
            worst[k] = max(worst.get(k, 0.0), v)
        cover.step(snap["rows"], snap["still_mask"], R, reset)  # coverage, from the snapshot itself
        run_prev = snap["running"][0].copy()
    env.close()
    twin.close()
    print(f"{case_id(case)}: worst gate fractions " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    cover.check()


def test_snapshot_needs_a_cat_handle(gpu):
    from h12env import H12FlatEnvCfg
    from h12env._abi import H12EnvError

    cfg = H12FlatEnvCfg()
    cfg.scene.num_envs = 4
    cfg.sim.device = "cuda:0"
    env = H12VelocityEnv(cfg)
    with pytest.raises(H12EnvError):
        env.cat_snapshot()
    env.close()
    assert CONSTRAINT_TERMS[6] == "base_orientation"
