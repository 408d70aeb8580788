"""GPU: the on-device safety monitor of the physics-only path (physics_monitor_kernel, monitor_reduce_kernel,
h12env.safety.SafetyMonitor) and the scripts built on it.

1  observer only: the monitored call leaves the workspace bit-identical to h12env_step_physics.
2  the accumulators equal their definition: every monitor word is bitwise the numpy float32 emulation
   (tests/helpers/monitor_emulation.py) applied to the GPU's own trace, on a run with sole contact, joints beyond
   their limits and saturated torques.
3  10 + 10 substeps equal 20, bitwise; reset(mask) zeroes exactly the masked envs and their next record has rate 0.
4  the trace against the oracle, teacher-forced per control step, under the gates of
   test_contact_force_and_torque_parity (feet 1e-2 max(10 N, |F|), torques 2e-3 max(1, |tau|)); an env-substep outside
   must be threshold-sensitive in the oracle itself, and at most 2 % may be (the cap of test_gpu_mujoco_contact.py).
5  the reduce kernel on planted buffers: counts and maxima exact, fp64 sums within 1e-12 of math.fsum, bitwise
   repeatable.
6  eval_policy.py and sim2sim.py --safety in a subprocess each.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import safety_scenario as SC
from forced import unexplained_envs
from h12env import H12FlatEnvCfg, mujoco_cfg
from h12env import safety as S
from h12env._abi import MON, MON_WORDS, SUM_EXTRA, SUM_WORDS, TRACE, H12EnvError
from h12env.env import H12VelocityEnv
from monitor_emulation import emulate

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SCRIPTS = ROOT / "h1v2-isaac_amd" / "scripts"
f32 = np.float32


def make(n, cfg):
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    env = H12VelocityEnv(cfg)
    env.reset()
    return env


def clone_state(dst, src):
    dst._state.copy_(src._state)


def same_state(a, b):
    return (torch.equal(a._fstate.view(torch.int32), b._fstate.view(torch.int32)) and torch.equal(a._istate, b._istate))


def q0_of(env):
    return np.asarray(env._model.q_default, f32)


@pytest.mark.parametrize("n", [97, 1])
@pytest.mark.parametrize("cfg_fn", [mujoco_cfg, H12FlatEnvCfg], ids=["mujoco", "flat"])
def test_observer_only(gpu, cfg_fn, n):
    a, b = make(n, cfg_fn()), make(n, cfg_fn())
    clone_state(b, a)
    mon = S.SafetyMonitor(a, trace_envs=min(n, 3), vel_limit=8.0)
    rng = np.random.default_rng(3)
    for t in range(5):
        q_ref = torch.from_numpy(SC.targets(rng, q0_of(a), n, 0.3)).cuda()
        a.step_physics(q_ref, 20, monitor=mon)
        b.step_physics(q_ref, 20)
        assert same_state(a, b), t
    pe = mon.per_env()
    assert (pe["substeps"] == 100).all() and mon.trace().shape == (100, min(n, 3), 51)
    assert float(pe["tau_abs_max"].min()) > 0  # it did observe
    a.close()
    b.close()


@pytest.mark.parametrize("cfg_name", ["H12RslEnvCfg", "H12RoughEnvCfg"])
def test_observer_only_other_feature_levels(gpu, cfg_name):
    """The kernel's feature levels 1 (Rsl: per-term extras) and 2 (Rough: heightfield) are separate instantiations."""
    from h12env import cfg as cfgs

    n = 97
    a, b = make(n, getattr(cfgs, cfg_name)()), make(n, getattr(cfgs, cfg_name)())
    clone_state(b, a)
    mon = S.SafetyMonitor(a, trace_envs=2)
    rng = np.random.default_rng(4)
    for t in range(3):
        q_ref = torch.from_numpy(SC.targets(rng, q0_of(a), n, 0.3)).cuda()
        a.step_physics(q_ref, 20, monitor=mon)
        b.step_physics(q_ref, 20)
        assert same_state(a, b), t
    assert (mon.per_env()["substeps"] == 60).all()
    a.close()
    b.close()


def drop_run(n, seed=5, pre=12, trace=None, **kw):
    """Robots dropped onto the floor under random targets (plain step_physics), then a monitor."""
    env = make(n, mujoco_cfg())
    rng = np.random.default_rng(seed)
    for _ in range(pre):
        env.step_physics(torch.from_numpy(SC.targets(rng, q0_of(env), n, 0.15)).cuda(), 20)
    return env, rng, S.SafetyMonitor(env, trace_envs=n if trace is None else trace, **kw)


def emulate_env(env, trace, vel, force_limit, mon=None):
    m = env._model
    return emulate(trace, np.asarray(m.q_lower, f32), np.asarray(m.q_upper, f32), np.asarray(m.mj_frc_limit, f32),
                   np.broadcast_to(f32(vel), (12,)), force_limit, mon=mon)


def test_accumulators_equal_their_definition(gpu):
    n = 37
    env, rng, mon = drop_run(n, vel_limit=6.0)
    for _ in range(3):  # targets up to several rad off: joints reach their limits, the PD saturates
        env.step_physics(torch.from_numpy(SC.targets(rng, q0_of(env), n, 1.0)).cuda(), 20, monitor=mon)
    tr = mon.trace()
    assert tr.shape == (60, n, 51) and np.isfinite(tr).all()
    got = mon._mon.cpu().numpy()
    want = emulate_env(env, tr, 6.0, mon.force_limit)
    diff = np.argwhere(got != want)
    assert diff.size == 0, (diff[:8], got[tuple(diff[0])], want[tuple(diff[0])])
    force = tr[..., TRACE["FORCE"][0]:TRACE["FORCE"][0] + 2]
    share = float((force > 0).any(axis=-1).mean())
    pv = int(got[MON["POS_VIOL_COUNT"][0]:MON["POS_VIOL_COUNT"][0] + 12].sum())
    sat = int(got[MON["TAU_SAT_COUNT"][0]:MON["TAU_SAT_COUNT"][0] + 12].sum())
    print(f"sole contact in {share:.2f} of env-substeps; {pv} position violations, {sat} saturated torques, "
          f"{int(got[MON['QD_VIOL_COUNT'][0]:MON['QD_VIOL_COUNT'][0] + 12].sum())} velocity violations")
    assert share > 0.3 and pv >= 1 and sat >= 1
    assert (got[MON["CONTACT_SUBSTEPS"][0]] > 0).any() and got.view(f32)[MON["FORCE_SUM"][0]].max() > 0
    # per_env() views are the same memory, named
    pe = mon.per_env()
    assert pe["pos_viol_count"].dtype == torch.int32 and pe["pos_viol_count"].shape == (12, n)
    assert pe["force_max"].dtype == torch.float32 and pe["force_max"].data_ptr() == mon._mon[MON["FORCE_MAX"][0]].data_ptr()
    # and the summary is the fold of these words
    d = mon.summary()
    assert d["substeps"] == 60 * n and d["num_envs"] == n
    assert sum(j["pos_viol_count"] for j in d["joints"].values()) == pv
    env.close()


def test_split_invariance_and_reset(gpu):
    n = 37
    a, rng, mon_a = drop_run(n, trace=0)
    b = make(n, mujoco_cfg())
    clone_state(b, a)
    mon_b = S.SafetyMonitor(b)
    for _ in range(2):
        q_ref = torch.from_numpy(SC.targets(rng, q0_of(a), n, 0.6)).cuda()
        a.step_physics(q_ref, 20, monitor=mon_a)
        b.step_physics(q_ref, 10, monitor=mon_b)
        b.step_physics(q_ref, 10, monitor=mon_b)
        assert torch.equal(mon_a._mon, mon_b._mon) and same_state(a, b)
    before = mon_a._mon.clone()
    mask = torch.from_numpy(np.random.default_rng(0).random(n) < 0.4).cuda()
    assert 0 < int(mask.sum()) < n
    mon_a.reset(mask)
    assert (mon_a._mon[:, mask] == 0).all() and torch.equal(mon_a._mon[:, ~mask], before[:, ~mask])
    q_ref = torch.from_numpy(SC.targets(rng, q0_of(a), n, 0.6)).cuda()
    a.step_physics(q_ref, 1, monitor=mon_a)
    pe = mon_a.per_env()
    assert (pe["substeps"][mask] == 1).all() and (pe["substeps"][~mask] == 41).all()
    for k in ("tau_rate_sum", "tau_rate_max", "q_rate_sum", "q_rate_max"):
        assert (pe[k][:, mask] == 0).all(), k  # the first record after a reset has rate 0
    assert (pe["tau_rate_max"][:, ~mask].max(dim=0).values > 0).all()  # a new target: the others see a torque step
    assert (pe["tau_prev"][:, mask].abs().max(dim=0).values > 0).all()
    # trace range beyond n is refused by the entry point (before any launch)
    with pytest.raises(H12EnvError, match="beyond n = 37"):
        bad = S.SafetyMonitor(a, trace_envs=n)
        bad.n_trace = n + 1
        a.step_physics(q_ref, 1, monitor=bad)
    a.close()
    b.close()


def test_trace_against_oracle_teacher_forced(gpu):
    n, steps = SC.TRACE_N, SC.TRACE_STEPS
    env = make(n, mujoco_cfg())
    mon = S.SafetyMonitor(env, trace_envs=n)
    rng = np.random.default_rng(SC.TRACE_SEED)
    off = contact = 0
    tq, ff = TRACE["TAU"][0], TRACE["FORCE"][0]
    for t in range(steps):
        F0 = env._fstate.cpu().numpy().copy()
        I0 = env._istate.cpu().numpy().copy()
        q_ref = SC.targets(rng, q0_of(env), n, SC.TRACE_SCALE)
        env.step_physics(torch.from_numpy(q_ref).cuda(), SC.N_SUB, monitor=mon)
        tr = mon._trace[-1].cpu().numpy()  # [20][n][51]
        assert np.isfinite(tr).all()
        # record k holds the state BEFORE substep k: record 0 is the snapshot
        assert (tr[0, :, TRACE["Q"][0]:TRACE["Q"][0] + 12].T == F0[13:25]).all()
        g = np.concatenate([tr[..., tq:tq + 12], tr[..., ff:ff + 2]], axis=-1).transpose(1, 0, 2).astype(np.float64)

        def rerun(Fp):
            return SC.oracle_records(env._model, env._ccfg, Fp, I0, q_ref)

        err = lambda x, b: SC.record_err(x, b).max(axis=1)  # noqa: E731
        base = rerun(F0)
        e = SC.record_err(g, base)
        gerr = e.max(axis=1)
        bad = unexplained_envs(F0, gerr, 1.0, rerun, err, base, g, seed=t)
        assert bad.size == 0, (t, bad[:8], gerr[bad[:8]])
        off += int((e > 1.0).sum())
        contact += int((base[..., 12:] > 0).any(axis=-1).sum())
    total = n * steps * SC.N_SUB
    print(f"env-substeps outside the gates {off} of {total} (all threshold-sensitive); sole contact in "
          f"{contact / total:.2f} of env-substeps")
    assert contact / total > 0.3
    assert off <= 0.02 * total
    env.close()


def test_foot_force_is_the_mean_over_inner_steps(gpu):
    """Two inner steps per substep (the MuJoCo-mode default is one, where a missing division by the inner-step count
    cannot show): the traced foot force is the mean over the inner steps, as the oracle's contact report -- same gates,
    same threshold-sensitivity rule and cap as the trace test, on a short run after the drop."""
    n, steps = 32, 6
    cfg = mujoco_cfg()
    cfg.sim.inner_steps = 2
    env = make(n, cfg)
    rng = np.random.default_rng(7)
    for _ in range(10):
        env.step_physics(torch.from_numpy(SC.targets(rng, q0_of(env), n, SC.TRACE_SCALE)).cuda(), SC.N_SUB)
    mon = S.SafetyMonitor(env, trace_envs=n)
    ff = TRACE["FORCE"][0]
    off = loaded = 0
    for t in range(steps):
        F0 = env._fstate.cpu().numpy().copy()
        I0 = env._istate.cpu().numpy().copy()
        q_ref = SC.targets(rng, q0_of(env), n, SC.TRACE_SCALE)
        env.step_physics(torch.from_numpy(q_ref).cuda(), SC.N_SUB, monitor=mon)
        tr = mon._trace[-1].cpu().numpy()
        g = np.concatenate([tr[..., TRACE["TAU"][0]:TRACE["TAU"][0] + 12], tr[..., ff:ff + 2]], axis=-1)
        g = g.transpose(1, 0, 2).astype(np.float64)

        def rerun(Fp):
            return SC.oracle_records(env._model, env._ccfg, Fp, I0, q_ref)

        err = lambda x, b: SC.record_err(x, b).max(axis=1)  # noqa: E731
        base = rerun(F0)
        e = SC.record_err(g, base)
        bad = unexplained_envs(F0, e.max(axis=1), 1.0, rerun, err, base, g, seed=t)
        assert bad.size == 0, (t, bad[:8], e.max(axis=1)[bad[:8]])
        off += int((e > 1.0).sum())
        loaded += int((base[..., 12:] > 50.0).any(axis=-1).sum())
    total = n * steps * SC.N_SUB
    assert loaded > 0.3 * total  # feet carrying load: a factor 2 in the force is far outside the gate
    assert off <= 0.02 * total
    env.close()


@pytest.mark.parametrize("n", [1, 37, 97, 4097])
def test_reduce_on_planted_buffers(gpu, n):
    env = make(n, mujoco_cfg())
    mon = S.SafetyMonitor(env)
    rng = np.random.default_rng(n)
    planted = np.zeros((MON_WORDS, n), np.int32)
    for name, (off, cnt) in MON.items():
        if S._kind(name) == "count":
            planted[off:off + cnt] = rng.integers(0, 100000, size=(cnt, n)) * (rng.random((cnt, n)) < 0.3)
        else:  # non-negative floats over ten decades (the "previous record" words too: the fold must ignore them)
            planted[off:off + cnt] = np.exp(rng.uniform(-12, 12, size=(cnt, n))).astype(f32).view(np.int32)
    mon._mon.copy_(torch.from_numpy(planted))
    w1 = mon.summary_words().cpu().numpy().copy()
    w2 = mon.summary_words().cpu().numpy().copy()
    assert (w1 == w2).all()  # bitwise repeatable
    want = S.fold_monitor_host(planted)
    d1, dw = w1.view(np.float64), want.view(np.float64)
    for name, (off, cnt) in MON.items():
        kind = S._kind(name)
        for w in range(off, off + cnt):
            if kind == "sum":
                assert abs(d1[w] - dw[w]) <= 1e-12 * abs(dw[w]), (name, w, d1[w], dw[w])
            else:  # counts, maxima, zeroed words: exact
                assert w1[w] == want[w], (name, w, w1[w], want[w])
    for k, w in SUM_EXTRA.items():
        assert w1[w] == want[w], k
    assert w1.shape == (SUM_WORDS,) and w1[SUM_EXTRA["ENVS"]] == n
    env.close()


def test_eval_policy_and_sim2sim_safety_scripts(gpu, tmp_path):
    from h12env.export import export_policy_as_jit, write_env_yaml
    from h12env.ppo import ActorCritic

    torch.manual_seed(0)
    pol = ActorCritic(450, 450, 12, [64, 32], [64, 32])
    for p in pol.actor.parameters():
        p.data.mul_(0.01)  # near-zero actions: the robot stands under the default-pose PD
    d = tmp_path / "policy"
    export_policy_as_jit(pol, None, str(d))
    write_env_yaml(H12FlatEnvCfg(), str(d / "env.yaml"))
    envv = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT / "h1v2-isaac_amd"), os.environ.get("PYTHONPATH", "")]))
    log = tmp_path / "log"
    p = subprocess.run([sys.executable, str(SCRIPTS / "eval_policy.py"), str(d), "--num_envs", "64", "--episode_length",
                        "0.5", "--trace_envs", "2", "--fused", "--log_dir", str(log)], cwd=tmp_path, env=envv,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for title in ("Avg Action Rate:", "Avg Force and Max Force:", "Position Violations:", "envs with any violation:"):
        assert title in p.stdout
    ev = json.loads((log / "eval.json").read_text())
    steps = 25
    assert ev["summary"]["substeps"] == 64 * steps * 20 and ev["run"]["num_envs"] == 64
    for i in (0, 1):
        assert (log / f"env_{i}" / "metrics.json").exists() and (log / f"env_{i}" / "safety_check.json").exists()
    m = json.loads((log / "env_0" / "metrics.json").read_text())
    assert len(m) == 20 * steps + 1 and set(m[0]) == {"joint_pos_limits", "total_mass_force"}
    assert S.check_safety(log / "env_0" / "metrics.json") == json.loads((log / "env_0" / "safety_check.json").read_text())
    tau = np.array([list(r["applied_torques"].values()) for r in m[1:]])
    force = np.array([list(r["foot_contact_forces"].values()) for r in m[1:]])
    assert (np.abs(tau).max(axis=1) > 0).all()           # real torques in every record
    assert (force[-200:].sum(axis=1) > 100.0).all()      # standing: the feet carry the robot
    assert 0.85 < m[-1]["base_lin_pos"][2] < 1.2
    p = subprocess.run([sys.executable, str(SCRIPTS / "sim2sim.py"), str(d), "--num_envs", "64", "--episode_length",
                        "0.2", "--safety"], cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "Avg Action Rate:" in p.stdout and "[sim2sim] 64 envs" in p.stdout
