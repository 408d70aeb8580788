"""GPU: mdp_terms -- the reward terms, `terminated` and `truncated` that step_kernel and the parity hook share -- on
the planted rows of tests/helpers/terms_ref.py, against that file's float64 restatement of the formulas.  The rows are
written into the workspace, h12env_eval_terms runs once, and every row must pass: the flags, is_terminated,
feet_air_time and every value the reference gives as exactly 0 bit-for-bit, the rest inside a gate derived from the
reference alone (terms_ref.gates: the float32 evaluation's own deviation x terms_ref.MARGIN).

Flat, Rsl, Rough and CaT cover the three kernel instantiations; Flat and Rough carry no weight on terms 12-19, so
those rows must stay exactly 0 there (on Rough inside an extended kernel), Rsl and CaT compute them.  Each config also
runs at 1 env and at 33, where the last env is alone in the second block and loads only the right leg's lane."""
import numpy as np
import pytest
import torch

import terms_ref as TR
from h12env import H12FlatEnvCfg
from h12env._abi import NREW, NREW_FLAT, REWARD_FUNCS, F, I
from h12env.cfg import H12CaTEnvCfg, H12RoughEnvCfg, H12RslEnvCfg
from h12env.env import H12VelocityEnv

pytestmark = pytest.mark.gpu
CFGS = dict(flat=H12FlatEnvCfg, rsl=H12RslEnvCfg, rough=H12RoughEnvCfg, cat=H12CaTEnvCfg)
RSL_ON = dict(flat=False, rsl=True, rough=False, cat=True)
_cache = {}


def table(name):
    """(consts, rows, float64 reference, gates) of a config: computed once, shared by its three env counts."""
    if name not in _cache:
        K = TR.consts(CFGS[name]())
        rows = TR.planted_rows(K)
        ref = TR.reference(K, rows)
        _cache[name] = (K, rows, ref, TR.gates(K, rows, ref[0]))
    return _cache[name]


def make(name, n):
    cfg = CFGS[name]()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    if name == "rough":   # a small heightfield: the terms do not read it
        g = cfg.scene.terrain.terrain_generator
        g.num_rows, g.num_cols, g.border_width = 6, 8, 5.0
    env = H12VelocityEnv(cfg)
    env.reset()
    torch.cuda.synchronize()
    return env


def put(env, name, vals):
    o, k = F[name]
    env._fstate[o:o + k] = torch.as_tensor(np.asarray(vals, np.float32).reshape(-1, k).T.copy(), device=env.device)


def load(env, rows):
    st = np.array([r["state"] for r in rows])
    env._fstate.zero_()
    for name, a in (("POS", st[:, 0:3]), ("QUAT", st[:, 3:7]), ("VLIN", st[:, 7:10]), ("WANG", st[:, 10:13]),
                    ("Q", st[:, 13:25]), ("QD", st[:, 25:37]), ("ACT", [r["act"] for r in rows]),
                    ("ACT_PREV", [r["act_prev"] for r in rows]), ("CMD", [r["cmd"] for r in rows]),
                    ("AIR", [r["air"] for r in rows]), ("CONTACT", [r["con"] for r in rows])):
        put(env, name, a)
    env._istate[I["EPLEN"][0]] = torch.as_tensor([r["eplen"] for r in rows], dtype=torch.int32, device=env.device)
    g = lambda k: torch.as_tensor(np.array([r[k] for r in rows], np.float32))  # noqa: E731
    return g("tau"), g("jacc"), g("fmax")


@pytest.mark.parametrize("n", ["all", 1, 33])
@pytest.mark.parametrize("name", list(CFGS))
def test_kernel_terms_match_the_restatement_on_planted_rows(gpu, name, n):
    K, rows, (rt, rterm, rtout), gate = table(name)
    assert K.rsl_on == RSL_ON[name]
    if n == "all":
        idx = list(range(len(rows)))
        assert len(idx) % 2 == 1 and len(idx) % 32 != 0
    else:
        sub = TR.subset_rows(rows, n)
        idx = [rows.index(r) for r in sub]
        assert len(idx) == n and (sub[-1]["fmax"][[0, 2]] == 0).all() and (sub[-1]["fmax"][[1, 3]] > 1).any()
    sel = [rows[i] for i in idx]
    env = make(name, len(sel))
    tau, jacc, fmax = load(env, sel)
    f0, i0 = env._fstate.clone(), env._istate.clone()
    terms, term, trunc, _ = env.eval_terms(tau, jacc, fmax)
    torch.cuda.synchronize()
    # the hook leaves the workspace bit-identical
    assert torch.equal(env._fstate.view(torch.int32), f0.view(torch.int32)) and torch.equal(env._istate, i0)
    got = (terms.cpu().numpy().astype(np.float64), term.cpu().numpy(), trunc.cpu().numpy())
    env.close()
    ref = (rt[:, idx], rterm[idx], rtout[idx])
    err = np.abs(got[0] - ref[0]) / np.maximum(np.abs(ref[0]), TR.SCALE)
    print(f"{name} n={len(sel)}: largest error relative to max(|ref|, 1) per term (gate {gate.max():.3g}):")
    for t in range(NREW):
        j = int(np.nanargmax(np.where(np.isfinite(err[t]), err[t], np.inf)))
        print(f"  {REWARD_FUNCS[t]:34s} {err[t, j]:.3e}  {sel[j]['label']}")
    assert np.isfinite(got[0]).all(), [sel[i]["label"] for i in np.argwhere(~np.isfinite(got[0]))[:, 1]]
    if not K.rsl_on:
        assert (got[0][NREW_FLAT:] == 0).all()
    bad = TR.mismatches(K, sel, ref, got, gate)
    assert not bad, bad[:20]


def test_rough_scan_heading_of_a_vertical_x_axis(gpu):
    """obs_frame normalises the same heading for the height scan.  With the body x axis vertical the unguarded
    0 * rsq(0) sent every ray to the heightfield's corner (a finite, constant scan); the heading is (1, 0) there, so
    the scan equals the one of the same base position at zero yaw bit for bit."""
    cfg = H12RoughEnvCfg()
    cfg.scene.num_envs = 3
    cfg.sim.device = "cuda:0"
    cfg.observations.policy.enable_corruption = False
    g = cfg.scene.terrain.terrain_generator
    g.num_rows, g.num_cols, g.border_width = 6, 8, 5.0
    env = H12VelocityEnv(cfg)
    env.reset()
    o, k = F["QUAT"]
    scans = []
    for quat in ((1.0, 0.0, 0.0, 0.0), (0.5, 0.5, 0.5, -0.5)):
        env._fstate[o:o + k] = torch.tensor(quat, device=env.device)[:, None].expand(4, 3)
        obs = env.observe()
        obs = (obs["policy"] if isinstance(obs, dict) else obs).cpu().numpy()
        assert np.isfinite(obs).all()
        scans.append(obs[:, 48:])
    env.close()
    assert np.ptp(scans[0], axis=1).max() > 1e-3       # the envs stand on relief: a scan of the corner would be flat
    assert np.array_equal(scans[0], scans[1])
