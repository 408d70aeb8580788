"""GPU: Random Network Distillation's HIP side -- the rnd_state observation group
(h12priv_observe_terms, csrc/h12_priv.hip), the fused reward step (h12learn_rnd_reward / h12learn_rnd_finish,
csrc/h12_rnd.hip), rnd.FusedRND against the torch module, the graph-captured update with the predictor in it, and
train.py --rnd --rnd_fused.

Accuracy of err: the kernel's |err - fp64| may be at most 8 times the CPU fp32 torch path's |err - fp64| on the same
row (the project's cap) plus a floor of 8 ulp of the case's largest embedding element.  The floor
covers rows where the torch path's own error happens to be (next to) zero: err's final rounding alone is up to
0.5 ulp(err), and err <= 2 sqrt(d_out) max|emb|, i.e. up to 8.1 ulp of the largest embedding at d_out = 65.
Measured ratios are in DESIGN.md section 7t."""
import copy
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from h12env import _learn, priv
from h12env import cfg as K
from h12env.env import H12VelocityEnv
from h12env.policy import FusedMLP
from h12env.ppo import EmpiricalNormalization, mlp
from h12env.rnd import FusedRND, RandomNetworkDistillation

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "h1v2-isaac_amd" / "shims"), str(ROOT / "h1v2-isaac_amd" / "scripts")]

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)
CAP = 8.0
FLOOR_ULP = 8.0


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- 1: masked rows
def make_env(name, n, terms=None, critic=True):
    cfg = getattr(K, name)()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    g = cfg.scene.terrain.terrain_generator
    if g is not None:  # a smaller grid keeps the terrain setup quick
        g.num_rows, g.num_cols, g.border_width = 6, 8, 5.0
    if critic:
        cfg.observations.critic = K.CriticObsCfg()
    cfg.observations.rnd_state = K.RndStateObsCfg() if terms is None else K.RndStateObsCfg(terms=terms)
    return H12VelocityEnv(cfg)


def step3(env, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    env.reset()
    out = None
    for _ in range(3):
        out = env.step(torch.randn(env.num_envs, 12, generator=g).to(env.device))
    return out[0]


def observe_terms(env, mask):
    lib, pc, ref, _, _ = env._rnd
    w, table = priv.layout_terms(bool(pc.terrain), mask)
    out = torch.full((env.num_envs, w), float("nan"), device=env.device)
    rc = lib.h12priv_observe_terms(env._state.data_ptr(), env.num_envs, ref, env.foot_contact_force.data_ptr(), mask,
                                   out.data_ptr(), env._stream())
    assert rc == 0, lib.h12priv_last_error()
    return out, table


def check_masks(env, obs, masks):
    full_w, full = priv.layout(env.terrain is not None)
    where = {name: (o, k) for name, o, k in full}
    crit = obs["critic"]
    assert crit.shape[1] == full_w
    for terms in masks:
        out, table = observe_terms(env, priv.term_mask(terms))
        assert [t for t, _, _ in table] == [t for t in priv.TERMS if t in terms]
        assert out.shape[1] == sum(priv.WIDTHS[t] for t in terms)
        for name, o, k in table:
            so, sk = where[name]
            assert sk == k and torch.equal(bits(out[:, o:o + k]), bits(crit[:, so:so + k])), name
    return full


@pytest.mark.timeout(120)
def test_masked_rows_are_the_full_rows_columns_flat(gpu):
    env = make_env("H12FlatEnvCfg", 64)
    obs = step3(env)
    assert env.rnd_state_dim == 36 and obs["rnd_state"].shape == (64, 36)
    names = priv.term_names(False)
    check_masks(env, obs, [K.RND_STATE_TERMS, ("feet_contact",), tuple(names)])
    whole, _ = observe_terms(env, priv.term_mask(names))
    assert torch.equal(bits(whole), bits(obs["critic"]))
    default, _ = observe_terms(env, priv.term_mask(K.RND_STATE_TERMS))
    assert torch.equal(bits(default), bits(obs["rnd_state"]))  # what step() returned is the call's output
    om = env.observation_manager
    assert om.group_obs_dim["rnd_state"] == (36,) and om.active_terms["rnd_state"] == list(K.RND_STATE_TERMS)
    assert torch.equal(om.compute()["rnd_state"], obs["rnd_state"])
    assert torch.equal(env.get_observations()["rnd_state"], obs["rnd_state"])
    # the group alone (no critic group) serves the same rows: it only reads
    alone = make_env("H12FlatEnvCfg", 64, critic=False)
    obs2 = step3(alone)
    assert set(obs2) == {"policy", "rnd_state"} and torch.equal(bits(obs2["rnd_state"]), bits(obs["rnd_state"]))
    assert torch.equal(obs2["policy"], obs["policy"])
    with pytest.raises(ValueError, match="rnd_state"):
        alone.bind_rollout(object())
    snap = alone.snapshot()
    g = torch.Generator(device="cpu").manual_seed(9)
    a = torch.randn(64, 12, generator=g).to(DEV)
    first = alone.step(a)[0]["rnd_state"].clone()
    alone.restore(snap)
    assert torch.equal(alone.step(a)[0]["rnd_state"], first)
    assert torch.equal(alone.observe()["rnd_state"], first)  # observe() of the same state: the same rows
    env.close()
    alone.close()


@pytest.mark.timeout(120)
def test_masked_rows_with_the_height_scan_rough(gpu):
    terms = ("base_lin_vel", "height_scan", "base_height", "feet_contact")
    env = make_env("H12RoughEnvCfg", 64, terms=terms)
    obs = step3(env)
    assert obs["rnd_state"].shape == (64, 3 + 187 + 1 + 2)
    names = priv.term_names(True)
    check_masks(env, obs, [terms, ("feet_contact",), K.RND_STATE_TERMS, tuple(names)])
    whole, _ = observe_terms(env, priv.term_mask(names))
    assert torch.equal(bits(whole), bits(obs["critic"]))
    mine, _ = observe_terms(env, priv.term_mask(terms))
    assert torch.equal(bits(mine), bits(obs["rnd_state"]))
    env.close()


# ---------------------------------------------------------------------------------------------- 2, 3: the reward kernel
NS = (1, 15, 16, 17, 33)


def rnd_case(d_in, d_out, norm, seed=0):
    """Predictor [32, 16] and target [8] (unequal depths) on the device, a trained state normaliser or none, the
    FusedMLP that packs them, and 33 input rows."""
    torch.manual_seed(1000 * d_in + 10 * d_out + seed)
    pred = mlp(d_in, [32, 16], d_out, "elu").to(DEV)
    tgt = mlp(d_in, [8], d_out, "elu").to(DEV)
    normalizer = None
    x = torch.randn(max(NS), d_in) * 1.5 + 0.3
    if norm:
        normalizer = EmpiricalNormalization([d_in]).train()
        normalizer(torch.randn(256, d_in) * 2.0 + 0.5)
        normalizer = normalizer.eval().to(DEV)
    f = FusedMLP([pred, tgt], normalizer)
    f.refresh()
    return pred, tgt, normalizer, f, x.to(DEV)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("d_out", [1, 16, 17, 65])
@pytest.mark.parametrize("d_in", [5, 16, 17])
def test_embeddings_are_the_forward_kernels_bits_and_err_is_within_the_cap(gpu, d_in, d_out, norm):
    pred, tgt, normalizer, f, x_all = rnd_case(d_in, d_out, norm)
    p64, t64 = copy.deepcopy(pred).cpu().double(), copy.deepcopy(tgt).cpu().double()
    p32, t32 = copy.deepcopy(pred).cpu(), copy.deepcopy(tgt).cpu()
    ratios = []
    for n in NS:
        x = x_all[:n].contiguous()
        xn = torch.full((n, d_in), float("nan"), device=DEV)
        err, e_pred, e_tgt = _learn.rnd_reward(f._desc, f._packed, x, xn=xn, emb=True)
        y_pred, y_tgt = _learn.mlp_forward(f._desc, f._packed, x)
        assert torch.equal(bits(e_pred), bits(y_pred)) and torch.equal(bits(e_tgt), bits(y_tgt))
        want_xn = (x - normalizer._mean) / (normalizer._std + normalizer.eps) if norm else x
        assert torch.equal(bits(xn), bits(want_xn))
        assert torch.equal(_learn.rnd_reward(f._desc, f._packed, x), err)  # without the optional outputs
        # err against fp64 networks on the same fp32 weights and the same normalised rows
        s = xn.cpu()
        with torch.no_grad():
            e64 = torch.linalg.norm(t64(s.double()) - p64(s.double()), dim=1)
            e32 = torch.linalg.norm(t32(s) - p32(s), dim=1)
            biggest = max(float(t64(s.double()).abs().max()), float(p64(s.double()).abs().max()))
        assert float(e64.min()) >= 1e-3, "precondition: the relative measure needs err >= 1e-3 on every row"
        mine = (err.cpu().double() - e64).abs()
        torchs = (e32.double() - e64).abs()
        floor = FLOOR_ULP * EPS32 * biggest
        ratios.append(float((mine / torchs.clamp(min=floor)).max()))
        print(f"d_in {d_in} d_out {d_out} norm {norm} n {n}: max |err - fp64| kernel {float(mine.max()):.3e} "
              f"torch {float(torchs.max()):.3e} floor {floor:.3e} worst ratio {ratios[-1]:.3f}")
        assert bool((mine <= CAP * torchs + floor).all()), (mine, torchs, floor)


# ---------------------------------------------------------------------------------------------- 4: the finish kernel
class FinishRef:
    """h12learn_rnd_finish restated in numpy fp64 (the formulas of DESIGN.md 7t)."""

    def __init__(self, gamma, until):
        self.gamma, self.until = float(np.float32(gamma)), until
        self.mean, self.var, self.std, self.count, self.avg = 0.0, 1.0, 1.0, 0, None

    def __call__(self, err, ext, weight):
        err, ext = err.astype(np.float64), ext.astype(np.float64)
        self.avg = err.copy() if self.avg is None else self.avg * self.gamma + err
        if self.count < self.until:
            n = err.shape[0]
            mean_x, var_x = self.avg.mean(), self.avg.var()
            self.count += n
            rate = n / self.count
            delta = mean_x - self.mean
            self.mean += rate * delta
            self.var += rate * (var_x - self.var + delta * (mean_x - self.mean))
            self.std = np.sqrt(self.var)
        v = err / self.std if self.std > 0 else err
        return v * weight, ext + v * weight


def finish_run(n, errs, exts, weight, until, normalize=True):
    t = lambda *s, **kw: torch.zeros(*s, device=DEV, **kw)  # noqa: E731
    avg, mean, var, std = t(n), t(1), torch.ones(1, device=DEV), torch.ones(1, device=DEV)
    count, first = t((), dtype=torch.long), torch.ones(1, dtype=torch.int32, device=DEV)
    w = torch.full((1,), weight, device=DEV)
    out = []
    for err, ext in zip(errs, exts):
        e, x = torch.from_numpy(err).to(DEV), torch.from_numpy(ext).to(DEV)
        intrinsic, total = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
        a = _learn.RndFinishArgs()
        a.n, a.normalize, a.gamma, a.until = n, int(normalize), 0.99, until
        a.err, a.ext_reward, a.weight = e.data_ptr(), x.data_ptr(), w.data_ptr()
        a.intrinsic, a.total = intrinsic.data_ptr(), total.data_ptr()
        if normalize:
            a.avg, a.mean, a.var, a.std = avg.data_ptr(), mean.data_ptr(), var.data_ptr(), std.data_ptr()
            a.count, a.first = count.data_ptr(), first.data_ptr()
        _learn.rnd_finish(a, torch.device(DEV))
        torch.cuda.synchronize()
        out.append(tuple(v.cpu().numpy().copy() for v in (intrinsic, total, avg, mean, var, std, count, first)))
    return out


@pytest.mark.timeout(60)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_finish_against_fp64_restatement(gpu, n):
    rng = np.random.default_rng(n)
    errs = [rng.uniform(0.5, 1.5, n).astype(np.float32) for _ in range(6)]
    errs[0][:] = 0.75  # an all-equal first batch: batch variance 0, running variance 0, std 0 (0.75 n is exact)
    exts = [rng.normal(0.0, 1.0, n).astype(np.float32) for _ in range(6)]
    weight, until = 0.37, 4 * n  # calls 4 and 5 find count >= until: the statistics are frozen
    got = finish_run(n, errs, exts, weight, until)
    ref = FinishRef(0.99, until)
    w32 = float(np.float32(weight))
    for k, (err, ext) in enumerate(zip(errs, exts)):
        intrinsic, total, avg, mean, var, std, count, first = got[k]
        want_i, want_t = ref(err, ext, w32)
        np.testing.assert_allclose(intrinsic, want_i, rtol=1e-5, err_msg=f"call {k}")
        assert np.array_equal(total, ext + intrinsic)  # one fp32 addition
        np.testing.assert_allclose(total, want_t, rtol=1e-5, atol=1e-5 * float(np.abs(want_i).max()))
        np.testing.assert_allclose(avg, ref.avg, rtol=1e-5)
        np.testing.assert_allclose([mean[0], var[0], std[0]], [ref.mean, ref.var, ref.std], rtol=1e-5, atol=1e-12)
        assert int(count) == ref.count == min(k + 1, 4) * n and int(first[0]) == 0
        if k == 0:
            assert std[0] == 0.0 and np.array_equal(intrinsic, err * np.float32(weight))  # std == 0: err passes
    again = finish_run(n, errs, exts, weight, until)
    for a, b in zip(got, again):
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()
    # normalisation off: exactly ext + err * weight in fp32, separately rounded
    off = finish_run(n, errs[:2], exts[:2], weight, until, normalize=False)
    for (intrinsic, total, *_), err, ext in zip(off, errs, exts):
        r = err * np.float32(weight)
        assert np.array_equal(intrinsic, r) and np.array_equal(total, ext + r)


@pytest.mark.timeout(60)
def test_finish_at_32768_envs_is_reproducible(gpu):
    n = 32768
    rng = np.random.default_rng(1)
    errs = [rng.uniform(0.5, 1.5, n).astype(np.float32) for _ in range(2)]
    exts = [rng.normal(0.0, 1.0, n).astype(np.float32) for _ in range(2)]
    a, b = finish_run(n, errs, exts, 1.0, 10 ** 8), finish_run(n, errs, exts, 1.0, 10 ** 8)
    ref = FinishRef(0.99, 10 ** 8)
    for k in range(2):
        want_i, _ = ref(errs[k], exts[k], 1.0)
        np.testing.assert_allclose(a[k][0], want_i, rtol=1e-5)
        for u, v in zip(a[k], b[k]):
            assert u.tobytes() == v.tobytes()


# ---------------------------------------------------------------------------------------------- 5: FusedRND
@pytest.mark.timeout(60)
def test_fused_rnd_against_the_torch_module_on_the_device(gpu):
    torch.manual_seed(5)
    kw = dict(num_outputs=16, predictor_hidden_dims=[64, 32], target_hidden_dims=[48], weight=0.4,
              state_normalization=True, reward_normalization=True)
    cpu32 = RandomNetworkDistillation(36, **kw).train()
    cpu64 = copy.deepcopy(cpu32).double().train()
    on_dev = copy.deepcopy(cpu32).to(DEV).train()
    fused_mod = copy.deepcopy(cpu32).to(DEV).train()
    fused = FusedRND(fused_mod)
    g = torch.Generator().manual_seed(3)
    for step in range(4):
        x = torch.randn(48, 36, generator=g) * 2.0 + 0.5
        ext = torch.randn(48, generator=g)
        r32, _ = cpu32.get_intrinsic_reward(x)
        r64, s64 = cpu64.get_intrinsic_reward(x.double())
        want, s_dev = on_dev.get_intrinsic_reward(x.to(DEV))
        intrinsic, total, s = fused(x.to(DEV), ext.to(DEV))
        with torch.no_grad():
            biggest = max(float(cpu64.target(s64).abs().max()), float(cpu64.predictor(s64).abs().max()))
        scale = 0.4 / float(cpu64.reward_normalizer._std)
        floor = FLOOR_ULP * EPS32 * biggest * scale
        diff = (intrinsic.cpu().double() - want.cpu().double()).abs()
        own = (r32.double() - r64).abs()
        print(f"step {step}: max |fused - torch| {float(diff.max()):.3e}, CPU fp32 torch's |x - fp64| "
              f"{float(own.max()):.3e}, floor {floor:.3e}")
        assert bool((diff <= CAP * own + floor).all()), (diff, own, floor)
        assert torch.equal(total, ext.to(DEV) + intrinsic)
        torch.testing.assert_close(s, s_dev, rtol=1e-6, atol=0)
        a, b = fused_mod.state_dict(), on_dev.state_dict()
        for k in a:
            if "normalizer" in k:
                torch.testing.assert_close(a[k], b[k], rtol=1e-6, atol=0, msg=k)
        assert fused_mod.update_counter == on_dev.update_counter == step + 1


# ---------------------------------------------------------------------------------------------- 6: update graph
@pytest.mark.timeout(300)
def test_graph_captured_update_with_rnd_equals_eager(gpu, monkeypatch):
    from h12env.ppo import OnPolicyRunner
    from isaaclab_rl.rsl_rl import (RslRlOnPolicyRunnerCfg, RslRlPpoActorCriticCfg, RslRlPpoAlgorithmCfg, RslRlRndCfg,
                                    RslRlVecEnvWrapper)

    def run(graph: bool):
        monkeypatch.setenv("H12_PPO_GRAPH", "1" if graph else "0")
        env = make_env("H12FlatEnvCfg", 64, critic=False)
        rnd = RslRlRndCfg(weight=5.0, state_normalization=True, reward_normalization=True, num_outputs=8,
                          predictor_hidden_dims=[64], target_hidden_dims=[32])
        c = RslRlOnPolicyRunnerCfg(seed=7, device=DEV, num_steps_per_env=4, max_iterations=1, save_interval=100,
                                   policy=RslRlPpoActorCriticCfg(actor_hidden_dims=[64], critic_hidden_dims=[64]),
                                   algorithm=RslRlPpoAlgorithmCfg(num_learning_epochs=2, num_mini_batches=4, rnd_cfg=rnd))
        r = OnPolicyRunner(RslRlVecEnvWrapper(env), c.to_dict(), device=DEV)
        target0 = copy.deepcopy(r.alg.rnd.target.state_dict())
        r.learn(1)
        torch.cuda.synchronize()
        out = (r, target0, dict(r.last_iteration_stats))
        env.close()
        return out

    (a, ta, sa), (b, tb, sb) = run(True), run(False)
    assert a.alg._graph is not None and b.alg._graph is None
    for p, q in zip(a.alg.policy.parameters(), b.alg.policy.parameters()):
        assert torch.equal(p, q), (p - q).abs().max()
    for p, q in zip(a.alg.rnd.predictor.parameters(), b.alg.rnd.predictor.parameters()):
        assert torch.equal(p, q), (p - q).abs().max()
    for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy", "Loss/rnd", "Loss/learning_rate", "Rnd/weight"):
        assert sa[k] == sb[k], k
    assert sa["Loss/rnd"] > 0 and sa["Rnd/weight"] == 5.0 * a.env.unwrapped.step_dt
    for k, v in a.alg.rnd.state_dict().items():
        assert torch.equal(v, b.alg.rnd.state_dict()[k]), k
    for r, t0 in ((a, ta), (b, tb)):
        for k, v in r.alg.rnd.target.state_dict().items():
            assert torch.equal(v, t0[k]), k
    assert torch.equal(ta["0.weight"], tb["0.weight"])


# ---------------------------------------------------------------------------------------------- 7: argument errors
def test_argument_errors_are_reported_before_any_launch(gpu):
    lib = _learn.learn_library()
    _, _, _, f, x = rnd_case(5, 3, False)
    err = torch.zeros(8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def reward(desc=f._desc, packed=f._packed.data_ptr(), xp=x.data_ptr(), n=8, e=err.data_ptr()):
        return lib.h12learn_rnd_reward(C.byref(desc), packed, xp, n, e, None, None, st)

    def unequal():
        d = _learn.MlpDesc.from_buffer_copy(f._desc)
        d.nets[1].dims[d.nets[1].n_layers] = 4
        return d

    def too_wide():
        d = _learn.MlpDesc.from_buffer_copy(f._desc)
        d.nets[0].dims[1] = _learn.mlp_max_width() + 1
        return d

    def one_net():
        d = _learn.MlpDesc.from_buffer_copy(f._desc)
        d.n_nets = 1
        return d

    for call, msg in ((lambda: reward(n=0), b"n = 0"), (lambda: reward(e=None), b"err is null"),
                      (lambda: reward(desc=unequal()), b"last width"), (lambda: reward(desc=too_wide()), b"dims[1]"),
                      (lambda: reward(desc=one_net()), b"n_nets = 1"), (lambda: reward(packed=None), b"packed is null"),
                      (lambda: reward(packed=f._packed.data_ptr() + 4), b"16-byte aligned"),
                      (lambda: reward(xp=None), b"x is null")):
        assert call() == -1 and msg in lib.h12learn_last_error(), (msg, lib.h12learn_last_error())
    assert torch.equal(err, torch.zeros(8, device=DEV))  # nothing was launched
    a = _learn.RndFinishArgs()
    assert lib.h12learn_rnd_finish(C.byref(a), st) == -1 and b"n = 0" in lib.h12learn_last_error()

    env = make_env("H12FlatEnvCfg", 64, critic=False)
    plib, pc, ref, _, _ = env._rnd
    out = torch.zeros(64, 65, device=DEV)
    args = (env._state.data_ptr(), 64, ref, None)
    assert plib.h12priv_observe_terms(*args, 0, out.data_ptr(), None) == -1
    assert b"names no term" in plib.h12priv_last_error()
    assert plib.h12priv_observe_terms(*args, 1 << priv.TERMS.index("height_scan"), out.data_ptr(), None) == -1
    assert b"height_scan on a plane task" in plib.h12priv_last_error()
    assert plib.h12priv_observe_terms(*args, 1 << len(priv.TERMS), out.data_ptr(), None) == -1
    assert b"past the table" in plib.h12priv_last_error()
    assert plib.h12priv_layout_terms(0, 0, None, None, None) == -1
    torch.cuda.synchronize()
    assert not out.any()
    with pytest.raises(ValueError, match="height_scan"):
        make_env("H12FlatEnvCfg", 64, terms=("height_scan",), critic=False)
    with pytest.raises(ValueError, match="order"):
        make_env("H12FlatEnvCfg", 64, terms=("joint_pos", "base_ang_vel"), critic=False)
    env.close()


# ---------------------------------------------------------------------------------------------- train.py
@pytest.mark.timeout(300)
def test_train_script_with_rnd_fused_on_rough_and_play_loads_the_checkpoint(gpu, tmp_path, monkeypatch):
    import train
    from h12env import ppo

    seen = []
    learn = ppo.OnPolicyRunner.learn

    def spy(self, *a, **kw):
        seen.append(self)
        return learn(self, *a, **kw)

    monkeypatch.setattr(ppo.OnPolicyRunner, "learn", spy)
    monkeypatch.chdir(tmp_path)
    argv = ["--task", "Isaac-Velocity-Rough-H12_12dof-v0", "--headless", "--num_envs", "64", "--max_iterations", "2",
            "--rnd", "--rnd_fused", "--rnd_weight", "2.0", "agent.algorithm.rnd_cfg.reward_normalization=true",
            "env.episode_length_s=0.2"]
    assert train.main(argv) == 0
    alg = seen[0].alg
    assert alg.rnd_fused is not None and alg.rnd.reward_normalization and alg.storage.t["rnd_state"].shape[2] == 36
    run = next((tmp_path / "logs" / "rsl_rl").glob("*/*"))
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2
    for key in ("Rnd/mean_extrinsic_reward", "Rnd/mean_intrinsic_reward", "Rnd/weight", "Loss/rnd"):
        assert key in lines[-1] and lines[-1][key] == lines[-1][key], key
    assert "rnd_state:" in (run / "params" / "env.yaml").read_text()
    ck = run / "model_2.pt"
    assert {"rnd_state_dict", "rnd_optimizer_state_dict"} <= set(torch.load(ck, weights_only=True))

    import gymnasium as gym
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    task = "Isaac-Velocity-Rough-H12_12dof-Play-v0"  # play.py's path: no rnd_cfg, the RND entries are ignored
    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    cfg.scene.num_envs = 16
    agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    env = RslRlVecEnvWrapper(gym.make(task, cfg=cfg))
    play = ppo.OnPolicyRunner(env, agent.to_dict(), log_dir=None, device=DEV)
    play.load(str(ck))
    policy = play.get_inference_policy(device=DEV)
    obs, _ = env.get_observations()
    with torch.inference_mode():
        for _ in range(3):
            obs, _, _, _ = env.step(policy(obs))
    assert torch.isfinite(obs).all()
    env.close()
