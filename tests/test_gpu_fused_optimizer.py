"""GPU: the fused optimiser step (h12learn_optim_step, csrc/h12_optim.hip; h12env.optim.FusedClipAdam / FusedClipRAdam;
``fused_optimizer`` of both trainers).  DESIGN.md section 7u.  u = 2^-24, C = the chunk, K = the table's capacity, F = the
partial sums the fold stages at a time.

Gate 1  against fp64: torch's own Adam / RAdam after clip_grad_norm_ on float64 CPU copies (tests/helpers/optim_ref.py).
        After every one of eight steps from zero state, for p, exp_avg and exp_avg_sq, the kernel's worst error is at most
        FACTOR x the worst error of the same torch classes in fp32 on the device + u max|ref|.  Also there: grad_norm
        within 2 u of the fp64 norm, and the step tensors read 1..8.
        The size sets [1] and [3] run TINY_SEQUENCES independently seeded sequences each, and the worst errors of a step
        are taken over all of them.  The worst error of one number is no measure of what fp32 costs: it is anywhere between
        0 and an ulp, and so is the yardstick's.  Measured on the MI355X with one sequence (seed 1), [1], lr on the device,
        max_norm 1: after step 7 exp_avg is 0.1375877 in fp64, the kernel's is one ulp (1.484e-08) away and torch's fp32
        happens to be 6.2e-11 away, a ratio of 107.7, while on all other 23 rows of that sequence the two agree bit for bit.
        The step is a clipped one: g' = g / (|g| + 1e-6) lies just under 1, the kernel narrows a double coefficient once
        where torch rounds |g| + 1e-6 and the quotient in fp32, so g' differs in its last bit and either side can land
        nearer.  An ulp after seven steps of an fp32 moving average is what any fp32 state carries; no bound of this form
        holds for a single number against a yardstick that can be exact by chance.  Over 16 sequences the yardstick's
        worst error is a stable half ulp and the gate is the issue's, FACTOR and allowance unchanged.
Gate 2  planted: all-zero gradients, a parameter without a gradient.
Gate 3  bitwise: run to run; a captured step against eager over three replays.
Gate 4  the trainers: CleanRL on the CaT task and ppo.PPO at 64 envs x 24 steps with the switch on, graphed == eager bit
        for bit; the binding's call counts; the default run never reaches it; checkpoints both ways.
"""
import json
import math
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
SHIMS = ROOT / "h1v2-isaac_amd" / "shims"
for p in (str(SHIMS), str(ROOT / "tests" / "helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

import optim_ref as R  # noqa: E402
from h12env import _learn, cleanrl  # noqa: E402
from h12env import optim as O  # noqa: E402

pytestmark = pytest.mark.gpu

U = R.U
FACTOR = 2.0  # the smallest power of two above the worst measured ratio (1.31, exp_avg_sq of [1] at step 7)
DEV = "cuda:0"
QUANTITIES = ("p", "exp_avg", "exp_avg_sq")
SIZE_SETS = ("one", "three", "C-1,C,C+1", "2C+1,1,12,5", "K+1 of 7", "misaligned", "agent", "F+1 blocks")
TINY_SEQUENCES = 16  # of the size sets with fewer than 64 elements: see gate 1 above


def fused_class(rule):
    return {"adam": O.FusedClipAdam, "radam": O.FusedClipRAdam}[rule]


def agent_params():
    envs = SimpleNamespace(unwrapped=SimpleNamespace(single_observation_space={"policy": SimpleNamespace(shape=(270,))},
                                                     single_action_space=SimpleNamespace(shape=(12,))))
    torch.manual_seed(11)
    return list(cleanrl.Agent(envs).parameters())


def make_case(name, seed=1):
    c, k, f = _learn.optim_chunk(), _learn.optim_max_tensors(), _learn.optim_fold()
    if name == "agent":
        case = R.make_case(None, seed, params=agent_params())
        assert len(case.sizes) == 17
        return case
    if name == "misaligned":
        return R.make_case([c + 1, 12], seed, offset=1)
    sizes = {"one": [1], "three": [3], "C-1,C,C+1": [c - 1, c, c + 1], "2C+1,1,12,5": [2 * c + 1, 1, 12, 5],
             "K+1 of 7": [7] * (k + 1), "F+1 blocks": [c * f + 1]}[name]
    return R.make_case(sizes, seed)


def run_fused(case, rule, lr_mode, lr, max_norm, beta2=0.999):
    """The case through the fused class on the device: per step the snapshot, the norm and the step tensors."""
    ps = R.device_params(case, DEV)
    lr_arg = torch.tensor(lr, dtype=torch.float32, device=DEV) if lr_mode == "dev" else lr
    opt = fused_class(rule)(ps, lr=lr_arg, max_norm=max_norm, **R.rule_kwargs(rule, beta2))
    steps, norms, counts = [], [], []
    for gs in case.grads:
        for p, g_ in zip(ps, gs):
            p.grad = g_.to(DEV)
        opt.step()
        steps.append(R.snapshot(ps, opt))
        norms.append(float(opt.last_grad_norm))
        counts.append({float(opt.state[p]["step"]) for p in ps})
    return SimpleNamespace(steps=steps, norms=norms, counts=counts, opt=opt, params=ps)


def gate1(cases, rule, lr_mode, max_norm, tag, beta2=0.999):
    """``cases``: one case, or the independently seeded sequences of a tiny size set, whose worst errors are pooled."""
    cases = cases if isinstance(cases, list) else [cases]
    # the device scalar is fp32: both references take the value it holds
    lr = float(torch.tensor(R.LR, dtype=torch.float32)) if lr_mode == "dev" else R.LR
    refs = [R.run_torch(c, rule, torch.float64, "cpu", lr, max_norm, beta2) for c in cases]
    t32s = [R.run_torch(c, rule, torch.float32, DEV, lr, max_norm, beta2) for c in cases]
    gots = [run_fused(c, rule, lr_mode, lr, max_norm, beta2) for c in cases]
    rows = []
    for s in range(cases[0].steps):
        for qi, q in enumerate(QUANTITIES):
            ek, scale = map(max, zip(*(R.worst(g.steps[s][qi], r.steps[s][qi]) for g, r in zip(gots, refs))))
            et = max(R.worst(t.steps[s][qi], r.steps[s][qi])[0] for t, r in zip(t32s, refs))
            ratio = max(0.0, ek - U * scale) / et if et > 0 else (0.0 if ek <= U * scale else math.inf)
            rows.append((s + 1, q, ek, et, scale))
            print(f"GATE1 {tag} step {s + 1} {q}: kernel {ek:.3e} torch32 {et:.3e} max|ref| {scale:.3e} ratio {ratio:.2f}")
        for case, got in zip(cases, gots):
            assert got.counts[s] == {float(s + 1)}, (s, got.counts[s])
            rel = abs(got.norms[s] - case.norms[s]) / case.norms[s]
            print(f"NORM {tag} step {s + 1}: kernel {got.norms[s]!r} fp64 {case.norms[s]!r} rel {rel:.3e}")
            assert rel <= 2 * U, (s, got.norms[s], case.norms[s])
    if max_norm is not None:  # the reference clipped on the steps the helper promised
        for case, ref in zip(cases, refs):
            assert [n > max_norm for n in ref.norms] == [n > max_norm for n in case.norms]
    for s, q, ek, et, scale in rows:
        assert ek <= FACTOR * et + U * scale, (tag, s, q, ek, et, scale)
    return refs[0], gots[0]


@pytest.mark.parametrize("rule", ["adam", "radam"])
@pytest.mark.parametrize("sizes", SIZE_SETS)
def test_eight_steps_against_fp64(gpu, rule, sizes):
    case = make_case(sizes)
    cases = case
    if sum(case.sizes) < 64:
        cases = [make_case(sizes, seed=1 + i) for i in range(TINY_SEQUENCES)]
    if sizes == "F+1 blocks":
        assert _learn.optim_workspace_bytes(case.sizes) == 8 * (_learn.optim_fold() + 1)
    if sizes == "K+1 of 7":
        assert len(case.sizes) == _learn.optim_max_tensors() + 1
    for lr_mode in ("dev", "host"):
        for max_norm in (R.MAX_NORM, None):
            ref, got = gate1(cases, rule, lr_mode, max_norm, f"{rule} [{sizes}] lr={lr_mode} max_norm={max_norm}")
    if sizes == "misaligned":
        assert all(p.data_ptr() % 16 == 4 for p in got.params)
    # every step moved every tensor, and eight steps cross RAdam's threshold: steps 1..5 plain, 6.. rectified
    assert all(not torch.equal(a, b) for a, b in zip(ref.steps[0][0], ref.steps[-1][0]))


def test_radam_with_beta2_09(gpu):
    """rho_inf = 19: rho_t = 4.58 at step 5 and 5.39 at step 6, so eight steps cross the threshold here too, with
    bias corrections and a rectification factor far from those of 0.999."""
    rho = lambda s, b=0.9: 19.0 - 2 * s * b ** s / (1 - b ** s)  # noqa: E731
    assert rho(5) < 4.6 and rho(6) > 5.3
    gate1(make_case("2C+1,1,12,5", seed=3), "radam", "dev", R.MAX_NORM, "radam beta2=0.9", beta2=0.9)


# ---------------------------------------------------------------------------------------------- gate 2
@pytest.mark.parametrize("rule", ["adam", "radam"])
def test_zero_gradients_and_a_parameter_without_gradient(gpu, rule):
    c = _learn.optim_chunk()
    case = R.make_case([c + 1, 5, 9], seed=5)
    ps = R.device_params(case, DEV)
    before = [p.detach().clone() for p in ps]
    opt = fused_class(rule)(ps, lr=torch.tensor(R.LR, device=DEV), max_norm=R.MAX_NORM, **R.rule_kwargs(rule))
    for p in ps[:2]:
        p.grad = torch.zeros_like(p)
    opt.step()
    for p, b in zip(ps, before):
        assert torch.equal(p.detach().view(torch.int32), b.view(torch.int32))  # bitwise: the sign of a zero too
    for p in ps[:2]:
        st = opt.state[p]
        assert float(st["step"]) == 1.0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert float(opt.last_grad_norm) == 0.0
    assert len(opt.state[ps[2]]) == 0  # no gradient: no state, no step
    # and with gradients on the two others the third still stays out of it
    for p, g_ in zip(ps[:2], case.grads[0]):
        p.grad = g_.to(DEV)
    opt.step()
    assert torch.equal(ps[2], before[2]) and len(opt.state[ps[2]]) == 0
    assert not torch.equal(ps[0], before[0]) and float(opt.state[ps[0]]["step"]) == 2.0
    want = math.sqrt(sum(float((g_.double() ** 2).sum()) for g_ in case.grads[0][:2]))
    assert abs(float(opt.last_grad_norm) - want) <= 2 * U * want


# ---------------------------------------------------------------------------------------------- gate 3
@pytest.mark.parametrize("rule", ["adam", "radam"])
def test_bitwise_run_to_run(gpu, rule):
    case = make_case("2C+1,1,12,5", seed=7)
    a = run_fused(case, rule, "dev", R.LR, R.MAX_NORM)
    b = run_fused(case, rule, "dev", R.LR, R.MAX_NORM)
    for sa, sb in zip(a.steps, b.steps):
        assert all(torch.equal(x, y) for qa, qb in zip(sa, sb) for x, y in zip(qa, qb))
    assert a.norms == b.norms and all(math.isfinite(n) for n in a.norms)


@pytest.mark.parametrize("rule", ["adam", "radam"])
def test_captured_step_equals_eager_over_three_replays(gpu, rule):
    """The gradients are rewritten in place and the device learning rate changes between the replays: the graph reads
    both, and the step tensors, from the addresses it captured."""
    case = make_case("2C+1,1,12,5", seed=9)
    lrs = (1e-3, 5e-4, 2e-3)

    def setup():
        ps = R.device_params(case, DEV)
        for p in ps:
            p.grad = torch.zeros_like(p)
        lr = torch.tensor(0.0, device=DEV)
        return ps, lr, fused_class(rule)(ps, lr=lr, max_norm=R.MAX_NORM, **R.rule_kwargs(rule))

    ps, lr, opt = setup()
    eager = []
    for s in range(3):
        lr.fill_(lrs[s])
        for p, g_ in zip(ps, case.grads[s]):
            p.grad.copy_(g_)
        opt.step()
        eager.append((R.snapshot(ps, opt), float(opt.last_grad_norm)))

    ps, lr, opt = setup()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()  # warm-up: creates the state and the workspace (zero gradients, lr 0: p stays)
    torch.cuda.current_stream().wait_stream(side)
    for p in ps:
        for t in opt.state[p].values():
            t.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    for s in range(3):
        lr.fill_(lrs[s])
        for p, g_ in zip(ps, case.grads[s]):
            p.grad.copy_(g_)
        g.replay()
        snap, norm = eager[s]
        assert all(torch.equal(x, y) for qa, qb in zip(R.snapshot(ps, opt), snap) for x, y in zip(qa, qb)), s
        assert float(opt.last_grad_norm) == norm and {float(opt.state[p]["step"]) for p in ps} == {float(s + 1)}
    assert eager[0][1] > R.MAX_NORM > eager[1][1]  # a clipped and an unclipped replay


# ---------------------------------------------------------------------------------------------- gate 4: CleanRL
TASK = "Isaac-Velocity-CaT-Flat-H12_12dof-v0"
LOSS_KEYS = ("Loss/mean_pg_loss", "Loss/mean_entropy_loss", "Loss/mean_v_loss", "Loss/mean_surrogate_loss",
             "Loss/clipfrac", "Loss/learning_rate")


def count_calls(mp):
    calls = []
    orig = _learn.optim_step
    mp.setattr(_learn, "optim_step", lambda *a, **k: (calls.append(a[0]), orig(*a, **k))[1])
    return calls


def trainer_run(tmp, graph, fused_loss, fused_optimizer):
    """cleanrl.PPO on the CaT task at 64 envs x 24 steps, minibatches of 384; the agent, the logged lines and the rules
    the binding was called with."""
    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from biped_tasks.tasks.agents import H12_12dof_FlatCleanRlPPOCfg
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("H12_PPO_GRAPH", "1" if graph else "0")
        mp.delenv("H12_CLEANRL_HEAD_FUSED", raising=False)
        mp.delenv("H12_OPTIMIZER_FUSED", raising=False)
        calls = count_calls(mp)
        cfg = load_cfg_from_registry(TASK, "env_cfg_entry_point")
        cfg.scene.num_envs = 64
        cfg.sim.device = DEV
        cfg.seed = 3
        env = gym.make(TASK, cfg=cfg)
        ppo_cfg = H12_12dof_FlatCleanRlPPOCfg(num_steps=24, num_iterations=2, minibatch_size=384, updates_epochs=2,
                                              save_interval=2)
        torch.manual_seed(21)
        run = tmp / f"g{int(graph)}_l{int(fused_loss)}_o{int(fused_optimizer)}"
        agent = cleanrl.PPO(env, ppo_cfg, str(run), fused_loss=fused_loss, fused_optimizer=fused_optimizer)
        env.close()
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    return SimpleNamespace(agent=agent, lines=lines, calls=calls)


@pytest.fixture(scope="module")
def trainer_runs(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fused_optimizer")
    return SimpleNamespace(graphed=trainer_run(tmp, True, True, True), eager=trainer_run(tmp, False, True, True),
                           default=trainer_run(tmp, True, False, False))


def test_cleanrl_graphed_update_equals_eager_bit_for_bit(trainer_runs):
    g, e = trainer_runs.graphed, trainer_runs.eager
    for (k, p), q in zip(g.agent.state_dict().items(), e.agent.state_dict().values()):
        assert torch.isfinite(p).all() and torch.equal(p, q), (k, float((p - q).abs().max()))
    for x, y in zip(g.lines, e.lines):
        assert all(math.isfinite(x[k]) for k in LOSS_KEYS)
        assert {k: x[k] for k in LOSS_KEYS} == {k: y[k] for k in LOSS_KEYS}
    assert len(g.lines) == len(e.lines) == 2
    # graphed: two warm-up calls and the capture; eager: 2 iterations x 2 epochs x 4 minibatches
    assert g.calls == [_learn.OPTIM_RADAM] * 3 and e.calls == [_learn.OPTIM_RADAM] * 16
    assert g.lines[0]["Loss/learning_rate"] != g.lines[1]["Loss/learning_rate"]  # annealed through the device scalar


def test_cleanrl_default_run_never_calls_the_binding_and_agrees_to_rounding(trainer_runs):
    f, d = trainer_runs.graphed, trainer_runs.default
    assert d.calls == [] and len(d.lines) == 2
    assert list(f.agent.state_dict()) == list(d.agent.state_dict())
    x, y = f.lines[0], d.lines[0]
    for key in LOSS_KEYS:
        print(f"FIRST {key}: fused {x[key]!r} default {y[key]!r}")
    for key in LOSS_KEYS:
        assert abs(x[key] - y[key]) <= 1e-3 * max(1.0, abs(y[key])), (key, x[key], y[key])


# ---------------------------------------------------------------------------------------------- gate 4: ppo.PPO
def ppo_run(monkeypatch, graph, fused_optimizer, fused_loss=False, resume=None, updates=2):
    """ppo.PPO on the Flat task's shapes (270 observations, 12 actions) at 64 envs x 24 steps, adaptive schedule, seeded
    rollouts; ``resume``: (policy state_dict, optimizer state_dict) loaded before the first update."""
    from h12env.ppo import PPO, ActorCritic

    monkeypatch.setenv("H12_PPO_GRAPH", "1" if graph else "0")
    monkeypatch.delenv("H12_OPTIMIZER_FUSED", raising=False)
    torch.manual_seed(7)
    pol = ActorCritic(270, 270, 12, [128, 64], [128, 64])
    alg = PPO(pol, num_learning_epochs=2, num_mini_batches=4, learning_rate=1e-3, schedule="adaptive", desired_kl=0.01,
              device=DEV, fused_loss=fused_loss, fused_optimizer=fused_optimizer)
    if resume is not None:
        alg.policy.load_state_dict(resume[0])
        alg.load_optimizer_state_dict(resume[1])
        alg.lr_after_load = float(alg._lr_t)
    alg.init_storage(64, 24, [270], None, [12])  # 1536 rows, minibatches of 384
    out = []
    for u in range(updates):
        g = torch.Generator(device=DEV).manual_seed(100 + u)
        for k, v in alg.storage.t.items():
            v.copy_(torch.randn(v.shape, generator=g, device=DEV) * (0.1 if k == "sigma" else 1.0))
        alg.storage.t["sigma"].abs_().add_(0.5)
        out.append(alg.update())
    return alg, out


@pytest.mark.parametrize("fused_loss", [False, True], ids=["alone", "with_fused_loss"])
def test_ppo_graphed_update_equals_eager_bit_for_bit(gpu, monkeypatch, fused_loss):
    calls = count_calls(monkeypatch)
    a, la = ppo_run(monkeypatch, True, True, fused_loss)
    in_graph = len(calls)
    b, lb = ppo_run(monkeypatch, False, True, fused_loss)
    assert in_graph == 3 and len(calls) - in_graph == 2 * 8 and set(calls) == {_learn.OPTIM_ADAM}
    assert a._graph is not None and b._graph is None and a.fused_optimizer and b.fused_optimizer
    assert type(a.optimizer) is O.FusedClipAdam and a.optimizer.max_norm == a.max_grad_norm
    assert a.optimizer.param_groups[0]["lr"] is a._lr_t
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.isfinite(p).all() and torch.equal(p, q), (p - q).abs().max()
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a.optimizer.state[p][k], b.optimizer.state[q][k])
        assert float(a.optimizer.state[p]["step"]) == 16.0
    assert la == lb and a.learning_rate == b.learning_rate and a.learning_rate != 1e-3  # the schedule moved it
    assert all(math.isfinite(v) for x in la for v in x.values())
    if not fused_loss:  # the default run never calls the binding, and the two agree to rounding
        n = len(calls)
        d, ld = ppo_run(monkeypatch, True, False)
        assert len(calls) == n and not d.fused_optimizer and type(d.optimizer) is torch.optim.Adam
        for x, y in zip(la, ld):
            for key in x:
                print(f"PPO {key}: fused {x[key]!r} default {y[key]!r}")
                assert abs(x[key] - y[key]) <= 1e-3 * max(1.0, abs(y[key])), (key, x, y)


@pytest.mark.parametrize("first", [True, False], ids=["fused_into_default", "default_into_fused"])
def test_ppo_checkpoints_resume_on_the_other_path(gpu, monkeypatch, first):
    a, _ = ppo_run(monkeypatch, True, first, updates=1)
    ck = ({k: v.clone() for k, v in a.policy.state_dict().items()}, a.optimizer_state_dict())
    assert isinstance(ck[1]["param_groups"][0]["lr"], float) and len(ck[1]["state"]) == len(list(a.policy.parameters()))
    b, lb = ppo_run(monkeypatch, True, not first, resume=ck, updates=1)
    assert b.fused_optimizer is (not first) and b.lr_after_load == a.learning_rate != 1e-3  # the schedule's, carried on
    assert b.optimizer.param_groups[0]["lr"] is b._lr_t
    for (k, p), q in zip(b.policy.state_dict().items(), ck[0].values()):
        assert torch.isfinite(p).all(), k
    assert not torch.equal(next(b.policy.parameters()), next(iter(ck[0].values())))
    for p in b.policy.parameters():  # the state went on from the checkpoint's: 8 steps there, 8 here
        st = b.optimizer.state[p]
        assert float(st["step"]) == 16.0 and st["step"].is_cuda and st["step"].dtype == torch.float32
        assert st["exp_avg_sq"].any()
    assert all(math.isfinite(v) for x in lb for v in x.values())
