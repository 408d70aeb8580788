"""GPU: what tests/test_gpu_recurrent.py never launches of the fused LSTM step (h12learn_lstm_pack / h12learn_lstm_step,
h12env.policy.FusedLSTMStep / RecurrentPolicy): the in-kernel observation normaliser, the shape edges of the cell and
saturated gates.  DESIGN.md section 7q.  The reference, its bound and the planted normalisers are those of
tests/helpers/lstm_ref.py, which tests/test_lstm_reference.py checks without a GPU (torch fp32 within half the bound;
a wrong eps placement, kind, column or gate order more than 10 times outside it).

a  normaliser {var: cleanrl.RunningMeanStd, std: ppo.EmpiricalNormalization} with three planted zero-variance columns
   (the first, the last, one inside; x within 1e-4 / 1e-2 of the mean there) and once per kind without them: every
   element of y, h', c' within the fp64 bound, and within twice the bound of the torch fp32 path (the module in eval
   mode, then torch.nn.LSTM + the MLP on the CPU).
b  shape edges without a normaliser: H below one tile and odd (1, 7), d_in an exact multiple of 16 (16, 32, 448: no
   zero column between x and h in the LDS image), and the widest shape the host check admits (1024, 256, [1024]: both
   LDS buffers at their limit).  Same assertions.
c  bitwise, with a normaliser: run to run, row subset, two networks == two calls, reset mask == zeroed state, live
   statistics (changed in place: seen by the next call), rebinding (EmpiricalNormalization.update rebinds _std).
d  eight free-running steps with planted dones inside the chained bound, over {none, var, std}.
e  saturation: gate pre-activations from -1e4 to 1e4 planted through bias_ih (every gate of every unit sees every
   value), c_in up to -1e30, the MLP's first pre-activations from -1e3 to 1e3: all finite and inside the bound; then
   through data: a zero-variance column and an outlier row (|z| > 1e3), which stays in its row.
f  RecurrentPolicy(fused=True) with a normaliser against fused=False, and deploy_policy(fused=True) on an export with
   a trained EmpiricalNormalization against the fp64 chain and nine CPU copies of the TorchScript module.
g  the runner with empirical_normalization=True on the real env: trains, get_inference_policy(fused=True) against the
   default one, save / load.
All comparisons are elementwise ``|got - ref| <= bound`` (lstm_ref.inside): a bound that is exactly 0 demands exact.
Measured on the MI355X, worst fraction of the bound, kernel / torch fp32: a 9.1e-3 / 8.1e-3 (1.2e-2 / 1.0e-2 without
planted columns), b 0.198 / 0.224 (the 1 -> 1 -> 1 network; 1.1e-3 at the widest shape), d 1.3e-2, e 1.6e-3 / 1.8e-3,
f 2.8e-2, g 1.5e-3; no non-finite value anywhere.  A library built with norm_mean[c + 1], and one with
sqrtf(var) + eps, fail a, c, d and f.
"""
import copy
import sys
from pathlib import Path

import pytest
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT / "h1v2-isaac_amd" / "shims"), str(ROOT / "tests" / "helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lstm_ref as R  # noqa: E402
from h12env.policy import FusedLSTMStep, RecurrentPolicy, deploy_policy  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (1, 17, 33)
REAL = [512, 256, 128]
NORM_SHAPES = [(1, 1, [], 1), (16, 7, [5], 3), (45, 64, [40, 24], 12), (448, 256, REAL, 12)]
EDGE_SHAPES = [(1, 1, [], 1), (16, 7, [5], 3), (32, 16, [16], 12), (448, 256, REAL, 12), (1024, 256, [1024], 12)]
MID = (45, 64, [40, 24], 12)
TASK = "Isaac-Velocity-Flat-H12_12dof-v0"


def check_step(tag, pairs, norm, x, before, ys, after):
    """The assertions of a and b on one call: ``ys`` and ``after`` are the kernel's outputs from ``before``.  Returns
    the worst fractions (kernel of the bound, torch of the bound)."""
    worst = worst_t = 0.0
    for k, (rnn, net) in enumerate(pairs):
        ref, bound = R.lstm_fp64_with_bound(rnn, net, x, *before[k], norm=norm)
        cpu = R.torch_cpu(rnn, net, x, *before[k], norm=norm)
        for name, got, r64, e, rt in zip("yhc", (ys[k], *after[k]), ref, bound, cpu):
            ok, fa = R.inside(got, r64, e)
            ok_t, fb = R.inside(got, rt, e, factor=2.0)
            _, ft = R.inside(rt, r64, e)
            print(f"{tag} net {k} {name}: kernel {fa:.3e} of the bound, kernel - torch {fb:.3e} of twice the bound, "
                  f"torch {ft:.3e}")
            assert ok, (tag, k, name, fa)
            assert ok_t, (tag, k, name, fb)
            worst, worst_t = max(worst, fa), max(worst_t, ft)
    return worst, worst_t


def run_shapes(what, shape, n_nets, kind, planted, seed):
    pairs = R.make_pairs(shape, n_nets, seed)
    norm = R.make_planted_norm(kind, shape[0], 100 + seed, planted=planted)
    f = FusedLSTMStep(pairs, norm)
    worst = worst_t = 0.0
    for n in NS:
        _, states = R.make_inputs(shape, n, n_nets, seed=1000 * seed + n)
        x = R.make_norm_x(n, shape[0], norm, seed=2000 * seed + n, planted=planted)
        before = R.clone_states(states)
        ys = f(x, states)  # eager: the first call of a shape over 64 KiB of LDS is outside any capture
        w, wt = check_step(f"shape {shape} nets {n_nets} kind {kind} planted {planted} n {n}", pairs, norm, x, before,
                           ys, states)
        worst, worst_t = max(worst, w), max(worst_t, wt)
    print(f"WORST {what} shape {shape} nets {n_nets} kind {kind} planted {planted}: kernel {worst:.3e} torch {worst_t:.3e}")


# ---------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("n_nets", [1, 2])
@pytest.mark.parametrize("case", range(len(NORM_SHAPES)))
@pytest.mark.parametrize("kind", ["var", "std"])
def test_normaliser_against_fp64_bound_and_torch(gpu, kind, case, n_nets):
    run_shapes("a", NORM_SHAPES[case], n_nets, kind, True, seed=case)


@pytest.mark.parametrize("kind", ["var", "std"])
def test_normaliser_without_planted_columns(gpu, kind):
    run_shapes("a-tight", MID, 2, kind, False, seed=5)


# ---------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("case", range(len(EDGE_SHAPES)))
def test_shape_edges_without_a_normaliser(gpu, case):
    run_shapes("b", EDGE_SHAPES[case], 2, "none", False, seed=10 + case)


# ---------------------------------------------------------------------------------------------- c
def same(states_a, states_b):
    return all(torch.equal(a, b) for pa, pb in zip(states_a, states_b) for a, b in zip(pa, pb))


def same_y(ya, yb):
    return all(torch.equal(a, b) for a, b in zip(ya, yb))


@pytest.fixture()
def bitwise(gpu):
    pairs = R.make_pairs(MID, 2, seed=41)
    norm = R.make_planted_norm("std", MID[0], 141)
    _, states = R.make_inputs(MID, 33, 2, seed=61)
    x = R.make_norm_x(33, MID[0], norm, seed=62)
    f = FusedLSTMStep(pairs, norm)
    new = R.clone_states(states)
    ys = f(x, new)
    return pairs, norm, f, x, states, ys, new


def test_bitwise_with_a_normaliser_run_to_run_rows_networks_and_reset(bitwise):
    pairs, norm, f, x, states, ys, new = bitwise
    again = R.clone_states(states)
    assert same_y(f(x, again), ys) and same(again, new)
    part = [(h[5:20].clone(), c[5:20].clone()) for h, c in states]
    yp = f(x[5:20].contiguous(), part)
    assert all(torch.equal(a, b[5:20]) for a, b in zip(yp, ys))
    assert all(torch.equal(a, b[5:20]) for pa, pb in zip(part, new) for a, b in zip(pa, pb))
    for k, pair in enumerate(pairs):
        st = R.clone_states(states[k:k + 1])
        (y,) = FusedLSTMStep([pair], norm)(x, st)
        assert torch.equal(y, ys[k]) and same(st, new[k:k + 1]), k
    mask = torch.zeros(33, dtype=torch.uint8, device="cuda")
    mask[[0, 7, 16, 32]] = 1
    masked, zeroed = R.clone_states(states), R.clone_states(states)
    ym = f(x, masked, reset=mask)
    for h, c in zeroed:
        h[mask.bool()] = 0
        c[mask.bool()] = 0
    yz = f(x, zeroed)
    assert same_y(ym, yz) and same(masked, zeroed)
    assert not torch.equal(ym[0][7], ys[0][7]) and torch.equal(ym[0][8], ys[0][8])
    # the normaliser is in it: without one the outputs differ
    assert not same_y(FusedLSTMStep(pairs)(x, R.clone_states(states)), ys)


@pytest.mark.parametrize("kind", ["std", "var"])
def test_bitwise_live_statistics_are_seen_without_a_repack(gpu, kind):
    pairs = R.make_pairs(MID, 2, seed=42)
    norm = R.make_planted_norm(kind, MID[0], 142)
    _, states = R.make_inputs(MID, 33, 2, seed=63)
    x = R.make_norm_x(33, MID[0], norm, seed=64)
    f = FusedLSTMStep(pairs, norm)
    y0 = f(x, R.clone_states(states))
    packed = f._packed.clone()
    mean, scale = (norm.running_mean, norm.running_var) if kind == "var" else (norm._mean, norm._std)
    ptrs = (mean.data_ptr(), scale.data_ptr())
    for stat in (mean, scale):
        if stat is mean:
            stat.add_(0.25)
        else:
            stat.mul_(1.5).add_(0.125)  # the planted columns too
        assert (mean.data_ptr(), scale.data_ptr()) == ptrs
        desc = f._desc
        st = R.clone_states(states)
        y1 = f(x, st)
        assert f._desc is desc and torch.equal(f._packed, packed)  # neither re-described nor re-packed
        assert not same_y(y1, y0)
        fresh = R.clone_states(states)
        assert same_y(FusedLSTMStep(pairs, norm)(x, fresh), y1) and same(fresh, st)
        check_step(f"live {kind}", pairs, norm, x, states, y1, st)
        y0 = y1


def test_bitwise_after_the_normaliser_rebinds_its_std(bitwise):
    pairs, norm, f, x, states, ys, new = bitwise
    old = norm._std
    norm.train()
    g = torch.Generator().manual_seed(65)
    norm((torch.randn(64, MID[0], generator=g) * 3 + 1).cuda())  # EmpiricalNormalization.update: _std = sqrt(_var)
    norm.eval()
    assert norm._std is not old and not torch.equal(norm._std, old)
    st = R.clone_states(states)
    y1 = f(x, st)
    assert not same_y(y1, ys)
    fresh = R.clone_states(states)
    assert same_y(FusedLSTMStep(pairs, norm)(x, fresh), y1) and same(fresh, st)
    check_step("rebound", pairs, norm, x, states, y1, st)
    old.fill_(float("nan"))  # the tensor that was rebound away is not read any more
    again = R.clone_states(states)
    assert same_y(f(x, again), y1) and same(again, st)


# ---------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("kind", ["none", "var", "std"])
def test_eight_free_running_steps_with_a_normaliser_stay_inside_the_chained_bound(gpu, kind):
    shape, n, steps = MID, 17, 8
    (rnn, net), = R.make_pairs(shape, 1, seed=7)
    norm = R.make_planted_norm(kind, shape[0], 107)
    f = FusedLSTMStep([(rnn, net)], norm)
    dones = torch.zeros(steps, n, dtype=torch.bool)
    dones[2, [0, 16]] = True
    dones[5, [3, 16]] = True
    state = [(torch.zeros(n, shape[1], device="cuda"), torch.zeros(n, shape[1], device="cuda"))]
    h64 = c64 = eh = ec = torch.zeros(n, shape[1], dtype=torch.float64, device="cuda")
    reset = None
    worst = 0.0
    for t in range(steps):
        x = R.make_norm_x(n, shape[0], norm, seed=800 + t)
        (y,) = f(x, state, reset=reset)  # the rows that were done at t - 1 read zeros
        (y64, h64, c64), (ey, eh, ec) = R.lstm_fp64_with_bound(rnn, net, x, h64, c64, eh, ec, norm=norm)
        for name, got, ref, e in (("y", y, y64, ey), ("h", state[0][0], h64, eh), ("c", state[0][1], c64, ec)):
            ok, fr = R.inside(got, ref, e)
            print(f"kind {kind} step {t} {name}: {fr:.3e} of the chained bound (largest bound {float(e.max()):.3e})")
            assert ok, (t, name, fr)
            worst = max(worst, fr)
        d = dones[t].cuda()
        reset = d.to(torch.uint8)
        h64, c64, eh, ec = (torch.where(d[:, None], torch.zeros_like(v), v) for v in (h64, c64, eh, ec))
    print(f"WORST d kind {kind}: kernel {worst:.3e}")


# ---------------------------------------------------------------------------------------------- e
SAT = (3, 16, [16, 16], 4)
SAT_VALUES = (-1e4, -200.0, -104.0, -103.0, -89.0, -88.0, -87.0, -30.0, 0.0, 30.0, 87.0, 88.0, 89.0, 103.0, 200.0, 1e4)
SAT_C = (0.0, 1.0, -50.0, 1e4, -1e30)


def test_saturated_gates_cell_and_elu_stay_finite_and_inside_the_bound(gpu):
    (rnn, net), = R.make_pairs(SAT, 1, seed=51)
    H = SAT[1]
    values = torch.tensor(SAT_VALUES, device="cuda")
    for p in rnn.parameters():
        p.zero_()
    net[0].bias.copy_(values / 10)
    f = FusedLSTMStep([(rnn, net)])
    n = len(SAT_C)
    x, [(h, _)] = R.make_inputs(SAT, n, 1, seed=52)
    c = torch.tensor(SAT_C, device="cuda")[:, None].expand(n, H).contiguous()
    seen = torch.zeros(4 * H, len(SAT_VALUES), dtype=torch.bool)
    worst = worst_t = 0.0
    for s in range(len(SAT_VALUES)):
        idx = (torch.arange(H)[None, :] + s + 5 * torch.arange(4)[:, None]) % len(SAT_VALUES)  # [gate][unit]
        rnn.bias_ih_l0.copy_(values[idx.reshape(-1).cuda()])
        seen[torch.arange(4 * H), idx.reshape(-1)] = True
        st = [(h.clone(), c.clone())]
        ys = f(x, st, repack=True)
        for got in (ys[0], *st[0]):
            assert torch.isfinite(got).all(), s
        w, wt = check_step(f"saturation setting {s}", [(rnn, net)], None, x, [(h, c)], ys, st)
        worst, worst_t = max(worst, w), max(worst_t, wt)
    assert seen.all()  # every gate of every unit saw every value
    print(f"WORST e planted: kernel {worst:.3e} torch {worst_t:.3e}")


def test_an_outlier_through_a_zero_variance_column_stays_finite_and_in_its_row(gpu):
    (rnn, net), = R.make_pairs(SAT, 1, seed=53)
    norm = R.make_norm("var", SAT[0], 153)
    norm.running_var[1] = 0.0  # a constant observation column: its scale is sqrt(eps) = 1e-4
    f = FusedLSTMStep([(rnn, net)], norm)
    n, row = 17, 6
    _, states = R.make_inputs(SAT, n, 1, seed=54)
    g = torch.Generator().manual_seed(55)
    mean = norm.running_mean.cpu()
    x = torch.randn(n, SAT[0], generator=g) * 2 + mean
    x[:, 1] = mean[1] + 1e-4 * (2 * torch.rand(n, generator=g) - 1)
    calm = x.clone().cuda()
    x[row, 1] = mean[1] + 1.0  # normalised: 1e4
    wild = x.cuda()
    z = ((wild[row].double() - norm.running_mean.double()) / torch.sqrt(norm.running_var.double() + norm.epsilon)
         ) @ rnn.weight_ih_l0.double().T
    print(f"largest |x_n W_ih^T| of the outlier row: {float(z.abs().max()):.1f}")
    assert float(z.abs().max()) > 1e3
    st_calm, st_wild = R.clone_states(states), R.clone_states(states)
    y_calm, y_wild = f(calm, st_calm), f(wild, st_wild)
    for got in (y_wild[0], *st_wild[0]):
        assert torch.isfinite(got).all()
    w, wt = check_step("outlier", [(rnn, net)], norm, wild, states, y_wild, st_wild)
    print(f"WORST e outlier: kernel {w:.3e} torch {wt:.3e}")
    keep = torch.arange(n, device="cuda") != row
    for a, b in zip((y_wild[0], *st_wild[0]), (y_calm[0], *st_calm[0])):
        assert torch.equal(a[keep], b[keep]) and not torch.equal(a[row], b[row])


# ---------------------------------------------------------------------------------------------- f
@pytest.mark.parametrize("kind", ["var", "std"])
def test_recurrent_policy_fused_with_a_normaliser_against_the_torch_modules(gpu, kind):
    shape, n = MID, 9
    (rnn, net), = R.make_pairs(shape, 1, seed=21)
    norm = R.make_planted_norm(kind, shape[0], 121)
    stats = {k: v.clone() for k, v in norm.state_dict().items()}
    fused, plain = RecurrentPolicy(rnn, net, norm, fused=True), RecurrentPolicy(rnn, net, norm)
    worst = 0.0
    for t in range(6):
        x = R.make_norm_x(n, shape[0], norm, seed=900 + t)
        if t == 2:
            d = torch.tensor([0, 1, 0, 0, 0, 0, 0, 0, 1], device="cuda")
            fused.reset(d), plain.reset(d)
        fused._ensure_state(n, x.device), plain._ensure_state(n, x.device)
        for dst, src in zip(plain.state, fused.state):  # both from the same fp32 state: one step apart
            dst.copy_(src)
        h0, c0 = fused.state[0][0].clone(), fused.state[1][0].clone()
        if t == 2:
            assert (h0[[1, 8]] == 0).all() and (c0[[1, 8]] == 0).all() and (h0[2] != 0).any()
        a, b = fused(x), plain(x)
        _, (e, eh, ec) = R.lstm_fp64_with_bound(rnn, net, x, h0, c0, norm=norm)
        for name, got, want, bound in (("y", a, b, e), ("h", fused.state[0][0], plain.state[0][0], eh),
                                       ("c", fused.state[1][0], plain.state[1][0], ec)):
            ok, fr = R.inside(got, want, bound, factor=2.0)
            print(f"kind {kind} step {t} {name}: fused - torch {fr:.3e} of twice the bound")
            assert ok and got.shape == want.shape, (t, name, fr)
            worst = max(worst, fr)
    assert a.shape == (n, shape[3])
    for k, v in norm.state_dict().items():  # inference reads the statistics, neither path updates them
        assert torch.equal(v, stats[k]), k
    print(f"WORST f policy kind {kind}: kernel - torch {worst:.3e} of twice the bound")


def test_deploy_policy_fused_on_an_export_with_a_trained_normaliser(gpu, tmp_path):
    from h12env.export import export_policy_as_jit
    from h12env.ppo import ActorCriticRecurrent, EmpiricalNormalization

    torch.manual_seed(4)
    policy = ActorCriticRecurrent(10, 10, 4, actor_hidden_dims=(24, 16), critic_hidden_dims=(8,), rnn_hidden_dim=14)
    norm = EmpiricalNormalization([10]).train()
    norm(torch.randn(64, 10) * 3 + 1)
    norm.eval()
    path = export_policy_as_jit(policy, norm, str(tmp_path))
    m = torch.jit.load(path)
    n, H = 9, 14
    p = deploy_policy(m, n, "cuda", fused=True)
    assert isinstance(p, RecurrentPolicy) and p._step is not None and p.normalizer is not None
    assert torch.equal(p.normalizer._std.cpu(), norm._std) and p.normalizer.eps == norm.eps
    copies = [torch.jit.load(path) for _ in range(n)]
    h64 = c64 = eh = ec = torch.zeros(n, H, dtype=torch.float64, device="cuda")
    g = torch.Generator().manual_seed(5)
    worst = worst_c = 0.0
    with torch.no_grad():
        for t in range(6):
            x = (torch.randn(n, 10, generator=g) * 3 + 1).cuda()
            if t == 2:  # robots 1 and 8 start a new episode
                d = torch.tensor([0, 1, 0, 0, 0, 0, 0, 0, 1], device="cuda")
                p.reset(d)
                for i in (1, 8):
                    copies[i] = torch.jit.load(path)
                h64, c64, eh, ec = (torch.where(d.bool()[:, None], torch.zeros_like(v), v) for v in (h64, c64, eh, ec))
            h0, c0 = p.state[0][0].clone(), p.state[1][0].clone()
            y = p(x)
            # the free-running chain in fp64
            (y64, h64, c64), (ey, eh, ec) = R.lstm_fp64_with_bound(p.rnn, p.mlp, x, h64, c64, eh, ec, norm=p.normalizer)
            for name, got, ref, e in (("y", y, y64, ey), ("h", p.state[0][0], h64, eh), ("c", p.state[1][0], c64, ec)):
                ok, fr = R.inside(got, ref, e)
                print(f"step {t} {name}: {fr:.3e} of the chained bound")
                assert ok, (t, name, fr)
                worst = max(worst, fr)
            # one step from the same fp32 state: the nine copies of the export, one robot each
            _, (e1, eh1, ec1) = R.lstm_fp64_with_bound(p.rnn, p.mlp, x, h0, c0, norm=p.normalizer)
            rows, hs, cs = [], [], []
            for i, cp in enumerate(copies):
                if t == 2 and i in (1, 8):
                    assert (cp.hidden_state == 0).all() and (h0[i] == 0).all()  # the fresh copy and the reset row
                cp.hidden_state.copy_(h0[i].cpu()[None, None]), cp.cell_state.copy_(c0[i].cpu()[None, None])
                rows.append(cp(x[i:i + 1].cpu()))
                hs.append(cp.hidden_state[0]), cs.append(cp.cell_state[0])
            for name, got, want, e in (("y", y, torch.cat(rows), e1), ("h", p.state[0][0], torch.cat(hs), eh1),
                                       ("c", p.state[1][0], torch.cat(cs), ec1)):
                ok, fr = R.inside(got, want, e, factor=2.0)
                print(f"step {t} {name}: fused - export {fr:.3e} of twice the one-step bound")
                assert ok, (t, name, fr)
                worst_c = max(worst_c, fr)
    print(f"WORST f export: kernel {worst:.3e} of the chained bound, kernel - export {worst_c:.3e} of twice the bound")


# ---------------------------------------------------------------------------------------------- g
def test_runner_with_empirical_normalization_trains_and_deploys_fused(gpu, monkeypatch, tmp_path):
    from test_gpu_recurrent import _recurrent_runner

    monkeypatch.delenv("H12_POLICY_FUSED", raising=False)
    agent, env, runner = _recurrent_runner(TASK, n=16, num_steps_per_env=8, empirical_normalization=True)
    assert runner.empirical_normalization and int(runner.obs_normalizer.count) == 0
    runner.learn(2)
    stats = runner.last_iteration_stats
    for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"):
        assert torch.isfinite(torch.tensor(stats[k])), (k, stats[k])
    print(f"normaliser count after learn(2): {int(runner.obs_normalizer.count)}")
    assert int(runner.obs_normalizer.count) > 0 and int(runner.critic_obs_normalizer.count) > 0
    assert not (runner.obs_normalizer._std == 1).all()

    pol = runner.alg.policy
    fused = runner.get_inference_policy(fused=True)
    default = runner.get_inference_policy()
    assert isinstance(fused, RecurrentPolicy) and fused.normalizer is runner.obs_normalizer
    assert not runner.obs_normalizer.training
    rnn, actor, norm = pol.memory_a.rnn, pol.actor, runner.obs_normalizer
    obs, _ = env.get_observations()
    firsts = []
    worst = 0.0
    with torch.inference_mode():
        for t in range(4):
            obs = obs.clone()
            fused._ensure_state(16, obs.device)
            h0, c0 = fused.state[0].clone(), fused.state[1].clone()
            pol.memory_a.hidden_states = (h0.clone(), c0.clone())  # both from the same state
            a, b = fused(obs), default(obs)
            firsts.append((obs, a.clone()))
            _, (e, eh, ec) = R.lstm_fp64_with_bound(rnn, actor, obs, h0[0], c0[0], norm=norm)
            hd, cd = pol.memory_a.hidden_states
            for name, got, want, bound in (("y", a, b, e), ("h", fused.state[0][0], hd[0], eh),
                                           ("c", fused.state[1][0], cd[0], ec)):
                ok, fr = R.inside(got, want, bound, factor=2.0)
                print(f"step {t} {name}: fused - default {fr:.3e} of twice the bound")
                assert ok, (t, name, fr)
                worst = max(worst, fr)
            obs, _, dones, _ = env.step(a)
            fused.reset(dones)
    print(f"WORST g: kernel - torch {worst:.3e} of twice the bound")
    path = str(tmp_path / "model.pt")
    runner.save(path)
    env.close()
    _, env2, fresh = _recurrent_runner(TASK, n=16, num_steps_per_env=8, empirical_normalization=True)
    assert int(fresh.obs_normalizer.count) == 0
    fresh.load(path)
    assert torch.equal(fresh.obs_normalizer._std, runner.obs_normalizer._std)
    with torch.inference_mode():
        again = fresh.get_inference_policy(fused=True)(firsts[0][0])
    env2.close()
    assert torch.equal(again, firsts[0][1])
