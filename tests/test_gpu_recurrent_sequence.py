"""MI355X: the LSTM sequence kernels of the recurrent update (csrc/h12_policy_rnn_train.hip: h12learn_lstm_seq_pack /
_forward / _backward), their autograd node (h12env.recurrent.lstm_sequence) and PPO(fused_rnn_update=True).
DESIGN.md section 7r.  Every reference is torch.nn.LSTM / fp64 on the CPU (tests/helpers/lstm_seq_ref.py).

1  forward inside the a-priori bound of lstm_ref.lstm_fp64_with_bound chained over T; the CPU fp32 nn.LSTM inside it too.
2  backward: per case the largest normalised error max|g - g64| / max|g64| over dz, dW_ih, dW_hh, both biases, dh0, dc0
   is at most FACTOR times the yardstick, the same quantity of the CPU fp32 library LSTM over the padded trajectories.
3  exact properties: a reset cuts the gradient, dones[T - 1] is not read, rows do not depend on their tile or on n, run
   to run, guard regions, two networks == two calls.
4  pack + forward + backward captured as one graph.
5  lstm_sequence on the device against the torch loop on the device, gradients by 2's rule.
6  the runner with the switch on; train.py --recurrent --fused_rnn_update as a child process.
"""
import functools
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[1]
SHIMS = ROOT / "h1v2-isaac_amd" / "shims"
for p in (str(SHIMS), str(ROOT / "tests" / "helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

from h12env import _learn  # noqa: E402
from h12env import recurrent as R  # noqa: E402
from lstm_ref import U, inside  # noqa: E402
from lstm_seq_ref import (GRADS, library_padded_grads, make_case, make_dones, resets, seq_fp64_with_bound,  # noqa: E402
                          seq_grads, worst_error)

pytestmark = pytest.mark.gpu

# (T, N, d_in, H): N in {1, 17, 33} (a partial tile, two tiles, three with a partial one), H in {1, 16, 20, 256} (below a
# tile, one tile, no multiple of 16, the widest: over 64 KiB of LDS), T in {1, 2, 8}, d_in in {1, 45}
CASES = [(1, 1, 1, 1), (2, 17, 1, 16), (8, 33, 45, 20), (8, 1, 45, 16), (2, 17, 45, 256), (1, 33, 1, 20), (8, 17, 1, 1)]
DONES = ("none", "all", "planted")
# The kernel's allowed factor over the yardstick: the smallest power of two at least twice the worst ratio measured on
# the MI355X over every case below, capped at 64.  Measured: ratios from 0.50 to 2.06 (the largest at (2, 17, 45, 256),
# dones "all": kernel 1.05e-6 against 5.1e-7), so 8.  A yardstick below U = 2^-24 is raised to U: a
# correctly rounded fp32 tensor is that far from its fp64 value relative to its largest element.
FACTOR = 8
TASK = "Isaac-Velocity-Flat-H12_12dof-v0"
SENTINEL = -7.5e8
GUARD = 64


@functools.lru_cache(maxsize=None)
def reference(case, kind, k=0):
    """Everything the CPU knows about network k of a case: inputs, the fp64 forward with its bound, the fp64 gradients
    and the library's.  Computed once, shared by the tests, never modified."""
    T, N, d_in, H = case
    rnn, x, h0, c0, dh = make_case(T, N, d_in, H, seed=1000 * CASES.index(case) + 7 * k + 1)
    dones = make_dones(kind, T, N)
    return {"rnn": rnn, "x": x, "h0": h0, "c0": c0, "dh": dh, "dones": dones,
            "fwd": seq_fp64_with_bound(rnn, x, dones, h0, c0), "g64": seq_grads(rnn, x, dones, h0, c0, dh),
            "lib": library_padded_grads(rnn, x, dones, h0, c0, dh)}


def guarded(shape, dev="cuda"):
    """A tensor of ``shape`` with GUARD sentinel floats behind it, all of it filled with the sentinel."""
    n = int(torch.tensor(shape).prod())
    flat = torch.full((n + GUARD,), SENTINEL, device=dev)
    return flat[:n].view(*shape), flat


def run_kernels(refs, dones, rows=None, guard=False):
    """pack, the projection GEMM, forward, backward and the weight-gradient GEMMs for the networks ``refs`` (one or two
    of reference()) on the device; ``rows``: a slice of envs to run alone.  Returns per network a dict of device tensors
    (h, c, gates and every name of GRADS), and the guard buffers."""
    dev = "cuda"
    rows = slice(None) if rows is None else rows
    d8 = (dones[:, rows] != 0).to(torch.uint8).to(dev).contiguous()
    T, N = d8.shape
    H = refs[0]["rnn"].hidden_size
    par = [{n: p.detach().to(dev) for n, p in r["rnn"].named_parameters()} for r in refs]
    desc = _learn.lstm_seq_desc([p["weight_hh_l0"] for p in par])
    packed = torch.empty(_learn.lstm_seq_packed_bytes(desc) // 4, device=dev)
    _learn.lstm_seq_pack(desc, packed)
    xs = [r["x"][:, rows].to(dev).reshape(T * N, -1) for r in refs]
    zxs = [torch.addmm(p["bias_ih_l0"] + p["bias_hh_l0"], x, p["weight_ih_l0"].t()).view(T, N, 4 * H)
           for p, x in zip(par, xs)]
    h0s = [r["h0"][rows].to(dev).contiguous() for r in refs]
    c0s = [r["c0"][rows].to(dev).contiguous() for r in refs]
    dhs = [r["dh"][:, rows].to(dev).contiguous() for r in refs]
    flats, fwd_out, bwd_out = [], None, None
    if guard:
        fwd_out, bwd_out = [], []
        for _ in refs:
            f = [guarded(s) for s in ((T, N, H), (T, N, H), (T, N, 4 * H))]
            b = [guarded(s) for s in ((T, N, 4 * H), (N, H), (N, H))]
            fwd_out.append(tuple(v for v, _ in f)), bwd_out.append(tuple(v for v, _ in b))
            flats += [fl for _, fl in f + b]
    fwd = _learn.lstm_seq_forward(desc, packed, zxs, d8, h0s, c0s, out=fwd_out)
    bwd = _learn.lstm_seq_backward(desc, packed, dhs, [(o[1], o[2]) for o in fwd], d8, c0s, out=bwd_out)
    keep = (~resets(d8)).float().unsqueeze(-1)
    res = []
    for x, h0, (h, c, gates), (dz, dh0, dc0) in zip(xs, h0s, fwd, bwd):
        dz2 = dz.view(T * N, 4 * H)
        h_prev = (torch.cat([h0[None], h[:-1]]) * keep).view(T * N, H)
        db = dz2.sum(0)
        res.append({"h": h, "c": c, "gates": gates, "dz": dz, "dW_ih": dz2.t() @ x, "dW_hh": dz2.t() @ h_prev,
                    "db_ih": db, "db_hh": db, "dh0": dh0, "dc0": dc0})
    torch.cuda.synchronize()
    return res, flats


def same_bits(a, b, names=("h", "c", "gates", "dz", "dh0", "dc0")):
    return all(torch.equal(a[k], b[k]) for k in names)


def cpu_fp32_steps(ref):
    """(h_seq, c_seq) of the CPU fp32 nn.LSTM stepped over t with the reset rule."""
    rnn, rs = ref["rnn"], resets(ref["dones"])
    state = (ref["h0"][None], ref["c0"][None])
    hs, cs = [], []
    with torch.no_grad():
        for t in range(ref["x"].shape[0]):
            keep = (~rs[t]).float()[None, :, None]
            _, state = rnn(ref["x"][t:t + 1], tuple(s * keep for s in state))
            hs.append(state[0][0]), cs.append(state[1][0])
    return torch.stack(hs), torch.stack(cs)


def yardstick(ref):
    return max(worst_error(ref["lib"], ref["g64"])[0], U)


# ---------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("n_nets", [1, 2])
@pytest.mark.parametrize("kind", DONES)
@pytest.mark.parametrize("case", CASES)
def test_forward_inside_the_bound_and_backward_against_fp64(gpu, case, kind, n_nets):
    refs = [reference(case, kind, k) for k in range(n_nets)]
    out, _ = run_kernels(refs, refs[0]["dones"])
    for k, (ref, got) in enumerate(zip(refs, out)):
        h32, c32 = cpu_fp32_steps(ref)
        for name, lib in (("h", h32), ("c", c32), ("gates", None)):
            r64, e = ref["fwd"][name]
            ok, worst = inside(got[name], r64, e)
            ok_t, worst_t = (True, 0.0) if lib is None else inside(lib, r64, e)
            print(f"FWD case {case} dones {kind} nets {n_nets} net {k} {name}: kernel {worst:.4f} of the bound, "
                  f"cpu nn.LSTM {worst_t:.4f}")
            assert ok and ok_t, (case, kind, k, name, worst, worst_t)
        err, per = worst_error(got, ref["g64"])
        yard = yardstick(ref)
        print(f"BWD case {case} dones {kind} nets {n_nets} net {k}: kernel {err:.3e}, yardstick {yard:.3e}, "
              f"ratio {err / yard:.3f}  " + " ".join(f"{n} {v:.2e}" for n, v in per.items()))
        assert err <= FACTOR * yard, (case, kind, k, per, yard)


# ---------------------------------------------------------------------------------------------- 3
BIG = (8, 33, 45, 20)


def test_a_reset_cuts_the_gradient(gpu):
    ref = dict(reference(BIG, "planted"))
    T, N = ref["dones"].shape
    t_d, row = T - 1, 1  # planted_dones puts the done at T - 1 on env 1; move it one step earlier so that it is read
    dones = ref["dones"].clone()
    dones[t_d - 1, row] = 1
    dh = ref["dh"].clone()
    dh[:t_d] = 0
    ref["dh"] = dh
    got = run_kernels([ref], dones)[0][0]
    assert (got["dz"][:t_d, row] == 0).all() and (got["dh0"][row] == 0).all() and (got["dc0"][row] == 0).all()
    assert (got["dz"][t_d, row] != 0).any()
    other = 4  # an env without a done: its gradient flows back to t = 0
    assert not dones[:, other].any() and (got["dz"][0, other] != 0).any() and (got["dh0"][other] != 0).any()


def test_last_dones_unread_run_to_run_row_subset_and_two_networks(gpu):
    refs = [reference(BIG, "planted", k) for k in range(2)]
    dones = refs[0]["dones"]
    two, _ = run_kernels(refs, dones)
    again, _ = run_kernels(refs, dones)
    assert all(same_bits(a, b) for a, b in zip(two, again))
    flipped = dones.clone()
    flipped[-1] = 1 - flipped[-1]
    assert all(same_bits(a, b) for a, b in zip(two, run_kernels(refs, flipped)[0]))
    for k in range(2):  # the two-network call against one-network calls
        assert same_bits(two[k], run_kernels([refs[k]], dones)[0][0]), k
    alone = run_kernels([refs[0]], dones, rows=slice(16, 33))[0][0]  # rows 16..32 as an N = 17 call
    for name in ("h", "c", "gates", "dz"):
        assert torch.equal(two[0][name][:, 16:33], alone[name]), name
    for name in ("dh0", "dc0"):
        assert torch.equal(two[0][name][16:33], alone[name]), name


@pytest.mark.parametrize("case", [(8, 33, 45, 20), (2, 17, 45, 256), (1, 1, 1, 1)])
def test_guard_regions_stay_untouched(gpu, case):
    refs = [reference(case, "planted", k) for k in range(2)]
    plain, _ = run_kernels(refs, refs[0]["dones"])
    got, flats = run_kernels(refs, refs[0]["dones"], guard=True)
    assert len(flats) == 12
    for f in flats:
        assert (f[-GUARD:] == SENTINEL).all() and (f[:-GUARD] != SENTINEL).all()
    assert all(same_bits(a, b) for a, b in zip(plain, got))


# ---------------------------------------------------------------------------------------------- 4
def test_pack_forward_backward_captured_as_one_graph(gpu):
    case = (2, 17, 45, 256)  # over 64 KiB of LDS: the eager calls below are the warm-up
    refs = [reference(case, "planted", k) for k in range(2)]
    eager, _ = run_kernels(refs, refs[0]["dones"])
    dev = "cuda"
    T, N, _, H = case
    d8 = (refs[0]["dones"] != 0).to(torch.uint8).to(dev)
    w = [r["rnn"].weight_hh_l0.detach().to(dev) for r in refs]
    desc = _learn.lstm_seq_desc(w)
    packed = torch.zeros(_learn.lstm_seq_packed_bytes(desc) // 4, device=dev)
    zxs = [torch.addmm((r["rnn"].bias_ih_l0 + r["rnn"].bias_hh_l0).detach().to(dev), r["x"].to(dev).reshape(T * N, -1),
                       r["rnn"].weight_ih_l0.detach().to(dev).t()).view(T, N, 4 * H) for r in refs]
    h0s, c0s = [r["h0"].to(dev) for r in refs], [r["c0"].to(dev) for r in refs]
    dhs = [r["dh"].to(dev) for r in refs]
    fwd = [tuple(torch.zeros(T, N, s, device=dev) for s in (H, H, 4 * H)) for _ in refs]
    bwd = [(torch.zeros(T, N, 4 * H, device=dev), torch.zeros(N, H, device=dev), torch.zeros(N, H, device=dev))
           for _ in refs]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _learn.lstm_seq_pack(desc, packed)
        _learn.lstm_seq_forward(desc, packed, zxs, d8, h0s, c0s, out=fwd)
        _learn.lstm_seq_backward(desc, packed, dhs, [(o[1], o[2]) for o in fwd], d8, c0s, out=bwd)
    for _ in range(2):
        for t in [packed] + [t for o in fwd + bwd for t in o]:
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        for e, f, b in zip(eager, fwd, bwd):
            got = dict(zip(("h", "c", "gates", "dz", "dh0", "dc0"), f + b))
            assert same_bits(e, got)


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("case,kind", [((8, 33, 45, 20), "planted"), ((2, 17, 45, 256), "all"), ((8, 17, 1, 1), "none")])
def test_autograd_node_against_the_torch_loop_and_fp64(gpu, case, kind):
    refs = [reference(case, kind, k) for k in range(2)]
    dev = "cuda"
    dones = refs[0]["dones"].to(dev)
    rnns = [nn.LSTM(r["rnn"].input_size, r["rnn"].hidden_size).to(dev) for r in refs]
    for m, r in zip(rnns, refs):
        m.load_state_dict(r["rnn"].state_dict())

    def leaves():
        return [tuple(r[n].to(dev)[None].clone().requires_grad_() for n in ("h0", "c0")) for r in refs]

    def grads(outs, states):
        for m in rnns:
            m.zero_grad()
        sum((o * r["dh"].to(dev)).sum() for o, r in zip(outs, refs)).backward()
        return [{"dW_ih": m.weight_ih_l0.grad.clone(), "dW_hh": m.weight_hh_l0.grad.clone(),
                 "db_ih": m.bias_ih_l0.grad.clone(), "db_hh": m.bias_hh_l0.grad.clone(), "dh0": s[0].grad[0],
                 "dc0": s[1].grad[0]} for m, s in zip(rnns, states)]

    xs = [r["x"].to(dev) for r in refs]
    st = leaves()
    pair = R.lstm_sequence_pair(rnns, xs, dones, st)
    assert all(type(o.grad_fn).__name__.startswith("_LstmSeq") for o in pair)
    g_pair = grads(pair, st)
    st1 = leaves()
    single = [R.lstm_sequence(m, x, dones, s) for m, x, s in zip(rnns, xs, st1)]
    g_single = grads(single, st1)
    st2 = leaves()
    loop = [R.lstm_sequence_torch(m, x, dones, s) for m, x, s in zip(rnns, xs, st2)]
    for k, ref in enumerate(refs):
        assert torch.equal(pair[k], single[k])
        r64, e = ref["fwd"]["h"]
        ok, worst = inside(pair[k], r64, e)
        ok_l, worst_l = inside(pair[k].detach().cpu() - loop[k].detach().cpu(), torch.zeros_like(r64), e, factor=2.0)
        print(f"AUTOGRAD case {case} net {k}: node {worst:.4f} of the bound, node - torch loop {worst_l:.4f} of twice")
        assert ok and ok_l, (k, worst, worst_l)
        yard = yardstick(ref)
        for name, g in (("pair", g_pair[k]), ("single", g_single[k])):
            per = {n: float((g[n].double().cpu() - ref["g64"][n]).abs().max() / max(float(ref["g64"][n].abs().max()), 1e-300))
                   for n in GRADS if n != "dz"}
            print(f"AUTOGRAD case {case} net {k} {name}: worst {max(per.values()):.3e}, yardstick {yard:.3e}, ratio "
                  f"{max(per.values()) / yard:.3f}")
            assert max(per.values()) <= FACTOR * yard, (name, per, yard)
        assert all(torch.equal(g_pair[k][n], g_single[k][n]) for n in g_pair[k])


# ---------------------------------------------------------------------------------------------- 6
def _recurrent_runner(n=64, **alg_kw):
    import dataclasses

    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from isaaclab_rl.rsl_rl import RslRlPpoActorCriticRecurrentCfg, RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    agent = load_cfg_from_registry(TASK, "rsl_rl_cfg_entry_point")
    agent.device = "cuda:0"
    agent.num_steps_per_env = 8
    for k, v in alg_kw.items():
        setattr(agent.algorithm, k, v)
    kept = {fl.name: getattr(agent.policy, fl.name) for fl in dataclasses.fields(agent.policy) if fl.name != "class_name"}
    agent.policy = RslRlPpoActorCriticRecurrentCfg(**kept)
    cfg = load_cfg_from_registry(TASK, "env_cfg_entry_point")
    cfg.scene.num_envs, cfg.sim.device, cfg.seed = n, "cuda:0", 3
    env = RslRlVecEnvWrapper(gym.make(TASK, cfg=cfg))
    return env, OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0")


def test_training_with_the_switch_on(gpu, monkeypatch):
    monkeypatch.delenv("H12_POLICY_FUSED", raising=False)
    monkeypatch.delenv("H12_RNN_UPDATE_FUSED", raising=False)
    env, runner = _recurrent_runner(fused_rnn_update=True)
    alg, policy = runner.alg, runner.alg.policy
    assert alg.fused_rnn_update and policy.memory_a.rnn.hidden_size == 256
    seen, nodes = [], []
    inner = alg._minibatch

    def probe(b, idx, stats, rec=None):
        if not seen:
            assert "masks" not in rec and rec["dones"].dtype == torch.uint8
            with torch.no_grad():
                policy.act(rec["observations"], dones=rec["dones"], hidden_states=rec["hidden_a"])
                ratio = torch.exp(policy.get_actions_log_prob(rec["actions"]) - rec["actions_log_prob"].squeeze(-1))
                seen.append(float((ratio - 1).abs().mean()))
        out = inner(b, idx, stats, rec=rec)
        nodes.append(policy.memory_a.rnn.weight_hh_l0.grad is not None)
        return out

    monkeypatch.setattr(alg, "_minibatch", probe)
    calls = []
    fwd = _learn.lstm_seq_forward
    monkeypatch.setattr(_learn, "lstm_seq_forward", lambda desc, *a, **k: (calls.append(desc.n_nets), fwd(desc, *a, **k))[1])
    before = {k: v.clone() for k, v in policy.state_dict().items()}
    runner.learn(2)
    env.close()
    stats = runner.last_iteration_stats
    for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"):
        assert torch.isfinite(torch.tensor(stats[k])), (k, stats[k])
    for k in ("memory_a.rnn.weight_hh_l0", "memory_c.rnn.weight_ih_l0", "actor.0.weight", "critic.0.weight"):
        assert not torch.equal(before[k], policy.state_dict()[k]), k
    # every minibatch went through one two-network kernel call (the probe's own act is a one-network call)
    assert calls.count(2) == len(nodes) == 2 * alg.num_learning_epochs * alg.num_mini_batches and all(nodes)
    print(f"first minibatch of the first epoch: mean |ratio - 1| = {seen[0]:.3e}")
    assert seen[0] < 1e-3


def test_train_script_with_fused_rnn_update(gpu, tmp_path):
    train = ROOT / "h1v2-isaac_amd" / "scripts" / "train.py"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, str(train), "--task", TASK, "--headless",
                        "--num_envs", "64", "--max_iterations", "2", "--recurrent", "--fused_rnn_update"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    run = next((tmp_path / "logs" / "rsl_rl" / "h12_12dof_flat").iterdir())
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2
    assert all(torch.isfinite(torch.tensor(float(v))) for ln in lines for k, v in ln.items() if k.startswith("Loss/"))
