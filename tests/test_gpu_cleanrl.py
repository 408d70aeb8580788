"""GPU: the learner-side kernels (h12learn_rms_forward, h12learn_gae_soft) and the CleanRL PPO of the CaT task on
the device: precision gates against fp64 restatements, bit-identity of the GAE with the fp32 torch loop, graphed
collection == eager collection, the fused normaliser against the torch path, and an end-to-end run.  The normaliser's
fold is also run at the depth training reaches (RMS_DEPTH_SHAPES: a second fetch batch, the wide segment tree, a
multi-chunk graph replay, count past 2^24); tests/test_rms_emulation.py shows on the CPU that these gates bite."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
SHIMS = ROOT / "h1v2-isaac_amd" / "shims"
if str(SHIMS) not in sys.path:
    sys.path.insert(0, str(SHIMS))

from h12env import cleanrl  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-8
TASK = "Isaac-Velocity-CaT-Flat-H12_12dof-v0"
PLAY = "Isaac-Velocity-CaT-Flat-H12_12dof-Play-v0"


# ---------------------------------------------------------------------------------------------- rms_forward
def rms_batches(n, d, calls=4, seed=0):
    """fp32-valued batches; column j is of kind j % 5: 1e3 + 1e-2 randn, a constant, -7e4 + randn, randn,
    3 + 5 randn (so d = 1 is the first offset column and d >= 3 holds all three hard ones)."""
    rs = np.random.RandomState(seed + 1000 * n + d)
    kind = np.arange(d) % 5
    off = np.choose(kind, [1e3, 2.5, -7e4, 0.0, 3.0])
    scl = np.choose(kind, [1e-2, 0.0, 1.0, 1.0, 5.0])
    return [(off + scl * rs.standard_normal((n, d))).astype(np.float32) for _ in range(calls)]


class Rms64:
    """RunningMeanStd.forward in float64 (ppo.py:9-62)."""

    def __init__(self, d):
        self.mean, self.var, self.count = np.zeros(d), np.ones(d), 1.0

    def __call__(self, x, update=True):
        x = x.astype(np.float64)
        if update:
            bm, bv, n = x.mean(0), x.var(0), x.shape[0]
            delta, tot = bm - self.mean, self.count + n
            m2 = self.var * self.count + bv * n + delta ** 2 * self.count * n / tot
            self.mean, self.var, self.count = self.mean + delta * n / tot, m2 / tot, tot
        return (x - self.mean) / np.sqrt(self.var + EPS)


def check_rms_gates(y, mean32, var32, count32, y64, ref: Rms64, what=""):
    """The gates of the issue, from the precision of fp32 (u = 2^-24); mean, var, sigma are the fp64 values."""
    mean, var = ref.mean, ref.var
    sigma = np.sqrt(var + EPS)
    ey = np.abs(y - y64) / (8 * U * (np.abs(mean) / sigma + np.abs(y64)) + 1e-7)
    em = np.abs(mean32 - mean) / (8 * U * np.abs(mean) + 1e-7 * sigma)
    ev = (np.abs(var32 - var) / var) / (16 * U + (8 * U * np.abs(mean) / sigma) ** 2)
    print(f"{what}: y {ey.max():.3f} mean {em.max():.3f} var {ev.max():.3f} of the bounds")
    assert ey.max() <= 1.0, (what, "y", ey.max())
    assert em.max() <= 1.0, (what, "mean", em.max())
    assert ev.max() <= 1.0, (what, "var", ev.max())
    assert count32 == ref.count, (what, count32, ref.count)


def _rms_shapes():
    from h12env._learn import rms_row_chunk

    R = rms_row_chunk()
    return [(1, 5), (2, 5), (65, 70), (300, 450), (130, 1), (R - 1, 70), (R, 70), (R + 1, 70), (2 * R + 1, 70)]


def _state(d, dev):
    return (torch.zeros(d, device=dev), torch.ones(d, device=dev), torch.ones((), device=dev))


# The smallest shapes that reach each path of the last block's fold (R = 64 rows per chunk, 256 folding threads):
# (n, d): (chunks, chunks per segment, segments, occupied segments).  tests/test_rms_emulation.py recomputes the
# figures from rms_row_chunk(), so a change of R or of the block size fails there and the shapes are chosen anew.
RMS_DEPTH_SHAPES = {
    (2049, 64): (33, 9, 4, 4),         # a second fetch batch of one chunk; segments of 9, 9, 9, 6; last chunk one row
    (4033, 70): (64, 16, 4, 4),        # two full fetch batches per segment (obs_rms at 4096 envs); 6-column tile
    (1100, 5): (18, 1, 32, 18),        # dp = 8 > d; a tree of 18 occupied, then 14 empty segments
    (2113, 12): (34, 3, 16, 12),       # dp = 16; the last segment is one chunk of one row
    (16385, 1): (257, 2, 256, 129),    # the tree's top level merges the lone segment 128 into segment 0
    (32768, 1): (512, 2, 256, 256),    # all 256 segments, the full 8-level tree (value_rms in training)
}
# d = 1 is rms_batches' column 1e3 + 1e-2 randn, whose gates (8u|mean| = 0.05 sigma) cannot see a lost row among
# 16385: the lone segment of (16385, 1) may be dropped unnoticed (tests/test_rms_emulation.py).  So the d = 1
# shapes run a second time on the zero-mean column (kind 3, the 1e-7 sigma gate), which is also what value_rms sees.
RMS_DEPTH_CASES = [(n, d, None) for n, d in RMS_DEPTH_SHAPES] + [(n, d, 3) for n, d in RMS_DEPTH_SHAPES if d == 1]
RMS_LATE_CASES = [(2049, 64, None), (16385, 1, None), (16385, 1, 3)]
RMS_LATE_COUNT = 2.0 ** 24 + 2  # count + n is no longer exact in fp32: 4096 envs are here after ~170 iterations


def rms_case_batches(n, d, kind=None, **kw):
    """rms_batches(n, d), or for a d = 1 case with a column kind, that column of rms_batches(n, kind + 1)."""
    if kind is None:
        return rms_batches(n, d, **kw)
    assert d == 1
    return [np.ascontiguousarray(b[:, kind:kind + 1]) for b in rms_batches(n, kind + 1, **kw)]


def rms_late_case(n, d, kind=None):
    """A late-training state: fp32 (mean, var, count) with the column statistics of a first batch (the constant
    column's variance set to 1e-4) and count = 2^24 + 2, and the three batches that follow."""
    b = rms_case_batches(n, d, kind, calls=4, seed=11)
    x0 = b[0].astype(np.float64)
    v = x0.var(0)
    return (x0.mean(0).astype(np.float32), np.where(v > 0, v, 1e-4).astype(np.float32), np.float32(RMS_LATE_COUNT),
            b[1:])


def check_rms_one_step(y, mean32, var32, count32, xb, before, what=""):
    """One updating call from the fp32 state ``before`` = (mean, var, count): the fp64 reference restarts from that
    state, so the drift of a long fp32 run (the reference algorithm's own property) is not under test.  The count
    is the reference's fp32 ``count + batch_count``, bit for bit (the exact sum is not representable)."""
    ref = Rms64(xb.shape[1])
    ref.mean, ref.var, ref.count = before[0].astype(np.float64), before[1].astype(np.float64), float(before[2])
    y64 = ref(xb, True)
    check_rms_gates(y, mean32, var32, ref.count, y64, ref, what)
    expect = np.float32(before[2]) + np.float32(xb.shape[0])
    assert np.float32(count32).tobytes() == expect.tobytes(), (what, float(count32), float(expect))


def test_rms_forward_against_fp64(gpu):
    from h12env import _learn

    for n, d in _rms_shapes():
        mean, var, count = _state(d, gpu)
        ws = _learn.rms_workspace(n, d, gpu)
        ref = Rms64(d)
        for i, xb in enumerate(rms_batches(n, d)):
            x = torch.from_numpy(xb).to(gpu)
            y = _learn.rms_forward(x, mean, var, count, EPS, True, ws)
            y64 = ref(xb, True)
            check_rms_gates(y.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy(), float(count), y64, ref,
                            f"n={n} d={d} call {i}")
        assert int(ws[0]) == 0  # the arrival counter is left at zero


def test_rms_forward_update_off_alias_and_reproducibility(gpu):
    from h12env import _learn

    for n, d in [(2, 5), (65, 70), (300, 450), (130, 1), (2049, 64), (16385, 1)]:
        b = rms_batches(n, d, calls=3, seed=5)
        mean, var, count = _state(d, gpu)
        ws = _learn.rms_workspace(n, d, gpu)
        _learn.rms_forward(torch.from_numpy(b[0]).to(gpu), mean, var, count, EPS, True, ws)
        s0 = [t.clone() for t in (mean, var, count)]
        # update = 0: statistics untouched (bitwise), y from the stored ones, no workspace needed
        x1 = torch.from_numpy(b[1]).to(gpu)
        y = _learn.rms_forward(x1, mean, var, count, EPS, False)
        for a, s in zip((mean, var, count), s0):
            assert torch.equal(a, s)
        ref = (b[1].astype(np.float64) - s0[0].cpu().numpy().astype(np.float64)) / np.sqrt(
            s0[1].cpu().numpy().astype(np.float64) + EPS)
        assert (np.abs(y.cpu().numpy() - ref) <= 8 * U * np.abs(ref) + 1e-7).all()
        # two runs from the same state: bit-identical statistics and output; y aliasing x: the same again
        x2 = torch.from_numpy(b[2]).to(gpu)
        outs = []
        for alias in (False, False, True):
            st = [s.clone() for s in s0]
            xin = x2.clone()
            yy = _learn.rms_forward(xin, *st, EPS, True, ws, out=xin if alias else None)
            if alias:
                assert yy.data_ptr() == xin.data_ptr()
            outs.append((yy, *st))
        for o in outs[1:]:
            for a, r in zip(o, outs[0]):
                assert torch.equal(a, r)


def test_running_mean_std_module_uses_the_kernel_in_place(gpu, monkeypatch):
    m = cleanrl.RunningMeanStd(shape=(70,)).to(gpu)
    ptrs = [b.data_ptr() for b in (m.running_mean, m.running_var, m.count)]
    xb = rms_batches(65, 70, calls=1)[0]
    x = torch.from_numpy(xb).to(gpu)
    y = m(x)
    assert ptrs == [b.data_ptr() for b in (m.running_mean, m.running_var, m.count)] and float(m.count) == 66.0
    ref = Rms64(70)
    y64 = ref(xb)
    check_rms_gates(y.cpu().numpy(), m.running_mean.cpu().numpy(), m.running_var.cpu().numpy(), float(m.count), y64, ref,
                    "module")
    # shape (): a 1-D batch is n rows of one column
    v = cleanrl.RunningMeanStd(shape=()).to(gpu)
    yv = v(x[:, 0].contiguous())
    ref1 = Rms64(1)
    y1 = ref1(xb[:, :1])
    assert yv.shape == (65,) and v.running_mean.shape == ()
    check_rms_gates(yv.cpu().numpy()[:, None], v.running_mean.cpu().numpy().reshape(1),
                    v.running_var.cpu().numpy().reshape(1), float(v.count), y1, ref1, "module, shape ()")
    # H12_CLEANRL_FUSED=0 selects the torch restatement (other summation order: close, not bit-equal by contract)
    monkeypatch.setenv("H12_CLEANRL_FUSED", "0")
    t = cleanrl.RunningMeanStd(shape=(70,)).to(gpu)
    yt = t(x)
    assert float(t.count) == 66.0
    np.testing.assert_allclose(yt.cpu().numpy(), y64, rtol=1e-3, atol=0.1)  # sanity only: same statistic


def test_rms_forward_against_fp64_at_fold_depth(gpu):
    """The fold as training runs it: more than one fetch batch per segment, a wide segment tree, idle lanes past d
    (RMS_DEPTH_CASES).  The gates are those of the shallow shapes: they do not depend on n."""
    from h12env import _learn

    for n, d, kind in RMS_DEPTH_CASES:
        mean, var, count = _state(d, gpu)
        ws = _learn.rms_workspace(n, d, gpu)
        ref = Rms64(d)
        for i, xb in enumerate(rms_case_batches(n, d, kind)):
            x = torch.from_numpy(xb).to(gpu)
            y = _learn.rms_forward(x, mean, var, count, EPS, True, ws)
            y64 = ref(xb, True)
            check_rms_gates(y.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy(), float(count), y64, ref,
                            f"depth n={n} d={d}{'' if kind is None else f' kind {kind}'} call {i}")
        assert int(ws[0]) == 0


def test_rms_forward_from_a_late_training_state(gpu):
    """count = 2^24 + 2 and statistics of the data's own scale: three one-step checks per shape."""
    from h12env import _learn

    for n, d, kind in RMS_LATE_CASES:
        m0, v0, c0, batches = rms_late_case(n, d, kind)
        mean, var = torch.from_numpy(m0).to(gpu), torch.from_numpy(v0).to(gpu)
        count = torch.tensor(float(c0), device=gpu)
        ws = _learn.rms_workspace(n, d, gpu)
        for i, xb in enumerate(batches):
            before = (mean.cpu().numpy(), var.cpu().numpy(), np.float32(float(count)))
            y = _learn.rms_forward(torch.from_numpy(xb).to(gpu), mean, var, count, EPS, True, ws)
            check_rms_one_step(y.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy(), float(count), xb, before,
                               f"late n={n} d={d}{'' if kind is None else f' kind {kind}'} call {i}")
        assert int(ws[0]) == 0


def test_rms_forward_replayed_in_a_graph_at_fold_depth(gpu):
    """64 chunks x 2 column tiles arrive on the counter inside a captured graph, as obs_rms does on every step of
    a 4096-env collection: three replays on fresh batches are bit-identical to the eager sequence."""
    from h12env import _learn

    n, d = 4033, 70
    b = rms_batches(n, d, calls=4, seed=7)
    mean, var, count = _state(d, gpu)
    ws = _learn.rms_workspace(n, d, gpu)
    eager = []
    for xb in b[1:]:
        y = _learn.rms_forward(torch.from_numpy(xb).to(gpu), mean, var, count, EPS, True, ws)
        eager.append([t.clone() for t in (y, mean, var, count)])
    # static input, output, state and workspace; one warm-up call, then the state is put back
    sx, (smean, svar, scount) = torch.from_numpy(b[0]).to(gpu), _state(d, gpu)
    sy, sws = torch.empty_like(sx), _learn.rms_workspace(n, d, gpu)
    _learn.rms_forward(sx, smean, svar, scount, EPS, True, sws, out=sy)
    torch.cuda.synchronize()
    assert int(sws[0]) == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _learn.rms_forward(sx, smean, svar, scount, EPS, True, sws, out=sy)
    for t, s in zip((smean, svar, scount), _state(d, gpu)):
        t.copy_(s)
    for i, (xb, e) in enumerate(zip(b[1:], eager)):
        sx.copy_(torch.from_numpy(xb))
        g.replay()
        for name, a, r in zip(("y", "mean", "var", "count"), (sy, smean, svar, scount), e):
            assert torch.equal(a, r), (i, name)
        assert int(sws[0]) == 0, i


def test_rms_forward_reuses_a_larger_workspace(gpu):
    """workspace_bytes >= need: one workspace sized for the largest depth shape, never zeroed again, serves the
    d = 1 shapes from the largest n down and back up (stale partials of the larger runs stay behind the smaller
    ones' range); bit-identical to exactly sized fresh workspaces."""
    from h12env import _learn

    need = _learn.learn_library().h12learn_rms_workspace_bytes
    shared = _learn.rms_workspace(*max(RMS_DEPTH_SHAPES, key=lambda s: need(*s)), gpu)
    seq = [32768, 16385, 130, 16385, 32768]
    assert all(need(n, 1) < shared.numel() * 4 for n in seq)
    runs = []
    for fresh in (False, True):
        mean, var, count = _state(1, gpu)
        outs = []
        for i, n in enumerate(seq):
            ws = _learn.rms_workspace(n, 1, gpu) if fresh else shared
            x = torch.from_numpy(rms_batches(n, 1, calls=1, seed=20 + i)[0]).to(gpu)
            y = _learn.rms_forward(x, mean, var, count, EPS, True, ws)
            assert int(ws[0]) == 0, (fresh, i)
            outs.append([t.clone() for t in (y, mean, var, count)])
        runs.append(outs)
    for i, (a, r) in enumerate(zip(*runs)):
        for name, s, t in zip(("y", "mean", "var", "count"), a, r):
            assert torch.equal(s, t), (i, seq[i], name)


# ---------------------------------------------------------------------------------------------- gae_soft
def _gae_inputs(T, N, dev, seed=0):
    g = torch.Generator().manual_seed(seed + 100 * T + N)
    r = torch.randn(T, N, generator=g)
    v = 3.0 * torch.randn(T, N, generator=g)
    d = 0.4 * torch.rand(T, N, generator=g) ** 2
    td = (torch.rand(T, N, generator=g) < 0.2).float()
    nv = 3.0 * torch.randn(N, generator=g)
    nd = 0.4 * torch.rand(N, generator=g)
    ntd = (torch.rand(N, generator=g) < 0.3).float()
    if N > 1:
        td[0, 0], ntd[0] = 1.0, 1.0
    return [t.to(dev) for t in (r, v, d, td, nv, nd, ntd)]


def _gae64(r, v, d, td, nv, nd, ntd, gamma, lam):
    r, v, d, td, nv, nd, ntd = (np.asarray(t.cpu(), dtype=np.float64) for t in (r, v, d, td, nv, nd, ntd))
    adv, last = np.zeros_like(r), 0.0
    for t in reversed(range(r.shape[0])):
        nn, tn, nx = (1 - nd, 1 - ntd, nv) if t == r.shape[0] - 1 else (1 - d[t + 1], 1 - td[t + 1], v[t + 1])
        delta = r[t] + gamma * nx * nn * tn - v[t]
        adv[t] = last = delta + gamma * lam * nn * tn * last
    return adv, adv + v


@pytest.mark.parametrize("T,N", [(1, 1), (1, 65), (3, 64), (24, 130)])
def test_gae_soft_bit_identical_to_torch_loop(gpu, T, N):
    from h12env import _learn

    gamma, lam = 0.99, 0.95
    inp = _gae_inputs(T, N, gpu)
    adv, ret = _learn.gae_soft(*inp, gamma, lam)
    adv_t, ret_t = cleanrl.gae_soft_torch(*inp, gamma, lam)
    assert torch.equal(adv, adv_t) and torch.equal(ret, ret_t)
    # fp64: 1e-5 relative to the magnitude of the summands (delta = r + gamma v' - v cancels, so the rounding error
    # of an element is relative to the values it was formed from, not to the element itself)
    a64, r64 = _gae64(*inp, gamma, lam)
    scale = max(np.abs(a64).max(), np.abs(r64).max())
    assert np.abs(adv.cpu().numpy() - a64).max() <= 1e-5 * scale
    assert np.abs(ret.cpu().numpy() - r64).max() <= 1e-5 * scale


# ---------------------------------------------------------------------------------------------- PPO on the CaT env
class _RecordRaw:
    """Pass-through env wrapper that keeps a copy of every raw policy observation (reset, then each step)."""

    def __init__(self, env):
        self.env, self.raw = env, []

    @property
    def unwrapped(self):
        return self.env.unwrapped

    def reset(self, *a, **k):
        o, e = self.env.reset(*a, **k)
        self.raw.append(o["policy"].clone())
        return o, e

    def step(self, action):
        out = self.env.step(action)
        self.raw.append(out[0]["policy"].clone())
        return out

    def close(self):
        return self.env.close()


def _make_env(task, n=64, seed=3):
    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry

    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    cfg.seed = seed
    return gym.make(task, cfg=cfg)


def _ppo_cfg(**kw):
    from biped_tasks.tasks.agents import H12_12dof_FlatCleanRlPPOCfg

    c = dict(num_steps=4, num_iterations=2, minibatch_size=128, updates_epochs=2, save_interval=2)
    c.update(kw)
    return H12_12dof_FlatCleanRlPPOCfg(**c)


def _collect(tmp, graph: str, n_envs=64, **cfg):
    import os

    old = os.environ.get("H12_PPO_GRAPH")
    os.environ["H12_PPO_GRAPH"] = graph
    try:
        env = _RecordRaw(_make_env(TASK, n=n_envs))
        rec = []
        torch.manual_seed(21)
        agent = cleanrl.PPO(env, _ppo_cfg(**cfg), str(tmp / f"graph{graph}"),
                            on_step=lambda i, o, a, lp, v: rec.append([t.clone() for t in (o, a, lp, v)]))
        env.close()
    finally:
        if old is None:
            os.environ.pop("H12_PPO_GRAPH")
        else:
            os.environ["H12_PPO_GRAPH"] = old
    return agent, rec, env.raw


@pytest.fixture(scope="module")
def collection_runs(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cleanrl_collect")
    return _collect(tmp, "1"), _collect(tmp, "0")


def test_graphed_collection_equals_eager_bit_for_bit(collection_runs):
    (ag, rg, _), (ae, re_, _) = collection_runs
    assert len(rg) == len(re_) == 8
    for i, (g, e) in enumerate(zip(rg, re_)):
        for name, a, b in zip(("obs", "action", "logprob", "value"), g, e):
            assert torch.equal(a, b), (i, name, float((a - b).abs().max()))
    for k in ("running_mean", "running_var", "count"):
        assert torch.equal(getattr(ag.obs_rms, k), getattr(ae.obs_rms, k)), k
        assert torch.equal(getattr(ag.value_rms, k), getattr(ae.value_rms, k)), k
    assert float(ag.obs_rms.count) == 1 + 9 * 64


def test_fused_normaliser_against_torch_path(collection_runs, monkeypatch):
    (_, rec, raw), _ = collection_runs
    monkeypatch.setenv("H12_CLEANRL_FUSED", "0")
    t = cleanrl.RunningMeanStd(shape=(raw[0].shape[1],)).to(raw[0].device)
    worst = 0.0
    for i, (r, (o, _, _, _)) in enumerate(zip(raw, rec)):
        yt = t(r).double()
        sigma = torch.sqrt(t.running_var.double() + EPS)
        bound = 8 * U * (t.running_mean.double().abs() / sigma + yt.abs()) + 1e-7
        ratio = float(((o.double() - yt).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (i, ratio)
    print(f"fused vs torch normaliser over the run: at most {worst:.3f} of the bound")


DEEP_ENVS = 2112  # obs_rms: 33 chunks x 270 columns, 9 per segment; value_rms: 4 x 2112 rows, 132 occupied segments


@pytest.fixture(scope="module")
def deep_collection_runs(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cleanrl_collect_deep")
    return [_collect(tmp, graph, n_envs=DEEP_ENVS, minibatch_size=DEEP_ENVS) for graph in ("1", "0")]


def test_graphed_collection_equals_eager_past_one_chunk(deep_collection_runs):
    """The multi-chunk arrival counter replayed inside the collection graph, as in training."""
    (ag, rg, _), (ae, re_, _) = deep_collection_runs
    assert len(rg) == len(re_) == 8 and rg[0][0].shape[0] == DEEP_ENVS
    for i, (g, e) in enumerate(zip(rg, re_)):
        for name, a, b in zip(("obs", "action", "logprob", "value"), g, e):
            assert torch.equal(a, b), (i, name, float((a - b).abs().max()))
    for k in ("running_mean", "running_var", "count"):
        assert torch.equal(getattr(ag.obs_rms, k), getattr(ae.obs_rms, k)), k
        assert torch.equal(getattr(ag.value_rms, k), getattr(ae.value_rms, k)), k
    assert float(ag.obs_rms.count) == 1 + 9 * DEEP_ENVS


def test_fused_normaliser_against_torch_path_past_one_chunk(deep_collection_runs, monkeypatch):
    (_, rec, raw), _ = deep_collection_runs
    monkeypatch.setenv("H12_CLEANRL_FUSED", "0")
    t = cleanrl.RunningMeanStd(shape=(raw[0].shape[1],)).to(raw[0].device)
    worst = 0.0
    for i, (r, (o, _, _, _)) in enumerate(zip(raw, rec)):
        yt = t(r).double()
        sigma = torch.sqrt(t.running_var.double() + EPS)
        bound = 8 * U * (t.running_mean.double().abs() / sigma + yt.abs()) + 1e-7
        ratio = float(((o.double() - yt).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (i, ratio)
    print(f"fused vs torch normaliser over the {DEEP_ENVS}-env run: at most {worst:.3f} of the bound")


def test_cleanrl_ppo_end_to_end_on_the_cat_task(gpu, tmp_path):
    import json

    env = _make_env(TASK)
    torch.manual_seed(4)
    cleanrl.PPO(env, _ppo_cfg(num_iterations=3), str(tmp_path))
    env.close()
    lines = [json.loads(x) for x in (tmp_path / "metrics.jsonl").read_text().splitlines()]
    assert [x["iter"] for x in lines] == [1, 2, 3]
    for x in lines:
        assert "Loss/mean_v_loss" in x and any(k.startswith("Episode_Reward/") for k in x)
        assert all(np.isfinite(v) for v in x.values()), x
    assert (tmp_path / "model_1.pt").exists()
    play = _make_env(PLAY, n=16)
    agent = cleanrl.Agent(play).to(gpu)
    agent.load_state_dict(torch.load(tmp_path / "model_1.pt", map_location=gpu, weights_only=True))
    agent.eval()
    obs = play.reset()[0]["policy"]
    with torch.no_grad():
        a = agent(obs)
        obs2 = play.step(a)[0]["policy"]
        a2 = agent(obs2)
    assert a.shape == (16, 12) and torch.isfinite(a).all() and torch.isfinite(a2).all()
    play.close()
