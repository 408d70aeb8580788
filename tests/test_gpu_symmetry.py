"""GPU: h12learn_mirror_rows against the torch table reference (bitwise), inside a captured graph, the mirror map
against the physics of the HIP env, and the PPO update / train.py with rsl_rl's symmetry options on the device."""
import copy
import json
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "h1v2-isaac_amd" / "shims"), str(ROOT / "tests" / "helpers")]

pytestmark = pytest.mark.gpu

FLAT_TERMS = ["base_ang_vel", "projected_gravity", "velocity_commands", "joint_pos", "joint_vel", "actions"]
SIGN = -(2 ** 31)


def table_of(d):
    from h12env import cfg as K
    from h12env import symmetry as S

    if d == 12:
        return S.action_table()
    if d == 45:
        return S.table_from_terms(FLAT_TERMS, 1)
    return S.mirror_table({235: K.H12RoughEnvCfg, 270: K.H12RslEnvCfg, 450: K.H12FlatEnvCfg}[d]())


def planted(n, d, seed, device="cuda:0"):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    flat = x.view(-1)
    for i, v in enumerate((float("nan"), float("inf"), float("-inf"), -0.0, 0.0)):
        flat[i::7][: max(1, flat.numel() // 30)] = v
    flat[flat.numel() // 2] = torch.tensor(0x7FC12345, dtype=torch.int32).view(torch.float32)  # a NaN with a payload
    return x.to(device)


def reference(x, table, idx, both, n_src=None):
    """The table applied to int32 views: gather, column gather, sign-bit XOR, concatenation."""
    xi = x.view(torch.int32)
    rows = xi if idx is None else xi[idx.clamp(0, (n_src or x.shape[0]) - 1)]
    src = table.src.long().to(x.device)
    sign = torch.where(table.flip.to(x.device), torch.tensor(SIGN, dtype=torch.int32, device=x.device),
                       torch.tensor(0, dtype=torch.int32, device=x.device))
    m = rows[:, src] ^ sign
    return torch.cat([rows, m]) if both else m


def indices(kind, n, device="cuda:0"):
    if kind == "none":
        return None
    if kind == "reversed":
        return torch.arange(n - 1, -1, -1, device=device)
    g = torch.Generator().manual_seed(n)
    return torch.randint(0, max(1, n // 2), (n + 3,), generator=g).to(device)  # repeats, and more rows than the source


# ---------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("both", [0, 1])
@pytest.mark.parametrize("d", [12, 45, 235, 270, 450])
def test_kernel_equals_the_table_reference_bitwise(gpu, d, both):
    from h12env._learn import mirror_rows

    t = table_of(d)
    packed = t.packed(gpu)
    for n in (1, 63, 64, 65, 257):
        x = planted(n, d, seed=1000 * d + n)
        assert torch.isnan(x).any() or n * d < 8
        for kind in ("none", "reversed", "repeats"):
            idx = indices(kind, n)
            got = mirror_rows(x, packed, idx, bool(both))
            want = reference(x, t, idx, both)
            assert got.shape == want.shape
            assert torch.equal(got.view(torch.int32), want), (n, kind)
    # the public path: the same launch behind MirrorTable.apply / augment
    out = t.apply(x, indices("reversed", 257), both=bool(both))
    assert torch.equal(out.view(torch.int32), reference(x, t, indices("reversed", 257), both))
    assert torch.equal(t.mirror(t.mirror(x)).view(torch.int32), x.view(torch.int32))


def test_out_of_range_indices_are_clamped(gpu):
    """An idx entry equal to n_src_rows (one past the end), far past it, and negative: each reads the nearest row of
    the source, with no error and nothing read outside x (x sits in the middle of a larger allocation)."""
    from h12env._learn import mirror_rows

    d, n_src = 450, 65
    t = table_of(d)
    whole = planted(n_src + 128, d, seed=5)
    x = whole[64:64 + n_src]
    idx = torch.tensor([0, n_src, n_src - 1, 2 ** 40, -1, -(2 ** 40), 7, n_src], device=gpu)
    for both in (0, 1):
        got = mirror_rows(x, t.packed(gpu), idx, bool(both))
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), reference(x, t, idx, both, n_src))
    assert torch.equal(got[1].view(torch.int32), x[n_src - 1].view(torch.int32))
    assert torch.equal(got[4].view(torch.int32), x[0].view(torch.int32))


def test_source_rows_past_2_31_elements(gpu):
    """Rows whose element offset in x exceeds 2^31 (64-bit row arithmetic): an 8.6 GB source, 70 gathered rows."""
    from h12env._learn import mirror_rows

    d = 450
    n_src = 2 ** 31 // d + 1000
    t = table_of(d)
    x = torch.empty((n_src, d), device=gpu)
    rows = torch.cat([torch.arange(n_src - 65, n_src), torch.tensor([0, 1, n_src // 2, 2 ** 31 // d, 2 ** 31 // d + 1])])
    x[rows.to(gpu)] = planted(rows.numel(), d, seed=9)
    idx = rows.flip(0).to(gpu)
    got = mirror_rows(x, t.packed(gpu), idx, True)
    want = reference(x, t, idx, 1)
    assert torch.equal(got.view(torch.int32), want)
    del x


def test_wrapper_refuses_wrong_tensors(gpu):
    from h12env._learn import mirror_rows

    t = table_of(12)
    x = torch.zeros(4, 12, device=gpu)
    with pytest.raises(ValueError):
        mirror_rows(x, t.packed(gpu)[:11])
    with pytest.raises(ValueError):
        mirror_rows(x, t.packed(gpu), torch.zeros(3, dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError):
        mirror_rows(x, t.packed(gpu), None, True, out=torch.zeros(4, 12, device=gpu))
    with pytest.raises(ValueError):
        mirror_rows(x.double(), t.packed(gpu))


def test_mirror_is_differentiable_on_the_device(gpu):
    """The map is its own transpose: the device path's backward against autograd through the torch indexing path."""
    t = table_of(45)
    x = torch.randn(9, 45, device=gpu, requires_grad=True)
    xc = x.detach().cpu().requires_grad_(True)
    idx = torch.tensor([8, 0, 0, 3], device=gpu)
    w = torch.randn(8, 45, device=gpu)
    (t.apply(x, idx, both=True) * w).sum().backward()
    (t.apply(xc, idx.cpu(), both=True) * w.cpu()).sum().backward()
    torch.testing.assert_close(x.grad.cpu(), xc.grad)


# ---------------------------------------------------------------------------------------------- 2. capture
def test_one_launch_is_capturable_and_replays_on_new_contents(gpu):
    from h12env._learn import mirror_rows

    d, n_src, n = 270, 300, 129
    t = table_of(d)
    packed = t.packed(gpu)
    x = planted(n_src, d, seed=1)
    idx = torch.randperm(n_src, generator=torch.Generator().manual_seed(0))[:n].to(gpu)
    out = torch.zeros(2 * n, d, device=gpu)
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        mirror_rows(x, packed, idx, True, out=out)
    torch.cuda.current_stream(gpu).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mirror_rows(x, packed, idx, True, out=out)
    first = reference(x, t, idx, 1)
    x.copy_(planted(n_src, d, seed=2))
    idx.copy_(torch.randperm(n_src, generator=torch.Generator().manual_seed(3))[:n].to(gpu))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    want = reference(x, t, idx, 1)
    assert not torch.equal(want, first)
    assert torch.equal(out.view(torch.int32), want)


# ---------------------------------------------------------------------------------------------- 3. physics
def test_map_is_pinned_by_the_physics_of_the_hip_env(gpu):
    """tests/test_symmetry.py::test_map_is_pinned_by_the_physics on the HIP env: 16 envs as 8 mirror pairs, 2 steps;
    the table's entry reproduces the paired env's column at <= 0.1 x the best other candidate's error."""
    import mirror_check as MC
    from h12env import symmetry as S
    from h12env.env import H12VelocityEnv

    cfg = MC.pair_cfg("flat", "cuda:0")
    env = H12VelocityEnv(cfg)
    try:
        env.reset()
        MC.mirror_commands(env._field("CMD"))
        rows = []
        for act in MC.paired_actions():
            obs, _, term, _, _ = env.step(torch.from_numpy(act).to(gpu))
            assert not term.any()
            rows.append(obs["policy"].cpu().numpy().copy())
        table = S.mirror_table(env)
        terms = env.observation_manager.active_terms["policy"]
        h = cfg.observations.policy.history_length
    finally:
        env.close()
    import numpy as np

    obs_a = np.concatenate([r[0::2] for r in rows])
    obs_b = np.concatenate([r[1::2] for r in rows])
    bad, worst, seen = MC.identify(table, terms, h, obs_a, obs_b)
    print(f"\nHIP env: {seen} columns, {len(bad)} misidentified, worst ratio {worst:.4f}")
    assert seen == 45
    assert not bad, bad
    assert worst <= MC.MARGIN


# ---------------------------------------------------------------------------------------------- 4. PPO
def ppo_run(monkeypatch, graph, mode):
    from h12env import cfg as K
    from h12env.ppo import PPO, ActorCritic

    monkeypatch.setenv("H12_PPO_GRAPH", "1" if graph else "0")
    torch.manual_seed(7)
    pol = ActorCritic(270, 270, 12, [128, 64], [128, 64])
    sym = None
    if mode is not None:
        sym = {"use_data_augmentation": True, "use_mirror_loss": mode == "both", "mirror_loss_coeff": 0.5,
               "data_augmentation_func": "h12env.symmetry:augment", "_env": K.H12RslEnvCfg()}
    alg = PPO(copy.deepcopy(pol), num_learning_epochs=2, num_mini_batches=4, learning_rate=1e-3, schedule="adaptive",
              desired_kl=0.01, device="cuda:0", symmetry_cfg=sym)
    alg.init_storage(64, 8, [270], None, [12])
    out = []
    for u in range(2):
        g = torch.Generator(device="cuda:0").manual_seed(100 + u)
        for k, v in alg.storage.t.items():
            v.copy_(torch.randn(v.shape, generator=g, device="cuda:0") * (0.1 if k == "sigma" else 1.0))
        alg.storage.t["sigma"].abs_().add_(0.5)
        out.append(alg.update())
    return alg, out


@pytest.mark.parametrize("mode", ["both", "augment"])
def test_graph_captured_symmetric_update_equals_eager(gpu, monkeypatch, mode):
    """64 envs x 8 steps: the update with symmetry replayed from the captured HIP graph (the gather + mirror launches
    are inside it) gives the eager update's parameters bit for bit, and not those of an update without symmetry."""
    a, la = ppo_run(monkeypatch, True, mode)
    b, lb = ppo_run(monkeypatch, False, mode)
    assert a._graph is not None and b._graph is None
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q), (p - q).abs().max()
    assert la == lb and a.learning_rate == b.learning_rate
    assert all(math.isfinite(x["symmetry"]) and x["symmetry"] > 0 for x in la)
    c, lc = ppo_run(monkeypatch, True, None)
    assert "symmetry" not in lc[0]
    assert any(not torch.equal(p, q) for p, q in zip(a.policy.parameters(), c.policy.parameters()))
    for p in a.policy.parameters():
        assert torch.isfinite(p).all()


# ---------------------------------------------------------------------------------------------- 5. train.py
def test_train_script_with_symmetry_both(gpu, tmp_path):
    train = ROOT / "h1v2-isaac_amd" / "scripts" / "train.py"
    r = subprocess.run([sys.executable, str(train), "--task", "Isaac-Velocity-Flat-H12_12dof-v0", "--headless",
                        "--num_envs", "64", "--max_iterations", "2", "--symmetry", "both"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    run = next((tmp_path / "logs" / "rsl_rl" / "h12_12dof_flat").iterdir())
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2
    assert all(math.isfinite(x["Loss/symmetry"]) and x["Loss/symmetry"] > 0 for x in lines)
    assert all(math.isfinite(v) for x in lines for v in x.values() if isinstance(v, float))
