"""GPU: a plain bench.py run (no --full) times the window, prints the contract line only, and --dump-outputs writes
what the last timed step returned: the arrays equal one process stepping the same envs with the same seeded actions
and episode lengths, bit for bit."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_outputs(gpu, tmp_path):
    n, K, B, W = 96, 7, 30, 3
    dump = tmp_path / "out"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--envs", str(n), "--steps", str(K), "--warmup", str(W),
           "--burn-in", str(B), "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == K and out["warmup"] == W and out["n_gpus"] == 1 and out["unit"] == "env-steps/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(n * 1e3 / out["ms_per_step"])
    for k in ("roofline", "cpu_baseline", "replay_bit_exact", "resets_in_window", "c4_rollout_allgather"):
        assert k not in out, k  # those take runs of their own: --full

    from h12env import H12FlatEnvCfg
    from h12env.env import H12VelocityEnv

    cfg = H12FlatEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    env = H12VelocityEnv(cfg)
    env.reset()
    pool = min(K + W + B, 256)
    g = torch.Generator(device="cuda:0").manual_seed(1234)  # bench.py: actions first, then the episode lengths
    acts = torch.randn(pool, n, 12, device="cuda:0", generator=g)
    env.episode_length_buf = torch.randint(0, env.max_episode_length, (n,), device="cuda:0", generator=g,
                                           dtype=torch.int32)
    for i in range(B + W + K):
        obs, rew, term, trunc, _ = env.step(acts[i % pool])
    torch.cuda.synchronize()
    want = {"obs_policy": obs["policy"], "reward": rew, "terminated": term, "time_outs": trunc}
    assert sorted(p.name for p in dump.iterdir()) == sorted(f"{k}.npy" for k in want)
    for k, v in want.items():
        a = np.load(dump / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(v.shape), k
        np.testing.assert_array_equal(a, v.float().cpu().numpy(), err_msg=k)
    assert np.isfinite(np.load(dump / "obs_policy.npy")).all()
    env.close()
