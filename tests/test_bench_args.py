"""CPU: bench.py's argument checks: the compact rollout records rebuild flat / rsl history rows only,
so --rollout on is rejected for the other tasks and 'auto' leaves them off at N > 1; --dump-rollout only for windows
that hold one rollout's data."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


@pytest.mark.parametrize("task", ["rough", "c5", "cat"])
def test_rollout_on_rejected_for_tasks_without_history_records(monkeypatch, task):
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--task", task, "--rollout", "on")
    a = parse(monkeypatch, "--task", task)  # auto stays accepted (and off for this task at any N)
    assert a.rollout == "auto" and task not in bench.ROLLOUT_TASKS


@pytest.mark.parametrize("task", ["flat", "rsl"])
def test_rollout_on_accepted_for_flat_and_rsl(monkeypatch, task):
    assert parse(monkeypatch, "--task", task, "--rollout", "on").rollout == "on"


def test_dump_rollout_window_bound(monkeypatch):
    parse(monkeypatch, "--rollout", "on", "--steps", "48", "--dump-rollout", "x.npz")
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--rollout", "on", "--steps", "49", "--dump-rollout", "x.npz")
    parse(monkeypatch, "--rollout", "on", "--steps", "24", "--rollout-decode", "--dump-rollout", "x.npz")
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--rollout", "on", "--steps", "25", "--rollout-decode", "--dump-rollout", "x.npz")


def test_pmc_summary_matched_by_source_or_device_isa(monkeypatch, tmp_path):
    """bench.load_pmc uses a PMC summary only for the current kernel: the same source hash, or the same device ISA
    hash as profiles/latest_isa.json (which must itself be made from the current source)."""
    import json

    src = bench.kernel_source_sha256()
    p = tmp_path / "pmc.json"
    p.write_text(json.dumps({"source_sha256": src, "kernels": {"step_kernel": {"x": 1}}}))
    assert bench.load_pmc(p)[0] == {"step_kernel": {"x": 1}}
    monkeypatch.setattr(bench, "load_isa", lambda: ({"isa_sha256": "aa"}, "isa"))
    p.write_text(json.dumps({"source_sha256": "old", "isa_sha256": "aa", "kernels": {"step_kernel": {}}}))
    assert bench.load_pmc(p)[0] == {"step_kernel": {}}
    for isa in ("bb", None):
        p.write_text(json.dumps({"source_sha256": "old", "isa_sha256": isa, "kernels": {"step_kernel": {}}}))
        k, why = bench.load_pmc(p)
        assert k == {} and "stale" in why
    monkeypatch.setattr(bench, "load_isa", lambda: ({}, "latest_isa.json: stale (kernel source changed)"))
    p.write_text(json.dumps({"source_sha256": "old", "isa_sha256": "aa", "kernels": {"step_kernel": {}}}))
    assert bench.load_pmc(p)[0] == {}


def test_kernel_source_hash_covers_the_headers(monkeypatch, tmp_path):
    """The summaries' key changes with a header-only edit (csrc/*.h, include/*.h), not only with csrc/h12env.hip."""
    import shutil

    from h12env import build as B

    base = bench.kernel_source_sha256()
    shutil.copytree(ROOT / "h1v2-isaac_amd" / "csrc", tmp_path / "h1v2-isaac_amd" / "csrc")
    shutil.copytree(ROOT / "include", tmp_path / "include")
    monkeypatch.setattr(B, "CSRC", tmp_path / "h1v2-isaac_amd" / "csrc")
    monkeypatch.setattr(B, "REPO", tmp_path)
    assert B.source_sha256() == base
    for f in (tmp_path / "h1v2-isaac_amd" / "csrc" / "h12_math.h", tmp_path / "include" / "h12env.h"):
        old = f.read_bytes()
        f.write_bytes(old + b"\n// edit\n")
        assert B.source_sha256() != base, f.name
        f.write_bytes(old)


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert a.full is False and a.dump_outputs is None and a.steps == 20 and a.warmup == 5
    a = parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full is True and a.dump_outputs == "d"
    with pytest.raises(SystemExit):  # ms_per_step is the window over --steps: an empty window has none
        parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_float32_arrays_within_the_budget(monkeypatch, tmp_path):
    import numpy as np
    import torch

    g = torch.Generator().manual_seed(0)
    n = 37
    arrays = {"obs_policy": torch.randn(n, 450, generator=g), "reward": torch.randn(n, generator=g),
              "terminated": torch.rand(n, generator=g) < 0.5, "time_outs": (torch.rand(n, generator=g) < 0.5).to(torch.uint8)}
    bench.dump_outputs(tmp_path / "all", arrays)
    for k, v in arrays.items():
        a = np.load(tmp_path / "all" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(v.shape)
        np.testing.assert_array_equal(a, v.float().numpy())
    assert not (tmp_path / "all" / "env_ids.npy").exists()
    # over the budget: the same seeded sample of envs for every array, ids beside them
    per_env = (450 + 3) * 4 + 8
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 10 * per_env + 5)
    for d in ("s1", "s2"):
        bench.dump_outputs(tmp_path / d, arrays)
    ids = np.load(tmp_path / "s1" / "env_ids.npy")
    assert ids.dtype == np.float64 and len(ids) == 10 and len(set(ids)) == 10 and (np.diff(ids) > 0).all()
    np.testing.assert_array_equal(ids, np.load(tmp_path / "s2" / "env_ids.npy"))
    total = 0
    for k, v in arrays.items():
        a = np.load(tmp_path / "s1" / f"{k}.npy")
        np.testing.assert_array_equal(a, v.float().numpy()[ids.astype(int)])
        total += a.nbytes
    assert total + ids.nbytes <= bench.DUMP_BUDGET_BYTES
