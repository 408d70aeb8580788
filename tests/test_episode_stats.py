"""h12env.ppo.EpisodeStats (the runner's reward / length deques) against rsl_rl's per-step rule, restated here as a
plain Python loop: after each step, for each env with dones > 0 in index order, append its running sums and its length to
the deques and zero them.  EpisodeStats records the finished episodes on the device at every step and moves them once
per iteration (flush); the deques must hold the same entries in the same order.  Rewards are integer-valued, so every
sum is exact and the comparison is for equality."""
from collections import deque

import pytest
import torch

from h12env.ppo import EpisodeStats

N, T = 5, 6
STREAMS = ("reward", "extrinsic", "intrinsic")


def planted():
    """dones [3 iterations][T][N] and integer-valued rewards per stream, reward = extrinsic + intrinsic.
    Iteration 0: env 0 is done at step 0 and again at step 4, envs 1 and 2 are done in the same step (2); env 3 is
    never done; env 4's first episode spans the flush and ends in iteration 1 (step 1), as does env 1's second (step 3).
    Iteration 2 has no done at all."""
    dones = torch.zeros(3, T, N, dtype=torch.long)
    for it, t, e in ((0, 0, 0), (0, 2, 1), (0, 2, 2), (0, 4, 0), (1, 1, 4), (1, 3, 1)):
        dones[it, t, e] = 1
    g = torch.Generator().manual_seed(0)
    extrinsic = torch.randint(-3, 4, (3, T, N), generator=g).float()
    intrinsic = torch.randint(0, 3, (3, T, N), generator=g).float()
    return dones, {"reward": extrinsic + intrinsic, "extrinsic": extrinsic, "intrinsic": intrinsic}


class PerStepRule:
    """The reference: Python floats and lists, the deques extended at every step."""

    def __init__(self, n, streams):
        self.sums = {k: [0.0] * n for k in streams}
        self.length = [0.0] * n
        self.buffers = {k: deque(maxlen=100) for k in (*streams, "length")}

    def step(self, dones, rewards):
        for e, d in enumerate(dones.tolist()):
            for k in self.sums:
                self.sums[k][e] += float(rewards[k][e])
            self.length[e] += 1.0
            if d > 0:
                for k in self.sums:
                    self.buffers[k].append(self.sums[k][e])
                    self.sums[k][e] = 0.0
                self.buffers["length"].append(self.length[e])
                self.length[e] = 0.0


def run_planted(streams, device, per_step=lambda f: f()):
    """Both over the planted case.  Returns the tracker's and the rule's deques as lists after each iteration's
    flush."""
    dones, rewards = planted()
    rule = PerStepRule(N, streams)
    stats = EpisodeStats(N, device, streams)
    dones_d = dones.to(device)
    rewards_d = {k: rewards[k].to(device) for k in streams}
    got, want = [], []
    for it in range(dones.shape[0]):
        for t in range(T):
            per_step(lambda: stats.step(dones_d[it, t], **{k: rewards_d[k][it, t] for k in streams}))
            rule.step(dones[it, t], {k: rewards[k][it, t] for k in streams})
        stats.flush()
        got.append({k: list(v) for k, v in stats.buffers.items()})
        want.append({k: list(v) for k, v in rule.buffers.items()})
    return got, want


def check_planted(got, want, streams):
    assert set(got[0]) == {*streams, "length"}
    for g, w in zip(got, want):
        assert g == w
    # the case is the one described: 4 episodes end in iteration 0, 2 in iteration 1, none in iteration 2
    assert [len(g["length"]) for g in got] == [4, 6, 6]
    assert got[0]["length"] == [1.0, 3.0, 3.0, 4.0]  # env 0; envs 1 and 2 in index order; env 0 again
    assert got[1]["length"][4:] == [8.0, 7.0]  # across the flush: env 4 from the start, env 1 since its first done
    assert got[2] == got[1]  # an iteration without a done leaves the deques as they were
    if "extrinsic" in streams:  # entry i of every deque is the same episode
        assert got[1]["reward"] == [e + i for e, i in zip(got[1]["extrinsic"], got[1]["intrinsic"])]


@pytest.mark.parametrize("streams", [("reward",), STREAMS], ids=["reward", "rnd"])
def test_deques_match_the_per_step_rule(streams):
    got, want = run_planted(streams, "cpu")
    check_planted(got, want, streams)


def test_nothing_recorded_means_nothing_flushed():
    stats = EpisodeStats(N, "cpu")
    stats.flush()
    assert all(len(b) == 0 for b in stats.buffers.values()) and set(stats.buffers) == {"reward", "length"}


def test_maxlen_keeps_the_last_100_in_step_major_order():
    """64 envs x 2 steps, every env done at both: 128 episodes; the deques keep the last 100, i.e. envs 28..63 of step
    0, then envs 0..63 of step 1."""
    n = 64
    env = torch.arange(n).float()
    rule = PerStepRule(n, STREAMS)
    stats = EpisodeStats(n, "cpu", STREAMS)
    ones = torch.ones(n, dtype=torch.long)
    for t in range(2):
        r = {"extrinsic": 1000.0 * t + env, "intrinsic": 3.0 * env + t}
        r["reward"] = r["extrinsic"] + r["intrinsic"]
        stats.step(ones, **r)
        rule.step(ones, r)
    stats.flush()
    got = {k: list(v) for k, v in stats.buffers.items()}
    assert got == {k: list(v) for k, v in rule.buffers.items()}
    assert all(len(v) == 100 for v in got.values())
    assert got["extrinsic"] == [float(e) for e in range(28, 64)] + [1000.0 + e for e in range(64)]
    assert got["length"] == [1.0] * 100
    assert got["reward"] == [e + i for e, i in zip(got["extrinsic"], got["intrinsic"])]


@pytest.mark.gpu
def test_gpu_step_does_not_sync_and_gives_the_same_deques(gpu):
    """The planted case on device tensors: the same deques, and no step() call synchronises with the host."""
    def no_sync(f):
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            f()
        finally:
            torch.cuda.set_sync_debug_mode(before)

    got, want = run_planted(STREAMS, gpu, per_step=no_sync)
    check_planted(got, want, STREAMS)
    # the mode is live in this build: a host read of a device value is refused under it
    with pytest.raises(RuntimeError):
        no_sync(lambda: torch.ones(1, device=gpu).item())
