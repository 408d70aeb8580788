"""Child process of test_gpu_recurrent.test_first_call_over_64_kib_of_lds_is_refused_inside_a_capture (the kernel's "LDS
limit raised" flag is per process, so the first call needs a fresh one).  At a shape that needs more than 64 KiB of
dynamic LDS (d_in 451, H 256: 16 x (724 + 1028) x 4 = 112 128 bytes):
  1. the first step, made while the stream is capturing, raises "outside a stream capture" and launches nothing: the
     state and the output buffers keep their bytes;
  2. the eager step after it succeeds;
  3. a second capture succeeds and its replay equals the eager result bit for bit.
Exits 0 and prints "ok lstm_step"; any failed step is an exception."""
import sys
from pathlib import Path

import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd"))

from h12env import _learn  # noqa: E402
from h12env._abi import H12EnvError  # noqa: E402
from h12env.policy import FusedLSTMStep  # noqa: E402


@torch.no_grad()
def main():
    torch.manual_seed(3)
    n, d_in, H = 16, 451, 256
    rnn = nn.LSTM(d_in, H).cuda().requires_grad_(False)
    net = nn.Sequential(nn.Linear(H, 12)).cuda().requires_grad_(False)
    f = FusedLSTMStep([(rnn, net)]).refresh()  # packs; the step kernel has not run in this process
    x = torch.randn(n, d_in, device="cuda")
    h0, c0 = torch.randn(n, H, device="cuda").tanh(), torch.randn(n, H, device="cuda")
    state = [(h0.clone(), c0.clone())]
    y = torch.full((n, 12), 7.0, device="cuda")
    torch.cuda.synchronize()

    def step(st):
        return _learn.lstm_step(f._desc, f._packed, x, st, out=(y,))

    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            x2 = x + 0  # the graph holds one torch operation, so it is not empty
            step(state)
    except H12EnvError as e:
        assert "outside a stream capture" in str(e) and "(-2)" in str(e), e
    else:
        raise AssertionError("the first call over 64 KiB of LDS was accepted inside a stream capture")
    del x2
    torch.cuda.synchronize()
    assert torch.equal(state[0][0], h0) and torch.equal(state[0][1], c0) and (y == 7.0).all()  # nothing was launched
    step(state)
    torch.cuda.synchronize()
    eager = (y.clone(), state[0][0].clone(), state[0][1].clone())
    assert torch.isfinite(eager[0]).all() and not torch.equal(eager[1], h0)
    state[0][0].copy_(h0), state[0][1].copy_(c0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(state)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((y, *state[0]), eager))
    print("ok lstm_step")


if __name__ == "__main__":
    main()
