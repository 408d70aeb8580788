"""h12env.graphs: the training-state snapshot (CPU) and the capture routine (GPU).

The snapshot is what undoes a capture's warm-up: parameters and optimiser state come back bit for bit, and a state
entry the warm-up created lazily comes back as its initial zero.  The capture tests pin what every "graph equals
eager" test of the trainers depends on: two warm-up runs, undone before the capture, the generator state of entry."""
import copy

import pytest
import torch
import torch.nn as nn

from h12env.graphs import TrainingState, capture


def make_net():
    torch.manual_seed(3)
    net = nn.Sequential(nn.Linear(5, 7), nn.Linear(7, 2))
    return net, torch.optim.Adam(net.parameters(), lr=1e-2), torch.randn(6, 5)


def step(net, opt, x):
    opt.zero_grad()
    net(x).square().sum().backward()
    opt.step()


def state_tensors(opt):
    return [(k, v) for s in opt.state.values() for k, v in sorted(s.items()) if torch.is_tensor(v)]


def test_snapshot_before_any_step_restores_parameters_and_zeroes_lazily_created_state():
    net, opt, x = make_net()
    ref = copy.deepcopy(net)
    ref_opt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    originals = [p.detach().clone() for p in net.parameters()]
    snap = TrainingState(net.parameters(), opt)
    step(net, opt, x), step(net, opt, x)
    assert all(not torch.equal(p, o) for p, o in zip(net.parameters(), originals))
    snap.restore()
    for p, o in zip(net.parameters(), originals):
        assert torch.equal(p, o)
    created = state_tensors(opt)
    assert {k for k, _ in created} == {"exp_avg", "exp_avg_sq", "step"} and len(created) == 3 * 4
    for k, v in created:
        assert not v.any(), k
    step(net, opt, x)   # the third step, from the restored state
    step(ref, ref_opt, x)  # the first step of an untouched copy
    for p, q in zip(net.parameters(), ref.parameters()):
        assert torch.equal(p, q)
    for (k, v), (_, w) in zip(state_tensors(opt), state_tensors(ref_opt)):
        assert torch.equal(v, w), k


def test_snapshot_after_one_step_restores_the_optimiser_state_exactly():
    net, opt, x = make_net()
    extra = torch.tensor([1.5, -2.0])
    step(net, opt, x)
    params = [p.detach().clone() for p in net.parameters()]
    before = [(k, v.clone()) for k, v in state_tensors(opt)]
    assert all(v.any() for _, v in before)
    snap = TrainingState(net.parameters(), opt, [extra])
    step(net, opt, x), step(net, opt, x)
    extra.add_(1.0)
    snap.restore()
    for p, o in zip(net.parameters(), params):
        assert torch.equal(p, o)
    after = state_tensors(opt)
    assert [k for k, _ in after] == [k for k, _ in before]
    for (k, v), (_, w) in zip(after, before):
        assert torch.equal(v, w), k
    assert float(after[[k for k, _ in after].index("step")][1]) == 1.0
    assert torch.equal(extra, torch.tensor([1.5, -2.0]))


# ---------------------------------------------------------------------------------------------- capture
N, D = 8, 4


class Body:
    """Adds noise to a static output, increments a state tensor in place, reads a static input."""

    def __init__(self, dev):
        g = torch.Generator(device="cpu").manual_seed(11)
        self.inp = torch.randn(N, D, generator=g).to(dev)
        self.out = torch.zeros(N, D, device=dev)
        self.state = torch.arange(N * D, dtype=torch.float32, device=dev).reshape(N, D)

    def __call__(self):
        self.out.add_(torch.randn_like(self.out))
        self.state.add_(1.0)
        return self.out, self.state + self.inp


def eager_three(dev, inputs):
    torch.manual_seed(5)
    b = Body(dev)
    rec = []
    for x in inputs:
        b.inp.copy_(x)
        out, y = b()
        rec.append((out.clone(), y.clone(), b.state.clone()))
    return rec


@pytest.mark.gpu
def test_capture_undoes_the_warm_up_and_replays_equal_eager_calls(gpu):
    inputs = [torch.full((N, D), float(k), device=gpu) for k in range(3)]
    eager = eager_three(gpu, inputs)
    torch.manual_seed(5)
    b = Body(gpu)
    state0, out0, rng0 = b.state.clone(), b.out.clone(), torch.cuda.get_rng_state(gpu)
    graph, (out, y) = capture(b, gpu, undo=(b.state, b.out), rng=True)
    torch.cuda.synchronize()
    assert torch.equal(b.state, state0) and torch.equal(b.out, out0)
    assert torch.equal(torch.cuda.get_rng_state(gpu), rng0)
    assert out is b.out
    for x, (e_out, e_y, e_state) in zip(inputs, eager):
        b.inp.copy_(x)
        graph.replay()
        assert torch.equal(out, e_out) and torch.equal(y, e_y) and torch.equal(b.state, e_state)
    assert not torch.equal(eager[0][0], eager[1][0] - eager[0][0])  # the draws differ from call to call


@pytest.mark.gpu
def test_capture_without_undo_leaves_exactly_two_warm_up_runs(gpu):
    torch.manual_seed(5)
    b = Body(gpu)
    state0, rng0 = b.state.clone(), torch.cuda.get_rng_state(gpu)
    seen = []
    graph, _ = capture(b, gpu, before_capture=lambda: seen.append(b.state.clone()))
    torch.cuda.synchronize()
    assert torch.equal(b.state, state0 + 2.0)          # two warm-up runs; the capture itself launches nothing
    assert len(seen) == 1 and torch.equal(seen[0], state0 + 2.0)  # before_capture: once, after the warm-up
    assert not torch.equal(torch.cuda.get_rng_state(gpu), rng0)   # rng=False: the draws stay consumed
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(b.state, state0 + 3.0)
