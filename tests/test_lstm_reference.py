"""CPU: the fp64 reference and a-priori bound of the fused LSTM step (tests/helpers/lstm_ref.py) tested on their own,
at every shape, normaliser kind and n that tests/test_gpu_recurrent_edges.py uses.  No kernel runs here.

Headroom        torch.nn.LSTM + the MLP in fp32 on the CPU (the normaliser module in eval mode in front) stays within
                half the bound everywhere: the bound is not vacuous for an honest fp32 evaluation.  Measured: worst
                0.224 of the bound (the 1 -> 1 -> 1 network without a normaliser), 0.0081 with the planted columns.
Discrimination  at (45, 64, [40, 24], 12), n = 17, with the planted zero-variance columns, an fp32 evaluation with one
                mistake (eps on the other side of the square root, the other kind's formula, the mean read one column
                on, eps dropped, gates f and g exchanged) leaves the bound by more than 10 times: a kernel that made
                it would fail the GPU tests.  Measured (the worst of y, h', c'): 2.6e3 to 9.8e4 times the bound for
                the finite ones; eps dropped divides by zero.
"""
import pytest
import torch

import lstm_ref as R

NS = (1, 17, 33)
# tests/test_gpu_recurrent_edges.py: a (with a normaliser) and b (without)
NORM_SHAPES = [(1, 1, [], 1), (16, 7, [5], 3), (45, 64, [40, 24], 12), (448, 256, [512, 256, 128], 12)]
EDGE_SHAPES = [(1, 1, [], 1), (16, 7, [5], 3), (32, 16, [16], 12), (448, 256, [512, 256, 128], 12),
               (1024, 256, [1024], 12)]
DISC_SHAPE = (45, 64, [40, 24], 12)


def worst_fraction(shape, kind, planted, n_nets, seed):
    pairs = R.make_pairs(shape, n_nets, seed, device="cpu")
    norm = R.make_planted_norm(kind, shape[0], 100 + seed, device="cpu", planted=planted)
    worst = 0.0
    for n in NS:
        _, states = R.make_inputs(shape, n, n_nets, seed=1000 * seed + n, device="cpu")
        x = R.make_norm_x(n, shape[0], norm, seed=2000 * seed + n, device="cpu", planted=planted)
        for (rnn, net), (h, c) in zip(pairs, states):
            ref, bound = R.lstm_fp64_with_bound(rnn, net, x, h, c, norm=norm)
            got = R.torch_cpu(rnn, net, x, h, c, norm=norm)
            for name, g, r, e in zip("yhc", got, ref, bound):
                ok, fr = R.inside(g, r, e)
                assert ok, (shape, kind, planted, n, name, fr)
                worst = max(worst, fr)
    return worst


@pytest.mark.parametrize("planted", [True, False])
@pytest.mark.parametrize("kind", ["var", "std"])
@pytest.mark.parametrize("case", range(len(NORM_SHAPES)))
def test_headroom_with_a_normaliser(case, kind, planted):
    w = worst_fraction(NORM_SHAPES[case], kind, planted, 2, seed=case)
    print(f"shape {NORM_SHAPES[case]} kind {kind} planted {planted}: torch fp32 at most {w:.3e} of the bound")
    assert w <= 0.5


@pytest.mark.parametrize("case", range(len(EDGE_SHAPES)))
def test_headroom_at_the_shape_edges(case):
    w = worst_fraction(EDGE_SHAPES[case], "none", False, 1, seed=10 + case)
    print(f"shape {EDGE_SHAPES[case]}: torch fp32 at most {w:.3e} of the bound")
    assert w <= 0.5


@pytest.fixture(scope="module")
def discrimination_case():
    out = {}
    for kind in ("var", "std"):
        (rnn, net), = R.make_pairs(DISC_SHAPE, 1, seed=31, device="cpu")
        norm = R.make_planted_norm(kind, DISC_SHAPE[0], 131, device="cpu")
        _, [(h, c)] = R.make_inputs(DISC_SHAPE, 17, 1, seed=32, device="cpu")
        x = R.make_norm_x(17, DISC_SHAPE[0], norm, seed=33, device="cpu")
        out[kind] = (rnn, net, norm, x, h, c, R.lstm_fp64_with_bound(rnn, net, x, h, c, norm=norm))
    return out


@pytest.mark.parametrize("kind", ["var", "std"])
def test_the_honest_evaluation_is_inside_at_the_discrimination_case(discrimination_case, kind):
    rnn, net, norm, x, h, c, (ref, bound) = discrimination_case[kind]
    x_n = R.normalise_torch(norm, x)
    cols = R.planted_columns(DISC_SHAPE[0])
    assert float(x_n[:, cols].abs().max()) <= 1.01 and float(x_n[:, cols].abs().max()) > 0.5
    for name, g, r, e in zip("yhc", R.torch_cpu(rnn, net, x, h, c, norm=norm), ref, bound):
        ok, fr = R.inside(g, r, e)
        assert ok and fr <= 0.5, (name, fr)


@pytest.mark.parametrize("mistake", R.MISTAKES)
@pytest.mark.parametrize("kind", ["var", "std"])
def test_a_planted_mistake_leaves_the_bound(discrimination_case, kind, mistake):
    rnn, net, norm, x, h, c, (ref, bound) = discrimination_case[kind]
    got = R.torch_cpu_with_mistake(rnn, net, x, h, c, norm, mistake)
    worst = 0.0
    for name, g, r, e in zip("yhc", got, ref, bound):
        ok, fr = R.inside(g, r, e)
        print(f"kind {kind} mistake {mistake} {name}: {fr:.3e} times the bound")
        worst = max(worst, fr)
    # the GPU tests assert every element of y, h' and c': the worst of them is what such a kernel would fail by (y goes
    # through gates that the wrong input saturates and through the MLP's compounded bound, so it moves least)
    assert worst > 10.0, worst
