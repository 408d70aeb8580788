"""Child process of test_gpu_policy.test_first_call_over_64_kib_of_lds_is_refused_inside_a_capture (the kernels'
"LDS limit raised" flags are per process, so the first calls need a fresh one).  For the inference kernel and then for
the two training kernels, at shapes that need more than 64 KiB of dynamic LDS:
  1. the first such call, made while the stream is capturing, raises "outside a stream capture";
  2. the eager call after it succeeds, inside the fp64 bound of mlp_bounds (the forward so within twice it of torch);
  3. a second capture succeeds and its replay equals the eager result bit for bit.
Exits 0 and prints one "ok" line per kernel; any failed step is an exception."""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import mlp_bounds as B  # noqa: E402
from h12env import _learn  # noqa: E402
from h12env._abi import H12EnvError  # noqa: E402
from h12env.policy import FusedMLP  # noqa: E402


def refused_in_capture(call, x):
    """call(x) inside a capture must raise; the graph holds one torch operation, so it is not empty."""
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            call(x + 0)
    except H12EnvError as e:
        assert "outside a stream capture" in str(e), e
        return
    raise AssertionError("the first call over 64 KiB of LDS was accepted inside a stream capture")


def captured(call, x):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(x)
    g.replay()
    torch.cuda.synchronize()
    return out


def inside(got, ref64, e, what, torch_out=None):
    """got within the a-priori bound e of fp64; torch_out obeys the same bound, so the two are within 2 e."""
    f = B.fraction(got, ref64, e)
    ft = 0.0 if torch_out is None else B.fraction(got, torch_out.double(), 2 * e)
    print(f"{what}: {f:.3e} of the fp64 bound, {ft:.3e} of twice the bound from torch")
    assert f <= 1.0 and ft <= 1.0, (what, f, ft)


@torch.no_grad()
def inference():
    # one layer 1024 -> 16, n = 16: 16 x (1028 + 20) x 4 = 67 072 bytes of LDS
    net = B.random_net([1024, 16], seed=7).cuda().requires_grad_(False)
    x = torch.randn(16, 1024, generator=torch.Generator().manual_seed(8)).cuda()
    f = FusedMLP([net])  # packs; the forward kernel has not run in this process
    torch.cuda.synchronize()
    refused_in_capture(f, x)
    (eager,) = f(x)
    _, _, y64, e = B.forward_fp64(B.linears(net), x)
    inside(eager, y64, e, "mlp_forward y", net(x))
    (replayed,) = captured(f, x)
    assert torch.equal(replayed, eager)
    print("ok mlp_forward")


def training():
    # 16 -> 512 -> 16, n = 32: both kernels need 32 x (20 + 516) x 4 = 68 608 bytes of LDS
    net = B.random_net([16, 512, 16], seed=9).cuda().requires_grad_(False)
    lins = B.linears(net)
    g = torch.Generator().manual_seed(10)
    x, dy = torch.randn(32, 16, generator=g).cuda(), torch.randn(32, 16, generator=g).cuda()
    desc = _learn.mlp_desc([[(m.weight.detach(), m.bias.detach()) for m in lins]])
    packed = torch.empty(_learn.mlp_packed_bytes(desc) // 4, device="cuda")
    packed_t = torch.empty(_learn.mlp_packed_t_bytes(desc) // 4, device="cuda")
    _learn.mlp_pack(desc, packed)
    _learn.mlp_pack_t(desc, packed_t)
    torch.cuda.synchronize()

    def forward(x):
        return _learn.mlp_forward_train(desc, packed, x)

    refused_in_capture(forward, x)
    y, hs = forward(x)
    hs64, es, y64, ey = B.forward_fp64(lins, x)
    with torch.no_grad():
        h_torch = net[1](net[0](x))
        inside(hs[0], hs64[0], es[0], "mlp_forward_train h", h_torch)
        inside(y, y64, ey, "mlp_forward_train y", net(x))
    y2, hs2 = captured(forward, x)
    assert torch.equal(y2, y) and torch.equal(hs2[0], hs[0])
    print("ok mlp_forward_train")

    def backward(dy):
        return _learn.mlp_backward(desc, packed_t, dy, hs, need_dx=True)

    refused_in_capture(backward, dy)
    dzs, dbs, dx = backward(dy)
    ref = B.backward_fp64(lins, x, hs, dy)  # teacher-forced on the saved activations, as in test_gpu_policy_train
    inside(dzs[0], *ref["dz"][0], "mlp_backward dz")
    inside(dx, *ref["dx"], "mlp_backward dx")
    for l in range(len(lins)):
        inside(dbs[l], *ref["db"][l], f"mlp_backward db[{l}]")
    dzs2, dbs2, dx2 = captured(backward, dy)
    assert torch.equal(dzs2[0], dzs[0]) and torch.equal(dx2, dx)
    assert all(torch.equal(a, b) for a, b in zip(dbs2, dbs))
    print("ok mlp_backward")


if __name__ == "__main__":
    inference()
    training()
