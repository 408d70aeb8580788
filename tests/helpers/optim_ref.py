"""References for the fused optimiser step (h12env.optim, csrc/h12_optim.hip).

The fp64 reference is torch's own ``Adam`` / ``RAdam`` after ``clip_grad_norm_`` on float64 CPU copies of the fp32 inputs:
independent of the code under test.  The fp32 yardstick is the same torch classes in fp32 on the device with their
default, non-capturable arguments.  Both are computed once per case and never modified.

Gradient sequences are seeded N(0, 1) times a per-step scale that alternates 10 and 1e-3, so that with max_norm = 1 clipped
steps (coef < 1) and unclipped steps (coef == 1) both occur; ``make_case`` asserts both from the fp64 norms."""
from __future__ import annotations

from types import SimpleNamespace

import torch

STEPS = 8
SCALES = (10.0, 1e-3)
MAX_NORM = 1.0
LR = 1e-3
U = 2.0 ** -24


def torch_class(rule: str):
    return {"adam": torch.optim.Adam, "radam": torch.optim.RAdam}[rule]


def rule_kwargs(rule: str, beta2: float = 0.999):
    """The hyper-parameters the trainers use: ppo's Adam (torch's defaults), cleanrl's RAdam (eps 1e-5)."""
    return dict(betas=(0.9, beta2), eps=1e-8 if rule == "adam" else 1e-5)


def make_case(sizes, seed: int, steps: int = STEPS, offset: int = 0, params=None):
    """Parameters (N(0, 1) unless given) and ``steps`` gradients for tensors of ``sizes`` elements, fp32 on the CPU.  With
    ``offset`` every tensor is a view ``offset`` floats into a buffer of its own."""
    g = torch.Generator().manual_seed(seed)
    if params is None:
        params = [torch.randn(n, generator=g) for n in sizes]
    else:
        params = [p.detach().clone().cpu() for p in params]
    grads = [[torch.randn(p.shape, generator=g) * SCALES[s % 2] for p in params] for s in range(steps)]
    norms = [float(torch.sqrt(sum((x.double() ** 2).sum() for x in gs))) for gs in grads]
    assert any(n > MAX_NORM * 1.01 for n in norms) and any(n < MAX_NORM * 0.99 for n in norms), norms
    return SimpleNamespace(sizes=[p.numel() for p in params], params=params, grads=grads, norms=norms, steps=steps,
                           offset=offset)


def run_torch(case, rule: str, dtype, device, lr: float, max_norm, beta2: float = 0.999):
    """``steps`` times clip_grad_norm_ + torch's optimiser on copies of the case; per step the (p, exp_avg, exp_avg_sq)
    of every tensor as float64 CPU tensors, and the norms clip_grad_norm_ returned."""
    ps = [torch.nn.Parameter(p.to(device=device, dtype=dtype)) for p in case.params]
    opt = torch_class(rule)(ps, lr=lr, **rule_kwargs(rule, beta2))
    out, norms = [], []
    for gs in case.grads:
        for p, g_ in zip(ps, gs):
            p.grad = g_.to(device=device, dtype=dtype)
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
        out.append(snapshot(ps, opt))
    return SimpleNamespace(steps=out, norms=norms, opt=opt, params=ps)


def snapshot(ps, opt):
    return tuple([t.detach().double().cpu().clone() for t in ts]
                 for ts in (ps, [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps]))


def device_params(case, device):
    """The case's parameters on the device as leaves the fused optimiser can take; with case.offset, views that start
    ``offset`` floats into a 16-byte aligned buffer (so misaligned for vector access when offset % 4 != 0)."""
    ps = []
    for p in case.params:
        if case.offset:
            buf = torch.zeros(p.numel() + case.offset, device=device)
            t = buf[case.offset:].view(p.shape)
            t.copy_(p)
            assert t.data_ptr() % 16 == (4 * case.offset) % 16 and t.is_contiguous()
        else:
            t = p.to(device)
        ps.append(t.requires_grad_(True))
    return ps


def worst(got, ref):
    """(the worst elementwise error, max|ref|) over every tensor of one quantity."""
    return (max(float((a - b).abs().max()) for a, b in zip(got, ref)), max(float(b.abs().max()) for b in ref))
