"""Shared by tests/test_gpu_policy_train.py and tests/test_policy_train_api.py: small Linear/ELU networks, exact-integer
networks, and the fp64 references with their a-priori error bounds (u = 2^-24) for the fused MLP's forward and backward.

Forward (no normaliser):   e_z = |W| e_h + (K + 2) u (|W||h| + |b|),   e_h = e_z + 4u |h|.
Backward, teacher-forced on the SAVED fp32 activations h_l (so the ELU branch of f'(h) = h > 0 ? 1 : h + 1 cannot flip):
    e(dZ_{L-1}) = 0
    e(dH_l) = e(dZ_{l+1}) |W_{l+1}| + (K + 2) u |dZ_{l+1}| |W_{l+1}|         K = the width summed over
    e(dZ_l) = f' e(dH_l) + 2u f' |dH_l|
    e(db_l) = sum_r e(dZ_l) + (n + 2) u sum_r |dZ_l|
    e(dW_l)[j, i] = sum_r e(dZ_l)[r, j] |H_{l-1}[r, i]| + (n + 2) u sum_r |dZ_l[r, j]| |H_{l-1}[r, i]|
dX is the dH of the input: e(dX) = e(dZ_0) |W_0| + (K + 2) u |dZ_0| |W_0|.
"""
import torch
import torch.nn as nn

U = 2.0 ** -24


def seq(dims, act=nn.ELU):
    mods = []
    for i in range(len(dims) - 1):
        mods.append(nn.Linear(dims[i], dims[i + 1]))
        if i + 2 < len(dims):
            mods.append(act())
    return nn.Sequential(*mods)


def linears(net):
    return [m for m in net if isinstance(m, nn.Linear)]


def random_net(dims, seed, bias_std=0.3):
    torch.manual_seed(seed)
    net = seq(dims)
    for m in linears(net):
        nn.init.normal_(m.bias, std=bias_std)
    return net


def int_weights(out, k_in, lo, span):
    j = torch.arange(out)[:, None]
    k = torch.arange(k_in)[None, :]
    return (3 * j + 5 * k + (j * k) % 4 + (j // 3)) % span + lo  # asymmetric in (j, k)


def int_net(dims, wlo, wspan, blo, bspan, zero_units=()):
    """A network with integer weights; ``zero_units``: (layer, unit) pairs whose weights and bias are zero, so that the
    unit's activation is exactly 0.  Returns (net, [(W int64, b int64)])."""
    net = seq(dims)
    ints = []
    for l, m in enumerate(linears(net)):
        W = int_weights(m.out_features, m.in_features, wlo, wspan)
        b = (7 * torch.arange(m.out_features)) % bspan + blo
        for zl, zu in zero_units:
            if zl == l:
                W[zu] = 0
                b[zu] = 0
        m.weight.data.copy_(W.float()), m.bias.data.copy_(b.float())
        ints.append((W.long(), b.long()))
    return net, ints


@torch.no_grad()
def int_reference(ints, x, dy):
    """int64 forward and backward of a network whose pre-activations are all >= 0 (ELU the identity, f' = 1).
    Returns a dict of exact results and ``peak``, the largest sum of absolute products of any of them (every partial
    sum of any summation order is at most that)."""
    hs, peak = [x.long()], 0
    for W, b in ints:
        peak = max(peak, int((hs[-1].abs() @ W.abs().T + b.abs()).max()))
        hs.append(hs[-1] @ W.T + b)
    assert all(int(h.min()) >= 0 for h in hs[1:-1]), "a pre-activation is negative: ELU is not the identity"
    L = len(ints)
    dz = [None] * L
    dz[L - 1] = dy.long()
    for l in range(L - 2, -1, -1):
        W = ints[l + 1][0]
        peak = max(peak, int((dz[l + 1].abs() @ W.abs()).max()))
        dz[l] = dz[l + 1] @ W
    peak = max(peak, int((dz[0].abs() @ ints[0][0].abs()).max()))
    dx = dz[0] @ ints[0][0]
    db = [d.sum(0) for d in dz]
    dW = [dz[l].T @ hs[l] for l in range(L)]
    for l in range(L):
        peak = max(peak, int(dz[l].abs().sum(0).max()), int((dz[l].abs().T @ hs[l].abs()).max()))
    return {"y": hs[-1], "h": hs[1:-1], "dz": dz[:-1], "dx": dx, "db": db, "dW": dW, "peak": peak}


@torch.no_grad()
def forward_fp64(lins, x):
    """([h64_l], [e_h_l]) for every hidden layer and (y64, e_y): fp64 of the fp32 parameters with the forward bound."""
    h, e = x.double(), torch.zeros_like(x, dtype=torch.float64)
    hs, es = [], []
    for i, lin in enumerate(lins):
        W, b = lin.weight.double(), lin.bias.double()
        K = W.shape[1]
        e = e @ W.abs().T + (K + 2) * U * (h.abs() @ W.abs().T + b.abs())
        h = h @ W.T + b
        if i + 1 < len(lins):
            h = torch.where(h > 0, h, torch.expm1(h))
            e = e + 4 * U * h.abs()
            hs.append(h), es.append(e)
    return hs, es, h, e


@torch.no_grad()
def backward_fp64(lins, x, hs, dy):
    """fp64 backward of the fp32 parameters, teacher-forced on the saved fp32 activations ``hs``, with the bounds of the
    module docstring.  Returns {"dz": [(ref, e)], "dx": (ref, e), "db": [(ref, e)], "dW": [(ref, e)]}."""
    L, n = len(lins), x.shape[0]
    Ws = [lin.weight.double() for lin in lins]
    acts = [x.double()] + [h.double() for h in hs]
    dz, ez = [None] * L, [None] * L
    dz[L - 1] = dy.double()
    ez[L - 1] = torch.zeros_like(dz[L - 1])
    for l in range(L - 2, -1, -1):
        W = Ws[l + 1]
        K = W.shape[0]
        dh = dz[l + 1] @ W
        eh = ez[l + 1] @ W.abs() + (K + 2) * U * (dz[l + 1].abs() @ W.abs())
        h = acts[l + 1]
        fp = torch.where(h > 0, torch.ones_like(h), h + 1)
        dz[l] = dh * fp
        ez[l] = fp * eh + 2 * U * fp * dh.abs()
    K = Ws[0].shape[0]
    dx = dz[0] @ Ws[0]
    ex = ez[0] @ Ws[0].abs() + (K + 2) * U * (dz[0].abs() @ Ws[0].abs())
    db = [(dz[l].sum(0), ez[l].sum(0) + (n + 2) * U * dz[l].abs().sum(0)) for l in range(L)]
    dW = [(dz[l].T @ acts[l], ez[l].T @ acts[l].abs() + (n + 2) * U * (dz[l].abs().T @ acts[l].abs()))
          for l in range(L)]
    return {"dz": list(zip(dz[:-1], ez[:-1])), "dx": (dx, ex), "db": db, "dW": dW}


def fraction(got, ref, e):
    """The worst |got - ref| / e over the elements; an element with e == 0 must be exact (inf otherwise)."""
    err = (got.double() - ref).abs()
    if not torch.isfinite(got).all():
        return float("inf")
    zero = e == 0
    if bool((err[zero] > 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / e[~zero]).max())
