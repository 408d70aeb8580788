"""Shared by tests/test_gpu_recurrent.py, tests/test_gpu_recurrent_edges.py and tests/test_lstm_reference.py (and
``make_norm`` by tests/test_gpu_policy.py): small (nn.LSTM, Linear/ELU) pairs, observation normalisers with planted
zero-variance columns, the fp64 reference of one fused LSTM step with its a-priori bound, and the torch fp32 path.
Every builder takes the device, so the reference itself is tested without a GPU.  U = 2^-24.

The bound (an fp32 evaluation of the same fp32 parameters, inputs and state against the fp64 one, elementwise):
    x_n  = (x - mean) / scale,   scale = sqrt(var + eps) (cleanrl.RunningMeanStd) | std + eps (ppo.EmpiricalNormalization)
    e_x  = 4 U (|x| + |mean|) / scale            (subtract, scale's add and sqrt, divide; 0 without a normaliser)
    e_z  = e_x |W_ih|^T + e_h |W_hh|^T + (K + 3) U (|x_n||W_ih|^T + |h||W_hh|^T + |b_ih| + |b_hh|),   K = d_in + H
           (a K + 1 term fmaf chain in any order, and the rounding of b_ih + b_hh at pack time)
    e_s  = e_z / 4 + 8 U s   for s = sigmoid(z)   (1/4-Lipschitz; expf within 2 ulp, one add, one true division)
    e_g  = e_z + 8 U |g|     for g = tanh(z)      (1-Lipschitz)
    e_c' = [f c] + [i g] + U |c'|,  [a b] = |a| e_b + |b| e_a + e_a e_b + U |a b|   (product rule, one rounding each)
    e_h' = [o tanh(c')],  e_tanh(c') = e_c' + 8 U |tanh(c')|
and e_h' feeds the MLP's bound of tests/test_gpu_policy.py:  e_z = |W| e_h + (K + 2) U (|W||h| + |b|),  e_h = e_z + 4 U |h|.
"""
import copy

import torch
import torch.nn as nn

U = 2.0 ** -24


def seq(dims):
    mods = []
    for i in range(len(dims) - 1):
        mods.append(nn.Linear(dims[i], dims[i + 1]))
        if i + 2 < len(dims):
            mods.append(nn.ELU())
    return nn.Sequential(*mods)


def make_pairs(shape, n_nets, seed, device="cuda"):
    """n_nets (nn.LSTM, MLP) pairs on ``device``; the second network's output is one column (a critic)."""
    d_in, H, hidden, d_out = shape
    torch.manual_seed(seed)
    pairs = []
    for i in range(n_nets):
        rnn, net = nn.LSTM(d_in, H), seq([H] + hidden + [d_out if i == 0 else 1])
        for p in list(rnn.parameters()) + list(net.parameters()):
            if p.dim() == 1:
                nn.init.normal_(p, std=0.3)
        pairs.append((rnn.to(device).requires_grad_(False), net.to(device).requires_grad_(False)))
    return pairs


def make_inputs(shape, n, n_nets, seed, device="cuda"):
    d_in, H, _, _ = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d_in, generator=g).to(device)
    states = [(torch.tanh(torch.randn(n, H, generator=g)).to(device), (1.5 * torch.randn(n, H, generator=g)).to(device))
              for _ in range(n_nets)]
    return x, states


def clone_states(states):
    return [(h.clone(), c.clone()) for h, c in states]


# ---------------------------------------------------------------------------------------------- normalisers
def make_norm(kind, d_in, seed, device="cuda"):
    """"none": None; "var": cleanrl.RunningMeanStd; "std": ppo.EmpiricalNormalization in eval mode."""
    from h12env.cleanrl import RunningMeanStd
    from h12env.ppo import EmpiricalNormalization

    if kind == "none":
        return None
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(d_in, generator=g) * 3
    var = torch.rand(d_in, generator=g) * 4 + 0.05
    if kind == "var":
        m = RunningMeanStd(shape=(d_in,))
        m.running_mean.copy_(mean), m.running_var.copy_(var)
    else:
        m = EmpiricalNormalization([d_in]).eval()
        m._mean.copy_(mean[None]), m._var.copy_(var[None]), m._std.copy_(var.sqrt()[None])
    return m.to(device)


def planted_columns(d_in):
    """The first, the last and one inside (fewer where d_in has fewer)."""
    return sorted({0, d_in // 2, d_in - 1})


def is_var_kind(norm):
    return hasattr(norm, "running_mean")


def make_planted_norm(kind, d_in, seed, device="cuda", planted=True):
    """``make_norm`` with the variance of ``planted_columns`` set to exactly 0: there the scale is sqrt(eps) = 1e-4
    (var) or eps = 1e-2 (std), which is what tells the two placements of eps apart."""
    m = make_norm(kind, d_in, seed, device)
    if m is not None and planted:
        cols = planted_columns(d_in)
        if is_var_kind(m):
            m.running_var[cols] = 0.0
        else:
            m._var[0, cols] = 0.0
            m._std[0, cols] = 0.0
    return m


def make_norm_x(n, d_in, norm, seed, device="cuda", planted=True):
    """x [n][d_in] around the normaliser's mean (N(0,1) without one); in the planted columns within +-1e-4 (var) or
    +-1e-2 (std) of the mean, so the normalised value stays within about +-1 there."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d_in, generator=g)
    if norm is None:
        return x.to(device)
    mean = (norm.running_mean if is_var_kind(norm) else norm._mean).reshape(-1).cpu()
    x = x * 2 + mean
    if planted:
        amp = 1e-4 if is_var_kind(norm) else 1e-2
        for c in planted_columns(d_in):
            x[:, c] = mean[c] + amp * (2 * torch.rand(n, generator=g) - 1)
    return x.to(device)


def norm_stats(norm):
    """(mean, scale) in fp64 as the module's own forward defines them."""
    if is_var_kind(norm):
        return norm.running_mean.double().reshape(-1), torch.sqrt(norm.running_var.double().reshape(-1) + norm.epsilon)
    return norm._mean.double().reshape(-1), norm._std.double().reshape(-1) + norm.eps


@torch.no_grad()
def normalise_torch(norm, x):
    """The normaliser module itself in fp32 on the CPU, statistics frozen (eval mode / update=False)."""
    m = copy.deepcopy(norm).cpu().eval()
    x = x.cpu()
    return m(x, update=False) if is_var_kind(m) else m(x)


# ---------------------------------------------------------------------------------------------- references
@torch.no_grad()
def lstm_fp64_with_bound(rnn, net, x, h, c, eh=None, ec=None, norm=None):
    """(y, h', c') in fp64 from the fp32 parameters of ``rnn`` / ``net``, the statistics of ``norm`` (None: x is read
    as it is) and the inputs x, h, c, and the a-priori bounds (e_y, e_h', e_c') of an fp32 evaluation whose incoming
    state is within (eh, ec) of (h, c).  The module docstring has the formulae."""
    x, h, c = x.double(), h.double(), c.double()
    eh = torch.zeros_like(h) if eh is None else eh
    ec = torch.zeros_like(c) if ec is None else ec
    ex = torch.zeros_like(x)
    if norm is not None:
        mean, scale = (t.to(x.device) for t in norm_stats(norm))
        ex = 4 * U * (x.abs() + mean.abs()) / scale
        x = (x - mean) / scale
    W_ih, W_hh = rnn.weight_ih_l0.double(), rnn.weight_hh_l0.double()
    b_ih, b_hh = rnn.bias_ih_l0.double(), rnn.bias_hh_l0.double()
    H = W_hh.shape[1]
    K = W_ih.shape[1] + H
    z = x @ W_ih.T + h @ W_hh.T + b_ih + b_hh
    ez = (ex @ W_ih.abs().T + eh @ W_hh.abs().T
          + (K + 3) * U * (x.abs() @ W_ih.abs().T + h.abs() @ W_hh.abs().T + b_ih.abs() + b_hh.abs()))
    zi, zf, zg, zo = z.split(H, dim=1)
    ei, ef, eg, eo = ez.split(H, dim=1)
    i, f, g, o = torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)
    ei, ef, eo = ei / 4 + 8 * U * i, ef / 4 + 8 * U * f, eo / 4 + 8 * U * o
    eg = eg + 8 * U * g.abs()

    def prod(a, ea, b, eb):
        return a.abs() * eb + b.abs() * ea + ea * eb + U * (a * b).abs()

    c2 = f * c + i * g
    ec2 = prod(f, ef, c, ec) + prod(i, ei, g, eg) + U * c2.abs()
    t = torch.tanh(c2)
    et = ec2 + 8 * U * t.abs()
    h2 = o * t
    eh2 = prod(o, eo, t, et)
    y, e = h2, eh2
    lins = [m for m in net if isinstance(m, nn.Linear)]
    for k, lin in enumerate(lins):  # the bound of tests/test_gpu_policy.py
        W, b = lin.weight.double(), lin.bias.double()
        e = e @ W.abs().T + (W.shape[1] + 2) * U * (y.abs() @ W.abs().T + b.abs())
        y = y @ W.T + b
        if k + 1 < len(lins):
            y = torch.where(y > 0, y, torch.expm1(y))
            e = e + 4 * U * y.abs()
    return (y, h2, c2), (e, eh2, ec2)


@torch.no_grad()
def torch_cpu(rnn, net, x, h, c, norm=None):
    """The normaliser module (eval mode), torch.nn.LSTM and the MLP on the CPU in fp32."""
    r = nn.LSTM(rnn.input_size, rnn.hidden_size)
    r.load_state_dict({k: v.cpu() for k, v in rnn.state_dict().items()})
    m = copy.deepcopy(net).cpu()
    x = x.cpu() if norm is None else normalise_torch(norm, x)
    out, (h2, c2) = r(x.unsqueeze(0), (h.cpu().unsqueeze(0), c.cpu().unsqueeze(0)))
    return m(out[0]), h2[0], c2[0]


MISTAKES = ("eps_other_side", "other_kind", "mean_shifted", "eps_dropped", "gates_f_g")


@torch.no_grad()
def torch_cpu_with_mistake(rnn, net, x, h, c, norm, mistake):
    """``torch_cpu`` with one planted mistake of the kind a kernel could make: an fp32 evaluation that the bound of
    ``lstm_fp64_with_bound`` must reject."""
    assert mistake in MISTAKES, mistake
    x = x.cpu().float()
    var_kind = is_var_kind(norm)
    mean = (norm.running_mean if var_kind else norm._mean).cpu().reshape(-1).float()
    stat = (norm.running_var if var_kind else norm._std).cpu().reshape(-1).float()  # what the kernel is handed
    eps = torch.tensor(norm.epsilon if var_kind else norm.eps, dtype=torch.float32)
    right = torch.sqrt(stat + eps) if var_kind else stat + eps
    if mistake == "eps_other_side":
        scale = torch.sqrt(stat) + eps if var_kind else torch.sqrt(stat * stat + eps)
    elif mistake == "other_kind":
        scale = stat + eps if var_kind else torch.sqrt(stat + eps)
    elif mistake == "eps_dropped":
        scale = torch.sqrt(stat) if var_kind else stat
    else:
        scale = right
    if mistake == "mean_shifted":
        mean = torch.roll(mean, -1)  # column c reads mean[c + 1]
    xn = (x - mean) / scale
    r = nn.LSTM(rnn.input_size, rnn.hidden_size)
    sd = {k: v.cpu().clone() for k, v in rnn.state_dict().items()}
    if mistake == "gates_f_g":
        H = rnn.hidden_size
        for v in sd.values():
            f_rows = v[H:2 * H].clone()
            v[H:2 * H] = v[2 * H:3 * H]
            v[2 * H:3 * H] = f_rows
    r.load_state_dict(sd)
    m = copy.deepcopy(net).cpu()
    out, (h2, c2) = r(xn.unsqueeze(0), (h.cpu().unsqueeze(0), c.cpu().unsqueeze(0)))
    return m(out[0]), h2[0], c2[0]


def inside(got, ref, bound, factor=1.0):
    """(every element finite and |got - ref| <= factor * bound, the worst |got - ref| / (factor * bound)).  The first
    is the assertion: compared with <=, so an element whose bound is exactly 0 must be exact; the second is for the
    log, taken over the elements with a non-zero bound (inf where the first fails on a zero bound or a non-finite)."""
    got, ref, bound = got.detach().double().cpu(), ref.detach().double().cpu(), factor * bound.detach().double().cpu()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    ok = bool(torch.isfinite(got).all()) and bool((err <= bound).all())
    nz = bound > 0
    worst = float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0
    if not ok and not worst > 1.0:
        worst = float("inf")
    return ok, worst
