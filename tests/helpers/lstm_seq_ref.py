"""Shared by tests/test_recurrent_sequence.py and tests/test_gpu_recurrent_sequence.py: references of the LSTM sequence
form (an LSTM over [T, N] that reads a zero state at step t wherever dones[t - 1] != 0).

  planted_dones         a done at t = 0, two consecutive dones, a done at T - 1 (each on another env where N allows)
  seq_fp64_with_bound   the forward in fp64 with the a-priori bound of lstm_ref.lstm_fp64_with_bound chained over the T
                        steps through its (eh, ec) arguments, resets applied to the state and to its bound; the gates'
                        bounds restate that helper's e_z / e_s / e_g formulae (it does not return them)
  seq_grads             the definition as a torch loop in a given dtype with every gradient the kernels and their GEMMs
                        produce (fp64: the reference; fp32 with ``mistake``: an emulation of a wrong kernel)
  library_padded_grads  the same gradients from the CPU fp32 nn.LSTM over split_and_pad_trajectories: the yardstick
  normalised_error      max |g - g64| / max |g64|
"""
import torch
import torch.nn as nn

from h12env.recurrent import split_and_pad_trajectories, unpad_trajectories
from lstm_ref import U, lstm_fp64_with_bound

GRADS = ("dz", "dW_ih", "dW_hh", "db_ih", "db_hh", "dh0", "dc0")
MISTAKES = ("reset_from_dones_t", "c_not_reset", "gates_f_g")


def planted_dones(T, N):
    d = torch.zeros(T, N)
    d[0, 0] = 1                       # a done at t = 0
    d[T - 1, 1 % N] = 1               # a done at T - 1
    t0 = max(0, T // 2 - 1)
    d[t0, 2 % N] = 1                  # two consecutive dones (one step apart where T allows)
    d[min(T - 1, t0 + 1), 2 % N] = 1
    return d


def make_dones(kind, T, N):
    return {"none": torch.zeros(T, N), "all": torch.ones(T, N), "planted": planted_dones(T, N)}[kind]


def make_case(T, N, d_in, H, seed):
    """(nn.LSTM on the CPU with N(0, 0.3) biases, x [T, N, d_in], h0, c0 [N, H], dh_seq [T, N, H]), all fp32."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    rnn = nn.LSTM(d_in, H)
    with torch.no_grad():
        for p in rnn.parameters():
            if p.dim() == 1:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    x = torch.randn(T, N, d_in, generator=g)
    h0 = torch.tanh(torch.randn(N, H, generator=g))
    c0 = 1.5 * torch.randn(N, H, generator=g)
    dh = torch.randn(T, N, H, generator=g)
    return rnn, x, h0, c0, dh


def resets(dones):
    d = dones != 0
    return torch.cat([torch.zeros_like(d[:1]), d[:-1]])


@torch.no_grad()
def seq_fp64_with_bound(rnn, x, dones, h0, c0):
    """{"h", "c", "gates"}: (fp64 value, bound) of h_seq, c_seq [T, N, H] and the activated gates [T, N, 4H]."""
    T, N = x.shape[:2]
    H = rnn.hidden_size
    rs = resets(dones)
    W_ih, W_hh = rnn.weight_ih_l0.double(), rnn.weight_hh_l0.double()
    b_ih, b_hh = rnn.bias_ih_l0.double(), rnn.bias_hh_l0.double()
    K = W_ih.shape[1] + H
    h, c = h0.double(), c0.double()
    eh, ec = torch.zeros_like(h), torch.zeros_like(c)
    out = {k: ([], []) for k in ("h", "c", "gates")}
    for t in range(T):
        keep = (~rs[t]).double()[:, None]
        h, c, eh, ec = h * keep, c * keep, eh * keep, ec * keep
        # the gates and their bounds: lstm_ref's module docstring, e_z, e_s, e_g
        xt = x[t].double()
        z = xt @ W_ih.T + h @ W_hh.T + b_ih + b_hh
        ez = eh @ W_hh.abs().T + (K + 3) * U * (xt.abs() @ W_ih.abs().T + h.abs() @ W_hh.abs().T + b_ih.abs()
                                                + b_hh.abs())
        zi, zf, zg, zo = z.split(H, dim=1)
        ei, ef, eg, eo = ez.split(H, dim=1)
        i, f, g, o = torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)
        out["gates"][0].append(torch.cat([i, f, g, o], 1))
        out["gates"][1].append(torch.cat([ei / 4 + 8 * U * i, ef / 4 + 8 * U * f, eg + 8 * U * g.abs(),
                                          eo / 4 + 8 * U * o], 1))
        (_, h2, c2), (_, eh2, ec2) = lstm_fp64_with_bound(rnn, nn.Sequential(), x[t], h, c, eh, ec)
        out["h"][0].append(h2), out["h"][1].append(eh2), out["c"][0].append(c2), out["c"][1].append(ec2)
        h, c, eh, ec = h2, c2, eh2, ec2
    return {k: (torch.stack(v), torch.stack(e)) for k, (v, e) in out.items()}


def seq_grads(rnn, x, dones, h0, c0, dh, dtype=torch.float64, mistake=None):
    """The definition as a torch loop in ``dtype``: {"h_seq", and every name of GRADS} for loss = sum(h_seq * dh).
    ``mistake``: one of MISTAKES, planted into the loop."""
    assert mistake is None or mistake in MISTAKES, mistake
    T, N = x.shape[:2]
    H = rnn.hidden_size
    W_ih, b_ih, b_hh = (p.detach().to(dtype) for p in (rnn.weight_ih_l0, rnn.bias_ih_l0, rnn.bias_hh_l0))
    W_hh = rnn.weight_hh_l0.detach().to(dtype).requires_grad_()
    x2 = x.to(dtype).reshape(T * N, -1)
    zx = (x2 @ W_ih.T + b_ih + b_hh).view(T, N, 4 * H).requires_grad_()
    h0, c0 = h0.to(dtype).clone().requires_grad_(), c0.to(dtype).clone().requires_grad_()
    d = (dones != 0).to(dtype)
    h, c = h0, c0
    hs = []
    for t in range(T):
        r = d[t] if mistake == "reset_from_dones_t" else (d[t - 1] if t > 0 else torch.zeros_like(d[0]))
        keep = (1 - r)[:, None]
        h = h * keep
        if mistake != "c_not_reset":
            c = c * keep
        z = zx[t] + h @ W_hh.T
        zi, zf, zg, zo = z.split(H, dim=1)
        if mistake == "gates_f_g":
            zf, zg = zg, zf
        i, f, g, o = torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs.append(h)
    h_seq = torch.stack(hs)
    (h_seq * dh.to(dtype)).sum().backward()
    dz2 = zx.grad.view(T * N, 4 * H)
    db = dz2.sum(0)
    return {"h_seq": h_seq.detach(), "dz": zx.grad, "dW_ih": dz2.T @ x2, "dW_hh": W_hh.grad, "db_ih": db, "db_hh": db,
            "dh0": h0.grad, "dc0": c0.grad}


def _padded_states(h0, c0, dones):
    """The padded form's start states ([1, n_traj, H] each, leaves) and the index of every env's first trajectory."""
    T, N = dones.shape
    starts = resets(dones)
    starts[0] = True
    per_env = starts.sum(0)
    first = torch.cat([per_env.new_zeros(1), per_env.cumsum(0)])
    n_traj = int(first[-1])
    at = first[:-1]
    hp, cp = (torch.zeros(1, n_traj, s.shape[1]).index_copy(1, at, s[None]).requires_grad_() for s in (h0, c0))
    return hp, cp, at


def library_padded_grads(rnn, x, dones, h0, c0, dh):
    """Every name of GRADS from the CPU fp32 library LSTM over the padded trajectories of ``dones``.  dz is the input
    gradient of a second run on the fp32 projection zx through an identity weight_ih with zero biases (products with 1
    and sums with 0 are exact, so that run's pre-activations are zx + h W_hh^T and its input gradient is dz)."""
    T, N = x.shape[:2]
    H = rnn.hidden_size
    lib = nn.LSTM(rnn.input_size, H)
    lib.load_state_dict(rnn.state_dict())
    d3 = dones[:, :, None]
    padded, masks = split_and_pad_trajectories(x, d3)
    hp, cp, at = _padded_states(h0, c0, dones)
    out, _ = lib(padded, (hp, cp))
    (unpad_trajectories(out, masks) * dh).sum().backward()
    res = {"dW_ih": lib.weight_ih_l0.grad, "dW_hh": lib.weight_hh_l0.grad, "db_ih": lib.bias_ih_l0.grad,
           "db_hh": lib.bias_hh_l0.grad, "dh0": hp.grad[0, at], "dc0": cp.grad[0, at]}
    eye = nn.LSTM(4 * H, H)
    with torch.no_grad():
        eye.weight_ih_l0.copy_(torch.eye(4 * H)), eye.weight_hh_l0.copy_(rnn.weight_hh_l0)
        eye.bias_ih_l0.zero_(), eye.bias_hh_l0.zero_()
        zx = torch.addmm(rnn.bias_ih_l0 + rnn.bias_hh_l0, x.reshape(T * N, -1), rnn.weight_ih_l0.T).view(T, N, 4 * H)
    zp = split_and_pad_trajectories(zx, d3)[0].requires_grad_()
    hp, cp, _ = _padded_states(h0, c0, dones)
    out, _ = eye(zp, (hp, cp))
    (unpad_trajectories(out, masks) * dh).sum().backward()
    res["dz"] = unpad_trajectories(zp.grad, masks)
    return res


def normalised_error(g, g64):
    """max |g - g64| / max |g64|; a reference that is all zero asks for exact zeros (0.0, or inf)."""
    g, g64 = g.detach().double().cpu(), g64.detach().double().cpu()
    assert g.shape == g64.shape, (g.shape, g64.shape)
    top = float(g64.abs().max())
    err = float((g - g64).abs().max())
    if top == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / top


def worst_error(grads, ref):
    """(the largest normalised error over GRADS, per-tensor errors)."""
    per = {k: normalised_error(grads[k], ref[k]) for k in GRADS}
    return max(per.values()), per
