"""Memory for the PPO runner's recurrent policy (rsl_rl 2.3 modules/actor_critic_recurrent.py and utils, restated):
``Memory`` wraps a time-major nn.LSTM / nn.GRU that is stepped during collection and run over padded trajectories in
the update; ``split_and_pad_trajectories`` / ``unpad_trajectories`` cut a (T, N, ...) rollout at its dones and back.

``lstm_sequence`` is the update's other form: the memory over the whole [T, N] rollout, reading a
zero state wherever the previous step was a done.  It gives what the padded trajectories give at every (t, env), has
fixed shapes and no host sync, and runs on the h12learn_lstm_seq_* kernels on the GPU."""
from __future__ import annotations

import torch
import torch.nn as nn


def split_and_pad_trajectories(tensor: torch.Tensor, dones: torch.Tensor):
    """(padded [T, n_traj, ...], masks [T, n_traj]) of ``tensor`` [T, N, ...] cut at ``dones`` [T, N, 1].  A trajectory
    ends at a done and at step T - 1; trajectories are ordered env-major (all of env 0's, then env 1's, ...) and
    zero-padded to length T; masks is True on the real steps."""
    T = tensor.shape[0]
    ends = dones.reshape(T, -1).clone() != 0
    ends[-1] = True
    flat_ends = ends.transpose(0, 1).reshape(-1)  # env-major
    last = flat_ends.nonzero()[:, 0]
    lengths = last - torch.cat([last.new_tensor([-1]), last[:-1]])
    pieces = torch.split(tensor.transpose(0, 1).flatten(0, 1), lengths.tolist())
    # a full-length piece of zeros makes pad_sequence pad to T whatever the longest trajectory is
    pieces = pieces + (torch.zeros(T, *tensor.shape[2:], device=tensor.device, dtype=tensor.dtype),)
    padded = nn.utils.rnn.pad_sequence(pieces)[:, :-1]
    masks = lengths > torch.arange(T, device=tensor.device).unsqueeze(1)
    return padded, masks


def unpad_trajectories(trajectories: torch.Tensor, masks: torch.Tensor) -> torch.Tensor:
    """The inverse of split_and_pad_trajectories: [T, N, ...] from the padded trajectories and their masks."""
    T = trajectories.shape[0]
    flat = trajectories.transpose(0, 1)[masks.transpose(0, 1)]  # env-major, every env exactly T real steps
    return flat.view(-1, T, *trajectories.shape[2:]).transpose(0, 1)


class Memory(nn.Module):
    """rsl_rl's Memory.  Step mode (``masks is None``) advances ``hidden_states`` by one step of ``input`` [N, d];
    batch mode runs the padded trajectories ``input`` [T, n_traj, d] from ``hidden_states`` and un-pads the output.

    ``keep_storage`` (not rsl_rl's): step mode then copies the new state into the existing state tensors instead of
    rebinding them, so a captured graph that updates the state in place keeps valid pointers."""

    def __init__(self, input_size: int, type: str = "lstm", num_layers: int = 1, hidden_size: int = 256):
        super().__init__()
        kinds = {"lstm": nn.LSTM, "gru": nn.GRU}
        if type.lower() not in kinds:
            raise ValueError(f"unknown rnn_type {type!r} (lstm or gru)")
        self.rnn = kinds[type.lower()](input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        self.hidden_states = None
        self.keep_storage = False

    def forward(self, input, masks=None, hidden_states=None, dones=None):
        if dones is not None:  # sequence mode: [T, N, d] with the state zeroed after a done, no padding
            if masks is not None:
                raise ValueError("masks (padded trajectories) and dones (the [T, N] sequence form) are mutually exclusive")
            if hidden_states is None:
                raise ValueError("Hidden states not passed to memory module during policy update")
            return lstm_sequence(self.rnn, input, dones, hidden_states)
        if masks is not None:
            if hidden_states is None:
                raise ValueError("Hidden states not passed to memory module during policy update")
            out, _ = self.rnn(input, hidden_states)
            return unpad_trajectories(out, masks)
        out, new = self.rnn(input.unsqueeze(0), self.hidden_states)
        if self.keep_storage and self.hidden_states is not None:
            for dst, src in zip(state_tensors(self.hidden_states), state_tensors(new)):
                dst.copy_(src)
        else:
            self.hidden_states = new
        return out

    def reset(self, dones=None, hidden_states=None):
        if dones is None:
            self.hidden_states = hidden_states
        elif self.hidden_states is not None:
            for s in state_tensors(self.hidden_states):
                s[..., dones == 1, :] = 0.0


def state_tensors(hidden_states) -> tuple:
    """The state tensors of an LSTM's (h, c) or a GRU's h."""
    return tuple(hidden_states) if isinstance(hidden_states, (tuple, list)) else (hidden_states,)


# ---------------------------------------------------------------------------------------------- sequence form
SEQ_MAX_HIDDEN = 256  # h12learn_lstm_max_hidden()


def lstm_sequence_limit(rnn: nn.Module) -> str | None:
    """Why the h12learn_lstm_seq_* kernels cannot run ``rnn`` (None: they can): a one-layer fp32 nn.LSTM of at most
    SEQ_MAX_HIDDEN units."""
    if not isinstance(rnn, nn.LSTM):
        return f"{type(rnn).__name__}: the sequence kernels are LSTM only"
    if rnn.num_layers != 1 or rnn.bidirectional or rnn.proj_size != 0 or not rnn.bias:
        return (f"num_layers = {rnn.num_layers}: the sequence kernels run one unidirectional layer with biases, no "
                "projection")
    if rnn.hidden_size > SEQ_MAX_HIDDEN:
        return f"hidden size {rnn.hidden_size}: the sequence kernels support at most {SEQ_MAX_HIDDEN}"
    if rnn.weight_hh_l0.dtype != torch.float32:
        return f"weights of {rnn.weight_hh_l0.dtype}: the sequence kernels are float32"
    return None


def _resets(dones: torch.Tensor, T: int, N: int) -> torch.Tensor:
    """reset [T, N] (bool): step t reads a zero state where dones[t - 1] != 0; t = 0 never does, dones[T - 1] is not read."""
    d = dones.reshape(T, N) != 0
    return torch.cat([torch.zeros_like(d[:1]), d[:-1]])


def lstm_sequence_torch(rnn: nn.Module, x: torch.Tensor, dones: torch.Tensor, hidden_states) -> torch.Tensor:
    """The definition, as a torch loop over t: ``rnn`` (any nn.LSTM / nn.GRU) stepped over x [T, N, d] from
    ``hidden_states`` ([layers, N, H] per state tensor), the state set to zero before step t wherever dones[t - 1] != 0.
    At every (t, env) this is what split_and_pad_trajectories -> rnn -> unpad_trajectories gives."""
    return _sequence_loop(rnn, x, dones, hidden_states)[0]


def _sequence_loop(rnn: nn.Module, x: torch.Tensor, dones: torch.Tensor, hidden_states):
    """lstm_sequence_torch's loop: (the outputs [T, N, H], the state after the last step, in the module's layout)."""
    T, N = x.shape[:2]
    keep = (~_resets(dones, T, N)).to(x.dtype)[:, None, :, None]  # [T, 1, N, 1]
    state = hidden_states
    out = []
    for t in range(T):
        if t > 0:
            state = tuple(s * keep[t] for s in state) if isinstance(state, (tuple, list)) else state * keep[t]
        y, state = rnn(x[t:t + 1], state)
        out.append(y)
    return torch.cat(out), state


class _LstmSeq(torch.autograd.Function):
    """lstm_sequence of 1..2 networks over the same dones as one node: the projection GEMM, h12learn_lstm_seq_forward,
    and in the backward h12learn_lstm_seq_backward and the weight-gradient GEMMs.  Arguments: dones ([T, N] bytes), then
    per network x [T, N, d], h0, c0 [N, H], weight_ih, weight_hh, bias_ih, bias_hh.  Returns the h_seq [T, N, H]."""

    PER_NET = 7

    @staticmethod
    def forward(ctx, dones, *flat):
        hs, _ = _LstmSeq._run(ctx, dones, *flat)
        return hs if len(hs) > 1 else hs[0]

    @staticmethod
    def _run(ctx, dones, *flat):
        """The forward: (the h_seq of every network, what h12learn_lstm_seq_forward returned per network)."""
        from . import _learn

        nets = [flat[i:i + _LstmSeq.PER_NET] for i in range(0, len(flat), _LstmSeq.PER_NET)]
        T, N = nets[0][0].shape[:2]
        desc = _learn.lstm_seq_desc([n[4].detach().contiguous() for n in nets])
        packed = torch.empty(_learn.lstm_seq_packed_bytes(desc) // 4, dtype=torch.float32, device=dones.device)
        _learn.lstm_seq_pack(desc, packed)  # once per call, for both networks
        xs = [n[0].detach().reshape(T * N, -1) for n in nets]
        zxs = [torch.addmm(n[5].detach() + n[6].detach(), x, n[3].detach().t()).view(T, N, -1)
               for n, x in zip(nets, xs)]
        h0s = [n[1].detach().contiguous() for n in nets]
        c0s = [n[2].detach().contiguous() for n in nets]
        out = _learn.lstm_seq_forward(desc, packed, zxs, dones, h0s, c0s)
        ctx.desc, ctx.packed, ctx.dones, ctx.n_nets = desc, packed, dones, len(nets)
        ctx.save_for_backward(*[t for i, n in enumerate(nets)
                                for t in (xs[i], h0s[i], c0s[i], n[3], out[i][0], out[i][1], out[i][2])])
        return tuple(o[0] for o in out), out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *dhs):
        from . import _learn

        saved = ctx.saved_tensors
        nets = [saved[i:i + 7] for i in range(0, len(saved), 7)]  # x, h0, c0, w_ih, h_seq, c_seq, gates
        T, N, H = nets[0][4].shape
        need = ctx.needs_input_grad
        need_state = any(need[1 + _LstmSeq.PER_NET * i + k] for i in range(ctx.n_nets) for k in (1, 2))
        dhs = [torch.zeros_like(n[4]) if g is None else g.contiguous() for g, n in zip(dhs, nets)]
        grads = _learn.lstm_seq_backward(ctx.desc, ctx.packed, dhs, [(n[5], n[6]) for n in nets], ctx.dones,
                                         [n[2] for n in nets], need_state_grads=need_state)
        keep = (~_resets(ctx.dones, T, N)).to(torch.float32).unsqueeze(-1)
        res = [None]
        for i, ((x, h0, c0, w_ih, h_seq, c_seq, gates), (dz, dh0, dc0)) in enumerate(zip(nets, grads)):
            base = 1 + _LstmSeq.PER_NET * i
            dz2 = dz.view(T * N, 4 * H)
            h_prev = (torch.cat([h0.unsqueeze(0), h_seq[:-1]]) * keep).view(T * N, H)
            db = dz2.sum(0)
            res += [(dz2 @ w_ih).view(T, N, -1) if need[base] else None,
                    dh0 if need[base + 1] else None, dc0 if need[base + 2] else None,
                    dz2.t() @ x, dz2.t() @ h_prev, db, db]
        return tuple(res)


class _LstmSeqState(_LstmSeq):
    """_LstmSeq of one network that also returns c after the last step, [N, H], as a non-differentiable output: with
    h_seq[-1] it is the state a following chunk of the sequence starts from (truncated BPTT detaches it anyway)."""

    @staticmethod
    def forward(ctx, dones, *flat):
        (h_seq,), out = _LstmSeq._run(ctx, dones, *flat)
        c_last = out[0][1][-1].clone()  # c_seq's last step: a copy, so that nothing holds a view of the saved tensor
        ctx.mark_non_differentiable(c_last)
        return h_seq, c_last

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dh, _dc_last):
        return _LstmSeq.backward(ctx, dh)


def _as_seq_args(rnn, x, hidden_states):
    h0, c0 = hidden_states
    return (x, h0.reshape(-1, rnn.hidden_size), c0.reshape(-1, rnn.hidden_size), rnn.weight_ih_l0, rnn.weight_hh_l0,
            rnn.bias_ih_l0, rnn.bias_hh_l0)


def _seq_dones(dones: torch.Tensor, T: int, N: int) -> torch.Tensor:
    d = dones.reshape(T, N)
    return (d if d.dtype == torch.uint8 else (d != 0).to(torch.uint8)).contiguous()


def _kernels_admitted(rnn, x) -> bool:
    return x.is_cuda and x.dtype == torch.float32 and lstm_sequence_limit(rnn) is None


def lstm_sequence(rnn: nn.Module, x: torch.Tensor, dones: torch.Tensor, hidden_states) -> torch.Tensor:
    """h_seq [T, N, H] of ``rnn`` over x [T, N, d], reading a zero state at step t wherever dones[t - 1, n] != 0, from
    ``hidden_states`` = (h0, c0), [layers, N, H] each as the module takes them.  On CUDA, for a one-layer fp32 nn.LSTM of at most SEQ_MAX_HIDDEN
    units, one autograd node on the h12learn_lstm_seq_* kernels (fixed shapes, no host sync); otherwise
    lstm_sequence_torch, the same definition as a torch loop."""
    if not _kernels_admitted(rnn, x):
        return lstm_sequence_torch(rnn, x, dones, hidden_states)
    T, N = x.shape[:2]
    return _LstmSeq.apply(_seq_dones(dones, T, N), *_as_seq_args(rnn, x, hidden_states))


def lstm_sequence_pair(rnns, xs, dones: torch.Tensor, hidden_states) -> tuple:
    """lstm_sequence of two memories (the actor's and the critic's) over the same dones.  When both are admitted and
    have the same hidden size they share one pack launch and one launch of each kernel; otherwise two lstm_sequence
    calls."""
    (ra, rc), (xa, xc) = rnns, xs
    if not (_kernels_admitted(ra, xa) and _kernels_admitted(rc, xc) and ra.hidden_size == rc.hidden_size
            and xa.shape[:2] == xc.shape[:2]):
        return tuple(lstm_sequence(r, x, dones, h) for r, x, h in zip(rnns, xs, hidden_states))
    T, N = xa.shape[:2]
    return _LstmSeq.apply(_seq_dones(dones, T, N), *_as_seq_args(ra, xa, hidden_states[0]),
                          *_as_seq_args(rc, xc, hidden_states[1]))


def lstm_sequence_state(rnn: nn.Module, x: torch.Tensor, dones: torch.Tensor, hidden_states, kernels: bool = True):
    """(h_seq, state after the last step) of lstm_sequence: the form a sequence that is cut into chunks needs, each chunk
    starting from the state the previous one ended with.  The returned state is in the module's layout ((h, c) or h,
    [layers, N, H]); dones[T - 1] is not applied to it -- the caller zeroes the rows that ended on the last step.
    ``kernels`` False keeps the library rnn (the torch loop of the definition) even where the h12learn_lstm_seq_*
    kernels could run; on them the state is detached (c after the last step is a by-product of the forward)."""
    T, N = x.shape[:2]
    if kernels and _kernels_admitted(rnn, x):
        h_seq, c_last = _LstmSeqState.apply(_seq_dones(dones, T, N), *_as_seq_args(rnn, x, hidden_states))
        return h_seq, (h_seq[-1].detach().unsqueeze(0), c_last.unsqueeze(0))
    return _sequence_loop(rnn, x, dones, hidden_states)
