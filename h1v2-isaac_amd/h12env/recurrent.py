"""Memory for the PPO runner's recurrent policy (rsl_rl 2.3 modules/actor_critic_recurrent.py and utils, restated):
``Memory`` wraps a time-major nn.LSTM / nn.GRU that is stepped during collection and run over padded trajectories in
the update; ``split_and_pad_trajectories`` / ``unpad_trajectories`` cut a (T, N, ...) rollout at its dones and back."""
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

    def forward(self, input, masks=None, hidden_states=None):
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
