"""HIP-graph capture for the trainers: the one place in the package that builds a ``torch.cuda.CUDAGraph``.

    graph, out = capture(body, device, undo=[state_tensor, TrainingState(params, optimizer, [lr_t])], rng=True)
    static_input.copy_(x);  graph.replay()          # ``out`` is overwritten by every replay

The rule every "graph equals eager" test rests on lives here: whatever the warm-up changed is put back bit for bit
before the capture, so the first replay starts exactly where the first eager call would.  The callers keep what
differs between them: the key of a graph, where the graphs are stored, the static input buffers."""
from __future__ import annotations

import os

import torch


def graph_enabled() -> bool:
    """H12_PPO_GRAPH=0 turns every captured body of both trainers into its eager run.  Each caller adds its own
    conditions (ppo: CUDA, a device learning rate, one rank; cleanrl: the HIP normaliser; a recurrent policy: fused
    collection)."""
    return os.environ.get("H12_PPO_GRAPH", "1") != "0"


class TrainingState:
    """Parameters, the tensor entries of ``optimizer.state`` and ``extra`` tensors (a device learning rate, statistics)
    as they are at construction; ``restore()`` copies them back in place."""

    def __init__(self, params, optimizer, extra=()):
        self.params, self.optimizer = list(params), optimizer
        self.tensors = self.params + list(extra)
        self._saved = [t.detach().clone() for t in self.tensors]
        self._opt = {p: {k: v.detach().clone() for k, v in optimizer.state.get(p, {}).items() if torch.is_tensor(v)}
                     for p in self.params}

    def restore(self):
        with torch.no_grad():
            for t, v in zip(self.tensors, self._saved):
                t.copy_(v)
            for p in self.params:
                for k, v in self.optimizer.state.get(p, {}).items():
                    if torch.is_tensor(v):
                        v.copy_(self._opt[p][k]) if k in self._opt[p] else v.zero_()  # lazily created since: initial 0


def capture(body, device, *, undo=(), rng=False, before_capture=None):
    """Capture ``body()`` as a HIP graph; returns ``(graph, body's outputs)``.

    1. ``body()`` runs twice on a side stream that waits on the current one (first launches load code objects, raise
       LDS limits and let libraries pick algorithms, none of which can happen under a capture); the streams are joined.
    2. Everything in ``undo`` is put back: a tensor is cloned on entry and copied back, any other object has its
       ``restore()`` called (``TrainingState``).
    3. ``before_capture()`` runs, if given (dropping gradients, so that the captured backward writes them).
    4. ``body()`` is captured once.
    5. ``rng``: the device generator's state is put back as it was on entry, because warm-up and capture consume
       draws: the replays then draw the sequence the eager path would draw.

    The state is restored at one point only, between warm-up and capture.  A capture launches nothing, so this is
    equivalent to restoring after it.  Grad mode and inference mode are the caller's, as for an eager ``body()``."""
    rng_state = torch.cuda.get_rng_state(device) if rng else None
    kept = [(t, t.clone()) if torch.is_tensor(t) else (t, None) for t in undo]
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        for _ in range(2):
            body()
    torch.cuda.current_stream(device).wait_stream(s)
    for t, v in kept:
        t.restore() if v is None else t.copy_(v)
    if before_capture is not None:
        before_capture()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = body()
    if rng:
        torch.cuda.set_rng_state(rng_state, device)
    return g, out
