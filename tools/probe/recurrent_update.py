#!/usr/bin/env python3
"""Time the update of the recurrent policy (one whole PPO.update() of an ActorCriticRecurrent) at the Flat task's shape:
4096 envs x 24 steps, 450 observations, LSTM of 256, MLPs 512-256-128, 4 minibatches x 5 epochs, dones planted at the rate
of the task's time-outs (one per 1000 env steps).

    python tools/probe/recurrent_update.py [--envs 4096] [--steps 24] [--rounds 6] [--reps 3] [--out FILE]

Two arms in one process, alternating (the first call of every turn is dropped), each timed between two device events over
--reps calls; median and minimum over the rounds, in ms per update:
  library   the default path (= the parent's behaviour): trajectories cut at the dones on the host, nn.LSTM over them
  fused     PPO(fused_rnn_update=True): the sequence form on h12learn_lstm_seq_forward / _backward
Both arms update from the same rollout every time (update() leaves the storage's tensors in place) at a learning rate of
1e-6, so the parameters stay where they are; the time does not depend on the values.

Separately, at the minibatch shape (T, N = envs / 4), forward + backward of one memory, in us:
  seq_one / seq_two   lstm_sequence (pack, projection GEMM, both kernels, weight-gradient GEMMs) for one network and
                      lstm_sequence_pair for two
  library_padded      nn.LSTM over the padded trajectories of the same dones (padding done outside the timed window),
                      un-padded, backward; one network
  kernel_*            h12learn_lstm_seq_forward / _backward alone, two networks in one launch
"""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd"))
DONE_RATE = 1.0e-3  # episode_length_s 20 / step_dt 0.02


def timed(fn, reps: int) -> float:
    """ms per call: one dropped call, then ``reps`` calls between two device events."""
    import torch

    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(v, scale=1.0):
    return {"median": scale * statistics.median(v), "min": scale * min(v), "samples": len(v)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import torch

    from h12env import _learn
    from h12env import recurrent as R
    from h12env.ppo import PPO, ActorCriticRecurrent

    if not torch.cuda.is_available():
        raise SystemExit("recurrent_update: no GPU (a timing needs the MI355X)")
    dev = "cuda:0"
    N, T, d, H = args.envs, args.steps, 450, 256
    torch.manual_seed(0)
    base = ActorCriticRecurrent(d, d, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128],
                                rnn_hidden_dim=H)
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(T + 1, N, d, generator=g).to(dev)
    dones = (torch.rand(T, N, generator=g) < DONE_RATE).float().to(dev)
    rewards = torch.randn(T, N, generator=g).to(dev)

    def make(fused: bool):
        alg = PPO(copy.deepcopy(base), num_learning_epochs=5, num_mini_batches=4, learning_rate=1e-6, schedule="fixed",
                  device=dev, fused_rnn_update=fused)
        alg.init_storage(N, T, [d], None, [12])
        torch.manual_seed(2)
        with torch.no_grad():
            alg.policy.act(obs[T]), alg.policy.evaluate(obs[T])  # the t = 0 states are not zero
            for t in range(T):
                alg.act(obs[t], obs[t])
                alg.process_env_step(rewards[t], dones[t], {})
            alg.compute_returns(obs[T])
        return alg

    algs = {"library": make(False), "fused": make(True)}
    for alg in algs.values():
        alg.update()
    torch.cuda.synchronize()
    samples = {k: [] for k in algs}
    for _ in range(args.rounds):
        for k, alg in algs.items():
            samples[k].append(timed(alg.update, args.reps))
    result = {"update_ms": {k: summary(v) for k, v in samples.items()}, "envs": N, "steps": T,
              "dones_in_rollout": int(dones.sum()), "minibatches": 4, "epochs": 5}

    # one memory at the minibatch shape
    n = N // 4
    rnns = [copy.deepcopy(base.memory_a.rnn).to(dev), copy.deepcopy(base.memory_c.rnn).to(dev)]
    x = obs[:T, :n].contiguous()
    dn = dones[:, :n].contiguous()
    d8 = (dn != 0).to(torch.uint8)
    w = torch.randn(T, n, H, device=dev)
    state = tuple(torch.tanh(torch.randn(1, n, H, device=dev)) for _ in range(2))
    padded, masks = R.split_and_pad_trajectories(x, dn[:, :, None])
    starts = torch.cat([torch.ones(1, n, device=dev), dn[:-1]]) != 0
    at = (torch.cat([starts.sum(0).new_zeros(1), starts.sum(0).cumsum(0)])[:-1])
    hidden = tuple(torch.zeros(1, masks.shape[1], H, device=dev).index_copy(1, at, s) for s in state)

    def grads_off():
        for m in rnns:
            m.zero_grad(set_to_none=True)

    def seq_one():
        grads_off()
        (R.lstm_sequence(rnns[0], x, d8, state) * w).sum().backward()

    def seq_two():
        grads_off()
        a, c = R.lstm_sequence_pair(rnns, (x, x), d8, (state, state))
        ((a + c) * w).sum().backward()

    def library_padded():
        grads_off()
        out, _ = rnns[0](padded, hidden)
        (R.unpad_trajectories(out, masks) * w).sum().backward()

    desc = _learn.lstm_seq_desc([m.weight_hh_l0.detach() for m in rnns])
    packed = torch.empty(_learn.lstm_seq_packed_bytes(desc) // 4, device=dev)
    _learn.lstm_seq_pack(desc, packed)
    zxs = [torch.randn(T, n, 4 * H, device=dev) for _ in rnns]
    h0s, c0s = [state[0][0].contiguous()] * 2, [state[1][0].contiguous()] * 2
    fwd = _learn.lstm_seq_forward(desc, packed, zxs, d8, h0s, c0s)
    bwd = _learn.lstm_seq_backward(desc, packed, [w, w], [(o[1], o[2]) for o in fwd], d8, c0s)
    arms = {"seq_one": seq_one, "seq_two": seq_two, "library_padded": library_padded,
            "kernel_forward_two": lambda: _learn.lstm_seq_forward(desc, packed, zxs, d8, h0s, c0s, out=fwd),
            "kernel_backward_two": lambda: _learn.lstm_seq_backward(desc, packed, [w, w], [(o[1], o[2]) for o in fwd],
                                                                    d8, c0s, out=bwd)}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            samples[k].append(timed(fn, 10 * args.reps))
    result["memory_us"] = {k: summary(v, 1e3) for k, v in samples.items()}
    result["memory_shape"] = {"T": T, "N": n, "trajectories": int(masks.shape[1])}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
