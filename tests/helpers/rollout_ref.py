"""Test infrastructure for the compact rollout records (h12env.rollout, include/h12env.h "Rollout records"): numpy
restatements of the gathered-buffer layout and of the row rebuild, and a step-by-step CircularBuffer model of the
observation history (T/utils/history/circular_buffer.py:79-170 semantics, the same the oracle's history write is
pinned to by tests/golden/circular_buffer.npz: term-major rows, oldest slot first, the first push after a reset fills
every slot).

For the HIP rebuild itself (rollout_decode_kernel): ``plant`` builds gathered records from chosen frames and done
flags, ``decode_windowed`` restates the kernel's window algorithm (with one planted mistake on request), and
``DECODE_CASES`` / ``case_inputs`` are the shapes and inputs tests/test_gpu_rollout_decode.py runs on the GPU and
tests/test_rollout_emulation.py proves to bite on the CPU."""
from __future__ import annotations

import functools
import zlib

import numpy as np

FRAME = 45
TERM_DIMS = (3, 3, 3, 12, 12, 12)  # ang_vel, gravity, command, q - q0, qd, action


def chunk_len(c: int, T: int, G: int) -> int:
    return min(G, T - c * G)


def step_offset(r: int, s: int, n_shards: int, T: int, G: int, step_bytes: int) -> int:
    """Byte offset of shard r's step record s in the gathered buffer (chunk-major, then shard, then step)."""
    c = s // G
    return (c * G * n_shards + r * chunk_len(c, T, G) + (s - c * G)) * step_bytes


def pack_gathered(shard_records: list[np.ndarray], T: int, G: int, step_bytes: int) -> np.ndarray:
    """What the chunked all_gather_into_tensor calls produce from the shards' (T * step_bytes) uint8 records."""
    R = len(shard_records)
    out = np.zeros(R * T * step_bytes, np.uint8)
    for c in range((T + G - 1) // G):
        t0, gc = c * G, chunk_len(c, T, G)
        for r in range(R):
            a = step_offset(r, t0, R, T, G, step_bytes)
            out[a:a + gc * step_bytes] = shard_records[r][t0 * step_bytes:(t0 + gc) * step_bytes]
    return out


def unpack(gathered: np.ndarray, n_shards: int, n: int, T: int, G: int, off: list[int], step_bytes: int) -> dict:
    """Global (T, n_shards * n, ...) arrays of every section of the gathered records."""
    out = {"frames": np.zeros((T, n_shards * n, FRAME), np.float32), "actions": np.zeros((T, n_shards * n, 12), np.float32),
           "rewards": np.zeros((T, n_shards * n), np.float32), "terminated": np.zeros((T, n_shards * n), np.uint8),
           "truncated": np.zeros((T, n_shards * n), np.uint8)}
    for r in range(n_shards):
        for s in range(T):
            b = step_offset(r, s, n_shards, T, G, step_bytes)
            rec = gathered[b:b + step_bytes]
            g = slice(r * n, (r + 1) * n)
            out["frames"][s, g] = rec[off[0]:off[0] + 4 * n * FRAME].view(np.float32).reshape(n, FRAME)
            out["actions"][s, g] = rec[off[1]:off[1] + 4 * n * 12].view(np.float32).reshape(n, 12)
            out["rewards"][s, g] = rec[off[2]:off[2] + 4 * n].view(np.float32)
            out["terminated"][s, g] = rec[off[3]:off[3] + n]
            out["truncated"][s, g] = rec[off[4]:off[4] + n]
    return out


def _col_maps(H: int):
    """Per row column: frame component c, term width d, slot h (0 oldest)."""
    comp, width, slot = [], [], []
    c0 = 0
    for d in TERM_DIMS:
        for h in range(H):
            for k in range(d):
                comp.append(c0 + k)
                width.append(d)
                slot.append(h)
        c0 += d
    return np.array(comp), np.array(width), np.array(slot)


def decode_ref(frames: np.ndarray, done: np.ndarray, tail: np.ndarray, H: int) -> np.ndarray:
    """(T, N, 45H) rows from frames (T, N, 45), done (T, N) and the rows before step 0 (N, 45H): the closed form
    h12env_rollout_decode evaluates (slot h of row t = frame max(t - (H - 1 - h), last done <= t), else the tail's
    slot h + t + 1).  A pure gather: the rows take frames.dtype, so on uint32 views of the words (frames and tail
    alike) every bit pattern comes through -- NaN payloads, signed zeros, infinities, denormals."""
    T, N, _ = frames.shape
    comp, width, slot = _col_maps(H)
    cols = np.arange(FRAME * H)
    last = np.full((T, N), -1)
    cur = np.full(N, -1)
    for t in range(T):
        cur = np.where(done[t] != 0, t, cur)
        last[t] = cur
    out = np.zeros((T, N, FRAME * H), frames.dtype)
    for t in range(T):
        src = t - (H - 1 - slot)[None, :]                      # (1, C)
        src = np.maximum(src, last[t][:, None])                # (N, C)
        from_frame = src >= 0
        fr = frames[np.clip(src, 0, T - 1), np.arange(N)[:, None], comp[None, :]]
        tl = tail[np.arange(N)[:, None], np.clip(cols + (t + 1) * width, 0, FRAME * H - 1)[None, :]]
        out[t] = np.where(from_frame, fr, tl)
    return out


def history_model(frames: np.ndarray, done: np.ndarray, tail: np.ndarray, H: int) -> np.ndarray:
    """The same rows by pushing frames through a per-env CircularBuffer (term-major flattening), step by step."""
    T, N, _ = frames.shape
    bounds = np.cumsum((0,) + TERM_DIMS)
    hist = []  # per env: list of H frames, oldest first, rebuilt from the tail row
    for e in range(N):
        fr = np.zeros((H, FRAME), np.float32)
        col = 0
        for j, d in enumerate(TERM_DIMS):
            fr[:, bounds[j]:bounds[j + 1]] = tail[e, col:col + H * d].reshape(H, d)
            col += H * d
        hist.append([fr[h] for h in range(H)])
    out = np.zeros((T, N, FRAME * H), np.float32)
    for t in range(T):
        for e in range(N):
            f = frames[t, e]
            hist[e] = [f] * H if done[t, e] else hist[e][1:] + [f]
            b = np.stack(hist[e])
            out[t, e] = np.concatenate([b[:, bounds[j]:bounds[j + 1]].reshape(-1) for j in range(len(TERM_DIMS))])
    return out


# ---------------------------------------------------------------- planted records and the kernel's own algorithm
# rollout_decode_kernel's geometry (csrc/h12env.hip; tests/test_rollout_emulation.py reads the constexpr line and
# fails when these differ, because the cases below were chosen for them)
DEC_ENVS, DEC_BLOCK, DEC_WT, DEC_MAX_BLOCKS = 8, 256, 16, 96
NHIST = 10
DEC_FR = DEC_WT + NHIST - 1

SENTINEL = np.uint32(0xFFEDCBA9)   # what every output word holds before a decode
POISON = np.uint32(0xBAD0BAD0)     # what the stand-in reads where the kernel would read outside what it staged
U8_FILL = 0xA5                     # the records' padding bytes (non-zero: a flag read past n is a done)


def plant(frames, actions, rewards, terminated, truncated, n_shards: int, n: int, T: int, G: int, layout=None):
    """The gathered records (uint8) of n_shards shards of n envs from global (T, n_shards * n, ...) arrays: every
    shard's T step records in the library's own layout (h12env_rollout_layout), laid out as the chunked all-gathers
    do (pack_gathered).  frames / actions / rewards: any 4-byte dtype (the words are copied); flags: uint8.
    Returns (records, (section offsets, step bytes))."""
    if layout is None:
        from h12env.rollout import record_layout

        layout = record_layout(n)
    off, S = layout
    shards = []
    for r in range(n_shards):
        g = slice(r * n, (r + 1) * n)
        rec = np.full((T, S), U8_FILL, np.uint8)
        for i, (a, width) in enumerate(((frames, 4 * FRAME), (actions, 4 * 12), (rewards, 4), (terminated, 1),
                                        (truncated, 1))):
            rec[:, off[i]:off[i] + n * width] = np.ascontiguousarray(a[:, g]).view(np.uint8).reshape(T, n * width)
        shards.append(rec.reshape(-1))
    return pack_gathered(shards, T, G, S), (list(off), S)


# one planted mistake each (decode_windowed's mutant=)
MUTANTS = (
    "short_lead_in",        # 1: f0 = w0 - (H - 2): one lead-in frame too few is staged
    "done_in_window_rows",  # 2: the last done step is looked for over [w0, w1) instead of the staged [f0, w1)
    "no_clamp",             # 3: src is not raised to the last done step
    "tail_offset_t",        # 4: the tail slot is col + t * width
    "ignore_truncated",     # 5: only terminated resets
    "last_chunk_len_G",     # 6: dec_step addresses the short last chunk with length G
    "group_base_padded",    # 7: a group's global env base is shard * bps * DEC_ENVS + e0 (right only when 8 | n)
    "flags_without_e0",     # 8: every group reads the done flags of its shard's first group
)


def decode_windowed(records, n_shards: int, n: int, T: int, G: int, H: int, t0: int, t1: int, tail, out, layout,
                    mutant: str | None = None) -> None:
    """Rows [t0, t1) into out (T, n_shards * n, 45H), in place, the way rollout_decode_kernel computes them -- not
    the closed form: a grid of min(groups, DEC_MAX_BLOCKS) blocks striding over groups of DEC_ENVS envs of one shard
    (ne, g0), the group's tail rows staged once, windows of DEC_WT rows with the frames and done flags of steps
    [f0, w1) staged (f0 = max(0, w0 - (H - 1))), the last done step per row found over the staged steps only,
    src = max(src, last), the tail slot col + (t + 1) * width, and dec_step's chunk-major addressing with the short
    last chunk.  tail and out hold 4-byte words of any dtype.  Shared memory keeps its contents from window to
    window and group to group as it does in the kernel; a read the kernel would make outside what it staged (before
    s_fr, past the records, the tail or the output) reads or writes POISON slack instead, so a mutant cannot fault
    here.  mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    assert out.flags.c_contiguous and out.shape == (T, n_shards * n, FRAME * H)
    off, S = layout
    ROW, NG = FRAME * H, n_shards * n
    G = min(G, T)
    comp, width, slot = _col_maps(H)
    cols = np.arange(ROW)
    bps = (n + DEC_ENVS - 1) // DEC_ENVS
    groups = n_shards * bps
    nb = min(groups, DEC_MAX_BLOCKS)
    slack = np.full((n_shards * bps * DEC_ENVS + DEC_ENVS) * ROW, POISON, np.uint32)
    flat = np.concatenate([np.ascontiguousarray(out).reshape(-1).view(np.uint32), slack])
    tl = np.concatenate([np.ascontiguousarray(tail).reshape(-1).view(np.uint32), slack])
    rec = np.concatenate([records, np.full((n_shards * G + 1) * S, POISON & 0xFF, np.uint8)])

    def step(r, s):  # dec_step
        c = s // G
        gc = G if mutant == "last_chunk_len_G" else min(G, T - c * G)
        return (c * G * n_shards + r * gc + (s - c * G)) * S

    for block in range(nb):
        s_fr = np.full((1 + DEC_FR, DEC_ENVS, FRAME), POISON, np.uint32)  # row 0: the words before s_fr
        s_last = np.full((DEC_ENVS, DEC_WT), -1)
        for grp in range(block, groups, nb):
            shard, e0 = divmod(grp, bps)
            e0 *= DEC_ENVS
            ne = min(DEC_ENVS, n - e0)
            g0 = (shard * bps * DEC_ENVS if mutant == "group_base_padded" else shard * n) + e0
            env = np.arange(ne)[:, None]
            s_tail = tl[g0 * ROW:(g0 + ne) * ROW].reshape(ne, ROW).copy()
            for w0 in range(t0, t1, DEC_WT):
                w1 = min(w0 + DEC_WT, t1)
                f0 = max(0, w0 - (H - 2 if mutant == "short_lead_in" else H - 1))
                nf = w1 - f0
                assert nf <= DEC_FR
                dn = np.zeros((max(nf, 0), ne), np.uint8)
                for ts in range(nf):
                    b = step(shard, f0 + ts)
                    a = b + off[0] + e0 * FRAME * 4
                    s_fr[1 + ts, :ne] = rec[a:a + ne * FRAME * 4].view(np.uint32).reshape(ne, FRAME)
                    fe = 0 if mutant == "flags_without_e0" else e0
                    dn[ts] = rec[b + off[3] + fe:b + off[3] + fe + ne]
                    if mutant != "ignore_truncated":
                        dn[ts] |= rec[b + off[4] + fe:b + off[4] + fe + ne]
                last = np.full(ne, -1)
                for ts in range(nf):
                    s = f0 + ts
                    if not (mutant == "done_in_window_rows" and s < w0):
                        last = np.where(dn[ts] != 0, s, last)
                    if s >= w0:
                        s_last[:ne, s - w0] = last
                for t in range(w0, w1):
                    src = np.broadcast_to(t - (H - 1 - slot)[None, :], (ne, ROW))
                    if mutant != "no_clamp":
                        src = np.maximum(src, s_last[:ne, t - w0][:, None])
                    row = 1 + src - f0
                    if mutant is None:  # the kernel reads only what this window staged
                        assert ((src < 0) | ((row >= 1) & (row <= nf))).all()
                    fr = s_fr[np.clip(row, 0, DEC_FR), env, comp[None, :]]
                    k = t if mutant == "tail_offset_t" else t + 1
                    tv = s_tail[env, np.clip(cols + k * width, 0, ROW - 1)[None, :]]
                    d = (t * NG + g0) * ROW
                    flat[d:d + ne * ROW] = np.where(src >= 0, fr, tv).reshape(-1)
    out.reshape(-1).view(np.uint32)[:] = flat[:out.size]


# The shapes the HIP decode is run at (tests/test_gpu_rollout_decode.py), the smallest that reach each path:
#   A  the smallest call: every slot comes from the tail or the one frame
#   B  one call, two windows (16 + 8); groups of 8 envs and of 1
#   C  three windows; shard 1's rows start at global env 37, 4 bytes past a 16-byte boundary, so its scalar stores
#      sit beside shard 0's float4 stores in one launch
#   D  the Rsl history across three shards, G does not divide T (last chunk 6), one call per chunk as RolloutGather
#      issues them: single windows whose lead-in frames come from earlier chunks
#   E  99 groups on 96 blocks: blocks 0-2 run a second group after the __syncthreads(); each shard's last group has 5
#   F1..F10  every instantiated history, two windows (16 + 4) over four chunks (6, 6, 6, 2)
# calls: "whole" = one call for [0, T); "chunks" = one call per chunk of G steps
DECODE_CASES = {
    "A": dict(shards=1, n=1, T=1, G=1, H=10, calls="whole"),
    "B": dict(shards=1, n=9, T=24, G=24, H=10, calls="whole"),
    "C": dict(shards=2, n=37, T=41, G=41, H=10, calls="whole"),
    "D": dict(shards=3, n=12, T=41, G=7, H=6, calls="chunks"),
    "E": dict(shards=3, n=261, T=17, G=17, H=10, calls="whole"),
    **{f"F{h}": dict(shards=2, n=9, T=20, G=6, H=h, calls="whole") for h in range(1, NHIST + 1)},
}
# the second tail-aliasing shape: T < H - 1, so every chunk of the second rollout still reads the tail
ALIAS_SMALL = dict(shards=2, n=9, T=5, G=2, H=10, calls="chunks")


def case_calls(case: dict) -> list[tuple[int, int]]:
    """The (t0, t1) of the decode calls of a case."""
    T, G = case["T"], case["G"]
    return [(0, T)] if case["calls"] == "whole" else [(a, min(a + G, T)) for a in range(0, T, G)]


# about 1 % of the planted words: quiet and signalling NaNs with payloads, +-0, +-inf, denormals
SPECIAL_WORDS = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0xFFFFFFFF, 0x7F800001, 0x7FA55AA5, 0xFF812345,
                          0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF,
                          0x807FFFFF, 0x00400000], np.uint32)


def random_words(rng, shape) -> np.ndarray:
    """Random 32-bit patterns, about 1 % of them SPECIAL_WORDS, none of them SENTINEL or POISON."""
    w = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    w[(w == SENTINEL) | (w == POISON)] ^= np.uint32(1)
    m = rng.random(shape) < 0.01
    w[m] = rng.choice(SPECIAL_WORDS, size=int(m.sum()))
    return w


def done_specs(T: int, H: int) -> list[tuple]:
    """The fixed list of per-env done patterns the env columns cycle through: (name, steps or probability, kind),
    kind 0 terminated only, 1 truncated only, 2 both, None a random one per done step.  The single resets around a
    window boundary (w0 = 16, 32) are listed where the step exists; the first nine hold every one around w0 = 16, so
    nine envs (case B) see them all."""
    def at(w0, k):
        return {"w0-H": w0 - H, "w0-(H-1)": w0 - (H - 1), "w0-1": w0 - 1, "w0": w0}[k]

    specs = [("never", [], 0), ("every", list(range(T)), None), ("16:w0-1", [at(16, "w0-1")], 0),
             ("first", [0], 1), ("16:w0-(H-1)", [at(16, "w0-(H-1)")], 1), ("last", [T - 1], 2),
             ("16:w0-H", [at(16, "w0-H")], 2), ("three", [s for s in range(5, 8)], None), ("16:w0", [16], 0),
             ("terminated", 0.15, 0), ("truncated", 0.15, 1), ("both", 0.15, 2), ("p0.15", 0.15, None),
             ("p0.5", 0.5, None)]
    specs += [(f"32:{k}", [at(32, k)], i % 3) for i, k in enumerate(("w0-H", "w0-(H-1)", "w0-1", "w0"))]
    keep = []
    for name, steps, kind in specs:
        if name == "three":  # moved inside a short rollout
            first = max(0, min(5, T - 3))
            steps = [s for s in range(first, first + 3) if s < T]
        elif isinstance(steps, list) and not all(0 <= s < T for s in steps):
            continue  # the step does not exist at this T
        elif ":" in name and int(name.split(":")[0]) >= T:
            continue  # nor does the window
        keep.append((name, steps, kind))
    return keep


def done_flags(rng, T: int, N: int, H: int):
    """(terminated, truncated) (T, N) uint8 of 0 / 1, env column j following done_specs(T, H)[j mod len]."""
    specs = done_specs(T, H)
    flags = np.zeros((2, T, N), np.uint8)
    for j in range(N):
        _, steps, kind = specs[j % len(specs)]
        if not isinstance(steps, list):
            steps = np.flatnonzero(rng.random(T) < steps)
        for s in steps:
            k = int(rng.integers(0, 3)) if kind is None else kind
            flags[0, s, j] = k != 1
            flags[1, s, j] = k != 0
    return flags[0], flags[1]


@functools.lru_cache(maxsize=None)
def _case_inputs(key: tuple, variant: int) -> dict:
    case = dict(key)
    R, n, T, G, H = case["shards"], case["n"], case["T"], case["G"], case["H"]
    NG = R * n
    rng = np.random.default_rng([zlib.crc32(repr(key).encode()), variant])
    d = {"frames": random_words(rng, (T, NG, FRAME)), "actions": random_words(rng, (T, NG, 12)),
         "rewards": random_words(rng, (T, NG)), "tail": random_words(rng, (NG, FRAME * H))}
    d["terminated"], d["truncated"] = done_flags(rng, T, NG, H)
    d["done"] = d["terminated"] | d["truncated"]
    d["records"], d["layout"] = plant(d["frames"], d["actions"], d["rewards"], d["terminated"], d["truncated"],
                                      R, n, T, G)
    d["ref"] = decode_ref(d["frames"], d["done"], d["tail"], H)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def case_inputs(case: dict, variant: int = 0) -> dict:
    """The planted inputs of a case (read-only uint32 words, computed once): frames, actions, rewards, tail,
    terminated, truncated, done, the gathered records with their layout, and ref = decode_ref of them."""
    return _case_inputs(tuple(sorted(case.items())), variant)
