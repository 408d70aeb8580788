"""A numpy fp32 restatement of h12learn_rms_forward's update (csrc/h12_learn.hip), for CPU tests of the
gates of tests/test_gpu_cleanrl.py:

  shift K = x[0] + tree_sum16(x[i] - x[0], i < min(n, 16)) / min(n, 16)
  per wave (16 rows of a 64-row chunk): md = tree_sum16(x - K) / cnt, M2 = tree_sum16((x - K - md)^2)
  per chunk: the waves Chan-merged in wave order
  fold: the chunk range cut into nseg = 256 / dp segments of per = ceil(chunks / nseg) chunks, each merged in index
        order (the kernel fetches them FOLD_BATCH at a time), then a stride-halving tree over the segments that
        skips empty ones
  update_mean_var_count_from_moments with batch_mean = K + mean_shifted, batch_var * batch_count = M2

Every operation is a separately rounded fp32 operation.  Device code may contract multiply-adds, so this is not
bit-equal to the GPU and nothing claims it is: it models the data flow, so that a gate which rejects a planted error
here is known to resolve that error, and inputs which pass here are known to be attainable.

``plant`` switches on one deliberate error (None = the documented algorithm):
  batch_restart        the segment accumulator restarts at every FOLD_BATCH-chunk batch (j == 0 for k + j == k0)
  drop_partial_batch   a trailing batch of fewer than FOLD_BATCH chunks, after a segment's first, is skipped
  skip_tree_top        the segment tree starts at nseg / 4
  full_last_chunk      the fold weighs the last chunk as a full one
  single_sample_shift  K = x[0]
"""
import numpy as np

ROWS = 64        # RMS_ROWS: rows per chunk
WAVE_ROWS = 16   # RMS_WAVE_ROWS
COLS = 64        # RMS_COLS
BLOCK = 256      # threads of the folding block
FOLD_BATCH = 8
PLANTS = ("batch_restart", "drop_partial_batch", "skip_tree_top", "full_last_chunk", "single_sample_shift")

F = np.float32


def fold_geometry(n, d, rows=ROWS, block=BLOCK, cols=COLS):
    """(chunks, per, nseg, occupied segments) of the fold for an [n][d] batch."""
    chunks = -(-n // rows)
    dp = cols
    if d < cols:
        dp = 1
        while dp < d:
            dp <<= 1
    nseg = block // dp
    per = -(-chunks // nseg)
    return chunks, per, nseg, -(-chunks // per)


def _tree_sum16(v):
    """v: (16, ...) -> pairwise sum over axis 0 in the kernel's order."""
    a = v[0::2] + v[1::2]
    b = a[0::2] + a[1::2]
    c = b[0::2] + b[1::2]
    return c[0] + c[1]


def _chan(na, ma, Ma, nb, mb, Mb):
    n = na + nb
    delta = mb - ma
    with np.errstate(divide="ignore", invalid="ignore"):
        m = ma + delta * nb / n
        M = Ma + Mb + delta * delta * na * nb / n
    return n, m, M


def _merge_where(sel, na, ma, Ma, nb, mb, Mb):
    n, m, M = _chan(na, ma, Ma, nb, mb, Mb)
    return np.where(sel, n, na), np.where(sel, m, ma), np.where(sel, M, Ma)


def column_shift(x, plant=None):
    if plant == "single_sample_shift":
        return x[0].copy()
    cnt = min(x.shape[0], WAVE_ROWS)
    v = np.zeros((WAVE_ROWS, x.shape[1]), F)
    v[:cnt] = x[:cnt] - x[0]
    return x[0] + _tree_sum16(v) / F(cnt)


def chunk_partials(x, K):
    """(rows per chunk, mean - K, M2) per (chunk, column)."""
    n, d = x.shape
    chunks = -(-n // ROWS)
    waves = ROWS // WAVE_ROWS
    rows = np.arange(chunks * ROWS).reshape(chunks, waves, WAVE_ROWS)
    have = (rows < n).transpose(2, 0, 1)[..., None]                    # (16, chunks, waves, 1)
    cnt = (rows < n).sum(2).astype(F)[..., None]                       # (chunks, waves, 1)
    xp = np.zeros((chunks * ROWS, d), F)
    xp[:n] = x
    xp = xp.reshape(chunks, waves, WAVE_ROWS, d).transpose(2, 0, 1, 3)  # (16, chunks, waves, d)
    v = np.where(have, xp - K, F(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        md = np.where(cnt > 0, _tree_sum16(v) / cnt, F(0))
    e = v - md
    M2 = _tree_sum16(np.where(have, e * e, F(0)))
    na, ma, Ma = np.broadcast_to(cnt[:, 0], md[:, 0].shape).copy(), md[:, 0].copy(), M2[:, 0].copy()
    for k in range(1, waves):
        ck = np.broadcast_to(cnt[:, k], ma.shape)
        na, ma, Ma = _merge_where(ck > 0, na, ma, Ma, ck, md[:, k], M2[:, k])
    assert na.dtype == ma.dtype == Ma.dtype == F
    return na, ma, Ma


def fold(n, pn, pm, pM, plant=None):
    """The last block's fold of the per-chunk partials: (mean - K, M2) per column of the whole batch."""
    chunks, d = pm.shape
    _, per, nseg, _ = fold_geometry(n, d)
    nb_chunk = pn[:, :1].copy()  # min(n - k * 64, 64)
    if plant == "full_last_chunk":
        nb_chunk[-1] = F(ROWS)
    seg = np.arange(nseg)
    k0 = seg * per
    k1 = np.minimum(k0 + per, chunks)
    na, ma, Ma = (np.zeros((nseg, d), F) for _ in range(3))
    for t in range(per):
        k = k0 + t
        valid = k < k1
        if plant == "drop_partial_batch" and t >= FOLD_BATCH:
            valid &= k0 + FOLD_BATCH * (t // FOLD_BATCH + 1) <= k1
        first = t % FOLD_BATCH == 0 if plant == "batch_restart" else t == 0
        kk = np.minimum(k, chunks - 1)
        nb, mb, Mb = np.broadcast_to(nb_chunk[kk], (nseg, d)), pm[kk], pM[kk]
        sel = valid[:, None]
        if first:
            na, ma, Ma = np.where(sel, nb, na), np.where(sel, mb, ma), np.where(sel, Mb, Ma)
        else:
            na, ma, Ma = _merge_where(sel, na, ma, Ma, nb, mb, Mb)
    stride = nseg >> (2 if plant == "skip_tree_top" else 1)
    while stride >= 1:
        lo, hi = slice(0, stride), slice(stride, 2 * stride)
        na[lo], ma[lo], Ma[lo] = _merge_where(na[hi] > 0, na[lo], ma[lo], Ma[lo], na[hi], ma[hi], Ma[hi])
        stride >>= 1
    assert ma.dtype == Ma.dtype == F
    return ma[0], Ma[0]


def rms_update(x, mean, var, count, plant=None):
    """One updating call on fp32 state: the new (mean, var, count)."""
    assert x.dtype == F and mean.dtype == F and var.dtype == F
    n = x.shape[0]
    K = column_shift(x, plant)
    fm, fM = fold(n, *chunk_partials(x, K), plant=plant)
    old, nf = F(count), F(n)
    tot = old + nf
    delta = (K - mean) + fm
    new_mean = mean + delta * nf / tot
    new_var = (var * old + fM + delta * delta * old * nf / tot) / tot
    assert new_mean.dtype == new_var.dtype == F and type(tot) is F
    return new_mean, new_var, tot


def rms_normalise(x, mean, var, eps):
    return (x - mean) / np.sqrt(var + F(eps))


class RmsEmu:
    """The running state of the stand-in, with the call surface of the tests' Rms64."""

    def __init__(self, d, plant=None, eps=1e-8):
        self.mean, self.var, self.count = np.zeros(d, F), np.ones(d, F), F(1)
        self.plant, self.eps = plant, eps

    def __call__(self, x, update=True):
        if update:
            self.mean, self.var, self.count = rms_update(x, self.mean, self.var, self.count, self.plant)
        return rms_normalise(x, self.mean, self.var, self.eps)
