// h12_learn.hip: learner-side kernels of libh12env.so for the CleanRL PPO of the CaT tasks (include/h12learn.h).
//
//   h12learn_rms_forward  running mean/variance update fused with the normalisation (RunningMeanStd.forward)
//   h12learn_gae_soft     GAE over soft (probabilistic) terminations
//   h12learn_mirror_rows  minibatch gather + mirror-symmetry column map + concatenation (h12env/symmetry.py)
//
// rms_forward, update != 0, is two launches:
//   1. rms_stats_kernel   grid (row chunks, column tiles).  A block reduces RMS_ROWS rows x 64 columns: lanes run
//      along the columns (a wave reads 256 contiguous bytes of a row, dword loads: a 450-float row is only 8-byte
//      aligned), each of the 4 waves takes RMS_WAVE_ROWS rows.  Per lane a shifted two-pass over the rows held in
//      registers gives (mean - K, M2), with a shift K per column common to every block (the mean of the column's
//      first rows), so partial means are small numbers whose rounding is relative to the spread of the column,
//      not to its offset; no E[x^2] - mean^2 anywhere.  The waves'
//      partials are Chan-merged in wave order and written per (chunk, column).  Every block then arrives on one
//      agent-scope acq_rel counter; the LAST block to arrive folds the chunks in index order into the running
//      statistics and resets the counter.  Nobody waits on anybody: no spin, no co-residency assumption, and the
//      merge order is fixed, so the statistics are bitwise reproducible.
//   2. rms_normalise_kernel  y = (x - mean) / sqrt(var + eps), flat over n*d.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/h12learn.h"

// the error record shared with h12_policy.hip (not part of the ABI)
int h12_learn_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3), visibility("hidden")));

namespace {

constexpr int RMS_WAVES = 4;
constexpr int RMS_WAVE_ROWS = 16;
constexpr int RMS_ROWS = RMS_WAVES * RMS_WAVE_ROWS;  // row-chunk size R
constexpr int RMS_COLS = 64;                         // one wave wide
constexpr int FOLD_BATCH = 8;                        // partials the folding block fetches at a time
constexpr int RMS_HEADER = 64;                      // bytes: the arrival counter, padded
constexpr int NORM_BLOCK = 256;
constexpr int NORM_PER_THREAD = 4;
constexpr int GAE_BLOCK = 64;
constexpr int MIR_WAVES = 4;
constexpr int MIR_WAVE_ROWS = 8;                     // rows a wave moves: 8 (16 with both) independent loads in flight
constexpr int MIR_ROWS = MIR_WAVES * MIR_WAVE_ROWS;  // rows per block
constexpr int MIR_COLS = 64;                         // one wave wide

thread_local char g_learn_err[256] = "";
int learn_err(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int learn_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_learn_err, sizeof g_learn_err, fmt, ap);
  va_end(ap);
  return code;
}
#define LEARN_HIP_TRY(expr)                                                               \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      (void)hipGetLastError();                                                            \
      return learn_err(H12LEARN_E_HIP, "%s: %s", #expr, hipGetErrorString(_e));           \
    }                                                                                     \
  } while (0)

// Chan merge of (nb, mb, M2b) into (na, ma, M2a); nb > 0.
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& M2a, float nb, float mb, float M2b) {
  const float n = na + nb;
  const float delta = mb - ma;
  ma = ma + delta * nb / n;
  M2a = M2a + M2b + delta * delta * na * nb / n;
  na = n;
}

// Pairwise sum of the 16 per-lane values: 4 roundings deep instead of 15, in a fixed order.
__device__ __forceinline__ float tree_sum16(const float (&v)[RMS_WAVE_ROWS]) {
  static_assert(RMS_WAVE_ROWS == 16, "tree_sum16 sums 16 values");
  const float a0 = v[0] + v[1], a1 = v[2] + v[3], a2 = v[4] + v[5], a3 = v[6] + v[7];
  const float a4 = v[8] + v[9], a5 = v[10] + v[11], a6 = v[12] + v[13], a7 = v[14] + v[15];
  return ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
}

// The shift K of column c that every block uses: the mean of the column's first min(n, 16) rows, computed the same
// way everywhere (so bit-equal in every block).  A partial mean is stored as (mean - K): of magnitude sigma / 4, not
// of the column's offset, nor of sigma as with a single sample as the shift, so its roundings in the Chan merges
// stay well inside 1e-7 sigma.
__device__ __forceinline__ float column_shift(const float* x, long long n, int d, int c) {
  const int cnt = n < RMS_WAVE_ROWS ? (int)n : RMS_WAVE_ROWS;
  const float x0 = x[c];
  float v[RMS_WAVE_ROWS];
#pragma unroll
  for (int i = 0; i < RMS_WAVE_ROWS; ++i) v[i] = i < cnt ? x[(size_t)i * (size_t)d + c] - x0 : 0.f;
  return x0 + tree_sum16(v) / (float)cnt;
}

__global__ __launch_bounds__(RMS_WAVES * 64) void rms_stats_kernel(const float* x, long long n, int d, float* mean,
                                                                    float* var, float* count, unsigned* counter,
                                                                    float2* partial) {
  __shared__ float2 s_part[RMS_WAVES][RMS_COLS];
  __shared__ int s_last;
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const long long chunk = blockIdx.x;
  const int c = blockIdx.y * RMS_COLS + lane;
  const long long rbase = chunk * RMS_ROWS + (long long)w * RMS_WAVE_ROWS;
  long long left = n - rbase;
  const int cnt = left <= 0 ? 0 : (left < RMS_WAVE_ROWS ? (int)left : RMS_WAVE_ROWS);

  float md = 0.f, M2 = 0.f;
  if (c < d && cnt > 0) {
    const float K = column_shift(x, n, d, c);
    const float* p = x + (size_t)rbase * (size_t)d + c;
    float v[RMS_WAVE_ROWS];
#pragma unroll
    for (int i = 0; i < RMS_WAVE_ROWS; ++i) v[i] = i < cnt ? p[(size_t)i * (size_t)d] - K : 0.f;
    md = tree_sum16(v) / (float)cnt;
#pragma unroll
    for (int i = 0; i < RMS_WAVE_ROWS; ++i) {
      const float e = v[i] - md;
      v[i] = i < cnt ? e * e : 0.f;
    }
    M2 = tree_sum16(v);
  }
  s_part[w][lane] = make_float2(md, M2);
  __syncthreads();
  if (w == 0 && c < d) {
    // wave 0 always has rows (chunks = ceil(n / RMS_ROWS)); the other waves are merged in wave order
    float na = (float)cnt, ma = md, Ma = M2;
    for (int k = 1; k < RMS_WAVES; ++k) {
      long long lk = n - (chunk * RMS_ROWS + (long long)k * RMS_WAVE_ROWS);
      const int ck = lk <= 0 ? 0 : (lk < RMS_WAVE_ROWS ? (int)lk : RMS_WAVE_ROWS);
      if (ck > 0) chan_merge(na, ma, Ma, (float)ck, s_part[k][lane].x, s_part[k][lane].y);
    }
    partial[(size_t)chunk * (size_t)d + c] = make_float2(ma, Ma);
  }

  // arrival: the partials were stored by wave 0; the barrier orders them before lane 0's acq_rel add, whose
  // release half writes them back at agent scope (one release per block, not one per thread).  Only the last
  // block to arrive goes on; its acquire makes every other block's partials visible.
  __syncthreads();
  if (tid == 0) {
    const unsigned total = gridDim.x * gridDim.y;
    const unsigned old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = old == total - 1u;
  }
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

  // fold: dp columns per pass (64, or the next power of two >= d when d < 64) x nseg = 256 / dp segments of the
  // chunk range.  A thread merges its segment's chunks in index order, then the segments are merged by a tree in
  // LDS: a fixed order, so the result is bitwise reproducible.
  __shared__ float s_fn[RMS_WAVES * 64], s_fm[RMS_WAVES * 64], s_fM[RMS_WAVES * 64];
  const float old_count = *count;
  const float nf = (float)n;
  const float tot = old_count + nf;
  const long long chunks = gridDim.x;
  int dp = RMS_COLS;
  if (d < RMS_COLS) {
    dp = 1;
    while (dp < d) dp <<= 1;
  }
  const int nseg = (RMS_WAVES * 64) / dp;
  const int fcol = tid & (dp - 1), seg = tid / dp;
  const long long per = (chunks + nseg - 1) / nseg;
  for (int base = 0; base < d; base += dp) {
    const int col = base + fcol;
    float na = 0.f, ma = 0.f, Ma = 0.f, K = 0.f;
    if (col < d) {
      if (seg == 0) K = column_shift(x, n, d, col);  // its loads overlap the merges below
      const long long k0 = (long long)seg * per;
      const long long k1 = k0 + per < chunks ? k0 + per : chunks;
      // the merges are a dependent chain: fetch FOLD_BATCH partials at a time so their latencies overlap
      for (long long k = k0; k < k1; k += FOLD_BATCH) {
        float2 pk[FOLD_BATCH];
#pragma unroll
        for (int j = 0; j < FOLD_BATCH; ++j)
          pk[j] = k + j < k1 ? partial[(size_t)(k + j) * (size_t)d + col] : make_float2(0.f, 0.f);
#pragma unroll
        for (int j = 0; j < FOLD_BATCH; ++j) {
          if (k + j < k1) {
            const long long lk = n - (k + j) * RMS_ROWS;
            const float nb = (float)(lk < RMS_ROWS ? lk : (long long)RMS_ROWS);
            if (k + j == k0) {
              na = nb, ma = pk[j].x, Ma = pk[j].y;
            } else {
              chan_merge(na, ma, Ma, nb, pk[j].x, pk[j].y);
            }
          }
        }
      }
    }
    s_fn[tid] = na, s_fm[tid] = ma, s_fM[tid] = Ma;
    __syncthreads();
    for (int stride = nseg >> 1; stride >= 1; stride >>= 1) {
      if (seg < stride) {
        const int o = tid + stride * dp;
        const float nb = s_fn[o];
        if (nb > 0.f) {  // empty segments (more segments than chunks) only ever sit at the upper end
          float an = s_fn[tid], am = s_fm[tid], aM = s_fM[tid];
          chan_merge(an, am, aM, nb, s_fm[o], s_fM[o]);
          s_fn[tid] = an, s_fm[tid] = am, s_fM[tid] = aM;
        }
      }
      __syncthreads();
    }
    if (seg == 0 && col < d) {
      // update_mean_var_count_from_moments with batch_mean = K + mean_shifted, batch_var * batch_count = M2
      const float m = mean[col];
      const float delta = (K - m) + s_fm[tid];
      mean[col] = m + delta * nf / tot;
      var[col] = (var[col] * old_count + s_fM[tid] + delta * delta * old_count * nf / tot) / tot;
    }
    __syncthreads();  // the LDS rows are reused by the next pass
  }
  if (tid == 0) {  // every thread read the old count before the barriers above
    *count = tot;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(NORM_BLOCK) void rms_normalise_kernel(const float* x, float* y, const float* mean,
                                                                    const float* var, size_t total, int d,
                                                                    float epsilon) {
  const size_t base = (size_t)blockIdx.x * (NORM_BLOCK * NORM_PER_THREAD);
  const unsigned c0 = (unsigned)(base % (size_t)d);  // uniform per block
#pragma unroll
  for (int k = 0; k < NORM_PER_THREAD; ++k) {
    const unsigned off = k * NORM_BLOCK + threadIdx.x;
    const size_t i = base + off;
    if (i < total) {
      const unsigned c = (c0 + off) % (unsigned)d;
      y[i] = (x[i] - mean[c]) / sqrtf(var[c] + epsilon);
    }
  }
}

// Every operation separately rounded, in the reference's left-to-right order.
__global__ __launch_bounds__(GAE_BLOCK) void gae_soft_kernel(const float* rewards, const float* values,
                                                             const float* dones, const float* true_dones,
                                                             const float* next_value, const float* next_done,
                                                             const float* next_true_done, float gamma,
                                                             float gamma_lambda, int T, int N, float* advantages,
                                                             float* returns) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * GAE_BLOCK + threadIdx.x;
  if (e >= N) return;
  float nv = next_value[e];
  float nn = 1.0f - next_done[e];
  float tn = 1.0f - next_true_done[e];
  float last = 0.0f;
  for (int t = T - 1; t >= 0; --t) {
    const size_t i = (size_t)t * (size_t)N + e;
    const float v = values[i];
    float a = gamma * nv;
    a = a * nn;
    a = a * tn;
    float delta = rewards[i] + a;
    delta = delta - v;
    float b = gamma_lambda * nn;
    b = b * tn;
    b = b * last;
    last = delta + b;
    advantages[i] = last;
    returns[i] = last + v;
    nv = v;
    nn = 1.0f - dones[i];
    tn = 1.0f - true_dones[i];
  }
}

// Gather + mirror + concatenation.  Grid (row chunks, column tiles), as in rms_stats_kernel: lanes run along 64
// output columns (dword accesses: a 450-float row is only 8-byte aligned), each of the 4 waves moves MIR_WAVE_ROWS
// rows with the lane's table entry held in a register.  The map moves a column by a few places inside its term, so
// a wave's reads of a row stay within the cache lines of its 64 columns and their neighbours; with both != 0 the
// original and the mirrored read of a source row hit the same lines (one fetch of the row from HBM).  The data are
// moved as 32-bit words and the sign is an XOR of bit 31: no floating-point instruction touches them, so NaN
// payloads, infinities and -0.0 pass whatever the device code's fast-math flags are.  The row index is wave-uniform
// (scalar loads of idx) and clamped to the source, the source column to the row.  A wave's rows past n re-read row
// n - 1 and store nothing, so every load is unconditional and the 8 (16) loads of a lane are in flight together.
template <bool BOTH, bool IDX>
__global__ __launch_bounds__(MIR_WAVES * 64) void mirror_rows_kernel(const uint32_t* x, long long n_src_rows,
                                                                     const long long* idx, long long n, int d,
                                                                     const uint32_t* table, uint32_t* out) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c = blockIdx.y * MIR_COLS + lane;
  const long long rbase = (long long)blockIdx.x * MIR_ROWS + (long long)w * MIR_WAVE_ROWS;
  if (c >= d || rbase >= n) return;
  const uint32_t t = table[c];
  const uint32_t sign = t & 0x80000000u;
  uint32_t src = t & 0x7fffffffu;
  src = src < (uint32_t)d ? src : (uint32_t)d - 1u;
  long long row[MIR_WAVE_ROWS];
#pragma unroll
  for (int i = 0; i < MIR_WAVE_ROWS; ++i) {  // the index loads first, so they are in flight together too
    const long long r = rbase + i < n ? rbase + i : n - 1;
    row[i] = IDX ? idx[r] : r;
  }
  uint32_t m[MIR_WAVE_ROWS], o[MIR_WAVE_ROWS];
#pragma unroll
  for (int i = 0; i < MIR_WAVE_ROWS; ++i) {
    const long long k = row[i] < 0 ? 0 : (row[i] < n_src_rows ? row[i] : n_src_rows - 1);
    const uint32_t* p = x + (size_t)k * (size_t)d;
    m[i] = p[src];
    if (BOTH) o[i] = p[c];
  }
  uint32_t* om = out + (BOTH ? (size_t)n * (size_t)d : (size_t)0);
#pragma unroll
  for (int i = 0; i < MIR_WAVE_ROWS; ++i) {
    const long long r = rbase + i;
    if (r < n) {
      om[(size_t)r * (size_t)d + c] = m[i] ^ sign;
      if (BOTH) out[(size_t)r * (size_t)d + c] = o[i];
    }
  }
}

}  // namespace

extern "C" {

int h12learn_rms_row_chunk(void) { return RMS_ROWS; }

size_t h12learn_rms_workspace_bytes(long long n, int d) {
  if (n < 1 || d < 1) return 0;
  const size_t chunks = (size_t)((n + RMS_ROWS - 1) / RMS_ROWS);
  return (size_t)RMS_HEADER + chunks * (size_t)d * sizeof(float2);
}

int h12learn_rms_forward(const float* x, float* y, float* mean, float* var, float* count, long long n, int d,
                         float epsilon, int update, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !y || !mean || !var || !count) return learn_err(H12LEARN_E_ARG, "rms_forward: null pointer");
  if (n < 1 || d < 1) return learn_err(H12LEARN_E_ARG, "rms_forward: n = %lld, d = %d (both must be >= 1)", n, d);
  hipStream_t s = (hipStream_t)stream;
  if (update) {
    const size_t need = h12learn_rms_workspace_bytes(n, d);
    if (!workspace || workspace_bytes < need)
      return learn_err(H12LEARN_E_ARG, "rms_forward: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (((uintptr_t)workspace & 15) != 0) return learn_err(H12LEARN_E_ARG, "rms_forward: workspace not 16-byte aligned");
    const long long chunks = (n + RMS_ROWS - 1) / RMS_ROWS;
    const int tiles = (d + RMS_COLS - 1) / RMS_COLS;
    if (chunks > 0x7fffffffLL || tiles > 65535 || chunks * tiles > 0xffffffffLL)
      return learn_err(H12LEARN_E_ARG, "rms_forward: n = %lld, d = %d exceed the grid", n, d);
    hipLaunchKernelGGL(rms_stats_kernel, dim3((unsigned)chunks, (unsigned)tiles), dim3(RMS_WAVES * 64), 0, s, x, n, d,
                       mean, var, count, (unsigned*)workspace, (float2*)((char*)workspace + RMS_HEADER));
    LEARN_HIP_TRY(hipGetLastError());
  }
  const size_t total = (size_t)n * (size_t)d;
  const size_t per_block = (size_t)NORM_BLOCK * NORM_PER_THREAD;
  const size_t blocks = (total + per_block - 1) / per_block;
  if (blocks > 0x7fffffffULL) return learn_err(H12LEARN_E_ARG, "rms_forward: n * d = %zu exceeds the grid", total);
  hipLaunchKernelGGL(rms_normalise_kernel, dim3((unsigned)blocks), dim3(NORM_BLOCK), 0, s, x, y, (const float*)mean,
                     (const float*)var, total, d, epsilon);
  LEARN_HIP_TRY(hipGetLastError());
  return H12LEARN_OK;
}

int h12learn_gae_soft(const float* rewards, const float* values, const float* dones, const float* true_dones,
                      const float* next_value, const float* next_done, const float* next_true_done, float gamma,
                      float gamma_lambda, int T, int N, float* advantages, float* returns, void* stream) {
  if (!rewards || !values || !dones || !true_dones || !next_value || !next_done || !next_true_done || !advantages ||
      !returns)
    return learn_err(H12LEARN_E_ARG, "gae_soft: null pointer");
  if (T < 1 || N < 1) return learn_err(H12LEARN_E_ARG, "gae_soft: T = %d, N = %d (both must be >= 1)", T, N);
  hipLaunchKernelGGL(gae_soft_kernel, dim3((N + GAE_BLOCK - 1) / GAE_BLOCK), dim3(GAE_BLOCK), 0, (hipStream_t)stream,
                     rewards, values, dones, true_dones, next_value, next_done, next_true_done, gamma, gamma_lambda, T,
                     N, advantages, returns);
  LEARN_HIP_TRY(hipGetLastError());
  return H12LEARN_OK;
}

int h12learn_mirror_rows(const float* x, long long n_src_rows, const long long* idx, long long n, int d,
                         const int* table, int both, float* out, void* stream) {
  if (!x) return learn_err(H12LEARN_E_ARG, "mirror_rows: x is null");
  if (!table) return learn_err(H12LEARN_E_ARG, "mirror_rows: table is null");
  if (!out) return learn_err(H12LEARN_E_ARG, "mirror_rows: out is null");
  if (d < 1) return learn_err(H12LEARN_E_ARG, "mirror_rows: d = %d (must be >= 1)", d);
  if (n < 0) return learn_err(H12LEARN_E_ARG, "mirror_rows: n = %lld (must be >= 0)", n);
  if (n_src_rows < 1) return learn_err(H12LEARN_E_ARG, "mirror_rows: n_src_rows = %lld (must be >= 1)", n_src_rows);
  if (!idx && n > n_src_rows)
    return learn_err(H12LEARN_E_ARG, "mirror_rows: n = %lld rows of a source of n_src_rows = %lld without idx", n,
                     n_src_rows);
  if (n == 0) return H12LEARN_OK;
  const long long chunks = (n + MIR_ROWS - 1) / MIR_ROWS;
  const int tiles = (d + MIR_COLS - 1) / MIR_COLS;
  if (chunks > 0x7fffffffLL || tiles > 65535)
    return learn_err(H12LEARN_E_ARG, "mirror_rows: n = %lld, d = %d exceed the grid", n, d);
  const dim3 grid((unsigned)chunks, (unsigned)tiles), block(MIR_WAVES * 64);
  const uint32_t* xs = (const uint32_t*)x;
  const uint32_t* tab = (const uint32_t*)table;
  uint32_t* o = (uint32_t*)out;
  hipStream_t s = (hipStream_t)stream;
  if (both && idx)
    hipLaunchKernelGGL((mirror_rows_kernel<true, true>), grid, block, 0, s, xs, n_src_rows, idx, n, d, tab, o);
  else if (both)
    hipLaunchKernelGGL((mirror_rows_kernel<true, false>), grid, block, 0, s, xs, n_src_rows, idx, n, d, tab, o);
  else if (idx)
    hipLaunchKernelGGL((mirror_rows_kernel<false, true>), grid, block, 0, s, xs, n_src_rows, idx, n, d, tab, o);
  else
    hipLaunchKernelGGL((mirror_rows_kernel<false, false>), grid, block, 0, s, xs, n_src_rows, idx, n, d, tab, o);
  LEARN_HIP_TRY(hipGetLastError());
  return H12LEARN_OK;
}

const char* h12learn_last_error(void) { return g_learn_err; }

}  // extern "C"

int h12_learn_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_learn_err, sizeof g_learn_err, fmt, ap);
  va_end(ap);
  return code;
}
