// h12_ppo_head.hip: the fused PPO loss head of libh12env.so (include/h12learn.h, h12learn_ppo_head): gather, Gaussian
// log-probability, KL, clipped surrogate, clipped value loss, their weighted sum and its gradients with respect to the
// actor's mean, the critic's value and the std parameter, in two launches.
//
//   1. ppo_head_rows_kernel<G>   a block owns HEAD_ROWS rows.  A row is a group of G lanes (G = 16 for A <= 16, else
//      32), lane a of the group its action a, and a wave's groups are consecutive rows: the wave's loads of mean (and of
//      directly read actions) cover 64 / G consecutive rows, contiguous in memory, and the gathered rows of actions,
//      old_mu and old_sigma are A contiguous floats each.  A wave takes its HEAD_UNROLL passes' loads in two batches
//      (indices; then everything addressed by them; nothing is used before the last load is issued).  The sums over a
//      row's actions are xor-butterflies inside the group (a fixed order, every lane of the group gets the same bits).
//      Lane 0 of a group holds the row's scalars (old log-probability, advantage, return, target value, value),
//      computes ratio, both surrogates, the value loss and d_value, and broadcasts d loss / d log_prob to its group.
//      The rows' surrogate / value / KL terms and their d_param terms go to LDS; after one barrier 3 + A threads add
//      them in row order and write the block's partial sums.
//   2. ppo_head_fold_kernel      one block.  The partials are staged through LDS in chunks (coalesced, all loads in
//      flight) and thread j adds quantity j in block-index order.  Thread 0 then forms the means, the entropy, the
//      total, the learning-rate rule and the statistics; threads 3 .. 3 + A finish d_param.
//
// No atomics, no counters, nothing to initialise: every output is a fixed-order sum.  The summed terms are fp32, the
// accumulators and the partials fp64, so a sum carries the rounding of its terms only.
//
// The CleanRL trainer's head (h12learn_cleanrl_head) follows the PPO head's kernels below.  What the two heads compute
// alike (the rows' bookkeeping, the clipped surrogate, the clipped value error, the two kinds of sum, the block's
// partial) is one device function each; their loads, value transform, third scalar and gradient scales differ and stay
// in two rows kernels and two fold epilogues.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/h12learn.h"

// the error record of h12_learn.hip (not part of the ABI)
int h12_learn_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3), visibility("hidden")));

// No multiply is fused into a following add anywhere in this file: the kernels restate torch's separately rounded
// operations.  At file scope, so that a helper inlined into a kernel cannot carry another setting than the kernel.
#pragma clang fp contract(off)

namespace {

constexpr int HEAD_WAVES = 4;
constexpr int HEAD_ROWS = 64;        // rows per block R
constexpr int HEAD_UNROLL = 4;       // passes whose loads are in flight together
constexpr int HEAD_MAX_A = 32;
constexpr int HEAD_SC = 3;           // per-row scalars that are summed: surrogate, value, KL (CleanRL: clip indicator)
constexpr int FOLD_THREADS = 256;
constexpr int FOLD_CHUNK = 128;      // blocks staged in LDS at a time
constexpr int FOLD_PER_THREAD = (FOLD_CHUNK * (HEAD_SC + HEAD_MAX_A) + FOLD_THREADS - 1) / FOLD_THREADS;
constexpr int SUM_BATCH = 8;        // LDS reads in flight ahead of a serial sum
template <int G>                    // G lanes per row: a block's passes, of HEAD_WAVES * (64 / G) rows each
constexpr int PASSES = HEAD_ROWS / (HEAD_WAVES * (64 / G));
static_assert(PASSES<16> % HEAD_UNROLL == 0 && PASSES<32> % HEAD_UNROLL == 0,
              "the passes are taken HEAD_UNROLL at a time");
static_assert(HEAD_ROWS % SUM_BATCH == 0, "the row sums read SUM_BATCH rows at a time");
constexpr double LOG_SQRT_2PI_D = 0.918938533204672741780329736406;  // log(sqrt(2 pi)), also 0.5 log(2 pi)
constexpr float LOG_SQRT_2PI = (float)LOG_SQRT_2PI_D;

struct LossScalars {  // the coefficients both heads have, narrowed once on the host
  float lo, hi;      // 1 -+ the clip coefficient
  float clip;        // the value clip
  float vcoef, ecoef;
};

struct HeadScalars : LossScalars {
  float kl_up, kl_down;  // 2 desired_kl, desired_kl / 2
};

#define HEAD_HIP_TRY(expr)                                                                  \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      (void)hipGetLastError();                                                              \
      return h12_learn_fail(H12LEARN_E_HIP, "%s: %s", #expr, hipGetErrorString(_e));        \
    }                                                                                       \
  } while (0)

template <int G, typename T = float>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, G);
  return v;
}

// torch.max's backward weights of x against y: (weight of x, weight of y)
__device__ __forceinline__ void max_weights(float x, float y, float& wx, float& wy) {
  wx = x > y ? 1.0f : (x == y ? 0.5f : 0.0f);
  wy = x < y ? 1.0f : (x == y ? 0.5f : 0.0f);
}

// ---- the rows both heads' rows kernels walk: a block's HEAD_ROWS rows in passes of HEAD_WAVES * (64 / G) rows
// the block row of lane group `grp` of wave `w` in pass `pass`
template <int G>
__device__ __forceinline__ int pass_row(int pass, int w, int grp) {
  return pass * (HEAD_WAVES * (64 / G)) + w * (64 / G) + grp;
}

// the row that is read for row r of m: rows past m re-read row m - 1 and store nothing
__device__ __forceinline__ long long read_row(long long r, long long m) { return r < m ? r : m - 1; }

// entry j of idx (null: j itself), and its clamp into the n_src source rows.  Two functions: the rows kernels issue
// every index load of a batch before the first clamp waits for one.
__device__ __forceinline__ long long source_row(const long long* idx, long long j) { return idx ? idx[j] : j; }
__device__ __forceinline__ long long clamp_row(long long k, long long n_src) {
  return k < 0 ? 0 : (k < n_src ? k : n_src - 1);
}

// the clipped surrogate of one row, max(-adv ratio, -adv clamp(ratio, lo, hi)); g_lp = d (that / m) / d log_prob
__device__ __forceinline__ float surrogate_row(float adv, float ratio, float lo, float hi, float inv_m, float& g_lp) {
  const float s1 = -adv * ratio;
  const float s2 = -adv * fminf(fmaxf(ratio, lo), hi);
  const bool inside = ratio >= lo && ratio <= hi;
  float w1, w2;
  max_weights(s1, s2, w1, w2);
  g_lp = inv_m * (-adv * (w1 + (inside ? w2 : 0.0f))) * ratio;
  return fmaxf(s1, s2);
}

// the clipped value error of one row, max((v - ret)^2, (target + clamp(v - target, -clip, clip) - ret)^2); dv = its
// derivative with respect to v
__device__ __forceinline__ float clipped_value_row(float v, float target, float ret, float clip, float& dv) {
  const float dvt = v - target;
  const float vc = target + fminf(fmaxf(dvt, -clip), clip);
  const bool inside_v = dvt >= -clip && dvt <= clip;
  const float e1 = v - ret, e2 = vc - ret;
  const float q1 = e1 * e1, q2 = e2 * e2;
  float v1, v2;
  max_weights(q1, q2, v1, v2);
  dv = v1 * (2.0f * e1) + (inside_v ? v2 * (2.0f * e2) : 0.0f);
  return fmaxf(q1, q2);
}

// row-order sum of one column of an LDS array of HEAD_ROWS rows, `stride` floats apart (fp64 accumulator: the sum then
// carries the rounding of its fp32 terms only); SUM_BATCH reads in flight ahead of the dependent adds
__device__ __forceinline__ double rows_sum(const float* col, int stride) {
  double acc = 0.0;
  for (int r = 0; r < HEAD_ROWS; r += SUM_BATCH) {
    float v[SUM_BATCH];
#pragma unroll
    for (int j = 0; j < SUM_BATCH; ++j) v[j] = col[(r + j) * stride];
#pragma unroll
    for (int j = 0; j < SUM_BATCH; ++j) acc += (double)v[j];
  }
  return acc;
}

// a block's partial, after the barrier behind its rows: threads [0, A) of wave 0 take the parameter columns of s_dp,
// threads [64, 64 + HEAD_SC) the scalars of s_sc
template <int G>
__device__ __forceinline__ void write_partial(const float (*s_dp)[G], const float (*s_sc)[HEAD_SC + 1], int A, int tid,
                                              double* partial) {
  double* out = partial + (size_t)blockIdx.x * (size_t)(HEAD_SC + A);
  if (tid < A) {
    out[HEAD_SC + tid] = rows_sum(&s_dp[0][tid], G);
  } else if (tid >= 64 && tid < 64 + HEAD_SC) {
    const int q = tid - 64;
    out[q] = rows_sum(&s_sc[0][q], HEAD_SC + 1);
  }
}

// the fold's sums: `blocks` partials of P quantities each are staged through s_buf (FOLD_CHUNK * (HEAD_SC + HEAD_MAX_A)
// doubles of LDS) in chunks (coalesced, all loads in flight); thread j < P returns quantity j added in block-index order
__device__ __forceinline__ double fold_sum(const double* partial, int blocks, int P, int tid, double* s_buf) {
  double acc = 0.0;
  for (int c0 = 0; c0 < blocks; c0 += FOLD_CHUNK) {
    const int cnt = blocks - c0 < FOLD_CHUNK ? blocks - c0 : FOLD_CHUNK;
    const int total = cnt * P;
    const double* src = partial + (size_t)c0 * (size_t)P;
    double stage[FOLD_PER_THREAD];  // every load of the chunk issued before the first LDS store
#pragma unroll
    for (int j = 0; j < FOLD_PER_THREAD; ++j) {
      const int i = tid + j * FOLD_THREADS;
      stage[j] = i < total ? src[i] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < FOLD_PER_THREAD; ++j) {
      const int i = tid + j * FOLD_THREADS;
      if (i < total) s_buf[i] = stage[j];
    }
    __syncthreads();
    if (tid < P) {
      // block-index order; SUM_BATCH reads in flight ahead of the dependent adds (a tail adds +0.0: no change)
      for (int b = 0; b < cnt; b += SUM_BATCH) {
        double v[SUM_BATCH];
#pragma unroll
        for (int j = 0; j < SUM_BATCH; ++j) v[j] = b + j < cnt ? s_buf[(b + j) * P + tid] : 0.0;
#pragma unroll
        for (int j = 0; j < SUM_BATCH; ++j) acc += v[j];
      }
    }
    __syncthreads();  // the buffer is reused by the next chunk
  }
  return acc;
}

template <int G>
__global__ __launch_bounds__(HEAD_WAVES * 64) void ppo_head_rows_kernel(h12learn_ppo_head_args p, HeadScalars sc,
                                                                        double* partial) {
  __shared__ float s_dp[HEAD_ROWS][G];
  __shared__ float s_sc[HEAD_ROWS][HEAD_SC + 1];

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int a = lane & (G - 1), grp = lane / G;
  const int A = p.A;
  const bool col = a < A;
  const int ac = col ? a : A - 1;  // lanes past A re-read the last column and contribute nothing
  const long long m = p.m, B = p.B;
  const float inv_m = 1.0f / (float)m;

  // the lane's column of the std parameter
  const float prm = p.std_param[ac];
  const float sigma = p.std_kind == H12LEARN_PPO_STD_LOG ? expf(prm) : prm;
  const float log_sigma = logf(sigma);
  const float two_var = 2.0f * (sigma * sigma);
  const float inv_sigma = 1.0f / sigma;
  const float inv_var = inv_sigma * inv_sigma;

  const long long block_row = (long long)blockIdx.x * HEAD_ROWS;
  for (int p0 = 0; p0 < PASSES<G>; p0 += HEAD_UNROLL) {
    long long rr[HEAD_UNROLL], k[HEAD_UNROLL];
    int rl[HEAD_UNROLL];
#pragma unroll
    for (int i = 0; i < HEAD_UNROLL; ++i) {  // batch 1: the indices
      rl[i] = pass_row<G>(p0 + i, w, grp);
      rr[i] = read_row(block_row + rl[i], m);
      k[i] = source_row(p.idx, rr[i] >= B ? rr[i] - B : rr[i]);  // a mirrored row has its original's sources
    }
    float mu[HEAD_UNROLL], act[HEAD_UNROLL], omu[HEAD_UNROLL], osg[HEAD_UNROLL];
    float olp[HEAD_UNROLL], adv[HEAD_UNROLL], ret[HEAD_UNROLL], tv[HEAD_UNROLL], val[HEAD_UNROLL];
#pragma unroll
    for (int i = 0; i < HEAD_UNROLL; ++i) {  // batch 2: everything else
      k[i] = clamp_row(k[i], p.n_src);
      const size_t er = (size_t)rr[i] * (size_t)A + ac, ek = (size_t)k[i] * (size_t)A + ac;
      mu[i] = p.mean[er];
      act[i] = p.actions[p.actions_direct ? er : ek];
      omu[i] = 0.0f, osg[i] = 1.0f;
      if (rr[i] < B) {  // the KL runs over the original samples only
        omu[i] = p.old_mu[ek];
        osg[i] = p.old_sigma[ek];
      }
      olp[i] = adv[i] = ret[i] = tv[i] = val[i] = 0.0f;
      if (a == 0) {
        olp[i] = p.old_log_prob[k[i]];
        adv[i] = p.advantages[k[i]];
        ret[i] = p.returns[k[i]];
        tv[i] = p.target_values[k[i]];
        val[i] = p.value[rr[i]];
      }
    }
#pragma unroll
    for (int i = 0; i < HEAD_UNROLL; ++i) {
      const bool live = block_row + rl[i] < m;
      const float d = act[i] - mu[i];
      const float dd = d * d;
      const float lp_a = -dd / two_var - log_sigma - LOG_SQRT_2PI;
      const float dm = omu[i] - mu[i];
      const float kl_a = logf(sigma / osg[i] + 1.0e-5f) + (osg[i] * osg[i] + dm * dm) / two_var - 0.5f;
      const float log_prob = group_sum<G>(col ? lp_a : 0.0f);
      const float kl = group_sum<G>(col ? kl_a : 0.0f);
      float g_lp = 0.0f;
      if (a == 0) {
        const float ratio = expf(log_prob - olp[i]);
        const float surr = surrogate_row(adv[i], ratio, sc.lo, sc.hi, inv_m, g_lp);
        float vl, dv;
        if (p.use_clipped_value_loss) {
          vl = clipped_value_row(val[i], tv[i], ret[i], sc.clip, dv);
        } else {
          const float e = ret[i] - val[i];
          vl = e * e;
          dv = -2.0f * e;
        }
        if (live) p.d_value[rr[i]] = (sc.vcoef * inv_m) * dv;
        s_sc[rl[i]][0] = live ? surr : 0.0f;
        s_sc[rl[i]][1] = live ? vl : 0.0f;
        s_sc[rl[i]][2] = live && rr[i] < B ? kl : 0.0f;
      }
      g_lp = __shfl(g_lp, 0, G);
      if (live && col) p.d_mean[(size_t)rr[i] * (size_t)A + a] = g_lp * (d * inv_var);
      // d log_prob / d sigma = (actions - mean)^2 / sigma^3 - 1 / sigma
      s_dp[rl[i]][a] = live && col ? g_lp * (dd * inv_var * inv_sigma - inv_sigma) : 0.0f;
    }
  }
  __syncthreads();
  write_partial<G>(s_dp, s_sc, A, tid, partial);
}

__global__ __launch_bounds__(FOLD_THREADS) void ppo_head_fold_kernel(h12learn_ppo_head_args p, HeadScalars sc,
                                                                      const double* partial, int blocks) {
  __shared__ double s_buf[FOLD_CHUNK * (HEAD_SC + HEAD_MAX_A)];
  __shared__ double s_fin[HEAD_SC + HEAD_MAX_A];
  __shared__ double s_ent[HEAD_MAX_A];
  const int tid = threadIdx.x;
  const int P = HEAD_SC + p.A;
  const bool is_log = p.std_kind == H12LEARN_PPO_STD_LOG;
  // issued before the partials are touched, so these latencies overlap the sums
  const float prm = tid >= HEAD_SC && tid < P ? p.std_param[tid - HEAD_SC] : 0.0f;
  const float lr = tid == 0 && p.lr ? *p.lr : 0.0f;
  float st[3] = {0.0f, 0.0f, 0.0f};
  if (tid == 0 && p.stats_accum) st[0] = p.stats_accum[0], st[1] = p.stats_accum[1], st[2] = p.stats_accum[2];
  const double acc = fold_sum(partial, blocks, P, tid, s_buf);
  if (tid < P) s_fin[tid] = acc;
  if (tid >= HEAD_SC && tid < P) {
    // d loss / d sigma = sum_r (...) - entropy_coef / sigma; the log parameter's gradient is that times sigma
    const float sigma = is_log ? expf(prm) : prm;
    const double g = acc - (double)sc.ecoef / (double)sigma;
    p.d_param[tid - HEAD_SC] = (float)(is_log ? g * (double)sigma : g);
    s_ent[tid - HEAD_SC] = (0.5 + LOG_SQRT_2PI_D) + (double)logf(sigma);
  }
  __syncthreads();
  if (tid == 0) {
    double ent_sum = 0.0;
    for (int a = 0; a < p.A; ++a) ent_sum += s_ent[a];
    const double surr_d = s_fin[0] / (double)p.m, vl_d = s_fin[1] / (double)p.m;
    const float surr = (float)surr_d, vl = (float)vl_d, ent = (float)ent_sum;
    const float kl = (float)(s_fin[2] / (double)p.B);
    p.out[0] = surr;
    p.out[1] = vl;
    p.out[2] = ent;
    p.out[3] = kl;
    p.out[4] = (float)(surr_d + (double)sc.vcoef * vl_d - (double)sc.ecoef * ent_sum);
    if (p.lr) {
      float next = lr;
      if (kl > sc.kl_up)
        next = fmaxf(lr * (1.0f / 1.5f), 1.0e-5f);  // torch divides by a host scalar as a product with its reciprocal
      else if (kl > 0.0f && kl < sc.kl_down)
        next = fminf(lr * 1.5f, 1.0e-2f);
      *p.lr = next;
    }
    if (p.stats_accum) {
      p.stats_accum[0] = st[0] + vl;
      p.stats_accum[1] = st[1] + surr;
      p.stats_accum[2] = st[2] + ent;
    }
  }
}

// ---- the CleanRL head (include/h12learn.h, h12learn_cleanrl_head): the same rows-in-lane-groups layout, butterflies,
// fp64 block partials and in-order fold, with the per-minibatch advantage normalisation in front of the rows:
//
//   1. cleanrl_adv_kernel        one wave per block of HEAD_ROWS rows, a row per lane: the gathered advantages' two-pass
//      (count, mean, M2) in fp64, the sums butterflies over the wave.
//   2. cleanrl_head_rows_kernel<G>   every block first merges the advantage partials of all blocks itself, in block-index
//      order: thread j stages partial j and its two merge coefficients (the counts in front of block j are j HEAD_ROWS, so
//      the divisions are off the dependent chain), thread 0 runs Chan's update over them.  Then the rows, as above.
//   3. cleanrl_head_fold_kernel  the in-order fold, the entropy, the total, the statistics, d_logstd.
constexpr int CLEAN_ADV = 3;   // a block's advantage partial: count, mean, M2
constexpr int MERGE_CHUNK = HEAD_WAVES * 64;  // advantage partials staged in LDS at a time

struct CleanScalars : LossScalars {
  float veps;
};

__global__ __launch_bounds__(64) void cleanrl_adv_kernel(h12learn_cleanrl_head_args p, double* apart) {
  static_assert(HEAD_ROWS == 64, "one wave per block, a row per lane");
  const int lane = threadIdx.x;
  const long long first = (long long)blockIdx.x * HEAD_ROWS;
  const long long left = p.m - first;
  const int n = left < HEAD_ROWS ? (int)left : HEAD_ROWS;
  const bool live = lane < n;
  const long long k = clamp_row(source_row(p.idx, read_row(first + lane, p.m)), p.n_src);
  const double x = (double)p.advantages[k];
  const double mean = group_sum<64, double>(live ? x : 0.0) / (double)n;
  const double d = live ? x - mean : 0.0;
  const double m2 = group_sum<64, double>(d * d);
  if (lane == 0) {
    double* out = apart + (size_t)blockIdx.x * CLEAN_ADV;
    out[0] = (double)n;
    out[1] = mean;
    out[2] = m2;
  }
}

// Chan's merge of the blocks' advantage partials in block-index order, by every thread of a block of MERGE_CHUNK threads
// together: s_adv[0] = the minibatch's mean, s_adv[1] = its std (correction 1) + 1e-8, both narrowed once.  Thread j
// stages partial j and its two coefficients (the count in front of block j is j HEAD_ROWS: the divisions are off the
// dependent chain), thread 0 runs the chain.  Ends on a barrier.
__device__ __forceinline__ void merge_adv(const double* apart, int blocks, long long m, int tid,
                                          double (*s_mg)[4], float* s_adv) {
  double mean = 0.0, m2 = 0.0;  // thread 0's running merge
  for (int c0 = 0; c0 < blocks; c0 += MERGE_CHUNK) {
    const int cnt = blocks - c0 < MERGE_CHUNK ? blocks - c0 : MERGE_CHUNK;
    if (tid < cnt) {
      const double* q = apart + (size_t)(c0 + tid) * CLEAN_ADV;
      const double nb = q[0], na = (double)(c0 + tid) * (double)HEAD_ROWS;  // every block before the last is full
      const double n = na + nb;
      s_mg[tid][0] = q[1];
      s_mg[tid][1] = q[2];
      s_mg[tid][2] = nb / n;
      s_mg[tid][3] = na * nb / n;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll 4
      for (int j = 0; j < cnt; ++j) {  // Chan: mean += delta nb / n;  M2 += M2_b + delta^2 na nb / n
        const double delta = s_mg[j][0] - mean;
        mean = mean + delta * s_mg[j][2];
        m2 = m2 + (s_mg[j][1] + delta * delta * s_mg[j][3]);
      }
    }
    __syncthreads();  // the buffer is reused by the next chunk
  }
  if (tid == 0) {
    s_adv[0] = (float)mean;
    s_adv[1] = (float)sqrt(m2 / (double)(m - 1)) + 1.0e-8f;  // torch.std: correction 1
  }
  __syncthreads();
}

template <int G>
__global__ __launch_bounds__(HEAD_WAVES * 64) void cleanrl_head_rows_kernel(h12learn_cleanrl_head_args p,
                                                                            CleanScalars sc, const double* apart,
                                                                            double* partial, int blocks) {
  __shared__ float s_dp[HEAD_ROWS][G];
  __shared__ float s_sc[HEAD_ROWS][HEAD_SC + 1];
  __shared__ double s_mg[MERGE_CHUNK][4];
  __shared__ float s_adv[2];

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int a = lane & (G - 1), grp = lane / G;
  const int A = p.A;
  const bool col = a < A;
  const int ac = col ? a : A - 1;  // lanes past A re-read the last column and contribute nothing
  const long long m = p.m;
  const float inv_m = 1.0f / (float)m;

  const float logstd = p.logstd[ac];
  const float sigma = expf(logstd);
  const float two_var = 2.0f * (sigma * sigma);
  const float inv_sigma = 1.0f / sigma;
  const float inv_var = inv_sigma * inv_sigma;
  // value_rms (update=False): (value - running_mean) / sqrt(running_var + epsilon)
  const float vmean = *p.value_mean;
  const float vsd = sqrtf(*p.value_var + sc.veps);

  float adv_mean = 0.0f, adv_den = 1.0f;
  if (p.norm_adv) {
    merge_adv(apart, blocks, m, tid, s_mg, s_adv);
    adv_mean = s_adv[0];
    adv_den = s_adv[1];
  }

  const long long block_row = (long long)blockIdx.x * HEAD_ROWS;
  for (int p0 = 0; p0 < PASSES<G>; p0 += HEAD_UNROLL) {
    long long rr[HEAD_UNROLL], k[HEAD_UNROLL];
    int rl[HEAD_UNROLL];
#pragma unroll
    for (int i = 0; i < HEAD_UNROLL; ++i) {  // batch 1: the indices
      rl[i] = pass_row<G>(p0 + i, w, grp);
      rr[i] = read_row(block_row + rl[i], m);
      k[i] = source_row(p.idx, rr[i]);
    }
    float mu[HEAD_UNROLL], act[HEAD_UNROLL];
    float olp[HEAD_UNROLL], adv[HEAD_UNROLL], ret[HEAD_UNROLL], vn[HEAD_UNROLL], val[HEAD_UNROLL];
#pragma unroll
    for (int i = 0; i < HEAD_UNROLL; ++i) {  // batch 2: everything else
      k[i] = clamp_row(k[i], p.n_src);
      mu[i] = p.mean[(size_t)rr[i] * (size_t)A + ac];
      act[i] = p.actions[(size_t)k[i] * (size_t)A + ac];
      olp[i] = adv[i] = ret[i] = vn[i] = val[i] = 0.0f;
      if (a == 0) {
        olp[i] = p.old_log_prob[k[i]];
        adv[i] = p.advantages[k[i]];
        ret[i] = p.returns_n[k[i]];
        vn[i] = p.values_n[k[i]];
        val[i] = p.value[rr[i]];
      }
    }
#pragma unroll
    for (int i = 0; i < HEAD_UNROLL; ++i) {
      const bool live = block_row + rl[i] < m;
      const float d = act[i] - mu[i];
      const float dd = d * d;
      const float lp_a = -dd / two_var - logstd - LOG_SQRT_2PI;
      const float log_prob = group_sum<G>(col ? lp_a : 0.0f);
      float g_lp = 0.0f;
      if (a == 0) {
        const float ad = p.norm_adv ? (adv[i] - adv_mean) / adv_den : adv[i];
        const float ratio = expf(log_prob - olp[i]);
        const float pg = surrogate_row(ad, ratio, sc.lo, sc.hi, inv_m, g_lp);
        const float nv = (val[i] - vmean) / vsd;
        float vl, dv;
        if (p.clip_vloss) {
          vl = clipped_value_row(nv, vn[i], ret[i], sc.clip, dv);
        } else {
          const float e = nv - ret[i];
          vl = e * e;
          dv = 2.0f * e;
        }
        // d loss / d v row = vf_coef * 0.5 / m; d nv / d value = 1 / sqrt(var + eps)
        if (live) p.d_value[rr[i]] = ((sc.vcoef * 0.5f * inv_m) * dv) / vsd;
        s_sc[rl[i]][0] = live ? pg : 0.0f;
        s_sc[rl[i]][1] = live ? vl : 0.0f;
        s_sc[rl[i]][2] = live && fabsf(ratio - 1.0f) > sc.clip ? 1.0f : 0.0f;
      }
      g_lp = __shfl(g_lp, 0, G);
      if (live && col) p.d_mean[(size_t)rr[i] * (size_t)A + a] = g_lp * (d * inv_var);
      // d log_prob / d logstd = (actions - mean)^2 / sigma^2 - 1
      s_dp[rl[i]][a] = live && col ? g_lp * (dd * inv_var - 1.0f) : 0.0f;
    }
  }
  __syncthreads();
  write_partial<G>(s_dp, s_sc, A, tid, partial);
}

__global__ __launch_bounds__(FOLD_THREADS) void cleanrl_head_fold_kernel(h12learn_cleanrl_head_args p, CleanScalars sc,
                                                                          const double* partial, int blocks) {
  __shared__ double s_buf[FOLD_CHUNK * (HEAD_SC + HEAD_MAX_A)];
  __shared__ double s_fin[HEAD_SC + HEAD_MAX_A];
  __shared__ double s_ent[HEAD_MAX_A];
  const int tid = threadIdx.x;
  const int P = HEAD_SC + p.A;
  // issued before the partials are touched, so these latencies overlap the sums
  const float logstd = tid >= HEAD_SC && tid < P ? p.logstd[tid - HEAD_SC] : 0.0f;
  float st[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (tid == 0 && p.stats_accum) {
#pragma unroll
    for (int j = 0; j < 5; ++j) st[j] = p.stats_accum[j];
  }
  const double acc = fold_sum(partial, blocks, P, tid, s_buf);
  if (tid < P) s_fin[tid] = acc;
  if (tid >= HEAD_SC && tid < P) {
    // the entropy is sum_a logstd[a] + const, the same for every row: d (-ent_coef * entropy) / d logstd[a] = -ent_coef
    p.d_logstd[tid - HEAD_SC] = (float)(acc - (double)sc.ecoef);
    s_ent[tid - HEAD_SC] = (0.5 + LOG_SQRT_2PI_D) + (double)logstd;
  }
  __syncthreads();
  if (tid == 0) {
    double ent_sum = 0.0;
    for (int a = 0; a < p.A; ++a) ent_sum += s_ent[a];
    const double pg_d = s_fin[0] / (double)p.m, v_d = 0.5 * (s_fin[1] / (double)p.m);
    float o[5];
    o[0] = (float)pg_d;
    o[1] = (float)ent_sum;
    o[2] = (float)v_d;
    o[3] = (float)(pg_d - (double)sc.ecoef * ent_sum + (double)sc.vcoef * v_d);
    o[4] = (float)(s_fin[2] / (double)p.m);
#pragma unroll
    for (int j = 0; j < 5; ++j) p.out[j] = o[j];
    if (p.stats_accum) {
#pragma unroll
      for (int j = 0; j < 5; ++j) p.stats_accum[j] = st[j] + o[j];
    }
  }
}

// ---- the host side: what the two entry points check and do alike.  `head` is the name their messages begin with.
long long head_blocks(long long m) { return (m + HEAD_ROWS - 1) / HEAD_ROWS; }

// the workspace of a head whose blocks keep `extra` doubles besides their HEAD_SC + A sums; 0, with the error recorded,
// for an m or an A out of range
size_t workspace_bytes(const char* head, long long m, int A, int extra) {
  if (m < 1) {
    h12_learn_fail(H12LEARN_E_ARG, "%s_workspace_bytes: m = %lld (must be >= 1)", head, m);
    return 0;
  }
  if (A < 1 || A > HEAD_MAX_A) {
    h12_learn_fail(H12LEARN_E_ARG, "%s_workspace_bytes: A = %d (1 .. %d)", head, A, HEAD_MAX_A);
    return 0;
  }
  return (size_t)head_blocks(m) * (size_t)(extra + HEAD_SC + A) * sizeof(double);
}

struct Required {
  const void* ptr;
  const char* name;
};

// The checks of the fields both argument structs have: m, A, n_src, the `rows` (named `rows_name`) source rows that are
// read without idx, the pointers that must be set, the workspace's size and alignment, the grid.  0, or the error.
template <typename Args, size_t N>
int check_head(const char* head, const Args& p, const char* rows_name, long long rows, const Required (&required)[N],
               int extra) {
  if (p.m < 1) return h12_learn_fail(H12LEARN_E_ARG, "%s: m = %lld (must be >= 1)", head, p.m);
  if (p.A < 1 || p.A > HEAD_MAX_A)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: A = %d (1 .. %d)", head, p.A, HEAD_MAX_A);
  if (p.n_src < 1) return h12_learn_fail(H12LEARN_E_ARG, "%s: n_src = %lld (must be >= 1)", head, p.n_src);
  if (!p.idx && rows > p.n_src)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: %s = %lld rows of sources of n_src = %lld without idx", head, rows_name,
                          rows, p.n_src);
  for (const Required& q : required)
    if (!q.ptr) return h12_learn_fail(H12LEARN_E_ARG, "%s: %s is null", head, q.name);
  const size_t need = workspace_bytes(head, p.m, p.A, extra);
  if (p.workspace_bytes < need)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: workspace_bytes = %zu, %zu needed", head, p.workspace_bytes, need);
  if (((uintptr_t)p.workspace & 7) != 0)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: workspace is not 8-byte aligned", head);
  if (head_blocks(p.m) > 0x7fffffffLL) return h12_learn_fail(H12LEARN_E_ARG, "%s: m = %lld exceeds the grid", head, p.m);
  return H12LEARN_OK;
}

LossScalars loss_scalars(double clip, double vcoef, double ecoef) {
  return {(float)(1.0 - clip), (float)(1.0 + clip), (float)clip, (float)vcoef, (float)ecoef};
}

// a head's rows kernel: 16 lanes per row up to 16 actions, 32 above
template <typename K, typename... KernelArgs>
void launch_rows(K rows16, K rows32, int A, long long blocks, hipStream_t s, KernelArgs... args) {
  hipLaunchKernelGGL(A <= 16 ? rows16 : rows32, dim3((unsigned)blocks), dim3(HEAD_WAVES * 64), 0, s, args...);
}

}  // namespace

extern "C" {

int h12learn_ppo_head_rows(void) { return HEAD_ROWS; }

int h12learn_ppo_head_max_actions(void) { return HEAD_MAX_A; }

size_t h12learn_ppo_head_workspace_bytes(long long m, int A) { return workspace_bytes("ppo_head", m, A, 0); }

int h12learn_ppo_head(const h12learn_ppo_head_args* args, void* stream) {
  if (!args) return h12_learn_fail(H12LEARN_E_ARG, "ppo_head: args is null");
  const h12learn_ppo_head_args& p = *args;
  const Required required[] = {{p.mean, "mean"}, {p.value, "value"}, {p.std_param, "std_param"},
                               {p.old_log_prob, "old_log_prob"}, {p.advantages, "advantages"}, {p.returns, "returns"},
                               {p.target_values, "target_values"}, {p.old_mu, "old_mu"}, {p.old_sigma, "old_sigma"},
                               {p.actions, "actions"}, {p.d_mean, "d_mean"}, {p.d_value, "d_value"},
                               {p.d_param, "d_param"}, {p.out, "out"}, {p.workspace, "workspace"}};
  if (const int rc = check_head("ppo_head", p, "B", p.B, required, 0)) return rc;
  if (p.B < 1 || (p.m != p.B && p.m != 2 * p.B))
    return h12_learn_fail(H12LEARN_E_ARG, "ppo_head: m = %lld is neither B nor 2 B (B = %lld)", p.m, p.B);
  if (p.std_kind != H12LEARN_PPO_STD_SCALAR && p.std_kind != H12LEARN_PPO_STD_LOG)
    return h12_learn_fail(H12LEARN_E_ARG, "ppo_head: std_kind = %d (H12LEARN_PPO_STD_SCALAR or _LOG)", p.std_kind);
  if (!(p.clip_param >= 0.0)) return h12_learn_fail(H12LEARN_E_ARG, "ppo_head: clip_param = %g (must be >= 0)", p.clip_param);
  if (p.lr && !(p.desired_kl > 0.0))
    return h12_learn_fail(H12LEARN_E_ARG, "ppo_head: desired_kl = %g with lr set (must be > 0)", p.desired_kl);

  const HeadScalars sc = {loss_scalars(p.clip_param, p.value_loss_coef, p.entropy_coef), (float)(p.desired_kl * 2.0),
                          (float)(p.desired_kl / 2.0)};
  const long long blocks = head_blocks(p.m);
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)p.workspace;
  launch_rows(ppo_head_rows_kernel<16>, ppo_head_rows_kernel<32>, p.A, blocks, s, p, sc, partial);
  HEAD_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ppo_head_fold_kernel, dim3(1), dim3(FOLD_THREADS), 0, s, p, sc, (const double*)partial,
                     (int)blocks);
  HEAD_HIP_TRY(hipGetLastError());
  return H12LEARN_OK;
}

int h12learn_cleanrl_head_rows(void) { return HEAD_ROWS; }

size_t h12learn_cleanrl_head_workspace_bytes(long long m, int A) {
  return workspace_bytes("cleanrl_head", m, A, CLEAN_ADV);
}

int h12learn_cleanrl_head(const h12learn_cleanrl_head_args* args, void* stream) {
  if (!args) return h12_learn_fail(H12LEARN_E_ARG, "cleanrl_head: args is null");
  const h12learn_cleanrl_head_args& p = *args;
  const Required required[] = {{p.mean, "mean"}, {p.value, "value"}, {p.logstd, "logstd"},
                               {p.old_log_prob, "old_log_prob"}, {p.advantages, "advantages"},
                               {p.returns_n, "returns_n"}, {p.values_n, "values_n"}, {p.actions, "actions"},
                               {p.value_mean, "value_mean"}, {p.value_var, "value_var"}, {p.d_mean, "d_mean"},
                               {p.d_value, "d_value"}, {p.d_logstd, "d_logstd"}, {p.out, "out"},
                               {p.workspace, "workspace"}};
  if (const int rc = check_head("cleanrl_head", p, "m", p.m, required, CLEAN_ADV)) return rc;
  if (p.norm_adv && p.m < 2)
    return h12_learn_fail(H12LEARN_E_ARG, "cleanrl_head: m = %lld with norm_adv (the std of one advantage is NaN)", p.m);
  if (!(p.clip_coef >= 0.0)) return h12_learn_fail(H12LEARN_E_ARG, "cleanrl_head: clip_coef = %g (must be >= 0)", p.clip_coef);
  if (!(p.value_eps >= 0.0)) return h12_learn_fail(H12LEARN_E_ARG, "cleanrl_head: value_eps = %g (must be >= 0)", p.value_eps);

  const CleanScalars sc = {loss_scalars(p.clip_coef, p.vf_coef, p.ent_coef), (float)p.value_eps};
  const long long blocks = head_blocks(p.m);
  hipStream_t s = (hipStream_t)stream;
  double* apart = (double*)p.workspace;
  double* partial = apart + (size_t)blocks * CLEAN_ADV;
  if (p.norm_adv) {
    hipLaunchKernelGGL(cleanrl_adv_kernel, dim3((unsigned)blocks), dim3(64), 0, s, p, apart);
    HEAD_HIP_TRY(hipGetLastError());
  }
  launch_rows(cleanrl_head_rows_kernel<16>, cleanrl_head_rows_kernel<32>, p.A, blocks, s, p, sc, (const double*)apart,
              partial, (int)blocks);
  HEAD_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(cleanrl_head_fold_kernel, dim3(1), dim3(FOLD_THREADS), 0, s, p, sc, (const double*)partial,
                     (int)blocks);
  HEAD_HIP_TRY(hipGetLastError());
  return H12LEARN_OK;
}

}  // extern "C"

