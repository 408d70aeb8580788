// h12_rnd.hip: the per-env-step work of Random Network Distillation (h12env/rnd.py) in two
// launches (include/h12learn.h, h12learn_rnd_*).
//
//   h12learn_rnd_reward   state normaliser + target network + predictor network + the row norm of their difference
//   h12learn_rnd_finish   the discounted-variation reward normaliser, the weight and the sum with the env's reward
//
// Reward.  Grid (row tiles); a block of 4 waves owns RND_ROWS = 16 rows.  It loads and normalises its input tile once
// into an LDS image X of its own, which both networks' first layers read; the hidden activations alternate between two
// further images A (outputs of layers 0, 2, ..) and B (layers 1, 3, ..), as in h12_policy.hip.  The layers run through
// mlp::layer of h12_mlp_core.h on the pack of h12learn_mlp_pack: an embedding element has the core's summation order
// and the bits h12learn_mlp_forward gives.  The target runs first and leaves its embedding in a fourth image E; the
// predictor's last layer replaces each element by target - predictor (an element belongs to one lane in both passes).
// Columns past the output width are zero in both (zero weight rows, zero bias), so they add nothing below.
// The squares are then summed in a fixed order: the 16 lanes of a tile (xor butterfly 8, 4, 2, 1), the tiles of a wave
// in tile order, the four waves in wave order through LDS.  Nothing in it depends on n or on the grid.
//
// Finish.  ONE block of FIN_THREADS threads: thread t folds elements t, t + FIN_THREADS, .. in index order, the threads
// of a wave by an xor butterfly, the waves in wave order; all fp32.  The mean pass and the variance pass (around that
// mean: population variance) are two such folds.  The same inputs give the same bits.
#include "h12_mlp_core.h"

namespace {

using namespace mlp;

constexpr int RND_ROWS = 16;
constexpr int RND_MAX_WIDTH = 1024;          // any width, as h12learn_mlp_forward
constexpr size_t RND_LDS_MOST = 160 * 1024;  // a CU's LDS
constexpr int FIN_THREADS = 1024;

__host__ __device__ inline size_t rnd_net_floats(const h12learn_mlp_net& net) {
  size_t s = 0;
  for (int l = 0; l < net.n_layers; ++l) s += layer_floats(net.dims[l], net.dims[l + 1]);
  return s;
}

struct rnd_outs {
  float* err;
  float* xn;
  float* emb[2];
};

__global__ __launch_bounds__(THREADS) void rnd_reward_kernel(h12learn_mlp_desc desc, const float* __restrict__ packed,
                                                             const float* __restrict__ x, long long n, rnd_outs outs,
                                                             int ldx, int lda, int ldb, int lde) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* bufx = lds;
  float* bufa = bufx + RND_ROWS * ldx;
  float* bufb = bufa + RND_ROWS * lda;
  float* bufe = bufb + RND_ROWS * ldb;
  float* part = bufe + RND_ROWS * lde;  // [WAVES][RND_ROWS]
  const long long row0 = (long long)blockIdx.x * RND_ROWS;

  // the normalised input tile: the loop of mlp_forward_kernel (same expression, same bits), and the rows leave to xn
  const int d_in = desc.d_in, k0 = pad16(d_in);
  for (int c = threadIdx.x; c < k0; c += THREADS) {
    float v[RND_ROWS];
#pragma unroll
    for (int r = 0; r < RND_ROWS; ++r)
      v[r] = (c < d_in && row0 + r < n) ? x[(size_t)(row0 + r) * (size_t)d_in + c] : 0.f;
    if (c < d_in && desc.norm_kind != H12LEARN_MLP_NORM_NONE) {
      const float m = desc.norm_mean[c];
      const float sc = desc.norm_kind == H12LEARN_MLP_NORM_VAR ? sqrtf(desc.norm_scale[c] + desc.norm_eps)
                                                               : desc.norm_scale[c] + desc.norm_eps;
#pragma unroll
      for (int r = 0; r < RND_ROWS; ++r)
        if (row0 + r < n) v[r] = (v[r] - m) / sc;  // rows past n stay zero
    }
#pragma unroll
    for (int r = 0; r < RND_ROWS; ++r) bufx[r * ldx + c] = v[r];
    if (outs.xn && c < d_in) {
#pragma unroll
      for (int r = 0; r < RND_ROWS; ++r)
        if (row0 + r < n) outs.xn[(size_t)(row0 + r) * (size_t)d_in + c] = v[r];
    }
  }
  __syncthreads();

  const int out = desc.nets[0].dims[desc.nets[0].n_layers];  // == the target's (checked on the host)
  for (int pass = 0; pass < 2; ++pass) {
    const int nidx = 1 - pass;  // the target (nets[1]) first
    const h12learn_mlp_net& net = desc.nets[nidx];
    const float* wp = packed + (nidx ? rnd_net_floats(desc.nets[0]) : 0);
    float* y = outs.emb[nidx];
    const float* hin = bufx;
    int ldin = ldx;
    for (int l = 0; l < net.n_layers; ++l) {
      const int in = net.dims[l], wout = net.dims[l + 1];
      const int kg = pad16(in) / 16, ntiles = pad16(wout) / 16;
      const float* bp = wp + (size_t)pad16(in) * (size_t)pad16(wout);
      __builtin_assume(bp != nullptr);
      const bool last = l == net.n_layers - 1;
      float* hout = (l & 1) ? bufb : bufa;  // image l + 1
      const int ldout = (l & 1) ? ldb : lda;
      layer<1>(wp, bp, hin, ldin, kg, ntiles, no_side(), [=](int j, int row, float v, float) {
        if (!last) {
          hout[row * ldout + j] = elu1(v);
        } else {
          float* e = bufe + row * lde + j;
          *e = pass == 0 ? v : *e - v;
          if (y && j < out && row0 + row < n) y[(size_t)(row0 + row) * (size_t)out + j] = v;
        }
      });
      wp = bp + pad16(wout);
      __syncthreads();
      hin = hout;
      ldin = ldout;
    }
  }

  // sum of squares per row: lanes of a tile, tiles of a wave, waves
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, q = lane >> 4;
  float racc[4] = {0.f, 0.f, 0.f, 0.f};
  const int etiles = pad16(out) / 16;
  for (int t = wave; t < etiles; t += WAVES) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float d = bufe[(4 * q + r) * lde + 16 * t + col];
      float s = d * d;
      s += __shfl_xor(s, 8, 16);
      s += __shfl_xor(s, 4, 16);
      s += __shfl_xor(s, 2, 16);
      s += __shfl_xor(s, 1, 16);
      racc[r] += s;
    }
  }
  if (col == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave * RND_ROWS + 4 * q + r] = racc[r];
  }
  __syncthreads();
  if (threadIdx.x < RND_ROWS && row0 + threadIdx.x < n) {
    const int r = threadIdx.x;
    const float s = ((part[r] + part[RND_ROWS + r]) + part[2 * RND_ROWS + r]) + part[3 * RND_ROWS + r];
    outs.err[row0 + r] = sqrtf(s);
  }
}

// the block's sum of v: threads of a wave by butterfly, waves in wave order; every thread receives it
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // red may still be read from the fold before
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  float s = red[0];
  for (int w = 1; w < FIN_THREADS / 64; ++w) s += red[w];
  return s;
}

// Every operation separately rounded (no contraction): the products and sums torch's separate kernels round.
__global__ __launch_bounds__(FIN_THREADS) void rnd_finish_kernel(h12learn_rnd_finish_args a) {
#pragma clang fp contract(off)
  __shared__ float red[FIN_THREADS / 64];
  const long long n = a.n;
  const int t = threadIdx.x;
  const float w = *a.weight;
  float sd = 0.f;
  if (a.normalize) {
    const bool first = *a.first != 0;
    const long long count = *a.count;
    float s = 0.f;
    for (long long i = t; i < n; i += FIN_THREADS) {
      const float e = a.err[i];
      const float v = first ? e : a.avg[i] * a.gamma + e;
      a.avg[i] = v;
      s += v;
    }
    const bool live = count < a.until;  // uniform: read before thread 0 writes below (block_sum's barriers)
    const float mean_x = block_sum(s, red) / (float)n;
    float m2 = 0.f;
    for (long long i = t; i < n; i += FIN_THREADS) {  // a thread re-reads the elements it wrote
      const float d = a.avg[i] - mean_x;
      m2 += d * d;
    }
    const float var_x = block_sum(m2, red) / (float)n;
    float mean = *a.mean, var = *a.var;
    sd = *a.std;
    __syncthreads();  // every thread has read the statistics
    if (live) {  // EmpiricalNormalization.update
      const long long c2 = count + n;
      const float rate = (float)n / (float)c2;
      const float delta = mean_x - mean;
      mean += rate * delta;
      var += rate * (var_x - var + delta * (mean_x - mean));
      sd = sqrtf(var);
      if (t == 0) {
        *a.count = c2;
        *a.mean = mean;
        *a.var = var;
        *a.std = sd;
      }
    }
    if (t == 0) *a.first = 0;
  }
  for (long long i = t; i < n; i += FIN_THREADS) {
    const float e = a.err[i];
    const float v = (a.normalize && sd > 0.f) ? e / sd : e;
    const float r = v * w;
    a.intrinsic[i] = r;
    a.total[i] = a.ext_reward[i] + r;
  }
}

int check_ptr(const void* p, const char* name, size_t align) {
  if (!p) return h12_learn_fail(H12LEARN_E_ARG, "%s is null", name);
  if ((uintptr_t)p & (align - 1)) return h12_learn_fail(H12LEARN_E_ARG, "%s not %zu-byte aligned", name, align);
  return H12LEARN_OK;
}

}  // namespace

extern "C" {

int h12learn_rnd_reward(const h12learn_mlp_desc* desc, const float* packed, const float* x, long long n, float* err,
                        float* xn, float* const* emb, void* stream) {
  int rc = check_desc(desc, "rnd_reward", RND_MAX_WIDTH);
  if (rc != H12LEARN_OK) return rc;
  if (desc->n_nets != 2)
    return h12_learn_fail(H12LEARN_E_ARG, "rnd_reward: n_nets = %d (2: predictor, target)", desc->n_nets);
  if (desc->norm_kind != H12LEARN_MLP_NORM_NONE && (!desc->norm_mean || !desc->norm_scale))
    return h12_learn_fail(H12LEARN_E_ARG, "rnd_reward: norm_mean / norm_scale is null");
  const h12learn_mlp_net &p = desc->nets[0], &g = desc->nets[1];
  const int out = p.dims[p.n_layers];
  if (out != g.dims[g.n_layers])
    return h12_learn_fail(H12LEARN_E_ARG, "rnd_reward: the predictor's last width %d differs from the target's %d", out,
                          g.dims[g.n_layers]);
  if ((rc = check_ptr(packed, "rnd_reward: packed", 16)) != H12LEARN_OK) return rc;
  if ((rc = check_ptr(x, "rnd_reward: x", 4)) != H12LEARN_OK) return rc;
  if (n < 1) return h12_learn_fail(H12LEARN_E_ARG, "rnd_reward: n = %lld (must be >= 1)", n);
  if ((rc = check_ptr(err, "rnd_reward: err", 4)) != H12LEARN_OK) return rc;
  if (xn && ((uintptr_t)xn & 3)) return h12_learn_fail(H12LEARN_E_ARG, "rnd_reward: xn not 4-byte aligned");
  rnd_outs outs = {};
  outs.err = err;
  outs.xn = xn;
  if (emb) {
    for (int i = 0; i < 2; ++i) {
      if ((rc = check_ptr(emb[i], i ? "rnd_reward: emb[1]" : "rnd_reward: emb[0]", 4)) != H12LEARN_OK) return rc;
      outs.emb[i] = emb[i];
    }
  }
  const long long tiles = (n + RND_ROWS - 1) / RND_ROWS;
  if (tiles > 0x7fffffffLL) return h12_learn_fail(H12LEARN_E_ARG, "rnd_reward: n = %lld exceeds the grid", n);
  // the four images: X the input, A / B the odd / even hidden images of both networks, E the embedding
  int wa = 16, wb = 16;
  for (int i = 0; i < 2; ++i)
    for (int l = 0; l + 1 < desc->nets[i].n_layers; ++l) {
      int& dst = (l & 1) ? wb : wa;
      if (pad16(desc->nets[i].dims[l + 1]) > dst) dst = pad16(desc->nets[i].dims[l + 1]);
    }
  const int ldx = pad16(desc->d_in) + LD_PAD, lda = wa + LD_PAD, ldb = wb + LD_PAD, lde = pad16(out) + LD_PAD;
  const size_t lds_bytes = ((size_t)RND_ROWS * (size_t)(ldx + lda + ldb + lde) + WAVES * RND_ROWS) * sizeof(float);
  if (lds_bytes > RND_LDS_MOST)
    return h12_learn_fail(H12LEARN_E_ARG, "rnd_reward: these widths need %zu bytes of LDS (input, two hidden images and "
                          "the embedding, 16 rows each), a block has %zu", lds_bytes, RND_LDS_MOST);
  static bool raised = false;
  rc = raise_lds_limit(reinterpret_cast<const void*>(rnd_reward_kernel), &raised, (int)RND_LDS_MOST, lds_bytes,
                       (hipStream_t)stream, "rnd_reward");
  if (rc != H12LEARN_OK) return rc;
  hipLaunchKernelGGL(rnd_reward_kernel, dim3((unsigned)tiles), dim3(THREADS), lds_bytes, (hipStream_t)stream, *desc,
                     packed, x, n, outs, ldx, lda, ldb, lde);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "rnd_reward launch: %s", hipGetErrorString(e));
  return H12LEARN_OK;
}

int h12learn_rnd_finish(const h12learn_rnd_finish_args* a, void* stream) {
  if (!a) return h12_learn_fail(H12LEARN_E_ARG, "rnd_finish: args is null");
  if (a->n < 1) return h12_learn_fail(H12LEARN_E_ARG, "rnd_finish: n = %lld (must be >= 1)", a->n);
  int rc;
  if ((rc = check_ptr(a->err, "rnd_finish: err", 4)) != H12LEARN_OK) return rc;
  if ((rc = check_ptr(a->ext_reward, "rnd_finish: ext_reward", 4)) != H12LEARN_OK) return rc;
  if ((rc = check_ptr(a->weight, "rnd_finish: weight", 4)) != H12LEARN_OK) return rc;
  if ((rc = check_ptr(a->intrinsic, "rnd_finish: intrinsic", 4)) != H12LEARN_OK) return rc;
  if ((rc = check_ptr(a->total, "rnd_finish: total", 4)) != H12LEARN_OK) return rc;
  if (a->normalize) {
    if ((rc = check_ptr(a->avg, "rnd_finish: avg", 4)) != H12LEARN_OK) return rc;
    if ((rc = check_ptr(a->mean, "rnd_finish: mean", 4)) != H12LEARN_OK) return rc;
    if ((rc = check_ptr(a->var, "rnd_finish: var", 4)) != H12LEARN_OK) return rc;
    if ((rc = check_ptr(a->std, "rnd_finish: std", 4)) != H12LEARN_OK) return rc;
    if ((rc = check_ptr(a->count, "rnd_finish: count", 8)) != H12LEARN_OK) return rc;
    if ((rc = check_ptr(a->first, "rnd_finish: first", 4)) != H12LEARN_OK) return rc;
    if (!(a->gamma >= 0.f && a->gamma <= 1.f))
      return h12_learn_fail(H12LEARN_E_ARG, "rnd_finish: gamma = %g (0..1)", (double)a->gamma);
  }
  hipLaunchKernelGGL(rnd_finish_kernel, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, *a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "rnd_finish launch: %s", hipGetErrorString(e));
  return H12LEARN_OK;
}

}  // extern "C"
