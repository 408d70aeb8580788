// h12_policy_train.hip: the training side of the fused policy MLP (include/h12learn.h, h12learn_mlp_*_train / _backward).
//
//   h12learn_mlp_pack_t          W[out][in] -> the tiled layout of h12_policy.hip over W^T (the dgrad's B operand)
//   h12learn_mlp_forward_train   every Linear/ELU layer of ONE network in one launch; also stores every hidden h_l
//   h12learn_mlp_backward        dZ_{L-1} = dY; dH_l = dZ_{l+1} W_{l+1}; dZ_l = dH_l * f'(h_l), the chain in LDS, one
//                                launch; per-block bias-gradient partials, folded in block order by a second launch
//
// Same design as h12_policy.hip (read its header first): v_mfma_f32_16x16x4_f32, K walked in groups of 16, fragments
// fetched MLP_DEPTH groups ahead, activations in two LDS buffers used alternately.  The forward reads the SAME packed
// weights as h12learn_mlp_forward and issues the same MFMA sequence per accumulator (bias, then g ascending, e = 0..3),
// so its y is bit-identical to the inference kernel's.
//
// Row tile: TR_ROWS = 32, two 16-row sub-tiles that share every B fragment.  A minibatch of 24 576 rows is 768 blocks
// (3 per CU) and every block streams the network once from L2: half the weight traffic of the 16-row inference tile,
// which exists to fill the chip at 4096 rows.  LDS: 32 x (468 + 516) floats = 123 KiB for 451-512-256-128, one block
// per CU; 64 rows do not fit.  Widths are limited to TR_MAX_WIDTH = 512 (129 KiB).
//
// dgrad.  dH_l[r][i] = sum_j dZ_{l+1}[r][j] W_{l+1}[j][i] is a "layer" with K = dims[l+2], output width dims[l+1] and
// no bias over the transposed pack: lane l holds W[k][col l & 15].  The accumulator starts at zero and the k order is
// that of the forward (g ascending, e = 0..3, the four k = 16 g + 4 q + e of one MFMA): a function of the layer's
// width alone.  f'(h) = h > 0 ? 1 : h + 1 is ELU's derivative taken from its output.  Rows past n are zero on load
// (dY) and masked on store; the padding columns of dZ are exactly zero (zero rows of the transposed pack).
//
// Bias gradients.  After a layer's dZ tile is complete in LDS, thread c sums column c over the 32 rows in row order
// and writes the partial to workspace[block][column]; bias_fold_kernel adds the partials of a column in block-index
// order.  No atomics: db is bitwise reproducible.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/h12learn.h"

// defined in h12_learn.hip: records the calling thread's h12learn_last_error message and returns code
int h12_learn_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3), visibility("hidden")));

namespace {

constexpr int TR_SUB = 2;             // 16-row sub-tiles of a block
constexpr int TR_ROWS = 16 * TR_SUB;  // rows of a block
constexpr int TR_WAVES = 4;
constexpr int TR_THREADS = TR_WAVES * 64;
constexpr int TR_TC = 4;     // output tiles a wave accumulates at a time
constexpr int TR_DEPTH = 4;  // k-groups fetched ahead of the MFMAs
constexpr int TR_MAX_WIDTH = 512;
constexpr int TR_LD_PAD = 4;
constexpr int PACK_BLOCK = 256;
constexpr int FOLD_BLOCK = 64;
constexpr int FOLD_UNROLL = 32;
constexpr size_t LDS_DEFAULT_LIMIT = 64 * 1024;
constexpr int LDS_MOST = TR_ROWS * 2 * (TR_MAX_WIDTH + TR_LD_PAD) * (int)sizeof(float);

using f32x4 = __attribute__((ext_vector_type(4))) float;

__host__ __device__ inline int pad16(int v) { return (v + 15) & ~15; }

// floats of one packed layer of h12learn_mlp_pack: padded weights followed by the padded bias
__host__ __device__ inline size_t layer_floats(int in, int out) {
  return (size_t)pad16(in) * (size_t)pad16(out) + (size_t)pad16(out);
}

// floats of one layer of the transposed pack: padded weights only
__host__ __device__ inline size_t layer_floats_t(int in, int out) { return (size_t)pad16(in) * (size_t)pad16(out); }

__global__ __launch_bounds__(PACK_BLOCK) void mlp_pack_t_kernel(h12learn_mlp_desc desc, float* packed_t,
                                                                 size_t total) {
  size_t i = (size_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
  if (i >= total) return;
  const size_t dst = i;
  const h12learn_mlp_net& net = desc.nets[0];
  for (int l = 0; l < net.n_layers; ++l) {
    const int in = net.dims[l], out = net.dims[l + 1];
    const size_t wsz = layer_floats_t(in, out);
    if (i < wsz) {
      const int kg = pad16(out) / 16;  // K of the dgrad is the layer's output width
      const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
      const size_t tg = i >> 8;
      const int g = (int)(tg % (size_t)kg), t = (int)(tg / (size_t)kg);
      const int c = 16 * t + (lane & 15), k = 16 * g + 4 * (lane >> 4) + e;  // W^T[c][k] = W[k][c]
      packed_t[dst] = (c < in && k < out) ? net.W[l][(size_t)k * (size_t)in + c] : 0.f;
      return;
    }
    i -= wsz;
  }
}

__device__ __forceinline__ float elu1(float v) { return v > 0.f ? v : expm1f(v); }

// NT output tiles (t0, t0 + 4, ...) of one layer for this wave over both 16-row sub-tiles: every B fragment is
// fetched once and multiplies the A fragment of either sub-tile.  bp == nullptr: the accumulators start at zero.
// side = pre(column, row in the block) is fetched for every element BEFORE the k loop (the backward's saved
// activation: its global-memory latency hides behind the MFMAs); epi(column, row, value, side) receives every element.
template <int NT, class Pre, class Epi>
__device__ __forceinline__ void tr_tiles(const float* __restrict__ wp, const float* __restrict__ bp,
                                         const float* arow, int ldin, int kg, int t0, Pre pre, Epi epi) {
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, q = lane >> 4;
  f32x4 acc[NT][TR_SUB];
  const f32x4* bsrc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int t = t0 + TR_WAVES * i;
    const float b = bp ? bp[16 * t + col] : 0.f;
#pragma unroll
    for (int s = 0; s < TR_SUB; ++s) acc[i][s] = f32x4{b, b, b, b};
    bsrc[i] = reinterpret_cast<const f32x4*>(wp + (size_t)t * (size_t)kg * 256) + lane;
  }
  float side[NT][TR_SUB][4];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
#pragma unroll
    for (int s = 0; s < TR_SUB; ++s) {
#pragma unroll
      for (int r = 0; r < 4; ++r) side[i][s][r] = pre(16 * (t0 + TR_WAVES * i) + col, 16 * s + 4 * q + r);
    }
  }
  f32x4 aq[TR_DEPTH][TR_SUB], bq[TR_DEPTH][NT];
#pragma unroll
  for (int d = 0; d < TR_DEPTH; ++d) {
    const int gl = d < kg ? d : kg - 1;  // past the end: a harmless reload of the last group
#pragma unroll
    for (int s = 0; s < TR_SUB; ++s) aq[d][s] = *reinterpret_cast<const f32x4*>(arow + 16 * s * ldin + 16 * gl);
#pragma unroll
    for (int i = 0; i < NT; ++i) bq[d][i] = bsrc[i][(size_t)gl * 64];
  }
  for (int g = 0; g < kg; g += TR_DEPTH) {
#pragma unroll
    for (int d = 0; d < TR_DEPTH; ++d) {
      if (g + d < kg) {  // wave-uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int i = 0; i < NT; ++i) {
#pragma unroll
            for (int s = 0; s < TR_SUB; ++s)
              acc[i][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[d][s][e], bq[d][i][e], acc[i][s], 0, 0, 0);
          }
        }
      }
      const int gl = g + d + TR_DEPTH < kg ? g + d + TR_DEPTH : kg - 1;
#pragma unroll
      for (int s = 0; s < TR_SUB; ++s) aq[d][s] = *reinterpret_cast<const f32x4*>(arow + 16 * s * ldin + 16 * gl);
#pragma unroll
      for (int i = 0; i < NT; ++i) bq[d][i] = bsrc[i][(size_t)gl * 64];
    }
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int j = 16 * (t0 + TR_WAVES * i) + col;
#pragma unroll
    for (int s = 0; s < TR_SUB; ++s) {
#pragma unroll
      for (int r = 0; r < 4; ++r) epi(j, 16 * s + 4 * q + r, acc[i][s][r], side[i][s][r]);
    }
  }
}

// One layer for this wave's output tiles t = wave, wave + 4, ..., TR_TC of them at a time, then 2, then 1.
// hin: [TR_ROWS][ldin] LDS image, K = 16 * kg columns of it.
template <class Pre, class Epi>
__device__ __forceinline__ void tr_layer(const float* __restrict__ wp, const float* __restrict__ bp, const float* hin,
                                         int ldin, int kg, int tiles, Pre pre, Epi epi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* arow = hin + (lane & 15) * ldin + 4 * (lane >> 4);
  int t0 = wave;
  int mine = tiles > wave ? (tiles - wave + TR_WAVES - 1) / TR_WAVES : 0;  // this wave's tiles
  for (; mine >= TR_TC; mine -= TR_TC, t0 += TR_WAVES * TR_TC) tr_tiles<TR_TC>(wp, bp, arow, ldin, kg, t0, pre, epi);
  static_assert(TR_TC == 4, "the remainder below is 2, then 1");
  if (mine >= 2) {
    tr_tiles<2>(wp, bp, arow, ldin, kg, t0, pre, epi);
    mine -= 2, t0 += TR_WAVES * 2;
  }
  if (mine >= 1) tr_tiles<1>(wp, bp, arow, ldin, kg, t0, pre, epi);
}

// The [TR_ROWS][16 * ceil(d / 16)] tile of src [n][d] at row0 into an LDS image: zero in the padding columns and in
// the rows past n.  A thread takes a column: its loads are in flight together.
__device__ __forceinline__ void load_tile(const float* __restrict__ src, int d, long long row0, long long n, float* buf,
                                          int ld) {
  const int kpad = pad16(d);
  for (int c = threadIdx.x; c < kpad; c += TR_THREADS) {
    float v[TR_ROWS];
#pragma unroll
    for (int r = 0; r < TR_ROWS; ++r) v[r] = (c < d && row0 + r < n) ? src[(size_t)(row0 + r) * (size_t)d + c] : 0.f;
#pragma unroll
    for (int r = 0; r < TR_ROWS; ++r) buf[r * ld + c] = v[r];
  }
}

struct train_ptrs {
  float* p[H12LEARN_MLP_MAX_LAYERS];
};
struct train_cptrs {
  const float* p[H12LEARN_MLP_MAX_LAYERS];
};

__global__ __launch_bounds__(TR_THREADS) void mlp_forward_train_kernel(h12learn_mlp_desc desc,
                                                                       const float* __restrict__ packed,
                                                                       const float* __restrict__ x, long long n,
                                                                       float* __restrict__ y, train_ptrs hs, int ld0,
                                                                       int ld1) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* hin = lds;
  float* hout = lds + TR_ROWS * ld0;
  int ldin = ld0, ldout = ld1;
  const h12learn_mlp_net& net = desc.nets[0];
  const long long row0 = (long long)blockIdx.x * TR_ROWS;

  load_tile(x, desc.d_in, row0, n, hin, ldin);
  __syncthreads();
  const auto no_side = [](int, int) { return 0.f; };

  const float* wp = packed;
  for (int l = 0; l < net.n_layers; ++l) {
    const int in = net.dims[l], out = net.dims[l + 1];
    const int kg = pad16(in) / 16, tiles = pad16(out) / 16;
    const float* bp = wp + (size_t)pad16(in) * (size_t)pad16(out);
    if (l + 1 < net.n_layers) {
      float* hg = hs.p[l];
      float* ho = hout;
      const int ldo = ldout;
      tr_layer(wp, bp, hin, ldin, kg, tiles, no_side, [=](int j, int row, float v, float) {
        const float h = elu1(v);
        ho[row * ldo + j] = h;
        if (j < out && row0 + row < n) hg[(size_t)(row0 + row) * (size_t)out + j] = h;
      });
    } else {
      tr_layer(wp, bp, hin, ldin, kg, tiles, no_side, [=](int j, int row, float v, float) {
        if (j < out && row0 + row < n) y[(size_t)(row0 + row) * (size_t)out + j] = v;
      });
    }
    wp = bp + pad16(out);
    __syncthreads();
    float* tp = hin;
    hin = hout, hout = tp;
    const int tl = ldin;
    ldin = ldout, ldout = tl;
  }
}

// Grid: row tiles.  cur holds dZ_l ([TR_ROWS][ld], padding columns and rows past n zero); per layer, top down: the
// bias-gradient partial of dZ_l, then dZ_{l-1} = (dZ_l W_l) * f'(h_{l-1}) into the other buffer and to dz[l - 1].
__global__ __launch_bounds__(TR_THREADS) void mlp_backward_kernel(h12learn_mlp_desc desc,
                                                                  const float* __restrict__ packed_t,
                                                                  const float* __restrict__ dy, train_cptrs hs,
                                                                  long long n, train_ptrs dzs, float* __restrict__ dx,
                                                                  float* __restrict__ partial, int tot, int ld0,
                                                                  int ld1) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* cur = lds;
  float* nxt = lds + TR_ROWS * ld0;
  int ldc = ld0, ldn = ld1;
  const h12learn_mlp_net& net = desc.nets[0];
  const int L = net.n_layers;
  const long long row0 = (long long)blockIdx.x * TR_ROWS;
  float* part = partial + (size_t)blockIdx.x * (size_t)tot;

  load_tile(dy, net.dims[L], row0, n, cur, ldc);
  __syncthreads();

  // offsets of layer L - 1: the transposed pack and the bias-gradient columns
  size_t woff = 0;
  int boff = 0;
  for (int l = 0; l + 1 < L; ++l) {
    woff += layer_floats_t(net.dims[l], net.dims[l + 1]);
    boff += net.dims[l + 1];
  }
  for (int l = L - 1; l >= 0; --l) {
    const int in = net.dims[l], out = net.dims[l + 1];
    for (int c = threadIdx.x; c < out; c += TR_THREADS) {
      float s = cur[c];
#pragma unroll
      for (int r = 1; r < TR_ROWS; ++r) s += cur[r * ldc + c];
      part[boff + c] = s;
    }
    const int kg = pad16(out) / 16, tiles = pad16(in) / 16;
    const float* wp = packed_t + woff;
    if (l > 0) {
      const float* hg = hs.p[l - 1];
      float* dzg = dzs.p[l - 1];
      float* o = nxt;
      const int ldo = ldn;
      tr_layer(
          wp, nullptr, cur, ldc, kg, tiles,
          [=](int j, int row) { return (j < in && row0 + row < n) ? hg[(size_t)(row0 + row) * (size_t)in + j] : 0.f; },
          [=](int j, int row, float v, float h) {
            const float dz = v * (h > 0.f ? 1.f : h + 1.f);
            o[row * ldo + j] = dz;
            if (j < in && row0 + row < n) dzg[(size_t)(row0 + row) * (size_t)in + j] = dz;
          });
      woff -= layer_floats_t(net.dims[l - 1], in);
      boff -= in;
    } else if (dx) {
      tr_layer(wp, nullptr, cur, ldc, kg, tiles, [](int, int) { return 0.f; }, [=](int j, int row, float v, float) {
        if (j < in && row0 + row < n) dx[(size_t)(row0 + row) * (size_t)in + j] = v;
      });
    }
    __syncthreads();
    float* tp = cur;
    cur = nxt, nxt = tp;
    const int tl = ldc;
    ldc = ldn, ldn = tl;
  }
}

// db[l][j] = the partials of column (l, j) added in block-index order
__global__ __launch_bounds__(FOLD_BLOCK) void bias_fold_kernel(h12learn_mlp_desc desc,
                                                               const float* __restrict__ partial, long long blocks,
                                                               int tot, train_ptrs db) {
  int c = blockIdx.x * FOLD_BLOCK + threadIdx.x;
  if (c >= tot) return;
  // FOLD_UNROLL independent loads in flight, then added in block order: the order of the sum is b = 0, 1, 2, ...
  float s = partial[c];
  long long b = 1;
  for (; b + FOLD_UNROLL <= blocks; b += FOLD_UNROLL) {
    float v[FOLD_UNROLL];
#pragma unroll
    for (int i = 0; i < FOLD_UNROLL; ++i) v[i] = partial[(size_t)(b + i) * (size_t)tot + c];
#pragma unroll
    for (int i = 0; i < FOLD_UNROLL; ++i) s += v[i];
  }
  for (; b < blocks; ++b) s += partial[(size_t)b * (size_t)tot + c];
  const h12learn_mlp_net& net = desc.nets[0];
  for (int l = 0; l < net.n_layers; ++l) {
    if (c < net.dims[l + 1]) {
      db.p[l][c] = s;
      return;
    }
    c -= net.dims[l + 1];
  }
}

int check_train_desc(const h12learn_mlp_desc* desc, const char* fn) {
  if (!desc) return h12_learn_fail(H12LEARN_E_ARG, "%s: desc is null", fn);
  if (desc->n_nets != 1) return h12_learn_fail(H12LEARN_E_ARG, "%s: n_nets = %d (must be 1)", fn, desc->n_nets);
  if (desc->norm_kind != H12LEARN_MLP_NORM_NONE)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: norm_kind = %d (H12LEARN_MLP_NORM_NONE only)", fn, desc->norm_kind);
  if (desc->d_in < 1 || desc->d_in > TR_MAX_WIDTH)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: d_in = %d (1..%d)", fn, desc->d_in, TR_MAX_WIDTH);
  const h12learn_mlp_net& net = desc->nets[0];
  if (net.n_layers < 1 || net.n_layers > H12LEARN_MLP_MAX_LAYERS)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: nets[0].n_layers = %d (1..%d)", fn, net.n_layers,
                          H12LEARN_MLP_MAX_LAYERS);
  if (net.dims[0] != desc->d_in)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: nets[0].dims[0] = %d differs from d_in = %d", fn, net.dims[0],
                          desc->d_in);
  for (int l = 1; l <= net.n_layers; ++l)
    if (net.dims[l] < 1 || net.dims[l] > TR_MAX_WIDTH)
      return h12_learn_fail(H12LEARN_E_ARG, "%s: nets[0].dims[%d] = %d (1..%d)", fn, l, net.dims[l], TR_MAX_WIDTH);
  return H12LEARN_OK;
}

int check_rows(long long n, const char* fn) {
  if (n < 1) return h12_learn_fail(H12LEARN_E_ARG, "%s: n = %lld (must be >= 1)", fn, n);
  if ((n + TR_ROWS - 1) / TR_ROWS > 0x7fffffffLL)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: n = %lld exceeds the grid", fn, n);
  return H12LEARN_OK;
}

int total_columns(const h12learn_mlp_net& net) {
  int tot = 0;
  for (int l = 0; l < net.n_layers; ++l) tot += net.dims[l + 1];
  return tot;
}

// More than 64 KiB of dynamic LDS: the first such call of a kernel raises its limit (an attribute of the function, no
// stream work).  That call must not be made while the stream is capturing.
int raise_lds_limit(const void* kernel, bool* raised, size_t lds_bytes, hipStream_t stream, const char* fn) {
  if (lds_bytes <= LDS_DEFAULT_LIMIT || *raised) return H12LEARN_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &st) != hipSuccess) {
    (void)hipGetLastError();
    st = hipStreamCaptureStatusNone;
  }
  if (st != hipStreamCaptureStatusNone)
    return h12_learn_fail(H12LEARN_E_HIP, "%s: the first call that needs more than 64 KiB of LDS must be made outside "
                          "a stream capture (warm up first)", fn);
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MOST);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return h12_learn_fail(H12LEARN_E_HIP, "%s: LDS limit: %s", fn, hipGetErrorString(e));
  }
  *raised = true;
  return H12LEARN_OK;
}

}  // namespace

extern "C" {

int h12learn_mlp_train_rows(void) { return TR_ROWS; }

int h12learn_mlp_train_max_width(void) { return TR_MAX_WIDTH; }

size_t h12learn_mlp_packed_t_bytes(const h12learn_mlp_desc* desc) {
  if (check_train_desc(desc, "mlp_packed_t_bytes") != H12LEARN_OK) return 0;
  size_t s = 0;
  for (int l = 0; l < desc->nets[0].n_layers; ++l)
    s += layer_floats_t(desc->nets[0].dims[l], desc->nets[0].dims[l + 1]);
  return s * sizeof(float);
}

int h12learn_mlp_pack_t(const h12learn_mlp_desc* desc, float* packed_t, void* stream) {
  int rc = check_train_desc(desc, "mlp_pack_t");
  if (rc != H12LEARN_OK) return rc;
  for (int l = 0; l < desc->nets[0].n_layers; ++l)
    if (!desc->nets[0].W[l]) return h12_learn_fail(H12LEARN_E_ARG, "mlp_pack_t: nets[0].W[%d] is null", l);
  if (!packed_t) return h12_learn_fail(H12LEARN_E_ARG, "mlp_pack_t: packed_t is null");
  if (((uintptr_t)packed_t & 15) != 0)
    return h12_learn_fail(H12LEARN_E_ARG, "mlp_pack_t: packed_t not 16-byte aligned");
  const size_t total = h12learn_mlp_packed_t_bytes(desc) / sizeof(float);
  const size_t blocks = (total + PACK_BLOCK - 1) / PACK_BLOCK;
  hipLaunchKernelGGL(mlp_pack_t_kernel, dim3((unsigned)blocks), dim3(PACK_BLOCK), 0, (hipStream_t)stream, *desc,
                     packed_t, total);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "mlp_pack_t launch: %s", hipGetErrorString(e));
  return H12LEARN_OK;
}

int h12learn_mlp_forward_train(const h12learn_mlp_desc* desc, const float* packed, const float* x, long long n,
                               float* y, float* const* h, void* stream) {
  const char* fn = "mlp_forward_train";
  int rc = check_train_desc(desc, fn);
  if (rc != H12LEARN_OK) return rc;
  if (!packed) return h12_learn_fail(H12LEARN_E_ARG, "%s: packed is null", fn);
  if (((uintptr_t)packed & 15) != 0) return h12_learn_fail(H12LEARN_E_ARG, "%s: packed not 16-byte aligned", fn);
  if (!x) return h12_learn_fail(H12LEARN_E_ARG, "%s: x is null", fn);
  if ((rc = check_rows(n, fn)) != H12LEARN_OK) return rc;
  if (!y) return h12_learn_fail(H12LEARN_E_ARG, "%s: y is null", fn);
  const h12learn_mlp_net& net = desc->nets[0];
  train_ptrs hs = {};
  if (net.n_layers > 1 && !h) return h12_learn_fail(H12LEARN_E_ARG, "%s: h is null", fn);
  for (int l = 0; l + 1 < net.n_layers; ++l) {
    if (!h[l]) return h12_learn_fail(H12LEARN_E_ARG, "%s: h[%d] is null", fn, l);
    hs.p[l] = h[l];
  }
  // buffer 0 holds the input and the outputs of the odd layers, buffer 1 the others
  int w0 = pad16(desc->d_in), w1 = 16;
  for (int l = 0; l + 1 < net.n_layers; ++l) {
    int& dst = (l & 1) ? w0 : w1;
    if (pad16(net.dims[l + 1]) > dst) dst = pad16(net.dims[l + 1]);
  }
  const int ld0 = w0 + TR_LD_PAD, ld1 = w1 + TR_LD_PAD;
  const size_t lds_bytes = (size_t)TR_ROWS * (size_t)(ld0 + ld1) * sizeof(float);
  static bool raised = false;
  rc = raise_lds_limit(reinterpret_cast<const void*>(mlp_forward_train_kernel), &raised, lds_bytes,
                       (hipStream_t)stream, fn);
  if (rc != H12LEARN_OK) return rc;
  const long long tiles = (n + TR_ROWS - 1) / TR_ROWS;
  hipLaunchKernelGGL(mlp_forward_train_kernel, dim3((unsigned)tiles), dim3(TR_THREADS), lds_bytes,
                     (hipStream_t)stream, *desc, packed, x, n, y, hs, ld0, ld1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return H12LEARN_OK;
}

size_t h12learn_mlp_backward_workspace_bytes(const h12learn_mlp_desc* desc, long long n) {
  if (check_train_desc(desc, "mlp_backward_workspace_bytes") != H12LEARN_OK) return 0;
  if (check_rows(n, "mlp_backward_workspace_bytes") != H12LEARN_OK) return 0;
  const size_t blocks = (size_t)((n + TR_ROWS - 1) / TR_ROWS);
  return blocks * (size_t)total_columns(desc->nets[0]) * sizeof(float);
}

int h12learn_mlp_backward(const h12learn_mlp_desc* desc, const float* packed_t, const float* dy,
                          const float* const* h, long long n, float* const* dz, float* const* db, float* dx,
                          void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "mlp_backward";
  int rc = check_train_desc(desc, fn);
  if (rc != H12LEARN_OK) return rc;
  if (!packed_t) return h12_learn_fail(H12LEARN_E_ARG, "%s: packed_t is null", fn);
  if (((uintptr_t)packed_t & 15) != 0) return h12_learn_fail(H12LEARN_E_ARG, "%s: packed_t not 16-byte aligned", fn);
  if (!dy) return h12_learn_fail(H12LEARN_E_ARG, "%s: dy is null", fn);
  if ((rc = check_rows(n, fn)) != H12LEARN_OK) return rc;
  const h12learn_mlp_net& net = desc->nets[0];
  const int L = net.n_layers;
  train_cptrs hs = {};
  train_ptrs dzs = {}, dbs = {};
  if (L > 1 && !h) return h12_learn_fail(H12LEARN_E_ARG, "%s: h is null", fn);
  if (L > 1 && !dz) return h12_learn_fail(H12LEARN_E_ARG, "%s: dz is null", fn);
  if (!db) return h12_learn_fail(H12LEARN_E_ARG, "%s: db is null", fn);
  for (int l = 0; l + 1 < L; ++l) {
    if (!h[l]) return h12_learn_fail(H12LEARN_E_ARG, "%s: h[%d] is null", fn, l);
    if (!dz[l]) return h12_learn_fail(H12LEARN_E_ARG, "%s: dz[%d] is null", fn, l);
    hs.p[l] = h[l];
    dzs.p[l] = dz[l];
  }
  for (int l = 0; l < L; ++l) {
    if (!db[l]) return h12_learn_fail(H12LEARN_E_ARG, "%s: db[%d] is null", fn, l);
    dbs.p[l] = db[l];
  }
  const size_t need = h12learn_mlp_backward_workspace_bytes(desc, n);
  if (!workspace) return h12_learn_fail(H12LEARN_E_ARG, "%s: workspace is null", fn);
  if (workspace_bytes < need)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: workspace_bytes = %zu, %zu needed", fn, workspace_bytes, need);
  // buffer 0 holds dZ_{L-1}, dZ_{L-3}, ..., buffer 1 the others
  int w0 = 16, w1 = 16;
  for (int l = 0; l < L; ++l) {
    int& dst = ((L - 1 - l) & 1) ? w1 : w0;
    if (pad16(net.dims[l + 1]) > dst) dst = pad16(net.dims[l + 1]);
  }
  const int ld0 = w0 + TR_LD_PAD, ld1 = w1 + TR_LD_PAD;
  const size_t lds_bytes = (size_t)TR_ROWS * (size_t)(ld0 + ld1) * sizeof(float);
  static bool raised = false;
  rc = raise_lds_limit(reinterpret_cast<const void*>(mlp_backward_kernel), &raised, lds_bytes, (hipStream_t)stream,
                       fn);
  if (rc != H12LEARN_OK) return rc;
  const long long tiles = (n + TR_ROWS - 1) / TR_ROWS;
  const int tot = total_columns(net);
  hipLaunchKernelGGL(mlp_backward_kernel, dim3((unsigned)tiles), dim3(TR_THREADS), lds_bytes, (hipStream_t)stream,
                     *desc, packed_t, dy, hs, n, dzs, dx, (float*)workspace, tot, ld0, ld1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  hipLaunchKernelGGL(bias_fold_kernel, dim3((unsigned)((tot + FOLD_BLOCK - 1) / FOLD_BLOCK)), dim3(FOLD_BLOCK), 0,
                     (hipStream_t)stream, *desc, (const float*)workspace, tiles, tot, dbs);
  e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "%s fold launch: %s", fn, hipGetErrorString(e));
  return H12LEARN_OK;
}

}  // extern "C"
