// h12_policy.hip: fused policy MLP forward of libh12env.so (include/h12learn.h, h12learn_mlp_*).
//
//   h12learn_mlp_pack      torch-layout weights W[out][in], b[out] -> the tiled, zero-padded layout below (one launch)
//   h12learn_mlp_forward   normaliser + every Linear/ELU layer of up to 4 networks over one input, one launch
//
// Forward.  Grid (row tiles, networks); a block of 4 waves owns MLP_ROWS = 16 rows of x for one network.  16 rows and
// not 32: actor-only inference at 4096 rows then has 256 blocks, one per CU of the chip; with 32 rows half the CUs
// would idle.  The price is that every block streams the network's weights once from L2 for 16 rows only.
//
// A layer is Y[16][out] = H[16][K] W^T + b on v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered fmaf chain):
//   A = H: lane l holds H[row l & 15][k], B = W^T: lane l holds W[col l & 15][k], both with k chosen by q = l >> 4;
//   D: lane l, register r holds Y[row 4 q + r][col l & 15].
// The bias is the accumulator's start value.  K is walked in groups of 16: k-group g, MFMA step e (0..3) and lane
// quarter q multiply k = 16 g + 4 q + e, so a lane's four A values of a group are one 16-byte LDS read and its four B
// values one 16-byte global read.  The summation order of an output element is therefore
//   bias, then for g = 0.., for e = 0..3: the four k = 16 g + 4 q + e (q = 0..3) of one MFMA,
// a function of the layer's K alone: never of n, of the row's position in its tile or of the grid.
//
// Activations never leave the CU: the normalised input tile and every layer's ELU output live in two LDS buffers
// used alternately, [16][width padded to 16, + 4 floats so rows stay 16-byte aligned and shift banks].  Columns past
// a layer's width are zero in the LDS image and in the packed weights (zero weight rows, zero bias: ELU(0) = 0 feeds
// the next layer's K padding), rows past n are zero on load and masked on store.  A wave owns the 16-column output
// tiles t = wave, wave + 4, ... and works on MLP_TC of them at a time (independent accumulators hide the MFMA's
// dependent latency); the fragments of a k-group are fetched MLP_DEPTH groups ahead of the MFMAs that read them.
//
// Packed layout, per network, per layer: [tile t][k-group g][lane l][e] floats holding W[16 t + (l & 15)][16 g +
// 4 (l >> 4) + e], then the padded bias [16 * tiles].  A wave's B fetch is 1 KiB contiguous.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/h12learn.h"

// defined in h12_learn.hip: records the calling thread's h12learn_last_error message and returns code
int h12_learn_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3), visibility("hidden")));

namespace {

constexpr int MLP_ROWS = 16;
constexpr int MLP_WAVES = 4;
constexpr int MLP_THREADS = MLP_WAVES * 64;
constexpr int MLP_TC = 4;           // output tiles a wave accumulates at a time
constexpr int MLP_DEPTH = 4;        // k-groups fetched ahead of the MFMAs
constexpr int MLP_MAX_WIDTH = 1024;  // any layer width, input included
constexpr int MLP_LD_PAD = 4;
constexpr int PACK_BLOCK = 256;
constexpr size_t LDS_DEFAULT_LIMIT = 64 * 1024;

using f32x4 = __attribute__((ext_vector_type(4))) float;

__host__ __device__ inline int pad16(int v) { return (v + 15) & ~15; }

// floats of one packed layer: padded weights followed by the padded bias
__host__ __device__ inline size_t layer_floats(int in, int out) {
  return (size_t)pad16(in) * (size_t)pad16(out) + (size_t)pad16(out);
}

__host__ __device__ inline size_t net_floats(const h12learn_mlp_net& net) {
  size_t s = 0;
  for (int l = 0; l < net.n_layers; ++l) s += layer_floats(net.dims[l], net.dims[l + 1]);
  return s;
}

__global__ __launch_bounds__(PACK_BLOCK) void mlp_pack_kernel(h12learn_mlp_desc desc, float* packed, size_t total) {
  size_t i = (size_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
  if (i >= total) return;
  const size_t dst = i;
  for (int nidx = 0; nidx < desc.n_nets; ++nidx) {
    const h12learn_mlp_net& net = desc.nets[nidx];
    for (int l = 0; l < net.n_layers; ++l) {
      const int in = net.dims[l], out = net.dims[l + 1];
      const size_t wsz = (size_t)pad16(in) * (size_t)pad16(out);
      if (i < wsz) {
        const int kg = pad16(in) / 16;
        const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
        const size_t tg = i >> 8;
        const int g = (int)(tg % (size_t)kg), t = (int)(tg / (size_t)kg);
        const int j = 16 * t + (lane & 15), k = 16 * g + 4 * (lane >> 4) + e;
        packed[dst] = (j < out && k < in) ? net.W[l][(size_t)j * (size_t)in + k] : 0.f;
        return;
      }
      i -= wsz;
      if (i < (size_t)pad16(out)) {
        packed[dst] = (int)i < out ? net.b[l][i] : 0.f;
        return;
      }
      i -= (size_t)pad16(out);
    }
  }
}

__device__ __forceinline__ float elu1(float v) { return v > 0.f ? v : expm1f(v); }

// NT output tiles (t0, t0 + 4, ...) of one layer for this wave, all of them valid.  The A and B fragments of k-group g
// are fetched MLP_DEPTH groups before the MFMAs that read them: with one block per CU there is one wave per SIMD and
// nothing else to hide the L2 latency of the weight stream behind.
template <int NT>
__device__ __forceinline__ void mlp_tiles(const float* __restrict__ wp, const float* __restrict__ bp,
                                          const float* arow, int kg, int t0, bool last, float* hout, int ldout,
                                          float* __restrict__ y, int d_out, long long row0, long long n) {
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, q = lane >> 4;
  f32x4 acc[NT];
  const f32x4* bsrc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int t = t0 + MLP_WAVES * i;
    const float b = bp[16 * t + col];
    acc[i] = f32x4{b, b, b, b};
    bsrc[i] = reinterpret_cast<const f32x4*>(wp + (size_t)t * (size_t)kg * 256) + lane;
  }
  f32x4 aq[MLP_DEPTH], bq[MLP_DEPTH][NT];
#pragma unroll
  for (int s = 0; s < MLP_DEPTH; ++s) {
    const int gl = s < kg ? s : kg - 1;  // past the end: a harmless reload of the last group
    aq[s] = *reinterpret_cast<const f32x4*>(arow + 16 * gl);
#pragma unroll
    for (int i = 0; i < NT; ++i) bq[s][i] = bsrc[i][(size_t)gl * 64];
  }
  for (int g = 0; g < kg; g += MLP_DEPTH) {
#pragma unroll
    for (int s = 0; s < MLP_DEPTH; ++s) {
      if (g + s < kg) {  // wave-uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int i = 0; i < NT; ++i)
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[s][e], bq[s][i][e], acc[i], 0, 0, 0);
        }
      }
      const int gl = g + s + MLP_DEPTH < kg ? g + s + MLP_DEPTH : kg - 1;
      aq[s] = *reinterpret_cast<const f32x4*>(arow + 16 * gl);
#pragma unroll
      for (int i = 0; i < NT; ++i) bq[s][i] = bsrc[i][(size_t)gl * 64];
    }
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int j = 16 * (t0 + MLP_WAVES * i) + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * q + r;
      if (!last) {
        hout[row * ldout + j] = elu1(acc[i][r]);
      } else if (j < d_out && row0 + row < n) {
        y[(size_t)(row0 + row) * (size_t)d_out + j] = acc[i][r];
      }
    }
  }
}

// One layer for this wave's output tiles t = wave, wave + 4, ..., MLP_TC of them at a time, then 2, then 1.  hin:
// [16][ldin] LDS image, K = 16 * kg columns of it.  Not the last layer: ELU into hout [16][ldout].  Last layer: masked
// store to y [n][d_out].
__device__ __forceinline__ void mlp_layer(const float* __restrict__ wp, const float* __restrict__ bp,
                                          const float* hin, int ldin, int kg, int tiles, bool last, float* hout,
                                          int ldout, float* __restrict__ y, int d_out, long long row0, long long n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* arow = hin + (lane & 15) * ldin + 4 * (lane >> 4);
  int t0 = wave;
  int mine = tiles > wave ? (tiles - wave + MLP_WAVES - 1) / MLP_WAVES : 0;  // this wave's tiles
  for (; mine >= MLP_TC; mine -= MLP_TC, t0 += MLP_WAVES * MLP_TC)
    mlp_tiles<MLP_TC>(wp, bp, arow, kg, t0, last, hout, ldout, y, d_out, row0, n);
  static_assert(MLP_TC == 4, "the remainder below is 2, then 1");
  if (mine >= 2) {
    mlp_tiles<2>(wp, bp, arow, kg, t0, last, hout, ldout, y, d_out, row0, n);
    mine -= 2, t0 += MLP_WAVES * 2;
  }
  if (mine >= 1) mlp_tiles<1>(wp, bp, arow, kg, t0, last, hout, ldout, y, d_out, row0, n);
}

struct mlp_outputs {
  float* y[H12LEARN_MLP_MAX_NETS];
};

__global__ __launch_bounds__(MLP_THREADS) void mlp_forward_kernel(h12learn_mlp_desc desc,
                                                                  const float* __restrict__ packed,
                                                                  const float* __restrict__ x, long long n,
                                                                  mlp_outputs outs, int ld0, int ld1) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* buf0 = lds;
  float* buf1 = lds + MLP_ROWS * ld0;
  const int nidx = blockIdx.y;
  const h12learn_mlp_net& net = desc.nets[nidx];
  const long long row0 = (long long)blockIdx.x * MLP_ROWS;

  const float* wp = packed;
  for (int i = 0; i < nidx; ++i) wp += net_floats(desc.nets[i]);

  // the normalised input tile, zero in the padding columns and in the rows past n
  const int d_in = desc.d_in, k0 = pad16(d_in);
  // a thread takes a column of the tile: its 16 loads are in flight together (x comes from HBM)
  for (int c = threadIdx.x; c < k0; c += MLP_THREADS) {
    float v[MLP_ROWS];
#pragma unroll
    for (int r = 0; r < MLP_ROWS; ++r)
      v[r] = (c < d_in && row0 + r < n) ? x[(size_t)(row0 + r) * (size_t)d_in + c] : 0.f;
    if (c < d_in && desc.norm_kind != H12LEARN_MLP_NORM_NONE) {
      const float m = desc.norm_mean[c];
      const float sc = desc.norm_kind == H12LEARN_MLP_NORM_VAR ? sqrtf(desc.norm_scale[c] + desc.norm_eps)
                                                               : desc.norm_scale[c] + desc.norm_eps;
#pragma unroll
      for (int r = 0; r < MLP_ROWS; ++r)
        if (row0 + r < n) v[r] = (v[r] - m) / sc;  // rows past n stay zero
    }
#pragma unroll
    for (int r = 0; r < MLP_ROWS; ++r) buf0[r * ld0 + c] = v[r];
  }
  __syncthreads();

  float* hin = buf0;
  float* hout = buf1;
  int ldin = ld0, ldout = ld1;
  for (int l = 0; l < net.n_layers; ++l) {
    const int in = net.dims[l], out = net.dims[l + 1];
    const int kg = pad16(in) / 16, tiles = pad16(out) / 16;
    const float* bp = wp + (size_t)pad16(in) * (size_t)pad16(out);
    mlp_layer(wp, bp, hin, ldin, kg, tiles, l == net.n_layers - 1, hout, ldout, outs.y[nidx], out, row0, n);
    wp = bp + pad16(out);
    __syncthreads();
    float* tp = hin;
    hin = hout, hout = tp;
    const int tl = ldin;
    ldin = ldout, ldout = tl;
  }
}

int check_desc(const h12learn_mlp_desc* desc, const char* fn) {
  if (!desc) return h12_learn_fail(H12LEARN_E_ARG, "%s: desc is null", fn);
  if (desc->n_nets < 1 || desc->n_nets > H12LEARN_MLP_MAX_NETS)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: n_nets = %d (1..%d)", fn, desc->n_nets, H12LEARN_MLP_MAX_NETS);
  if (desc->d_in < 1 || desc->d_in > MLP_MAX_WIDTH)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: d_in = %d (1..%d)", fn, desc->d_in, MLP_MAX_WIDTH);
  if (desc->norm_kind != H12LEARN_MLP_NORM_NONE && desc->norm_kind != H12LEARN_MLP_NORM_VAR &&
      desc->norm_kind != H12LEARN_MLP_NORM_STD)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: norm_kind = %d", fn, desc->norm_kind);
  for (int i = 0; i < desc->n_nets; ++i) {
    const h12learn_mlp_net& net = desc->nets[i];
    if (net.n_layers < 1 || net.n_layers > H12LEARN_MLP_MAX_LAYERS)
      return h12_learn_fail(H12LEARN_E_ARG, "%s: nets[%d].n_layers = %d (1..%d)", fn, i, net.n_layers,
                                H12LEARN_MLP_MAX_LAYERS);
    if (net.dims[0] != desc->d_in)
      return h12_learn_fail(H12LEARN_E_ARG, "%s: nets[%d].dims[0] = %d differs from d_in = %d", fn, i,
                                net.dims[0], desc->d_in);
    for (int l = 1; l <= net.n_layers; ++l)
      if (net.dims[l] < 1 || net.dims[l] > MLP_MAX_WIDTH)
        return h12_learn_fail(H12LEARN_E_ARG, "%s: nets[%d].dims[%d] = %d (1..%d)", fn, i, l, net.dims[l],
                                  MLP_MAX_WIDTH);
  }
  return H12LEARN_OK;
}

int check_pointers(const h12learn_mlp_desc* desc, const char* fn) {
  if (desc->norm_kind != H12LEARN_MLP_NORM_NONE && (!desc->norm_mean || !desc->norm_scale))
    return h12_learn_fail(H12LEARN_E_ARG, "%s: norm_mean / norm_scale is null", fn);
  for (int i = 0; i < desc->n_nets; ++i)
    for (int l = 0; l < desc->nets[i].n_layers; ++l)
      if (!desc->nets[i].W[l] || !desc->nets[i].b[l])
        return h12_learn_fail(H12LEARN_E_ARG, "%s: nets[%d].W[%d] / b[%d] is null", fn, i, l, l);
  return H12LEARN_OK;
}

// widths of the two LDS buffers: buffer 0 holds the input and the outputs of the odd layers, buffer 1 the others
void lds_widths(const h12learn_mlp_desc* desc, int* ld0, int* ld1) {
  int w0 = pad16(desc->d_in), w1 = 16;
  for (int i = 0; i < desc->n_nets; ++i)
    for (int l = 0; l + 1 < desc->nets[i].n_layers; ++l) {
      const int w = pad16(desc->nets[i].dims[l + 1]);
      int& dst = (l & 1) ? w0 : w1;
      if (w > dst) dst = w;
    }
  *ld0 = w0 + MLP_LD_PAD;
  *ld1 = w1 + MLP_LD_PAD;
}

}  // namespace

extern "C" {

int h12learn_mlp_max_width(void) { return MLP_MAX_WIDTH; }

size_t h12learn_mlp_packed_bytes(const h12learn_mlp_desc* desc) {
  if (check_desc(desc, "mlp_packed_bytes") != H12LEARN_OK) return 0;
  size_t s = 0;
  for (int i = 0; i < desc->n_nets; ++i) s += net_floats(desc->nets[i]);
  return s * sizeof(float);
}

int h12learn_mlp_pack(const h12learn_mlp_desc* desc, float* packed, void* stream) {
  int rc = check_desc(desc, "mlp_pack");
  if (rc == H12LEARN_OK) rc = check_pointers(desc, "mlp_pack");
  if (rc != H12LEARN_OK) return rc;
  if (!packed) return h12_learn_fail(H12LEARN_E_ARG, "mlp_pack: packed is null");
  if (((uintptr_t)packed & 15) != 0) return h12_learn_fail(H12LEARN_E_ARG, "mlp_pack: packed not 16-byte aligned");
  const size_t total = h12learn_mlp_packed_bytes(desc) / sizeof(float);
  const size_t blocks = (total + PACK_BLOCK - 1) / PACK_BLOCK;
  hipLaunchKernelGGL(mlp_pack_kernel, dim3((unsigned)blocks), dim3(PACK_BLOCK), 0, (hipStream_t)stream, *desc, packed,
                     total);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "mlp_pack launch: %s", hipGetErrorString(e));
  return H12LEARN_OK;
}

int h12learn_mlp_forward(const h12learn_mlp_desc* desc, const float* packed, const float* x, long long n,
                         float* const* y, void* stream) {
  int rc = check_desc(desc, "mlp_forward");
  if (rc == H12LEARN_OK) rc = check_pointers(desc, "mlp_forward");
  if (rc != H12LEARN_OK) return rc;
  if (!packed) return h12_learn_fail(H12LEARN_E_ARG, "mlp_forward: packed is null");
  if (((uintptr_t)packed & 15) != 0)
    return h12_learn_fail(H12LEARN_E_ARG, "mlp_forward: packed not 16-byte aligned");
  if (!x) return h12_learn_fail(H12LEARN_E_ARG, "mlp_forward: x is null");
  if (n < 1) return h12_learn_fail(H12LEARN_E_ARG, "mlp_forward: n = %lld (must be >= 1)", n);
  if (!y) return h12_learn_fail(H12LEARN_E_ARG, "mlp_forward: y is null");
  mlp_outputs outs = {};
  for (int i = 0; i < desc->n_nets; ++i) {
    if (!y[i]) return h12_learn_fail(H12LEARN_E_ARG, "mlp_forward: y[%d] is null", i);
    outs.y[i] = y[i];
  }
  const long long tiles = (n + MLP_ROWS - 1) / MLP_ROWS;
  if (tiles > 0x7fffffffLL) return h12_learn_fail(H12LEARN_E_ARG, "mlp_forward: n = %lld exceeds the grid", n);
  int ld0, ld1;
  lds_widths(desc, &ld0, &ld1);
  const size_t lds_bytes = (size_t)MLP_ROWS * (size_t)(ld0 + ld1) * sizeof(float);
  if (lds_bytes > LDS_DEFAULT_LIMIT) {
    // wide networks only (the 450-512-256-128 policy needs 63 KiB): raise the kernel's dynamic LDS limit once to
    // what the widest supported network needs; an attribute of the function, no stream work
    static bool raised = false;
    if (!raised) {
      const int most = MLP_ROWS * 2 * (MLP_MAX_WIDTH + MLP_LD_PAD) * (int)sizeof(float);
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_forward_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, most);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        return h12_learn_fail(H12LEARN_E_HIP, "mlp_forward: LDS limit: %s", hipGetErrorString(e));
      }
      raised = true;
    }
  }
  hipLaunchKernelGGL(mlp_forward_kernel, dim3((unsigned)tiles, (unsigned)desc->n_nets), dim3(MLP_THREADS), lds_bytes,
                     (hipStream_t)stream, *desc, packed, x, n, outs, ld0, ld1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "mlp_forward launch: %s", hipGetErrorString(e));
  return H12LEARN_OK;
}

}  // extern "C"
