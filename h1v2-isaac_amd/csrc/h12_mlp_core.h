// h12_mlp_core.h: what the fused policy MLP's inference kernel (h12_policy.hip) and its training kernels
// (h12_policy_train.hip) share: the packed weight layout, the order of summation, the MFMA tile routines and the host
// checks.  Internal to libh12env.so; each .hip file's header says only what is its own.
//
// A layer is Y[rows][out] = H[rows][K] W^T + b on v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered fmaf chain), 16
// rows ("sub-tile") by 16 columns ("tile") per MFMA:
//   A = H: lane l holds H[row l & 15][k], B = W^T: lane l holds W[col l & 15][k], both with k chosen by q = l >> 4;
//   D: lane l, register r holds Y[row 4 q + r][col l & 15].
// The bias is the accumulator's start value (no bias: zero).  K is walked in groups of 16: k-group g, MFMA step e
// (0..3) and lane quarter q multiply k = 16 g + 4 q + e, so a lane's four A values of a group are one 16-byte LDS read
// and its four B values one 16-byte global read.  The summation order of an output element is therefore
//   bias, then for g = 0.., for e = 0..3: the four k = 16 g + 4 q + e (q = 0..3) of one MFMA,
// a function of the layer's K alone: never of n, of the row's position in its tile, of the rows of a block or of the
// grid.  Kernels that read the same pack through these routines give the same bits.
//
// Activations never leave the CU: a block's input tile and every layer's output live in two LDS buffers used
// alternately, [rows][width padded to 16, + LD_PAD floats so rows stay 16-byte aligned and shift banks].  Columns past
// a layer's width are zero in the LDS image and in the packed weights (zero weight rows, zero bias: ELU(0) = 0 feeds
// the next layer's K padding), rows past n are zero on load and masked on store.  A wave owns the 16-column output
// tiles t = wave, wave + 4, ... and works on TC of them at a time (independent accumulators hide the MFMA's dependent
// latency); the fragments of a k-group are fetched DEPTH groups ahead of the MFMAs that read them.
//
// Packed layout of a matrix M[rows][K] (W, or W^T for the dgrad): [tile t][k-group g][lane l][e] floats holding
// M[16 t + (l & 15)][16 g + 4 (l >> 4) + e], zero past either extent.  A wave's B fetch is 1 KiB contiguous.
// h12learn_mlp_pack stores, per network and layer, W so packed and then the padded bias [16 * tiles].
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/h12learn.h"

// defined in h12_learn.hip: records the calling thread's h12learn_last_error message and returns code
int h12_learn_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3), visibility("hidden")));

namespace mlp {

constexpr int WAVES = 4;
constexpr int THREADS = WAVES * 64;
constexpr int TC = 4;      // output tiles a wave accumulates at a time
constexpr int DEPTH = 4;   // k-groups fetched ahead of the MFMAs
constexpr int LD_PAD = 4;
constexpr int PACK_BLOCK = 256;
constexpr size_t LDS_DEFAULT_LIMIT = 64 * 1024;

using f32x4 = __attribute__((ext_vector_type(4))) float;

__host__ __device__ inline int pad16(int v) { return (v + 15) & ~15; }

// floats of one packed matrix, and of one layer of h12learn_mlp_pack: the matrix followed by the padded bias
__host__ __device__ inline size_t matrix_floats(int in, int out) { return (size_t)pad16(in) * (size_t)pad16(out); }
__host__ __device__ inline size_t layer_floats(int in, int out) { return matrix_floats(in, out) + (size_t)pad16(out); }

// float i of a packed matrix with kg k-groups holds M[*row][*k]
__device__ __forceinline__ void pack_index(size_t i, int kg, int* row, int* k) {
  const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
  const size_t tg = i >> 8;
  const int g = (int)(tg % (size_t)kg), t = (int)(tg / (size_t)kg);
  *row = 16 * t + (lane & 15);
  *k = 16 * g + 4 * (lane >> 4) + e;
}

__device__ __forceinline__ float elu1(float v) { return v > 0.f ? v : expm1f(v); }

// NT output tiles (t0, t0 + 4, ...) of one layer for this wave, all of them valid, over the block's SUB 16-row
// sub-tiles: every B fragment is fetched once and multiplies the A fragment of each sub-tile.  The A and B fragments
// of k-group g are fetched DEPTH groups before the MFMAs that read them: with one block per CU there is one wave per
// SIMD and nothing else to hide the L2 latency of the weight stream behind.  bp == nullptr: the accumulators start at
// zero.  side = pre(column, row in the block) is fetched for every element BEFORE the k loop (the backward's saved
// activation: its global-memory latency hides behind the MFMAs); epi(column, row, value, side) receives every element.
// The A fragments of k-group g, one per sub-tile.  The one-sub-tile overload says the same without a loop: with a
// one-trip loop to remove first, the compiler schedules the inference kernel's k loop worse (7 s_waitcnt per pass
// instead of 1, 2.4 % of the kernel's time on the MI355X).
template <int SUB>
__device__ __forceinline__ void load_a(f32x4 (&a)[SUB], const float* arow, int ldin, int g) {
#pragma unroll
  for (int s = 0; s < SUB; ++s) a[s] = *reinterpret_cast<const f32x4*>(arow + 16 * s * ldin + 16 * g);
}
__device__ __forceinline__ void load_a(f32x4 (&a)[1], const float* arow, int, int g) {
  a[0] = *reinterpret_cast<const f32x4*>(arow + 16 * g);
}

template <int NT, int SUB, class Pre, class Epi>
__device__ __forceinline__ void tiles(const float* __restrict__ wp, const float* __restrict__ bp, const float* arow,
                                      int ldin, int kg, int t0, Pre pre, Epi epi) {
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, q = lane >> 4;
  f32x4 acc[NT][SUB];
  const f32x4* bsrc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int t = t0 + WAVES * i;
    const float b = bp ? bp[16 * t + col] : 0.f;
#pragma unroll
    for (int s = 0; s < SUB; ++s) acc[i][s] = f32x4{b, b, b, b};
    bsrc[i] = reinterpret_cast<const f32x4*>(wp + (size_t)t * (size_t)kg * 256) + lane;
  }
  float side[NT][SUB][4];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
#pragma unroll
    for (int s = 0; s < SUB; ++s) {
#pragma unroll
      for (int r = 0; r < 4; ++r) side[i][s][r] = pre(16 * (t0 + WAVES * i) + col, 16 * s + 4 * q + r);
    }
  }
  f32x4 aq[DEPTH][SUB], bq[DEPTH][NT];
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    const int gl = d < kg ? d : kg - 1;  // past the end: a harmless reload of the last group
    load_a(aq[d], arow, ldin, gl);
#pragma unroll
    for (int i = 0; i < NT; ++i) bq[d][i] = bsrc[i][(size_t)gl * 64];
  }
  for (int g = 0; g < kg; g += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      if (g + d < kg) {  // wave-uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int i = 0; i < NT; ++i) {
#pragma unroll
            for (int s = 0; s < SUB; ++s)
              acc[i][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[d][s][e], bq[d][i][e], acc[i][s], 0, 0, 0);
          }
        }
      }
      const int gl = g + d + DEPTH < kg ? g + d + DEPTH : kg - 1;
      load_a(aq[d], arow, ldin, gl);
#pragma unroll
      for (int i = 0; i < NT; ++i) bq[d][i] = bsrc[i][(size_t)gl * 64];
    }
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int j = 16 * (t0 + WAVES * i) + col;
#pragma unroll
    for (int s = 0; s < SUB; ++s) {
#pragma unroll
      for (int r = 0; r < 4; ++r) epi(j, 16 * s + 4 * q + r, acc[i][s][r], side[i][s][r]);
    }
  }
}

// One layer for this wave's output tiles t = wave, wave + 4, ..., TC of them at a time, then 2, then 1.
// hin: [16 * SUB][ldin] LDS image, K = 16 * kg columns of it.
template <int SUB, class Pre, class Epi>
__device__ __forceinline__ void layer(const float* __restrict__ wp, const float* __restrict__ bp, const float* hin,
                                      int ldin, int kg, int ntiles, Pre pre, Epi epi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* arow = hin + (lane & 15) * ldin + 4 * (lane >> 4);
  int t0 = wave;
  int mine = ntiles > wave ? (ntiles - wave + WAVES - 1) / WAVES : 0;  // this wave's tiles
  for (; mine >= TC; mine -= TC, t0 += WAVES * TC) tiles<TC, SUB>(wp, bp, arow, ldin, kg, t0, pre, epi);
  static_assert(TC == 4, "the remainder below is 2, then 1");
  if (mine >= 2) {
    tiles<2, SUB>(wp, bp, arow, ldin, kg, t0, pre, epi);
    mine -= 2, t0 += WAVES * 2;
  }
  if (mine >= 1) tiles<1, SUB>(wp, bp, arow, ldin, kg, t0, pre, epi);
}

// a pre of layer() for the kernels that need no side value
struct no_side {
  __device__ float operator()(int, int) const { return 0.f; }
};

// The [ROWS][16 * ceil(d / 16)] tile of src [n][d] at row0 into an LDS image: zero in the padding columns and in the
// rows past n.  A thread takes a column: its loads are in flight together (src comes from HBM).
template <int ROWS>
__device__ __forceinline__ void load_tile(const float* __restrict__ src, int d, long long row0, long long n, float* buf,
                                          int ld) {
  const int kpad = pad16(d);
  for (int c = threadIdx.x; c < kpad; c += THREADS) {
    float v[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) v[r] = (c < d && row0 + r < n) ? src[(size_t)(row0 + r) * (size_t)d + c] : 0.f;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) buf[r * ld + c] = v[r];
  }
}

// Shape checks of a descriptor whose widths, the input's included, may be up to max_width.
inline int check_desc(const h12learn_mlp_desc* desc, const char* fn, int max_width) {
  if (!desc) return h12_learn_fail(H12LEARN_E_ARG, "%s: desc is null", fn);
  if (desc->n_nets < 1 || desc->n_nets > H12LEARN_MLP_MAX_NETS)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: n_nets = %d (1..%d)", fn, desc->n_nets, H12LEARN_MLP_MAX_NETS);
  if (desc->d_in < 1 || desc->d_in > max_width)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: d_in = %d (1..%d)", fn, desc->d_in, max_width);
  if (desc->norm_kind != H12LEARN_MLP_NORM_NONE && desc->norm_kind != H12LEARN_MLP_NORM_VAR &&
      desc->norm_kind != H12LEARN_MLP_NORM_STD)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: norm_kind = %d", fn, desc->norm_kind);
  for (int i = 0; i < desc->n_nets; ++i) {
    const h12learn_mlp_net& net = desc->nets[i];
    if (net.n_layers < 1 || net.n_layers > H12LEARN_MLP_MAX_LAYERS)
      return h12_learn_fail(H12LEARN_E_ARG, "%s: nets[%d].n_layers = %d (1..%d)", fn, i, net.n_layers,
                            H12LEARN_MLP_MAX_LAYERS);
    if (net.dims[0] != desc->d_in)
      return h12_learn_fail(H12LEARN_E_ARG, "%s: nets[%d].dims[0] = %d differs from d_in = %d", fn, i, net.dims[0],
                            desc->d_in);
    for (int l = 1; l <= net.n_layers; ++l)
      if (net.dims[l] < 1 || net.dims[l] > max_width)
        return h12_learn_fail(H12LEARN_E_ARG, "%s: nets[%d].dims[%d] = %d (1..%d)", fn, i, l, net.dims[l], max_width);
  }
  return H12LEARN_OK;
}

// Widths of the two LDS buffers.  The images a block holds one after the other alternate between them: image 0 (the
// tile it loads) and every even one in buffer 0, the odd ones in buffer 1.
struct lds_images {
  int w[2] = {16, 16};
  void hold(int image, int width) {
    int& dst = w[image & 1];
    if (pad16(width) > dst) dst = pad16(width);
  }
  int ld(int buffer) const { return w[buffer] + LD_PAD; }
  size_t bytes(int rows) const { return (size_t)rows * (size_t)(ld(0) + ld(1)) * sizeof(float); }
};

// a forward pass: the input, then the output of every layer but the last, of every network
inline lds_images forward_images(const h12learn_mlp_desc* desc) {
  lds_images im;
  im.hold(0, desc->d_in);
  for (int i = 0; i < desc->n_nets; ++i)
    for (int l = 0; l + 1 < desc->nets[i].n_layers; ++l) im.hold(l + 1, desc->nets[i].dims[l + 1]);
  return im;
}

// the LDS bytes of a kernel's widest supported network
constexpr int lds_most(int rows, int max_width) { return rows * 2 * (max_width + LD_PAD) * (int)sizeof(float); }

// More than 64 KiB of dynamic LDS: the first such call of a kernel raises its limit to most (an attribute of the
// function, no stream work).  That call must not be made while the stream is capturing.  raised is the kernel's own
// flag: one per kernel and process, not per device.
inline int raise_lds_limit(const void* kernel, bool* raised, int most, size_t lds_bytes, hipStream_t stream,
                           const char* fn) {
  if (lds_bytes <= LDS_DEFAULT_LIMIT || *raised) return H12LEARN_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &st) != hipSuccess) {
    (void)hipGetLastError();
    st = hipStreamCaptureStatusNone;
  }
  if (st != hipStreamCaptureStatusNone)
    return h12_learn_fail(H12LEARN_E_HIP, "%s: the first call that needs more than 64 KiB of LDS must be made outside "
                          "a stream capture (warm up first)", fn);
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, most);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return h12_learn_fail(H12LEARN_E_HIP, "%s: LDS limit: %s", fn, hipGetErrorString(e));
  }
  *raised = true;
  return H12LEARN_OK;
}

}  // namespace mlp
