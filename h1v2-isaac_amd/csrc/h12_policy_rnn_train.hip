// h12_policy_rnn_train.hip: the recurrent policy's update on HIP (include/h12learn.h, h12learn_lstm_seq_*).
//
//   h12learn_lstm_seq_pack      W_hh and W_hh^T of up to 2 networks -> the tiled, zero-padded pack (one launch)
//   h12learn_lstm_seq_forward   the LSTM over [T][n] with done resets, keeping the gates and c for the backward
//   h12learn_lstm_seq_backward  back-propagation through time: dz [T][n][4H] and, optionally, dh0 / dc0
//
// The packed layout, the order of summation and the tile routines are those of h12_mlp_core.h: read its header first.
// The input projection zx = x W_ih^T + b_ih + b_hh and the weight gradients are the caller's GEMMs; what is here is the
// recurrence, which no GEMM expresses: z_t = zx_t + h_{t-1} W_hh^T and, backwards, dh_{t-1} = dz_t W_hh.
//
// Both kernels: grid (row tiles of 16, networks), 4 waves; a block OWNS its 16 rows for all T steps and loops over t, so
// the state never leaves the CU and nothing is exchanged between blocks.  Three LDS images:
//   A [16][pad16(H)]    forward: h_{t-1} (h0 at t = 0, zero where the row is reset);  backward: the carry dh_c
//   B [16][pad16(4H)]   forward: the gate pre-activations;                             backward: dz_t
//   C [16][pad16(H)]    forward: c_{t-1};                                             backward: the carry dc_c
// An element of C is read and written by the same thread only.  Per step, two barriers:
//   forward   layer<1>(W_hh pack: A -> B, zx_t through the core's side value) | pointwise (B, C -> gates, c, h; A, C)
//   backward  pointwise (A, C, saved gates and c -> dz_t; B, C) | layer<1>(W_hh^T pack: B -> A, zero where reset at t)
// Order of summation: a gate pre-activation is the core's bias-free k chain over h_{t-1} (from zero), THEN + zx; a dh_c
// element is the core's k chain over the 4H columns of dz_t from zero, and dh = dh_seq + dh_c.  Both orders depend on H
// alone.  Rows are independent of one another, rows past n are zero on load and masked on store, and there are no
// atomics: every output is bitwise reproducible and independent of n, T, the row's place in its tile and the grid.
//
// reset(t, row) = t >= 1 && dones[t - 1][row] != 0; dones[T - 1] is never read.
#include "h12_mlp_core.h"

namespace {

using namespace mlp;

constexpr int SEQ_ROWS = 16;
constexpr int SEQ_MAX_HIDDEN = 256;  // h12learn_lstm_max_hidden(): 4H stays within the core's widest layer
constexpr int SEQ_MAX_T = 4096;

// floats of one network's pack: W_hh (K = pad16(H), 4H rows), then W_hh^T (K = pad16(4H), H rows)
__host__ __device__ inline size_t seq_net_floats(int H) { return 2 * matrix_floats(H, 4 * H); }

__global__ __launch_bounds__(PACK_BLOCK) void lstm_seq_pack_kernel(h12learn_lstm_seq_desc desc, float* packed,
                                                                   size_t total) {
  size_t i = (size_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
  if (i >= total) return;
  const size_t dst = i;
  const int H = desc.hidden, G = 4 * H;
  const size_t per = seq_net_floats(H), wsz = matrix_floats(H, G);
  const int nidx = (int)(i / per);
  i -= (size_t)nidx * per;
  const float* w = desc.w_hh[nidx];
  int j, k;
  float v = 0.f;
  if (i < wsz) {  // W_hh: output row j of 4H, k of H
    pack_index(i, pad16(H) / 16, &j, &k);
    if (j < G && k < H) v = w[(size_t)j * (size_t)H + k];
  } else {  // W_hh^T: output row j of H, k of 4H
    pack_index(i - wsz, pad16(G) / 16, &j, &k);
    if (j < H && k < G) v = w[(size_t)k * (size_t)H + j];
  }
  packed[dst] = v;
}

// sigmoid with a true division and the library's expf, as in h12_policy_rnn.hip
__device__ __forceinline__ float sigmoid1(float z) { return 1.f / (1.f + expf(-z)); }

__global__ __launch_bounds__(THREADS) void lstm_seq_forward_kernel(int H, const float* __restrict__ packed,
                                                                   h12learn_lstm_seq_io io, int lda, int ldb) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* bufA = lds;
  float* bufB = bufA + SEQ_ROWS * lda;
  float* bufC = bufB + SEQ_ROWS * ldb;
  const int nidx = blockIdx.y;
  const long long n = io.n;
  const long long row0 = (long long)blockIdx.x * SEQ_ROWS;
  const int kh = pad16(H), G = 4 * H, T = io.T;
  const float* wp = packed + (size_t)nidx * seq_net_floats(H);
  const float* __restrict__ zx = io.zx[nidx];
  const unsigned char* __restrict__ dones = io.dones;
  float* h_seq = io.h_seq[nidx];
  float* c_seq = io.c_seq[nidx];
  float* gates = io.gates[nidx];

  // t = 0 reads h0 / c0: zero in the padding columns and in the rows past n
  {
    const float* h0 = io.h0[nidx];
    const float* c0 = io.c0[nidx];
    for (int e = threadIdx.x; e < SEQ_ROWS * kh; e += THREADS) {
      const int row = e / kh, u = e - row * kh;
      const bool live = u < H && row0 + row < n;
      const size_t at = (size_t)(row0 + row) * (size_t)H + u;
      bufA[row * lda + u] = live ? h0[at] : 0.f;
      bufC[row * lda + u] = live ? c0[at] : 0.f;
    }
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const size_t step0 = (size_t)t * (size_t)n;  // first row of step t in the [T][n] tensors
    // z = h_prev W_hh^T (the bias-free k chain), then + zx[t], into image B
    layer<1>(wp, nullptr, bufA, lda, kh / 16, pad16(G) / 16,
             [=](int j, int row) {
               return (j < G && row0 + row < n) ? zx[(step0 + (size_t)(row0 + row)) * (size_t)G + j] : 0.f;
             },
             [=](int j, int row, float v, float side) { bufB[row * ldb + j] = v + side; });
    __syncthreads();

    // pointwise: torch's gate order i, f, g, o.  What the next step reads (h in A, c in C) is zero where that step resets
    const bool more = t + 1 < T;
    for (int e = threadIdx.x; e < SEQ_ROWS * kh; e += THREADS) {
      const int row = e / kh, u = e - row * kh;
      if (u >= H || row0 + row >= n) continue;  // A and C stay zero there
      const float* z = bufB + row * ldb + u;
      const float cp = bufC[row * lda + u];
      const float ig = sigmoid1(z[0]), fg = sigmoid1(z[H]), gg = tanhf(z[2 * H]), og = sigmoid1(z[3 * H]);
      const float cn = fg * cp + ig * gg;
      const float hn = og * tanhf(cn);
      const size_t r = step0 + (size_t)(row0 + row);
      float* gout = gates + r * (size_t)G + u;
      gout[0] = ig, gout[H] = fg, gout[2 * H] = gg, gout[3 * H] = og;
      c_seq[r * (size_t)H + u] = cn;
      h_seq[r * (size_t)H + u] = hn;
      const bool reset_next = more && dones[r] != 0;
      bufA[row * lda + u] = reset_next ? 0.f : hn;
      bufC[row * lda + u] = reset_next ? 0.f : cn;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(THREADS) void lstm_seq_backward_kernel(int H, const float* __restrict__ packed,
                                                                    h12learn_lstm_seq_grad_io io, int lda, int ldb) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* bufA = lds;
  float* bufB = bufA + SEQ_ROWS * lda;
  float* bufC = bufB + SEQ_ROWS * ldb;
  const int nidx = blockIdx.y;
  const long long n = io.n;
  const long long row0 = (long long)blockIdx.x * SEQ_ROWS;
  const int kh = pad16(H), G = 4 * H, kg4 = pad16(G), T = io.T;
  const float* wpt = packed + (size_t)nidx * seq_net_floats(H) + matrix_floats(H, G);
  const unsigned char* __restrict__ dones = io.dones;
  const float* __restrict__ dh_seq = io.dh_seq[nidx];
  const float* __restrict__ gates = io.gates[nidx];
  const float* __restrict__ c_seq = io.c_seq[nidx];
  const float* __restrict__ c0 = io.c0[nidx];
  float* dz = io.dz[nidx];
  float* dh0 = io.dh0[nidx];
  float* dc0 = io.dc0[nidx];

  // the carries start at zero; B's rows past n and its columns past 4H stay zero throughout
  for (int e = threadIdx.x; e < SEQ_ROWS * kh; e += THREADS) {
    const int row = e / kh, u = e - row * kh;
    bufA[row * lda + u] = 0.f;
    bufC[row * lda + u] = 0.f;
  }
  for (int e = threadIdx.x; e < SEQ_ROWS * kg4; e += THREADS) {
    const int row = e / kg4, j = e - row * kg4;
    bufB[row * ldb + j] = 0.f;
  }
  __syncthreads();

  for (int t = T - 1; t >= 0; --t) {
    const size_t step0 = (size_t)t * (size_t)n;
    for (int e = threadIdx.x; e < SEQ_ROWS * kh; e += THREADS) {
      const int row = e / kh, u = e - row * kh;
      if (u >= H || row0 + row >= n) continue;
      const size_t r = step0 + (size_t)(row0 + row);
      const bool reset = t >= 1 && dones[r - (size_t)n] != 0;
      const size_t at = (size_t)(row0 + row) * (size_t)H + u;
      const float cp = reset ? 0.f : (t == 0 ? c0[at] : c_seq[(r - (size_t)n) * (size_t)H + u]);
      const float* gin = gates + r * (size_t)G + u;
      const float ig = gin[0], fg = gin[H], gg = gin[2 * H], og = gin[3 * H];
      const float tc = tanhf(c_seq[r * (size_t)H + u]);
      const float dh = dh_seq[r * (size_t)H + u] + bufA[row * lda + u];
      const float d_o = dh * tc;
      const float dc = bufC[row * lda + u] + dh * og * (1.f - tc * tc);
      const float d_i = dc * gg, d_g = dc * ig, d_f = dc * cp;
      const float zi = d_i * ig * (1.f - ig), zf = d_f * fg * (1.f - fg), zg = d_g * (1.f - gg * gg),
                  zo = d_o * og * (1.f - og);
      float* zout = dz + r * (size_t)G + u;
      zout[0] = zi, zout[H] = zf, zout[2 * H] = zg, zout[3 * H] = zo;
      float* zl = bufB + row * ldb + u;
      zl[0] = zi, zl[H] = zf, zl[2 * H] = zg, zl[3 * H] = zo;
      const float dcc = dc * fg;
      bufC[row * lda + u] = reset ? 0.f : dcc;  // a row that is reset at t sends nothing further back
      if (t == 0 && dc0) dc0[at] = dcc;
    }
    __syncthreads();

    // dh_c = dz_t W_hh (the k chain over 4H from zero) into image A, zero where the row is reset at t
    layer<1>(wpt, nullptr, bufB, ldb, kg4 / 16, kh / 16,
             [=](int, int row) {
               return (t >= 1 && row0 + row < n && dones[step0 - (size_t)n + (size_t)(row0 + row)] != 0) ? 0.f : 1.f;
             },
             [=](int j, int row, float v, float keep) {
               bufA[row * lda + j] = keep != 0.f ? v : 0.f;
               if (t == 0 && dh0 && j < H && row0 + row < n) dh0[(size_t)(row0 + row) * (size_t)H + j] = v;
             });
    __syncthreads();
  }
}

size_t seq_lds_bytes(int H) {
  return (size_t)SEQ_ROWS * (size_t)(2 * (pad16(H) + LD_PAD) + pad16(4 * H) + LD_PAD) * sizeof(float);
}

int check_seq_desc(const h12learn_lstm_seq_desc* desc, const char* fn, bool pointers) {
  if (!desc) return h12_learn_fail(H12LEARN_E_ARG, "%s: desc is null", fn);
  if (desc->n_nets < 1 || desc->n_nets > H12LEARN_LSTM_MAX_NETS)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: n_nets = %d (1..%d)", fn, desc->n_nets, H12LEARN_LSTM_MAX_NETS);
  if (desc->hidden < 1 || desc->hidden > SEQ_MAX_HIDDEN)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: hidden = %d (1..%d)", fn, desc->hidden, SEQ_MAX_HIDDEN);
  if (pointers)
    for (int i = 0; i < desc->n_nets; ++i)
      if (!desc->w_hh[i]) return h12_learn_fail(H12LEARN_E_ARG, "%s: w_hh[%d] is null", fn, i);
  return H12LEARN_OK;
}

int check_seq_call(const h12learn_lstm_seq_desc* desc, const float* packed, const void* io, int T, long long n,
                   const char* fn) {
  const int rc = check_seq_desc(desc, fn, false);
  if (rc != H12LEARN_OK) return rc;
  if (!packed) return h12_learn_fail(H12LEARN_E_ARG, "%s: packed is null", fn);
  if (((uintptr_t)packed & 15) != 0) return h12_learn_fail(H12LEARN_E_ARG, "%s: packed not 16-byte aligned", fn);
  if (!io) return h12_learn_fail(H12LEARN_E_ARG, "%s: io is null", fn);
  if (T < 1 || T > SEQ_MAX_T) return h12_learn_fail(H12LEARN_E_ARG, "%s: io.T = %d (1..%d)", fn, T, SEQ_MAX_T);
  if (n < 1) return h12_learn_fail(H12LEARN_E_ARG, "%s: io.n = %lld (must be >= 1)", fn, n);
  if ((n + SEQ_ROWS - 1) / SEQ_ROWS > 0x7fffffffLL)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: io.n = %lld exceeds the grid", fn, n);
  return H12LEARN_OK;
}

}  // namespace

extern "C" {

size_t h12learn_lstm_seq_packed_bytes(const h12learn_lstm_seq_desc* desc) {
  if (check_seq_desc(desc, "lstm_seq_packed_bytes", false) != H12LEARN_OK) return 0;
  return (size_t)desc->n_nets * seq_net_floats(desc->hidden) * sizeof(float);
}

int h12learn_lstm_seq_pack(const h12learn_lstm_seq_desc* desc, float* packed, void* stream) {
  const int rc = check_seq_desc(desc, "lstm_seq_pack", true);
  if (rc != H12LEARN_OK) return rc;
  if (!packed) return h12_learn_fail(H12LEARN_E_ARG, "lstm_seq_pack: packed is null");
  if (((uintptr_t)packed & 15) != 0)
    return h12_learn_fail(H12LEARN_E_ARG, "lstm_seq_pack: packed not 16-byte aligned");
  const size_t total = h12learn_lstm_seq_packed_bytes(desc) / sizeof(float);
  const size_t blocks = (total + PACK_BLOCK - 1) / PACK_BLOCK;
  hipLaunchKernelGGL(lstm_seq_pack_kernel, dim3((unsigned)blocks), dim3(PACK_BLOCK), 0, (hipStream_t)stream, *desc,
                     packed, total);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "lstm_seq_pack launch: %s", hipGetErrorString(e));
  return H12LEARN_OK;
}

int h12learn_lstm_seq_forward(const h12learn_lstm_seq_desc* desc, const float* packed, const h12learn_lstm_seq_io* io,
                              void* stream) {
  const char* fn = "lstm_seq_forward";
  int rc = check_seq_call(desc, packed, io, io ? io->T : 1, io ? io->n : 1, fn);
  if (rc != H12LEARN_OK) return rc;
  if (!io->dones) return h12_learn_fail(H12LEARN_E_ARG, "%s: io.dones is null", fn);
  for (int i = 0; i < desc->n_nets; ++i)
    if (!io->zx[i] || !io->h0[i] || !io->c0[i] || !io->h_seq[i] || !io->c_seq[i] || !io->gates[i])
      return h12_learn_fail(H12LEARN_E_ARG, "%s: io.zx / h0 / c0 / h_seq / c_seq / gates [%d] is null", fn, i);
  const int H = desc->hidden;
  const size_t lds_bytes = seq_lds_bytes(H);
  static bool raised = false;
  rc = raise_lds_limit(reinterpret_cast<const void*>(lstm_seq_forward_kernel), &raised,
                       (int)seq_lds_bytes(SEQ_MAX_HIDDEN), lds_bytes, (hipStream_t)stream, fn);
  if (rc != H12LEARN_OK) return rc;
  const long long tiles = (io->n + SEQ_ROWS - 1) / SEQ_ROWS;
  hipLaunchKernelGGL(lstm_seq_forward_kernel, dim3((unsigned)tiles, (unsigned)desc->n_nets), dim3(THREADS), lds_bytes,
                     (hipStream_t)stream, H, packed, *io, pad16(H) + LD_PAD, pad16(4 * H) + LD_PAD);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return H12LEARN_OK;
}

int h12learn_lstm_seq_backward(const h12learn_lstm_seq_desc* desc, const float* packed,
                               const h12learn_lstm_seq_grad_io* io, void* stream) {
  const char* fn = "lstm_seq_backward";
  int rc = check_seq_call(desc, packed, io, io ? io->T : 1, io ? io->n : 1, fn);
  if (rc != H12LEARN_OK) return rc;
  if (!io->dones) return h12_learn_fail(H12LEARN_E_ARG, "%s: io.dones is null", fn);
  for (int i = 0; i < desc->n_nets; ++i)
    if (!io->dh_seq[i] || !io->gates[i] || !io->c_seq[i] || !io->c0[i] || !io->dz[i])
      return h12_learn_fail(H12LEARN_E_ARG, "%s: io.dh_seq / gates / c_seq / c0 / dz [%d] is null", fn, i);
  const int H = desc->hidden;
  const size_t lds_bytes = seq_lds_bytes(H);
  static bool raised = false;
  rc = raise_lds_limit(reinterpret_cast<const void*>(lstm_seq_backward_kernel), &raised,
                       (int)seq_lds_bytes(SEQ_MAX_HIDDEN), lds_bytes, (hipStream_t)stream, fn);
  if (rc != H12LEARN_OK) return rc;
  const long long tiles = (io->n + SEQ_ROWS - 1) / SEQ_ROWS;
  hipLaunchKernelGGL(lstm_seq_backward_kernel, dim3((unsigned)tiles, (unsigned)desc->n_nets), dim3(THREADS), lds_bytes,
                     (hipStream_t)stream, H, packed, *io, pad16(H) + LD_PAD, pad16(4 * H) + LD_PAD);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return H12LEARN_OK;
}

}  // extern "C"
