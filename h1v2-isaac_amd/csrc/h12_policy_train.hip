// h12_policy_train.hip: the training side of the fused policy MLP (include/h12learn.h, h12learn_mlp_*_train / _backward).
//
//   h12learn_mlp_pack_t          W[out][in] -> the packed layout over W^T (the dgrad's B operand)
//   h12learn_mlp_forward_train   every Linear/ELU layer of ONE network in one launch; also stores every hidden h_l
//   h12learn_mlp_backward        dZ_{L-1} = dY; dH_l = dZ_{l+1} W_{l+1}; dZ_l = dH_l * f'(h_l), the chain in LDS, one
//                                launch; per-block bias-gradient partials, folded in block order by a second launch
//
// The packed layout, the order of summation, the LDS images and the tile routines are those of h12_mlp_core.h: read
// its header first.  The forward reads the SAME packed weights as h12learn_mlp_forward through the same tile routine,
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
#include "h12_mlp_core.h"

namespace {

using namespace mlp;

constexpr int TR_SUB = 2;             // 16-row sub-tiles of a block
constexpr int TR_ROWS = 16 * TR_SUB;  // rows of a block
constexpr int TR_MAX_WIDTH = 512;
constexpr int FOLD_BLOCK = 64;
constexpr int FOLD_UNROLL = 32;

__global__ __launch_bounds__(PACK_BLOCK) void mlp_pack_t_kernel(h12learn_mlp_desc desc, float* packed_t,
                                                                 size_t total) {
  size_t i = (size_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
  if (i >= total) return;
  const size_t dst = i;
  const h12learn_mlp_net& net = desc.nets[0];
  for (int l = 0; l < net.n_layers; ++l) {
    const int in = net.dims[l], out = net.dims[l + 1];
    const size_t wsz = matrix_floats(in, out);
    if (i < wsz) {
      int c, k;
      pack_index(i, pad16(out) / 16, &c, &k);  // K of the dgrad is the layer's output width; W^T[c][k] = W[k][c]
      packed_t[dst] = (c < in && k < out) ? net.W[l][(size_t)k * (size_t)in + c] : 0.f;
      return;
    }
    i -= wsz;
  }
}

struct train_ptrs {
  float* p[H12LEARN_MLP_MAX_LAYERS];
};
struct train_cptrs {
  const float* p[H12LEARN_MLP_MAX_LAYERS];
};

__global__ __launch_bounds__(THREADS) void mlp_forward_train_kernel(h12learn_mlp_desc desc,
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

  load_tile<TR_ROWS>(x, desc.d_in, row0, n, hin, ldin);
  __syncthreads();

  const float* wp = packed;
  for (int l = 0; l < net.n_layers; ++l) {
    const int in = net.dims[l], out = net.dims[l + 1];
    const int kg = pad16(in) / 16, tiles = pad16(out) / 16;
    const float* bp = wp + (size_t)pad16(in) * (size_t)pad16(out);
    if (l + 1 < net.n_layers) {
      float* hg = hs.p[l];
      float* ho = hout;
      const int ldo = ldout;
      layer<TR_SUB>(wp, bp, hin, ldin, kg, tiles, no_side(), [=](int j, int row, float v, float) {
        const float h = elu1(v);
        ho[row * ldo + j] = h;
        if (j < out && row0 + row < n) hg[(size_t)(row0 + row) * (size_t)out + j] = h;
      });
    } else {
      layer<TR_SUB>(wp, bp, hin, ldin, kg, tiles, no_side(), [=](int j, int row, float v, float) {
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
__global__ __launch_bounds__(THREADS) void mlp_backward_kernel(h12learn_mlp_desc desc,
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

  load_tile<TR_ROWS>(dy, net.dims[L], row0, n, cur, ldc);
  __syncthreads();

  // offsets of layer L - 1: the transposed pack and the bias-gradient columns
  size_t woff = 0;
  int boff = 0;
  for (int l = 0; l + 1 < L; ++l) {
    woff += matrix_floats(net.dims[l], net.dims[l + 1]);
    boff += net.dims[l + 1];
  }
  for (int l = L - 1; l >= 0; --l) {
    const int in = net.dims[l], out = net.dims[l + 1];
    for (int c = threadIdx.x; c < out; c += THREADS) {
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
      layer<TR_SUB>(
          wp, nullptr, cur, ldc, kg, tiles,
          [=](int j, int row) { return (j < in && row0 + row < n) ? hg[(size_t)(row0 + row) * (size_t)in + j] : 0.f; },
          [=](int j, int row, float v, float h) {
            const float dz = v * (h > 0.f ? 1.f : h + 1.f);
            o[row * ldo + j] = dz;
            if (j < in && row0 + row < n) dzg[(size_t)(row0 + row) * (size_t)in + j] = dz;
          });
      woff -= matrix_floats(net.dims[l - 1], in);
      boff -= in;
    } else if (dx) {
      layer<TR_SUB>(wp, nullptr, cur, ldc, kg, tiles, no_side(), [=](int j, int row, float v, float) {
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

// one network without a normaliser, no wider than TR_MAX_WIDTH
int check_train_desc(const h12learn_mlp_desc* desc, const char* fn) {
  if (desc && desc->n_nets != 1) return h12_learn_fail(H12LEARN_E_ARG, "%s: n_nets = %d (must be 1)", fn, desc->n_nets);
  if (desc && desc->norm_kind != H12LEARN_MLP_NORM_NONE)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: norm_kind = %d (H12LEARN_MLP_NORM_NONE only)", fn, desc->norm_kind);
  return check_desc(desc, fn, TR_MAX_WIDTH);
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

}  // namespace

extern "C" {

int h12learn_mlp_train_rows(void) { return TR_ROWS; }

int h12learn_mlp_train_max_width(void) { return TR_MAX_WIDTH; }

size_t h12learn_mlp_packed_t_bytes(const h12learn_mlp_desc* desc) {
  if (check_train_desc(desc, "mlp_packed_t_bytes") != H12LEARN_OK) return 0;
  size_t s = 0;
  for (int l = 0; l < desc->nets[0].n_layers; ++l)
    s += matrix_floats(desc->nets[0].dims[l], desc->nets[0].dims[l + 1]);
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
  const lds_images im = forward_images(desc);
  const size_t lds_bytes = im.bytes(TR_ROWS);
  static bool raised = false;
  rc = raise_lds_limit(reinterpret_cast<const void*>(mlp_forward_train_kernel), &raised,
                       lds_most(TR_ROWS, TR_MAX_WIDTH), lds_bytes, (hipStream_t)stream, fn);
  if (rc != H12LEARN_OK) return rc;
  const long long tiles = (n + TR_ROWS - 1) / TR_ROWS;
  hipLaunchKernelGGL(mlp_forward_train_kernel, dim3((unsigned)tiles), dim3(THREADS), lds_bytes,
                     (hipStream_t)stream, *desc, packed, x, n, y, hs, im.ld(0), im.ld(1));
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
  lds_images im;  // dZ_{L-1}, the tile loaded, first
  for (int l = 0; l < L; ++l) im.hold(L - 1 - l, net.dims[l + 1]);
  const size_t lds_bytes = im.bytes(TR_ROWS);
  static bool raised = false;
  rc = raise_lds_limit(reinterpret_cast<const void*>(mlp_backward_kernel), &raised,
                       lds_most(TR_ROWS, TR_MAX_WIDTH), lds_bytes, (hipStream_t)stream, fn);
  if (rc != H12LEARN_OK) return rc;
  const long long tiles = (n + TR_ROWS - 1) / TR_ROWS;
  const int tot = total_columns(net);
  hipLaunchKernelGGL(mlp_backward_kernel, dim3((unsigned)tiles), dim3(THREADS), lds_bytes, (hipStream_t)stream,
                     *desc, packed_t, dy, hs, n, dzs, dx, (float*)workspace, tot, im.ld(0), im.ld(1));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  hipLaunchKernelGGL(bias_fold_kernel, dim3((unsigned)((tot + FOLD_BLOCK - 1) / FOLD_BLOCK)), dim3(FOLD_BLOCK), 0,
                     (hipStream_t)stream, *desc, (const float*)workspace, tiles, tot, dbs);
  e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "%s fold launch: %s", fn, hipGetErrorString(e));
  return H12LEARN_OK;
}

}  // extern "C"
