// h12_policy.hip: fused policy MLP forward of libh12env.so (include/h12learn.h, h12learn_mlp_*).
//
//   h12learn_mlp_pack      torch-layout weights W[out][in], b[out] -> the tiled, zero-padded pack (one launch)
//   h12learn_mlp_forward   normaliser + every Linear/ELU layer of up to 4 networks over one input, one launch
//
// The packed layout, the order of summation, the LDS images and the tile routines are those of h12_mlp_core.h: read
// its header first.
//
// Forward.  Grid (row tiles, networks); a block of 4 waves owns MLP_ROWS = 16 rows of x for one network.  16 rows and
// not 32: actor-only inference at 4096 rows then has 256 blocks, one per CU of the chip; with 32 rows half the CUs
// would idle.  The price is that every block streams the network's weights once from L2 for 16 rows only.
#include "h12_mlp_core.h"

namespace {

using namespace mlp;

constexpr int MLP_ROWS = 16;
constexpr int MLP_MAX_WIDTH = 1024;  // any layer width, input included

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
      const size_t wsz = matrix_floats(in, out);
      if (i < wsz) {
        int j, k;
        pack_index(i, pad16(in) / 16, &j, &k);
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

struct mlp_outputs {
  float* y[H12LEARN_MLP_MAX_NETS];
};

__global__ __launch_bounds__(THREADS) void mlp_forward_kernel(h12learn_mlp_desc desc, const float* __restrict__ packed,
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

  // the normalised input tile, zero in the padding columns and in the rows past n: load_tile of h12_mlp_core.h with
  // the normaliser between its loads and its stores.  Written out here: through load_tile and a functor the compiler
  // sets this loop up differently and the kernel measured 0.3 % slower
  const int d_in = desc.d_in, k0 = pad16(d_in);
  for (int c = threadIdx.x; c < k0; c += THREADS) {
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
    __builtin_assume(bp != nullptr);  // every layer has a bias: no test of it in tiles() (as before: DESIGN.md 7m)
    // not the last layer: ELU into hout [16][ldout]; the last layer: masked store to y [n][out]
    const bool last = l == net.n_layers - 1;
    float* y = outs.y[nidx];
    layer<1>(wp, bp, hin, ldin, kg, tiles, no_side(), [=](int j, int row, float v, float) {
      if (!last) {
        hout[row * ldout + j] = elu1(v);
      } else if (j < out && row0 + row < n) {
        y[(size_t)(row0 + row) * (size_t)out + j] = v;
      }
    });
    wp = bp + pad16(out);
    __syncthreads();
    float* tp = hin;
    hin = hout, hout = tp;
    const int tl = ldin;
    ldin = ldout, ldout = tl;
  }
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

}  // namespace

extern "C" {

int h12learn_mlp_max_width(void) { return MLP_MAX_WIDTH; }

size_t h12learn_mlp_packed_bytes(const h12learn_mlp_desc* desc) {
  if (check_desc(desc, "mlp_packed_bytes", MLP_MAX_WIDTH) != H12LEARN_OK) return 0;
  size_t s = 0;
  for (int i = 0; i < desc->n_nets; ++i) s += net_floats(desc->nets[i]);
  return s * sizeof(float);
}

int h12learn_mlp_pack(const h12learn_mlp_desc* desc, float* packed, void* stream) {
  int rc = check_desc(desc, "mlp_pack", MLP_MAX_WIDTH);
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
  int rc = check_desc(desc, "mlp_forward", MLP_MAX_WIDTH);
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
  const lds_images im = forward_images(desc);
  const size_t lds_bytes = im.bytes(MLP_ROWS);
  // wide networks only (the 450-512-256-128 policy needs 63 KiB)
  static bool raised = false;
  rc = raise_lds_limit(reinterpret_cast<const void*>(mlp_forward_kernel), &raised,
                       lds_most(MLP_ROWS, MLP_MAX_WIDTH), lds_bytes, (hipStream_t)stream, "mlp_forward");
  if (rc != H12LEARN_OK) return rc;
  hipLaunchKernelGGL(mlp_forward_kernel, dim3((unsigned)tiles, (unsigned)desc->n_nets), dim3(THREADS), lds_bytes,
                     (hipStream_t)stream, *desc, packed, x, n, outs, im.ld(0), im.ld(1));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "mlp_forward launch: %s", hipGetErrorString(e));
  return H12LEARN_OK;
}

}  // extern "C"
