// h12_policy_rnn.hip: fused recurrent policy step of libh12env.so (include/h12learn.h, h12learn_lstm_*).
//
//   h12learn_lstm_pack   nn.LSTM layer-0 parameters and the MLP's W / b -> the tiled, zero-padded pack (one launch)
//   h12learn_lstm_step   normaliser + LSTM cell + every Linear/ELU layer of up to 2 networks over one input, one launch
//
// The packed layout, the order of summation, the LDS images and the tile routines are those of h12_mlp_core.h: read
// its header first.  The cell is one more layer of that core: the matrix [W_ih | W_hh] ([4H][kx + kh], kx = d_in and
// kh = H each padded to 16, so no k-group straddles the two inputs) over the LDS image [x | h], the bias b_ih + b_hh
// summed at pack time.  Per network the pack holds that matrix, its padded bias [16 * tiles of 4H], then the MLP's
// layers as h12learn_mlp_pack lays them out.
//
// Step.  Grid (row tiles, networks); a block of 4 waves owns LSTM_ROWS = 16 rows for one network, as in h12_policy.hip:
//   1. the block loads its rows of x (normalised) and of h_in into LDS buffer 0 (rows whose reset byte is set read
//      h = 0), layer<1> writes the gate pre-activations [16][4H] to LDS buffer 1;
//   2. after one barrier a pointwise pass reads the gates from LDS and c_in from global memory, forms c' and h', stores
//      them to c_out / h_out and writes h' into buffer 0, now the input image of the MLP's first layer;
//   3. the MLP's layers alternate between the two buffers, the last one stores y.
// The gates never leave the CU.  A block reads every h_in element of its rows in 1 before it writes any h_out in 2,
// and an element of c is read and written by the same thread, so h_out == h_in and c_out == c_in are legal.
#include "h12_mlp_core.h"

namespace {

using namespace mlp;

constexpr int LSTM_ROWS = 16;
constexpr int LSTM_MAX_HIDDEN = 256;  // 4H stays within the core's widest layer
constexpr int LSTM_MAX_WIDTH = 1024;  // d_in and any width of the MLP

__host__ __device__ inline int lstm_k(int d_in, int hidden) { return pad16(d_in) + pad16(hidden); }

// floats of one network's pack: the cell's matrix and bias, then the MLP's layers
__host__ __device__ inline size_t lstm_net_floats(const h12learn_lstm_desc& desc, int i) {
  size_t s = layer_floats(lstm_k(desc.d_in, desc.hidden), 4 * desc.hidden);
  const h12learn_mlp_net& net = desc.mlp.nets[i];
  for (int l = 0; l < net.n_layers; ++l) s += layer_floats(net.dims[l], net.dims[l + 1]);
  return s;
}

__global__ __launch_bounds__(PACK_BLOCK) void lstm_pack_kernel(h12learn_lstm_desc desc, float* packed, size_t total) {
  size_t i = (size_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
  if (i >= total) return;
  const size_t dst = i;
  const int d_in = desc.d_in, H = desc.hidden, kx = pad16(d_in), K = lstm_k(d_in, H), G = 4 * H;
  for (int nidx = 0; nidx < desc.mlp.n_nets; ++nidx) {
    const h12learn_lstm_cell& cell = desc.cells[nidx];
    const size_t wsz = matrix_floats(K, G);
    if (i < wsz) {
      int j, k;
      pack_index(i, K / 16, &j, &k);
      float v = 0.f;
      if (j < G) {
        if (k < kx) {
          if (k < d_in) v = cell.w_ih[(size_t)j * (size_t)d_in + k];
        } else if (k - kx < H) {
          v = cell.w_hh[(size_t)j * (size_t)H + (k - kx)];
        }
      }
      packed[dst] = v;
      return;
    }
    i -= wsz;
    if (i < (size_t)pad16(G)) {
      packed[dst] = (int)i < G ? cell.b_ih[i] + cell.b_hh[i] : 0.f;
      return;
    }
    i -= (size_t)pad16(G);
    const h12learn_mlp_net& net = desc.mlp.nets[nidx];
    for (int l = 0; l < net.n_layers; ++l) {
      const int in = net.dims[l], out = net.dims[l + 1];
      const size_t lsz = matrix_floats(in, out);
      if (i < lsz) {
        int j, k;
        pack_index(i, pad16(in) / 16, &j, &k);
        packed[dst] = (j < out && k < in) ? net.W[l][(size_t)j * (size_t)in + k] : 0.f;
        return;
      }
      i -= lsz;
      if (i < (size_t)pad16(out)) {
        packed[dst] = (int)i < out ? net.b[l][i] : 0.f;
        return;
      }
      i -= (size_t)pad16(out);
    }
  }
}

// sigmoid with a true division and the library's expf
__device__ __forceinline__ float sigmoid1(float z) { return 1.f / (1.f + expf(-z)); }

__global__ __launch_bounds__(THREADS) void lstm_step_kernel(h12learn_lstm_desc desc, const float* __restrict__ packed,
                                                            h12learn_lstm_io io, int ld0, int ld1) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* buf0 = lds;
  float* buf1 = lds + LSTM_ROWS * ld0;
  const int nidx = blockIdx.y;
  const h12learn_mlp_net& net = desc.mlp.nets[nidx];
  const long long n = io.n;
  const long long row0 = (long long)blockIdx.x * LSTM_ROWS;
  const int d_in = desc.d_in, H = desc.hidden, kx = pad16(d_in), kh = pad16(H), G = 4 * H;

  const float* wp = packed;
  for (int i = 0; i < nidx; ++i) wp += lstm_net_floats(desc, i);

  // image 0: [x normalised | h], zero in both paddings and in the rows past n; a reset row reads h = 0
  const float* x = io.x;
  const float* h_in = io.h_in[nidx];
  const unsigned char* reset = io.reset;
  for (int c = threadIdx.x; c < kx + kh; c += THREADS) {
    float v[LSTM_ROWS];
    if (c < kx) {
#pragma unroll
      for (int r = 0; r < LSTM_ROWS; ++r)
        v[r] = (c < d_in && row0 + r < n) ? x[(size_t)(row0 + r) * (size_t)d_in + c] : 0.f;
      if (c < d_in && desc.norm_kind != H12LEARN_MLP_NORM_NONE) {
        const float m = desc.norm_mean[c];
        const float sc = desc.norm_kind == H12LEARN_MLP_NORM_VAR ? sqrtf(desc.norm_scale[c] + desc.norm_eps)
                                                                 : desc.norm_scale[c] + desc.norm_eps;
#pragma unroll
        for (int r = 0; r < LSTM_ROWS; ++r)
          if (row0 + r < n) v[r] = (v[r] - m) / sc;  // rows past n stay zero
      }
    } else {
      const int u = c - kx;
#pragma unroll
      for (int r = 0; r < LSTM_ROWS; ++r) {
        const bool live = u < H && row0 + r < n && !(reset && reset[row0 + r]);
        v[r] = live ? h_in[(size_t)(row0 + r) * (size_t)H + u] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < LSTM_ROWS; ++r) buf0[r * ld0 + c] = v[r];
  }
  __syncthreads();

  // the gate pre-activations z = [x | h] [W_ih | W_hh]^T + (b_ih + b_hh) into buffer 1
  {
    const int K = kx + kh;
    const float* bp = wp + matrix_floats(K, G);
    __builtin_assume(bp != nullptr);
    layer<1>(wp, bp, buf0, ld0, K / 16, pad16(G) / 16, no_side(),
             [=](int j, int row, float v, float) { buf1[row * ld1 + j] = v; });
    wp = bp + pad16(G);
  }
  __syncthreads();

  // pointwise: torch's gate order i, f, g, o.  h' becomes the MLP's input image in buffer 0, zero past H
  {
    const float* c_in = io.c_in[nidx];
    float* h_out = io.h_out[nidx];
    float* c_out = io.c_out[nidx];
    for (int e = threadIdx.x; e < LSTM_ROWS * kh; e += THREADS) {
      const int row = e / kh, u = e - row * kh;
      float hn = 0.f;
      if (u < H) {
        const float* z = buf1 + row * ld1 + u;
        const bool valid = row0 + row < n;
        const size_t at = (size_t)(row0 + row) * (size_t)H + u;
        const float cp = (valid && !(reset && reset[row0 + row])) ? c_in[at] : 0.f;
        const float ig = sigmoid1(z[0]), fg = sigmoid1(z[H]), gg = tanhf(z[2 * H]), og = sigmoid1(z[3 * H]);
        const float cn = fg * cp + ig * gg;
        hn = og * tanhf(cn);
        if (valid) {
          c_out[at] = cn;
          h_out[at] = hn;
        }
      }
      buf0[row * ld0 + u] = hn;
    }
  }
  __syncthreads();

  float* hin = buf0;
  float* hout = buf1;
  int ldin = ld0, ldout = ld1;
  for (int l = 0; l < net.n_layers; ++l) {
    const int in = net.dims[l], out = net.dims[l + 1];
    const int kg = pad16(in) / 16, tiles = pad16(out) / 16;
    const float* bp = wp + (size_t)pad16(in) * (size_t)pad16(out);
    __builtin_assume(bp != nullptr);
    const bool last = l == net.n_layers - 1;
    float* y = io.y[nidx];
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

// buffer 0: [x | h], then the MLP's even images (its input h' first); buffer 1: the gates, then the odd images
lds_images step_images(int d_in, int hidden, const h12learn_mlp_desc* m) {
  lds_images im;
  im.hold(0, lstm_k(d_in, hidden));
  im.hold(1, 4 * hidden);
  if (m)
    for (int i = 0; i < m->n_nets; ++i)
      for (int l = 0; l + 1 < m->nets[i].n_layers; ++l) im.hold(l + 1, m->nets[i].dims[l + 1]);
  return im;
}

int check_lstm(const h12learn_lstm_desc* desc, const char* fn, bool pointers) {
  if (!desc) return h12_learn_fail(H12LEARN_E_ARG, "%s: desc is null", fn);
  if (desc->mlp.n_nets < 1 || desc->mlp.n_nets > H12LEARN_LSTM_MAX_NETS)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: mlp.n_nets = %d (1..%d)", fn, desc->mlp.n_nets, H12LEARN_LSTM_MAX_NETS);
  if (desc->hidden < 1 || desc->hidden > LSTM_MAX_HIDDEN)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: hidden = %d (1..%d)", fn, desc->hidden, LSTM_MAX_HIDDEN);
  if (desc->d_in < 1 || desc->d_in > LSTM_MAX_WIDTH)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: d_in = %d (1..%d)", fn, desc->d_in, LSTM_MAX_WIDTH);
  if (desc->norm_kind != H12LEARN_MLP_NORM_NONE && desc->norm_kind != H12LEARN_MLP_NORM_VAR &&
      desc->norm_kind != H12LEARN_MLP_NORM_STD)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: norm_kind = %d", fn, desc->norm_kind);
  if (desc->norm_kind != H12LEARN_MLP_NORM_NONE && (!desc->norm_mean || !desc->norm_scale))
    return h12_learn_fail(H12LEARN_E_ARG, "%s: norm_mean / norm_scale is null", fn);
  if (desc->mlp.norm_kind != H12LEARN_MLP_NORM_NONE)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: mlp.norm_kind = %d (the normaliser is the desc's own, on x)", fn,
                          desc->mlp.norm_kind);
  if (desc->mlp.d_in != desc->hidden)
    return h12_learn_fail(H12LEARN_E_ARG, "%s: mlp.d_in = %d differs from hidden = %d", fn, desc->mlp.d_in,
                          desc->hidden);
  const int rc = check_desc(&desc->mlp, fn, LSTM_MAX_WIDTH);
  if (rc != H12LEARN_OK || !pointers) return rc;
  for (int i = 0; i < desc->mlp.n_nets; ++i) {
    const h12learn_lstm_cell& c = desc->cells[i];
    if (!c.w_ih || !c.w_hh || !c.b_ih || !c.b_hh)
      return h12_learn_fail(H12LEARN_E_ARG, "%s: cells[%d].w_ih / w_hh / b_ih / b_hh is null", fn, i);
    for (int l = 0; l < desc->mlp.nets[i].n_layers; ++l)
      if (!desc->mlp.nets[i].W[l] || !desc->mlp.nets[i].b[l])
        return h12_learn_fail(H12LEARN_E_ARG, "%s: mlp.nets[%d].W[%d] / b[%d] is null", fn, i, l, l);
  }
  return H12LEARN_OK;
}

}  // namespace

extern "C" {

int h12learn_lstm_max_hidden(void) { return LSTM_MAX_HIDDEN; }

size_t h12learn_lstm_packed_bytes(const h12learn_lstm_desc* desc) {
  if (check_lstm(desc, "lstm_packed_bytes", false) != H12LEARN_OK) return 0;
  size_t s = 0;
  for (int i = 0; i < desc->mlp.n_nets; ++i) s += lstm_net_floats(*desc, i);
  return s * sizeof(float);
}

int h12learn_lstm_pack(const h12learn_lstm_desc* desc, float* packed, void* stream) {
  const int rc = check_lstm(desc, "lstm_pack", true);
  if (rc != H12LEARN_OK) return rc;
  if (!packed) return h12_learn_fail(H12LEARN_E_ARG, "lstm_pack: packed is null");
  if (((uintptr_t)packed & 15) != 0) return h12_learn_fail(H12LEARN_E_ARG, "lstm_pack: packed not 16-byte aligned");
  const size_t total = h12learn_lstm_packed_bytes(desc) / sizeof(float);
  const size_t blocks = (total + PACK_BLOCK - 1) / PACK_BLOCK;
  hipLaunchKernelGGL(lstm_pack_kernel, dim3((unsigned)blocks), dim3(PACK_BLOCK), 0, (hipStream_t)stream, *desc, packed,
                     total);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "lstm_pack launch: %s", hipGetErrorString(e));
  return H12LEARN_OK;
}

int h12learn_lstm_step(const h12learn_lstm_desc* desc, const float* packed, const h12learn_lstm_io* io, void* stream) {
  int rc = check_lstm(desc, "lstm_step", false);
  if (rc != H12LEARN_OK) return rc;
  if (!packed) return h12_learn_fail(H12LEARN_E_ARG, "lstm_step: packed is null");
  if (((uintptr_t)packed & 15) != 0) return h12_learn_fail(H12LEARN_E_ARG, "lstm_step: packed not 16-byte aligned");
  if (!io) return h12_learn_fail(H12LEARN_E_ARG, "lstm_step: io is null");
  if (!io->x) return h12_learn_fail(H12LEARN_E_ARG, "lstm_step: io.x is null");
  if (io->n < 1) return h12_learn_fail(H12LEARN_E_ARG, "lstm_step: io.n = %lld (must be >= 1)", io->n);
  for (int i = 0; i < desc->mlp.n_nets; ++i)
    if (!io->h_in[i] || !io->c_in[i] || !io->h_out[i] || !io->c_out[i] || !io->y[i])
      return h12_learn_fail(H12LEARN_E_ARG, "lstm_step: io.h_in / c_in / h_out / c_out / y [%d] is null", i);
  const long long tiles = (io->n + LSTM_ROWS - 1) / LSTM_ROWS;
  if (tiles > 0x7fffffffLL) return h12_learn_fail(H12LEARN_E_ARG, "lstm_step: io.n = %lld exceeds the grid", io->n);
  const lds_images im = step_images(desc->d_in, desc->hidden, &desc->mlp);
  const size_t lds_bytes = im.bytes(LSTM_ROWS);
  // the real shape (450 inputs, H = 256) needs about 110 KiB
  static bool raised = false;
  const size_t most = step_images(LSTM_MAX_WIDTH, LSTM_MAX_HIDDEN, nullptr).bytes(LSTM_ROWS);
  rc = raise_lds_limit(reinterpret_cast<const void*>(lstm_step_kernel), &raised, (int)most, lds_bytes,
                       (hipStream_t)stream, "lstm_step");
  if (rc != H12LEARN_OK) return rc;
  hipLaunchKernelGGL(lstm_step_kernel, dim3((unsigned)tiles, (unsigned)desc->mlp.n_nets), dim3(THREADS), lds_bytes,
                     (hipStream_t)stream, *desc, packed, *io, im.ld(0), im.ld(1));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h12_learn_fail(H12LEARN_E_HIP, "lstm_step launch: %s", hipGetErrorString(e));
  return H12LEARN_OK;
}

}  // extern "C"
