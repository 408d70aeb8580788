// h12_optim.hip: one optimiser step of both trainers in two launches (include/h12learn.h, h12learn_optim_*; DESIGN.md
// section 7u): the global gradient norm, then the clip coefficient and the Adam or RAdam update of every tensor.
//
//   optim_norm_kernel          per block the fp64 sum of g^2 over its chunk -> partial[block]; step[t] += 1
//   optim_apply_kernel<rule>   every block folds all partials, forms the step's scalars in double, updates its chunk
//
// Table.  The tensors' pointers travel in the kernel arguments (optim_table, at most OPT_MAX_TENSORS per launch), as
// torch's multi-tensor apply passes them: no device copy, and a captured step replays the addresses it saw.  A block
// owns one chunk of OPT_CHUNK elements of one tensor; chunk_end[] is the running count of chunks, and the block finds its
// tensor by bisection in it.  More tensors than the table holds are more launches of each kernel: every norm launch
// writes its own range of partial[], every apply launch folds the whole of it.
//
// Ownership.  Thread t of a block owns the 4-element groups t, t + OPT_THREADS, .. of the chunk, that is elements
// 4 t + j + 4 OPT_THREADS i.  Where p, g, exp_avg and exp_avg_sq are all 16-byte aligned a whole group is one 16-byte
// access; otherwise, and for the group the tensor ends in, the same elements move one by one.  Which thread owns which
// element, and hence every sum's order, depends on the tensor sizes alone, never on the alignment.
//
// Sums.  g^2 is exact in fp64.  A thread adds its elements in index order, a wave its lanes by an xor butterfly (32, 16,
// .., 1), the block its waves in wave order.  The apply kernel stages OPT_FOLD partials at a time in LDS and every thread
// adds them in block-index order.  No atomics, no arrival counter: launch 2 starts after launch 1 on the stream.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/h12learn.h"

// defined in h12_learn.hip: records the calling thread's h12learn_last_error message and returns code
int h12_learn_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3), visibility("hidden")));

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_WAVES = OPT_THREADS / 64;
constexpr int OPT_CHUNK = 2048;  // elements of a block: OPT_GROUPS 4-element groups per thread
constexpr int OPT_GROUPS = OPT_CHUNK / (4 * OPT_THREADS);
constexpr int OPT_MAX_TENSORS = 64;
constexpr int OPT_FOLD = OPT_THREADS;  // partials staged at a time by the apply kernel's fold
static_assert(OPT_GROUPS * 4 * OPT_THREADS == OPT_CHUNK, "a chunk is a whole number of groups per thread");

using f32x4 = __attribute__((ext_vector_type(4))) float;

struct optim_table {
  float* p[OPT_MAX_TENSORS];
  const float* g[OPT_MAX_TENSORS];
  float* m[OPT_MAX_TENSORS];
  float* v[OPT_MAX_TENSORS];
  float* step[OPT_MAX_TENSORS];
  long long numel[OPT_MAX_TENSORS];
  int chunk_end[OPT_MAX_TENSORS];  // chunks of tensors 0..t of this launch
  int n;
};

struct optim_scalars {
  double beta1, beta2, eps, max_norm, lr;
  const float* lr_dev;
  float* grad_norm;  // written by block 0 when not null
  const double* partial;
  int n_partials;  // of the whole step
};

// the tensor of this block and the block's first element in it
__device__ __forceinline__ int find_tensor(const optim_table& tab, int block, long long* e0) {
  int lo = 0, hi = tab.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (block < tab.chunk_end[mid]) hi = mid; else lo = mid + 1;
  }
  const int first = lo ? tab.chunk_end[lo - 1] : 0;
  *e0 = (long long)(block - first) * OPT_CHUNK;
  return lo;
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// a group of 4 elements starting at e (a multiple of 4): whole and vector when it lies inside the tensor
__device__ __forceinline__ void load4(const float* __restrict__ src, long long e, long long numel, bool vec, float (&x)[4]) {
  if (vec && e + 4 <= numel) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(src + e);
    x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = e + j < numel ? src[e + j] : 0.f;
  }
}

__device__ __forceinline__ void store4(float* __restrict__ dst, long long e, long long numel, bool vec, const float (&x)[4]) {
  if (vec && e + 4 <= numel) {
    f32x4 q;
    q.x = x[0], q.y = x[1], q.z = x[2], q.w = x[3];
    *reinterpret_cast<f32x4*>(dst + e) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (e + j < numel) dst[e + j] = x[j];
  }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_norm_kernel(optim_table tab, double* __restrict__ partial) {
  __shared__ double red[OPT_WAVES];
  long long e0;
  const int t = find_tensor(tab, blockIdx.x, &e0);
  const float* __restrict__ g = tab.g[t];
  const long long numel = tab.numel[t];
  // the same test as the apply kernel's, so that both kernels agree on the path of a tensor
  const bool vec = aligned16(tab.p[t], g, tab.m[t], tab.v[t]);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < OPT_GROUPS; ++i) {
    const long long e = e0 + 4 * ((long long)threadIdx.x + (long long)OPT_THREADS * i);
    if (e >= numel) break;
    float x[4];
    load4(g, e, numel, vec, x);
#pragma unroll
    for (int j = 0; j < 4; ++j) s += (double)x[j] * (double)x[j];  // elements past the end are zero: they add +0
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double b = red[0];
#pragma unroll
    for (int w = 1; w < OPT_WAVES; ++w) b += red[w];
    partial[blockIdx.x] = b;
    if (e0 == 0) *tab.step[t] = *tab.step[t] + 1.f;  // the tensor's first chunk: one writer per tensor
  }
}

// Per element every operation is separately rounded (no contraction): the fp32 operations of torch's kernels.
template <int RULE>
__global__ __launch_bounds__(OPT_THREADS) void optim_apply_kernel(optim_table tab, optim_scalars sc) {
#pragma clang fp contract(off)
  __shared__ double stage[OPT_FOLD];
  // the whole step's sum of squares, in block-index order; every thread adds the same numbers in the same order
  double S = 0.0;
  for (int base = 0; base < sc.n_partials; base += OPT_FOLD) {
    const int cnt = min(OPT_FOLD, sc.n_partials - base);
    __syncthreads();  // the stage may still be read from the round before
    if ((int)threadIdx.x < cnt) stage[threadIdx.x] = sc.partial[base + threadIdx.x];
    __syncthreads();
    for (int i = 0; i < cnt; ++i) S += stage[i];
  }
  const double norm = sqrt(S);
  const double coef = sc.max_norm > 0.0 ? fmin(1.0, sc.max_norm / (norm + 1e-6)) : 1.0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && sc.grad_norm) *sc.grad_norm = (float)norm;

  long long e0;
  const int t = find_tensor(tab, blockIdx.x, &e0);
  float* __restrict__ p = tab.p[t];
  const float* __restrict__ g = tab.g[t];
  float* __restrict__ m = tab.m[t];
  float* __restrict__ v = tab.v[t];
  const long long numel = tab.numel[t];
  const bool vec = aligned16(p, g, m, v);

  // the step's scalars in double from the step count (launch 1 has incremented it), each narrowed once
  const double s = (double)*tab.step[t];
  const double lr = sc.lr_dev ? (double)*sc.lr_dev : sc.lr;
  const double b2s = pow(sc.beta2, s);
  const double bc1 = 1.0 - pow(sc.beta1, s);
  const double bc2 = 1.0 - b2s;
  const float coef_f = (float)coef;
  const float omb1 = (float)(1.0 - sc.beta1), beta2_f = (float)sc.beta2, omb2 = (float)(1.0 - sc.beta2);
  const float eps_f = (float)sc.eps;
  const float bc2_sqrt = (float)sqrt(bc2);
  // Adam
  const float neg_step_size = (float)(-(lr / bc1));
  // RAdam
  const double rho_inf = 2.0 / (1.0 - sc.beta2) - 1.0;
  const double rho_t = rho_inf - 2.0 * s * b2s / bc2;
  const bool rectified = rho_t > 5.0;
  const float bc1_f = (float)bc1, lr_f = (float)lr;
  const float rect = rectified ? (float)sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf /
                                             ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
                               : 1.f;

#pragma unroll
  for (int i = 0; i < OPT_GROUPS; ++i) {
    const long long e = e0 + 4 * ((long long)threadIdx.x + (long long)OPT_THREADS * i);
    if (e >= numel) break;
    float pp[4], gg[4], mm[4], vv[4];
    load4(p, e, numel, vec, pp);
    load4(g, e, numel, vec, gg);
    load4(m, e, numel, vec, mm);
    load4(v, e, numel, vec, vv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gc = gg[j] * coef_f;
      const float m1 = mm[j] + (gc - mm[j]) * omb1;
      float v1 = vv[j] * beta2_f;
      v1 = v1 + omb2 * (gc * gc);
      mm[j] = m1;
      vv[j] = v1;
      if (RULE == H12LEARN_OPTIM_ADAM) {
        const float denom = sqrtf(v1) / bc2_sqrt + eps_f;
        pp[j] = pp[j] + neg_step_size * (m1 / denom);
      } else {
        float u = (m1 / bc1_f) * lr_f;
        if (rectified) {
          const float alr = (1.f / (sqrtf(v1) + eps_f)) * bc2_sqrt;
          u = (u * alr) * rect;
        }
        pp[j] = pp[j] - u;
      }
    }
    store4(p, e, numel, vec, pp);
    store4(m, e, numel, vec, mm);
    store4(v, e, numel, vec, vv);
  }
}

long long chunks_of(long long numel) { return (numel + OPT_CHUNK - 1) / OPT_CHUNK; }

// the whole step's chunk count, or -1 with the error set
long long total_chunks(const long long* numel, int n_tensors, const char* fn) {
  if (n_tensors < 1) return h12_learn_fail(H12LEARN_E_ARG, "%s: n_tensors = %d (must be >= 1)", fn, n_tensors);
  if (!numel) return h12_learn_fail(H12LEARN_E_ARG, "%s: numel is null", fn);
  long long total = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (numel[t] < 1) return h12_learn_fail(H12LEARN_E_ARG, "%s: numel[%d] = %lld (must be >= 1)", fn, t, numel[t]);
    if (numel[t] > (1LL << 40)) return h12_learn_fail(H12LEARN_E_ARG, "%s: numel[%d] = %lld is too large", fn, t, numel[t]);
    total += chunks_of(numel[t]);
    if (total > 0x7fffffffLL)
      return h12_learn_fail(H12LEARN_E_ARG, "%s: numel[0..%d] need more than 2^31 - 1 blocks", fn, t);
  }
  return total;
}

int check_entry(const void* ptr, const char* field, int t, size_t align) {
  if (!ptr) return h12_learn_fail(H12LEARN_E_ARG, "optim_step: %s[%d] is null", field, t);
  if ((uintptr_t)ptr & (align - 1))
    return h12_learn_fail(H12LEARN_E_ARG, "optim_step: %s[%d] not %zu-byte aligned", field, t, align);
  return H12LEARN_OK;
}

}  // namespace

extern "C" {

int h12learn_optim_chunk(void) { return OPT_CHUNK; }

int h12learn_optim_max_tensors(void) { return OPT_MAX_TENSORS; }

int h12learn_optim_fold(void) { return OPT_FOLD; }

size_t h12learn_optim_workspace_bytes(const long long* numel, int n_tensors) {
  const long long total = total_chunks(numel, n_tensors, "optim_workspace_bytes");
  return total < 0 ? 0 : (size_t)total * sizeof(double);
}

int h12learn_optim_step(const h12learn_optim_args* a, void* stream) {
  if (!a) return h12_learn_fail(H12LEARN_E_ARG, "optim_step: args is null");
  if (a->rule != H12LEARN_OPTIM_ADAM && a->rule != H12LEARN_OPTIM_RADAM)
    return h12_learn_fail(H12LEARN_E_ARG, "optim_step: rule = %d (H12LEARN_OPTIM_ADAM or H12LEARN_OPTIM_RADAM)", a->rule);
  if (!(a->beta1 >= 0.0 && a->beta1 < 1.0))
    return h12_learn_fail(H12LEARN_E_ARG, "optim_step: beta1 = %g (0 <= beta1 < 1)", a->beta1);
  if (!(a->beta2 >= 0.0 && a->beta2 < 1.0))
    return h12_learn_fail(H12LEARN_E_ARG, "optim_step: beta2 = %g (0 <= beta2 < 1)", a->beta2);
  if (!(a->eps > 0.0 && a->eps <= DBL_MAX))
    return h12_learn_fail(H12LEARN_E_ARG, "optim_step: eps = %g (must be > 0 and finite)", a->eps);
  if (!(a->max_norm >= -DBL_MAX && a->max_norm <= DBL_MAX))
    return h12_learn_fail(H12LEARN_E_ARG, "optim_step: max_norm = %g (finite; <= 0: no clip)", a->max_norm);
  if (a->lr_dev) {
    if ((uintptr_t)a->lr_dev & 3) return h12_learn_fail(H12LEARN_E_ARG, "optim_step: lr_dev not 4-byte aligned");
  } else if (!(a->lr >= 0.0 && a->lr <= DBL_MAX)) {
    return h12_learn_fail(H12LEARN_E_ARG, "optim_step: lr = %g (must be >= 0 and finite)", a->lr);
  }
  const long long total = total_chunks(a->numel, a->n_tensors, "optim_step");
  if (total < 0) return (int)total;
  if (!a->p) return h12_learn_fail(H12LEARN_E_ARG, "optim_step: p is null");
  if (!a->g) return h12_learn_fail(H12LEARN_E_ARG, "optim_step: g is null");
  if (!a->exp_avg) return h12_learn_fail(H12LEARN_E_ARG, "optim_step: exp_avg is null");
  if (!a->exp_avg_sq) return h12_learn_fail(H12LEARN_E_ARG, "optim_step: exp_avg_sq is null");
  if (!a->step) return h12_learn_fail(H12LEARN_E_ARG, "optim_step: step is null");
  for (int t = 0; t < a->n_tensors; ++t) {
    int rc;
    if ((rc = check_entry(a->p[t], "p", t, 4)) != H12LEARN_OK) return rc;
    if ((rc = check_entry(a->g[t], "g", t, 4)) != H12LEARN_OK) return rc;
    if ((rc = check_entry(a->exp_avg[t], "exp_avg", t, 4)) != H12LEARN_OK) return rc;
    if ((rc = check_entry(a->exp_avg_sq[t], "exp_avg_sq", t, 4)) != H12LEARN_OK) return rc;
    if ((rc = check_entry(a->step[t], "step", t, 4)) != H12LEARN_OK) return rc;
  }
  if (a->grad_norm && ((uintptr_t)a->grad_norm & 3))
    return h12_learn_fail(H12LEARN_E_ARG, "optim_step: grad_norm not 4-byte aligned");
  if (!a->workspace) return h12_learn_fail(H12LEARN_E_ARG, "optim_step: workspace is null");
  if ((uintptr_t)a->workspace & 7) return h12_learn_fail(H12LEARN_E_ARG, "optim_step: workspace not 8-byte aligned");
  if (a->workspace_bytes < (size_t)total * sizeof(double))
    return h12_learn_fail(H12LEARN_E_ARG, "optim_step: workspace_bytes = %zu, %zu are needed", a->workspace_bytes,
                          (size_t)total * sizeof(double));

  double* partial = static_cast<double*>(a->workspace);
  optim_scalars sc = {a->beta1, a->beta2, a->eps, a->max_norm, a->lr, a->lr_dev, a->grad_norm, partial, (int)total};
  // pass 0: every norm launch; pass 1: every apply launch, each over the same slices of the tensor list
  for (int pass = 0; pass < 2; ++pass) {
    long long first_block = 0;
    for (int t0 = 0; t0 < a->n_tensors; t0 += OPT_MAX_TENSORS) {
      optim_table tab = {};
      tab.n = a->n_tensors - t0 < OPT_MAX_TENSORS ? a->n_tensors - t0 : OPT_MAX_TENSORS;
      int blocks = 0;
      for (int i = 0; i < tab.n; ++i) {
        tab.p[i] = a->p[t0 + i];
        tab.g[i] = a->g[t0 + i];
        tab.m[i] = a->exp_avg[t0 + i];
        tab.v[i] = a->exp_avg_sq[t0 + i];
        tab.step[i] = a->step[t0 + i];
        tab.numel[i] = a->numel[t0 + i];
        blocks += (int)chunks_of(a->numel[t0 + i]);
        tab.chunk_end[i] = blocks;
      }
      if (pass == 0) {
        hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tab,
                           partial + first_block);
      } else {
        if (t0 > 0) sc.grad_norm = nullptr;  // the step's first apply launch writes it
        if (a->rule == H12LEARN_OPTIM_ADAM)
          hipLaunchKernelGGL(optim_apply_kernel<H12LEARN_OPTIM_ADAM>, dim3((unsigned)blocks), dim3(OPT_THREADS), 0,
                             (hipStream_t)stream, tab, sc);
        else
          hipLaunchKernelGGL(optim_apply_kernel<H12LEARN_OPTIM_RADAM>, dim3((unsigned)blocks), dim3(OPT_THREADS), 0,
                             (hipStream_t)stream, tab, sc);
      }
      hipError_t e = hipGetLastError();
      if (e != hipSuccess)
        return h12_learn_fail(H12LEARN_E_HIP, "optim_step launch (%s): %s", pass ? "apply" : "norm", hipGetErrorString(e));
      first_block += blocks;
    }
  }
  return H12LEARN_OK;
}

}  // extern "C"
