// h12_student.hip: the deployable ("student") observation rows (include/h12student.h).  One
// launch per call, 256 threads per block; a block owns STU_EPB = 32 consecutive envs (at H = 10 its staged rows are
// 56 KiB of LDS, so two blocks still share a CU; 8192 envs are 256 blocks, one per CU).  Three phases, a barrier
// between each:
//   1. the new frame of every env of the block, [env][45] in LDS, noise added and scaled:
//        wave 0        one lane per env: angular velocity, projected gravity (h12_priv.hip's expression), command
//        waves 1-3     the 36 joint rows (Q - Q0, QD, ACT), lanes across envs: contiguous 128-byte segments of the
//                      field-major workspace; a thread's loads are issued together, then noise, scale and LDS stores
//      and, beside it, the column table of the row (W entries: frame column, term width, newest-slot flag) and the
//      per-env fill flag (H12_I_PACK bits 9-10 == 0 or, when the caller gives one, its fill mask; or no prev at all)
//   2. the rows as they lie in the output ([env][W], term-major), a wave per row, lanes across columns: a column of the
//      newest slot, or of a row that fills, takes the frame value from LDS; every other column is prev one frame on
//      (column + the term's width): a straight copy with a per-term offset, read coalesced along the row
//   3. the block's rows leave as ONE contiguous span of nb * W floats in 16-byte stores (32 * 45 * H * 4 bytes per full
//      block, a multiple of 16); the last (nb * W) % 4 floats of a ragged last block leave in scalar stores.
// The noise of frame column c of env e is a pure function of (seed, env_offset + e, step index, c): Philox stream 5,
// block c >> 2, word c & 3 -- nothing of n, the grid or the shard enters.  A thread draws the block of its own column:
// the 45 columns of an env are spread over threads, so an env's 12 blocks are drawn 30 times, several of them one after
// another in a joint thread.  That is what the launch waits for at H = 1 (measured latency-bound, not traffic-bound: DESIGN.md
// section 7s); drawing each block once per env and sharing it through LDS is the known next step.
// Everything is arithmetic into fixed addresses: a non-finite base state only makes its own columns non-finite.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/h12student.h"
#include "h12_math.h"
#include "h12_model_gen.h"

namespace {

constexpr int STU_BLOCK = 256;  // threads per block
constexpr int STU_EPB = 32;     // envs per block
constexpr int FRAME = H12STUDENT_FRAME;
constexpr int NJ3 = 3 * H12_NJ;  // joint_pos, joint_vel, actions
constexpr int COL_JOINT = 9;
constexpr int MAX_W = FRAME * H12STUDENT_MAX_HISTORY;
constexpr int COL_PASSES = (MAX_W + 63) / 64;  // phase 2: column passes of a wave over one row
static_assert(H12_F_QD == H12_F_Q + H12_NJ && H12_F_ACT == H12_F_QD + H12_NJ, "Q, QD, ACT are 36 consecutive fields");
static_assert(COL_JOINT + NJ3 == FRAME, "frame width");
static_assert((STU_EPB * FRAME * sizeof(float)) % 16 == 0, "a block's span and the LDS carve start on 16-byte boundaries");
static_assert(STU_EPB <= 64 && (STU_EPB & (STU_EPB - 1)) == 0, "envs per block");
// the right leg's default pose is the left leg's with the yaw / roll joints negated: those defaults are 0, so the
// per-leg table serves both legs
static_assert(h12m::Q0[0] == 0.f && h12m::Q0[2] == 0.f && h12m::Q0[5] == 0.f, "mirrored joints with a non-zero default");

constexpr int TERM_OFF[H12STUDENT_NTERMS] = {0, 3, 6, 9, 21, 33};
constexpr int TERM_WIDTH[H12STUDENT_NTERMS] = {3, 3, 3, H12_NJ, H12_NJ, H12_NJ};

struct StuArgs {
  const float* F;
  const int32_t* I;
  int n;
  const float* prev;
  const uint8_t* fill_mask;
  float* out;
  int H, W;
  uint32_t seed_lo, seed_hi, env_offset, step_lo, step_hi;
  // per term: the noise half-width (0: the term takes no noise) and the scale
  float nz0, nz1, nz2, nz3, nz4, nz5;
  float sc0, sc1, sc2, sc3, sc4, sc5;
};

__device__ __forceinline__ float q0_of(int k) {  // h12m::Q0[k % 6] without an indexed constant table
  const int j = k >= 6 ? k - 6 : k;
  return j == 1 ? h12m::Q0[1] : (j == 3 ? h12m::Q0[3] : (j == 4 ? h12m::Q0[4] : 0.f));
}

// R[2][:] of the base orientation, h12_priv.hip's expressions
//   tq = 2 / (qw qw + qx qx + qy qy + qz qz);  tq (qx qz - qw qy),  tq (qy qz + qw qx),  1 - tq (qx qx + qy qy)
// with every multiply-add explicit and contraction off.  Which products of such an expression the compiler fuses
// depends on what else uses them, and priv_obs_kernel computes the whole matrix: the same C text fuses differently in
// the two kernels (an add of two products against a fused multiply-add in 1 - tq (qx qx + qy qy): one rounding, up to
// 9 ulp after the cancellation against 1).  The sequence below is the one priv_obs_kernel compiles to, so the projected
// gravity of both groups is the same bits; tests/test_gpu_student.py compares them and fails if either side drifts.
__device__ __forceinline__ void gravity_row(float qw, float qx, float qy, float qz, float* R2) {
#pragma clang fp contract(off)
  const float n2 = __builtin_fmaf(qz, qz, __builtin_fmaf(qy, qy, __builtin_fmaf(qw, qw, qx * qx)));
  const float tq = 2.f / n2;
  R2[0] = __builtin_fmaf(qx, qz, -(qw * qy)) * tq;
  R2[1] = __builtin_fmaf(qw, qx, qy * qz) * tq;
  R2[2] = __builtin_fmaf(-__builtin_fmaf(qx, qx, qy * qy), tq, 1.f);
}

// (value + U(-nz, nz)) * sc of frame column c of global env g; nz == 0: value * sc, the noise path is not entered
__device__ __forceinline__ float corrupt(const StuArgs& A, uint32_t g, int c, float v, float nz, float sc) {
  if (nz > 0.f) {
    uint32_t r[4];
    h12::philox(A.seed_lo, A.seed_hi, g, A.step_lo, ((uint32_t)H12STUDENT_RNG_STREAM << 16) | (uint32_t)(c >> 2), A.step_hi, r);
    const int k = c & 3;
    const uint32_t x = k == 0 ? r[0] : (k == 1 ? r[1] : (k == 2 ? r[2] : r[3]));
    v += __builtin_fmaf(2.f * nz, h12::u01(x), -nz);
  }
  return v * sc;
}

__global__ __launch_bounds__(STU_BLOCK) void student_obs_kernel(StuArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int W = A.W, H = A.H, n = A.n, t = threadIdx.x;
  float* rows = lds;                              // [STU_EPB][W]
  float* fr = rows + STU_EPB * W;                 // [STU_EPB][FRAME]
  int* s_fill = reinterpret_cast<int*>(fr + STU_EPB * FRAME);  // [STU_EPB]
  int* s_tab = s_fill + STU_EPB;                  // [W]: frame column | term width << 8 | newest slot << 16
  const int e0 = blockIdx.x * STU_EPB;
  const int nb = n - e0 < STU_EPB ? n - e0 : STU_EPB;

  // ---- phase 1: the column table, the fill flags, the new frames
  for (int c = t; c < W; c += STU_BLOCK) {
    const int term = c < 3 * H ? 0 : (c < 6 * H ? 1 : (c < 9 * H ? 2 : (c < 21 * H ? 3 : (c < 33 * H ? 4 : 5))));
    const int off = term < 3 ? 3 * term : 9 + H12_NJ * (term - 3), w = term < 3 ? 3 : H12_NJ;
    const int l = c - off * H;
    const int h = term < 3 ? l / 3 : l / H12_NJ;
    s_tab[c] = (off + (l - h * w)) | (w << 8) | (h == H - 1 ? (1 << 16) : 0);
  }
  if (t < 64) {
    if (t < nb) {  // nb <= STU_EPB <= 64
      const int e = e0 + t;
      const uint32_t g = A.env_offset + (uint32_t)e;
      auto fld = [&](int f) { return A.F[(size_t)f * n + e]; };
      float* r = fr + t * FRAME;
      const float qw = fld(H12_F_QUAT), qx = fld(H12_F_QUAT + 1), qy = fld(H12_F_QUAT + 2), qz = fld(H12_F_QUAT + 3);
      float R2[3];
      gravity_row(qw, qx, qy, qz, R2);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        r[a] = corrupt(A, g, a, fld(H12_F_WANG + a), A.nz0, A.sc0);
        r[3 + a] = corrupt(A, g, 3 + a, -R2[a], A.nz1, A.sc1);
        r[6 + a] = corrupt(A, g, 6 + a, fld(H12_F_CMD + a), A.nz2, A.sc2);
      }
      const int pk = A.I[(size_t)H12_I_PACK * n + e];
      // reset by the step before the call; or, with a fill mask, what the caller says
      const bool fresh = A.fill_mask ? A.fill_mask[e] != 0 : ((pk >> 9) & 3) == 0;
      s_fill[t] = (A.prev == nullptr || fresh) ? 1 : 0;
    }
  } else {
    // item idx = row j (of the 36) x env el, el fastest: a thread's loads first (independent, all in flight), then the
    // LDS stores.  A ragged block's spare lanes load the block's last env; they do not store.
    constexpr int NT = STU_BLOCK - 64, ITEMS = NJ3 * STU_EPB, PASSES = ITEMS / NT;
    static_assert(ITEMS % NT == 0, "whole passes");
    float v[PASSES];
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
      const int idx = t - 64 + i * NT;
      const int j = idx / STU_EPB, el = idx & (STU_EPB - 1);
      v[i] = A.F[(size_t)(H12_F_Q + j) * n + e0 + (el < nb ? el : nb - 1)];
    }
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
      const int idx = t - 64 + i * NT;
      const int j = idx / STU_EPB, el = idx & (STU_EPB - 1), term = j / H12_NJ;
      if (el < nb) {
        const float x = term == 0 ? v[i] - q0_of(j) : v[i];
        const float nz = term == 0 ? A.nz3 : (term == 1 ? A.nz4 : A.nz5);
        const float sc = term == 0 ? A.sc3 : (term == 1 ? A.sc4 : A.sc5);
        fr[el * FRAME + COL_JOINT + j] = corrupt(A, A.env_offset + (uint32_t)(e0 + el), COL_JOINT + j, x, nz, sc);
      }
    }
  }
  __syncthreads();

  // ---- phase 2: the rows, a wave per row; a row's loads (up to COL_PASSES per lane) are issued before its LDS stores
  {
    const int wave = t >> 6, lane = t & 63;
    for (int el = wave; el < nb; el += STU_BLOCK / 64) {
      const bool fill = s_fill[el] != 0;
      const float* pr = fill ? rows : A.prev + (size_t)(e0 + el) * W;  // not read when the row fills (prev may be null)
      const float* f = fr + el * FRAME;
      float v[COL_PASSES];
#pragma unroll
      for (int p = 0; p < COL_PASSES; ++p) {
        const int c = lane + 64 * p;
        v[p] = 0.f;
        if (c < W) {
          const int code = s_tab[c];
          v[p] = (fill || (code >> 16)) ? f[code & 0xFF] : pr[c + ((code >> 8) & 0xFF)];
        }
      }
#pragma unroll
      for (int p = 0; p < COL_PASSES; ++p) {
        const int c = lane + 64 * p;
        if (c < W) rows[el * W + c] = v[p];
      }
    }
  }
  __syncthreads();

  // ---- phase 3: the block's span
  const int total = nb * W;
  float* dst = A.out + (size_t)e0 * W;
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(A.out) & 15) == 0) {  // e0 * W * 4 is a multiple of 16 for every block
    const int nv = total >> 2;
    for (int i = t; i < nv; i += STU_BLOCK)
      reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(rows)[i];
    done = nv << 2;
  }
  for (int i = done + t; i < total; i += STU_BLOCK) dst[i] = rows[i];
}

thread_local char g_err[256] = "";
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
bool fin(float x) {  // on the bit pattern: this file's device pass is compiled with -ffinite-math-only
  uint32_t u;
  memcpy(&u, &x, sizeof u);
  return (u & 0x7f800000u) != 0x7f800000u;
}

}  // namespace

extern "C" {

const char* h12student_last_error(void) { return g_err; }

int h12student_layout(int history, int32_t* width, int32_t table[H12STUDENT_NTERMS][3], int32_t* n_terms) {
  if (history < 1 || history > H12STUDENT_MAX_HISTORY)
    return fail(H12STUDENT_E_ARG, "history: %d (1 .. %d)", history, H12STUDENT_MAX_HISTORY);
  for (int t = 0; t < H12STUDENT_NTERMS; ++t)
    if (table) { table[t][0] = t; table[t][1] = TERM_OFF[t] * history; table[t][2] = TERM_WIDTH[t] * history; }
  if (width) *width = FRAME * history;
  if (n_terms) *n_terms = H12STUDENT_NTERMS;
  return H12STUDENT_OK;
}

int h12student_observe(const void* workspace, int n, const h12student_config* cfg, const float* prev, float* out,
                       int64_t step_index, void* stream) {
  if (!workspace) return fail(H12STUDENT_E_ARG, "workspace: null");
  if (reinterpret_cast<uintptr_t>(workspace) & 3) return fail(H12STUDENT_E_ARG, "workspace: not 4-byte aligned");
  if (n < 1) return fail(H12STUDENT_E_ARG, "n: %d (>= 1)", n);
  if ((long long)n * MAX_W > 0x7fffffffLL) return fail(H12STUDENT_E_ARG, "n: %d (too many envs)", n);
  if (!cfg) return fail(H12STUDENT_E_ARG, "cfg: null");
  if (cfg->history < 1 || cfg->history > H12STUDENT_MAX_HISTORY)
    return fail(H12STUDENT_E_ARG, "cfg.history: %d (1 .. %d)", cfg->history, H12STUDENT_MAX_HISTORY);
  for (int t = 0; t < H12STUDENT_NTERMS; ++t) {
    if (!fin(cfg->noise[t]) || !(cfg->noise[t] >= 0.f))
      return fail(H12STUDENT_E_ARG, "cfg.noise[%d]: not finite or negative", t);
    if (!fin(cfg->scale[t])) return fail(H12STUDENT_E_ARG, "cfg.scale[%d]: not finite", t);
  }
  if (!out) return fail(H12STUDENT_E_ARG, "out: null");
  if (reinterpret_cast<uintptr_t>(out) & 3) return fail(H12STUDENT_E_ARG, "out: not 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(prev) & 3) return fail(H12STUDENT_E_ARG, "prev: not 4-byte aligned");
  const int W = FRAME * cfg->history;
  if (prev) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(prev), b = reinterpret_cast<uintptr_t>(out);
    const uintptr_t bytes = (uintptr_t)n * W * sizeof(float);
    if (a < b + bytes && b < a + bytes) return fail(H12STUDENT_E_ARG, "out: overlaps prev");
  }

  StuArgs A;
  memset(&A, 0, sizeof A);
  A.F = static_cast<const float*>(workspace);
  A.I = reinterpret_cast<const int32_t*>(A.F + (size_t)H12_NF_FLOAT * n);
  A.n = n;
  A.prev = prev;
  A.fill_mask = cfg->fill_mask;
  A.out = out;
  A.H = cfg->history;
  A.W = W;
  A.seed_lo = cfg->seed_lo; A.seed_hi = cfg->seed_hi; A.env_offset = cfg->env_offset;
  A.step_lo = (uint32_t)step_index;
  A.step_hi = (uint32_t)((uint64_t)step_index >> 32);
  const bool on = cfg->enable_corruption != 0;
  float* nz[H12STUDENT_NTERMS] = {&A.nz0, &A.nz1, &A.nz2, &A.nz3, &A.nz4, &A.nz5};
  float* sc[H12STUDENT_NTERMS] = {&A.sc0, &A.sc1, &A.sc2, &A.sc3, &A.sc4, &A.sc5};
  for (int t = 0; t < H12STUDENT_NTERMS; ++t) {
    *nz[t] = on ? cfg->noise[t] : 0.f;
    *sc[t] = cfg->scale[t];
  }
  const int blocks = (n + STU_EPB - 1) / STU_EPB;
  const size_t lds = ((size_t)STU_EPB * W + STU_EPB * FRAME + STU_EPB + W) * sizeof(float);
  hipLaunchKernelGGL(student_obs_kernel, dim3(blocks), dim3(STU_BLOCK), lds, static_cast<hipStream_t>(stream), A);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(H12STUDENT_E_HIP, "launch: %s", hipGetErrorString(err));
  return H12STUDENT_OK;
}

}  // extern "C"
