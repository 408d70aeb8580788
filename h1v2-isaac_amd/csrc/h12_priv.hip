// h12_priv.hip: the privileged ("critic") observation rows (include/h12priv.h).  One launch per
// call, 256 threads per block; a block owns EPB consecutive envs -- 64 on the plane (W = 65), 16 with a heightfield
// (W = 252: the scan's heightfield reads are scattered, one cache line per lane, and bound by the rate at which one CU
// takes them, so the work is spread over four times as many blocks; measured in DESIGN.md section 7k):
//   wave 0        one lane per env: the base terms (COM velocity in the base frame, angular velocity, projected gravity,
//                 command), base height, contact flags / timers / forces, lags, friction, added mass
//   waves 1-3     the 36 joint rows (Q - Q0, QD, ACT), lanes across envs: contiguous segments of the field-major
//                 workspace (256 bytes per wave pass at 64 envs); a wave's loads are issued together, then stored
//   all waves     heightfield only: the 17 x 11 scan, SCAN_TPE = 16 threads per env, each with the env's pose in
//                 registers and 12 rays whose heightfield loads do not depend on one another -- the 187 dependent loads
//                 of a row are spread over threads (per (env, ray), as rough_obs_kernel's are)
//                 and a thread's are in flight together
// The block's rows are staged in LDS as they lie in the output ([env][W], no padding) and leave as ONE contiguous span
// of nb * W floats in 16-byte stores (EPB * W * 4 bytes per full block, a multiple of 16 for both layouts); the last
// (nb * W) % 4 floats of a ragged last block leave in scalar stores.
// h12priv_observe_terms (the rnd_state group) launches priv_terms_kernel: the same block body
// (priv_rows), whose rows then leave column run by column run into the compacted [n][W'] output.
// Device code is compiled with -ffinite-math-only and a diverged base can be non-finite: whatever becomes a heightfield
// index is taken from values whose bit patterns were checked first (sane_bits), and the indices are clamped once more
// with integer operations.  Everything else is arithmetic into fixed addresses.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/h12priv.h"
#include "h12_model_gen.h"

namespace {

constexpr int PRIV_BLOCK = 256;       // threads per block
constexpr int EPB_PLANE = 64;         // envs per block
constexpr int EPB_TERRAIN = 16;       // ... with the height scan
constexpr int SCAN_TPE = PRIV_BLOCK / EPB_TERRAIN;                  // scan threads per env
constexpr int SCAN_RPT = (H12_NSCAN + SCAN_TPE - 1) / SCAN_TPE;    // rays per thread
constexpr int NJ3 = 3 * H12_NJ;  // joint_pos, joint_vel, actions
constexpr int COL_JOINT = 12, COL_TAIL = 48;
static_assert(H12_F_QD == H12_F_Q + H12_NJ && H12_F_ACT == H12_F_QD + H12_NJ, "Q, QD, ACT are 36 consecutive fields");
static_assert(COL_TAIL + 17 == H12PRIV_W_PLANE, "row width");
static_assert((EPB_PLANE * H12PRIV_W_PLANE * sizeof(float)) % 16 == 0 && (EPB_TERRAIN * H12PRIV_W_TERRAIN * sizeof(float)) % 16 == 0,
              "a block's span starts on a 16-byte boundary");
// the right leg's default pose is the left leg's with the yaw / roll joints negated: those defaults are 0, so the
// per-leg table serves both legs
static_assert(h12m::Q0[0] == 0.f && h12m::Q0[2] == 0.f && h12m::Q0[5] == 0.f, "mirrored joints with a non-zero default");

struct PrivArgs {
  const float* F;
  const int32_t* I;
  int n;
  const float* ff;
  float* out;
  int W, terrain;
  const float* heights;
  int nx, ny;
  float inv_hs, x0, y0;
  float mus, mud;
  int env_mu, env_mass;
  float scan_off, scan_clip;
  float scale[H12PRIV_NTERMS];
  // h12priv_observe_terms only: the compacted row's width, whether the scan is among the terms, and the runs of
  // consecutive columns of the full row that make it up (adjacent terms merged)
  int Wout, scan_on, nseg;
  struct { int src, dst, w; } seg[H12PRIV_NTERMS];
};

// |x| <= 1e6 on the bit pattern: false for NaN, +-inf and magnitudes whose products below could overflow
__device__ __forceinline__ bool sane_bits(float x) { return (__float_as_uint(x) & 0x7fffffffu) <= 0x49742400u; }

__device__ __forceinline__ float q0_of(int k) {  // h12m::Q0[k % 6] without an indexed constant table
  const int j = k >= 6 ? k - 6 : k;
  return j == 1 ? h12m::Q0[1] : (j == 3 ? h12m::Q0[3] : (j == 4 ? h12m::Q0[4] : 0.f));
}

// h12env.hip's ground() restated: height of the triangle mesh at (x, y), flat border outside the grid.  x, y finite.
__device__ __forceinline__ float ground_at(const PrivArgs& A, float x, float y) {
  const float u = fminf(fmaxf((x - A.x0) * A.inv_hs, 0.f), (float)(A.nx - 1) - 1e-3f);
  const float v = fminf(fmaxf((y - A.y0) * A.inv_hs, 0.f), (float)(A.ny - 1) - 1e-3f);
  int ix = (int)u, iy = (int)v;
  const float fu = u - (float)ix, fv = v - (float)iy;
  ix = ix < 0 ? 0 : (ix > A.nx - 2 ? A.nx - 2 : ix);
  iy = iy < 0 ? 0 : (iy > A.ny - 2 ? A.ny - 2 : iy);
  const float* hp = A.heights + (size_t)ix * A.ny + iy;
  // triangle (00, 11, 01) above the diagonal, (00, 10, 11) below: the third vertex by a computed offset, so the three
  // loads are unconditional and those of a thread's rays can all be in flight (the same differences as ground())
  const bool up = fv >= fu;
  const float h00 = hp[0], h11 = hp[A.ny + 1], h2 = hp[up ? 1 : A.ny];
  const float d0 = h2 - h00, d1 = h11 - h2;
  const float a = up ? d1 : d0, b = up ? d0 : d1;
  return h00 + fu * a + fv * b;
}

// base position and yaw direction (cos, sin) of env e for the heightfield queries; an env whose base pose is not
// sane reads the heightfield at the world origin
__device__ __forceinline__ void scan_pose(const PrivArgs& A, int e, float* p) {
  float v[7];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    v[k] = A.F[(size_t)(H12_F_POS + k) * A.n + e];
    ok = ok && sane_bits(v[k]);
  }
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = 0.f;
  }
  const float w = v[3], x = v[4], y = v[5], z = v[6];
  const float F = w * w + x * x + y * y + z * z;
  p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = 1.f; p[4] = 0.f;
  if (F > 1e-12f) {
    const float t = 2.f / F;
    const float hx = 1.f - t * (y * y + z * z), hy = t * (x * y + w * z);  // R[0][0], R[1][0]
    const float s2 = hx * hx + hy * hy;
    if (s2 > 1e-20f) {
      const float hn = 1.f / sqrtf(s2);
      p[3] = hx * hn;
      p[4] = hy * hn;
    }
  }
}

// The block's work, shared by the two kernels below.  MASKED (h12priv_observe_terms): the rows are built in LDS by the
// same code, and only the columns of A.seg leave.
template <int PRIV_EPB, bool TERRAIN, bool MASKED>
__device__ __forceinline__ void priv_rows(const PrivArgs& A, float* rows /* LDS [PRIV_EPB][W] */) {
  const int W = A.W, n = A.n, t = threadIdx.x;
  const int e0 = blockIdx.x * PRIV_EPB;
  const int nb = n - e0 < PRIV_EPB ? n - e0 : PRIV_EPB;
  const float* S = A.scale;
  if (t < 64) {
    if (t < nb) {  // nb <= PRIV_EPB <= 64
      const int e = e0 + t;
      auto fld = [&](int f) { return A.F[(size_t)f * n + e]; };
      float* r = rows + t * W;
      const float qw = fld(H12_F_QUAT), qx = fld(H12_F_QUAT + 1), qy = fld(H12_F_QUAT + 2), qz = fld(H12_F_QUAT + 3);
      const float tq = 2.f / (qw * qw + qx * qx + qy * qy + qz * qz);
      float R[3][3];
      R[0][0] = 1.f - tq * (qy * qy + qz * qz); R[0][1] = tq * (qx * qy - qw * qz); R[0][2] = tq * (qx * qz + qw * qy);
      R[1][0] = tq * (qx * qy + qw * qz); R[1][1] = 1.f - tq * (qx * qx + qz * qz); R[1][2] = tq * (qy * qz - qw * qx);
      R[2][0] = tq * (qx * qz - qw * qy); R[2][1] = tq * (qy * qz + qw * qx); R[2][2] = 1.f - tq * (qx * qx + qy * qy);
      const float wb[3] = {fld(H12_F_WANG), fld(H12_F_WANG + 1), fld(H12_F_WANG + 2)};
      // base_com_vel / obs_frame of h12env.hip: v_origin + (R w) x (R c), back into the base frame
      const float c[3] = {h12m::ROOT_COM[0], h12m::ROOT_COM[1], h12m::ROOT_COM[2]};
      float ww[3], cw[3], vc[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        ww[a] = R[a][0] * wb[0] + R[a][1] * wb[1] + R[a][2] * wb[2];
        cw[a] = R[a][0] * c[0] + R[a][1] * c[1] + R[a][2] * c[2];
      }
      vc[0] = fld(H12_F_VLIN) + (ww[1] * cw[2] - ww[2] * cw[1]);
      vc[1] = fld(H12_F_VLIN + 1) + (ww[2] * cw[0] - ww[0] * cw[2]);
      vc[2] = fld(H12_F_VLIN + 2) + (ww[0] * cw[1] - ww[1] * cw[0]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        r[a] = (R[0][a] * vc[0] + R[1][a] * vc[1] + R[2][a] * vc[2]) * S[H12PRIV_T_BASE_LIN_VEL];
        r[3 + a] = wb[a] * S[H12PRIV_T_BASE_ANG_VEL];
        r[6 + a] = -R[2][a] * S[H12PRIV_T_PROJECTED_GRAVITY];
        r[9 + a] = fld(H12_F_CMD + a) * S[H12PRIV_T_VELOCITY_COMMANDS];
      }
      float* q = r + (TERRAIN ? COL_TAIL + H12_NSCAN : COL_TAIL);
      float bh = fld(H12_F_POS + 2);
      if (TERRAIN) {
        float p[5];
        scan_pose(A, e, p);
        bh -= ground_at(A, p[0], p[1]);
      }
      q[0] = bh * S[H12PRIV_T_BASE_HEIGHT];
      const int pk = A.I[(size_t)H12_I_PACK * n + e];
      const bool fresh = ((pk >> 9) & 3) == 0;  // reset by the step that wrote foot_force (ContactSensor.reset)
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        q[1 + f] = (((pk >> (13 + 4 * f)) & 0xF) ? 1.f : 0.f) * S[H12PRIV_T_FEET_CONTACT];
        q[3 + f] = fld(H12_F_AIR + f) * S[H12PRIV_T_FEET_AIR_TIME];
        q[5 + f] = fld(H12_F_CONTACT + f) * S[H12PRIV_T_FEET_CONTACT_TIME];
        const float force = (A.ff && !fresh) ? A.ff[(size_t)2 * e + f] : 0.f;
        q[7 + f] = force * S[H12PRIV_T_FEET_FORCE];
      }
#pragma unroll
      for (int g = 0; g < 3; ++g) q[9 + g] = (float)((pk >> (3 * g)) & 7) * S[H12PRIV_T_ACTUATOR_LAG];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float mu = A.env_mu ? fld(H12_F_MU + k) : ((k & 1) ? A.mud : A.mus);
        q[12 + k] = mu * S[H12PRIV_T_SOLE_FRICTION];
      }
      q[16] = (A.env_mass ? fld(H12_F_DMASS) : 0.f) * S[H12PRIV_T_ADDED_MASS];
    }
  } else {
    // item idx = row j (of the 36) x env el, el fastest: a thread's loads first (independent, all in flight), then the
    // LDS stores.  A ragged block's spare lanes load the block's last env, a spare pass the last item; neither stores.
    constexpr int NT = PRIV_BLOCK - 64, ITEMS = NJ3 * PRIV_EPB, PASSES = (ITEMS + NT - 1) / NT;
    const float s0 = S[H12PRIV_T_JOINT_POS], s1 = S[H12PRIV_T_JOINT_VEL], s2 = S[H12PRIV_T_ACTIONS];
    float v[PASSES];
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
      const int idx = t - 64 + i * NT, idc = idx < ITEMS ? idx : ITEMS - 1;
      const int j = idc / PRIV_EPB, el = idc & (PRIV_EPB - 1);
      v[i] = A.F[(size_t)(H12_F_Q + j) * n + e0 + (el < nb ? el : nb - 1)];
    }
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
      const int idx = t - 64 + i * NT;
      const int j = idx / PRIV_EPB, el = idx & (PRIV_EPB - 1), term = j / H12_NJ;
      if (idx < ITEMS && el < nb)
        rows[el * W + COL_JOINT + j] = (term == 0 ? v[i] - q0_of(j) : v[i]) * (term == 0 ? s0 : (term == 1 ? s1 : s2));
    }
  }
  if (TERRAIN && (!MASKED || A.scan_on)) {
    static_assert(!TERRAIN || PRIV_BLOCK == PRIV_EPB * SCAN_TPE, "SCAN_TPE threads per env");
    static_assert((PRIV_EPB & (PRIV_EPB - 1)) == 0 && PRIV_EPB <= 64, "envs per block");
    const int el = t / SCAN_TPE, r0 = t - el * SCAN_TPE;
    if (el < nb) {
      float p[5];
      scan_pose(A, e0 + el, p);
      float* dstrow = rows + el * W + COL_TAIL;
#pragma unroll
      for (int k = 0; k < SCAN_RPT; ++k) {
        const int ray = r0 + k * SCAN_TPE;
        const int rc = ray < H12_NSCAN ? ray : H12_NSCAN - 1;  // the last pass is ragged: computed, not stored
        const int iy = rc / H12_SCAN_NX, ix = rc - iy * H12_SCAN_NX;
        const float xl = H12PRIV_SCAN_RES * (float)(ix - (H12_SCAN_NX - 1) / 2);
        const float yl = H12PRIV_SCAN_RES * (float)(iy - (H12_SCAN_NY - 1) / 2);
        const float hz = ground_at(A, p[0] + p[3] * xl - p[4] * yl, p[1] + p[4] * xl + p[3] * yl);
        const float v = fminf(fmaxf(p[2] - hz - A.scan_off, -A.scan_clip), A.scan_clip);
        if (ray < H12_NSCAN) dstrow[ray] = v * S[H12PRIV_T_HEIGHT_SCAN];
      }
    }
  }
  __syncthreads();
  if (MASKED) {  // run by run: item i of a run is (env i / w, column i % w); e0 + el < n and dst + c < Wout
    for (int k = 0; k < A.nseg; ++k) {
      const int w = A.seg[k].w, src = A.seg[k].src, dstc = A.seg[k].dst;
      for (int i = t; i < nb * w; i += PRIV_BLOCK) {
        const int el = i / w, c = i - el * w;
        A.out[(size_t)(e0 + el) * A.Wout + dstc + c] = rows[el * W + src + c];
      }
    }
    return;
  }
  const int total = nb * W;
  float* dst = A.out + (size_t)e0 * W;
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(A.out) & 15) == 0) {  // e0 * W * 4 is a multiple of 16 for every block
    const int nv = total >> 2;
    for (int i = t; i < nv; i += PRIV_BLOCK)
      reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(rows)[i];
    done = nv << 2;
  }
  for (int i = done + t; i < total; i += PRIV_BLOCK) dst[i] = rows[i];
}

template <int PRIV_EPB, bool TERRAIN>
__global__ __launch_bounds__(PRIV_BLOCK) void priv_obs_kernel(PrivArgs A) {
  extern __shared__ __attribute__((aligned(16))) float rows[];  // [PRIV_EPB][W]
  priv_rows<PRIV_EPB, TERRAIN, false>(A, rows);
}

template <int PRIV_EPB, bool TERRAIN>
__global__ __launch_bounds__(PRIV_BLOCK) void priv_terms_kernel(PrivArgs A) {
  extern __shared__ __attribute__((aligned(16))) float rows[];  // [PRIV_EPB][W]
  priv_rows<PRIV_EPB, TERRAIN, true>(A, rows);
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

constexpr int TERM_WIDTH[H12PRIV_NTERMS] = {3, 3, 3, 3, H12_NJ, H12_NJ, H12_NJ, H12_NSCAN, 1, 2, 2, 2, 2, 3, 4, 1};

}  // namespace

extern "C" {

const char* h12priv_last_error(void) { return g_err; }

int h12priv_layout(int terrain, int32_t* width, int32_t table[H12PRIV_NTERMS][3], int32_t* n_terms) {
  if (terrain != 0 && terrain != 1) return fail(H12PRIV_E_ARG, "terrain: %d (0 | 1)", terrain);
  int off = 0, rows = 0;
  for (int t = 0; t < H12PRIV_NTERMS; ++t) {
    if (t == H12PRIV_T_HEIGHT_SCAN && !terrain) continue;
    if (table) { table[rows][0] = t; table[rows][1] = off; table[rows][2] = TERM_WIDTH[t]; }
    off += TERM_WIDTH[t];
    ++rows;
  }
  if (width) *width = off;
  if (n_terms) *n_terms = rows;
  return H12PRIV_OK;
}

}  // extern "C"

namespace {

// the argument checks of both launches and the kernel arguments they share
int fill_args(const void* workspace, int n, const h12priv_config* cfg, const float* foot_force, float* out,
              PrivArgs& A) {
  if (!workspace) return fail(H12PRIV_E_ARG, "workspace: null");
  if (reinterpret_cast<uintptr_t>(workspace) & 3) return fail(H12PRIV_E_ARG, "workspace: not 4-byte aligned");
  if (n < 1) return fail(H12PRIV_E_ARG, "n: %d (>= 1)", n);
  if ((long long)n * H12PRIV_W_TERRAIN > 0x7fffffffLL) return fail(H12PRIV_E_ARG, "n: %d (too many envs)", n);
  if (!cfg) return fail(H12PRIV_E_ARG, "cfg: null");
  if (!out) return fail(H12PRIV_E_ARG, "out: null");
  if (reinterpret_cast<uintptr_t>(out) & 3) return fail(H12PRIV_E_ARG, "out: not 4-byte aligned");
  if (cfg->terrain != 0 && cfg->terrain != 1) return fail(H12PRIV_E_ARG, "cfg.terrain: %d (0 | 1)", cfg->terrain);
  if (cfg->terrain) {
    if (!cfg->heights) return fail(H12PRIV_E_ARG, "cfg.heights: null with cfg.terrain set");
    if (cfg->nx < 2 || cfg->ny < 2) return fail(H12PRIV_E_ARG, "cfg.nx, ny: %d x %d (>= 2 each)", cfg->nx, cfg->ny);
    if ((long long)cfg->nx * cfg->ny > 0x7fffffffLL) return fail(H12PRIV_E_ARG, "cfg.nx, ny: %d x %d", cfg->nx, cfg->ny);
    if (!(cfg->hscale >= 1e-6f && cfg->hscale <= 1e6f)) return fail(H12PRIV_E_ARG, "cfg.hscale: must be in [1e-6, 1e6]");
    if (!(cfg->x0 >= -1e6f && cfg->x0 <= 1e6f && cfg->y0 >= -1e6f && cfg->y0 <= 1e6f))
      return fail(H12PRIV_E_ARG, "cfg.x0, y0: must be in [-1e6, 1e6]");
    if (!(cfg->scan_clip >= 0.f && fin(cfg->scan_clip)) || !fin(cfg->scan_offset))
      return fail(H12PRIV_E_ARG, "cfg.scan_offset / scan_clip: not finite or negative clip");
  }
  if (!fin(cfg->mu_static) || !fin(cfg->mu_dynamic)) return fail(H12PRIV_E_ARG, "cfg.mu_static / mu_dynamic: not finite");
  for (int t = 0; t < H12PRIV_NTERMS; ++t)
    if (!fin(cfg->scale[t])) return fail(H12PRIV_E_ARG, "cfg.scale[%d]: not finite", t);

  memset(&A, 0, sizeof A);
  A.F = static_cast<const float*>(workspace);
  A.I = reinterpret_cast<const int32_t*>(A.F + (size_t)H12_NF_FLOAT * n);
  A.n = n;
  A.ff = foot_force;
  A.out = out;
  A.terrain = cfg->terrain;
  A.W = cfg->terrain ? H12PRIV_W_TERRAIN : H12PRIV_W_PLANE;
  if (cfg->terrain) {
    A.heights = cfg->heights; A.nx = cfg->nx; A.ny = cfg->ny;
    A.inv_hs = 1.f / cfg->hscale; A.x0 = cfg->x0; A.y0 = cfg->y0;
    A.scan_off = cfg->scan_offset; A.scan_clip = cfg->scan_clip;
  }
  A.mus = cfg->mu_static; A.mud = cfg->mu_dynamic;
  A.env_mu = cfg->per_env_friction != 0; A.env_mass = cfg->per_env_mass != 0;
  for (int t = 0; t < H12PRIV_NTERMS; ++t) A.scale[t] = cfg->scale[t];
  return H12PRIV_OK;
}

// the runs of a term mask: H12PRIV_E_ARG for a mask that names no term, a term past the table, or height_scan
// without a heightfield
int mask_runs(int terrain, uint32_t mask, PrivArgs* A, int32_t* width, int32_t table[H12PRIV_NTERMS][3],
              int32_t* n_terms) {
  if (mask == 0) return fail(H12PRIV_E_ARG, "term_mask: 0 (names no term)");
  if (mask >> H12PRIV_NTERMS)
    return fail(H12PRIV_E_ARG, "term_mask: 0x%x names a term past the table (%d terms)", mask, H12PRIV_NTERMS);
  if (((mask >> H12PRIV_T_HEIGHT_SCAN) & 1u) && !terrain)
    return fail(H12PRIV_E_ARG, "term_mask: height_scan on a plane task (no heightfield)");
  int src = 0, dst = 0, rows = 0, nseg = 0;
  for (int t = 0; t < H12PRIV_NTERMS; ++t) {
    if (t == H12PRIV_T_HEIGHT_SCAN && !terrain) continue;
    const int w = TERM_WIDTH[t];
    if ((mask >> t) & 1u) {
      if (table) { table[rows][0] = t; table[rows][1] = dst; table[rows][2] = w; }
      if (A) {
        if (nseg && A->seg[nseg - 1].src + A->seg[nseg - 1].w == src) {
          A->seg[nseg - 1].w += w;
        } else {
          A->seg[nseg].src = src; A->seg[nseg].dst = dst; A->seg[nseg].w = w;
          ++nseg;
        }
      }
      dst += w;
      ++rows;
    }
    src += w;
  }
  if (A) { A->nseg = nseg; A->Wout = dst; A->scan_on = (mask >> H12PRIV_T_HEIGHT_SCAN) & 1u; }
  if (width) *width = dst;
  if (n_terms) *n_terms = rows;
  return H12PRIV_OK;
}

}  // namespace

extern "C" {

int h12priv_layout_terms(int terrain, uint32_t term_mask, int32_t* width, int32_t table[H12PRIV_NTERMS][3],
                         int32_t* n_terms) {
  if (terrain != 0 && terrain != 1) return fail(H12PRIV_E_ARG, "terrain: %d (0 | 1)", terrain);
  return mask_runs(terrain, term_mask, nullptr, width, table, n_terms);
}

int h12priv_observe(const void* workspace, int n, const h12priv_config* cfg, const float* foot_force, float* out,
                    void* stream) {
  PrivArgs A;
  const int rc = fill_args(workspace, n, cfg, foot_force, out, A);
  if (rc != H12PRIV_OK) return rc;
  const int epb = A.terrain ? EPB_TERRAIN : EPB_PLANE;
  const int blocks = (n + epb - 1) / epb;
  const size_t lds = (size_t)epb * A.W * sizeof(float);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A.terrain)
    hipLaunchKernelGGL((priv_obs_kernel<EPB_TERRAIN, true>), dim3(blocks), dim3(PRIV_BLOCK), lds, s, A);
  else
    hipLaunchKernelGGL((priv_obs_kernel<EPB_PLANE, false>), dim3(blocks), dim3(PRIV_BLOCK), lds, s, A);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(H12PRIV_E_HIP, "launch: %s", hipGetErrorString(err));
  return H12PRIV_OK;
}

int h12priv_observe_terms(const void* workspace, int n, const h12priv_config* cfg, const float* foot_force,
                          uint32_t term_mask, float* out, void* stream) {
  PrivArgs A;
  int rc = fill_args(workspace, n, cfg, foot_force, out, A);
  if (rc == H12PRIV_OK) rc = mask_runs(cfg->terrain, term_mask, &A, nullptr, nullptr, nullptr);
  if (rc != H12PRIV_OK) return rc;
  const int epb = A.terrain ? EPB_TERRAIN : EPB_PLANE;
  const int blocks = (n + epb - 1) / epb;
  const size_t lds = (size_t)epb * A.W * sizeof(float);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A.terrain)
    hipLaunchKernelGGL((priv_terms_kernel<EPB_TERRAIN, true>), dim3(blocks), dim3(PRIV_BLOCK), lds, s, A);
  else
    hipLaunchKernelGGL((priv_terms_kernel<EPB_PLANE, false>), dim3(blocks), dim3(PRIV_BLOCK), lds, s, A);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(H12PRIV_E_HIP, "launch: %s", hipGetErrorString(err));
  return H12PRIV_OK;
}

}  // extern "C"
