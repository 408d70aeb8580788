// h12_render.hip: ray-cast renderer of the kinematic skeleton over the task's ground (include/h12render.h; the image
// is defined in DESIGN.md section 7i).  Two launches per call:
//   render_setup_kernel  one block per view: forward kinematics from POS / QUAT / Q, the primitive table and the
//                        overlay rows in the view's env frame, the camera basis, each row's screen-space bound
//   render_kernel        one 16 x 16 pixel tile per block, one thread per pixel: rows staged in LDS, a 64-bit mask of
//                        the rows whose bound meets the tile, analytic intersections, ground, shadow ray, shading
// Device code is compiled with -ffinite-math-only: non-finite inputs are detected on their bit patterns and never
// enter arithmetic, and +inf is stored as a bit pattern.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/h12render.h"

namespace {

constexpr int TILE = 16;                  // pixels per tile edge; 256 threads per block
constexpr int HDR_WORDS = 32;             // per-view header
constexpr int PRIM_WORDS = 24;            // per-row record
constexpr int VIEW_WORDS = HDR_WORDS + H12RENDER_MAX_PRIMS * PRIM_WORDS;
// header words
enum { H_EYE = 0, H_F = 3, H_R = 6, H_U = 9, H_NTOT = 12, H_CFX = 13, H_CFY = 14, H_CPAR = 15, H_ORG = 16 };
// row words
enum { P_TYPE = 0, P_A = 1, P_D = 4, P_RAD = 7, P_RGB = 8, P_AX = 11, P_BB = 20 };

// packed table (host -> device, h12render_pack_table)
struct Table {
  int32_t n_prims;
  int32_t parent[H12_NJ];
  int32_t axis[H12_NJ];
  float joint_pos[H12_NJ][3];
  float foot_pts[H12_NFOOT_PTS][3];
  float root_height;
  int32_t pad[2];
  h12render_prim rows[1];  // n_prims rows
};

// display constants of the overlays and the background
constexpr float CONTACT_RADIUS = 0.02f;
constexpr float ARROW_RADIUS = 0.012f, ARROW_GAIN = 0.5f, ARROW_Z = 0.55f, ARROW_DZ = 0.05f, ARROW_MIN = 1e-3f;
constexpr float COL_CONTACT[3] = {1.0f, 0.15f, 0.1f}, COL_CMD[3] = {0.1f, 0.8f, 0.2f}, COL_VEL[3] = {0.1f, 0.3f, 1.0f};
constexpr float COL_CHK0[3] = {0.55f, 0.55f, 0.55f}, COL_CHK1[3] = {0.35f, 0.35f, 0.35f};
constexpr float COL_FAR[3] = {0.45f, 0.45f, 0.45f};
constexpr float COL_HORIZON[3] = {0.80f, 0.86f, 0.93f}, COL_ZENITH[3] = {0.30f, 0.50f, 0.85f};
constexpr float AMBIENT = 0.35f, DIFFUSE = 0.65f;
constexpr float BIG = 3.0e38f;

struct RenderArgs {
  const float* F;
  const int32_t* I;
  int n;
  const int32_t* env_ids;
  int n_views;
  const float* view_origins;
  const float* heights;
  int nx, ny;
  float inv_hs, x0, y0;
  const Table* table;
  int n_prims, overlays, cull;
  float* scratch;
  uint8_t* rgb;
  int32_t* id;
  float* depth;
  int W, H, origin_type;
  float eye[3], lookat[3], tan_half, sun[3], far;
  int n_march;
};

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// conservative pixel bound of the sphere (c, R) given in camera coordinates (x right, y up, z forward)
__device__ void screen_bound(float xc, float yc, float zc, float R, float tx, float ty, int W, int H, int* bb) {
  bb[0] = 0; bb[1] = W - 1; bb[2] = 0; bb[3] = H - 1;
  if (!(zc > 1.01f * R + 1e-3f)) return;  // touches the camera plane: the whole frame
  const float den = zc * zc - R * R;
  const float sx = R * sqrtf(fmaxf(xc * xc + den, 0.f)), sy = R * sqrtf(fmaxf(yc * yc + den, 0.f));
  const float xlo = (xc * zc - sx) / den, xhi = (xc * zc + sx) / den;
  const float ylo = (yc * zc - sy) / den, yhi = (yc * zc + sy) / den;
  const float lim = 1.0e6f;
  const float j0 = fminf(fmaxf((xlo / tx + 1.f) * 0.5f * (float)W - 0.5f, -lim), lim);
  const float j1 = fminf(fmaxf((xhi / tx + 1.f) * 0.5f * (float)W - 0.5f, -lim), lim);
  const float i0 = fminf(fmaxf((-yhi / ty + 1.f) * 0.5f * (float)H - 0.5f, -lim), lim);
  const float i1 = fminf(fmaxf((-ylo / ty + 1.f) * 0.5f * (float)H - 0.5f, -lim), lim);
  bb[0] = (int)floorf(j0) - 1; bb[1] = (int)ceilf(j1) + 1; bb[2] = (int)floorf(i0) - 1; bb[3] = (int)ceilf(i1) + 1;
}

__global__ __launch_bounds__(64) void render_setup_kernel(RenderArgs A) {
  __shared__ float sR[H12RENDER_NBODY][9];
  __shared__ float sp[H12RENDER_NBODY][3];
  __shared__ float sh[HDR_WORDS];
  __shared__ int s_valid;
  const int v = blockIdx.x, t = threadIdx.x;
  const int n = A.n;
  int e = A.env_ids[v];
  e = e < 0 ? 0 : (e >= n ? n - 1 : e);
  const Table* T = A.table;
  // the validated row count bounds what the table itself says, so the view's records always fit the scratch area
  const int np = T->n_prims < 0 ? 0 : (T->n_prims > A.n_prims ? A.n_prims : T->n_prims);
  const int ntot = A.overlays ? np + H12RENDER_NOVERLAY : np;
  static_assert(H12RENDER_MAX_PRIMS == 64, "one setup thread and one mask bit per row");
  float* out = A.scratch + (size_t)v * VIEW_WORDS;
  auto fld = [&](int f) { return A.F[(size_t)f * n + e]; };
  if (t == 0) {
    // non-finite state: background only (no rows), the base taken at its initial height for the camera
    bool ok = true;
    for (int k = 0; k < 7; ++k) ok = ok && finite_bits(fld(H12_F_POS + k));
    for (int k = 0; k < H12_NJ; ++k) ok = ok && finite_bits(fld(H12_F_Q + k));
    if (A.overlays) {
      for (int k = 0; k < 3; ++k) ok = ok && finite_bits(fld(H12_F_VLIN + k));
      for (int k = 0; k < 2; ++k) ok = ok && finite_bits(fld(H12_F_CMD + k));
    }
    float org[3] = {0.f, 0.f, 0.f};
    if (A.heights) {
      bool oko = true;
      for (int k = 0; k < 3; ++k) oko = oko && finite_bits(fld(H12_F_ORIGIN + k));
      if (oko) for (int k = 0; k < 3; ++k) org[k] = fld(H12_F_ORIGIN + k);
      else ok = false;
    } else if (A.view_origins) {
      for (int k = 0; k < 3; ++k) org[k] = A.view_origins[3 * v + k];
    }
    float qw = 1.f, qx = 0.f, qy = 0.f, qz = 0.f;
    float pb[3] = {0.f, 0.f, T->root_height};
    if (ok) {
      qw = fld(H12_F_QUAT); qx = fld(H12_F_QUAT + 1); qy = fld(H12_F_QUAT + 2); qz = fld(H12_F_QUAT + 3);
      const float nn = qw * qw + qx * qx + qy * qy + qz * qz;
      if (!(nn > 1e-30f) || !finite_bits(nn)) { ok = false; qw = 1.f; qx = qy = qz = 0.f; }
      else { const float inv = 1.f / sqrtf(nn); qw *= inv; qx *= inv; qy *= inv; qz *= inv; }
    }
    if (ok) {
      // the view's env frame: env-local on the plane, world minus the env origin on a heightfield
      for (int k = 0; k < 3; ++k) pb[k] = A.heights ? fld(H12_F_POS + k) - org[k] : fld(H12_F_POS + k);
      for (int k = 0; k < 3; ++k) ok = ok && finite_bits(pb[k]);
      if (!ok) { pb[0] = pb[1] = 0.f; pb[2] = T->root_height; qw = 1.f; qx = qy = qz = 0.f; }
    }
    s_valid = ok ? 1 : 0;
    float* R0 = sR[0];
    R0[0] = 1 - 2 * (qy * qy + qz * qz); R0[1] = 2 * (qx * qy - qw * qz); R0[2] = 2 * (qx * qz + qw * qy);
    R0[3] = 2 * (qx * qy + qw * qz); R0[4] = 1 - 2 * (qx * qx + qz * qz); R0[5] = 2 * (qy * qz - qw * qx);
    R0[6] = 2 * (qx * qz - qw * qy); R0[7] = 2 * (qy * qz + qw * qx); R0[8] = 1 - 2 * (qx * qx + qy * qy);
    for (int k = 0; k < 3; ++k) sp[0][k] = pb[k];
    for (int j = 0; j < H12_NJ; ++j) {
      int par = T->parent[j] + 1;
      par = par < 0 ? 0 : (par > j ? j : par);  // a parent precedes its child
      const float q = ok ? fld(H12_F_Q + j) : 0.f;
      const float c = cosf(q), s = sinf(q);
      // R_b = R_p * Rot(axis, q): the joint mixes the two columns after its axis (cyclic), the axis column stays
      const int ax = T->axis[j];
      const int k0 = ax == 0 ? 0 : (ax == 1 ? 1 : 2);
      const int ku = ax == 0 ? 1 : (ax == 1 ? 2 : 0), kw = ax == 0 ? 2 : (ax == 1 ? 0 : 1);
      const float* Rp = sR[par];
      float* Rb = sR[j + 1];
      for (int a = 0; a < 3; ++a) {
        const float pu = Rp[3 * a + ku], pw = Rp[3 * a + kw];
        Rb[3 * a + k0] = Rp[3 * a + k0];
        Rb[3 * a + ku] = c * pu + s * pw;
        Rb[3 * a + kw] = c * pw - s * pu;
      }
      for (int a = 0; a < 3; ++a)
        sp[j + 1][a] = sp[par][a] + Rp[3 * a] * T->joint_pos[j][0] + Rp[3 * a + 1] * T->joint_pos[j][1] +
                       Rp[3 * a + 2] * T->joint_pos[j][2];
    }
    // camera
    float eye[3], la[3], f[3], r[3], u[3];
    for (int k = 0; k < 3; ++k) {
      const float base = A.origin_type == H12RENDER_ORIGIN_ASSET_ROOT ? pb[k] : 0.f;
      eye[k] = base + A.eye[k];
      la[k] = base + A.lookat[k];
    }
    for (int k = 0; k < 3; ++k) f[k] = A.lookat[k] - A.eye[k];  // the offset form: independent of the base
    float inv = 1.f / sqrtf(dot3(f, f));
    for (int k = 0; k < 3; ++k) f[k] *= inv;
    r[0] = f[1]; r[1] = -f[0]; r[2] = 0.f;  // f x z
    inv = 1.f / sqrtf(r[0] * r[0] + r[1] * r[1]);
    r[0] *= inv; r[1] *= inv;
    u[0] = r[1] * f[2] - r[2] * f[1]; u[1] = r[2] * f[0] - r[0] * f[2]; u[2] = r[0] * f[1] - r[1] * f[0];
    (void)la;
    for (int k = 0; k < 3; ++k) { sh[H_EYE + k] = eye[k]; sh[H_F + k] = f[k]; sh[H_R + k] = r[k]; sh[H_U + k] = u[k]; }
    sh[H_NTOT] = __int_as_float(ok ? ntot : 0);
    // checker phase of the env origin: the cell index of the origin is split off so that the per-pixel
    // coordinate stays env-local
    const float cux = org[0] / H12RENDER_CHECKER, cuy = org[1] / H12RENDER_CHECKER;
    const float fx0 = floorf(cux), fy0 = floorf(cuy);
    sh[H_CFX] = cux - fx0; sh[H_CFY] = cuy - fy0;
    const float lim = 1.0e9f;
    sh[H_CPAR] = __int_as_float((((int)fminf(fmaxf(fx0, -lim), lim)) + ((int)fminf(fmaxf(fy0, -lim), lim))) & 1);
    for (int k = 0; k < 3; ++k) sh[H_ORG + k] = org[k];
    for (int k = H_ORG + 3; k < HDR_WORDS; ++k) sh[k] = 0.f;
  }
  __syncthreads();
  if (t < HDR_WORDS / 2) { out[2 * t] = sh[2 * t]; out[2 * t + 1] = sh[2 * t + 1]; }
  const bool ok = s_valid != 0;
  float rec[PRIM_WORDS];
  for (int k = 0; k < PRIM_WORDS; ++k) rec[k] = 0.f;
  int type = 0;
  if (ok && t < np) {
    const h12render_prim& pr = T->rows[t];
    int b = pr.body < 0 ? 0 : (pr.body >= H12RENDER_NBODY ? H12RENDER_NBODY - 1 : pr.body);
    const float* R = sR[b];
    float w0[3];
    for (int a = 0; a < 3; ++a) w0[a] = sp[b][a] + R[3 * a] * pr.p0[0] + R[3 * a + 1] * pr.p0[1] + R[3 * a + 2] * pr.p0[2];
    type = pr.type;
    for (int a = 0; a < 3; ++a) { rec[P_A + a] = w0[a]; rec[P_RGB + a] = pr.rgb[a]; }
    if (type == H12RENDER_CAPSULE) {
      for (int a = 0; a < 3; ++a) {
        const float dl = R[3 * a] * (pr.p1[0] - pr.p0[0]) + R[3 * a + 1] * (pr.p1[1] - pr.p0[1]) + R[3 * a + 2] * (pr.p1[2] - pr.p0[2]);
        rec[P_D + a] = dl;
      }
      rec[P_RAD] = pr.radius;
    } else {
      for (int a = 0; a < 3; ++a) rec[P_D + a] = pr.p1[a];
      for (int k = 0; k < 9; ++k) rec[P_AX + k] = R[k];
    }
  } else if (ok && t < ntot) {
    const int o = t - np;
    if (o < 8) {  // sole contact spheres: foot o / 4, point o % 4
      const int pk = A.I[(size_t)H12_I_PACK * n + e];
      if ((pk >> (13 + o)) & 1) {
        const int b = 6 * (o / 4) + 6;
        const float* R = sR[b];
        const float* pl = T->foot_pts[o % 4];
        type = H12RENDER_CAPSULE;
        for (int a = 0; a < 3; ++a) {
          rec[P_A + a] = sp[b][a] + R[3 * a] * pl[0] + R[3 * a + 1] * pl[1] + R[3 * a + 2] * pl[2];
          rec[P_RGB + a] = COL_CONTACT[a];
        }
        rec[P_RAD] = CONTACT_RADIUS;
      }
    } else {  // velocity arrows: commanded (o == 8), actual (o == 9), both in the base's yaw frame
      const float* R = sR[0];
      float hx = R[0], hy = R[3];
      const float hn = sqrtf(hx * hx + hy * hy);
      float vx, vy;
      if (o == 8) { vx = fld(H12_F_CMD); vy = fld(H12_F_CMD + 1); }
      else {
        const float wv[3] = {fld(H12_F_VLIN), fld(H12_F_VLIN + 1), fld(H12_F_VLIN + 2)};
        vx = R[0] * wv[0] + R[3] * wv[1] + R[6] * wv[2];
        vy = R[1] * wv[0] + R[4] * wv[1] + R[7] * wv[2];
      }
      const float sp2 = sqrtf(vx * vx + vy * vy);
      if (hn > 1e-6f && sp2 > ARROW_MIN) {
        hx /= hn; hy /= hn;
        type = H12RENDER_CAPSULE;
        rec[P_A] = sp[0][0]; rec[P_A + 1] = sp[0][1]; rec[P_A + 2] = sp[0][2] + ARROW_Z + (o == 9 ? ARROW_DZ : 0.f);
        rec[P_D] = ARROW_GAIN * (vx * hx - vy * hy); rec[P_D + 1] = ARROW_GAIN * (vx * hy + vy * hx); rec[P_D + 2] = 0.f;
        rec[P_RAD] = ARROW_RADIUS;
        for (int a = 0; a < 3; ++a) rec[P_RGB + a] = o == 8 ? COL_CMD[a] : COL_VEL[a];
      }
    }
  }
  if (type != H12RENDER_CAPSULE && type != H12RENDER_BOX) type = 0;
  rec[P_TYPE] = __int_as_float(type);
  int bb[4] = {0, -1, 0, -1};
  if (type) {
    float c[3], Rb;
    if (type == H12RENDER_CAPSULE) {
      for (int a = 0; a < 3; ++a) c[a] = rec[P_A + a] + 0.5f * rec[P_D + a];
      Rb = 0.5f * sqrtf(dot3(&rec[P_D], &rec[P_D])) + rec[P_RAD];
    } else {
      for (int a = 0; a < 3; ++a) c[a] = rec[P_A + a];
      Rb = sqrtf(dot3(&rec[P_D], &rec[P_D]));
    }
    float d[3];
    for (int a = 0; a < 3; ++a) d[a] = c[a] - sh[H_EYE + a];
    const float ty = A.tan_half, tx = A.tan_half * (float)A.W / (float)A.H;
    screen_bound(dot3(d, &sh[H_R]), dot3(d, &sh[H_U]), dot3(d, &sh[H_F]), Rb, tx, ty, A.W, A.H, bb);
  }
  for (int k = 0; k < 4; ++k) rec[P_BB + k] = __int_as_float(bb[k]);
  float4* o4 = reinterpret_cast<float4*>(out + HDR_WORDS + t * PRIM_WORDS);
  for (int k = 0; k < PRIM_WORDS / 4; ++k) o4[k] = make_float4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
}

// entry distance of the ray (o, v), |v| = 1, into row p (LDS); BIG when it misses or the entry is not ahead.
// nrm: the outward normal at the entry.
__device__ __forceinline__ float hit_prim(const float* p, const float* o, const float* v, float* nrm, bool want_n) {
  const int type = __float_as_int(p[P_TYPE]);
  if (type == H12RENDER_CAPSULE) {
    const float* ba = p + P_D;
    const float r = p[P_RAD];
    const float oa[3] = {o[0] - p[P_A], o[1] - p[P_A + 1], o[2] - p[P_A + 2]};
    const float baba = dot3(ba, ba), bard = dot3(ba, v), baoa = dot3(ba, oa), rdoa = dot3(v, oa), oaoa = dot3(oa, oa);
    const float a = baba - bard * bard;
    float y;
    if (a > 1e-8f * baba) {
      const float b = baba * rdoa - baoa * bard;
      const float c = baba * oaoa - baoa * baoa - r * r * baba;
      const float h = b * b - a * c;
      if (h < 0.f) return BIG;
      const float t = (-b - sqrtf(h)) / a;
      y = baoa + t * bard;
      if (y > 0.f && y < baba) {
        if (!(t > 0.f)) return BIG;
        if (want_n) {
          const float s = y / baba, ir = 1.f / r;
          for (int k = 0; k < 3; ++k) nrm[k] = (oa[k] + t * v[k] - ba[k] * s) * ir;
        }
        return t;
      }
    } else {
      y = bard > 0.f ? -1.f : baba + 1.f;
    }
    float oc[3];
    for (int k = 0; k < 3; ++k) oc[k] = y <= 0.f ? oa[k] : oa[k] - ba[k];
    const float b = dot3(v, oc), c = dot3(oc, oc) - r * r;
    const float h = b * b - c;
    if (!(h > 0.f)) return BIG;
    const float t = -b - sqrtf(h);
    if (!(t > 0.f)) return BIG;
    if (want_n) {
      const float ir = 1.f / r;
      for (int k = 0; k < 3; ++k) nrm[k] = (oc[k] + t * v[k]) * ir;
    }
    return t;
  }
  if (type == H12RENDER_BOX) {
    const float oc[3] = {o[0] - p[P_A], o[1] - p[P_A + 1], o[2] - p[P_A + 2]};
    const float* R = p + P_AX;
    float tn = -BIG, tf = BIG, sgn = 0.f;
    int axis = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float ol = R[i] * oc[0] + R[3 + i] * oc[1] + R[6 + i] * oc[2];
      const float vl = R[i] * v[0] + R[3 + i] * v[1] + R[6 + i] * v[2];
      const float hh = p[P_D + i];
      if (fabsf(vl) < 1e-12f) {
        if (fabsf(ol) > hh) return BIG;
        continue;
      }
      const float inv = 1.f / vl;
      const float t1 = (-hh - ol) * inv, t2 = (hh - ol) * inv;
      const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
      if (lo > tn) { tn = lo; axis = i; sgn = vl > 0.f ? -1.f : 1.f; }
      tf = fminf(tf, hi);
    }
    if (!(tn < tf) || !(tn > 0.f)) return BIG;
    if (want_n) { nrm[0] = sgn * R[axis]; nrm[1] = sgn * R[3 + axis]; nrm[2] = sgn * R[6 + axis]; }
    return tn;
  }
  return BIG;
}

// the heightfield of h12env.hip's ground(), restated in the view's env frame (ground_local's formulation): height
// relative to the env origin at the env-local point (xl, yl) and the slopes.
__device__ __forceinline__ float ground_at(const RenderArgs& A, const float* org, float xl, float yl, float& gx, float& gy) {
  const float cu = (org[0] - A.x0) * A.inv_hs, cv = (org[1] - A.y0) * A.inv_hs;
  const float lim = 1.0e6f;
  const float iu0 = fminf(fmaxf(floorf(cu), -lim), lim), iv0 = fminf(fmaxf(floorf(cv), -lim), lim);
  const float u = (cu - floorf(cu)) + xl * A.inv_hs, w = (cv - floorf(cv)) + yl * A.inv_hs;
  const float fu0 = floorf(u), fv0 = floorf(w);
  int ix = (int)iu0 + (int)fminf(fmaxf(fu0, -lim), lim), iy = (int)iv0 + (int)fminf(fmaxf(fv0, -lim), lim);
  float fu = u - fu0, fv = w - fv0;
  if (ix < 0) { ix = 0; fu = 0.f; }
  if (ix > A.nx - 2) { ix = A.nx - 2; fu = 1.f - 1e-3f; }
  if (iy < 0) { iy = 0; fv = 0.f; }
  if (iy > A.ny - 2) { iy = A.ny - 2; fv = 1.f - 1e-3f; }
  const float* hp = A.heights + (size_t)ix * A.ny + iy;
  const float h00 = hp[0], h01 = hp[1], h10 = hp[A.ny], h11 = hp[A.ny + 1];
  float a, b;
  if (fv >= fu) { a = h11 - h01; b = h01 - h00; }
  else { a = h10 - h00; b = h11 - h10; }
  gx = a * A.inv_hs;
  gy = b * A.inv_hs;
  return (h00 - org[2]) + fu * a + fv * b;
}

__global__ __launch_bounds__(TILE * TILE) void render_kernel(RenderArgs A) {
  __shared__ __attribute__((aligned(16))) float sv[VIEW_WORDS];
  __shared__ unsigned long long s_mask;
  const int v = blockIdx.z, t = threadIdx.x;
  const float* src = A.scratch + (size_t)v * VIEW_WORDS;
  const int ntot_g = __float_as_int(src[H_NTOT]);
  const int ntot = ntot_g < 0 ? 0 : (ntot_g > H12RENDER_MAX_PRIMS ? H12RENDER_MAX_PRIMS : ntot_g);
  const int words = HDR_WORDS + ntot * PRIM_WORDS;
  for (int k = t; k < words / 4; k += TILE * TILE)
    reinterpret_cast<float4*>(sv)[k] = reinterpret_cast<const float4*>(src)[k];
  __syncthreads();
  const int tj0 = blockIdx.x * TILE, ti0 = blockIdx.y * TILE;
  if (t < 64) {
    bool in = false;
    if (t < ntot) {
      const float* p = sv + HDR_WORDS + t * PRIM_WORDS;
      in = __float_as_int(p[P_TYPE]) != 0;
      if (in && A.cull) {
        const int j0 = __float_as_int(p[P_BB]), j1 = __float_as_int(p[P_BB + 1]);
        const int i0 = __float_as_int(p[P_BB + 2]), i1 = __float_as_int(p[P_BB + 3]);
        in = j0 <= tj0 + TILE - 1 && j1 >= tj0 && i0 <= ti0 + TILE - 1 && i1 >= ti0;
      }
    }
    const unsigned long long m = __ballot(in);
    if (t == 0) s_mask = m;
  }
  __syncthreads();
  const int j = tj0 + (t & (TILE - 1)), i = ti0 + (t >> 4);
  if (j >= A.W || i >= A.H) return;
  const float* eye = sv + H_EYE;
  const float x = (((float)j + 0.5f) / (float)A.W * 2.f - 1.f) * (A.tan_half * (float)A.W / (float)A.H);
  const float y = -(((float)i + 0.5f) / (float)A.H * 2.f - 1.f) * A.tan_half;
  float d[3];
  for (int k = 0; k < 3; ++k) d[k] = sv[H_F + k] + x * sv[H_R + k] + y * sv[H_U + k];
  const float inv = 1.f / sqrtf(dot3(d, d));
  for (int k = 0; k < 3; ++k) d[k] *= inv;

  // nearest primitive: strict < in index order, so a tie goes to the lower index
  float tbest = BIG, nb[3] = {0.f, 0.f, 1.f};
  int best = H12RENDER_ID_SKY;
  unsigned long long m = s_mask;
  while (m) {
    const int p = __ffsll((long long)m) - 1;
    m &= m - 1;
    float nn[3];
    const float tp = hit_prim(sv + HDR_WORDS + p * PRIM_WORDS, eye, d, nn, true);
    if (tp < tbest) { tbest = tp; best = p; nb[0] = nn[0]; nb[1] = nn[1]; nb[2] = nn[2]; }
  }
  // ground: wins only when strictly nearer than the primitive
  float tg = BIG, ng[3] = {0.f, 0.f, 1.f};
  if (!A.heights) {
    if (d[2] < 0.f && eye[2] > 0.f) tg = eye[2] / (-d[2]);
  } else {
    const float* org = sv + H_ORG;
    float gx, gy, lo = 0.f;
    for (int k = 1; k <= A.n_march; ++k) {
      if (lo >= tbest) break;  // a hit from here on could not beat the primitive
      const float hi = (float)k * H12RENDER_MARCH_STEP;
      const float g = eye[2] + hi * d[2] - ground_at(A, org, eye[0] + hi * d[0], eye[1] + hi * d[1], gx, gy);
      if (g <= 0.f) {
        float a = lo, b = hi;
        for (int q = 0; q < H12RENDER_NBISECT; ++q) {
          const float mid = 0.5f * (a + b);
          const float gm = eye[2] + mid * d[2] - ground_at(A, org, eye[0] + mid * d[0], eye[1] + mid * d[1], gx, gy);
          if (gm <= 0.f) b = mid; else a = mid;
        }
        tg = b;
        ground_at(A, org, eye[0] + tg * d[0], eye[1] + tg * d[1], gx, gy);
        const float in2 = 1.f / sqrtf(gx * gx + gy * gy + 1.f);
        ng[0] = -gx * in2; ng[1] = -gy * in2; ng[2] = in2;
        break;
      }
      lo = hi;
    }
  }
  if (!(tg > 0.f) || !(tg < A.far)) tg = BIG;

  float col[3];
  float tout = 0.f;
  int idout;
  if (tg < tbest || best >= 0) {
    const bool gnd = tg < tbest;
    const float th = gnd ? tg : tbest;
    float nh[3], alb[3], hp[3];
    for (int k = 0; k < 3; ++k) { nh[k] = gnd ? ng[k] : nb[k]; hp[k] = eye[k] + th * d[k]; }
    if (gnd) {
      if (th < H12RENDER_CHECKER_FAR) {
        const int cx = (int)floorf(sv[H_CFX] + hp[0] / H12RENDER_CHECKER), cy = (int)floorf(sv[H_CFY] + hp[1] / H12RENDER_CHECKER);
        const int par = (cx + cy + __float_as_int(sv[H_CPAR])) & 1;
        for (int k = 0; k < 3; ++k) alb[k] = par ? COL_CHK1[k] : COL_CHK0[k];
      } else {
        for (int k = 0; k < 3; ++k) alb[k] = COL_FAR[k];
      }
    } else {
      const float* p = sv + HDR_WORDS + best * PRIM_WORDS + P_RGB;
      for (int k = 0; k < 3; ++k) alb[k] = p[k];
    }
    const float ndl = dot3(nh, A.sun);
    float lit = 0.f;
    if (ndl > 0.f) {
      lit = 1.f;
      float so[3];
      for (int k = 0; k < 3; ++k) so[k] = hp[k] + H12RENDER_SHADOW_EPS * nh[k];
      for (int p = 0; p < ntot; ++p) {  // every row casts shadows: no tile mask here
        float dummy[3];
        if (hit_prim(sv + HDR_WORDS + p * PRIM_WORDS, so, A.sun, dummy, false) < BIG) { lit = 0.f; break; }
      }
    }
    const float sh = AMBIENT + DIFFUSE * fmaxf(ndl, 0.f) * lit;
    for (int k = 0; k < 3; ++k) col[k] = alb[k] * sh;
    tout = th;
    idout = gnd ? H12RENDER_ID_GROUND : best;
  } else {
    const float s = fminf(fmaxf(0.5f + 0.5f * d[2], 0.f), 1.f);
    for (int k = 0; k < 3; ++k) col[k] = (1.f - s) * COL_HORIZON[k] + s * COL_ZENITH[k];
    idout = H12RENDER_ID_SKY;
  }
  const size_t pix = ((size_t)v * A.H + i) * A.W + j;
  for (int k = 0; k < 3; ++k)
    A.rgb[pix * 3 + k] = (uint8_t)(int)floorf(255.f * fminf(fmaxf(col[k], 0.f), 1.f) + 0.5f);
  if (A.id) A.id[pix] = idout;
  if (A.depth)
    reinterpret_cast<uint32_t*>(A.depth)[pix] = idout == H12RENDER_ID_SKY ? 0x7f800000u : __float_as_uint(tout);
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
size_t table_bytes(int n) { return offsetof(Table, rows) + sizeof(h12render_prim) * (size_t)n; }

}  // namespace

extern "C" {

const char* h12render_last_error(void) { return g_err; }

int h12render_layout(int n_views, int width, int height, size_t* scratch_bytes, size_t* rgb_bytes, size_t* id_bytes,
                     size_t* depth_bytes) {
  if (n_views < 1 || n_views > 65535) return fail(H12RENDER_E_ARG, "n_views: %d (1..65535)", n_views);
  if (width < 1 || width > 8192) return fail(H12RENDER_E_ARG, "width: %d (1..8192)", width);
  if (height < 1 || height > 8192) return fail(H12RENDER_E_ARG, "height: %d (1..8192)", height);
  const size_t px = (size_t)n_views * width * height;
  if (scratch_bytes) *scratch_bytes = (size_t)n_views * VIEW_WORDS * sizeof(float);
  if (rgb_bytes) *rgb_bytes = px * 3;
  if (id_bytes) *id_bytes = px * 4;
  if (depth_bytes) *depth_bytes = px * 4;
  return H12RENDER_OK;
}

size_t h12render_table_bytes(int n_prims) {
  if (n_prims < 0 || n_prims > H12RENDER_MAX_PRIMS) {
    fail(H12RENDER_E_ARG, "n_prims: %d (0..%d)", n_prims, H12RENDER_MAX_PRIMS);
    return 0;
  }
  return (table_bytes(n_prims) + 15) & ~(size_t)15;
}

int h12render_pack_table(const h12env_model* model, const h12render_prim* prims, int n_prims, void* out_host) {
  if (!model) return fail(H12RENDER_E_ARG, "model: null");
  if (!out_host) return fail(H12RENDER_E_ARG, "out_host: null");
  if (n_prims < 0 || n_prims > H12RENDER_MAX_PRIMS)
    return fail(H12RENDER_E_ARG, "n_prims: %d (0..%d)", n_prims, H12RENDER_MAX_PRIMS);
  if (n_prims > 0 && !prims) return fail(H12RENDER_E_ARG, "prims: null");
  for (int j = 0; j < H12_NJ; ++j) {
    if (model->parent[j] < -1 || model->parent[j] >= j) return fail(H12RENDER_E_ARG, "model.parent[%d]: %d", j, model->parent[j]);
    if (model->axis[j] < 0 || model->axis[j] > 2) return fail(H12RENDER_E_ARG, "model.axis[%d]: %d", j, model->axis[j]);
    for (int a = 0; a < 3; ++a)
      if (!fin(model->joint_pos[j][a])) return fail(H12RENDER_E_ARG, "model.joint_pos[%d]: not finite", j);
  }
  for (int p = 0; p < H12_NFOOT_PTS; ++p)
    for (int a = 0; a < 3; ++a)
      if (!fin(model->foot_pts[p][a])) return fail(H12RENDER_E_ARG, "model.foot_pts[%d]: not finite", p);
  if (!fin(model->root_height)) return fail(H12RENDER_E_ARG, "model.root_height: not finite");
  for (int i = 0; i < n_prims; ++i) {
    const h12render_prim& p = prims[i];
    if (p.type != H12RENDER_CAPSULE && p.type != H12RENDER_BOX) return fail(H12RENDER_E_ARG, "prims[%d].type: %d", i, p.type);
    if (p.body < 0 || p.body >= H12RENDER_NBODY) return fail(H12RENDER_E_ARG, "prims[%d].body: %d (0..12)", i, p.body);
    for (int a = 0; a < 3; ++a) {
      if (!fin(p.p0[a])) return fail(H12RENDER_E_ARG, "prims[%d].p0: not finite", i);
      if (!fin(p.p1[a])) return fail(H12RENDER_E_ARG, "prims[%d].p1: not finite", i);
      if (!(p.rgb[a] >= 0.f && p.rgb[a] <= 1.f)) return fail(H12RENDER_E_ARG, "prims[%d].rgb: outside [0, 1]", i);
      if (p.type == H12RENDER_BOX && !(p.p1[a] > 0.f)) return fail(H12RENDER_E_ARG, "prims[%d].p1: half extents must be > 0", i);
    }
    if (p.type == H12RENDER_CAPSULE && !(p.radius > 0.f && fin(p.radius)))
      return fail(H12RENDER_E_ARG, "prims[%d].radius: must be > 0 and finite", i);
  }
  memset(out_host, 0, h12render_table_bytes(n_prims));
  Table* T = static_cast<Table*>(out_host);
  T->n_prims = n_prims;
  for (int j = 0; j < H12_NJ; ++j) {
    T->parent[j] = model->parent[j];
    T->axis[j] = model->axis[j];
    for (int a = 0; a < 3; ++a) T->joint_pos[j][a] = model->joint_pos[j][a];
  }
  for (int p = 0; p < H12_NFOOT_PTS; ++p)
    for (int a = 0; a < 3; ++a) T->foot_pts[p][a] = model->foot_pts[p][a];
  T->root_height = model->root_height;
  for (int i = 0; i < n_prims; ++i) T->rows[i] = prims[i];
  return H12RENDER_OK;
}

int h12render_render(const h12render_frame* fr, const h12render_camera* cam, void* stream) {
  if (!fr) return fail(H12RENDER_E_ARG, "frame: null");
  if (!cam) return fail(H12RENDER_E_ARG, "camera: null");
  if (!fr->fstate) return fail(H12RENDER_E_ARG, "fstate: null");
  if (!fr->istate) return fail(H12RENDER_E_ARG, "istate: null");
  if (fr->n_envs < 1) return fail(H12RENDER_E_ARG, "n_envs: %d", fr->n_envs);
  if (fr->n_views < 1 || fr->n_views > 65535) return fail(H12RENDER_E_ARG, "n_views: %d (1..65535)", fr->n_views);
  if (!fr->env_ids) return fail(H12RENDER_E_ARG, "env_ids: null");
  if (!fr->env_ids_host) return fail(H12RENDER_E_ARG, "env_ids_host: null");
  for (int v = 0; v < fr->n_views; ++v)
    if (fr->env_ids_host[v] < 0 || fr->env_ids_host[v] >= fr->n_envs)
      return fail(H12RENDER_E_ARG, "env_ids[%d]: %d (0..%d)", v, fr->env_ids_host[v], fr->n_envs - 1);
  if (fr->heights) {
    if (fr->nx < 2 || fr->ny < 2) return fail(H12RENDER_E_ARG, "nx, ny: %d x %d (>= 2 each)", fr->nx, fr->ny);
    if (!(fr->hscale > 0.f && fin(fr->hscale))) return fail(H12RENDER_E_ARG, "hscale: must be > 0 and finite");
    if (!fin(fr->x0) || !fin(fr->y0)) return fail(H12RENDER_E_ARG, "x0, y0: not finite");
  }
  if (!fr->table) return fail(H12RENDER_E_ARG, "table: null");
  const int ntot = fr->n_prims + (fr->overlays ? H12RENDER_NOVERLAY : 0);
  if (fr->n_prims < 0 || ntot > H12RENDER_MAX_PRIMS)
    return fail(H12RENDER_E_ARG, "n_prims: %d rows + %d overlay rows (at most %d)", fr->n_prims, ntot - fr->n_prims,
                H12RENDER_MAX_PRIMS);
  if (cam->width < 1 || cam->width > 8192) return fail(H12RENDER_E_ARG, "camera.width: %d (1..8192)", cam->width);
  if (cam->height < 1 || cam->height > 8192) return fail(H12RENDER_E_ARG, "camera.height: %d (1..8192)", cam->height);
  if (cam->origin_type != H12RENDER_ORIGIN_WORLD && cam->origin_type != H12RENDER_ORIGIN_ASSET_ROOT)
    return fail(H12RENDER_E_ARG, "camera.origin_type: %d", cam->origin_type);
  double f[3], fn = 0, sn = 0;
  for (int a = 0; a < 3; ++a) {
    if (!fin(cam->eye[a])) return fail(H12RENDER_E_ARG, "camera.eye: not finite");
    if (!fin(cam->lookat[a])) return fail(H12RENDER_E_ARG, "camera.lookat: not finite");
    if (!fin(cam->sun_dir[a])) return fail(H12RENDER_E_ARG, "camera.sun_dir: not finite");
    f[a] = (double)cam->lookat[a] - (double)cam->eye[a];
    fn += f[a] * f[a];
    sn += (double)cam->sun_dir[a] * cam->sun_dir[a];
  }
  if (!(fn > 1e-12)) return fail(H12RENDER_E_ARG, "camera.lookat: equals eye");
  if (!(f[0] * f[0] + f[1] * f[1] > 1e-10 * fn)) return fail(H12RENDER_E_ARG, "camera.lookat: view direction parallel to z");
  if (!(std::fabs(sn - 1.0) < 1e-3)) return fail(H12RENDER_E_ARG, "camera.sun_dir: not a unit vector");
  if (!(cam->fovy > 1e-3f && cam->fovy < 3.13f)) return fail(H12RENDER_E_ARG, "camera.fovy: %g rad (0..pi)", (double)cam->fovy);
  if (!(cam->far > 0.f && cam->far <= H12RENDER_MAX_FAR))
    return fail(H12RENDER_E_ARG, "camera.far: %g (0..%g]", (double)cam->far, (double)H12RENDER_MAX_FAR);
  size_t need = 0;
  h12render_layout(fr->n_views, cam->width, cam->height, &need, nullptr, nullptr, nullptr);
  if (!fr->scratch || ((uintptr_t)fr->scratch & 15)) return fail(H12RENDER_E_ARG, "scratch: null or not 16-byte aligned");
  if (fr->scratch_bytes < need) return fail(H12RENDER_E_ARG, "scratch_bytes: %zu < %zu", fr->scratch_bytes, need);
  if (!fr->rgb) return fail(H12RENDER_E_ARG, "rgb: null");
  if ((uintptr_t)fr->table & 3) return fail(H12RENDER_E_ARG, "table: not 4-byte aligned");

  RenderArgs A;
  memset(&A, 0, sizeof A);
  A.F = fr->fstate; A.I = fr->istate; A.n = fr->n_envs;
  A.env_ids = fr->env_ids; A.n_views = fr->n_views;
  A.view_origins = fr->heights ? nullptr : fr->view_origins;
  A.heights = fr->heights; A.nx = fr->nx; A.ny = fr->ny;
  A.inv_hs = fr->heights ? 1.f / fr->hscale : 0.f; A.x0 = fr->x0; A.y0 = fr->y0;
  A.table = static_cast<const Table*>(fr->table);
  A.n_prims = fr->n_prims; A.overlays = fr->overlays != 0; A.cull = fr->cull != 0;
  A.scratch = static_cast<float*>(fr->scratch);
  A.rgb = fr->rgb; A.id = fr->id; A.depth = fr->depth;
  A.W = cam->width; A.H = cam->height; A.origin_type = cam->origin_type;
  for (int a = 0; a < 3; ++a) { A.eye[a] = cam->eye[a]; A.lookat[a] = cam->lookat[a]; A.sun[a] = cam->sun_dir[a]; }
  A.tan_half = (float)std::tan(0.5 * (double)cam->fovy);
  A.far = cam->far;
  A.n_march = (int)std::ceil((double)cam->far / (double)H12RENDER_MARCH_STEP);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(render_setup_kernel, dim3(fr->n_views), dim3(64), 0, s, A);
  const dim3 grid((cam->width + TILE - 1) / TILE, (cam->height + TILE - 1) / TILE, fr->n_views);
  hipLaunchKernelGGL(render_kernel, grid, dim3(TILE * TILE), 0, s, A);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(H12RENDER_E_HIP, "launch: %s", hipGetErrorString(err));
  return H12RENDER_OK;
}

}  // extern "C"
