/* h12render.h: device ray-caster of the robot's kinematic skeleton over the task's ground (csrc/h12_render.hip,
 * part of libh12env.so).  Replaces what the reference gets from Isaac Sim's viewport through
 * gym.wrappers.RecordVideo(render_mode="rgb_array") (scripts/rsl_rl/{train,play}.py, scripts/clean_rl/{train,play}.py).
 *
 * The entry points work on caller-owned raw pointers only: the env's field-major workspace (h12env.h: fstate
 * [H12_NF_FLOAT][n], istate [H12_NF_INT][n]), a packed primitive table, optionally the heightfield as
 * h12env_set_terrain takes it, a list of env ids (one view each) and a camera.  No h12env handle is needed.
 * h12render_render is two stream-ordered launches (render_setup_kernel, render_kernel); it allocates nothing, never
 * synchronises, uses no atomics and may be captured in a graph.  It only reads the workspace.
 * Return 0 or a negative code; the message of the last failure on the calling thread is h12render_last_error().
 * All arguments are validated before any HIP call.
 *
 * The image is defined exactly in DESIGN.md section 7i (camera, primitives, ground, nearest hit, shading, overlays).
 */
#ifndef H12RENDER_H
#define H12RENDER_H

#include <stddef.h>
#include <stdint.h>

#include "h12env.h"

#ifdef __cplusplus
extern "C" {
#endif

#define H12RENDER_OK 0
#define H12RENDER_E_ARG (-1)
#define H12RENDER_E_HIP (-2)

#define H12RENDER_MAX_PRIMS 64     /* table rows + overlay rows of one view (the tile mask is 64 bits) */
#define H12RENDER_NOVERLAY 10      /* 8 sole contact spheres (foot-major), commanded velocity, actual velocity */
#define H12RENDER_NBODY 13         /* 0 pelvis, 1..12 the leg links in body_names order */

#define H12RENDER_CAPSULE 1        /* p0, p1: segment end points (body frame); radius */
#define H12RENDER_BOX 2            /* p0: centre, p1: half extents (body frame axes) */

#define H12RENDER_ORIGIN_WORLD 0      /* eye / lookat absolute in the view's env frame */
#define H12RENDER_ORIGIN_ASSET_ROOT 1 /* eye / lookat offsets from the env's base position (no rotation) */

#define H12RENDER_ID_SKY (-1)
#define H12RENDER_ID_GROUND (-2)

/* constants of the image definition (not tunables) */
#define H12RENDER_MARCH_STEP 0.05f /* heightfield march step along the ray [m] */
#define H12RENDER_NBISECT 16       /* bisections of the bracketing march interval */
#define H12RENDER_MAX_FAR 200.0f   /* largest far distance accepted (bounds the march count at 4000) */
#define H12RENDER_CHECKER 0.5f     /* checker cell [m] */
#define H12RENDER_CHECKER_FAR 10.0f /* hits at t >= this get the uniform ground colour */
#define H12RENDER_SHADOW_EPS 1e-3f /* shadow ray origin = hit + this * n */

typedef struct h12render_prim {
  int32_t type;      /* H12RENDER_CAPSULE / H12RENDER_BOX */
  int32_t body;      /* 0..12 */
  float p0[3], p1[3];
  float radius;      /* capsule only */
  float rgb[3];      /* linear albedo in [0, 1] */
} h12render_prim;

typedef struct h12render_camera {
  int32_t width, height;   /* pixels, 1..8192 each */
  int32_t origin_type;     /* H12RENDER_ORIGIN_* */
  float eye[3], lookat[3];
  float fovy;              /* vertical field of view [rad], (0, pi) */
  float sun_dir[3];        /* unit vector towards the sun */
  float far;               /* ground hits beyond this distance are sky; (0, H12RENDER_MAX_FAR] */
} h12render_camera;

typedef struct h12render_frame {
  const float* fstate;       /* device [H12_NF_FLOAT][n_envs], read only */
  const int32_t* istate;     /* device [H12_NF_INT][n_envs], read only */
  int32_t n_envs;
  const int32_t* env_ids;    /* device [n_views], each in [0, n_envs): validated by the caller's host copy below */
  const int32_t* env_ids_host; /* host copy of env_ids, checked against n_envs before any launch */
  int32_t n_views;           /* M >= 1 */
  const float* view_origins; /* device [n_views][3] or NULL (zeros): plane only, world = env-local + this */
  const float* heights;      /* device heightfield as h12env_set_terrain, or NULL for the plane z = 0; with a
                                heightfield the workspace POS is world and H12_F_ORIGIN the env origin */
  int32_t nx, ny;
  float hscale, x0, y0;
  const void* table;         /* device copy of the packed table (h12render_pack_table) */
  int32_t n_prims;           /* rows of that table */
  int32_t overlays;          /* != 0: append the H12RENDER_NOVERLAY overlay rows */
  int32_t cull;              /* != 0: per-tile primitive culling (same image either way) */
  void* scratch;             /* device, h12render_layout's scratch_bytes, 16-byte aligned */
  size_t scratch_bytes;
  uint8_t* rgb;              /* device [M][H][W][3] (required) */
  int32_t* id;               /* device [M][H][W] or NULL: primitive index, H12RENDER_ID_GROUND, H12RENDER_ID_SKY */
  float* depth;              /* device [M][H][W] or NULL: t along the unit ray, +inf for sky */
} h12render_frame;

/* Buffer sizes for n_views views of width x height pixels (no device needed). */
int h12render_layout(int n_views, int width, int height, size_t* scratch_bytes, size_t* rgb_bytes, size_t* id_bytes,
                     size_t* depth_bytes);
/* Bytes of the packed table of n_prims rows; 0 with the error set when n_prims is out of range. */
size_t h12render_table_bytes(int n_prims);
/* Validates the rows and writes the packed table (the kinematic constants of model + the rows) into out_host; the
 * caller copies it to the device once. */
int h12render_pack_table(const h12env_model* model, const h12render_prim* prims, int n_prims, void* out_host);
/* The two launches. */
int h12render_render(const h12render_frame* frame, const h12render_camera* cam, void* stream);
const char* h12render_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* H12RENDER_H */
