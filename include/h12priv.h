/* h12priv.h: the privileged ("critic") observation group of the H1-2 velocity tasks (csrc/h12_priv.hip, part of
 * libh12env.so).  rsl_rl's asymmetric actor-critic reads it as extras["observations"]["critic"]; the reference's task
 * cfgs define no such group (velocity_env_cfg.py:113-141 has the policy group only), so the row is this project's own
 * and is defined here and in DESIGN.md section 7k.
 *
 * h12priv_observe turns the env's field-major workspace (h12env.h: fstate [H12_NF_FLOAT][n], istate [H12_NF_INT][n])
 * as the last h12env_step / h12env_reset left it into one noise-free fp32 row per env, row-major (n, W), no history.
 * It works on caller-owned raw pointers only (no h12env handle), is ONE stream-ordered launch, allocates nothing,
 * never synchronises, uses no atomics, only reads the workspace and may be captured in a graph.
 * Return 0 or a negative code; the message of the last failure on the calling thread is h12priv_last_error().
 * All arguments are validated before any HIP call.
 *
 * Row layout (terms in this order; W = 65 on the plane, 252 with a heightfield):
 *   base_lin_vel 3       pelvis COM velocity in the base frame, R^T (VLIN + R WANG x R ROOT_COM)
 *   base_ang_vel 3       WANG
 *   projected_gravity 3  -R[2][:]
 *   velocity_commands 3  CMD
 *   joint_pos 12         Q - Q0            joint_vel 12  QD            actions 12  ACT
 *   height_scan 187      heightfield only: the policy's 17 x 11 scan (x fastest), clip(z - hit z - offset), no noise
 *   base_height 1        POS.z; heightfield: POS.z - ground height under the base
 *   feet_contact 2       1.0 when any of the foot's four sole-sphere flags (H12_I_PACK bits 13 + 4 foot ..) is set
 *   feet_air_time 2      H12_F_AIR         feet_contact_time 2  H12_F_CONTACT
 *   feet_force 2         foot_force of the step (|net contact force|), 0 for an env reset by it (PACK bits 9-10 == 0)
 *   actuator_lag 3       the three actuator groups' lags (PACK bits 0-8) as floats
 *   sole_friction 4      H12_F_MU (static L, dynamic L, static R, dynamic R), or the constant pair for both soles
 *   added_mass 1         H12_F_DMASS, or 0
 * Every value is multiplied by its term's scale.
 */
#ifndef H12PRIV_H
#define H12PRIV_H

#include <stddef.h>
#include <stdint.h>

#include "h12env.h"

#ifdef __cplusplus
extern "C" {
#endif

#define H12PRIV_OK 0
#define H12PRIV_E_ARG (-1)
#define H12PRIV_E_HIP (-2)

enum {
  H12PRIV_T_BASE_LIN_VEL = 0, H12PRIV_T_BASE_ANG_VEL, H12PRIV_T_PROJECTED_GRAVITY, H12PRIV_T_VELOCITY_COMMANDS,
  H12PRIV_T_JOINT_POS, H12PRIV_T_JOINT_VEL, H12PRIV_T_ACTIONS, H12PRIV_T_HEIGHT_SCAN, H12PRIV_T_BASE_HEIGHT,
  H12PRIV_T_FEET_CONTACT, H12PRIV_T_FEET_AIR_TIME, H12PRIV_T_FEET_CONTACT_TIME, H12PRIV_T_FEET_FORCE,
  H12PRIV_T_ACTUATOR_LAG, H12PRIV_T_SOLE_FRICTION, H12PRIV_T_ADDED_MASS, H12PRIV_NTERMS
};

#define H12PRIV_W_PLANE 65
#define H12PRIV_W_TERRAIN (H12PRIV_W_PLANE + H12_NSCAN) /* 252 */
#define H12PRIV_SCAN_RES 0.1f /* the scan grid's spacing [m]: the policy group's (h12env_config.scan_resolution) */

typedef struct h12priv_config {
  int32_t terrain;           /* 0: plane z = 0, no height_scan term; 1: heightfield below (required then) */
  const float* heights;      /* device heightfield as h12env_set_terrain takes it */
  int32_t nx, ny;
  float hscale, x0, y0;
  float mu_static, mu_dynamic; /* the constant sole friction, emitted when per_env_friction == 0 */
  int32_t per_env_friction;  /* != 0: sole_friction reads H12_F_MU */
  int32_t per_env_mass;      /* != 0: added_mass reads H12_F_DMASS */
  float scan_offset, scan_clip; /* the policy group's height_scan offset and clip (h12env_config) */
  float scale[H12PRIV_NTERMS]; /* per term, indexed by H12PRIV_T_* */
} h12priv_config;

/* Host only (no device access): the row width for the terrain flag and the rows (term id, offset, width) of the terms
 * present, in row order.  table may be NULL; n_terms receives the number of rows written. */
int h12priv_layout(int terrain, int32_t* width, int32_t table[H12PRIV_NTERMS][3], int32_t* n_terms);
/* The launch.  workspace: the env workspace of n envs (h12env_state_bytes(n): the float fields, then the int fields);
 * foot_force: device [n][2] (h12env_step_out.foot_force) or NULL (zeros); out: device [n][W]. */
int h12priv_observe(const void* workspace, int n, const h12priv_config* cfg, const float* foot_force, float* out,
                    void* stream);
/* A subset of the row's terms, compacted (the rnd_state group, h12env/rnd.py): term_mask has bit H12PRIV_T_x set for
 * every term that is written, in row order; out is device [n][W'] with W' the sum of their widths.  The rows are built
 * by the device code of h12priv_observe, so every column holds the bits of the same column of the full row; ONE launch.
 * A mask that names no term, a term past the table, or height_scan without cfg.terrain is H12PRIV_E_ARG.
 * h12priv_layout_terms (host only) gives W' and the (term id, offset, width) rows of the compacted row. */
int h12priv_layout_terms(int terrain, uint32_t term_mask, int32_t* width, int32_t table[H12PRIV_NTERMS][3],
                         int32_t* n_terms);
int h12priv_observe_terms(const void* workspace, int n, const h12priv_config* cfg, const float* foot_force,
                          uint32_t term_mask, float* out, void* stream);
const char* h12priv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* H12PRIV_H */
