/* h12student.h: the deployable ("student") observation group of the H1-2 velocity tasks (csrc/h12_student.hip, part
 * of libh12env.so).  A distilled student policy reads it as extras["observations"]["student"]: only what the robot
 * measures (no base linear velocity, no height scan), with the Flat task's noise and a term-major history, so a policy
 * trained on it runs behind the deploy stack's observation handler unchanged.  DESIGN.md section 7s.
 *
 * h12student_observe turns the env's field-major workspace (h12env.h: fstate [H12_NF_FLOAT][n], istate [H12_NF_INT][n])
 * as the last h12env_step / h12env_reset left it, and the previous call's rows, into one fp32 row per env, row-major
 * (n, W), W = 45 H.  It works on caller-owned raw pointers only (no h12env handle, no state of its own: the history
 * lives in the caller's two row buffers), is ONE stream-ordered launch, allocates nothing, never synchronises, uses no
 * atomics, only reads the workspace and prev, and may be captured in a graph.
 * Return 0 or a negative code; the message of the last failure on the calling thread is h12student_last_error().
 * All arguments are validated before any HIP call.
 *
 * Frame (45 floats, the Flat policy frame's order and definitions):
 *   base_ang_vel 3       WANG
 *   projected_gravity 3  -R[2][:]  (the expression of h12_priv.hip)
 *   velocity_commands 3  CMD
 *   joint_pos 12         Q - Q0            joint_vel 12  QD            actions 12  ACT
 * Every value is (value + U(-noise_term, noise_term)) * scale_term: noise first, then scale, no clip.  The noise of frame
 * column c is word c & 3 of
 *   philox4x32-10(key = seed_lo, seed_hi; counter = env_offset + e, step_lo, (5 << 16) | (c >> 2), step_hi)
 * mapped to u = (word >> 8) / 2^24 and fma(2 noise, u, -noise): a pure function of (seed, global env id, step index,
 * column).  Stream 5 is this group's; streams 1-4 are the env's (h12env.hip).  A term whose noise is 0, and every term
 * with enable_corruption == 0, is not touched by the noise path at all.
 *
 * Row: term-major, [term][frame oldest -> newest][width] -- term t starts at column H * (its frame offset), the layout
 * CircularBuffer.buffer() flattening gives and the deploy handler rebuilds.  A row whose H12_I_PACK bits 9-10 are 0 was
 * reset by the step before the call: all H of its frames take the new frame.  Any other row drops its oldest frame
 * (reads prev one frame on) and appends the new one.  prev == NULL: every row fills.  cfg.fill_mask, when set, names
 * the rows that fill instead of the workspace's bits.
 */
#ifndef H12STUDENT_H
#define H12STUDENT_H

#include <stddef.h>
#include <stdint.h>

#include "h12env.h"

#ifdef __cplusplus
extern "C" {
#endif

#define H12STUDENT_OK 0
#define H12STUDENT_E_ARG (-1)
#define H12STUDENT_E_HIP (-2)

enum {
  H12STUDENT_T_BASE_ANG_VEL = 0, H12STUDENT_T_PROJECTED_GRAVITY, H12STUDENT_T_VELOCITY_COMMANDS, H12STUDENT_T_JOINT_POS,
  H12STUDENT_T_JOINT_VEL, H12STUDENT_T_ACTIONS, H12STUDENT_NTERMS
};

#define H12STUDENT_FRAME 45       /* floats per frame */
#define H12STUDENT_MAX_HISTORY 10
#define H12STUDENT_RNG_STREAM 5   /* the Philox stream of this group's noise */

typedef struct h12student_config {
  int32_t history;             /* H, 1 .. H12STUDENT_MAX_HISTORY */
  int32_t enable_corruption;   /* 0: no noise */
  uint32_t seed_lo, seed_hi;   /* the env's seed (h12env_config.seed) */
  uint32_t env_offset;         /* global id of env 0 (h12env_create's env_offset) */
  float noise[H12STUDENT_NTERMS]; /* per term, indexed by H12STUDENT_T_*: the half-width n of U(-n, n); finite, >= 0 */
  float scale[H12STUDENT_NTERMS]; /* per term; finite */
  const uint8_t* fill_mask;    /* NULL: a row fills where its H12_I_PACK bits 9-10 are 0.  Else device [n] bytes that
                                * replace that rule: row e fills where fill_mask[e] != 0 and shifts where it is 0 (a
                                * masked reset knows which rows it reset; the workspace's bits also name the rows the
                                * step before it reset) */
} h12student_config;

/* Host only (no device access): the row width W = 45 H and the rows (term id, offset, width in the row = H x frame
 * width) of the terms, in row order.  table may be NULL; n_terms receives the number of rows written. */
int h12student_layout(int history, int32_t* width, int32_t table[H12STUDENT_NTERMS][3], int32_t* n_terms);
/* The launch.  workspace: the env workspace of n envs (h12env_state_bytes(n): the float fields, then the int fields);
 * prev: device [n][W], the rows of the previous call, or NULL (every row fills); out: device [n][W], must not overlap
 * prev; step_index: the noise counter (the env passes h12env_step's step_index; any int64 is taken). */
int h12student_observe(const void* workspace, int n, const h12student_config* cfg, const float* prev, float* out,
                       int64_t step_index, void* stream);
const char* h12student_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* H12STUDENT_H */
