/* h12learn.h: learner-side device entry points of libh12env.so (csrc/h12_learn.hip).
 *
 * The CleanRL PPO of the CaT tasks (h12env/cleanrl.py) calls two pieces of per-step / per-iteration work that
 * are launch-bound in torch: the running mean/variance normaliser and the soft-termination GAE.
 *
 * Every compute entry point
 *   - takes raw device pointers and a HIP stream,
 *   - allocates nothing and never synchronises (safe inside HIP graph capture),
 *   - keeps all state on the device; the caller owns the workspace (size: *_workspace_bytes).
 * They return 0 on success and a negative code otherwise; the message of the last failure on the calling
 * thread is h12learn_last_error().  These functions are independent of the env ABI version (h12env.h).
 */
#ifndef H12LEARN_H
#define H12LEARN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H12LEARN_OK 0
#define H12LEARN_E_ARG (-1)
#define H12LEARN_E_HIP (-2)

/* Rows of x one block of the statistics kernel reduces (the row-chunk size R); a query so tests can place
 * n at R-1, R, R+1, 2R+1. */
int h12learn_rms_row_chunk(void);

/* Bytes of workspace h12learn_rms_forward needs for an [n][d] input.  The first 64 bytes hold the arrival
 * counter: the caller zeroes the workspace once after allocating it; every call leaves the counter at zero. */
size_t h12learn_rms_workspace_bytes(long long n, int d);

/* RunningMeanStd.forward(x, update): x, y are [n][d] fp32 row-major contiguous (y may alias x); mean[d],
 * var[d] and the scalar count are fp32 device tensors updated in place when update != 0 (Chan merge of the
 * batch mean / population variance over the n rows, update_mean_var_count_from_moments), then
 * y = (x - mean) / sqrt(var + epsilon).  With update == 0 the statistics are only read and workspace may be
 * null.  Two launches with update, one without.  The statistics are bitwise reproducible from run to run
 * (per-chunk shifted two-pass partials, merged in chunk-index order by the last block to arrive). */
int h12learn_rms_forward(const float* x, float* y, float* mean, float* var, float* count, long long n, int d,
                         float epsilon, int update, void* workspace, size_t workspace_bytes, void* stream);

/* GAE over soft terminations (CaT): rewards, values, dones, true_dones, advantages, returns are [T][N] fp32;
 * next_value, next_done, next_true_done are [N].  Backward over t, with nn = 1 - done[t+1] and
 * tn = 1 - true_done[t+1] (the next_* inputs at t = T-1):
 *   delta = r[t] + gamma * v[t+1] * nn * tn - v[t];  adv[t] = last = delta + gamma_lambda * nn * tn * last
 *   returns = adv + values
 * evaluated left to right in separately rounded fp32 operations (no contraction): bit-identical to the fp32
 * torch loop.  gamma_lambda is the product gamma * lambda formed in double by the caller, then narrowed. */
int h12learn_gae_soft(const float* rewards, const float* values, const float* dones, const float* true_dones,
                      const float* next_value, const float* next_done, const float* next_true_done,
                      float gamma, float gamma_lambda, int T, int N, float* advantages, float* returns,
                      void* stream);

const char* h12learn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* H12LEARN_H */
