/* h12learn.h: learner-side device entry points of libh12env.so (csrc/h12_learn.hip, csrc/h12_policy.hip,
 * csrc/h12_policy_train.hip, csrc/h12_policy_rnn.hip, csrc/h12_policy_rnn_train.hip, csrc/h12_rnd.hip,
 * csrc/h12_optim.hip, csrc/h12_ppo_head.hip).
 *
 * The CleanRL PPO of the CaT tasks (h12env/cleanrl.py) calls two pieces of per-step / per-iteration work that
 * are launch-bound in torch: the running mean/variance normaliser and the soft-termination GAE.  The third piece,
 * further down, is the policy's forward itself (h12env/policy.py): normaliser and every layer in one launch.  The
 * rsl_rl-style PPO (h12env/ppo.py) uses h12learn_mirror_rows for its mirror-symmetry augmentation and, opt-in,
 * h12learn_ppo_head for its loss head (at the end of this header).
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

/* Mirror-symmetry map of observation / action rows (h12env/symmetry.py), fused with the minibatch gather and the
 * concatenation of rsl_rl's data augmentation, in one launch:
 *   out[r, j] = (flip[j] ? -x : x)[row(r), src[j]],  row(r) = idx ? idx[r] : r,  r < n, j < d.
 * x is [n_src_rows][d], table[d] holds src | flip << 31, idx (null, or n int64 entries) selects the source rows.
 * both != 0: out has 2n rows, rows [0, n) the gathered originals, rows [n, 2n) their mirrors (one read of each source
 * row); both == 0: out has the n mirrored rows.  out must not overlap x.  The values move as 32-bit words and the sign
 * is an XOR of bit 31, so NaN, +-inf and -0.0 pass bit for bit.  An idx entry outside [0, n_src_rows) is clamped into
 * it and a src outside [0, d) to d - 1: nothing outside x is read.  Without idx, n <= n_src_rows.  n == 0 launches
 * nothing. */
int h12learn_mirror_rows(const float* x, long long n_src_rows, const long long* idx, long long n, int d,
                         const int* table /* src | flip << 31 */, int both, float* out, void* stream);

/* ---- fused policy MLP forward (csrc/h12_policy.hip): input normaliser + every Linear/ELU layer of up to
 * H12LEARN_MLP_MAX_NETS networks over one shared input, in one launch, in exact fp32 (f32-input MFMA). */
#define H12LEARN_MLP_MAX_NETS 4
#define H12LEARN_MLP_MAX_LAYERS 8

#define H12LEARN_MLP_NORM_NONE 0 /* x as it is */
#define H12LEARN_MLP_NORM_VAR 1  /* (x - mean) / sqrt(scale + eps), scale = variance: cleanrl.RunningMeanStd */
#define H12LEARN_MLP_NORM_STD 2  /* (x - mean) / (scale + eps), scale = std: ppo.EmpiricalNormalization */

/* One network: n_layers Linear layers, ELU (alpha = 1) between them, the last one linear.  dims[0] is the input
 * width (== desc.d_in), dims[l + 1] the output width of layer l.  W[l] is the torch weight [dims[l+1]][dims[l]]
 * row-major contiguous fp32, b[l] the bias [dims[l+1]]; device pointers, read only. */
typedef struct h12learn_mlp_net {
  int n_layers;
  int dims[H12LEARN_MLP_MAX_LAYERS + 1];
  const float* W[H12LEARN_MLP_MAX_LAYERS];
  const float* b[H12LEARN_MLP_MAX_LAYERS];
} h12learn_mlp_net;

/* norm_mean[d_in], norm_scale[d_in]: fp32 device vectors, read only, ignored with H12LEARN_MLP_NORM_NONE.  The
 * division is a true (correctly rounded) division, as in torch. */
typedef struct h12learn_mlp_desc {
  int n_nets;
  int d_in;
  int norm_kind;
  float norm_eps;
  const float* norm_mean;
  const float* norm_scale;
  h12learn_mlp_net nets[H12LEARN_MLP_MAX_NETS];
} h12learn_mlp_desc;

/* The largest supported width of any layer, the input included. */
int h12learn_mlp_max_width(void);

/* Bytes of the packed weights of desc (shapes only: the pointers are not read); 0 with h12learn_last_error set when
 * the shapes are invalid. */
size_t h12learn_mlp_packed_bytes(const h12learn_mlp_desc* desc);

/* One launch: copies every W / b of desc into the tiled, zero-padded layout the forward reads (packed: 16-byte
 * aligned, h12learn_mlp_packed_bytes).  Run it after every change of the weights; it may be captured. */
int h12learn_mlp_pack(const h12learn_mlp_desc* desc, float* packed, void* stream);

/* One launch: y[i] ([n][d_out_i] fp32) = network i of desc applied to the normalised x ([n][d_in] contiguous fp32),
 * from the weights in packed (the W / b pointers of desc are not read).  An output element is
 * bias + sum_k h[k] W[j][k] accumulated as one fmaf chain whose k order depends on the layer's input width alone, so
 * a row's result does not depend on n, on its position or on the other rows.  Networks wider than 512 need more
 * than 64 KiB of LDS: the first such call of a process raises the kernel's limit, and fails with H12LEARN_E_HIP
 * ("must be made outside a stream capture (warm up first)") when its stream is capturing. */
int h12learn_mlp_forward(const h12learn_mlp_desc* desc, const float* packed, const float* x, long long n,
                         float* const* y, void* stream);

/* ---- training side of the fused policy MLP (csrc/h12_policy_train.hip): forward that keeps the hidden activations,
 * and the backward through every layer, one launch each, on the same exact-fp32 MFMA design.  ONE network per call
 * (desc.n_nets == 1) and H12LEARN_MLP_NORM_NONE only; every width, the input included, at most
 * h12learn_mlp_train_max_width().  The weight gradients dW_l = dZ_l^T H_{l-1} are left to the caller's GEMM library.
 * Blocks own h12learn_mlp_train_rows() rows; more than 64 KiB of LDS are needed for wide networks, and the first such
 * call of either kernel raises its limit: that call fails with H12LEARN_E_HIP when its stream is capturing. */

/* Rows of a block of the training kernels (the row tile R); a query so tests can place n at R-1, R, R+1, 2R+1. */
int h12learn_mlp_train_rows(void);

/* The largest supported width of any layer of the training kernels, the input included (>= 512). */
int h12learn_mlp_train_max_width(void);

/* Bytes of the transposed packed weights of desc (shapes only); 0 with h12learn_last_error set when invalid. */
size_t h12learn_mlp_packed_t_bytes(const h12learn_mlp_desc* desc);

/* One launch: every W of desc into the tiled, zero-padded layout of h12learn_mlp_pack taken over W^T (per layer
 * [16-column tile of the layer's INPUT][k-group of its OUTPUT][lane][4], no bias): the B operand of the dgrad
 * dH = dZ W.  packed_t: 16-byte aligned, h12learn_mlp_packed_t_bytes.  Run after every change of the weights; it may
 * be captured.  The b pointers of desc are not read. */
int h12learn_mlp_pack_t(const h12learn_mlp_desc* desc, float* packed_t, void* stream);

/* One launch: y ([n][d_out]) = the network of desc on x ([n][d_in] contiguous fp32) from packed (h12learn_mlp_pack of
 * the same desc), bit-identical to h12learn_mlp_forward, and h[l] ([n][dims[l+1]], l < n_layers - 1) = the ELU output
 * of hidden layer l.  h may be null for a single layer. */
int h12learn_mlp_forward_train(const h12learn_mlp_desc* desc, const float* packed, const float* x, long long n,
                               float* y, float* const* h, void* stream);

/* Bytes of workspace h12learn_mlp_backward needs for n rows (the per-block bias-gradient partials); it needs no
 * initialisation.  0 with h12learn_last_error set when desc or n is invalid. */
size_t h12learn_mlp_backward_workspace_bytes(const h12learn_mlp_desc* desc, long long n);

/* Two launches.  dy is [n][d_out], h[l] the activations h12learn_mlp_forward_train saved, packed_t the transposed pack.
 * With dZ_{L-1} = dy, for l = L-2 .. 0:  dH_l = dZ_{l+1} W_{l+1},  dZ_l = dH_l * f'(h_l),  f'(h) = h > 0 ? 1 : h + 1
 * (ELU's derivative from its output).  Writes dz[l] ([n][dims[l+1]], l < L - 1), dx ([n][d_in]) = dZ_0 W_0 when dx is
 * not null, and every bias gradient db[l][j] = sum_r dZ_l[r][j] (l < L; db[L-1] sums dy).  A dZ / dx element is one
 * fmaf chain from zero whose order depends on the summed layer's width alone; db sums each block's rows in row order
 * and the blocks in block-index order (second launch), without atomics: everything is bitwise reproducible.  The W / b
 * pointers of desc are not read. */
int h12learn_mlp_backward(const h12learn_mlp_desc* desc, const float* packed_t, const float* dy,
                          const float* const* h, long long n, float* const* dz, float* const* db, float* dx,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused recurrent policy step (csrc/h12_policy_rnn.hip): input normaliser, one LSTM cell and the Linear/ELU MLP
 * that reads its hidden state, for up to H12LEARN_LSTM_MAX_NETS networks over one shared input (actor and critic of
 * rsl_rl's ActorCriticRecurrent when both read the same observation; two calls otherwise), in one launch, in exact
 * fp32 on the design of h12learn_mlp_forward.  One LSTM layer, hidden size at most h12learn_lstm_max_hidden().
 *
 * Per network, with torch.nn.LSTM's layer-0 parameters and gate order (i, f, g, o):
 *     z  = [x | h] [W_ih | W_hh]^T + (b_ih + b_hh)        the bias is summed once, at pack time
 *     i, f, o = sigmoid(z_i), sigmoid(z_f), sigmoid(z_o);  g = tanh(z_g)
 *     c' = f * c + i * g;   h' = o * tanh(c');   y = MLP(h')
 * sigmoid(z) = 1 / (1 + expf(-z)) with a true division.  A z element is one fmaf chain from the bias over x's columns
 * (padded to 16), then h's: its order depends on (d_in, hidden) alone, and that of a y element on the MLP's widths, never
 * on n, on the row's position or on the grid.  The gates stay in LDS. */
#define H12LEARN_LSTM_MAX_NETS 2

/* One cell's parameters: w_ih [4 hidden][d_in], w_hh [4 hidden][hidden], b_ih and b_hh [4 hidden]; row-major contiguous
 * fp32 device pointers, read only by h12learn_lstm_pack. */
typedef struct h12learn_lstm_cell {
  const float* w_ih;
  const float* w_hh;
  const float* b_ih;
  const float* b_hh;
} h12learn_lstm_cell;

/* d_in: the width of x; the norm_* fields are the input normaliser of h12learn_mlp_desc, applied to x.  mlp holds the
 * networks that follow the cells: mlp.n_nets (1..H12LEARN_LSTM_MAX_NETS) is the number of networks of the call,
 * mlp.d_in == hidden, mlp.norm_kind == H12LEARN_MLP_NORM_NONE; network i reads cell i's h'. */
typedef struct h12learn_lstm_desc {
  int d_in;
  int hidden;
  int norm_kind;
  float norm_eps;
  const float* norm_mean;
  const float* norm_scale;
  h12learn_lstm_cell cells[H12LEARN_LSTM_MAX_NETS];
  h12learn_mlp_desc mlp;
} h12learn_lstm_desc;

/* The tensors of one step: x [n][d_in], shared by the networks; reset (null, or n bytes): a non-zero byte makes that
 * row read h = c = 0; per network h_in, c_in, h_out, c_out [n][hidden] and y [n][d_out].  A block owns its 16 rows
 * completely and reads its rows of h and c before it writes any of them: h_out == h_in and c_out == c_in (in place) is
 * legal.  No other overlap between an output and an input, or between two networks' states, is. */
typedef struct h12learn_lstm_io {
  const float* x;
  const unsigned char* reset;
  long long n;
  const float* h_in[H12LEARN_LSTM_MAX_NETS];
  const float* c_in[H12LEARN_LSTM_MAX_NETS];
  float* h_out[H12LEARN_LSTM_MAX_NETS];
  float* c_out[H12LEARN_LSTM_MAX_NETS];
  float* y[H12LEARN_LSTM_MAX_NETS];
} h12learn_lstm_io;

/* The largest supported hidden size (4 * hidden is a layer width of the MLP core). */
int h12learn_lstm_max_hidden(void);

/* Bytes of the packed weights of desc (shapes only); 0 with h12learn_last_error set when the shapes are invalid. */
size_t h12learn_lstm_packed_bytes(const h12learn_lstm_desc* desc);

/* One launch: per network the matrix [W_ih | W_hh] in the tiled, zero-padded layout of h12learn_mlp_pack (the K axis
 * padded per segment: x to 16, then h to 16), the bias b_ih + b_hh, then the network's MLP layers as h12learn_mlp_pack
 * packs them.  packed: 16-byte aligned, h12learn_lstm_packed_bytes.  Run it after every change of the weights; it may
 * be captured. */
int h12learn_lstm_pack(const h12learn_lstm_desc* desc, float* packed, void* stream);

/* One launch, grid (row tiles of 16, networks), from the weights in packed (the parameter pointers of desc are not
 * read).  The real shape (450 inputs, hidden 256) needs more than 64 KiB of LDS: the first such call of a process
 * raises the kernel's limit, and fails with H12LEARN_E_HIP ("must be made outside a stream capture (warm up first)")
 * when its stream is capturing. */
int h12learn_lstm_step(const h12learn_lstm_desc* desc, const float* packed, const h12learn_lstm_io* io, void* stream);

/* ---- the recurrent policy's update (csrc/h12_policy_rnn_train.hip): one LSTM layer run over a whole rollout
 * [T][n] with the state zeroed after a done, and its back-propagation through time, one launch each, for up to
 * H12LEARN_LSTM_MAX_NETS networks (the actor's and the critic's memories) over the same T, n, hidden size and dones.
 * Exact fp32 on the design of h12learn_mlp_forward; hidden size 1 .. h12learn_lstm_max_hidden(), 1 <= T <= 4096, n >= 1.
 *
 * The caller's GEMM library makes the input projection zx = x W_ih^T + b_ih + b_hh ([T][n][4 hidden]) and, from dz, the
 * weight gradients (dW_ih = dz^T x, dW_hh = dz^T h_prev with h_prev the reset-masked, shifted h_seq, db = sum dz).
 *
 * Forward, gate order i, f, g, o (torch's), for t = 0 .. T-1:
 *     reset(t, r) = t >= 1 && dones[t-1][r] != 0         dones[T-1] is never read; t = 0 always reads h0 / c0
 *     h_prev, c_prev = 0 where reset, else h_seq[t-1], c_seq[t-1] (h0, c0 at t = 0)
 *     z = zx[t] + h_prev W_hh^T                           a bias-free k chain over h_prev from zero, THEN + zx
 *     i, f, o = sigmoid(z_i), sigmoid(z_f), sigmoid(z_o);  g = tanh(z_g)         (1 / (1 + expf(-z)), true division)
 *     c_seq[t] = f c_prev + i g;   h_seq[t] = o tanh(c_seq[t]);   gates[t] = (i, f, g, o)   the activated gates
 * Backward, for t = T-1 .. 0, the carries dh_c, dc_c starting at zero:
 *     dh = dh_seq[t] + dh_c;   do = dh tanh(c_t);   dc = dc_c + dh o (1 - tanh(c_t)^2)
 *     di = dc g;  dg = dc i;  df = dc c_prev
 *     dz[t] = (di i (1 - i), df f (1 - f), dg (1 - g^2), do o (1 - o))
 *     dc_c = dc f;   dh_c = dz[t] W_hh                    a k chain over the 4 hidden columns from zero
 *     where reset(t, r): dh_c = dc_c = 0                  a reset row sends nothing further back
 * dh0 / dc0 (each may be null) receive the carries after t = 0.
 *
 * A block owns 16 rows for all T steps and the rows are independent: an output element's summation order depends on
 * the hidden size alone, never on n, T, the row's place in its tile or the grid; no atomics; every output is bitwise
 * reproducible.  All tensors contiguous; no output may overlap an input.  A hidden size above 160 needs more than
 * 64 KiB of LDS: the first such call of each kernel raises its limit, and fails with H12LEARN_E_HIP ("must be made
 * outside a stream capture (warm up first)") when its stream is capturing. */
typedef struct h12learn_lstm_seq_desc {
  int n_nets; /* 1 .. H12LEARN_LSTM_MAX_NETS */
  int hidden;
  const float* w_hh[H12LEARN_LSTM_MAX_NETS]; /* [4 hidden][hidden], read only by h12learn_lstm_seq_pack */
} h12learn_lstm_seq_desc;

typedef struct h12learn_lstm_seq_io {
  int T;
  int reserved; /* 0 */
  long long n;
  const unsigned char* dones;                 /* [T][n] bytes, shared by the networks */
  const float* zx[H12LEARN_LSTM_MAX_NETS];    /* [T][n][4 hidden] */
  const float* h0[H12LEARN_LSTM_MAX_NETS];    /* [n][hidden] */
  const float* c0[H12LEARN_LSTM_MAX_NETS];    /* [n][hidden] */
  float* h_seq[H12LEARN_LSTM_MAX_NETS];       /* [T][n][hidden] */
  float* c_seq[H12LEARN_LSTM_MAX_NETS];       /* [T][n][hidden], kept for the backward */
  float* gates[H12LEARN_LSTM_MAX_NETS];       /* [T][n][4 hidden], kept for the backward */
} h12learn_lstm_seq_io;

typedef struct h12learn_lstm_seq_grad_io {
  int T;
  int reserved; /* 0 */
  long long n;
  const unsigned char* dones;                  /* [T][n] bytes */
  const float* dh_seq[H12LEARN_LSTM_MAX_NETS]; /* [T][n][hidden] */
  const float* gates[H12LEARN_LSTM_MAX_NETS];  /* as the forward wrote them */
  const float* c_seq[H12LEARN_LSTM_MAX_NETS];
  const float* c0[H12LEARN_LSTM_MAX_NETS];
  float* dz[H12LEARN_LSTM_MAX_NETS];           /* [T][n][4 hidden] */
  float* dh0[H12LEARN_LSTM_MAX_NETS];          /* [n][hidden], or null */
  float* dc0[H12LEARN_LSTM_MAX_NETS];          /* [n][hidden], or null */
} h12learn_lstm_seq_grad_io;

/* Bytes of the pack of desc (shapes only): per network W_hh in the layout of h12learn_mlp_pack (K = hidden padded to 16,
 * 4 hidden output rows, no bias), then W_hh^T as h12learn_mlp_pack_t lays a layer out (K = 4 hidden padded to 16, hidden
 * output rows).  0 with h12learn_last_error set when the shapes are invalid. */
size_t h12learn_lstm_seq_packed_bytes(const h12learn_lstm_seq_desc* desc);

/* One launch: both operands of every network into packed (16-byte aligned, h12learn_lstm_seq_packed_bytes).  Run it
 * after every change of the weights; it may be captured. */
int h12learn_lstm_seq_pack(const h12learn_lstm_seq_desc* desc, float* packed, void* stream);

/* One launch each, grid (row tiles of 16, networks), from the weights in packed (desc.w_hh is not read). */
int h12learn_lstm_seq_forward(const h12learn_lstm_seq_desc* desc, const float* packed, const h12learn_lstm_seq_io* io,
                              void* stream);
int h12learn_lstm_seq_backward(const h12learn_lstm_seq_desc* desc, const float* packed,
                               const h12learn_lstm_seq_grad_io* io, void* stream);

/* ---- Random Network Distillation's per-env-step work (csrc/h12_rnd.hip; h12env/rnd.py): the
 * intrinsic reward of one collection step in two launches.
 *
 * h12learn_rnd_reward, one launch.  desc.n_nets == 2: nets[0] is the predictor, nets[1] the target, both over the
 * normalised x ([n][d_in] contiguous fp32; norm_* as for h12learn_mlp_forward); their depths and hidden widths may
 * differ, their last widths are equal.  packed is h12learn_mlp_pack of the same desc (the W / b pointers are not read):
 * repack after every change of the predictor.  Per row r:
 *     err[r] = sqrtf(sum_j (target(xn_r)[j] - predictor(xn_r)[j])^2)
 * Both embeddings come from the tile routines of h12learn_mlp_forward and carry its bits; the squares are summed in a
 * fixed order (the 16 columns of a tile by an xor butterfly, a wave's tiles in order, the four waves in order) that
 * depends on the output width alone, never on n or the grid.  xn (may be null) receives the normalised rows [n][d_in];
 * emb (may be null; a test hook) is float*[2] and receives the predictor's and the target's embedding [n][d_out].
 * Every width up to h12learn_mlp_max_width(); a block holds the input tile, two hidden images and the embedding, 16 rows
 * each, in LDS, and widths whose images exceed a CU's 160 KiB are H12LEARN_E_ARG.  More than 64 KiB: the first such
 * call raises the kernel's limit and fails with H12LEARN_E_HIP when its stream is capturing. */
int h12learn_rnd_reward(const h12learn_mlp_desc* desc, const float* packed, const float* x, long long n, float* err,
                        float* xn, float* const* emb, void* stream);

/* h12learn_rnd_finish, one launch of one block.  With normalize != 0 (rnd.EmpiricalDiscountedVariationNormalization):
 *     avg[i]  = *first ? err[i] : avg[i] * gamma + err[i]          separately rounded; *first is then set to 0
 *     while *count < until: the scalar statistics take the batch mean and population variance of avg by
 *         ppo.EmpiricalNormalization's rule (count += n; rate = n / count; delta = mean_x - mean; mean += rate delta;
 *         var += rate (var_x - var + delta (mean_x - mean)); std = sqrt(var))
 *     v[i]    = *std > 0 ? err[i] / *std : err[i]                  with the statistics just updated
 * and v = err otherwise (the statistics pointers are then not read).  Then, separately rounded,
 *     intrinsic[i] = v[i] * *weight;   total[i] = ext_reward[i] + intrinsic[i].
 * The sums are fp32: a thread folds its elements in index order, a wave its lanes by an xor butterfly, the block its
 * waves in order.  The same inputs give the same bits; n >= 1.  intrinsic / total may alias nothing else. */
typedef struct h12learn_rnd_finish_args {
  long long n;
  int normalize;
  float gamma;
  long long until;
  const float* err;        /* [n] */
  const float* ext_reward; /* [n] */
  const float* weight;     /* device scalar */
  float* avg;              /* [n] */
  float* mean;             /* device scalars */
  float* var;
  float* std;
  long long* count;
  int* first;
  float* intrinsic;        /* [n] */
  float* total;            /* [n] */
} h12learn_rnd_finish_args;

int h12learn_rnd_finish(const h12learn_rnd_finish_args* args, void* stream);

/* ---- fused optimiser step (csrc/h12_optim.hip; h12env/optim.py): the global gradient-norm clip
 * of nn.utils.clip_grad_norm_ and the Adam or RAdam update of every parameter tensor, in two launches.
 *
 * Tensors.  n_tensors >= 1 contiguous fp32 tensors of numel[t] >= 1 elements, any 4-byte alignment: the parameter p[t],
 * its gradient g[t] (read only: it is NOT rescaled in memory), the moments exp_avg[t] and exp_avg_sq[t], and step[t], a
 * device fp32 scalar holding the number of steps taken so far, as torch's optimisers keep it.  p, g, exp_avg, exp_avg_sq,
 * step and numel are HOST arrays of n_tensors entries; the device pointers travel in the kernels' arguments, so nothing
 * is copied to the device and a captured step replays the addresses it saw.  No tensor may overlap another.
 *
 * Launch 1.  A block owns one chunk of h12learn_optim_chunk() elements of one tensor and writes the fp64 sum of g^2 over
 * it (products and sums in fp64: a thread's elements in index order, a wave's lanes by an xor butterfly, the waves in
 * order) to the workspace; one thread per tensor writes step[t] += 1.  It runs without a clip too.
 * Launch 2.  Every block adds all partial sums in block-index order, h12learn_optim_fold() at a time through LDS, to S,
 * and forms in double
 *     norm = sqrt(S);   coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1          (clip_grad_norm_'s)
 *     s = step[t] (after launch 1);   lr = lr_dev ? *lr_dev : lr
 *     bc1 = 1 - beta1^s;   bc2 = 1 - beta2^s
 *     rho_inf = 2 / (1 - beta2) - 1;   rho_t = rho_inf - 2 s beta2^s / bc2
 *     rect = sqrt((rho_t - 4) (rho_t - 2) rho_inf / ((rho_inf - 4) (rho_inf - 2) rho_t))
 * Each of coef, 1 - beta1, beta2, 1 - beta2, eps, sqrt(bc2), -(lr / bc1), bc1, lr and rect is narrowed to fp32 once.  Then
 * per element, in separately rounded fp32 operations (no contraction; sqrt and / correctly rounded), the expressions of
 * torch 2.10's _single_tensor_adam / _single_tensor_radam in their non-capturable branches (Python-float scalars) with
 * weight_decay = 0, no amsgrad, maximize = False:
 *     g' = g * coef
 *     m  = m + (g' - m) * (1 - beta1)                                     exp_avg.lerp_(grad, 1 - beta1)
 *     v  = v * beta2;   v = v + (1 - beta2) * (g' * g')                   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, ..)
 *   H12LEARN_OPTIM_ADAM
 *     p  = p + (-(lr / bc1)) * (m / (sqrt(v) / sqrt(bc2) + eps))          param.addcdiv_(exp_avg, denom, value=-step_size)
 *   H12LEARN_OPTIM_RADAM
 *     u  = (m / bc1) * lr
 *     rho_t > 5 (compared in double):  u = (u * ((1 / (sqrt(v) + eps)) * sqrt(bc2))) * rect
 *     p  = p - u
 * Block 0 writes (float)norm to grad_norm when it is not null.  rho_t comes from the step count in double: at
 * beta2 = 0.999 it is 4.9960 at step 5 and 5.9942 at step 6, so rectification starts at step 6, as in torch's default
 * (non-capturable) RAdam; an fp32 rho_t is off by 1 % of (rho_t - 4) there.
 *
 * Vector (16-byte) accesses where p, g, exp_avg and exp_avg_sq of a tensor are all 16-byte aligned, element accesses
 * otherwise; which thread owns which element is the same on both paths, so every sum's order, and every output bit,
 * depends on the tensor sizes alone.  More than h12learn_optim_max_tensors() tensors: further launches of each kernel
 * (all of launch 1 first); the norm is over all tensors.  No atomics, nothing to initialise, every output bitwise
 * reproducible.  Inputs are assumed finite. */
#define H12LEARN_OPTIM_ADAM 0
#define H12LEARN_OPTIM_RADAM 1

typedef struct h12learn_optim_args {
  int rule;      /* H12LEARN_OPTIM_* */
  int n_tensors; /* >= 1 */
  double beta1;  /* 0 <= beta < 1 */
  double beta2;
  double eps;      /* > 0 */
  double max_norm; /* <= 0: no clip */
  double lr;       /* >= 0; read when lr_dev is null */
  const float* lr_dev; /* device scalar, or null */
  float* const* p;           /* host arrays of n_tensors device pointers */
  const float* const* g;
  float* const* exp_avg;
  float* const* exp_avg_sq;
  float* const* step;        /* device fp32 scalars */
  const long long* numel;    /* host array */
  float* grad_norm; /* device scalar, or null */
  void* workspace;  /* 8-byte aligned, h12learn_optim_workspace_bytes(numel, n_tensors) */
  size_t workspace_bytes;
} h12learn_optim_args;

/* Elements of a block (the chunk C); a query so tests can place numel at C-1, C, C+1, 2C+1. */
int h12learn_optim_chunk(void);

/* Tensors one launch's table holds (K); K + 1 tensors take two launches of each kernel. */
int h12learn_optim_max_tensors(void);

/* Partial sums launch 2 stages at a time (F); F + 1 blocks take two rounds of its fold. */
int h12learn_optim_fold(void);

/* Bytes of workspace: one fp64 partial sum per block, sum_t ceil(numel[t] / C) of them.  0 with h12learn_last_error set
 * when n_tensors or a numel is invalid. */
size_t h12learn_optim_workspace_bytes(const long long* numel, int n_tensors);

/* Two launches (norm, apply) for up to K tensors.  Every field is validated before any HIP call. */
int h12learn_optim_step(const h12learn_optim_args* args, void* stream);

/* ---- fused PPO loss head (csrc/h12_ppo_head.hip): everything PPO._minibatch (h12env/ppo.py) computes between the
 * networks' outputs and loss.backward(), in two launches: the minibatch gathers of the per-sample tensors, the Gaussian
 * log-probability and entropy, the KL of the adaptive schedule, the clipped surrogate, the (clipped) value loss, the
 * weighted sum, and the gradients of
 *     loss = surrogate + value_loss_coef * value_loss - entropy_coef * entropy
 * with respect to the actor's mean, the critic's value and the std parameter, the 1/m and 1/B means folded in.
 *
 * Rows.  m rows of network outputs; B = m (plain) or B = m / 2 (data augmentation: rows [B, 2B) are the mirrored
 * samples).  Row r reads the rollout's per-sample tensors at source row k = idx[r < B ? r : r - B] (idx null: k is that
 * row number itself, n_src >= B); an entry outside [0, n_src) is clamped into it, so nothing outside the sources is
 * read.  actions is [n_src][A] read at row k, or, with actions_direct != 0, [m][A] read at row r (the augmented
 * actions arrive gathered and mirrored).  The KL mean and the entropy mean run over rows [0, B).
 *
 * Per row, with sigma[a] = std_param[a] (H12LEARN_PPO_STD_SCALAR) or exp(std_param[a]) (H12LEARN_PPO_STD_LOG), in fp32:
 *     log_prob = sum_a  -(actions - mean)^2 / (2 sigma^2) - log(sigma) - log(sqrt(2 pi))
 *     ratio    = exp(log_prob - old_log_prob)
 *     s1 = -adv * ratio,  s2 = -adv * clamp(ratio, lo, hi),  lo = 1 - clip_param, hi = 1 + clip_param
 *     surrogate row = max(s1, s2)
 *     e1 = value - returns,  e2 = (target + clamp(value - target, -clip_param, clip_param)) - returns
 *     value row = max(e1^2, e2^2)                (use_clipped_value_loss == 0: (returns - value)^2)
 *     kl row (r < B) = sum_a  log(sigma / old_sigma + 1e-5) + (old_sigma^2 + (old_mu - mean)^2) / (2 sigma^2) - 0.5
 *     entropy row = sum_a  0.5 + 0.5 log(2 pi) + log(sigma)       (the same for every row)
 * The bounds lo, hi, +-clip_param and the two coefficients are formed in double and narrowed once, as torch narrows the
 * Python scalars.
 *
 * Tie / boundary rule: what torch autograd gives for that expression.  clamp passes the gradient on its CLOSED
 * interval; max(x, y) gives x the weight [x > y] + [x == y] / 2 and y the weight [x < y] + [x == y] / 2.  Hence
 *     d surrogate row / d ratio = -adv * (w1 + inside * w2),   inside = lo <= ratio <= hi,
 *         w1 = [s1 > s2] + [s1 == s2] / 2,  w2 = [s1 < s2] + [s1 == s2] / 2:
 *       inside the clip range (boundaries included) s1 and s2 are the same number, the halves add up: -adv, the full
 *       gradient; outside it the clamp passes nothing: -adv where the unclipped term is the larger, 0 where the clipped
 *       one is, -adv / 2 on an exact tie (adv == 0);
 *     d value row / d value = 2 e1 v1 + inside_v * 2 e2 v2,   inside_v = -clip_param <= value - target <= clip_param,
 *         v1, v2 the weights of e1^2 against e2^2 as above (inside the range e2 is e1 up to the rounding of
 *         target + (value - target), so either operand can be the larger and both carry the gradient).
 * The comparisons are made on separately rounded fp32 operations (no contraction), the ones torch makes.
 *
 * Outputs: d_mean [m][A], d_value [m], d_param [A] (the gradient of std, or of log_std), out[5] = surrogate loss, value
 * loss, entropy mean, KL mean, total loss.  Optional, in the second launch after the KL mean is known:
 *   lr           not null: rsl_rl's adaptive schedule on the device scalar, in place: lr / 1.5 (floor 1e-5) when
 *                kl > 2 desired_kl; lr * 1.5 (ceiling 1e-2) when 0 < kl < desired_kl / 2; unchanged otherwise.
 *   stats_accum  not null: stats_accum[0..2] += value loss, surrogate loss, entropy mean.
 *
 * Reductions without atomics: the row kernel writes, per block of h12learn_ppo_head_rows() rows, the partial sums of
 * the surrogate, value and KL rows and of d_param to the workspace (rows in row order), the fold adds the blocks in
 * block-index order: every output is bitwise reproducible from run to run.  The terms are fp32, the accumulators and
 * the partial sums fp64, so a sum carries the rounding of its terms only.  The workspace needs no initialisation.
 * Inputs are assumed finite (the library's device code is built with -ffinite-math-only). */
#define H12LEARN_PPO_STD_SCALAR 0
#define H12LEARN_PPO_STD_LOG 1

typedef struct h12learn_ppo_head_args {
  long long m;     /* rows of mean / value */
  long long B;     /* minibatch rows: m, or m / 2 under data augmentation */
  long long n_src; /* rows of the rollout tensors */
  int A;           /* actions, 1 .. h12learn_ppo_head_max_actions() */
  int std_kind;    /* H12LEARN_PPO_STD_* */
  int actions_direct;
  int use_clipped_value_loss;
  const float* mean;      /* [m][A] */
  const float* value;     /* [m] */
  const float* std_param; /* [A] */
  const long long* idx;   /* [B] or null */
  const float* old_log_prob;  /* [n_src] */
  const float* advantages;    /* [n_src] */
  const float* returns;       /* [n_src] */
  const float* target_values; /* [n_src] */
  const float* old_mu;        /* [n_src][A] */
  const float* old_sigma;     /* [n_src][A] */
  const float* actions;       /* [n_src][A], or [m][A] with actions_direct */
  double clip_param;
  double value_loss_coef;
  double entropy_coef;
  double desired_kl; /* read only when lr is not null; must then be > 0 */
  float* d_mean;     /* [m][A] */
  float* d_value;    /* [m] */
  float* d_param;    /* [A] */
  float* out;        /* [5] */
  float* lr;          /* device scalar, or null */
  float* stats_accum; /* [3], or null */
  void* workspace;    /* 8-byte aligned, h12learn_ppo_head_workspace_bytes(m, A) */
  size_t workspace_bytes;
} h12learn_ppo_head_args;

/* Rows of a block of the row kernel (the row tile R); a query so tests can place m at R-1, R, R+1, 2R+1. */
int h12learn_ppo_head_rows(void);

/* The largest supported number of actions (>= 32). */
int h12learn_ppo_head_max_actions(void);

/* Bytes of workspace for m rows of A actions: ceil(m / R) blocks of 3 + A fp64 partial sums.  0 with
 * h12learn_last_error set when m or A is invalid. */
size_t h12learn_ppo_head_workspace_bytes(long long m, int A);

/* Two launches (row kernel, fold).  No output may overlap an input. */
int h12learn_ppo_head(const h12learn_ppo_head_args* args, void* stream);

const char* h12learn_last_error(void);

/* ---- fused CleanRL loss head (csrc/h12_ppo_head.hip): the block of cleanrl.PPO (h12env/cleanrl.py) from `logratio` to
 * `loss`, with the minibatch gathers, the per-minibatch advantage normalisation, the de-normalisation of the critic's
 * output through value_rms (update=False) and the gradients of
 *     loss = mean(pg) - ent_coef * entropy + vf_coef * 0.5 * mean(v)
 * with respect to the actor's mean, the critic's value and actor_logstd, in three launches (two without norm_adv).
 *
 * Rows.  m rows of network outputs; row r reads the rollout's per-sample tensors at source row k = idx[r] (idx null:
 * k = r, n_src >= m); an entry outside [0, n_src) is clamped into it.  Per row, in fp32 on separately rounded operations:
 *     log_prob = sum_a  -(actions[k][a] - mean[r][a])^2 / (2 sigma^2) - logstd[a] - log(sqrt(2 pi)),  sigma = exp(logstd)
 *     ratio    = exp(log_prob - old_log_prob[k])
 *     clip row = |ratio - 1| > clip_coef                                   (strict)
 *     adv      = advantages[k];  norm_adv: (adv - mean_mb) / (std_mb + 1e-8), mean_mb and std_mb (correction 1) over
 *                the m gathered advantages
 *     pg row   = max(-adv * ratio, -adv * clamp(ratio, 1 - clip_coef, 1 + clip_coef))
 *     nv       = (value[r] - *value_mean) / sqrt(*value_var + value_eps)
 *     v row    = clip_vloss ? max((nv - returns_n[k])^2,
 *                                 (values_n[k] + clamp(nv - values_n[k], -clip_coef, clip_coef) - returns_n[k])^2)
 *                           : (nv - returns_n[k])^2
 *     entropy  = sum_a  0.5 + 0.5 log(2 pi) + logstd[a]                    (the same for every row: computed once)
 * The bounds 1 -+ clip_coef, +-clip_coef, the two coefficients and value_eps are formed in double and narrowed once.
 * Tie / boundary rule: that of h12learn_ppo_head above (closed-interval clamp, half weights on an exact max tie).
 *
 * Advantage statistics: each block of h12learn_cleanrl_head_rows() rows writes the shifted two-pass (count, mean, M2) of
 * its rows' gathered advantages in fp64; every block of the row kernel merges these partials itself in block-index order
 * (Chan's update, fp64) and narrows mean and sqrt(M2 / (m - 1)) once.  No E[x^2] - mean^2 anywhere.
 *
 * Outputs: d_mean [m][A], d_value [m] (through the de-normalisation: / sqrt(*value_var + value_eps)), d_logstd [A],
 * out[5] = pg loss, entropy, v loss (the 0.5 included), total loss, clip fraction.  stats_accum not null:
 * stats_accum[0..4] += out[0..4].
 *
 * Reductions as for h12learn_ppo_head: fp32 terms, fp64 row-order block partials, an in-order fold; no atomics, nothing
 * to initialise, every output bitwise reproducible from run to run.  Inputs are assumed finite. */
typedef struct h12learn_cleanrl_head_args {
  long long m;     /* rows of mean / value */
  long long n_src; /* rows of the rollout tensors */
  int A;           /* actions, 1 .. h12learn_ppo_head_max_actions() */
  int norm_adv;    /* needs m >= 2 (the std of one element is NaN) */
  int clip_vloss;
  int reserved;    /* 0 */
  const float* mean;         /* [m][A] */
  const float* value;        /* [m] */
  const float* logstd;       /* [A] */
  const long long* idx;      /* [m] or null */
  const float* old_log_prob; /* [n_src] */
  const float* advantages;   /* [n_src] */
  const float* returns_n;    /* [n_src], normalised by value_rms */
  const float* values_n;     /* [n_src], normalised by value_rms */
  const float* actions;      /* [n_src][A] */
  const float* value_mean;   /* device scalar: value_rms.running_mean */
  const float* value_var;    /* device scalar: value_rms.running_var */
  double value_eps;          /* value_rms.epsilon, >= 0 */
  double clip_coef;          /* >= 0 */
  double ent_coef;
  double vf_coef;
  float* d_mean;      /* [m][A] */
  float* d_value;     /* [m] */
  float* d_logstd;    /* [A] */
  float* out;         /* [5] */
  float* stats_accum; /* [5], or null */
  void* workspace;    /* 8-byte aligned, h12learn_cleanrl_head_workspace_bytes(m, A) */
  size_t workspace_bytes;
} h12learn_cleanrl_head_args;

/* Rows of a block (the row tile R of both the advantage kernel and the row kernel). */
int h12learn_cleanrl_head_rows(void);

/* Bytes of workspace for m rows of A actions: ceil(m / R) blocks of 3 (count, mean, M2) + 3 + A fp64 partials.  0 with
 * h12learn_last_error set when m or A is invalid. */
size_t h12learn_cleanrl_head_workspace_bytes(long long m, int A);

/* Three launches (advantage partials, rows, fold; without norm_adv the first is left out).  No output may overlap an
 * input. */
int h12learn_cleanrl_head(const h12learn_cleanrl_head_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* H12LEARN_H */
