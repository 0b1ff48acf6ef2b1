/*
 * segan_hip.h — C ABI of libsegan_hip.so, the MI355X (gfx950) kernels behind the
 * SEGAN+/WSEGAN GAN training step.
 *
 * The reference (santi-pdp/segan_pytorch) has no FFI: every FLOP of its hot path is
 * an implicit ATen op dispatched by a torch.nn module.  Each entry point below
 * replaces one such implicit op (the reference call site it stands in for is cited
 * per function); the Python package `segan_pytorch_amd` binds them with ctypes (see
 * INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *  - all tensors are contiguous fp32, NCL ([batch, channel, time]) like torch;
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch's allocator);
 *    the library never allocates, frees or keeps a pointer past the call;
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it and the
 *    call returns without synchronising;
 *  - return value: 0 on success, negative on error; segan_last_error() returns a
 *    thread-local message.  Nothing throws, nothing calls exit().
 *
 * Weight tensors are [m, n, K] in both directions: Conv1d.weight = [Cout, Cin, K]
 * (m = low-rate side = Cout) and ConvTranspose1d.weight = [Cin, Cout, K] (m = Cin).
 */
#ifndef SEGAN_HIP_H
#define SEGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGAN_ABI_VERSION 17

#define SEGAN_PAD_REFLECT 0
#define SEGAN_PAD_ZERO 1

#define SEGAN_ACT_NONE 0
#define SEGAN_ACT_TANH 1

/* A logical [B, C0+C1, L] activation made of up to two channel segments, with an
 * optional per-channel transform applied while it is staged into LDS:
 *     v = x * scale[c] + shift[c];   v = v > 0 ? v : v * slope[c]
 * (each vector may be NULL = identity; c indexes the concatenated channel axis).
 * This is how PReLU (modules.py:101), BatchNorm-normalise (modules.py:100), the
 * skip scale alpha and both torch.cat's (generator.py:76,205) are folded into the
 * consumer's load instead of being materialised.
 * Alignment of p0 / p1 (each segment is contiguous [B, Ci, L]): 4 bytes wherever the source is an
 * activation that is staged sample by sample — the input of segan_conv1d_fwd and
 * segan_deconv1d_fwd and the `hi` operand of segan_wgrad, in every precision (scalar and
 * one-dword buffer loads in the fp32 kernels; the bf16 packing passes read S consecutive samples
 * through vector types declared 4-byte aligned).  16 bytes for the `lo` operand of segan_wgrad,
 * which every kernel reads four samples at a time (float4 loads, 16-byte LDS-DMA; Ls % 4 == 0
 * keeps the rows aligned): segan_wgrad returns -1 with a message for a lo pointer that is not.
 * scale / shift / slope are read element by element: 4 bytes. */
typedef struct segan_src {
  const float* p0;
  const float* p1; /* NULL when C1 == 0 */
  int32_t C0;
  int32_t C1;
  const float* scale;
  const float* shift;
  const float* slope;
} segan_src;

int segan_abi_version(void);
const char* segan_last_error(void);

/* Workgroup slots the launch planners leave free for OTHER kernels (default 0, or the environment's
 * SEGAN_RESERVED_SLOTS): the contraction kernels run persistent grids of one workgroup per resident
 * slot with equal shares of the work, so a foreign kernel that holds n slots while one is launched
 * (RCCL's channels during a data-parallel step: one 256-thread workgroup each) delays it by a
 * whole share (+25-33 %), not by n / slots.  With a reserve of n the grids are planned for n fewer
 * workgroups.  Process-wide (an atomic: safe to call while other threads launch); returns the
 * previous value.  The data-parallel path leaves it at 0 on purpose: measured with emulated 32-channel
 * collectives behind the production reducer, a static reserve costs more (+2.3 ms per
 * step while no collective is resident) than the delayed shares it avoids (+1.6 ms) — it is a knob
 * for a first multi-GPU run, not a default.  (There is no reference counterpart: the reference is
 * single-GPU, README.md:79.) */
int segan_set_reserved_slots(int n);

/* Bytes of packed-weight workspace segan_pack_weights needs for each form. */
size_t segan_packed_f_bytes(int M, int N, int S);
size_t segan_packed_t_bytes(int M, int N, int S);

/* Re-lay w[m][n][K] into the two polyphase packings the contraction kernels read
 * (either destination may be NULL).  `pad_t` is the transposed-form padding: the
 * ConvTranspose1d padding for a deconv weight (modules.py:115), 0 for a conv
 * weight (whose T form is its data gradient in padded coordinates).
 * The packed buffers are OPAQUE operands of the entry points below: consume them only through
 * segan_conv1d_fwd / segan_deconv1d_dgrad (wf) and segan_deconv1d_fwd / segan_conv1d_dgrad (wt) called
 * with the same (M, N, K, S, pad_t).  (Since ABI v12 the F packing of a K = 31 weight with an even
 * channel count N > 2 keeps, in the padding-tap row of every odd channel, the row-30 weights of its
 * even partner — the contraction kernels merge the two half-empty MFMA steps of a channel pair —
 * so wf is no longer a plain zero-padded transpose of w.) */
int segan_pack_weights(const float* w, float* wf, float* wt, int M, int N, int K, int S,
                       int pad_t, void* stream);

/* Precision of the four forward / data-gradient contractions below (`precision` argument):
 *   SEGAN_PREC_FP32   exact fp32 on v_mfma_f32_32x32x2_f32; packed weights from
 *                     segan_pack_weights (the default, and the benchmarked configuration)
 *   SEGAN_PREC_BF16   operands rounded to bf16, fp32 accumulate (BASELINE config 5)
 *   SEGAN_PREC_BF16X3 every fp32 operand split exactly into 3 bf16 planes, 6 partial products:
 *                     fp32-class accuracy on the bf16 matrix cores
 * The two bf16 modes read weights packed by segan_pack_weights_bf (planes = 1 / 3); a
 * geometry they do not cover returns -3 (unsupported) and the caller uses fp32. */
#define SEGAN_PREC_FP32 0
#define SEGAN_PREC_BF16 1
#define SEGAN_PREC_BF16X3 3
/* fp32 with BLOCKED accumulation: the contraction runs into the MFMA accumulators for 256 terms
 * at a time and the block sums are added in a second register set, so the rounding error grows
 * with sqrt(256) + sqrt(K/256) instead of sqrt(K): forward error against fp64 3e-7 instead of
 * 1.5-2.2e-6 on the deep layers (tests/diag/diag_accum.py), at two instead of three resident
 * waves per SIMD (~3 % of the contraction rate, 1.5-2.2 % of the training step).  Same packed weights as SEGAN_PREC_FP32;
 * built for stride 4, other strides run the plain kernels.  Not a mode of segan_wgrad (its
 * contractions are split into short pieces already). */
#define SEGAN_PREC_FP32_BLOCKED 4
size_t segan_packed_bf_bytes(int M, int N, int S, int tform, int planes);
int segan_pack_weights_bf(const float* w, void* out, int M, int N, int K, int S, int tform,
                          int pad_t, int planes, void* stream);

/* Scratch of the bf16 / bf16x3 forms (precision 1 / 3) of the four contraction entry points:
 * the activation operand is converted ONCE per call into bf16 planes in tile order (transform,
 * both channel segments, padding, roll and polyphase split applied), from where both MFMA operands
 * stream into LDS by LDS-DMA.  op: 0 conv forward, 1 conv data gradient, 2 deconv forward,
 * 3 deconv data gradient; N, M as in that entry point; L = length of the HIGH-rate side; pad =
 * its padL / pad argument.  Pass a buffer of at least this size as `scratch`; without one (or for
 * a geometry the bf16 kernels do not cover) the entry point returns SEGAN_EUNSUPPORTED and the
 * caller repeats the call with SEGAN_PREC_FP32 and the fp32 weight packing. */
size_t segan_bf16_scratch_bytes(int op, int B, int N, int M, int L, int K, int S, int pad, int planes);
/* Scratch of the four forward / data-gradient contractions below (`scratch`, `scratch_bytes`;
 * may be NULL / 0).  The fp32 kernels run whole rounds of equal tiles one per workgroup and cut
 * the tiles of the last, partial round along the contraction across ALL workgroups
 * (stream-K); a cut tile's pieces are written to `scratch` as accumulator slabs and summed in
 * chunk order by a second small kernel — a fixed order, so results are bit-reproducible run
 * to run (no atomics).  segan_corr_scratch_bytes() is the size that always suffices (128 MiB);
 * with less (or NULL) the launch simply stays one-tile-per-workgroup.  The scratch must not be
 * shared by launches that may run concurrently (different streams). */
size_t segan_corr_scratch_bytes(void);
/* Diagnostics (tests): how the calling thread's last fp32 forward / data-gradient contraction
 * was launched: {kernel (1 general, 2 fast), workgroups, tiles, tiles run whole, (tile, chunk)
 * units per workgroup of the stream-K part or 0, input transform mode}. */
void segan_debug_last_corr(int* out6);
/* The same for the last fp32 weight gradient: {kernel (1 general, 2 fast), tiles, contraction
 * splits, chunks per split, resident workgroups per CU assumed, hi loads per lane}. */
void segan_debug_last_wgrad(int* out6);

/* GConv1DBlock forward without norm/activation (modules.py:91-99):
 *   out[b,m,t] = bias[m] + sum_{n,k} w[m,n,k] * pad(roll(x))[b,n,S*t+k]
 * x: [B, N, L] (segan_src), out: [B, M, L/S].  mode = reflect with
 * (K/2-1, K/2) padding (stride>1) as the reference, or zero padding `padL`.
 * `roll` is the discriminator phase shift (discriminator.py:160-172; the conv sees
 * torch.roll(x, roll, 2)).  The output is the PRE-activation; its consumer applies
 * PReLU/BN through its own segan_src. */
int segan_conv1d_fwd(const segan_src* x, const void* wf, const float* bias, float* out, int B,
                     int N, int M, int L, int K, int S, int padL, int mode, int roll,
                     int precision, void* scratch, size_t scratch_bytes, void* stream);

/* Data gradient of the above (autograd of modules.py:98-99): dx[b,n,i] += over the
 * reflect-padded, rolled coordinates.  da: [B, M, L/S]; dx: [B, N, L] is fully
 * overwritten.  `halo` is scratch of B*N*(K-1) floats.  `w` (optional) is the UNPACKED
 * weight [M][N][K]: when given and N <= 2 (the first layer: 1-2 input channels) a direct
 * VALU kernel is used instead of the MFMA tile kernel and `wt` may be NULL. */
int segan_conv1d_dgrad(const float* da, const void* wt, const float* w, float* dx, float* halo,
                       int B, int N, int M, int L, int K, int S, int padL, int roll, int precision,
                       void* scratch, size_t scratch_bytes, void* stream);

/* Weight gradient shared by both layer types (W form):
 *   dw[m,n,k] += sum_{b,t} lo[b,m,t] * pad(roll(hi))[b,n,S*t+k]
 * conv:   lo = da (grad of pre-activation), hi = layer input x, reflect padding;
 * deconv: lo = layer input x (with its transform), hi = dy, zero padding.
 * Accumulates into dw, which is how torch accumulates .grad.  The contraction over (b, t) is
 * split across workgroups; by default the partial tiles are added with fp32 atomics (order
 * varies run to run, results differ in the last bits); with SEGAN_WGRAD_DETERMINISTIC in
 * `flags` they are written to `scratch` and added in split order by a second kernel
 * (bit-reproducible; fp32 only).
 * `precision`: SEGAN_PREC_*; the bf16 modes contract 8 samples per MFMA operand and return
 * -3 (SEGAN_EUNSUPPORTED) for Ls % 4 != 0 or very short rows: the caller falls back to fp32.
 * `scratch` / `scratch_bytes` (may be NULL / 0 unless deterministic): segan_wgrad_scratch_bytes
 * (...) bytes.  fp32: a lo operand with a transform or in two segments is materialised there
 * once per call (the fast kernel streams lo by LDS-DMA), followed by the partial tiles of the
 * deterministic mode.  bf16 modes: the lo operand converted ONCE into bf16 planes laid out for
 * the kernel (every column tile of dw re-reads it). */
#define SEGAN_WGRAD_DETERMINISTIC 1
size_t segan_wgrad_scratch_bytes(int B, int M, int N, int Ls, int S, int precision, int flags);
int segan_wgrad(const segan_src* lo, const segan_src* hi, float* dw, int B, int M, int N, int Ls,
                int K, int S, int padL, int mode, int roll, int precision, int flags, void* scratch,
                size_t scratch_bytes, void* stream);

/* GDeconv1DBlock forward (modules.py:135-141): ConvTranspose1d(stride S, padding
 * `pad`) trimmed to S*Ls samples, + bias, optional tanh (last generator layer).
 *   y[b,n,j] = bias[n] + sum_{m} sum_{t,k: S*t+k-pad=j} x[b,m,t] * w[m,n,k]
 * x: [B, M, Ls] as a segan_src (the skip concat and alpha scaling of
 * generator.py:64-76 are its second segment), y: [B, N, S*Ls].  `w` (optional): the
 * UNPACKED weight; with N <= 2 (the last generator layer, Cout = 1) the direct VALU
 * kernel is used and `wt` may be NULL. */
int segan_deconv1d_fwd(const segan_src* x, const void* wt, const float* w, const float* bias,
                       float* y, int B, int M, int N, int Ls, int K, int S, int pad, int act,
                       int precision, void* scratch, size_t scratch_bytes, void* stream);

/* Data gradient of the deconv: dx[b,m,t] = sum_{n,k} w[m,n,k] * dy[b,n,S*t+k-pad].
 * The M rows are split at M0 into two destinations (dx0: [B,M0,Ls], dx1:
 * [B,M-M0,Ls]); a NULL destination skips that half's tiles entirely (the z half of
 * the first decoder layer needs no gradient). */
int segan_deconv1d_dgrad(const float* dy, const void* wf, float* dx0, float* dx1, int B, int M,
                         int M0, int N, int Ls, int K, int S, int pad, int precision, void* scratch,
                         size_t scratch_bytes, void* stream);

/* ---- per-channel pointwise / reduction kernels ------------------------------------ */

/* BatchNorm1d training statistics (modules.py:10-11; torch.nn.BatchNorm1d): per
 * channel mean and biased variance of x[B,C,L]; writes scale = gamma*rstd and
 * shift = beta - mean*scale for the consumer's segan_src, saves mean/rstd for the
 * backward, and updates running_mean / running_var (momentum, unbiased variance)
 * when they are non-NULL.  `ws` is scratch of 3*C*nsplit floats (nsplit from
 * segan_bn_nsplit, which is also the split count of act_bwd / tanh_bwd). */
int segan_bn_nsplit(int B, int C, int L);
int segan_bn_stats(const float* x, const float* gamma, const float* beta, float eps,
                   float momentum, float* running_mean, float* running_var, float* mean,
                   float* rstd, float* scale, float* shift, float* ws, int B, int C, int L,
                   void* stream);
/* The same in two calls, for synchronised BatchNorm under data parallelism: `partial` leaves
 * this rank's (count, mean, M2) per channel and batch split in ws[nsplit][C][3]; the caller
 * all-gathers the ranks' ws; `final` combines nsplit_total = world*nsplit partials (Chan et
 * al.) exactly as segan_bn_stats does for one rank. */
int segan_bn_partial(const float* x, float* ws, int B, int C, int L, void* stream);
int segan_bn_final(const float* ws, int nsplit_total, const float* gamma, const float* beta,
                   float eps, float momentum, float* running_mean, float* running_var, float* mean,
                   float* rstd, float* scale, float* shift, int C, void* stream);

/* y = tanh(x*scale[c] + shift[c]) on [B, C, L] (scale / shift may be NULL): the generator's
 * last block when it carries a BatchNorm (modules.py:135-141 with norm_type='bnorm'). */
int segan_affine_tanh(const float* x, const float* scale, const float* shift, float* y, int B,
                      int C, int L, void* stream);
/* y = x * scale[c] * mask on [B, C, L] (scale may be NULL; y may alias x): nn.Dropout on the skip
 * path (generator.py:53-54,70-71) with mask = 0 or 1/(1-p) per element, and its backward. */
int segan_scale_mask(const float* x, const float* scale, const float* mask, float* y, int B, int C,
                     int L, void* stream);

/* y = prelu(x*scale[c] + shift[c], slope[c]) materialised (used for the FC input
 * h.view(B,-1) of discriminator.py:181 and for int_act / ret_hid outputs). */
int segan_affine_prelu(const float* x, const float* scale, const float* shift, const float* slope,
                       float* y, int B, int C, int L, void* stream);

/* GSkip with merge_mode 'sum' (generator.py:64-74): out = prelu(x0, slope0) + alpha[c]*x1
 * (slope0 NULL = identity); all [B,C,L]. */
int segan_sum_skip(const float* x0, const float* slope0, const float* x1, const float* alpha,
                   float* out, int B, int C, int L, void* stream);

/* Backward through an (optional BN) + PReLU/identity + optional alpha-skip tap of a
 * pre-activation a[B,C,L]:
 *   v  = a*scale + shift (BN folded; identity when NULL)
 *   g  = dh * (v > 0 ? 1 : slope)          (+ alpha * dskip when dskip != NULL)
 *   dslope += sum dh * min(v, 0) ; dalpha += sum dskip * a ; dbias += sum da
 *   BN: dbeta += sum g ; dgamma += sum g*xhat ; da = scale*(g - dbeta/N - xhat*dgamma/N)
 * Any gradient output may be NULL.  ws: scratch of (4*nsplit + 2)*C floats. */
int segan_act_bwd(const float* a, const float* dh, const float* dskip, const float* slope,
                  const float* alpha, const float* bn_mean, const float* bn_rstd,
                  const float* bn_gamma, const float* bn_beta, float* da, float* dslope,
                  float* dalpha, float* dgamma, float* dbeta, float* dbias, float* ws, int B, int C,
                  int L, void* stream);
/* The BatchNorm branch of segan_act_bwd in two calls (synchronised BatchNorm): `reduce`
 * accumulates dslope / dgamma / dbeta from this rank's samples and leaves the per-channel
 * (sum g, sum g*xhat) in totals[C][2]; the caller all-reduces (sums) totals; `apply` writes da
 * with the global totals and the global per-channel element count, and accumulates dbias. */
int segan_act_bwd_bn_reduce(const float* a, const float* dh, const float* slope,
                            const float* bn_mean, const float* bn_rstd, const float* bn_gamma,
                            const float* bn_beta, float* dslope, float* dgamma, float* dbeta,
                            float* totals, float* ws, int B, int C, int L, void* stream);
int segan_act_bwd_bn_apply(const float* a, const float* dh, const float* slope,
                           const float* bn_mean, const float* bn_rstd, const float* bn_gamma,
                           const float* bn_beta, const float* totals, float* da, float* dbias,
                           float* ws, int B, int C, int L, double count_total, void* stream);

/* tanh backward of the generator output with the L1 term of model.py:316-319 fused:
 *   g = dy_adv (may be NULL) + l1_scale * sign(y - clean) (when clean != NULL)
 *   da = g * (1 - y*y) ; dbias += sum da.   ws: scratch of nsplit*C floats. */
int segan_tanh_bwd(const float* y, const float* dy, const float* clean, float l1_scale, float* da,
                   float* dbias, float* ws, int B, int C, int L, void* stream);

/* ---- dense layers of the discriminator head (discriminator.py:111-117) ------------ */

/* C[M,N] (+)= op(A)[M,K] * op(B)[K,N] with explicit element strides; exact fp32 on
 * MFMA.  beta0 != 0 overwrites C, otherwise accumulates.  Small outputs split the contraction
 * across workgroups: partials are added with fp32 atomics, or — SEGAN_GEMM_DETERMINISTIC in
 * `flags` — written as slabs into `scratch` (segan_gemm_scratch_bytes, 16-byte aligned) and
 * added in split order by a second kernel (bit-reproducible); deterministic without scratch keeps
 * the contraction whole in one workgroup per tile. */
#define SEGAN_GEMM_DETERMINISTIC 1
size_t segan_gemm_scratch_bytes(int M, int N, int K);
int segan_gemm(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn,
               float* C, int64_t ldc, int M, int N, int K, int beta0, int flags, void* scratch,
               size_t scratch_bytes, void* stream);

/* y[r,c] = prelu(x[r,c] + bias[c], slope[c]) (slope NULL = identity), rows x cols. */
int segan_bias_prelu_rows(const float* x, const float* bias, const float* slope, float* y,
                          int rows, int cols, void* stream);
/* backward: dx = dy*(v>0?1:slope), dslope[c] += sum dy*min(v,0), dbias[c] += sum dx,
 * with v = x + bias. */
int segan_bias_prelu_rows_bwd(const float* x, const float* bias, const float* slope,
                              const float* dy, float* dx, float* dslope, float* dbias, int rows,
                              int cols, void* stream);

/* ---- losses (train.py:94 nn.MSELoss; model.py:79 F.l1_loss) ------------------------ */
/* loss[0] = mean((x - target)^2) (loss may be NULL);
 * grad (may be NULL) = 2*(x-target)/n * gscale * (gout ? gout[0] : 1), gout being the
 * upstream scalar gradient as a DEVICE pointer (no host sync). */
int segan_mse_const(const float* x, float target, float* loss, float* grad, const float* gout,
                    float gscale, int n, void* stream);
/* F.binary_cross_entropy_with_logits against a constant label (WSEGAN --vanilla_gan,
 * model.py:582-583); same argument meaning as segan_mse_const. */
int segan_bce_logits_const(const float* x, float target, float* loss, float* grad,
                           const float* gout, float gscale, int n, void* stream);
/* loss[0] = mean(|x - y|)  (n may be large; ws: scratch of 1024 floats). */
int segan_l1_mean(const float* x, const float* y, float* loss, float* ws, int64_t n,
                  void* stream);
/* grad = sign(x - y) / n * gscale * (gout ? gout[0] : 1)   (torch.sign: sign(0) = 0). */
int segan_l1_bwd(const float* x, const float* y, const float* gout, float gscale, float* grad,
                 int64_t n, void* stream);

/* Data gradient of conv1d_fwd for SHORT rows (L/S in {4, 8, 16, 32, 64}; N % 4 == 0, M % 16 == 0;
 * any supported stride), as the GEMM + col2im of a transposed conv: no zero-halo columns, the
 * reflect fold and the roll are applied in the epilogue, complete dx rows are stored (no halo
 * scratch).  `wg` is the "G" packing of the weight: wg[m][n*32 + r*U + u] = w[m][n][S*u + r]
 * (U = 32/S; 0 for S*u + r >= K), segan_packed_g_bytes() bytes, written by
 * segan_pack_weights_g.  Same result as segan_conv1d_dgrad (fp32).  Returns SEGAN_EUNSUPPORTED
 * for other geometries. */
size_t segan_packed_g_bytes(int M, int N, int S);
int segan_pack_weights_g(const float* w, float* wg, int M, int N, int K, int S, void* stream);
int segan_conv1d_dgrad_short(const float* da, const float* wg, float* dx, int B, int N, int M,
                             int L, int K, int S, int padL, int roll, void* stream);

/* Global pooling over time of x[rows][L] (rows = B*C), the 'gmax' / 'gavg' discriminator heads
 * (discriminator.py:128-137,183-190).  mode 0: y[row] = max, idx[row] = the FIRST position
 * attaining it; mode 1: y[row] = mean (idx unused, may be NULL).  bwd: dx[row][t] =
 * (t == idx[row]) ? dy[row] : 0, or dy[row] / L.  Rows of -inf give -inf at index 0; the maximum
 * of a row that contains NaN is unspecified (AdaptiveMaxPool1d propagates the NaN; this kernel
 * keeps one only where it is the first element a lane visits): activations here are finite. */
int segan_pool_time_fwd(const float* x, float* y, int* idx, int rows, int L, int mode,
                        void* stream);
int segan_pool_time_bwd(const float* dy, const int* idx, float* dx, int rows, int L, int mode,
                        void* stream);

/* F.mse_loss between two tensors (--reg_loss mse_loss, train.py:179, model.py:79): loss[0] =
 * mean((x - y)^2) (ws: 1024 floats); grad = 2*(x - y)/n * gscale * (gout ? gout[0] : 1). */
int segan_mse_mean(const float* x, const float* y, float* loss, float* ws, int64_t n,
                   void* stream);
int segan_mse_bwd(const float* x, const float* y, const float* gout, float gscale, float* grad,
                  int64_t n, void* stream);

/* ---- spectral normalisation ('snorm', modules.py:12-14, discriminator.py:118-121) -------
 * torch.nn.utils.spectral_norm with its defaults (one power iteration in training mode,
 * eps 1e-12) on a weight [A][Bd][K] viewed as a matrix with rows = dim 0 (Conv1d, Linear,
 * PReLU) or dim 1 (ConvTranspose1d):
 *   power_iteration != 0:  v <- normalize(W^T u), u <- normalize(W v)   (u, v updated in place)
 *   sigma[0] = u . (W v);  w_sn = w / sigma
 * ws: scratch of segan_snorm_ws_floats(...) floats (shared by fwd and bwd). */
size_t segan_snorm_ws_floats(int A, int Bd, int K, int dim);
int segan_snorm_fwd(const float* w, float* u, float* v, float* w_sn, float* sigma, float* ws, int A,
                    int Bd, int K, int dim, int power_iteration, float eps, void* stream);
/* dw += dw_sn/sigma - (<dw_sn, w>/sigma^2) u v^T   (u, v: the vectors the forward used) */
int segan_snorm_bwd(const float* dw_sn, const float* w, const float* u, const float* v,
                    const float* sigma, float* dw, float* ws, int A, int Bd, int K, int dim,
                    void* stream);

/* ---- STFT power loss of the WSEGAN step (model.py:640-653) ------------------------------
 * torch.stft(x, n_fft, hop_length=hop, win_length=win, normalized=True) with window=None:
 * a rectangular window zero-padded to n_fft, centre (reflect) padding of n_fft/2.  Only `win`
 * samples of a frame are non-zero, so the transform is frames[B*NF, win] x basis[win, 2*nbins]
 * (NF = 1 + T/hop, nbins = n_fft/2+1; columns [0,nbins) real, [nbins,2nbins) imaginary) run
 * through segan_gemm.  Rows of the basis and of the spectra are `pitch` =
 * segan_stft_pitch(n_fft) floats wide (2*nbins rounded up to a multiple of 4, pad columns
 * zero) so that they are 16-byte aligned for the GEMM.  Requires n_fft/2 < T.  segan_stft_frames
 * and segan_stft_overlap_add also require an even n_fft (SEGAN_EINVAL otherwise): for an odd one
 * the padded index can pass the reach of one reflection and the frame count differs from
 * torch.stft's. */
int segan_stft_pitch(int n_fft);
int segan_stft_basis(float* basis, int n_fft, int win, void* stream);
int segan_stft_frames(const float* x, float* frames, int B, int T, int n_fft, int hop, int win,
                      void* stream);
/* db[r][k] = 10*log10(re^2 + im^2 + eps) of S[rows][pitch]  (eps = 10e-20, model.py:646) */
int segan_powdb(const float* S, float* db, int64_t rows, int nbins, int pitch, float eps,
                void* stream);
/* dS = ddb * d(db)/d(re, im) */
int segan_powdb_bwd(const float* S, const float* ddb, float* dS, int64_t rows, int nbins, int pitch,
                    float eps, void* stream);
/* dx[B][T] = adjoint of segan_stft_frames applied to dframes[B*NF][win] (overwrites dx) */
int segan_stft_overlap_add(const float* dframes, float* dx, int B, int T, int n_fft, int hop,
                           int win, void* stream);

/* ---- input side (se_dataset.py:108-117,196-197) ------------------------------------------
 * int16 PCM slices -> (2/65535)(x-32767)+1 -> pre-emphasis y[n] = x[n] - coef*x[n-1], computed
 * in double and rounded once like numpy does (bit-exact).  pcm: [B][2][T+1] (clean row, noisy
 * row; element 0 of a row is the wav sample preceding the slice), first[B]: 1 when the slice
 * starts its wav (then y[0] = x[0]).  Outputs clean/noisy [B][T] fp32. */
int segan_pcm16_prep(const int16_t* pcm, const unsigned char* first, float* clean, float* noisy,
                     int B, int T, double coef, void* stream);

/* ---- output side and validation --------------------------------------
 * De-emphasis x[n] = coef*x[n-1] + y[n] per row of y[rows][T] (se_dataset.py:119-126: the
 * reference's per-sample python loop at the end of SEGAN.generate, model.py:154-156) as a
 * blocked scan; coef <= 0 copies.  x may alias y. */
int segan_deemphasis(const float* y, float* x, int rows, int T, double coef, void* stream);
/* Segmental SNR of utils.py:350-395 for rows of ref / deg [rows][T]: seg[rows][nframes] (nframes
 * = segan_ssnr_frames(T, srate)) holds the clamped per-frame values, out[rows][2] = (overall
 * SNR in dB, mean segmental SNR). */
int segan_ssnr_frames(int T, int srate);
int segan_ssnr(const float* ref, const float* deg, float* seg, float* out, int rows, int T,
               int srate, double eps, void* stream);
/* Per-frame objective quality measures of the reference's CompositeEval, fp64 like numpy, on the
 * SSNR frames (nframes = segan_ssnr_frames(T, srate); nothing is launched when it is 0) of
 * ref / deg [rows][T]; dist[rows][nframes].  srate: a 30 ms window of 4 .. 1024 samples.
 *   segan_wss: weighted spectral slope distortion (utils.py:442-596);
 *   segan_llr: log-likelihood ratio (utils.py:598-716), LPC order 16 (srate >= 10000) or 10;
 *              NaN where the clean frame is digital silence. */
int segan_wss(const float* ref, const float* deg, double* dist, int rows, int T, int srate,
              void* stream);
int segan_llr(const float* ref, const float* deg, double* dist, int rows, int T, int srate,
              void* stream);
/* STOI, short-time objective intelligibility (Taal et al. 2011; the reference's utils/stoi.m,
 * DESIGN.md section 10), fp64, of row r = ref / deg [rows][T] restricted to its first lengths[r]
 * samples (lengths: device int[rows], each in 0 .. T; values outside are clamped; NULL: all T).
 * srate: 4000 .. 48000 Hz.
 *   segan_stoi_plan (host only, no device): pq[2] = (p, q), 10000 / srate in lowest terms;
 *     *ntaps = 2*10*max(p, q) + 1 resampling taps, written to taps when it is not NULL (cap >= *ntaps);
 *     bands[15][2] (when not NULL) = the DFT bins [lo, hi) of each third-octave band.
 *     srate 10000: (1, 1), one tap 1.0 (no resampling).
 *   segan_stoi_dims (host only): the stage sizes for rows of T samples, dims[5] = (Ly resampled
 *     length, F frames of Ly, Lc compacted length (F - 1)*128 + 256, Fb = F - 1 band frames,
 *     S = Fb - 29 segments), each 0 where negative.  The buffers of segan_stoi hold
 *     xr, yr [rows][Ly], energy [rows][F], mask, kept [rows][F] (int), count [rows] (int),
 *     xs, ys [rows][Lc], X, Y [rows][15][Fb], rho [rows][S][15], d [rows]; each at least one
 *     element.  Per row: the resampled signals (zero past ceil(len*p/q)), clean frame energies
 *     in dB, keep mask (1/0), kept frame indices (first count[r] valid), M = count[r], compacted
 *     signals (zero past (M-1)*128 + 256), band envelopes (first max(M-1, 0) frames valid),
 *     segment correlations (first max(M-30, 0) segments valid) and d, NaN without segments or
 *     with a NaN correlation.  Deterministic: no atomics, each row independent of the others. */
int segan_stoi_plan(int srate, int* pq, int* ntaps, double* taps, int cap, int* bands);
int segan_stoi_dims(int T, int srate, int* dims);
int segan_stoi(const float* ref, const float* deg, const int* lengths, int rows, int T, int srate,
               double* xr, double* yr, double* energy, int* mask, int* kept, int* count,
               double* xs, double* ys, double* X, double* Y, double* rho, double* d, void* stream);
/* ESTOI, extended STOI (Jensen & Taal 2016; DESIGN.md section 10, "ESTOI"): segan_stoi's
 * arguments, conventions and stages up to the band envelopes X, Y (buffer sizes from
 * segan_stoi_dims), then per segment s the 15 x 30 windows of X and of Y normalised along their
 * rows and then their columns (mean removed, unit norm; a vector of no energy, or whose centred
 * energy is at most 2^-40 of its energy, becomes zeros) and dm[rows][S] = their inner product /
 * 30 (first max(M-30, 0) segments valid), d[rows] = the mean of the row's dm, NaN without
 * segments.  No clipping, no energy scaling.  Added without a change of SEGAN_ABI_VERSION: the
 * export is purely additive, every earlier entry keeps its signature and its results. */
int segan_estoi(const float* ref, const float* deg, const int* lengths, int rows, int T, int srate,
                double* xr, double* yr, double* energy, int* mask, int* kept, int* count,
                double* xs, double* ys, double* X, double* Y, double* dm, double* d, void* stream);
/* Three more objective measures, fp64, of row r = ref / deg [rows][T] restricted to its first
 * lengths[r] samples (device int[rows], clamped to 0 .. T; NULL: all T); DESIGN.md section 13.
 * Frames, window and srate limits are those of segan_wss / segan_llr; row r has
 * segan_ssnr_frames(lengths[r], srate) frames of its own, and frames_out [rows][nframes]
 * (nframes = segan_ssnr_frames(T, srate), at least one element) is NaN past them.  Every sum runs
 * in a fixed order without atomics: a row's values do not depend on T, on the other rows or on
 * the samples past its length, and two calls return the same bits.
 *   segan_fwsegsnr: frequency-weighted segmental SNR.  Per frame the DFT magnitudes of all
 *     nfft/2 bins, each spectrum divided by its sum, through WSS's 25 critical-band filters
 *     (ce, pe); sum(W snr) / sum(W) with W = ce^0.2, snr = 10 log10(ce^2 / max((ce - pe)^2,
 *     2^-52)), clipped to [-10, 35]; NaN where that is not finite (a frame of digital silence in
 *     either signal).  row_out[rows]: the mean of the row's finite frames, NaN without any.
 *   segan_cepdist: LPC cepstrum distance.  LLR's lags and order (16 for srate >= 10000, else 10),
 *     Levinson-Durbin in fp64 without LLR's fp32 rounding, c_1 = -a_1, c_n = -a_n - (1/n)
 *     sum_{k<n} k c_k a_{n-k}; min(10, 10 sqrt(2) / ln 10 * ||c(ref) - c(deg)||_2); NaN where
 *     either frame has no energy.  Nothing is launched when nframes is 0.
 *   segan_sisdr: scale-invariant SDR (Le Roux et al. 2019) of whole rows.  Both means removed,
 *     alpha = <s,x> / <s,s>, e = alpha s - x summed sample by sample in a second pass;
 *     row_out[rows] = 10 log10(alpha^2 <s,s> / <e,e>): NaN where <s,s> is 0, +inf where <e,e> is.
 *     ws: workspace of rows * (4 * ceil(T / SEGAN_SISDR_SPAN) + 4) doubles.
 * Added without a change of SEGAN_ABI_VERSION: the exports are purely additive, every earlier
 * entry keeps its signature and its results. */
#define SEGAN_SISDR_SPAN 4096
int segan_fwsegsnr(const float* ref, const float* deg, const int* lengths, int rows, int T,
                   int srate, double* frames_out, double* row_out, void* stream);
int segan_cepdist(const float* ref, const float* deg, const int* lengths, int rows, int T,
                  int srate, double* frames_out, void* stream);
int segan_sisdr(const float* ref, const float* deg, const int* lengths, int rows, int T,
                double* row_out, double* ws, void* stream);
/* BSS-eval SDR (the SDR of bss_eval_sources with a distortion filter of `taps` <= 512 taps), fp64
 * on fp32 rows ref / deg [rows][T], row r restricted to its first lengths[r] = L samples (device
 * int[rows], clamped to 0 .. T; NULL: all T); DESIGN.md section 15.  With s, x the row, zero
 * outside [0, L), and n = taps:
 *   r[k] = sum_t s[t] s[t+k], d[k] = sum_t s[t] x[t+k], k < n: exact products, added per span of
 *     SEGAN_SDR_SPAN samples of t in ascending order, then the spans in ascending order;
 *   Toeplitz(r) c = d by the Levinson recursion; at order m with prediction error E_m <=
 *     2^-40 r[0] the recursion stops, c[k] = 0 for k >= m, and m is the order reached (else n);
 *   st[t] = sum_k c[k] s[t-k] (k ascending), t < L + n - 1; St = sum st^2, Ee = sum (x - st)^2,
 *     sample by sample;
 *   row_out[rows] = 10 log10(St / Ee) dB; NaN where L == 0, r[0] == 0 or St == Ee == 0; else +inf
 *     where Ee == 0 (deg == g ref, g a power of two: c = g delta exactly), -inf where St == 0.
 * No atomics, every sum in an order fixed by the sample index: a row's bits depend neither on T,
 * nor on the other rows, nor on the samples past its length.
 *   segan_sdr_dims (host only): out[3] = {SEGAN_SDR_SPAN, ceil(T / SEGAN_SDR_SPAN), the doubles of
 *     segan_sdr's workspace `ws`}.
 *   segan_sdr: stages_out (may be NULL) [rows][3 taps + 3]: r[taps], d[taps], c[taps], the order
 *     reached, St, Ee of each row.
 *   segan_toeplitz_solve: the solver on its own, r / d / c_out [rows][n] fp64, n <= 512,
 *     order_out int[rows]; same guard.
 * rows in 1 .. 65535, T > 0, taps in 1 .. SEGAN_SDR_MAX_TAPS, checked before any launch.  Added
 * without a change of SEGAN_ABI_VERSION: the exports are purely additive. */
#define SEGAN_SDR_SPAN 4096
#define SEGAN_SDR_MAX_TAPS 512
int segan_sdr_dims(int rows, int T, int taps, long long* out);
int segan_sdr(const float* ref, const float* deg, const int* lengths, int rows, int T, int taps,
              double* row_out, double* stages_out, double* ws, void* stream);
int segan_toeplitz_solve(const double* r, const double* d, int rows, int n, double* c_out,
                         int* order_out, void* stream);
/* SRMR, the speech-to-reverberation modulation energy ratio of Falk, Zheng and Chan (2010): the
 * time-domain measure with 23 gammatone channels and 8 modulation bands, no energy normalisation;
 * it needs no clean signal.  fp64 on fp32 rows x [rows][T] at `rate` (8000 or 16000), row r
 * restricted to its first lengths[r] = N samples (device int[rows], clamped to 0 .. T; NULL: all
 * T); DESIGN.md section 16, scripts/srmr_oracle.py.  Per row:
 *   the gammatone channels (four cascaded biquads each, zero state, sequential in time); the
 *   envelope |analytic(y)| on the row zero-padded to its own L, the smallest power of two >= N;
 *   the eight Q = 2 modulation band-passes; E[i][k][f] = sum (w m)^2 over the full frames of
 *   ceil(0.256 rate) samples every ceil(0.064 rate), w the periodic Hamming window; Ebar the mean
 *   over the frames in ascending order; BW = ERB of the first channel, from the lowest centre
 *   frequency upwards, at which the cumulated share of sum_k Ebar exceeds 90 %; K* = 5 .. 8 from
 *   BW against the bands' left cutoffs (5 where BW lies at or below the fifth band's);
 *   row_out[rows] = sum_i sum_{k<4} Ebar / sum_i sum_{4<=k<K*} Ebar; NaN for a row shorter than
 *   one frame or without energy.
 * No atomics, every sum and recurrence in an order fixed by the sample index: a row's bits depend
 * neither on T, nor on the other rows, nor on the samples past its length, and a row times a
 * power of two gives the same bits.
 *   segan_srmr_dims (host only): out[4] = {L of T, the frames of T, the doubles of workspace per
 *     row, the doubles of segan_srmr's workspace `ws` for `rows` rows}.
 *   segan_srmr: ws 16-byte aligned; stages_out (may be NULL) [rows][SEGAN_SRMR_STAGE]: the centre
 *     frequencies [23], sum e_i^2 over the N samples [23], Ebar [23][8], BW, K*, the cumulated
 *     share that decided BW, the value.
 *   segan_fft_z2z: the batched complex fp64 transform of n = 2^log2n points on its own, in / out
 *     [rows][n] interleaved (re, im), 16-byte aligned; inverse != 0: the inverse with 1/n.
 *     n <= 2^SEGAN_FFT_LDS_LOG2 runs in LDS and may be in place; larger n as two levels, in != out.
 * rows in 1 .. 65535, T in 1 .. 2^SEGAN_FFT_MAX_LOG2, log2n in 1 .. SEGAN_FFT_MAX_LOG2, checked
 * before any launch.  Added without a change of SEGAN_ABI_VERSION: the exports are purely
 * additive. */
#define SEGAN_SRMR_CHANNELS 23
#define SEGAN_SRMR_BANDS 8
#define SEGAN_SRMR_STAGE 234
#define SEGAN_FFT_LDS_LOG2 12
#define SEGAN_FFT_MAX_LOG2 20
int segan_fft_z2z(const double* in, double* out, int rows, int log2n, int inverse, void* stream);
int segan_srmr_dims(int rows, int T, int rate, long long* out);
int segan_srmr(const float* x, const int* lengths, int rows, int T, int rate, double* row_out,
               double* stages_out, double* ws, void* stream);
/* Pitch tracking by YIN (de Cheveigne & Kawahara 2002) with a 5 ms hop, and the F0 / voicing
 * measures on two such contours; DESIGN.md section 19, scripts/pitch_oracle.py.  fp64 on fp32 rows
 * x [rows][T] at `srate` (16000 or 8000), row r restricted to its first lengths[r] = L samples
 * (device int[rows], clamped to 0 .. T; NULL: all T).  At 16 kHz H = 80, tau_min = 40, tau_max =
 * 266 (8 kHz: all halved), NB = SEGAN_PITCH_NB hop blocks per frame:
 *   hop blocks u < nb = (L - (tau_max + 1)) / H (0 below that): S_u(tau) = sum x[j] x[j+tau],
 *     E_u(tau) = sum x[j+tau]^2 over j in [uH, uH + H) ascending, tau = 0 .. tau_max + 1 (exact
 *     products);
 *   frames t < nf = nb - NB + 1 (0 below that): the blocks t .. t + NB - 1 added in ascending
 *     order; d(0) = 0, d(tau) = (E(0) + E(tau)) - 2 R(tau); c(tau) the ascending running sum of
 *     d(1 .. tau); d'(tau) = d(tau) tau / c(tau) where c(tau) > 0, else 1;
 *   the pick: the smallest tau in [tau_min, tau_max] with d'(tau) < theta, then onwards while
 *     tau < tau_max and d'(tau + 1) < d'(tau); none, or c(tau_max + 1) not > 0: unvoiced;
 *   f0 = srate / (tau + delta), delta = clamp(0.5 (a - c) / (a - 2 b + c), -0.5, 0.5) with
 *     a, b, c = d' at tau - 1, tau, tau + 1 (0 where the denominator is not > 0).
 *   segan_pitch_frames (host only): nf of a row of T samples, -1 for a bad argument.
 *   segan_pitch_dims (host only): out[6] = {H, tau_min, tau_max, nb of T, F = nf of T, the doubles
 *     of workspace `ws` for `rows` rows}.
 *   segan_pitch: f0 [rows][F] (0 when unvoiced), lag int[rows][F] (0 when unvoiced), ap [rows][F]
 *     (d' at the pick; the minimum of d' over [tau_min, tau_max] when unvoiced); frames from the
 *     row's own nf on: f0 = 0, lag = -1, ap = NaN.  theta in (0, 1].  F == 0: nothing is written.
 *   segan_pitch_cmnd: d' itself, cmnd [rows][F][tau_max + 2] (NaN from the row's own nf on).
 *   segan_f0_eval: f0 / lag [rows][F] of the clean and the processed contour, nframes int[rows]
 *     (device, clamped to 0 .. F; NULL: F), F >= 0; out4 [rows][4] = (f0_mae in Hz over the clean
 *     contour's voiced frames, vuv_acc, f0_kld between the log-f0 distributions, voiced), on the
 *     log-f0 contours interpolated linearly over the unvoiced frames, every sum in ascending frame
 *     order.  NaN: all four without a frame; f0_mae and f0_kld where either contour has no voiced
 *     frame; f0_kld below two frames or with a constant processed contour.
 * No atomics, every sum in an order fixed by the indices: a row's bits depend neither on T, nor on
 * the other rows, nor on the samples past its length, and a row times a power of two gives the
 * same lags and f0 bits.  rows in 1 .. 65535, T in 1 .. 2^24, checked before any launch.  Added
 * without a change of SEGAN_ABI_VERSION: the exports are purely additive. */
#define SEGAN_PITCH_NB 5
int segan_pitch_frames(int T, int srate);
int segan_pitch_dims(int rows, int T, int srate, long long* out);
int segan_pitch(const float* x, const int* lengths, int rows, int T, int srate, double theta,
                double* f0, int* lag, double* ap, double* ws, void* stream);
int segan_pitch_cmnd(const float* x, const int* lengths, int rows, int T, int srate, double* cmnd,
                     double* ws, void* stream);
int segan_f0_eval(const double* f0_ref, const int* lag_ref, const double* f0_deg,
                  const int* lag_deg, const int* nframes, int rows, int F, double* out4,
                  void* stream);

/* ---- Wiener and log-MMSE baseline enhancers ----------------------------
 * One short-time spectral enhancer with two gain rules, defined by scripts/denoise_oracle.py: the
 * decision-directed a-priori SNR of Ephraim & Malah with the VAD-gated noise estimate of Loizou's
 * wiener_as / logmmse programs, written from the literature.  Rows x [rows][T] of x_dtype
 * (SEGAN_DT_F32 or SEGAN_DT_F64) at srate 16000 or 8000, row r restricted to its first lengths[r]
 * samples L (device int[rows], clamped to 0 .. T; NULL: all T); all arithmetic fp64.  F = srate /
 * 50, H = F / 2, N = 2 F; w = the Hamming window 0.54 - 0.46 cos(2 pi n / (F - 1)) times H / sum w.
 *   lambda[k] = max(m[k]^2, 2^-100), m = the mean of |DFT_N(w x[j F : (j + 1) F])[k]| over j < 6
 *     added in ascending j, k = 0 .. F;
 *   frame t < nf = L / H - 1: S = DFT_N(w x[t H : t H + F]), s2 = |S|^2, gamma = min(s2 / lambda,
 *     40), xi = max(0.98 P / lambda + (1 - 0.98) max(gamma - 1, 0), 10^-2.5), P = |G S|^2 of the
 *     frame before (t = 0: the first term is 0.98);
 *   v_t = (sum_k c_k (gamma xi / (1 + xi) - log(1 + xi))) / F, c = 1, 2, .., 2, 1, the bins added
 *     in groups of 64 (ascending k inside a group from zero, then the groups in ascending order
 *     from zero); v_t < 0.15: lambda <- max(0.98 lambda + 0.02 s2, 2^-100) after gamma and xi of
 *     the frame were formed;
 *   A = xi / (1 + xi); G = A (SEGAN_DENOISE_WIENER, Scalart & Filho 1996) or A exp(E1(max(A gamma,
 *     2^-40)) / 2) (SEGAN_DENOISE_LOGMMSE, Ephraim & Malah 1985; not clipped), E1 by its power
 *     series below 1 and the modified Lentz continued fraction from 1 on, to a relative step 2^-53;
 *   y[n] = sum_t o_t[n - t H], o_t = the first F samples of real(IDFT_N(G S)) with the Hermitian
 *     extension, the earlier frame added first; y[n] = 0 from (nf + 1) H to T.
 *   L < 6 F: nf = 0 and y = x below L, 0 from L on.
 *   segan_denoise_dims (host only): out[5] = {F, H, N, nf of a row of T samples, the bytes of
 *     workspace `ws` for `rows` rows: 16 (F + 1) nf + 8 (F + 1) a row}.
 *   segan_denoise: y [rows][T] of y_dtype (SEGAN_DT_F64, or SEGAN_DT_F32 rounded once), nframes
 *     int[rows]; vad double[rows][nf of T] = v_t and update int[rows][nf of T] = 1 where lambda was
 *     updated at the frame, each optional (NULL), NaN and -1 from the row's own nf on.  ws: 16-byte
 *     aligned.
 * No atomics, no scratch, every sum in an order fixed by the indices: a row's bits depend neither
 * on T, nor on the other rows, nor on the samples past its length.  rows in 1 .. 65535, T in
 * 1 .. 2^24, checked before any launch.  Added without a change of SEGAN_ABI_VERSION: the exports
 * are purely additive. */
#define SEGAN_DENOISE_WIENER 0
#define SEGAN_DENOISE_LOGMMSE 1
int segan_denoise_dims(int rows, int T, int srate, long long* out);
int segan_denoise(const void* x, int x_dtype, const int* lengths, int rows, int T, int srate,
                  int rule, void* y, int y_dtype, int* nframes, double* vad, int* update, void* ws,
                  void* stream);

/* ---- on-the-fly additive noise (the reference's Additive, utils.py:43-297)
 * fp64 arithmetic on fp32 rows x / clean [rows][T], row r restricted to its first lengths[r]
 * samples (device int[rows], clamped to 0 .. T; NULL: all T).  One workgroup per row, no atomics:
 * a row's result depends on neither the other rows nor its position.
 *   segan_asl_p56: ITU-T P.56 method-B active speech level (utils.py:180-297).  Envelope q = two
 *     cascaded filters y[n] = (1-g)|x[n]| + g y[n-1], g = exp(-1/(0.03 srate)); thresholds c_j =
 *     2^(j-15), j = 0 .. nbits-2; counts[r][j] = samples at most ceil(0.2 srate) after a sample
 *     with q >= c_j (the reference's hangover loop); then the reference's finalisation and
 *     bin_interp, bounded to 1000 iterations.  nbits must be 16 (otherwise -3, unsupported).
 *     level[rows][4] = (sq = sum x^2, asl_ms, asl, c0), c0 NaN and asl_ms = asl = 0 where the
 *     reference returns (0, 0, None); counts int[rows][15]; status int[rows], bit 0 = iteration
 *     cap reached; q (optional, may be NULL) double[rows][T], zero past the row's length.
 *   segan_additive_mix (utils.py:98-134 and 89-95): segment = bank[starts[r] .. + len) of the flat
 *     fp32 noise bank of n_bank samples, Pn = its mean square, sf = sqrt(px[r] / Pn /
 *     10^(snr_db[r]/10)), v = clean + sf*segment; while max(v) >= 1 or min(v) < -1 every sample is
 *     divided by 1.1, then 1.2, ... (n successive fp64 divisions), then rounded to fp32 once.
 *     starts int64[rows], snr_db / px double[rows] are device arrays.  prev / prev_out (both or
 *     neither): float[rows], the clean sample preceding each row, mixed with bank[starts[r] - 1]
 *     and divided the same way (for a pre-emphasis that follows).  noisy[rows][T] (clean past the
 *     row's length); info double[rows][2] = (Pn, sf); istat int[rows][2] = (n, status): bit 0 =
 *     division cap (1000) reached, bit 1 = Pn == 0, bit 2 = segment (or starts[r] - 1 with prev)
 *     outside the bank; with bit 1 or 2 sf = 0 and the bank is not read.  px == 0 gives sf = 0. */
int segan_asl_p56(const float* x, const int* lengths, int rows, int T, int srate, int nbits,
                  double* level, int* counts, int* status, double* q, void* stream);
int segan_additive_mix(const float* clean, const int* lengths, const float* bank, int64_t n_bank,
                       const int64_t* starts, const double* snr_db, const double* px,
                       const float* prev, int rows, int T, float* noisy, float* prev_out,
                       double* info, int* istat, void* stream);
/* The mixer inside the pcm16 loader.  index (device int[n], NULL: 0 .. n-1) names the batch items
 * 0 .. B-1 that rows 0 .. n-1 stand for; n <= 65535.
 *   segan_pcm16_wave: wave[n][T] = the clean row of pcm[B][2][T+1] (segan_pcm16_prep's layout)
 *     normalised (2/65535)(x-32767)+1 and rounded to fp32, prev[n] = the same of the row's
 *     element 0 (the wav sample preceding the slice);
 *   segan_preemph_rows: y[index[k]][t] = x[k][t] - coef*x[k][t-1] (x[k][-1] = prev[k]) in double,
 *     rounded once; y[.][0] = x[k][0] where first[index[k]] is set; coef <= 0 copies.  x [n][T],
 *     y [B][T]: only the indexed rows of y are written. */
int segan_pcm16_wave(const int16_t* pcm, const int* index, float* wave, float* prev, int n, int B,
                     int T, void* stream);
int segan_preemph_rows(const float* x, const float* prev, const unsigned char* first,
                       const int* index, float* y, int n, int B, int T, double coef, void* stream);

/* ---- sample-rate conversion (the reference's librosa.load(path, 16000), se_dataset.py:72,408, or
 * an offline sox pass) -----------------------------------------------------
 * Rows of audio converted by p / q = rate_out / rate_in (lowest terms), fp64 arithmetic.  The
 * filter is scipy.signal.resample_poly's: mx = max(p, q), lh = zeros*mx, h[t] = sinc(t / mx) *
 * kaiser(2 lh + 1, beta)[t + lh] for t = -lh .. lh, taps G[t] = p h[t] / sum(h).  Row r holds
 * Lx = lengths[r] samples (device int[rows], clamped to 0 .. T; NULL: all T) and yields
 * Ly = ceil(Lx p / q) outputs y[m] = sum_n x[n] G[m q - n p] over |m q - n p| <= lh, 0 <= n < Lx
 * (ascending n); outputs from Ly to Ly_max are zero.  Equal rates are the identity (p = q = 1, one
 * tap 1.0).  (zeros, beta) = (10, 5.0) is scipy's default filter and the one STOI uses; the package's
 * default is (32, 8.6).  sum(h) is taken in index order, as segan_stoi_plan takes it (towards 10 kHz at
 * (10, 5.0) the taps are then its taps bit for bit), unless that order's rounding moves a tap by more
 * than 1e-15: then a compensated sum normalises, and the taps stay within 1e-15 of the exact filter.
 * Limits: rates 4000 .. 192000 Hz, zeros 1 .. 64, beta 0 .. 20, max(p, q) <= 4096, Ly <= 2^30:
 * outside them -3 (unsupported); -1 for arguments that are no rates, counts, finite non-negative
 * beta, dtypes or sizes at all.  Both are reported before anything is launched.
 *   segan_resample_plan (host only, no device): pq[2] = (p, q); *ntaps = 2 lh + 1 taps, written to
 *     taps when it is not NULL (cap >= *ntaps).
 *   segan_resample_dims (host only): dims[2] = (Ly for rows of T samples, the kernel's output tile:
 *     one workgroup computes that many consecutive outputs of one row).
 *   segan_resample: x [rows][T] of x_dtype (SEGAN_DT_F32, or SEGAN_DT_I16 with the values used as
 *     they are) -> y [rows][Ly_max] of y_dtype (SEGAN_DT_F64; SEGAN_DT_F32, rounded once from the
 *     fp64 sum; SEGAN_DT_I16, rounded half to even and saturated to -32768 .. 32767, never
 *     wrapped).  Ly_max >= the Ly of T.  out_lengths (optional) int[rows] = each row's Ly.  nclip
 *     (optional) int[rows] = the row's saturated samples (0 unless y is int16); counting them needs
 *     the workspace ws, int[rows * ceil(Ly_max / tile)] (may be NULL otherwise).  The polyphase
 *     tap table is built and uploaded on the first call per (device, p, q, zeros, beta) and kept.
 *     No atomics; a row's result is bitwise independent of the other rows and of its position. */
#define SEGAN_DT_F32 0
#define SEGAN_DT_I16 1
#define SEGAN_DT_F64 2
int segan_resample_plan(int rate_in, int rate_out, int zeros, double beta, int* pq, int* ntaps,
                        double* taps, int cap);
int segan_resample_dims(int T, int rate_in, int rate_out, int* dims);
int segan_resample(const void* x, int x_dtype, const int* lengths, int rows, int T, int rate_in,
                   int rate_out, int zeros, double beta, void* y, int y_dtype, int Ly_max,
                   int* out_lengths, int* nclip, int* ws, void* stream);

/* ---- on-the-fly reverberation (room impulse responses) ------------------
 * Row r of x [rows][T] is convolved with its own RIR h (L taps, direct path at tap d, h[d] = 1):
 *   y[n] = sum_{k < L} h[k] x[n + d - k],  n = -1 .. len_r - 1,
 * with x[-1] = prev[r] (0 without prev), x zero elsewhere outside 0 .. len_r - 1 (len_r =
 * lengths[r] clamped to 0 .. T; NULL: T).  y[-1] is returned as prev_out[r]; y[n] = 0 from len_r.
 * Uniformly partitioned overlap-save convolution: partition P = SEGAN_REVERB_P samples, transform
 * size 2P, both transforms as unsplit segan_gemm products against a shared basis.  A real 2P
 * spectrum is packed into 2P floats: column f = Re X[f] (f = 0 .. P), column P + f = Im X[f]
 * (f = 1 .. P-1).  No atomics: a row's result is bitwise independent of the other rows, of its
 * position and of the batch size.
 *   segan_reverb_dims (host only): dims[8] = (P, blocks per row NB, frames M of the two products,
 *     ceil(max_taps / P), floats of the staging buffer, of a spectrum buffer, of the inverse
 *     transform, of the whole workspace of segan_reverb_rows).  NB depends on T and max_delay only.
 *   segan_reverb_basis: fwd [2P][2P] (time x column) and inv [2P][P] (column x output P .. 2P-1),
 *     from fp64 sincospi of exactly reduced arguments.
 *   segan_reverb_bank: taps [n_parts][P] (every RIR zero-padded to whole partitions, concatenated)
 *     -> H [n_parts][2P], the spectra of the partitions zero-padded to 2P: 8 bytes per padded tap.
 *   table int[n_rirs][4] = (first partition, partitions, taps, d) per RIR; rir_ids int[rows].
 *   segan_reverb_stage: xs [(frames + 1) P]: a zero block, then per row NB blocks = (P-1 zeros,
 *     prev), x, zeros; frame g of the forward product starts at xs + g P (sam = P, sak = 1).
 *   segan_reverb_forward / segan_reverb_inverse: X [frames][2P] = frames x fwd; yt [frames][P] =
 *     Y x inv with the contraction in blocks of 64 added in order (one accumulator over all 2P
 *     terms of an inverse transform doubles the error against fp64).
 *   segan_reverb_fdl: Y[r, a] = sum_{b < partitions, b <= a} X[r, a-b] H[first + b], complex per
 *     bin, b ascending, X / Y [frames][2P] with frame r NB + a.
 *   segan_reverb_finish: y[r][n] = yt[r NB P + P + n + d], prev_out[r] (may be NULL) = the same at
 *     n = -1, status int[rows]: SEGAN_REVERB_ST_RIR = the id is outside the table, or the table
 *     entry is outside the bank of bank_parts partitions or inconsistent; SEGAN_REVERB_ST_DELAY =
 *     d exceeds the max_delay the blocks were sized for.  A flagged row reads nothing of the bank
 *     or the transforms: y = x, prev_out = prev.
 *   segan_reverb_rows: the whole chain (stage, product, delay line, product, finish) on `stream`;
 *     ws: workspace of dims[7] floats, 16-byte aligned.
 * Added without a change of SEGAN_ABI_VERSION: the exports are purely additive. */
#ifndef SEGAN_REVERB_P
#define SEGAN_REVERB_P 128   /* compile-time; the analytic start sqrt(L/2), not yet measured against 64 / 256 */
#endif
#define SEGAN_REVERB_ST_RIR 1
#define SEGAN_REVERB_ST_DELAY 2
#define SEGAN_REVERB_MAX_ROWS 32768
#define SEGAN_REVERB_MAX_FRAMES 8000000
int segan_reverb_dims(int rows, int T, int max_delay, int max_taps, int64_t* dims);
int segan_reverb_basis(float* fwd, float* inv, void* stream);
int segan_reverb_bank(const float* taps, int64_t n_parts, const float* fwd, float* H, void* stream);
int segan_reverb_stage(const float* x, const int* lengths, const float* prev, float* xs, int rows,
                       int T, int blocks, int frames, void* stream);
int segan_reverb_forward(const float* xs, const float* fwd, float* X, int frames, void* stream);
int segan_reverb_inverse(const float* Y, const float* inv, float* yt, int frames, void* stream);
int segan_reverb_fdl(const float* X, const float* H, int64_t bank_parts, const int* rir_ids,
                     const int* table, int n_rirs, float* Y, int rows, int T, int blocks,
                     int frames, void* stream);
int segan_reverb_finish(const float* yt, const float* x, const int* lengths, const float* prev,
                        int64_t bank_parts, const int* rir_ids, const int* table, int n_rirs,
                        float* y, float* prev_out, int* status, int rows, int T, int blocks,
                        int frames, void* stream);
int segan_reverb_rows(const float* x, const int* lengths, const float* prev, const float* H,
                      int64_t bank_parts, const int* rir_ids, const int* table, int n_rirs,
                      const float* fwd, const float* inv, int rows, int T, int max_delay, float* ws,
                      int64_t ws_floats, float* y, float* prev_out, int* status, void* stream);

/* ---- on-the-fly clipping, chunk removal and band limiting --------------
 * Three signal-level distortions of fp32 rows x [rows][T], row r restricted to its first
 * lengths[r] samples (device int[rows], clamped to 0 .. T; NULL: all T); rows <= 65535.  One
 * workgroup per row (per tile of SEGAN_FIR_TILE outputs for the FIR), no atomics, no scratch: a
 * row's result is bitwise independent of the other rows and of its position.  No product is
 * contracted with a sum.
 *   segan_clip_rows: m[r] = max |x[r][:len]| (exact), thr[r] = (float)((double)factor[r] *
 *     (double)m[r]) with factor double[rows] on the device, y = min(max(x, -thr), thr); samples
 *     from len on are copied.  prev / prev_out (both or neither) float[rows]: the sample preceding
 *     the row, clamped the same way; it takes no part in m.  nclipped int[rows] = samples of the
 *     row that changed.  status int[rows]: SEGAN_CLIP_ST_SILENT = m == 0 or len == 0,
 *     SEGAN_CLIP_ST_FACTOR = factor outside (0, 1] (thr = 0); a flagged row, and its prev, is
 *     copied unchanged.
 *   segan_chop_rows: sample t < len is active when q[r][t] >= c0[r] (q double[rows][T], c0
 *     double[rows]: the envelope and the threshold exactly as segan_asl_p56 writes them; no
 *     hangover); n = nactive[r] is their number.  Slot c < C <= SEGAN_CHOP_MAX with dur[r][c] > 0
 *     (int[rows][C], samples; <= 0: unused) takes k = min((long)floor(u[r][c] * (double)n), n - 1)
 *     (u double[rows][C] in [0, 1)) and starts[r][c] = the index of the k-th active sample from 0
 *     (-1 for an unused slot); y = 0 on the union of [start_c, min(start_c + dur_c, len)), x
 *     elsewhere; nzeroed[r] = the size of the union.  status: SEGAN_CHOP_ST_NOLEVEL = c0 is NaN or
 *     n == 0: the row is copied and every start is -1.  Integers throughout.
 *   segan_fir_rows: row r is filtered with filter ids[r] of bank double[nf][kmax + 1] (one-sided
 *     taps h[0 .. K[f]] of a symmetric filter, zeros after them; K int[nf]; kmax <=
 *     SEGAN_FIR_MAX_K): with xe[-1] = prev[r] (0 without prev), xe[t] = x[t] for 0 <= t < len, 0
 *     elsewhere,  y[n] = h[0] xe[n] + sum_{k = 1 .. K} h[k] (xe[n-k] + xe[n+k]),  n = -1 .. len-1,
 *     in fp64 with k ascending: the inner sum first, then the product, then the accumulation, each
 *     rounded on its own.  y[-1] goes to prev_out[r]; y[n] = 0 from len on.  y / prev_out are of
 *     y_dtype: SEGAN_DT_F64, or SEGAN_DT_F32 (rounded once from the fp64 sum).  status:
 *     SEGAN_FIR_ST_ID = the id is outside the bank (or its K outside 0 .. kmax): y = x, prev_out =
 *     prev.  A sample's sum does not depend on the tile it falls in.
 * Added without a change of SEGAN_ABI_VERSION: the exports are purely additive. */
#define SEGAN_CLIP_ST_SILENT 1
#define SEGAN_CLIP_ST_FACTOR 2
#define SEGAN_CHOP_MAX 8
#define SEGAN_CHOP_ST_NOLEVEL 1
#define SEGAN_FIR_TILE 1024
#define SEGAN_FIR_MAX_K 2048
#define SEGAN_FIR_ST_ID 1
int segan_clip_rows(const float* x, const int* lengths, const float* prev, const double* factor,
                    int rows, int T, float* y, float* prev_out, float* m, float* thr,
                    int* nclipped, int* status, void* stream);
int segan_chop_rows(const float* x, const int* lengths, const double* q, const double* c0,
                    const double* u, const int* dur, int rows, int T, int C, float* y, int* starts,
                    int* nactive, int* nzeroed, int* status, void* stream);
int segan_fir_rows(const float* x, const int* lengths, const float* prev, const double* bank,
                   const int* K, int nf, int kmax, const int* ids, int rows, int T, void* y,
                   int y_dtype, void* prev_out, int* status, void* stream);

/* ---- on-the-fly whispered speech: noise-excited LPC resynthesis -------
 * fp32 rows x [rows][T] at 16 kHz, row r restricted to its first lengths[r] samples (device
 * int[rows], clamped to 0 .. T; NULL: all T), prev float[rows] (NULL: zeros) the sample before the
 * row; rows <= 65535, T <= 2^30.  Index j = n + 1 (j = 0 is prev); frame f = 0 .. F-1, F = len /
 * SEGAN_WHISPER_H + 2, covers j in [(f-1) H, (f+1) H); Fmax = segan_whisper_frames(T) is the frame
 * stride of every per-frame array.  All arithmetic is fp64 with every operation rounded on its
 * own, in an order fixed by sample and frame index: no atomics, no scratch, a row's result is
 * bitwise independent of the other rows and of T beyond len.
 *   segan_whisper_noise: u[r][i] = the unit-variance noise sample j0 + i of seeds[r] (device
 *     long long[rows]): the four words of Philox4x32-10 at counter (lo32(J), hi32(J), 0, 0), J =
 *     j + 2^20, key (lo32(seed), hi32(seed)), summed as integers, less 2 (2^32 - 1), divided by
 *     sqrt((2^64 - 1) / 3).  -2^20 <= j0 <= 2^31.
 *   segan_whisper_lags: r [rows][Fmax][P + 1]: the lags 0 .. P of window[m] * xe over each frame
 *     (window double[N], lagwin double[P + 1], both on the device), times lagwin[l], r[0] times
 *     1.0001.  Frames from F on come out zero.
 *   segan_whisper_lpc: n sets of lags r [n][P + 1] -> a [n][P + 1] (a[0] = 1), sigma [n] = sqrt(E
 *     / 192), order int[n]: Levinson-Durbin, stopped at order m - 1 with the higher coefficients
 *     zero when k_m is not |k_m| < 1 or E has fallen to 2^-40 r[0].  r[0] <= 0 or NaN (a silent
 *     frame): a = [1, 0 ..], sigma = 0, order = 0.
 *   segan_whisper_synth: per frame, from zero state and after SEGAN_WHISPER_WU warm-up samples,
 *     v[j] = e[j] - a[P] v[j-P] - .. - a[1] v[j-1] with e[j] = (sigma (u[j] - tau u[j-1])) /
 *     sqrt(1 + tau tau), tau = tilts[r] (device double[rows]); window[m] v goes to ws (at least
 *     rows * N * Fmax doubles); y[j] = the earlier frame's share + the later one's, divided by
 *     peak[r] = max |y[0 .. len]| when that exceeds 1.  y[r][n] = y[n + 1], zero from len on, and
 *     prev_out[r] = y[0], of y_dtype (SEGAN_DT_F32, rounded once, or SEGAN_DT_F64).  status
 *     int[rows]: SEGAN_WHISPER_ST_SILENT = every frame of the row is silent,
 *     SEGAN_WHISPER_ST_TILT = tau outside [0, 1): the row and prev are copied, peak = 0.  nsilent
 *     int[rows] = silent frames below F; minorder int[rows] = the lowest order among the others
 *     (P without any).
 *   segan_whisper_rows: the three in turn on `stream`; ws holds segan_whisper_ws_doubles(rows, T).
 * Added without a change of SEGAN_ABI_VERSION: the exports are purely additive. */
#define SEGAN_WHISPER_N 512
#define SEGAN_WHISPER_H 256
#define SEGAN_WHISPER_P 16
#define SEGAN_WHISPER_WU 256
#define SEGAN_WHISPER_ST_SILENT 1
#define SEGAN_WHISPER_ST_TILT 2
int segan_whisper_frames(int T);
long long segan_whisper_ws_doubles(int rows, int T);
int segan_whisper_noise(const long long* seeds, long long j0, int count, int rows, double* u,
                        void* stream);
int segan_whisper_lags(const float* x, const int* lengths, const float* prev, const double* window,
                       const double* lagwin, int rows, int T, double* r, void* stream);
int segan_whisper_lpc(const double* r, long long n, double* a, double* sigma, int* order,
                      void* stream);
int segan_whisper_synth(const float* x, const int* lengths, const float* prev, const double* r,
                        const double* a, const double* sigma, const int* order,
                        const long long* seeds, const double* tilts, const double* window, int rows,
                        int T, double* ws, long long ws_doubles, void* y, int y_dtype,
                        void* prev_out, double* peak, int* status, int* nsilent, int* minorder,
                        void* stream);
int segan_whisper_rows(const float* x, const int* lengths, const float* prev,
                       const long long* seeds, const double* tilts, const double* window,
                       const double* lagwin, int rows, int T, double* ws, long long ws_doubles,
                       void* y, int y_dtype, void* prev_out, double* peak, int* status,
                       int* nsilent, int* minorder, void* stream);

/* ---- optimizers (model.py:219-228) ---------------------------------------------------- */
/* torch.optim.RMSprop (no momentum, not centered): sq = alpha*sq + (1-alpha)*g*g;
 * p -= lr * g / (sqrt(sq) + eps), over a flat arena of n floats. */
int segan_rmsprop_step(float* p, const float* g, float* sq, float lr, float alpha, float eps,
                       int64_t n, void* stream);
/* torch.optim.Adam without weight decay/amsgrad; `step` is the 1-based step count.  The betas
 * are doubles because torch forms 1 - beta and the bias corrections in double: 1 - beta2 taken
 * from an fp32 0.999 is 1.3e-5 off, and exp_avg_sq with it. */
int segan_adam_step(float* p, const float* g, float* m, float* v, float lr, double beta1,
                    double beta2, float eps, int step, int64_t n, void* stream);
int segan_fill(float* p, float value, int64_t n, void* stream);
int segan_scale(float* p, float s, int64_t n, void* stream);

/* ---- data-parallel exchange (the reference has none: README.md:79) --------
 * One communicator per process (= per GPU) over RCCL, bound at run time (dlopen of librccl.so.1:
 * a host process that already carries an RCCL, e.g. PyTorch-ROCm, keeps exactly one copy).  The
 * communicator is the only library-owned resource.  Rendezvous: rank 0 calls
 * segan_comm_unique_id, ships the segan_comm_id_bytes() bytes to the other ranks over any side
 * channel, then every rank calls segan_comm_init (a collective) with its device current.
 * segan_allreduce: in-place SUM over ranks of n floats followed by * scale (1/world = the mean
 * of the per-rank gradients: D 25.8 M floats between the D backward passes and its optimizer
 * step, G 64.8 M floats between the G backward and its step — or bucket by bucket from inside
 * the backward), enqueued on `stream`, asynchronous w.r.t. the host.  segan_broadcast: rank
 * `root`'s n floats to all (initial weights).  segan_allgather: recv[world][n] <- send[n]
 * (synchronised-BatchNorm partial statistics). */
int segan_comm_id_bytes(void);
int segan_comm_unique_id(void* id_out);
int segan_comm_init(void** comm_out, int world, int rank, const void* id);
int segan_comm_destroy(void* comm);
int segan_comm_rank(void* comm);
int segan_comm_world(void* comm);
int segan_allreduce(void* comm, float* buf, size_t n, float scale, void* stream);
int segan_broadcast(void* comm, float* buf, size_t n, int root, void* stream);
int segan_allgather(void* comm, const float* send, float* recv, size_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEGAN_HIP_H */
