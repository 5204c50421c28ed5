/* gridnext_hip.h - C ABI of libgridnext_hip.so: the MI355X (gfx950) kernels of GridNext's f∘g training path.
 *
 * The reference (adaly/gridnext) is pure Python on stock PyTorch and has NO FFI of its own; each entry point
 * below replaces the torch operator sequence at the cited reference location (paths relative to the reference
 * root).  Conventions:
 *   - plain C: device pointers + sizes + a stream handle (gnx_stream_t is HIP's hipStream_t); no torch types, no HIP include;
 *   - the caller owns every buffer (outputs and workspaces included); nothing is allocated, freed or cached
 *     across calls inside the library, kernels are enqueued on `stream` and the call returns immediately;
 *   - return value 0 = enqueued, <0 = error (GNX_ERR_*), never throws; re-entrant per stream;
 *   - activations are channels-last fp32 matrices X[rows][channels] with a leading dimension `ld*` in
 *     elements (rows = spots, or spots x H x W); labels are int64.
 */
#ifndef GRIDNEXT_HIP_H
#define GRIDNEXT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNX_OK 0
#define GNX_ERR_BAD_ARG (-1)
#define GNX_ERR_LAUNCH (-2)
#define GNX_ERR_UNSUPPORTED (-3)

typedef struct ihipStream_t* gnx_stream_t; /* HIP's own hipStream_t: an opaque pointer in plain C, the same type in HIP */

/* ---- corrector g: hexagonal convolution --------------------------------------------------------------------
 * Replaces hexagdly.Conv2d(kernel_size=1, stride=1, bias=True) as instantiated in
 * gridnext/gridnet_models.py:130-147 (any kernel_size: gnx_hexconv_k_* below).  x/y/dx/dy: [B][H][W][C] channels-last.  kernel0 [O][I][3][1],
 * kernel1 [O][I][2][2], bias [O] (hexagdly's parameter shapes).  mode 0: hexagdly addressing (odd columns
 * shifted down, gridnext/hexagdly_tools.py:68); mode 1: Visium odd-right grid, i.e. the
 * rot90/flip -> conv -> flip/rot90 sandwich of gridnet_models.py:178-185 without moving data.
 * Any I, O >= 1: up to 64 x 64 channels (weight gradient: 32 x 32) are one launch, wider layers are tiled over
 * channel chunks inside the call. */
int gnx_hexconv_fwd(const float* x, const float* kernel0, const float* kernel1, const float* bias, float* y,
                    int B, int H, int W, int I, int O, int mode, gnx_stream_t stream);
int gnx_hexconv_bwd_data(const float* dy, const float* kernel0, const float* kernel1, float* dx,
                         int B, int H, int W, int I, int O, int mode, gnx_stream_t stream);
long gnx_hexconv_bwd_weight_workspace(int B, int H, int W, int I, int O); /* floats */
int gnx_hexconv_bwd_weight(const float* x, const float* dy, float* dkernel0, float* dkernel1, float* dbias,
                           float* workspace, int B, int H, int W, int I, int O, int mode, int accumulate,
                           gnx_stream_t stream);
/* n hex layers' weight gradients as ONE launch plus one batched reduce - exactly gnx_hexconv_bwd_weight for every item, bit
 * for bit (same kernel body, slab layout, fixed-order reduce): the five hexagdly.Conv2d layers of the corrector
 * (gridnet_models.py:128-148) are independent once their output gradients exist and cost a launch apiece.  Layers wider than
 * 32 channels on either side, or more than 8 items: GNX_ERR_UNSUPPORTED, nothing launched (make the single calls).  `items`:
 * HOST array; each item's workspace: gnx_hexconv_bwd_weight_workspace(B, H, W, I, O) floats. */
typedef struct {
    const float* x; const float* dy; float* dkernel0; float* dkernel1; float* dbias; float* workspace;
    int B, H, W, I, O, mode, accumulate, pad;
} gnx_hexconv_wgrad_item;
int gnx_hexconv_bwd_weight_batch(const void* items, int n, gnx_stream_t stream);
/* Radius-k layers: hexagdly.Conv2d(in, out, kernel_size=k, stride=1) for k = 1 .. 8 (k > 8: GNX_ERR_UNSUPPORTED), the layer a
 * custom corrector puts in place of the size-1 ones of gridnet_models.py:130-147 (a subclass overriding _init_corrector, as
 * notebooks/register_concat.ipynb does); modes, layouts and channel counts as above.  `kernels` / `dkernels`: HOST arrays of
 * k + 1 device pointers in hexagdly's order, kernel0 [O][I][2k+1][1] and kernel{j} [O][I][2k+1-j][2] for j = 1..k: tap a of
 * kernel0 is (dp, dq) = (0, a - k), tap (a, b) of kernel{j} is (dp, dq) = ((2b - 1) j, top(j, p) + a) with
 * top(j, p) = -k + floor(j/2) + (j odd ? p mod 2 : 0) (p: the parity-axis coordinate - the column in mode 0, the Visium row in
 * mode 1; q: the other).  A NULL dkernels[j] or dbias: that gradient is not wanted, nothing is written there.  k = 1 gives
 * the size-1 entry points' results (other summation order).  Deterministic: no atomics. */
int gnx_hexconv_k_fwd(const float* x, const float* const* kernels, const float* bias, float* y,
                      int B, int H, int W, int I, int O, int k, int mode, gnx_stream_t stream);
int gnx_hexconv_k_bwd_data(const float* dy, const float* const* kernels, float* dx,
                           int B, int H, int W, int I, int O, int k, int mode, gnx_stream_t stream);
long gnx_hexconv_k_bwd_weight_workspace(int B, int H, int W, int I, int O, int k); /* floats */
int gnx_hexconv_k_bwd_weight(const float* x, const float* dy, float* const* dkernels, float* dbias, float* workspace,
                             int B, int H, int W, int I, int O, int k, int mode, int accumulate, gnx_stream_t stream);

/* ---- corrector g: Cartesian convolution ---------------------------------------------------------------------
 * Replaces nn.Conv2d(I, O, k, padding=k//2) as instantiated in gridnext/gridnet_models.py:51-66 (3x3, 5x5, 5x5, 3x3), for any
 * odd kh x kw with stride 1 and zero "same" padding: y[b,r,c,o] = bias[o] + sum_{a,b',i} weight[o,i,a,b'] *
 * x[b, r + a - kh/2, c + b' - kw/2, i] (cross-correlation, as torch; positions outside the array read zero).  x/y/dx/dy:
 * [B][H][W][C] channels-last; weight [O][I][kh][kw] (nn.Conv2d's own layout), bias [O] or NULL.  Any I, O >= 1, chunked as the
 * hex entry points.  An even kh or kw: GNX_ERR_BAD_ARG; kh * kw > 217 (the taps of the radius-8 hex layer):
 * GNX_ERR_UNSUPPORTED, nothing launched.  A NULL dweight or dbias: that gradient is not wanted, nothing is written there.
 * Deterministic: no atomics. */
/* forward of the corrector's nn.Conv2d layers, gridnext/gridnet_models.py:51-66 */
int gnx_gridconv_fwd(const float* x, const float* weight, const float* bias, float* y,
                     int B, int H, int W, int I, int O, int kh, int kw, gnx_stream_t stream);
/* their data gradient (autograd of gridnext/gridnet_models.py:51-66) */
int gnx_gridconv_bwd_data(const float* dy, const float* weight, float* dx,
                          int B, int H, int W, int I, int O, int kh, int kw, gnx_stream_t stream);
/* workspace of gnx_gridconv_bwd_weight, gridnext/gridnet_models.py:51-66 */
long gnx_gridconv_bwd_weight_workspace(int B, int H, int W, int I, int O, int kh, int kw); /* floats */
/* their weight and bias gradient (autograd of gridnext/gridnet_models.py:51-66): one slab per 64 positions, fixed-order reduce */
int gnx_gridconv_bwd_weight(const float* x, const float* dy, float* dweight, float* dbias, float* workspace,
                            int B, int H, int W, int I, int O, int kh, int kw, int accumulate, gnx_stream_t stream);

/* ---- batch normalisation (+ReLU) over matrix rows -----------------------------------------------------------
 * nn.BatchNorm2d(32) of the corrector (gridnet_models.py:134-146) and nn.BatchNorm1d of the count MLP
 * (notebooks/Tutorial_visium_count.ipynb cell 12), torch semantics (biased var to normalise, unbiased for
 * running_var, momentum, num_batches_tracked). */
long gnx_bn_workspace(long M, int C); /* floats, for train_stats / relu_bwd / colsum */
int gnx_bn_train_stats(const float* x, long ld, long M, int C, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, long long* num_batches_tracked, float momentum,
                       float eps, float* scale, float* shift, float* save_mean, float* save_invstd,
                       float* workspace, gnx_stream_t stream);
/* The same with the layer's persistent sync words (gnx_bn_sync_words; see gnx_bn_train_stats_apply_sync): the form that puts
 * several workgroups on a channel block then needs no memset node in front of it.  sync == NULL: exactly gnx_bn_train_stats. */
int gnx_bn_train_stats_sync(const float* x, long ld, long M, int C, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, long long* num_batches_tracked, float momentum,
                       float eps, float* scale, float* shift, float* save_mean, float* save_invstd,
                       float* workspace, void* sync, gnx_stream_t stream);
/* gnx_bn_train_stats + gnx_scale_shift_relu in one call (one launch for matrices of up to 4992 rows: g's BatchNorm2d(32)
 * over one Visium grid, gridnet_models.py:134-146; the count MLP's BatchNorm1d). */
int gnx_bn_train_stats_apply(const float* x, long ld, long M, int C, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, long long* num_batches_tracked, float momentum,
                             float eps, float* scale, float* shift, float* save_mean, float* save_invstd, float* y, long ldy,
                             int relu, float* workspace, gnx_stream_t stream);
int gnx_bn_fold_eval(int C, const float* gamma, const float* beta, const float* running_mean,
                     const float* running_var, float eps, float* scale, float* shift, float* save_mean,
                     float* save_invstd, gnx_stream_t stream);
int gnx_scale_shift_relu(const float* x, long ldx, float* y, long ldy, long M, int C, const float* scale,
                         const float* shift, int relu, gnx_stream_t stream);
/* relu: 0 = plain BN, 1 = BN -> ReLU with x the BN input, 2 = BN -> ReLU with x holding the ACTIVATED output
 * relu(scale x + shift) (eval statistics only, scale != 0: the forward stored the bottleneck that way; needs 4 | C, 4 | ld* and
 * 16-B aligned pointers, GNX_ERR_UNSUPPORTED otherwise and with training != 0).  dx, dgamma, dbeta may be NULL.  Every leading
 * dimension must be >= C (lddx only where dx is given): GNX_ERR_BAD_ARG, as for M <= 0, C <= 0 or a NULL required pointer. */
int gnx_bn_relu_bwd(const float* dy, long lddy, const float* x, long ldx, float* dx, long lddx, long M, int C,
                    const float* scale, const float* shift, const float* save_mean, const float* save_invstd,
                    float* dgamma, float* dbeta, int relu, int training, int accumulate, int dx_accumulate,
                    float* workspace, gnx_stream_t stream);
/* Round 5 - matrices of 2049 ... 8192 rows (one 78 x 64 Visium grid: the corrector's two BatchNorm2d(32), gridnet_models.py:131-140,
 * and the count MLP's BatchNorm1d; dense block 2 of a batch of 32 patches) run gnx_bn_train_stats[_apply] / gnx_bn_relu_bwd with
 * FOUR workgroups per 16-channel block: a row lane keeps its <= 8 rows in registers (one round of loads for all walks) and the
 * four partial sums are exchanged behind a bounded barrier of those workgroups (added in workgroup order: deterministic; two-pass
 * variance as before).  The barrier's counters live in the workspace and are zeroed by a memset node per call - or, with the
 * `_sync` entry points, in gnx_bn_sync_words(C) 32-bit words the caller zeroed ONCE and keeps for this layer (never shared by
 * launches that may overlap): the kernels leave them zero, no memset node is needed.  sync == NULL: the plain entry points. */
long gnx_bn_sync_words(int C);
int gnx_bn_train_stats_apply_sync(const float* x, long ld, long M, int C, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, long long* num_batches_tracked, float momentum,
                                  float eps, float* scale, float* shift, float* save_mean, float* save_invstd, float* y, long ldy,
                                  int relu, float* workspace, void* sync, gnx_stream_t stream);
int gnx_bn_relu_bwd_sync(const float* dy, long lddy, const float* x, long ldx, float* dx, long lddx, long M, int C,
                         const float* scale, const float* shift, const float* save_mean, const float* save_invstd, float* dgamma,
                         float* dbeta, int relu, int training, int accumulate, int dx_accumulate, float* workspace, void* sync,
                         gnx_stream_t stream);
/* Transitions (norm -> relu -> conv 1x1 -> avgpool 2x2, densenet.py:47-54, run pool-first): gnx_bnrelu_avgpool2 = the pooled,
 * activated input [imgs*(S/2)^2][C] of the 1x1 conv (operand of its weight gradient); gnx_bn_relu_bwd_pooled = the adjoint
 * of norm -> relu given the gradient of the POOLED map (== gnx_avgpool2_bwd + gnx_bn_relu_bwd(relu = 1, training = 0)
 * without the full-size intermediate).  Eval statistics; 4 | C, 4 | ld*, 16-B aligned pointers (GNX_ERR_UNSUPPORTED otherwise).
 * The pool is torch's floor pool: gnx_bn_relu_bwd_pooled takes any S >= 2 (the last row and column of an odd map get dx = 0 and
 * add nothing to dgamma / dbeta); gnx_bnrelu_avgpool2 takes even S only (GNX_ERR_UNSUPPORTED for an odd one). */
int gnx_bnrelu_avgpool2(const float* in, long ldi, float* out, long ldo, long imgs, int C, int S, const float* scale,
                        const float* shift, gnx_stream_t stream);
int gnx_bn_relu_bwd_pooled(const float* dYp, long lddy, const float* x, long ldx, float* dx, long lddx, long imgs, int S,
                           int C, const float* scale, const float* shift, const float* save_mean,
                           const float* save_invstd, float* dgamma, float* dbeta, int accumulate, float* workspace,
                           gnx_stream_t stream);
int gnx_colsum(const float* x, long ld, long M, int C, float* out, int accumulate, float* workspace,
               gnx_stream_t stream);

/* ---- foreground-masked softmax cross-entropy + argmax/accuracy ------------------------------------------------
 * The permute/reshape/boolean-gather/labels-1/CrossEntropyLoss/torch.max chain of gridnext/training.py:152-160,
 * :176-177 (label_base 1) and the plain CE + argmax of :61-62 (label_base 0).  stats = {n_counted, n_correct}. */
long gnx_masked_ce_workspace(long M); /* doubles */
int gnx_masked_ce_fwd(const float* logits, long ld, const long long* labels, long M, int C, int label_base,
                      float accum_iters, float* loss, long long* stats, long long* preds, double* workspace,
                      gnx_stream_t stream);
int gnx_masked_ce_bwd(const float* logits, long ld, const long long* labels, long M, int C, int label_base,
                      const long long* stats, const float* dloss, float accum_iters, float* dlogits, long lddz,
                      gnx_stream_t stream);
/* The same chain for a criterion with options: the `criterion` argument of gridnext/training.py:11 and :101, applied at :61
 * and :159, when it is nn.CrossEntropyLoss(weight, ignore_index, reduction, label_smoothing) with class-index targets.  A row is
 * selected iff label >= label_base, y = label - label_base; a selected row with y == ignore_index is ignored.  weight: C
 * device floats or NULL (all ones); label_smoothing e in [0, 1]; reduction 0 = 'mean', 1 = 'sum' (anything else, or e outside
 * [0, 1]: GNX_ERR_BAD_ARG).  With lp = log_softmax(z) and S = the selected, not ignored rows:
 *   num = sum_{i in S} [(1-e) w[y_i] (-lp[i,y_i]) + (e/C) sum_c w[c] (-lp[i,c])],  den = sum_{i in S} w[y_i] ('mean') | 1 ('sum'),
 *   loss = num / den / accum_iters  (den == 0 under 'mean': NaN, as torch; 'sum' over nothing: 0),
 *   dz[i,c] = (p[i,c] a_i - t[i,c]) dloss / (den accum_iters) on S, 0 elsewhere, a_i = (1-e) w[y_i] + (e/C) sum_c w[c],
 *   t[i,c] = (1-e) w[y_i] [c == y_i] + (e/C) w[c].
 * stats = {n_selected, n_correct} and preds ignore weight, smoothing and ignore_index (ignored rows count in both).  `den`: one
 * device double the forward writes and the backward reads (no host read-back).  y >= C on a row of S: loss (and that row's dz)
 * NaN, nothing read out of bounds.  Deterministic: fixed-order two-stage sums in double.  Workspace: doubles. */
long gnx_masked_ce_opt_workspace(long M); /* doubles */
int gnx_masked_ce_opt_fwd(const float* logits, long ld, const long long* labels, long M, int C, int label_base,
                          const float* weight, float label_smoothing, long long ignore_index, int reduction,
                          float accum_iters, float* loss, long long* stats, double* den, long long* preds,
                          double* workspace, gnx_stream_t stream);
int gnx_masked_ce_opt_bwd(const float* logits, long ld, const long long* labels, long M, int C, int label_base,
                          const float* weight, float label_smoothing, long long ignore_index, int reduction,
                          const double* den, const float* dloss, float accum_iters, float* dlogits, long lddz,
                          gnx_stream_t stream);
/* The loops' per-batch bookkeeping (training.py:73-75, :176-178: running_loss += loss.item() * batch_size; running_corrects +=
 * correct) on device-resident sums, one launch: acc[0] += (double)*loss * weight, acc[1] += *correct, acc[2] += counted ?
 * *counted : counted_const (acc: 3 doubles on the device; loss / correct / counted: device scalars as gnx_masked_ce_fwd
 * leaves them). */
int gnx_meter_add(double* acc, const float* loss, double weight, const long long* correct, const long long* counted,
                  double counted_const, gnx_stream_t stream);

/* Row softmax + first-argmax of channels-last logits: torch.argmax / F.softmax of gridnext/utils.py:43-47. */
int gnx_softmax_rows(const float* logits, long ld, long M, int C, float* probs, long ldp, long long* preds,
                     gnx_stream_t stream);

/* ---- multi-tensor Adam / AdamW step ------------------------------------------------------------------------------
 * The `optimizer.step()` calls of gridnext/training.py:67 (train_spotwise) and :167-170 (train_gridwise: g's optimizer and
 * the optional f_opt), which the tutorials build as optim.Adam(model.parameters(), lr=...).  Per element, torch's
 * single-tensor order: g = grad + weight_decay * p (decoupled: p *= 1 - lr * weight_decay first, g = grad);
 * m += (g - m) * (1 - beta1); v = beta2 * v + (1 - beta2) * g * g; p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps) with
 * bc = 1 - beta^t in double, t = the tensor's own float32 step count, incremented on the device (no host read-back).
 * p, grad, m, v, step: HOST arrays of n device pointers (4-byte alignment suffices), numel: host array of n element counts
 * (0 allowed), coef: 2 * n device floats of workspace.  The pointer table travels as kernel arguments, gnx_adam_table_tensors()
 * tensors per launch pair (a one-block step-count prologue, then one block per gnx_adam_chunk() elements): capturable; a
 * replay is valid while the addresses stand.  Hyperparameters are taken by value at every call. */
long gnx_adam_table_tensors(void);
long gnx_adam_chunk(void);
int gnx_adam_step(float* const* p, const float* const* grad, float* const* m, float* const* v, float* const* step,
                  const long* numel, int n, float* coef, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int decoupled, gnx_stream_t stream);

/* ---- count-MLP spot head: fp32 MFMA GEMM -------------------------------------------------------------------------
 * F.linear forward / input-gradient / weight-gradient of the nn.Sequential in Tutorial_visium_count.ipynb cell 12.
 * C[M][N] = opA(A) opB(B) (+bias) (+C).  a_kmajor: A[k*lda+m] (a (genes, H*W) count grid read in place, replacing
 * the permute+copy of gridnet_models.py:167-169); b_kmajor: B[k*ldb+n].
 * GNX_ERR_BAD_ARG (nothing launched): a NULL A / B / C, K <= 0, M < 0, N < 0, ldc < N, or a leading dimension below the
 * operand's contiguous extent - lda < K (row-major A) resp. lda < M (K-major A), ldb < K resp. ldb < N.  M == 0 or N == 0
 * is GNX_OK and writes nothing. */
int gnx_gemm_f32(const float* A, long lda, int a_kmajor, const float* B, long ldb, int b_kmajor, const float* bias,
                 float* C, long ldc, long M, long N, long K, int accumulate, gnx_stream_t stream);
/* The same product given `workspace` (gnx_gemm_f32_workspace(M, N, K) floats; NULL allowed when that is 0): the
 * 2000 -> 500 layer over a whole grid (gridnet_models.py:83-86 runs f on all 4992 B positions) then splits K over
 * workgroups and sums the partial tiles in a fixed order. */
long gnx_gemm_f32_workspace(long M, long N, long K);
int gnx_gemm_f32_ws(const float* A, long lda, int a_kmajor, const float* B, long ldb, int b_kmajor, const float* bias,
                    float* C, long ldc, long M, long N, long K, int accumulate, float* workspace, gnx_stream_t stream);

/* ---- DenseNet-BC image spot classifier, forward (gridnext/densenet.py) ------------------------------------------------
 * conv1x1_bnrelu : _DenseLayer norm1->relu1->conv1 (:35-40) and _Transition norm->relu->conv->pool (:47-54, pool=1)
 * conv3x3_bnrelu : _DenseLayer norm2->relu2->conv2 (:41); weights repacked by gnx_repack_conv3x3 to [tap][N][K]
 * conv_stem      : features.conv0 (:98-105), NCHW patches in, channels-last out
 * bnrelu_maxpool : norm0->relu0->pool0 (:106-110);  bnrelu_avgpool : norm_final->relu->adaptive_avg_pool (:153-156) */
int gnx_conv1x1_bnrelu(const float* A, long lda, const float* W, float* out, long ldc, long M, int N, int K,
                       const float* scale, const float* shift, int pool, int S_in, gnx_stream_t stream);
/* The same (pool = 0) given `workspace` (gnx_conv1x1_workspace(M, N, K) floats; 0 = the shape does not split, NULL allowed):
 * on matrices of few 128-row tiles - a batch of 32 patches, train_spotwise at the tutorial's batch size (training.py:11-98) -
 * the K range is split over workgroups and the partial tiles are summed in a fixed order. */
long gnx_conv1x1_workspace(long M, int N, int K);
int gnx_conv1x1_bnrelu_ws(const float* A, long lda, const float* W, float* out, long ldc, long M, int N, int K,
                          const float* scale, const float* shift, float* workspace, gnx_stream_t stream);
/* conv1x1_bnrelu_act: conv1x1_bnrelu (pool = 0) storing relu(out_scale[n] * y + out_shift[n]) -- _DenseLayer's norm2->relu2
 * (:38-39) folded into conv1's store in eval mode, so conv2 reads a ready operand (scale = shift = NULL below). */
int gnx_conv1x1_bnrelu_act(const float* A, long lda, const float* W, float* out, long ldc, long M, int N, int K,
                           const float* scale, const float* shift, const float* out_scale, const float* out_shift,
                           gnx_stream_t stream);
/* Opt-in form of conv1x1_bnrelu_act / conv1x1_bnrelu (pool = 0) for N = 128 on SPLIT bf16 operands (csrc/conv1x1_split.hip): every
 * fp32 operand = hi + lo in bf16, a product = three v_mfma_f32_32x32x16_bf16 with fp32 accumulation (a_lo b_hi + a_hi b_lo +
 * a_hi b_hi); tensors stay fp32 in HBM.  A whole DenseNet-121 in this arithmetic: logits 7e-6 of their range, CE 1e-6 from float64
 * (tools/diag/split_operand_feasibility.py).  Wp = gnx_conv1x1_split_pack of conv1.weight [128][K]
 * (gnx_conv1x1_split_pack_halves(K) 16-bit elements).  out_scale = NULL: no activation on the store.  4 | K, 4 | lda, 16-B aligned
 * A / scale / shift, else GNX_ERR_UNSUPPORTED. */
long gnx_conv1x1_split_pack_halves(int K);
int gnx_conv1x1_split_pack(const float* W, void* Wp, int K, gnx_stream_t stream);
int gnx_conv1x1_bnrelu_act_split(const float* A, long lda, const void* Wp, float* out, long ldc, long M, int K,
                                 const float* scale, const float* shift, const float* out_scale, const float* out_shift,
                                 gnx_stream_t stream);
/* The 3x3 companion (csrc/conv3x3_split.hip): conv2 (:41; N = 32, K = 128, padding 1) on an fp32 bottleneck that conv1 stored
 * activated, as nine shifted products of split bf16 operands - gnx_conv3x3_bnrelu with scale = shift = NULL in fp32-grade
 * arithmetic, bound by the bottleneck's bytes instead of the fp32 matrix instruction.  Wp = gnx_conv3x3_split_pack of
 * conv2.weight [32][128][3][3] (gnx_conv3x3_split_pack_halves() 16-bit elements).  S in {4, 8, 16, 32, 64}, S * S | M, 4 | lda,
 * 16-B aligned A, else GNX_ERR_UNSUPPORTED. */
long gnx_conv3x3_split_pack_halves(void);
int gnx_conv3x3_split_pack(const float* W, void* Wp, gnx_stream_t stream);
int gnx_conv3x3_split(const float* A, long lda, const void* Wp, float* out, long ldc, long M, int S, gnx_stream_t stream);
/* conv1's weight gradient on split bf16 operands (csrc/wgrad_split.hip; opt-in): gnx_wgrad_bnrelu with taps = 1, pool = 0 -
 * dW [N][K] (+)= dY^T relu(scale . X + shift) as torch.autograd derives it for densenet.py:35-37 - with fp32 operands in HBM, three
 * 16-bit matrix instructions per product and fp32 accumulation; slabs over pixels summed in a fixed order.  scale = shift = NULL: no
 * activation.  4 | N, K, lddy, ldx and 16-B aligned operands, else GNX_ERR_UNSUPPORTED. */
long gnx_wgrad1x1_split_workspace(long M, int N, int K);
int gnx_wgrad1x1_split(const float* dY, long lddy, const float* X, long ldx, const float* scale, const float* shift, float* dW,
                       float* workspace, long M, int N, int K, int accumulate, gnx_stream_t stream);
/* ... and conv2's (taps = 9, N = 32, K = 128, no prologue: A is the activated bottleneck, dY the layer's 32 gradient columns; dW in
 * conv2.weight's layout [32][128][3][3]).  S in {4, 8, 16, 32, 64}, S * S | M, 4 | lddy, lda, 16-B aligned operands. */
long gnx_wgrad3x3_split_workspace(long M);
int gnx_wgrad3x3_split(const float* dY, long lddy, const float* A, long lda, float* dW, float* workspace, long M, int S,
                       int accumulate, gnx_stream_t stream);
/* Training backward of norm1 -> relu1 -> conv1 (:35-37) w.r.t. the layer input, eval statistics: conv1's data gradient
 * dY . Wt^T (Wt = gnx_transpose_weight of conv1.weight) fused with the BN + ReLU backward and accumulated into the block
 * gradient dX[:, :N]; dbeta / dgamma from per-tile column sums (fixed order).  Same result as gnx_conv1x1_bnrelu followed by
 * gnx_bn_relu_bwd(relu = 1, training = 0, dx_accumulate = 1).  Whole tiles only, else GNX_ERR_UNSUPPORTED. */
long gnx_conv1x1_dgrad_bn_workspace(long M, int N);
int gnx_conv1x1_dgrad_bnrelu_bwd(const float* dY, long lddy, const float* Wt, const float* X, long ldx, float* dX, long lddx,
                                 long M, int N, int K, const float* scale, const float* shift, const float* mean,
                                 const float* invstd, float* dgamma, float* dbeta, int accumulate, float* workspace,
                                 gnx_stream_t stream);
/* The same pass ALSO producing conv1's weight gradient dW[K][N] (= gnx_wgrad_bnrelu(taps = 1) with the forward's BN + ReLU
 * prologue) from the tiles it stages: one pass over dY, X and dX instead of two (round 4).  Argument names as above, but with
 * N = 128 bottleneck channels fixed: dB [M][128] (lddb), W1t = conv1.weight transposed [K][128], G = the block gradient
 * (+= in columns [0, K)), 32 | K.  workspace: gnx_conv1x1_dgrad_wgrad_workspace(M, K) floats. */
long gnx_conv1x1_dgrad_wgrad_workspace(long M, int K);
int gnx_conv1x1_dgrad_wgrad_bnrelu_bwd(const float* dB, long lddb, const float* W1t, const float* X, long ldx, float* G, long ldg,
                                       long M, int K, const float* scale, const float* shift, const float* mean,
                                       const float* invstd, float* dgamma, float* dbeta, float* dW, float* workspace,
                                       int accumulate, gnx_stream_t stream);
/* Which kernel body a call runs ("conv1 forms"; tests/conv1_ref.py restates the dispatch).  gnx_conv1x1_form answers
 * for gnx_conv1x1_bnrelu (out_scale = out_shift = workspace = NULL), gnx_conv1x1_bnrelu_ws (pool = S_in = 0) and
 * gnx_conv1x1_bnrelu_act (pool = S_in = 0, workspace = NULL) with a GNX_C1_* code; *workgroups = the grid's x size, *splits = the z
 * size of the K-split launch (0 when not split); both may be NULL.  gnx_conv1x1_dgrad_bnrelu_bwd_form returns the producer waves
 * per workgroup (4) of the fused data gradient.  Nothing is launched, no operand is read - only the pointers' NULL-ness and
 * alignment count.  A call that returns an error: that GNX_ERR_* and 0 workgroups; M == 0: the default form, 0 workgroups. */
#define GNX_C1_GENERIC 0     /* conv1x1_kernel<pool 0, fast 0>: any alignment, any K */
#define GNX_C1_GENERIC_VEC 1 /* <0, 1>: 16-B aligned A / W / scale / shift, 4 | lda, 4 | K */
#define GNX_C1_POOL 2        /* <1, 0> */
#define GNX_C1_POOL_VEC 3    /* <1, 1> */
#define GNX_C1_SPLIT 4       /* K split over blockIdx.z into the workspace + conv1x1_split_reduce_kernel */
#define GNX_C1_WS 5          /* persistent conv1x1_ws_kernel: 128 | M, 32 | N, 32 | K <= 2048, leading dimensions < 65536 */
#define GNX_C1_WS_ACT 6      /* ... with the BN + ReLU prologue */
#define GNX_C1_WS_POOL 7     /* ... pooling producers (prologue required, even S_in) */
int gnx_conv1x1_form(const float* A, long lda, const float* W, const float* out, long ldc, long M, int N, int K,
                     const float* scale, const float* shift, int pool, int S_in, const float* out_scale, const float* out_shift,
                     const float* workspace, int* workgroups, int* splits);
int gnx_conv1x1_dgrad_bnrelu_bwd_form(const float* dY, long lddy, const float* Wt, const float* X, long ldx, const float* dX,
                                      long lddx, long M, int N, int K, const float* scale, const float* shift, const float* mean,
                                      const float* invstd, const float* dgamma, const float* dbeta, int accumulate,
                                      const float* workspace, int* workgroups);
/* conv2's data gradient fused with norm2 -> relu2's adjoint (eval statistics; A_act = the ACTIVATED bottleneck the training
 * forward stored): dX = scale * g * [A_act > 0] with g = conv3x3(dY, Wb), dbeta / dgamma from the same pass.  Replaces
 * gnx_conv3x3_bnrelu(dY, Wb) + gnx_bn_relu_bwd(relu = 2) (torch.autograd through densenet.py:41).  N == 128, K == 32. */
long gnx_conv3x3_dgrad_bn_workspace(long M, int N); /* floats */
int gnx_conv3x3_dgrad_bnrelu_bwd(const float* dY, long lddy, const float* Wb, const float* A_act, long lda, float* dX,
                                 long lddx, long M, int N, int K, int S, const float* scale, const float* shift,
                                 const float* mean, const float* invstd, float* dgamma, float* dbeta, int accumulate,
                                 float* workspace, gnx_stream_t stream);
int gnx_repack_conv3x3(const float* w, float* wr, int N, int K, gnx_stream_t stream);
int gnx_conv3x3_bnrelu(const float* A, long lda, const float* Wr, float* out, long ldc, long M, int N, int K, int S,
                       const float* scale, const float* shift, gnx_stream_t stream);
/* conv2 (:41) of a pre-activated bottleneck with Winograd F(2,3) along x: 12 matrix "taps" per output pair instead of 18.
 * Same result as gnx_conv3x3_bnrelu(scale = shift = NULL) up to rounding; weights from gnx_winograd_conv3x3_weights
 * ([N][K][3][3] -> [3][4][N][K]).  GNX_ERR_UNSUPPORTED outside N == 32, 32 | K, S in {4, 8, 16, 32, 64}. */
int gnx_winograd_conv3x3_weights(const float* w, float* wu, int N, int K, gnx_stream_t stream);
int gnx_conv3x3_winograd(const float* A, long lda, const float* Wu, float* out, long ldc, long M, int N, int K, int S,
                         gnx_stream_t stream);
/* The same call on the 8-wave kernel (512-pixel tiles) whatever M: S = 16 or 32 only, GNX_ERR_UNSUPPORTED otherwise.  The same
 * bits as gnx_conv3x3_winograd, which runs this form from 262144 rows on (GNX_C3_WINO8); here for tests at small M. */
int gnx_conv3x3_winograd_wide(const float* A, long lda, const float* Wu, float* out, long ldc, long M, int N, int K, int S,
                              gnx_stream_t stream);
/* Which kernel a conv2 call runs, without launching it (the launchers act on the same decision; DESIGN.md, "conv2 forms").
 * gnx_conv3x3_form / gnx_conv3x3_winograd_form return a GNX_C3_* code, the other two the waves per workgroup (4 or 8) of the
 * persistent LDS-DMA kernel; *workgroups (may be NULL) receives the grid's x size.  Arguments as the call's (pointers count by
 * NULL-ness and alignment only, nothing is read).  A call that returns an error: that GNX_ERR_* and 0 workgroups; M == 0: 0
 * workgroups. */
#define GNX_C3_GENERIC 0 /* conv3x3_kernel: any alignment, any K, S >= 80 */
#define GNX_C3_PIPE5 1   /* register-pipelined, strip rows per thread 5: S <= 15 */
#define GNX_C3_PIPE6 2   /* 16 <= S <= 31 */
#define GNX_C3_PIPE7 3   /* 32 <= S <= 47 */
#define GNX_C3_PIPE9 4   /* 48 <= S <= 79 */
#define GNX_C3_DMA4 5    /* persistent LDS-DMA, 128-row tiles: no prologue, N == 32, 64 | K, 128 | M */
#define GNX_C3_DMA8 6    /* ... 256-row tiles: S <= 32, 256 | M, M >= 262144 */
#define GNX_C3_DMAG4 7   /* the same kernel in its data-gradient shape: K == 32, 64 | N */
#define GNX_C3_DMAG8 8
#define GNX_C3_WINO 9    /* Winograd F(2,3) along x, 4 waves, 256-pixel tiles (the last may be ragged) */
#define GNX_C3_WINO8 10  /* ... 8 waves, 512-pixel tiles: S = 16 or 32, M >= 262144 */
int gnx_conv3x3_form(const float* A, long lda, const float* Wr, const float* out, long ldc, long M, int N, int K, int S,
                     const float* scale, const float* shift, int* workgroups);
int gnx_conv3x3_winograd_form(const float* A, long lda, const float* Wu, const float* out, long ldc, long M, int N, int K, int S,
                              int* workgroups);
int gnx_conv3x3_dgrad_bnrelu_bwd_form(const float* dY, long lddy, const float* Wb, const float* A_act, long lda, const float* dX,
                                      long lddx, long M, int N, int K, int S, const float* scale, const float* shift,
                                      const float* mean, const float* invstd, const float* workspace, int* workgroups);
int gnx_conv3x3_f16_dma_form(const void* A16, long lda16, const void* Wr16, const void* out, long ldc, long M, int N, int K,
                             int S, int* workgroups);
/* The same for the BatchNorm, weight-gradient and GEMM launchers ("BatchNorm forms", "Weight-gradient forms", "GEMM forms",
 * DESIGN.md; tests/bn_ref.py, wgrad_ref.py and gemm_ref.py restate the dispatch).  Each query takes its entry point's arguments in
 * its order, without the stream; every out-pointer may be NULL; *workgroups = the workgroups of the call's first launch.  Nothing
 * is launched or set, no operand is read.  A call that returns an error: that GNX_ERR_* and 0 in every out value.
 * gnx_bn_train_stats_form: gnx_bn_train_stats_apply[_sync]'s arguments, y = NULL for gnx_bn_train_stats[_sync].  The form is
 * chosen on x alone; *fused = 1: y is written by that launch (a one-launch form and 16-B y), 0 with y: gnx_scale_shift_relu
 * follows.  gnx_bn_relu_bwd_form: gnx_bn_relu_bwd[_sync]; *dx_vec4: on the two slab forms, dx through the 16-B kernel. */
#define GNX_BN_MULTI 0       /* four workgroups per 16 channels: 2048 < M <= 8192, C <= 1024, 16-B operands */
#define GNX_BN_SMALL_KEEP 1  /* one workgroup per 16 channels, a lane's rows kept in registers: M <= 2048, 16-B operands */
#define GNX_BN_SMALL_STRIP 2 /* ... walking its strip twice: M <= 4992 (where multi does not apply: C > 1024) */
#define GNX_BN_SLAB_VEC 3    /* per-slab partial sums through 16-B loads + a reduce (forward: a 16-B workspace too) */
#define GNX_BN_SLAB 4        /* ... through scalar loads: any alignment */
#define GNX_BN_EVAL_FUSED 5  /* backward, eval statistics, 16-B operands: dx and the partial sums in one pass (relu = 2 included) */
int gnx_bn_train_stats_form(const float* x, long ld, long M, int C, const float* gamma, const float* beta,
                            const float* running_mean, const float* running_var, const long long* num_batches_tracked,
                            float momentum, float eps, const float* scale, const float* shift, const float* save_mean,
                            const float* save_invstd, const float* y, long ldy, int relu, const float* workspace, int* fused,
                            int* workgroups);
int gnx_bn_relu_bwd_form(const float* dy, long lddy, const float* x, long ldx, const float* dx, long lddx, long M, int C,
                         const float* scale, const float* shift, const float* save_mean, const float* save_invstd,
                         const float* dgamma, const float* dbeta, int relu, int training, int accumulate, int dx_accumulate,
                         const float* workspace, int* dx_vec4, int* workgroups);
/* gnx_wgrad_bnrelu_form: *splits = the position splits whose slabs the call writes; *vec_x / *vec_dy: X (with scale / shift) and
 * dY go through 16-B loads.  gnx_wgrad_bnrelu_batch takes an item iff this says GNX_WG_T1 (taps 1) or GNX_WG_T9 (taps 9, on the
 * maps of item 0).  gnx_conv0_wgrad_form: *workgroups = the blocks, each of which writes four slabs. */
#define GNX_WG_T1 0          /* 128 x 256 transposed images: taps 1, 4 | K > 128, 128 | N, 16-B operands */
#define GNX_WG_T9 1          /* three shifted dY copies: taps 9, N == 32, 128 | K, S in {4, 8, 16, 32}, 32 | M, 16-B operands */
#define GNX_WG_PF 2          /* register-prefetched 1x1: 4 | K, 128 | N, 16-B operands */
#define GNX_WG_PLAIN1 3      /* 1x1, any alignment */
#define GNX_WG_POOL 4        /* the transition: 2x2 mean first */
#define GNX_WG_PLAIN9 5      /* 3x3, any alignment, any S whose halo fits 160 KB of LDS */
#define GNX_WG_STEM_FAST 6   /* conv0 7x7 stride 2, pad 3, O == 64, whole tiles, 16-B operands */
#define GNX_WG_STEM_PLAIN7 7 /* conv0 7x7 stride 2 */
#define GNX_WG_STEM_PLAIN3 8 /* conv0 3x3 stride 1 */
int gnx_wgrad_bnrelu_form(const float* dY, long lddy, const float* X, long ldx, const float* scale, const float* shift,
                          const float* dW, const float* workspace, long M, int N, int K, int S, int taps, int pool, int accumulate,
                          int* workgroups, int* splits, int* vec_x, int* vec_dy);
int gnx_conv0_wgrad_form(const float* x, const float* dS, long ldd, const float* dW, const float* workspace, long imgs, int H,
                         int W, int O, int KH, int KW, int stride, int pad, int accumulate, int* workgroups);
/* gnx_gemm_f32_form: gnx_gemm_f32_ws's arguments (workspace = NULL: gnx_gemm_f32); *splits = the K splits (1: none); *a_vec /
 * *b_vec: the operand goes through 16-B buffer loads (always on the wide and big bodies).  M == 0 or N == 0: GNX_GEMM_PLAIN, 0
 * workgroups. */
#define GNX_GEMM_WIDE 0      /* 256 x 128 tiles, K split over workgroups: M >= 2048, N >= 256, K >= 512, 16-B operands */
#define GNX_GEMM_BIG 1       /* 128 x 64 tiles: M >= 2048, N >= 256, 16-B operands */
#define GNX_GEMM_TALL 2      /* 64 x 64 tiles, K split 2 or 3 ways: N <= 128, K >= 1024, with a workspace */
#define GNX_GEMM_PLAIN 3     /* 64 x 64 tiles */
int gnx_gemm_f32_form(const float* A, long lda, int a_kmajor, const float* B, long ldb, int b_kmajor, const float* bias,
                      const float* C, long ldc, long M, long N, long K, int accumulate, const float* workspace, int* workgroups,
                      int* splits, int* a_vec, int* b_vec);
/* The eval layers of ONE dense block (fp32 path, running statistics) for two disjoint row ranges [0, M0) and [M0, M) of the
 * same block buffer `buf` [M][ld], host code over the launchers above (csrc/block_ranges.hip).  Per layer and range:
 * gnx_conv1x1_bnrelu_act(K = cin, N = mid) into the range's own rows of the bottleneck scratch `bott` [M][mid], then
 * gnx_conv3x3_winograd (W2u != NULL; a shape it declines goes on to the direct form, as in the per-layer path) or
 * gnx_conv3x3_bnrelu (W2r, no prologue) into columns [cin, cin + growth) of those rows.  Spots are independent in eval mode, so
 * one range can be at a layer's conv2 while the other is at its conv1: the persistent kernels of the 8 x 8 and 4 x 4 maps leave
 * most CUs empty in their last round of tiles, and a launch of the other range takes them.  Range 0 runs on `stream`, range 1
 * on a side stream the library creates once per device and keeps; fork and join are one reused event each (record + stream
 * wait), after the call `stream` is ordered after both ranges.  The same kernels on the same rows: the same bits as one range.
 * The plan (gnx_dense_block_ranges_form returns it, nothing launched; a negative GNX_ERR_* where the call returns that):
 *   GNX_BR_ONE    one range [0, M) on `stream`: M0 == 0 or M0 == M (an empty range launches nothing), or a split that is not
 *                 legal - both ranges whole spots and whole 128-row tiles, range 0 whole 256-pixel Winograd tiles where a layer
 *                 has W2u, and every launch of either range the same kernel form (gnx_conv1x1_form, gnx_conv3x3_form,
 *                 gnx_conv3x3_winograd_form) as over all M rows.  An illegal split is never an error and never runs as a pair;
 *   GNX_BR_SERIAL a legal split while `stream` is capturing: range 0's layers, then range 1's, all on `stream` (a captured
 *                 graph stays one chain; the side stream is not touched);
 *   GNX_BR_TWO    a legal split on the two streams.
 * GNX_ERR_BAD_ARG: a NULL buf / bott / layers / W1 / W2r / scale or shift, M0 outside [0, M], M not whole spots, a layer's
 * columns outside ld.  GNX_ERR_LAUNCH: a HIP call failed (stream, event, capture query, kernel launch) - nothing further is
 * launched; after the fork the join is still attempted, so `stream` stays ordered after what the side stream was given. */
#define GNX_BR_ONE 0
#define GNX_BR_SERIAL 1
#define GNX_BR_TWO 2
typedef struct {
    const float* W1; const float* W2u; const float* W2r; const float* scale1; const float* shift1; const float* scale2;
    const float* shift2;
    int cin, pad;
} gnx_dense_layer_item;
int gnx_dense_block_ranges(float* buf, long ld, float* bott, long M, long M0, int S, int mid, int growth, const void* layers,
                           int n_layers, gnx_stream_t stream);
int gnx_dense_block_ranges_form(const float* buf, long ld, const float* bott, long M, long M0, int S, int mid, int growth,
                                const void* layers, int n_layers, gnx_stream_t stream);
int gnx_conv_stem(const float* x, const float* w, float* out, long ldc, long imgs, int Cin, int H, int W, int O,
                  int KH, int KW, int stride, int pad, gnx_stream_t stream);
/* conv0 -> norm0 -> relu0 -> pool0 (:105-110) fused for the 128- and 256-px geometries (conv map 64 or 128 wide, even
 * height, W = 2 Wo): the conv0 map never goes to HBM.  Returns GNX_ERR_UNSUPPORTED for any other geometry: run gnx_conv_stem + gnx_bnrelu_maxpool then. */
int gnx_conv_stem_bnrelu_maxpool(const float* x, const float* w, float* out, long ldo, long imgs, int Cin, int H, int W,
                                 int O, int KH, int KW, int stride, int pad, const float* scale, const float* shift,
                                 gnx_stream_t stream);
/* The same kernel also recording each pooled element's window index (0..8, first maximum of the scan as torch's
 * max_pool2d, densenet.py:110) in argmax [imgs*(Ho/2)*(Wo/2)][O] bytes - the forward of the f-trained step under running
 * statistics (training.py:126); gnx_maxpool_bwd_argmax_bnrelu is its adjoint. */
int gnx_conv_stem_bnrelu_maxpool_argmax(const float* x, const float* w, float* out, long ldo, unsigned char* argmax,
                                        long imgs, int Cin, int H, int W, int O, int KH, int KW, int stride, int pad,
                                        const float* scale, const float* shift, gnx_stream_t stream);
int gnx_bnrelu_maxpool(const float* in, long ldi, float* out, long ldo, long imgs, int C, int Hi, int Wi,
                       const float* scale, const float* shift, gnx_stream_t stream);
int gnx_bnrelu_avgpool(const float* in, long ldi, float* out, long ldo, long imgs, int C, int S2,
                       const float* scale, const float* shift, gnx_stream_t stream);
/* Which body of csrc/stem_pool.hip a call with these arguments runs, without launching anything: the launch arguments without
 * the stream, all pointers const.  Returns the code below, or the negative GNX_ERR_* the call would return; *workgroups (may be
 * NULL): the workgroups of the launch, 0 on an error or when imgs == 0 (then the code is the family's code 0).  Only the
 * pointers' alignment and NULL-ness count.
 *   gnx_conv_stem_form              gnx_conv_stem.
 *   gnx_conv_stem_pool_form         the fp32-operand fused stems, conv_stem_pool_kernel<Wo, out_f16, x_is_u8, argmax != NULL>:
 *       gnx_conv_stem_bnrelu_maxpool         x_is_u8 = out_f16 = 0, argmax = src_idx = NULL, src_imgs = 0
 *       gnx_conv_stem_bnrelu_maxpool_idx     ... with src_idx (NULL: GNX_ERR_BAD_ARG from the entry point itself) and src_imgs
 *       gnx_conv_stem_bnrelu_maxpool_argmax  ... with argmax (NULL: likewise)
 *       gnx_conv_stem_bnrelu_maxpool_h16     out_f16 = 1
 *       gnx_conv_stem_bnrelu_maxpool_u8      x_is_u8 = 1, out_f16 as given
 *       gnx_conv_stem_bnrelu_maxpool_u8_idx  x_is_u8 = 1 with src_idx and src_imgs
 *   gnx_conv_stem_pool_f16mul_form  gnx_conv_stem_bnrelu_maxpool_f16mul (rows_total = 0) and, with any other rows_total,
 *                                   gnx_conv_stem_bnrelu_maxpool_f16mul_cb (ldo is not looked at), that entry's own checks included.
 *   gnx_bnrelu_maxpool_form         gnx_bnrelu_maxpool (argmax = NULL) and gnx_bnrelu_maxpool_argmax.
 * The average pools and gnx_u8_to_f32 have one body each. */
#define GNX_STEM_GENERIC 0 /* conv_stem_kernel: 128 x 64 tiles, any Cin, KH <= 7, KW <= 8 */
#define GNX_STEM_PATCH7 1  /* conv_stem_patch_kernel<2, 7, 3>: Cin = 3, 7x7 stride 2, O <= 64; up to 768 workgroups over 8 x 16 tiles */
#define GNX_STEM_PATCH3 2  /* conv_stem_patch_kernel<1, 3, 3>: Cin = 3, 3x3 stride 1, O <= 64 */
#define GNX_SP_64 0        /* conv map 64 wide (128-px patches): up to 512 workgroups */
#define GNX_SP_128 1       /* conv map 128 wide (256-px patches): up to 256 workgroups */
#define GNX_SP16_64 0      /* conv_stem_pool_f16_kernel<64, x_is_u8>: up to 768 workgroups */
#define GNX_SP16_128 1     /* conv_stem_pool_f16_kernel<128, x_is_u8>: up to 768 workgroups */
#define GNX_MP_SCALAR 0    /* bnrelu_maxpool_kernel<argmax != NULL>: any alignment; up to 8192 workgroups */
#define GNX_MP_VEC4 1      /* bnrelu_maxpool_vec4_kernel: 4 | C, ldi, ldo, 16-B operands, 4-B argmax; up to 16384 workgroups */
int gnx_conv_stem_form(const float* x, const float* w, const float* out, long ldc, long imgs, int Cin, int H, int W, int O, int KH,
                       int KW, int stride, int pad, int* workgroups);
int gnx_conv_stem_pool_form(const void* x, int x_is_u8, const float* w, const void* out, int out_f16, long ldo, long imgs, int Cin,
                            int H, int W, int O, int KH, int KW, int stride, int pad, const float* scale, const float* shift,
                            const unsigned char* argmax, const int* src_idx, long src_imgs, int* workgroups);
int gnx_conv_stem_pool_f16mul_form(const void* x, int x_is_u8, const float* w, const void* out16, long ldo, long rows_total,
                                   long imgs, int Cin, int H, int W, int O, int KH, int KW, int stride, int pad, const float* scale,
                                   const float* shift, const float* norm, int* workgroups);
int gnx_bnrelu_maxpool_form(const float* in, long ldi, const float* out, long ldo, const unsigned char* argmax, long imgs, int C,
                            int Hi, int Wi, const float* scale, const float* shift, int* workgroups);

/* ---- empty spots (csrc/spot_compact.hip) ----------------------------------------------------------------------------
 * A frozen eval-mode f maps every all-zero patch to the same row, and real arrays zero-fill every position without
 * tissue: the eval forward runs the non-empty spots plus ONE empty one and copies that row to the other empty spots.
 * gnx_spot_compact: x = N spots of spot_bytes bytes, contiguous (16 | spot_bytes, 16-B aligned, else
 *   GNX_ERR_UNSUPPORTED); a spot is empty iff ALL ITS BYTES are zero (-0.0 and NaN are not empty).  Device ints out,
 *   ascending and the same on every run: fg_idx [N] = the non-empty spots, then the first empty spot repeated up to N (so
 *   fg_idx[0 .. n) is a list of the non-empty spots padded with an empty one); bg_idx [N] = the empty spots in
 *   [0, n_bg); counts = {n_fg, n_bg}; flags [N] = scratch.
 * gnx_conv_stem_bnrelu_maxpool_idx / _u8_idx: the fused stems (fp32 output) reading patch src_idx[i] of the src_imgs
 *   patches of x as output image i, imgs = entries of the list (entries outside [0, src_imgs) are clamped): no gathered
 *   copy of the patches.
 * gnx_bnrelu_avgpool_idx: gnx_bnrelu_avgpool writing image i's row to out row dst_idx[i] (< dst_rows, else not written).
 * gnx_spot_broadcast_rows: rows [n_rows][C] (ld): row bg_idx[0] copied to the rows bg_idx[1 .. n_bg). */
int gnx_spot_compact(const void* x, long spot_bytes, long N, int* flags, int* fg_idx, int* bg_idx, int* counts,
                     gnx_stream_t stream);
int gnx_spot_broadcast_rows(float* rows, long ld, long n_rows, int C, const int* bg_idx, long n_bg, gnx_stream_t stream);
int gnx_conv_stem_bnrelu_maxpool_idx(const float* x, const float* w, float* out, long ldo, long imgs, int Cin, int H, int W,
                                     int O, int KH, int KW, int stride, int pad, const float* scale, const float* shift,
                                     const int* src_idx, long src_imgs, gnx_stream_t stream);
int gnx_conv_stem_bnrelu_maxpool_u8_idx(const unsigned char* x8, const float* w, float* out, long ldo, long imgs, int Cin,
                                        int H, int W, int O, int KH, int KW, int stride, int pad, const float* scale,
                                        const float* shift, const float* norm, const int* src_idx, long src_imgs,
                                        gnx_stream_t stream);
int gnx_bnrelu_avgpool_idx(const float* in, long ldi, float* out, long ldo, long imgs, int C, int S2, const float* scale,
                           const float* shift, const int* dst_idx, long dst_rows, gnx_stream_t stream);

/* fp16-MFMA variants (BASELINE config 5, "fp16 MFMA conv path"): same contract, operands rounded to fp16 in LDS,
 * v_mfma_f32_32x32x16_f16, fp32 accumulate/outputs.  Return GNX_ERR_UNSUPPORTED for unaligned pointers or K % 4 != 0. */
int gnx_conv1x1_bnrelu_f16(const float* A, long lda, const float* W, float* out, long ldc, long M, int N, int K,
                           const float* scale, const float* shift, int pool, int S_in, gnx_stream_t stream);
int gnx_conv3x3_bnrelu_f16(const float* A, long lda, const float* Wr, float* out, long ldc, long M, int N, int K, int S,
                           const float* scale, const float* shift, gnx_stream_t stream);
/* Config 5 with the bottleneck kept in fp16: conv1 stores it activated (the consumer's norm2 -> relu2, :38-39) and rounded to
 * fp16 [M][N] (ldc16 in halves); conv2 then streams it and the fp16 tap-major weights (gnx_repack_conv3x3's layout rounded
 * once) global -> LDS by DMA and multiplies with v_mfma_f32_32x32x16_f16, fp32 accumulation, fp32 output.
 * gnx_conv3x3_f16_dma: N == 32, 128 | K, 128 | M, S in {4, 8, 16, 32, 64}, 16-B aligned; else GNX_ERR_UNSUPPORTED. */
int gnx_conv1x1_bnrelu_f16_act16(const float* A, long lda, const float* W, void* out16, long ldc16, long M, int N, int K,
                                 const float* scale, const float* shift, const float* out_scale, const float* out_shift,
                                 gnx_stream_t stream);
int gnx_conv3x3_f16_dma(const void* A16, long lda16, const void* Wr16, float* out, long ldc, long M, int N, int K, int S,
                        gnx_stream_t stream);
/* Config 5 with fp16 BLOCK BUFFERS (the concatenated features themselves live in HBM as fp16, as they do under the
 * reference's autocast): the stem, conv1 (and the transitions: pool = 1, out_scale = out_shift = NULL), conv2 and the final
 * pool reading / writing [rows][ld halves]; arithmetic as the entry points above. */
int gnx_conv_stem_bnrelu_maxpool_h16(const float* x, const float* w, void* out16, long ldo, long imgs, int Cin, int H, int W,
                                     int O, int KH, int KW, int stride, int pad, const float* scale, const float* shift,
                                     gnx_stream_t stream);
/* ---- uint8 patches (SURVEY 8f-2 input pipeline) -------------------------------------------------------------------
 * The reference converts 8-bit patch files to floats on the host (torchvision ToTensor, gridnext/image_datasets.py:102-105,
 * :185; optionally Normalize) and moves 4 bytes per pixel host -> device (training.py:135-139).  Here patches stay uint8
 * [imgs][3][H][W] until the stem kernel's operand load: u8 / 255 and, with norm != NULL, (v - mean[c]) / std[c] - bit for bit
 * the floats torch produces.  norm: device floats {mean[3], std[3], 1/std[3]}.  gnx_conv_stem_bnrelu_maxpool_u8 = the fused
 * stem (same geometries; out_f16: pooled map stored as fp16); gnx_u8_to_f32 = the conversion alone (H*W % 4 == 0), for the
 * training forward (conv0's weight gradient re-reads float patches) and other geometries. */
int gnx_conv_stem_bnrelu_maxpool_u8(const unsigned char* x8, const float* w, void* out, long ldo, long imgs, int Cin, int H,
                                    int W, int O, int KH, int KW, int stride, int pad, const float* scale,
                                    const float* shift, const float* norm, int out_f16, gnx_stream_t stream);
int gnx_u8_to_f32(const unsigned char* x8, float* out, long imgs, int C, int H, int W, const float* norm,
                  gnx_stream_t stream);
/* ---- Resize + CenterCrop of uint8 patches (the first steps of the tutorials' transform) ------------------------------
 * The tutorials build their datasets with Compose([Resize(256), CenterCrop(224), ToTensor(), Normalize(mean, std)]), all of it
 * on the host, per patch, in PIL (gridnext/image_datasets.py:102-105, :113-117).  Here the stored bytes go to the device and
 * x8 [imgs][3][H0][W0] uint8 (any base alignment) -> out [imgs][3][Ph][Pw]: the window (top, left, Ph, Pw) of every plane
 * resized to (Hr, Wr).  The bytes are Pillow's for resize((Wr, Hr), BILINEAR) + crop, bit for bit: its two-pass fixed-point
 * resampling - per axis scale = in / out, support = max(scale, 1), taps [xmin, xmax) = [(int)(center - support + 0.5),
 * (int)(center + support + 0.5)) clamped to the axis, center = (i + 0.5) scale, weights max(0, 1 - |(x + 0.5 - center) *
 * (1 / support)|) divided by their sequential sum, each rounded to k = (int)(0.5 + w 2^22); a pass is
 * clip((2^21 + sum pixel k) >> 22, 0, 255); horizontal first, into bytes, then vertical.  The caller passes the tables of the
 * WINDOW's columns and rows as device int32: hcoef [Pw][ksw], hbnd [Pw][2] = {first tap, taps}, vcoef [Ph][ksh], vbnd [Ph][2],
 * with ksw, ksh from the gnx_resize_ksize query (in, out); an axis whose size does not change has ksize 1 and the identity table {2^22},
 * {window start + i, 1}.  Every table entry is clamped before it addresses anything.  GNX_ERR_UNSUPPORTED (nothing is
 * launched): a reduction above 8x on an axis (ksize > 17), a plane too wide for one output row's inputs to fit the LDS.
 * GNX_ERR_BAD_ARG: a window outside the resized image.  The _f32 form stores ToTensor (+ Normalize, norm as above or NULL) of
 * those bytes as floats - the floats gnx_u8_to_f32 gives for the byte output. */
int gnx_resize_ksize(int n_in, int n_out);
int gnx_resize_crop_u8(const unsigned char* x8, unsigned char* out, long imgs, int H0, int W0, int Hr, int Wr, int top, int left,
                       int Ph, int Pw, const int* hcoef, const int* hbnd, const int* vcoef, const int* vbnd,
                       gnx_stream_t stream);
int gnx_resize_crop_u8_f32(const unsigned char* x8, float* out, long imgs, int H0, int W0, int Hr, int Wr, int top, int left,
                           int Ph, int Pw, const int* hcoef, const int* hbnd, const int* vcoef, const int* vbnd,
                           const float* norm, gnx_stream_t stream);
/* ---- Patch grid of a Visium array from the whole-slide image -----------------------------------------------------------
 * The reference's grid_from_wsi_visium (gridnext/imgprocess.py:198-236) edge-pads the whole slide on the host, cuts a window
 * around every in-tissue spot, resizes it with Image.fromarray(window).resize((P, P)) - Pillow's default filter, BICUBIC - and
 * stores it, planar, at the spot's odd-right cell of a (78, 64, 3, P, P) grid.  Here the slide is resident on the device as
 * uint8 [Hs][Ws][3] (interleaved, any base alignment) and one gather writes out [grid_h][grid_w][3][P][P]: for every spot
 * {x_px, y_px, grid_row, grid_col} the window of source rows and columns [c - half, c + half) (half = window_size / 2), every
 * coordinate clamped to the slide (= the slice of the edge-padded slide), resized to P x P.  The bytes are Pillow's, bit for
 * bit: its two-pass fixed-point resampling as for gnx_resize_crop_u8, with the bicubic kernel (a = -0.5; ((a + 2) x - (a + 3))
 * x^2 + 1 for |x| < 1, (((x - 5) x + 8) x - 4) a for |x| < 2), support = 2 max(in / out, 1), ksize = ceil(support) 2 + 1,
 * negative weights rounded to k = (int)(-0.5 + w 2^22); horizontal pass first, into bytes, then vertical.  coef [P][ksize],
 * bnd [P][2] = {first tap, taps}: device int32, ONE table pair for both axes and all spots (every window is 2 half square);
 * 2 half == P is the identity (ksize 1; a deinterleaving copy, the tables are not read).  Only the listed cells are written:
 * the caller zero-fills the rest.  spots is HOST memory, int32 [n][4]: the entry point checks it and hands it to the kernel in
 * the launch arguments (no device table, no allocation, nothing read back).  Every spot coordinate and table entry is
 * clamped before it addresses anything; all byte offsets are 64-bit.  GNX_ERR_BAD_ARG (nothing is launched): a grid_row /
 * grid_col outside the grid, a ksize that is not the one of (2 half, P).  GNX_ERR_UNSUPPORTED (nothing is launched): a window
 * above 4x the patch (ksize > 17), a window too wide for one output row's inputs to fit the LDS.  The _f32 form stores
 * ToTensor (+ Normalize, norm = device floats {mean[3], std[3], 1/std[3]} or NULL) of those bytes, as gnx_resize_crop_u8_f32. */
int gnx_wsi_patch_grid_u8(const unsigned char* slide, int Hs, int Ws, const int* spots, int n, int half, int P, int grid_h,
                          int grid_w, const int* coef, const int* bnd, int ksize, unsigned char* out, gnx_stream_t stream);
int gnx_wsi_patch_grid_u8_f32(const unsigned char* slide, int Hs, int Ws, const int* spots, int n, int half, int P, int grid_h,
                              int grid_w, const int* coef, const int* bnd, int ksize, float* out, const float* norm,
                              gnx_stream_t stream);
/* The _lut forms: SpaCell's colour-cast removal (gridnext/imgprocess.py:49-67: per channel Image.point(i -> i * 255 / p99)
 * over the WHOLE slide) folded into the gather of grid_from_wsi_visium (imgprocess.py:198-236).  lut: device uint8 [3][256],
 * channel-major, the table gnx_rgb_lut_u8 takes, at any alignment.  Every source byte of channel c is replaced by lut[c][byte]
 * before it enters the resampler; a per-pixel map commutes with the edge replication, so out is, bit for bit, the plain entry
 * point run on gnx_rgb_lut_u8(slide, lut) = Pillow's point + resize - while the slide is neither written nor copied (the
 * table lies in 768 bytes of LDS next to the staged rows).  Arguments, checks and refusals are the plain sibling's, and a NULL
 * lut with n > 0 is GNX_ERR_BAD_ARG (nothing is launched). */
int gnx_wsi_patch_grid_u8_lut(const unsigned char* slide, int Hs, int Ws, const int* spots, int n, int half, int P, int grid_h,
                              int grid_w, const int* coef, const int* bnd, int ksize, unsigned char* out,
                              const unsigned char* lut /* [3][256] */, gnx_stream_t stream);
int gnx_wsi_patch_grid_u8_f32_lut(const unsigned char* slide, int Hs, int Ws, const int* spots, int n, int half, int P,
                                  int grid_h, int grid_w, const int* coef, const int* bnd, int ksize, float* out,
                                  const float* norm, const unsigned char* lut /* [3][256] */, gnx_stream_t stream);
/* The fused stem with fp16 matrix operands (config 5: patch and weights rounded to fp16 at the LDS stash,
 * v_mfma_f32_32x32x16_f16, fp32 accumulate), pooled map stored as fp16; x float patches, or uint8 when x_is_u8 (norm as
 * above, else NULL). */
int gnx_conv_stem_bnrelu_maxpool_f16mul(const void* x, int x_is_u8, const float* w, void* out16, long ldo, long imgs,
                                        int Cin, int H, int W, int O, int KH, int KW, int stride, int pad,
                                        const float* scale, const float* shift, const float* norm, gnx_stream_t stream);
int gnx_conv1x1_bnrelu_f16_h(const void* A16, long lda16, const float* W, void* out16, long ldc16, long M, int N, int K,
                             const float* scale, const float* shift, const float* out_scale, const float* out_shift,
                             int pool, int S_in, gnx_stream_t stream);
/* gnx_conv1x1_bnrelu_h16: the dense-layer case of gnx_conv1x1_bnrelu_f16_h (pool = 0, consumer activation) with the weight
 * rounded to fp16 once (W16 [N][K] halves): chunks of 64 channels, 16-B loads. */
int gnx_conv1x1_bnrelu_h16(const void* A16, long lda16, const void* W16, void* out16, long ldc16, long M, int N, int K,
                           const float* scale, const float* shift, const float* out_scale, const float* out_shift,
                           gnx_stream_t stream);
/* Transitions of config 5 in two steps (pool-first: norm -> relu -> 2x2 mean, then the 1x1 conv on a quarter of the rows,
 * densenet.py:47-54): gnx_bnrelu_avgpool2_h16 writes the pooled, activated block buffer [imgs*(S/2)^2][C] halves;
 * gnx_conv1x1_bnrelu_h16 with scale = shift = NULL (no prologue) and out_scale = out_shift = NULL (no consumer activation)
 * multiplies it. */
int gnx_bnrelu_avgpool2_h16(const void* in16, long ldi, void* out16, long ldo, long imgs, int C, int S, const float* scale,
                            const float* shift, gnx_stream_t stream);
int gnx_conv3x3_f16_dma_h(const void* A16, long lda16, const void* Wr16, void* out16, long ldc16, long M, int N, int K, int S,
                          gnx_stream_t stream);
int gnx_bnrelu_avgpool_h16(const void* in16, long ldi, float* out, long ldo, long imgs, int C, int S2, const float* scale,
                           const float* shift, gnx_stream_t stream);
/* A DenseNet transition of the fp16 path as ONE kernel on channel-blocked fp16 buffers (transition_f16.hip):
 * norm -> relu -> conv 1x1 (K -> N) -> avgpool 2x2 (gridnext/densenet.py:47-53), evaluated pool-first; the
 * pooled activated operand exists in the LDS only (bit-identical to gnx_bnrelu_avgpool2_h16_cb's output).
 * gnx_transition_f16_pack: conv.weight [N][K] fp32 -> wp (N * K halves, MFMA fragment order).
 * gnx_transition_f16: X16 [K / 32][rows_in][32] -> channel blocks [0, N / 32) of Y16 [..][rows_out][32]; S in {8, 16, 32, 64};
 * 32 | K, 64 <= K <= 1024; 128 | N <= 512; 128 | n_img * (S / 2)^2; anything else: GNX_ERR_UNSUPPORTED (callers take the
 * two-kernel form). */
int gnx_transition_f16_pack(const float* w, void* wp, int N, int K, gnx_stream_t stream);
int gnx_transition_f16(const void* X16, long rows_in, long n_img, int S, int K, int N, const void* wp, const float* scale,
                       const float* shift, void* Y16, long rows_out, gnx_stream_t stream);
/* The same transition as the TAPED forward of the fp16 gradient path (training.py:164-171 stepping f_opt): additionally stores
 * the pooled activated operand avgpool2(relu(norm(x))) - which the kernel holds in the LDS anyway; bit for bit
 * gnx_bnrelu_avgpool2_h16_cb's output - as a row-major fp16 matrix P16 [n_img * (S / 2)^2][ldp] (columns [0, K); 8 | ldp), the
 * operand of the transition's 1x1 weight gradient.  Everything else is gnx_transition_f16 bit for bit. */
int gnx_transition_f16_tape(const void* X16, long rows_in, long n_img, int S, int K, int N, const void* wp, const float* scale,
                            const float* shift, void* Y16, long rows_out, void* P16, long ldp, gnx_stream_t stream);
/* One whole dense layer of config 5 in ONE kernel (gridnext/densenet.py:35-44: cat -> norm1 -> relu1 -> conv1 -> norm2 ->
 * relu2 -> conv2) on a CHANNEL-BLOCKED fp16 block buffer X16 [channels / 32][rows_total][32] - element (row, c) at
 * (c >> 5) * rows_total * 32 + row * 32 + (c & 31), so the 32 channels a K-loop stage needs of consecutive pixels are
 * contiguous memory: reads channel blocks [0, K / 32), writes block K / 32; the 128-channel bottleneck lives in LDS only.
 * gnx_dense_layer_f16_pack rounds conv1.weight [128][K] and conv2.weight [32][128][3][3] (fp32, torch layouts) to fp16 ONCE
 * into the MFMA-fragment order the kernel streams (w1p: 128 * K halves, w2p: 36 864 halves).  bn_size * growth_rate = 128,
 * growth_rate = 32; S in {4, 8, 16, 32, 64}; 32 | K, 64 <= K <= 1024; 128 | n_img * S * S; anything else: GNX_ERR_UNSUPPORTED (callers
 * fall back to the two-kernel pair on row-major buffers).  The `_cb` entry points are the neighbours of that layout: the
 * fp16 stem and the transition's 1x1 conv STORE channel-blocked, the transition's pooling pass and the final pool READ it. */
int gnx_dense_layer_f16_pack(const float* w1, const float* w2, void* w1p, void* w2p, int K, gnx_stream_t stream);
int gnx_dense_layer_f16(void* X16, long rows_total, long n_img, int S, int K, const void* w1p, const void* w2p,
                        const float* scale1, const float* shift1, const float* scale2, const float* shift2, gnx_stream_t stream);
/* The same layer as the TAPED forward of the fp16 gradient path (training.py:164-171 stepping f_opt): additionally stores the
 * activated bottleneck relu2(norm2(conv1(.))) - the tile the kernel holds in the LDS anyway - as A16 [4][a_rows_total][32]
 * halves (channel-blocked like X16), the operand of conv2's weight gradient and of norm2's adjoint.  Everything else is
 * gnx_dense_layer_f16 bit for bit. */
int gnx_dense_layer_f16_tape(void* X16, long rows_total, long n_img, int S, int K, const void* w1p, const void* w2p,
                             const float* scale1, const float* shift1, const float* scale2, const float* shift2, void* A16,
                             long a_rows_total, gnx_stream_t stream);
/* gnx_conv_stem_bnrelu_maxpool_f16mul storing into the channel-blocked buffer [O / 32][rows_total][32] halves.  32 | O, and
 * rows_total >= imgs * (Ho / 2) * (Wo / 2), every pooled row of the launch: GNX_ERR_BAD_ARG otherwise, nothing launched. */
int gnx_conv_stem_bnrelu_maxpool_f16mul_cb(const void* x, int x_is_u8, const float* w, void* out16, long rows_total, long imgs,
                                           int Cin, int H, int W, int O, int KH, int KW, int stride, int pad, const float* scale,
                                           const float* shift, const float* norm, gnx_stream_t stream);
int gnx_conv1x1_bnrelu_h16_cb(const void* A16, long lda16, const void* W16, void* out16, long rows_total, long M, int N, int K,
                              const float* scale, const float* shift, const float* out_scale, const float* out_shift,
                              gnx_stream_t stream);
int gnx_bnrelu_avgpool2_h16_cb(const void* in16, long rows_total, void* out16, long ldo, long imgs, int C, int S,
                               const float* scale, const float* shift, gnx_stream_t stream);
int gnx_bnrelu_avgpool_h16_cb(const void* in16, long rows_total, float* out, long ldo, long imgs, int C, int S2,
                              const float* scale, const float* shift, gnx_stream_t stream);

/* ---- DenseNet-BC backward (the gradients torch.autograd derives for gridnext/densenet.py) -----------------------------
 * Data gradients reuse gnx_conv1x1_bnrelu / gnx_conv3x3_bnrelu with weights transformed by gnx_transpose_weight
 * ([N][K] -> [K][N]) and gnx_repack_conv3x3_bwd ([N][K][3][3] -> [8-tap][K][N]).
 * gnx_wgrad_bnrelu: dW of conv1 / conv2 / transition conv (taps 1|9, pool), BN+ReLU prologue recomputed while staging.
 * gnx_conv0_wgrad : dW of features.conv0 from NCHW patches.  Pool adjoints: maxpool (pool0), avgpool2 (transition),
 * rows_broadcast (adaptive_avg_pool). */
long gnx_wgrad_workspace(long M, int N, int K, int taps); /* floats */
int gnx_wgrad_bnrelu(const float* dY, long lddy, const float* X, long ldx, const float* scale, const float* shift,
                     float* dW, float* workspace, long M, int N, int K, int S, int taps, int pool, int accumulate,
                     gnx_stream_t stream);
/* n independent weight gradients of ONE kind as one launch per 24 items plus one batched reduce: exactly
 * gnx_wgrad_bnrelu(item..., taps, pool = 0) for every item, bit for bit (same kernel bodies, slab layout and fixed-order
 * reduce) - the dense layers of a block at a batch of 32 patches are 16-64 workgroups each and cost their launch whatever they
 * compute (densenet.py:35-44 backwards, training.py:45-71).  taps = 9: the same S for all items.  Shapes the transposed-image
 * kernels do not take: GNX_ERR_UNSUPPORTED, nothing launched (make the single calls).  `items`: HOST array. */
typedef struct {
    const float* dY; long lddy; const float* X; long ldx; const float* scale; const float* shift; float* dW; float* workspace;
    long M; int N, K, S, accumulate;
} gnx_wgrad_item;
int gnx_wgrad_bnrelu_batch(const void* items, int n, int taps, gnx_stream_t stream);
int gnx_transpose_weight(const float* w, float* wt, int N, int K, gnx_stream_t stream);
/* Every weight re-layout of one kind for a whole network in one launch (a training step re-lays all conv weights out after
 * each optimizer step: 3 x 58 launches for DenseNet-121).  `table`: n entries {const float* src; float* dst; int N; int K;}
 * (24 bytes each, DEVICE memory); kind 0 = gnx_repack_conv3x3, 1 = gnx_repack_conv3x3_bwd, 2 = gnx_transpose_weight. */
int gnx_relayout_weights_batch(const void* table, int n, int kind, gnx_stream_t stream);
int gnx_repack_conv3x3_bwd(const float* w, float* wb, int N, int K, gnx_stream_t stream);
int gnx_rows_broadcast(const float* in, long ldi, float* out, long ldo, long imgs, int C, int S2, float alpha,
                       gnx_stream_t stream);
int gnx_avgpool2_bwd(const float* dP, long ldp, float* dA, long lda, long imgs, int C, int S, gnx_stream_t stream);
int gnx_maxpool_bwd(const float* in, long ldi, const float* pooled, long ldp, const float* dOut, long lddo, float* dAct,
                    long lda, long imgs, int C, int Hi, int Wi, const float* scale, const float* shift,
                    gnx_stream_t stream);
/* Pooling by recorded index (the training forward): gnx_bnrelu_maxpool_argmax = gnx_bnrelu_maxpool that also stores, per
 * pooled element, which of its 3x3 window elements (0..8, row-major) is the maximum - the FIRST maximal one of the scan, as
 * torch's max_pool2d (densenet.py:110) picks it; gnx_maxpool_bwd_argmax routes d(pooled) back by that index: no value
 * comparison, no re-read of the conv0 map, ties (constant regions: white background, empty spots) go where torch sends
 * them.  argmax: [imgs*Ho*Wo][C] bytes; 4 | C for the backward. */
int gnx_bnrelu_maxpool_argmax(const float* in, long ldi, float* out, long ldo, unsigned char* argmax, long imgs, int C,
                              int Hi, int Wi, const float* scale, const float* shift, gnx_stream_t stream);
int gnx_maxpool_bwd_argmax(const unsigned char* argmax, const float* dOut, long lddo, float* dAct, long lda, long imgs,
                           int C, int Hi, int Wi, gnx_stream_t stream);
/* The same adjoint carried through norm0 -> relu0 (densenet.py:107-109) with running statistics: dPre = gradient of the
 * conv0 map; the ReLU mask is read off the pooled activated output (`pooled`, ldp), `scale` = gamma / sqrt(var + eps). */
int gnx_maxpool_bwd_argmax_bnrelu(const unsigned char* argmax, const float* dOut, long lddo, const float* pooled, long ldp,
                                  const float* scale, float* dPre, long lda, long imgs, int C, int Hi, int Wi,
                                  gnx_stream_t stream);
long gnx_conv0_wgrad_workspace(long imgs, int H, int W, int O, int KH, int KW, int stride, int pad); /* floats */
int gnx_conv0_wgrad(const float* x, const float* dS, long ldd, float* dW, float* workspace, long imgs, int H, int W,
                    int O, int KH, int KW, int stride, int pad, int accumulate, gnx_stream_t stream);
/* The gradient of features.conv0 with respect to its input, the NCHW patches (densenet.py:105-107: conv0 7x7 stride 2 pad 3;
 * the small_inputs stem beside it, densenet.py:101-104: 3x3 stride 1 pad 1) - a transposed convolution O -> 3 channels:
 *   dX[i][c][y][x] = sum over (o, ky, kx) of dS[(i*Ho + yo)*Wo + xo][o] * w[o][c][ky][kx],
 *   yo*stride = y + pad - ky, xo*stride = x + pad - kx; only integer yo in [0, Ho) and xo in [0, Wo) contribute;
 *   Ho, Wo as gnx_conv_stem and gnx_conv0_wgrad compute them.
 * dS [imgs*Ho*Wo][O] with leading dimension ldd >= O (may be a column window of a wider buffer; read 16 B at a time where
 * 4 | ldd and dS is 16-B aligned, by single floats otherwise); w: conv0.weight [O][3][KH][KW]; dX: [imgs][3][H][W], EVERY element
 * written (the caller does not pre-zero).  fp32 throughout, no atomics, one summation order per element (ky, kx, o ascending):
 * bit-reproducible, and an image's result does not depend on imgs, on its position in the batch or on the grid.
 * (KH, KW, stride, pad) = (7, 7, 2, 3) or (3, 3, 1, 1), O <= 64, any H, W >= 1; anything else: GNX_ERR_UNSUPPORTED, nothing
 * launched. */
int gnx_conv0_dgrad(const float* dS, long ldd, const float* w, float* dX, long imgs, int H, int W, int O, int KH, int KW,
                    int stride, int pad, gnx_stream_t stream);

/* ---- DenseNet-BC backward on the fp16-MFMA path (BASELINE config 5 with f trained: what torch.autograd derives for
 * gridnext/densenet.py:35-54 when training.py:164-171 steps f_opt; BatchNorm on running statistics, training.py:126) --------
 * Tape and gradients are fp16, row-major: block buffer X16 [M][c_total], block gradient G16 (same shape), activated bottleneck
 * A16 [M][128] (conv1's output after norm2 -> relu2, as gnx_conv1x1_bnrelu_h16 stores it), its gradient dB16 [M][128].
 * v_mfma_f32_32x32x16_f16, fp32 accumulation, fp32 parameter gradients.  `ls`: device floats {s, 1/s}, a power-of-two loss
 * scale - every fp16 gradient tensor holds s x the true gradient, every fp32 result is multiplied by 1/s; `flag` (device int,
 * may be NULL) is OR-ed with 1 when a result is not finite.  Workspaces in floats; `accumulate` != 0 adds to the outputs.
 *   gnx_wgrad1x1_f16: dW[N][K] = sum_m dY16[m][n] act(X16[m][k]), act = relu(scale x + shift) or identity (scale NULL)
 *                     - conv1 (:37) and the transition conv (:51, X16 = the pooled activated map of gnx_bnrelu_avgpool2_h16)
 *   gnx_wgrad3x3_f16: dW[32][128][3][3] of conv2 (:40) from dY16 (the layer's 32 gradient columns) and A16, S x S maps
 *   gnx_conv3x3_dgrad_bnrelu_bwd_f16: dB16 = scale2 * conv3x3^T(dY16, W2) * [A16 > 0] (+ dgamma2, dbeta2; gamma2 != 0);
 *                     W2b16 = conv2.weight as [tap][128][32] halves
 *   gnx_conv1x1_dgrad_bnrelu_bwd_f16: G16[:, :K] += scale1 * (dB16 . W1) * [bn1(X16) > 0] (+ dgamma1, dbeta1); W1t16 =
 *                     conv1.weight transposed to [K][128] halves; 32 | K
 *   gnx_tail_bwd_f16: norm_final -> relu -> adaptive_avg_pool (:153-156): G16 [imgs S2][C] = s * scale [bn(X16) > 0] dfeats / S2
 *   gnx_trans_bwd_f16: transition norm -> relu -> avgpool 2x2 (:48-53, pool-first) from the pooled gradient dP16: writes G16
 *   gnx_h16_cols_to_f32: out[M][C] = G16[:, :C] / s (the gradient of the pooled stem map, handed to the fp32 stem adjoints)
 *   gnx_stem_bwd_f16: conv0 -> norm0 -> relu0 -> pool0 (:105-110) differentiated in one pass over the PATCHES (P = 128 / 256,
 *                     64 channels): the conv0 rows are recomputed exactly as gnx_conv_stem_bnrelu_maxpool_f16mul computes them,
 *                     pool0's winners found by torch's first-maximum rule, G16[:, :64] (s x the pooled map's gradient) routed to
 *                     them and contracted with the im2col of the staged rows: dW [64][3][7][7], dgamma / dbeta [64] (gamma != 0) */
long gnx_wgrad1x1_f16_workspace(long M, int N, int K);
int gnx_wgrad1x1_f16(const void* dY16, long lddy, const void* X16, long ldx, const float* scale, const float* shift, float* dW,
                     float* workspace, long M, int N, int K, const float* ls, int accumulate, int* flag, gnx_stream_t stream);
long gnx_wgrad3x3_f16_workspace(long M);
int gnx_wgrad3x3_f16(const void* dY16, long lddy, const void* A16, float* dW, float* workspace, long M, int S, const float* ls,
                     int accumulate, int* flag, gnx_stream_t stream);
long gnx_conv3x3_dgrad_bnrelu_bwd_f16_workspace(long M);
int gnx_conv3x3_dgrad_bnrelu_bwd_f16(const void* dY16, long lddy, const void* W2b16, const void* A16, void* dB16, long M, int S,
                                     const float* scale2, const float* gamma2, const float* beta2, float* dgamma, float* dbeta,
                                     float* workspace, const float* ls, int accumulate, int* flag, gnx_stream_t stream);
long gnx_conv1x1_dgrad_bnrelu_bwd_f16_workspace(long M, int K);
int gnx_conv1x1_dgrad_bnrelu_bwd_f16(const void* dB16, const void* W1t16, const void* X16, long ldx, void* G16, long ldg, long M,
                                     int K, const float* scale, const float* shift, const float* mean, const float* invstd,
                                     float* dgamma, float* dbeta, float* workspace, const float* ls, int accumulate, int* flag,
                                     gnx_stream_t stream);
/* The same pass also producing conv1's weight gradient dW[128][K] (fp32, (+)=; = gnx_wgrad1x1_f16(dB16, X16, scale, shift)) from
 * the tiles it stages: the separate pass over dB16 and X16 is not made.  workspace: gnx_conv1x1_dgrad_wgrad_f16_workspace floats. */
long gnx_conv1x1_dgrad_wgrad_f16_workspace(long M, int K);
int gnx_conv1x1_dgrad_wgrad_bnrelu_bwd_f16(const void* dB16, const void* W1t16, const void* X16, long ldx, void* G16, long ldg,
                                           long M, int K, const float* scale, const float* shift, const float* mean,
                                           const float* invstd, float* dgamma, float* dbeta, float* dW, float* workspace,
                                           const float* ls, int accumulate, int* flag, gnx_stream_t stream);
long gnx_tail_bwd_f16_workspace(long imgs, int C);
int gnx_tail_bwd_f16(const float* dfeats, long ldf, const void* X16, long ldx, void* G16, long ldg, long imgs, int C, int S2,
                     const float* scale, const float* shift, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                     float* workspace, const float* ls, int accumulate, int* flag, gnx_stream_t stream);
long gnx_trans_bwd_f16_workspace(long imgs, int C, int S);
int gnx_trans_bwd_f16(const void* dP16, long ldp, const void* X16, long ldx, void* G16, long ldg, long imgs, int C, int S,
                      const float* scale, const float* shift, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                      float* workspace, const float* ls, int accumulate, int* flag, gnx_stream_t stream);
int gnx_h16_cols_to_f32(const void* G16, long ldg, float* out, long ldo, long M, int C, const float* ls, int* flag,
                        gnx_stream_t stream);
/* `_lb` forms (round 5): the same kernels with the block buffer X16, its gradient G16, the pooled gradient dP16 and the
 * activated bottleneck A16 each addressed through (ld, bs) - element (row, c) at row * ld + (c >> 5) * bs + (c & 31).
 * (ld, 32) is the row-major [rows][ld] matrix of the entry points above; (32, rows_total * 32) is the CHANNEL-BLOCKED form
 * [C / 32][rows_total][32] of gnx_dense_layer_f16_tape, so the gradient path of gridnext/densenet.py:35-54 runs forward and
 * backward on the same buffers (a layer's dY = its own 32-channel block: pass that block's address with lddy = 32).
 * Same workspaces; gnx_conv1x1_dgrad_wgrad_bnrelu_bwd_f16_lb with dW == NULL is the pass without the weight gradient
 * (workspace gnx_conv1x1_dgrad_bnrelu_bwd_f16_workspace). */
/* The fp16 operands of one dense layer's backward from its fp32 weights in one launch (densenet.py:35-44 backwards; bn_size *
 * growth = 128, growth = 32): W1t16 [K][128] = conv1.weight [128][K] transposed, W2b16 [9][128][32] = conv2.weight
 * [32][128][3][3] as [tap][m][n]; each value rounded once. */
int gnx_dense_bwd_f16_pack(const float* w1, const float* w2, void* W1t16, void* W2b16, int K, gnx_stream_t stream);
int gnx_wgrad3x3_f16_lb(const void* dY16, long lddy, const void* A16, long lda, long bsa, float* dW, float* workspace, long M, int S,
                        const float* ls, int accumulate, int* flag, gnx_stream_t stream);
int gnx_conv3x3_dgrad_bnrelu_bwd_f16_lb(const void* dY16, long lddy, const void* W2b16, const void* A16, long lda, long bsa,
                                        void* dB16, long M, int S, const float* scale2, const float* gamma2, const float* beta2,
                                        float* dgamma, float* dbeta, float* workspace, const float* ls, int accumulate, int* flag,
                                        gnx_stream_t stream);
/* conv2's WHOLE backward in one pass over dY16 and A16 (round 5): dB16, dgamma2 / dbeta2 (= gnx_conv3x3_dgrad_bnrelu_bwd_f16_lb)
 * and dW2 [32][128][3][3] (= gnx_wgrad3x3_f16_lb) - a workgroup of eight waves stages each 128-pixel tile once, four waves take
 * the data gradient, four the weight gradient: 576 instead of 896 bytes per pixel.  S in {4, 8, 16, 32, 64}, 128 | M; otherwise
 * GNX_ERR_UNSUPPORTED (make the two calls).  workspace: gnx_conv3x3_bwd_f16_workspace(M) floats. */
long gnx_conv3x3_bwd_f16_workspace(long M);
int gnx_conv3x3_bwd_f16_lb(const void* dY16, long lddy, const void* W2b16, const void* A16, long lda, long bsa, void* dB16, float* dW,
                           long M, int S, const float* scale2, const float* gamma2, const float* beta2, float* dgamma,
                           float* dbeta, float* workspace, const float* ls, int accumulate, int* flag, gnx_stream_t stream);
int gnx_conv1x1_dgrad_wgrad_bnrelu_bwd_f16_lb(const void* dB16, const void* W1t16, const void* X16, long ldx, long bsx, void* G16,
                                              long ldg, long bsg, long M, int K, const float* scale, const float* shift,
                                              const float* mean, const float* invstd, float* dgamma, float* dbeta, float* dW,
                                              float* workspace, const float* ls, int accumulate, int* flag, gnx_stream_t stream);
int gnx_tail_bwd_f16_lb(const float* dfeats, long ldf, const void* X16, long ldx, long bsx, void* G16, long ldg, long bsg, long imgs,
                        int C, int S2, const float* scale, const float* shift, const float* mean, const float* invstd,
                        float* dgamma, float* dbeta, float* workspace, const float* ls, int accumulate, int* flag,
                        gnx_stream_t stream);
int gnx_trans_bwd_f16_lb(const void* dP16, long ldp, long bsp, const void* X16, long ldx, long bsx, void* G16, long ldg, long bsg,
                         long imgs, int C, int S, const float* scale, const float* shift, const float* mean, const float* invstd,
                         float* dgamma, float* dbeta, float* workspace, const float* ls, int accumulate, int* flag,
                         gnx_stream_t stream);
long gnx_stem_bwd_f16_workspace(long imgs, int P);
int gnx_stem_bwd_f16(const float* x, const float* w, const float* scale, const float* shift, const float* gamma, const float* beta,
                     const void* G16, long ldg, float* dW, float* dgamma, float* dbeta, float* workspace, long imgs, int P, int O,
                     const float* ls, int accumulate, int* flag, gnx_stream_t stream);
/* Which body a call of the fp16 gradient path runs and on what plan, without launching it (the launchers act on the same plan;
 * DESIGN.md, "fp16 backward forms"; tests/bwd_f16_ref.py restates the dispatch).  Each query takes its entry point's arguments in
 * its order, without the stream (the `_lb` arguments where there is one; gnx_conv1x1_dgrad_wgrad_bnrelu_bwd_f16_form: dW NULL or
 * not picks the kernel and the slab cap); every out-pointer may be NULL; nothing is launched, no operand is read.  They return a
 * GNX_B16_* / GNX_H16_* code; a call that returns an error: that GNX_ERR_* and 0 in every out value.  *workgroups = the grid of
 * the first launch (padding workgroups included), *slabs = the workspace slabs it writes, *tiles_per_slab = the 64-row (conv2's
 * data gradient: 128-row) tiles of every slab but the last.  gnx_conv3x3_bwd_f16_form: *workgroups = the workgroups that own a
 * tile (= slabs of each workspace half).  tail / trans: *slots = the image / pooled-pixel slots (= workspace slabs), *blocked =
 * the channel-blocked thread map.  gnx_conv1x1_bnrelu_h16[_cb]_form: *workgroups = the whole grid; M == 0: GNX_H16_M128, 0. */
#define GNX_B16_WG1 0     /* wgrad1x1_f16_kernel<false>: the operand as it is */
#define GNX_B16_WG1_ACT 1 /* <true>: relu(scale x + shift) applied while staging */
#define GNX_B16_WG3 2     /* wgrad3x3_f16_kernel: any S <= 64, any M */
#define GNX_B16_WG3_PAD 3 /* wgrad3x3_f16_p2_kernel<S>: zero-padded dY image, S in {4, 8, 16, 32, 64}, 64 | M */
#define GNX_B16_DG3 4     /* dgrad3x3_bn_f16_kernel<0>: any S <= 64, any M */
#define GNX_B16_DG3_PAD 5 /* dgrad3x3_bn_f16_kernel<S>: S in {4, 8, 16, 32, 64}, 128 | M */
#define GNX_B16_C3 6      /* conv3x3_bwd_f16_kernel<S>: both roles in one workgroup, S in {4, 8, 16, 32, 64}, 128 | M */
#define GNX_B16_DG1 7     /* dgrad1x1_bn_f16_kernel<false>: up to 768 workgroups */
#define GNX_B16_DG1_WG 8  /* <true>: with conv1's weight gradient, up to 512 workgroups */
#define GNX_B16_TAIL 9    /* tail_bwd_f16_kernel */
#define GNX_B16_TRANS 10  /* trans_bwd_f16_kernel */
#define GNX_H16_M128 11   /* conv1x1_h16_kernel: 128-row tiles, M < 131072 */
#define GNX_H16_M256 12   /* conv1x1_h16_m256_kernel: 256-row tiles, M >= 131072 */
int gnx_wgrad1x1_f16_form(const void* dY16, long lddy, const void* X16, long ldx, const float* scale, const float* shift,
                          const float* dW, const float* workspace, long M, int N, int K, const float* ls, int accumulate,
                          const int* flag, int* workgroups, int* slabs, int* tiles_per_slab);
int gnx_wgrad3x3_f16_form(const void* dY16, long lddy, const void* A16, long lda, long bsa, const float* dW, const float* workspace,
                          long M, int S, const float* ls, int accumulate, const int* flag, int* workgroups, int* slabs,
                          int* tiles_per_slab);
int gnx_conv3x3_dgrad_bnrelu_bwd_f16_form(const void* dY16, long lddy, const void* W2b16, const void* A16, long lda, long bsa,
                                          const void* dB16, long M, int S, const float* scale2, const float* gamma2,
                                          const float* beta2, const float* dgamma, const float* dbeta, const float* workspace,
                                          const float* ls, int accumulate, const int* flag, int* workgroups, int* slabs,
                                          int* tiles_per_slab);
int gnx_conv3x3_bwd_f16_form(const void* dY16, long lddy, const void* W2b16, const void* A16, long lda, long bsa, const void* dB16,
                             const float* dW, long M, int S, const float* scale2, const float* gamma2, const float* beta2,
                             const float* dgamma, const float* dbeta, const float* workspace, const float* ls, int accumulate,
                             const int* flag, int* workgroups, int* tiles_per_workgroup);
int gnx_conv1x1_dgrad_wgrad_bnrelu_bwd_f16_form(const void* dB16, const void* W1t16, const void* X16, long ldx, long bsx,
                                                const void* G16, long ldg, long bsg, long M, int K, const float* scale,
                                                const float* shift, const float* mean, const float* invstd, const float* dgamma,
                                                const float* dbeta, const float* dW, const float* workspace, const float* ls,
                                                int accumulate, const int* flag, int* workgroups, int* slabs, int* tiles_per_slab);
int gnx_tail_bwd_f16_form(const float* dfeats, long ldf, const void* X16, long ldx, long bsx, const void* G16, long ldg, long bsg,
                          long imgs, int C, int S2, const float* scale, const float* shift, const float* mean, const float* invstd,
                          const float* dgamma, const float* dbeta, const float* workspace, const float* ls, int accumulate,
                          const int* flag, int* slots, int* workgroups, int* blocked);
int gnx_trans_bwd_f16_form(const void* dP16, long ldp, long bsp, const void* X16, long ldx, long bsx, const void* G16, long ldg,
                           long bsg, long imgs, int C, int S, const float* scale, const float* shift, const float* mean,
                           const float* invstd, const float* dgamma, const float* dbeta, const float* workspace, const float* ls,
                           int accumulate, const int* flag, int* slots, int* workgroups, int* blocked);
int gnx_conv1x1_bnrelu_h16_form(const void* A16, long lda16, const void* W16, const void* out16, long ldc16, long M, int N, int K,
                                const float* scale, const float* shift, const float* out_scale, const float* out_shift,
                                int* workgroups);
int gnx_conv1x1_bnrelu_h16_cb_form(const void* A16, long lda16, const void* W16, const void* out16, long rows_total, long M, int N,
                                   int K, const float* scale, const float* shift, const float* out_scale, const float* out_shift,
                                   int* workgroups);

/* ---- content fingerprint: the key of the frozen-classifier row cache ------------------------------------------
 * train_gridwise evaluates the frozen f on every array in every epoch (gridnext/training.py:126 forces
 * patch_classifier.eval(), :146 calls model(inputs)); a frozen f maps equal bytes to equal rows, so the grid models
 * (gridnext_amd/fcache.py) keep each array's rows under a fingerprint of its bytes and skip f when they see it again.
 *
 * The fingerprint F(bytes[0 .. n)) is a pair of 64-bit words.  All arithmetic is modulo 2^64, >> is a logical shift:
 *   mix(x; a, b):  x ^= x >> 30;  x *= a;  x ^= x >> 27;  x *= b;  x ^= x >> 31;  return x      (splitmix64's finalizer)
 *   K0 = 0x9E3779B97F4A7C15   K1 = 0xC2B2AE3D27D4EB4F   M1 = 0xBF58476D1CE4E5B9   M2 = 0x94D049BB133111EB
 *   w_i, i = 0 .. ceil(n / 8) - 1: the bytes 8 i .. 8 i + 7 read as one little-endian 64-bit word, bytes at n and
 *                                  beyond taken as zero
 *   S0 = sum_i mix(w_i ^ ((i + 1) K0); M1, M2)          S1 = sum_i mix(w_i ^ ((i + 1) K1); M2, M1)
 *   F  = ( mix(S0 + (n + 1) K0; M1, M2),  mix(S1 + (n + 1) K1; M2, M1) )
 * It is a function of the bytes and of n alone - not of the address, its alignment, the grid or the order of the
 * partial sums (a sum modulo 2^64 has none).  mix is a bijection, so changing one word always changes both sums; the
 * position enters each term, so the value depends on the order of the words; n enters last, so buffers of zeros of
 * different lengths differ.  NOT cryptographic: equal fingerprints are easy to construct on purpose.  For data nobody
 * constructed, the two words behave as 128 independent random bits: among N different buffers the chance that any two
 * share a fingerprint is about N^2 / 2^129 (10^6 arrays: 1.5e-27).
 *
 * gnx_fingerprint128_batch: out[s][0 .. 2) = F of the seg_bytes bytes at base + s * seg_bytes, s = 0 .. n_seg - 1.
 * Any byte alignment of base, any seg_bytes (0 included); no byte outside [base, base + n_seg * seg_bytes) is read.
 * Segments of at most gnx_fingerprint128_split_bytes() bytes (32 768) - or more than 1 024 segments - take one workgroup
 * each in ONE launch and no workspace; longer ones are cut into parts of that size (as many as keep the grid within
 * 2 048 workgroups, then larger parts) whose sums go through `workspace` (gnx_fingerprint128_batch_workspace bytes,
 * 8-byte aligned; every word of it that is read was written by the same call) to a second, small launch.  Both forms
 * give the same bits.  out: 8-byte aligned, written with ordinary vector stores; no atomics. */
long gnx_fingerprint128_split_bytes(void);
long gnx_fingerprint128_batch_workspace(size_t seg_bytes, int n_seg); /* bytes; 0: the one-launch form */
int gnx_fingerprint128_batch(const void* base, size_t seg_bytes, int n_seg, uint64_t* out /* [n_seg][2] */, void* workspace,
                             gnx_stream_t stream);

/* ---- Colour-cast removal of a resident whole-slide image ---------------------------------------------------------------
 * The reference's remove_color_cast / scale_rgb (gridnext/imgprocess.py:49-67) take np.percentile(channel, q=99) of the whole
 * slide per channel and apply Image.point(i -> i * 255 / p) to every byte.  Here the slide is resident as interleaved uint8
 * [n_pixels][3] at ANY byte alignment, and the work is two streaming passes; the percentiles and the table
 * clip(round(i * scale), 0, 255) are the host's (gridnext_amd/imgprocess.py), in double, between the two.  All indexing and all
 * totals are 64-bit (n_pixels may exceed 2^32); no byte outside the image is read or written; no atomics on global memory.
 *
 * gnx_rgb_hist_u8: hist[c][v] = the number of pixels whose channel c holds v.  hist (device, 8-byte aligned, [3][256]) is
 * OVERWRITTEN; n_pixels == 0 gives all zeros.  workspace: gnx_rgb_hist_u8_workspace(n_pixels) bytes, 8-byte aligned (one slab
 * of partial sums per workgroup; every word that is read was written by the same call).  Integer sums: the result does not
 * depend on the launch geometry or on the alignment.
 *
 * gnx_rgb_lut_u8: dst[3 p + c] = lut[c][src[3 p + c]], lut device uint8 [3][256].  src and dst at any alignment, independently;
 * dst == src (in place) is allowed; ranges that overlap without being equal are GNX_ERR_BAD_ARG and nothing is launched. */
long gnx_rgb_hist_u8_workspace(size_t n_pixels); /* bytes */
int gnx_rgb_hist_u8(const unsigned char* img, size_t n_pixels, uint64_t* hist /* [3][256] */, void* workspace,
                    gnx_stream_t stream);
int gnx_rgb_lut_u8(const unsigned char* src, unsigned char* dst, size_t n_pixels, const unsigned char* lut /* [3][256] */,
                   gnx_stream_t stream);

/* ---- Train-time augmentation of uint8 patches on the device ------------------------------------------------------------
 * The reference leaves augmentation to the `img_transforms` hook of its datasets (gridnext/image_datasets.py:102-105 and
 * :184-187): per-patch PIL calls on the host.  Here the patches are already on the device, src [n][3][P][P] uint8 at ANY base
 * alignment, and one launch writes dst, dst_n patches of the same shape (bytes, or floats in the _f32 form):
 *   codes [n] device uint8, or NULL = the identity on every patch.  Only the low three bits count: code = 4 f + r is
 *     out = rot90^r(fliplr^f(x)), exactly torch.rot90(x.flip(-1) if f else x, r, (-2, -1)); in Pillow's Image.transpose:
 *     1, 2, 3 = ROTATE_90, ROTATE_180, ROTATE_270; 4 = FLIP_LEFT_RIGHT; 5 = TRANSPOSE; 6 = FLIP_TOP_BOTTOM; 7 = TRANSVERSE.
 *   luts [n][3][256] device uint8 at any alignment, or NULL: byte b of channel c of patch k becomes luts[k][c][b] (a per-pixel
 *     map commutes with the permutation, so the order of the two does not matter).
 *   dst_rows [n] device int32, or NULL = k -> k: patch k is written to row dst_rows[k] of dst.  An index outside [0, dst_n) is
 *     skipped, nothing is written for it; every index is checked before it addresses anything.  Distinct rows are the caller's
 *     duty.  (A compact gather of the in-tissue spots lands in the cells of a zero-filled (78, 64, 3, P, P) grid this way.)
 *   The _f32 form stores ToTensor (+ Normalize, norm = {mean[3], std[3], 1/std[3]} or NULL) of the byte result - the floats
 *     gnx_u8_to_f32 gives for the u8 form's output, bit for bit.
 * Where P % 4 == 0 and the bases are aligned (4 bytes; 16 for the float destination) all global traffic is dwords or wider; any
 * other P or alignment is computed byte by byte.  The four transposing codes go through an LDS tile, so reads and writes both
 * run along rows.  All byte offsets are 64-bit.  n == 0: GNX_OK, nothing is written.  GNX_ERR_BAD_ARG (nothing is launched): a
 * NULL src or dst with n > 0, P <= 0, n < 0, dst_n < 0, dst_n < n with a NULL dst_rows, a source range that overlaps the
 * destination range (there is no in-place form).  GNX_ERR_UNSUPPORTED: P > 32768.
 *
 * gnx_patch_grey_sum_u8: sums[k] = the sum over the pixels of patch k of (19595 R + 38470 G + 7471 B + 0x8000) >> 16, Pillow's
 * convert('L'): exact integers, one reduction per patch in a fixed structure, no atomics.  sums: device, 8-byte aligned, [n]. */
int gnx_patch_augment_u8(const unsigned char* src, unsigned char* dst, long n, int P, long dst_n, const unsigned char* codes,
                         const unsigned char* luts, const int* dst_rows, gnx_stream_t stream);
int gnx_patch_augment_u8_f32(const unsigned char* src, float* dst, long n, int P, long dst_n, const unsigned char* codes,
                             const unsigned char* luts, const int* dst_rows, const float* norm, gnx_stream_t stream);
int gnx_patch_grey_sum_u8(const unsigned char* src, long n, int P, unsigned long long* sums, gnx_stream_t stream);

/* ---- Saturation and hue jitter of uint8 patches on the device ----------------------------------------------------------
 * The other half of torchvision's ColorJitter, which the reference would reach through the same `img_transforms` hook
 * (gridnext/image_datasets.py:102-105 and :184-187) as per-patch PIL calls: ImageEnhance.Color and torchvision's adjust_hue
 * (convert('HSV'), the H plane plus a shift modulo 256, convert('RGB')).  Neither is a per-channel byte map - a pixel's three
 * channels are needed at once - so this is a launch of its own: gnx_patch_augment_u8[_f32] with two more per-patch operands,
 *   sat [n] device float32 (4-byte aligned), or NULL = no saturation stage: every channel c of a pixel becomes Pillow's
 *     Image.blend of the pixel's grey value L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 with c, in float32 without
 *     contraction: t = float(L) + sat[k] * float(c - L); 0 <= sat[k] <= 1 truncates t, any other factor gives 0 where
 *     t <= 0, 255 where t >= 255 and truncates elsewhere.  A NaN factor is the caller's error (the bytes are unspecified).
 *   hue [n] device uint8, or NULL = no hue stage: the pixel goes to Pillow's HSV bytes, hue[k] is added to H modulo 256, and
 *     the result goes back to RGB, in Pillow's float / double arithmetic operation for operation (gridnext_amd/transforms.py:
 *     rgb_to_hsv_u8, hsv_to_rgb_u8).  A present stage makes the round trip even with hue[k] == 0, and the round trip is lossy:
 *     that is what Pillow gives.
 * Per patch: the turn, then luts, then saturation, then hue, then the byte or float store.  Every other argument, the freedom
 * of alignment, the refusals and the error codes are those of gnx_patch_augment_u8[_f32]; additionally a sat that is not
 * 4-byte aligned is GNX_ERR_BAD_ARG.  With sat == hue == NULL the result equals gnx_patch_augment_u8[_f32]'s.  The unit of
 * work is a 64 x 64 tile of a patch with all three planes; no atomics, no in-place form. */
int gnx_patch_augment_hs_u8(const unsigned char* src, unsigned char* dst, long n, int P, long dst_n, const unsigned char* codes,
                            const unsigned char* luts, const float* sat, const unsigned char* hue, const int* dst_rows,
                            gnx_stream_t stream);
int gnx_patch_augment_hs_u8_f32(const unsigned char* src, float* dst, long n, int P, long dst_n, const unsigned char* codes,
                                const unsigned char* luts, const float* sat, const unsigned char* hue, const int* dst_rows,
                                const float* norm, gnx_stream_t stream);

/* ---- Evaluation metrics on the device -----------------------------------------------------------------------------------
 * The numeric half of the reference's gridnext/plotting.py, which goes through sklearn on host arrays.  All pointers are
 * device pointers; outputs and workspaces are the caller's; nothing is allocated or kept inside the library; every launch
 * goes to `stream`.  Each `bad` word (int64, 8-byte aligned) is OVERWRITTEN by its call: zeroed, then counted into.
 *
 * gnx_confusion_counts (plotting.py:103-134, sklearn's confusion_matrix): counts[t][p] = the number of i with y_true[i] == t
 *   and y_pred[i] == p; int64 [K][K], rows true, columns predicted, OVERWRITTEN (the call zeroes it).  Per-workgroup 32-bit
 *   LDS counters, flushed with 64-bit vector atomics: integer adds, so the result is exact and independent of the order.  A
 *   pair with either label outside [0, K) is not counted; it adds one to *bad.  GNX_ERR_BAD_ARG: n <= 0, K <= 0, a NULL
 *   pointer.  GNX_ERR_UNSUPPORTED: K > gnx_confusion_max_classes() = 64 (K * K counters of 4 bytes: 16 KB of LDS), n > 2^40.
 *
 * gnx_clf_curve (plotting.py:14-98: label_binarize, roc_curve, precision_recall_curve and auc per class): the binary
 *   classifier curve of every class c in [0, C) in one call.  scores: float32 [n][ld] row-major, ld >= C, column c the score of
 *   class c; y_true: int64 [n]; sample i is a positive of class c iff y_true[i] == c, any other value (outside [0, C) too) is a
 *   negative for every class.  Per class, over the DISTINCT score values in descending order (-0.0 and +0.0 are one value,
 *   reported as +0.0; denormals are distinct values; +-inf are ordinary values):
 *     thresholds[c * n + k]   the k-th distinct score,
 *     tps / fps[c * n + k]    int64: positives / negatives with a score >= that value,
 *     n_thresholds[c] = T_c   the number of distinct values; only the first T_c entries of a row are written.
 *   thresholds, tps and fps (row stride n) may each be NULL when only the areas are wanted.  auroc[c], auprc[c]: float64.
 *     auroc = S / (2 P N), S = sum_k (fp_k - fp_{k-1}) (tp_k + tp_{k-1}) in int64, tp_0 = fp_0 = 0, P positives, N negatives:
 *       one division of two converted integers.  Needs 2 P N < 2^63, which n < 2^31 guarantees; below 2 P N < 2^53 both
 *       conversions are exact and the result is the correctly rounded rational.
 *     auprc = sum_k (r_k - r_{k-1}) (p_k + p_{k-1}) / 2, r_k = tp_k / P, p_k = tp_k / (tp_k + fp_k), r_0 = 0, p_0 = 1:
 *       sklearn 1.7's auc(recall, precision).  float64, summed in a fixed order (per thread in index order, per workgroup in a
 *       fixed tree, the workgroups' partial sums in index order): equal inputs give equal bits; no floating-point atomics.
 *     A class without positives: auroc NaN, auprc 0.5.  A class without negatives: auroc NaN, auprc 1.0.
 *   A NaN score has no place in the order: *bad = the number of NaN scores in the C columns; the other outputs are then
 *   unspecified (but stay in bounds).  The order is a stable LSD radix sort (four passes of 8-bit digits over a key built
 *   from the float's bits; see gridnext_amd/csrc/metrics.hip).  A class's launch geometry depends on n alone: a column gives
 *   the same bits alone and among others.  Elements are handled in tiles of gnx_clf_curve_tile() by at most
 *   gnx_clf_curve_max_groups() workgroups per class.
 *   workspace: gnx_clf_curve_workspace(n, C) bytes (0 for arguments gnx_clf_curve refuses), 8-byte aligned; every word that is
 *   read was written by the same call.  GNX_ERR_BAD_ARG (nothing is launched, nothing written): n <= 0, C <= 0, ld < C, a NULL
 *   scores, y_true, n_thresholds, auroc, auprc, bad or workspace.  GNX_ERR_UNSUPPORTED: n >= 2^31, C > 65535.
 *
 * gnx_misclass_density (plotting.py:138-149): out[y][x] = (double)(1.0f - smax[true[y][x] - 1][y][x]) where true[y][x] > 0,
 *   else 0.0; smax float32 [C][H][W], true int64 [H][W], out float64 [H][W].  The subtraction is float32's, as numpy's on the
 *   reference's float32 input.  A label above C reads nothing, stores 0.0 and adds one to *bad. */
long gnx_clf_curve_tile(void);
long gnx_clf_curve_max_groups(void);
long gnx_confusion_max_classes(void);
int gnx_confusion_counts(const long long* y_true, const long long* y_pred, long n, int K, long long* counts /* [K][K] */,
                         long long* bad, gnx_stream_t stream);
long gnx_clf_curve_workspace(long n, int C); /* bytes */
int gnx_clf_curve(const float* scores, long ld, const long long* y_true, long n, int C, float* thresholds, long long* tps,
                  long long* fps, long long* n_thresholds, double* auroc, double* auprc, long long* bad, void* workspace,
                  gnx_stream_t stream);
int gnx_misclass_density(const float* smax, const long long* true_labels, int C, long H, long W, double* out, long long* bad,
                         gnx_stream_t stream);

/* ---- Sparse count matrices on the device ---------------------------------------------------------------------------------
 * The count side of the reference's tutorial (notebooks/Tutorial_visium_count.ipynb): an AnnData with a scipy-sparse X
 * (visium_datasets.py:221-272), sc.pp.normalize_total and sc.pp.log1p on it, X.mean(0) / X.std(0) for the gene selection, and
 * the dense tensors of anndata_to_tensordataset (count_datasets.py:347-376) and anndata_to_grids (utils.py:197-217).  Here the
 * matrix stays sparse and resident, and an item is densified by one launch.
 *
 * A LINE is a row of a CSR matrix or a column of a CSC matrix: line l owns the entries lineptr[l] .. lineptr[l + 1] of idx
 * (int32, strictly increasing within a line) and val (fp32); lineptr is int64.  All pointers are device pointers.
 *   lines       optional int32 [n_lines]: which lines, in which order (repeats allowed); NULL: the lines 0 .. n_lines - 1.
 *               A negative entry is an empty line in every entry point that takes a list, here and in the blocks below
 *               (gene_lines): no entry is read for it (the matrix has at least one line: lineptr[0] and lineptr[1] are
 *               read), expand writes a row of zeros, the moments are 0, 0, the maximum is 0.
 *   pos_of_idx  optional int32 map idx -> position; a negative value drops the entry; NULL: the identity.  The caller
 *               guarantees that it is injective on its non-negative values (two entries on one position would race).
 *   idx_mask    optional uint8 mask over indices, non-zero = counted; NULL: all.
 * No atomics; every result has one summation order; n_lines == 0 (n == 0) is GNX_OK and launches nothing.  More than
 * 2^31 - 1 lines: GNX_ERR_UNSUPPORTED.
 *
 * gnx_sparse_expand_f32 (count_datasets.py:347-376 with a CSR over spots, lines = a batch's spots, pos_of_idx = gene ->
 *   channel; utils.py:197-217 with one array's CSC, lines = the genes in channel order, pos_of_idx = spot -> odd-right cell,
 *   L = ld_out = H * W, which writes the contiguous (G, H, W) tensor): out[i * ld_out + p] for p in [0, L) = val[e] when an
 *   entry e of line i maps to p, else 0.0f.  Every such element is written exactly once, zeros included: no memset goes in
 *   front; the padding p in [L, ld_out) is not touched.  A position outside [0, L) drops the entry.  One workgroup per line
 *   and chunk of gnx_sparse_expand_chunk() = 8192 positions (32 KB of LDS).  GNX_ERR_BAD_ARG, nothing launched: L <= 0,
 *   ld_out < L, n_lines < 0, a NULL lineptr or out, an out that is not 4-byte aligned, a NULL idx or val with n_lines > 0.
 *   GNX_ERR_UNSUPPORTED: L > 65535 * 8192.
 * gnx_sparse_line_moments_f64 (the tutorial's X.sum(1) inside normalize_total: CSR lines, gene mask; its X.mean(0) and
 *   X.std(0) per array: the array's CSC lines, spot mask): out[2 i] = the sum, out[2 i + 1] = the sum of squares of the
 *   entries of line i whose idx_mask[idx] != 0, in double.  One wavefront per line: lane j adds the entries j, j + 64, ... in
 *   that order, then the fixed shuffle tree over the 64 lanes - equal inputs give equal bits.
 * gnx_sparse_line_max_f32 (the per-gene maximum that the [0, 1] expression target of notebooks/counts_from_img.ipynb divides
 *   by: an array's CSC lines; or CSR lines under a gene mask): out[i] = the largest of 0.0f and the entries of line i whose
 *   idx_mask[idx] != 0; a line without a kept entry gives 0, the implicit value (counts, raw or normalised, are not
 *   negative).  One wavefront per line, the same walk; a maximum has no order, so the result is exact.
 * gnx_sparse_line_clip_moments_f64 (the second pass of the Seurat-v3 gene selection, below: an array's CSC lines, clip[i] the
 *   bound of row i): the moments of the entries cut at their row's bound - per kept entry t = fmin((double) v, clip[i]);
 *   out[2 i] = the sum of t, out[2 i + 1] = the sum of t^2, every square entering its lane's sum through ONE fma, s2 =
 *   fma(t, t, s2), t * t being inexact in double when the bound is no fp32 number.  The walk and the tree are
 *   gnx_sparse_line_moments_f64's: with clip[i] = +inf the two give equal bits (v * v is exact).  A NaN bound does not clip
 *   (fmin).  A NULL clip is GNX_ERR_BAD_ARG, in the place of a NULL out in the order of the status codes.
 * gnx_sparse_div_by_line_f32 / gnx_sparse_div_by_idx_f32 (the division inside sc.pp.normalize_total, for a CSR over spots
 *   and for a CSC whose indices are spots): in place val[e] = val[e] / divisor[line of e], over the lines 0 .. n_lines - 1;
 *   and val[e] = val[e] / divisor[idx[e]] over the entries 0 .. n - 1.  IEEE round-to-nearest fp32 division, numpy's bits.
 * gnx_log1p_f32 (sc.pp.log1p): in place val[e] = log1pf(val[e]), e in [0, n). */
long gnx_sparse_expand_chunk(void);
int gnx_sparse_expand_f32(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                          const int* pos_of_idx, float* out, long ld_out, long L, gnx_stream_t stream);
int gnx_sparse_line_moments_f64(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                                const uint8_t* idx_mask, double* out /* [n_lines][2] */, gnx_stream_t stream);
int gnx_sparse_line_clip_moments_f64(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                                     const uint8_t* idx_mask, const double* clip /* [n_lines], row i's bound */,
                                     double* out /* [n_lines][2] */, gnx_stream_t stream);
int gnx_sparse_line_max_f32(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                            const uint8_t* idx_mask, float* out /* [n_lines] */, gnx_stream_t stream);
int gnx_sparse_div_by_line_f32(const long long* lineptr, float* val, long n_lines, const float* divisor, gnx_stream_t stream);
int gnx_sparse_div_by_idx_f32(const int* idx, float* val, long n, const float* divisor, gnx_stream_t stream);
int gnx_log1p_f32(float* val, long n, gnx_stream_t stream);

/* ---- A Linear layer over sparse count rows ---------------------------------------------------------------------------------
 * The first layer of the count classifier (Tutorial_visium_count.ipynb cell 12: nn.Linear(G, 500) on a spot's G counts) without
 * the dense operand: the forward is an SpMM over the resident CSR, the weight gradient an SpMM over the resident per-array
 * CSCs.  Lines, lineptr, idx and val are the sparse-count block's; all pointers are device pointers; no atomics.
 *
 * The weight is GENE-MAJOR: W[G][F], row g the F output features of gene (channel) g, ldw >= F - the transpose of
 * nn.Linear.weight - so an entry gathers one contiguous row of F floats.
 *
 * Summation order, both entry points: per output element ONE chain, acc = 0.0f, then acc = fmaf(val[e], row(e)[f], acc) over
 * the kept entries e of the line in entry order, then the element = init + acc with init the bias (forward), the element as it
 * is (accumulate) or 0.0f.  The chain depends on the line alone: an output row has the same bits alone, in any batch, at any
 * position, at any 4-byte alignment of any buffer, for any ld, and on a second call.  With n kept entries the element lies
 * within g T of the exact value, g = (n + 1) u / (1 - (n + 1) u), u = 2^-24, T = |init| + sum |val[e] row(e)[f]|.
 *
 * gnx_sparse_linear_fwd_f32: for i < n_lines, f < F: out[i * ld_out + f] = bias[f] + sum over the entries e of line lines[i]
 *   of val[e] * W[chan(idx[e]) * ldw + f].  bias NULL: 0.0f in its place.  lines: optional int32 [n_lines], repeats allowed,
 *   a NEGATIVE value = no line (the row is the bias alone: an empty cell of a grid); NULL: the lines 0 .. n_lines - 1.
 *   chan_of_idx: optional int32 map gene -> channel, a negative value drops the entry; NULL: the identity.  The caller
 *   guarantees channels below the rows of W.  Every out[i][0 .. F) is written exactly once, no memset goes in front, the
 *   padding [F, ld_out) is not touched.
 * gnx_sparse_linear_wgrad_f32, over ONE array's CSC (lines = genes, idx = the spot's row within the array): for c < n_channels,
 *   f < F: dW[c * ldw + f] (+)= sum over the entries e of line gene_lines[c] (NULL: line c; negative: no line) with
 *   pos_of_idx[idx[e]] >= 0 of val[e] * dY[pos_of_idx[idx[e]] * ld_dy + f], in entry order = the array's row order.
 *   pos_of_idx: int32 map row of this array -> position (row of dY) in the batch, or -1; NULL: the identity.  accumulate == 0
 *   writes every dW[c][0 .. F), zeros included; accumulate != 0 adds the line's sum to what is there: the caller walks its
 *   arrays in a fixed order and the first call writes.  The order is storage order, not batch order: dW has the same bits
 *   under any permutation of the batch (rows of dY permuted along).
 * One workgroup per (line, slice of F), a thread per 4 adjacent features where W / dY and its leading dimension are 16-byte
 *   multiples, else per feature: the same chains either way.
 * GNX_ERR_BAD_ARG, nothing launched: F <= 0, ldw < F, ld_out < F, ld_dy < F, a negative count, a NULL lineptr / W / out / dY /
 *   dW, a NULL idx or val with a positive count, a W / out / bias / dY / dW / val that is not 4-byte aligned.
 *   GNX_ERR_UNSUPPORTED: more than 2^31 - 1 lines, F > gnx_sparse_linear_max_f() = 1048576.  A count of 0: GNX_OK, no launch.
 * The bias gradient is gnx_colsum of dY; there is no input gradient (the input is an index list). */
long gnx_sparse_linear_max_f(void);
int gnx_sparse_linear_fwd_f32(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                              const int* chan_of_idx, const float* W, long ldw, const float* bias, float* out, long ld_out,
                              long F, gnx_stream_t stream);
int gnx_sparse_linear_wgrad_f32(const long long* lineptr, const int* idx, const float* val, const int* gene_lines,
                                long n_channels, const int* pos_of_idx, const float* dY, long ld_dy, float* dW, long ldw, long F,
                                int accumulate, gnx_stream_t stream);

/* ---- The Gram matrix of sparse counts ------------------------------------------------------------------------------------
 * The hot part of fitting a PCA on resident counts (scripts/fit_pca_unified_cortex.py:33-100: PCA().fit on the normalised,
 * log1p'd, z-scored training arrays; its PCs are what use_pcs selects in count_datasets.py:309-342, :347-376, :382-422,
 * :427-475 and utils.py:197-205): the genes x genes second-moment matrix X^T X, in double, from ONE array's CSC and the
 * storage's CSR.  Lines, lineptr, idx and val are the sparse-count block's; all pointers are device pointers; no atomics.
 *
 * gnx_sparse_gram_f64: for a, b < n_channels: C[a * ldc + b] (+)= the double sum, over the entries e of CSC line gene_lines[a]
 *   (NULL: line a; negative: no line, the row is zeros) with spot r = csc_idx[e] and value v = csc_val[e], and over the
 *   entries e' of CSR line row0 + r with chan_of_idx[csr_idx[e']] == b, of (double) v * (double) csr_val[e'].  The product of
 *   two fp32 values is exact in double: only the additions round, and sums of integer products below 2^53 are exact.
 *   row0: the CSR row of the array's first spot.  chan_of_idx: optional int32 map gene -> channel, a negative value (or one
 *   of n_channels or more) drops the entry; NULL: the identity.  The caller guarantees that it is injective on its kept
 *   values (two entries of a row on one channel would race).
 *   Every C[a][0 .. n_channels) is written exactly once per call, zeros included: no memset goes in front; the padding
 *   [n_channels, ldc) is not touched.  accumulate != 0 adds the array's sum to what is there: the caller walks its arrays in
 *   a fixed order and the first call writes.  The full matrix is written; symmetry is not used.
 * Summation order: one workgroup per (row a, chunk of gnx_sparse_gram_chunk() = 2048 columns) with 4 wavefronts; wavefront w
 *   adds the entries k = w, w + 4, ... of line a, in that order, into its own strip of doubles in the LDS (4 x 2048 x 8 bytes
 *   = 64 KB at most), its lanes striding the spot's CSR row; then element = strip 0 + strip 1 + strip 2 + strip 3, in that
 *   order, (+ C when accumulating).  A function of the inputs alone: a second call gives equal bits.  With n terms an element
 *   lies within n 2^-53 sum |v u| of the exact value.
 * GNX_ERR_BAD_ARG, nothing launched: n_channels < 0, ldc < n_channels, row0 < 0, a NULL csc_ptr, csr_ptr or C, a NULL idx or
 *   val with n_channels > 0, a C that is not 8-byte aligned, a val that is not 4-byte aligned.  GNX_ERR_UNSUPPORTED:
 *   n_channels > 65535 * 2048.  n_channels == 0: GNX_OK, no launch. */
long gnx_sparse_gram_chunk(void);
int gnx_sparse_gram_f64(const long long* csc_ptr, const int* csc_idx, const float* csc_val, const int* gene_lines,
                        long n_channels, const long long* csr_ptr, const int* csr_idx, const float* csr_val, long row0,
                        const int* chan_of_idx, double* C, long ldc, int accumulate, gnx_stream_t stream);

/* ---- Per-gene moments of an expression prediction against sparse counts ------------------------------------------------
 * The evaluation stage of notebooks/counts_from_img.ipynb (a DenseNet whose head predicts a spot's [0, 1]-scaled expression
 * vector): which genes the image predicts - the per-gene Pearson correlation, R^2 and MSE between prediction and measured
 * expression over held-out spots - from five sums per gene channel, in double, without a dense (B, G) target.  Lines,
 * lineptr, idx and val are the sparse-count block's; all pointers are device pointers; no atomics; eager, forward only.
 *
 * The table: double M[G][ld_m], ld_m >= 5, row c the gene channel c:
 *   M[c][0] = sum p    M[c][1] = sum p^2    over the B rows of z                        (gnx_act_col_moments_f64)
 *   M[c][2] = sum t    M[c][3] = sum t^2    M[c][4] = sum p t    over the kept entries  (gnx_sparse_pred_moments_f64)
 *   The columns [5, ld_m) are never touched, and neither call touches the other's columns.
 * Per element: p = act((double) z), act the identity (GNX_ACT_NONE) or the sigmoid in double (GNX_ACT_SIGMOID) in its
 *   overflow-free two-branch form, 1 / (1 + exp(-z)) for z >= 0, else e / (1 + e) with e = exp(z): p lies in [0, 1] for every
 *   z that is not NaN, infinities included.  t = (double) fl32(val[e] * gene_scale[c]), the fp32 product that is the target of
 *   expression.SparseMSELoss for fp32 z; gene_scale NULL: t = val[e].  Squares and products enter the sums through
 *   fma(x, y, sum): t^2 is exact in double, so is the product of the fma before its one rounding.
 * accumulate == 0 writes the call's columns for every channel, zeros included: no memset goes in front.  accumulate != 0
 *   adds the call's sum to what is there (one more rounding per element): M = M + sum.
 *
 * gnx_act_col_moments_f64 (notebooks/counts_from_img.ipynb: nn.Sigmoid() on the head's output, per gene over the spots): z is
 *   row-major [B][ldz], ldz >= G, read along rows.  Summation order, per column: 128 strips; strip s adds the rows s,
 *   s + 128, s + 256, ... in that order, each from 0.0; then sum = ((strip 0 + strip 1) + strip 2) + ... + strip 127.  One
 *   workgroup per 8 adjacent columns (the double sigmoid bounds the kernel, so the columns are spread over many workgroups),
 *   8 threads per strip, the strips folded through the LDS by one thread per column.  The order depends on B alone - not on
 *   G, ldz, the alignment of z or M, or the other columns - and B is never split over workgroups: no workspace, no second
 *   launch, no counters.  B == 0 with accumulate == 0 writes zeros.
 * gnx_sparse_pred_moments_f64 (notebooks/counts_from_img.ipynb: nn.MSELoss against the spot's normalised counts, per gene),
 *   over ONE array's CSC with the conventions of gnx_sparse_linear_wgrad_f32: gene_lines[c] is the CSC line of channel c (NULL:
 *   line c; negative: no line, the channel's sums are 0); pos_of_idx maps a row of this array to a row of z, -1 drops the
 *   entry, NULL is the identity; the caller guarantees positions below the rows of z.  p is taken at z[pos * ldz + c],
 *   ldz >= n_channels.  One wavefront per line: lane j adds the kept ones of the entries j, j + 64, ... in that order, then
 *   the fixed shuffle tree over the 64 lanes - the walk of gnx_sparse_line_moments_f64.  The caller walks its arrays in a
 *   fixed order.
 * Both: equal inputs give equal bits.  With n terms added so far into an element, calls included, the element lies within
 *   (n + 16) 2^-53 sum |term| of the exact sum of the exact terms: any order of n additions is within n 2^-53 sum |term|,
 *   and 16 covers the roundings inside one term with more than twofold margin (exp, taken within 1 ulp in double, on both
 *   branches; the add, the divide, the product).
 * GNX_ERR_BAD_ARG, nothing launched: a NULL z, M or lineptr, a NULL idx or val with a positive count, a negative B, G or
 *   n_channels, ldz < G (< n_channels), ld_m < 5, an activation that is neither code, an M that is not 8-byte aligned, a z,
 *   val or gene_scale that is not 4-byte aligned.  GNX_ERR_UNSUPPORTED: G or n_channels above 2^31 - 1.  G == 0 or
 *   n_channels == 0: GNX_OK, no launch. */
#define GNX_ACT_NONE 0
#define GNX_ACT_SIGMOID 1
int gnx_act_col_moments_f64(const float* z, long ldz, long B, long G, int activation, double* M, long ld_m, int accumulate,
                            gnx_stream_t stream);
int gnx_sparse_pred_moments_f64(const long long* lineptr, const int* idx, const float* val, const int* gene_lines,
                                long n_channels, const int* pos_of_idx, const float* gene_scale, const float* z, long ldz,
                                int activation, double* M, long ld_m, int accumulate, gnx_stream_t stream);

/* ---- Highly variable genes, Seurat v3: the loess fit -------------------------------------------------------------------------
 * The reference chooses its genes from RAW counts (notebooks/register_hvgs.ipynb: sc.pp.highly_variable_genes(adata,
 * flavor='seurat_v3', n_top_genes=2150); the result is the select_genes of gridnext/count_datasets.py's datasets): per gene the
 * variance of the counts cut at a bound that a loess fit of log10(variance) on log10(mean) sets, over that fit's variance.
 * The two device parts are the clipped second pass over the counts (gnx_sparse_line_clip_moments_f64, in the sparse-count
 * block) and this fit; windows, ranking and the rest are host work (gridnext_amd/hvg.py, which fixes the arithmetic).
 *
 * gnx_loess_fit_f64: xs, ys: n doubles, xs sorted ascending.  Evaluation point i < n_eval <= n is x0 = xs[i]; it has the window
 *   [lo[i], lo[i] + cnt[i]) of positions (int32; cut to [0, n) by the kernel, so nothing else is ever read), inv_h[i] = 1 / h
 *   with h the window's largest distance to x0 (0.0: every weight is 1 and u is 0, which takes degree 0) and degree[i] in
 *   0 .. 2.  out[i] = beta_0 of the weighted least-squares polynomial of that degree in u = (x - x0) * inv_h with tricube
 *   weights w = (1 - |u|^3)^3 for |u| < 1, else 0: local regression without robustness iterations, evaluated directly.
 * Summation order: one wavefront per point; lane j takes the window's elements j, j + 64, ... in that order and adds, in double
 *   from 0.0, w, p1 = w u, p2 = p1 u, p3 = p2 u, p4 = p3 u (plain products, plain additions) and fma(w, y, .), fma(p1, y, .),
 *   fma(p2, y, .); the eight sums go through the fixed shuffle tree over the 64 lanes; lane 0 solves the (d + 1) x (d + 1)
 *   system of the moments m0 .. m4 and r0 .. r2 by LDL^T without pivoting: l10 = m1 / m0, l20 = m2 / m0, d1 = m2 - l10 m1,
 *   l21 = (m3 - l20 m1) / d1, d2 = (m4 - l20 m2) - l21 (l21 d1), z1 = r1 - l10 r0, z2 = (r2 - l20 r0) - l21 z1, b2 = z2 / d2,
 *   b1 = z1 / d1 - l21 b2, beta_0 = (r0 / m0 - l10 b1) - l20 b2 (degree 1: b2 = 0 and the terms with l20, l21 are absent;
 *   degree 0: r0 / m0), nothing contracted.  A function of the point's window alone: equal inputs give equal bits.  No atomics;
 *   out[i] is written exactly once, nothing beyond out[n_eval - 1].
 * GNX_ERR_BAD_ARG, nothing launched: n < 0, n_eval < 0, n_eval > n, with n_eval > 0 a NULL pointer or an xs, ys, inv_h or out
 *   that is not 8-byte aligned.  GNX_ERR_UNSUPPORTED: n > 2^31 - 1.  n_eval == 0: GNX_OK, no launch.  The degrees live on the
 *   device, where the launcher - which never synchronises - cannot read them: a point whose degree lies outside 0 .. 2 gets
 *   NaN, the other points are not affected; gridnext_amd/hvg.py refuses such a degree (ValueError) before anything is uploaded. */
int gnx_loess_fit_f64(const double* xs, const double* ys, long n, const int* lo, const int* cnt, const double* inv_h,
                      const int* degree, double* out, long n_eval, gnx_stream_t stream);

/* ---- Spatially variable genes: the neighbour sums of Moran's I and Geary's C -----------------------------------------------
 * The reference builds the spot graph of an array as an N x N pdist matrix (gridnext/graph_datasets.py:145-157: `0 < d <= 1`
 * on coordinates scaled by sqrt(3) / 2, with a TODO that asks for the O(N) enumeration); here the graph is a table of integer
 * offsets, nbr[r][k] = the row of spot r's k-th neighbour within the array or -1 (gridnext_amd/spatial.py, which fixes the
 * arithmetic of the two statistics), and the per-gene sums over it are one walk of the array's CSC.  Lines, lineptr, idx and
 * val are the sparse-count block's; all pointers are device pointers; no atomics.
 *
 * gnx_sparse_line_spatial_f64, over ONE array's CSC (lines = genes, idx = the spot's row within the array, n_idx spots): with x
 *   the line as a dense vector of n_idx values (0 where the line has no entry), for every table t < n_tables and row i < n_lines
 *     out[(t * n_lines + i) * 3 + 0] = P = sum over the line's entries (r, v) of v * s_r,  s_r = sum_k x[nbr[t][r][k]]
 *     out[(t * n_lines + i) * 3 + 1] = D = sum deg_r v          deg_r = the number of r's K table entries inside [0, n_idx)
 *     out[(t * n_lines + i) * 3 + 2] = Q = sum deg_r v^2
 *   nbr is [n_tables][n_idx][K] int32.  A table entry outside [0, n_idx) is an absent neighbour (-1 by convention); an entry of
 *   the line whose idx lies outside [0, n_idx) is skipped, as gnx_sparse_expand_f32 skips positions: nothing outside the
 *   buffers described here is ever read or written.  A negative line is an empty line: three zeros.
 * Summation order: one workgroup of 256 threads per (line, table).  The line is expanded into n_idx floats of LDS; thread j
 *   takes the entries j, j + 256, ... of the line in that order; per entry s_r is added in double from 0.0 over k = 0 .. K - 1
 *   (present neighbours only), then p = fma(v, s_r, p), d += deg v, q += (deg v) v in double (deg v and (deg v) v are exact);
 *   the 64 lanes of a wavefront go through the fixed shuffle tree, the four wavefronts' sums are added in wavefront order from
 *   the first.  A function of the line and the table alone - not of how a launch spreads lines and tables over its grid (at most
 *   2048 workgroups in x, row i walked by workgroup i mod gridDim.x, the tables dealt over gridDim.y): equal inputs give equal
 *   bits.  Every element of out is written exactly once per call; nothing is cleared in front of the launch.
 * gnx_sparse_spatial_max_idx() = 32768: the cap on n_idx (128 KB of the CU's 160 KB of LDS).
 * GNX_ERR_BAD_ARG, nothing launched, out untouched: n_lines < 0, a NULL lineptr, nbr or out, K outside 1 .. 32, n_tables < 1,
 *   n_idx < 1, an out that is not 8-byte or an nbr that is not 4-byte aligned, with n_lines > 0 a NULL idx or val.
 *   GNX_ERR_UNSUPPORTED: more than 2^31 - 1 lines, n_idx above the cap, more than 65535 tables.  n_lines == 0: GNX_OK, no launch. */
long gnx_sparse_spatial_max_idx(void);
int gnx_sparse_line_spatial_f64(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                                long n_idx, const int* nbr, long K, long n_tables, double* out, gnx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GRIDNEXT_HIP_H */
