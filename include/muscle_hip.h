/* libmuscle_hip — C ABI of the MI355X (gfx950) kernels behind the MCL / MuSCLe training hot path.
 *
 * The reference (SCoulY/MuSCLe) is pure PyTorch and has no FFI of its own; what each entry point
 * replaces is the ATen/cuDNN op sequence at the cited reference line (paths relative to the
 * reference repository).  The drop-in boundary a user sees is the Python surface in muscle_amd/
 * (same class and function names as src/__init__.py:1-6); this header is the boundary *under* it.
 *
 * Conventions
 *   - every activation is NHWC fp32, viewed as a row-major matrix [rows = N*H*W, C]; C % 4 == 0 and
 *     every pointer 16-byte aligned (the kernels use 16-byte accesses);
 *   - weights keep the reference's state_dict layouts (conv [Cout, Cin/groups, k, k], linear [out, in]);
 *   - the caller owns all memory; the library never allocates, never retains a pointer past return;
 *   - calls only enqueue work on `stream` (a hipStream_t passed as void*), never synchronise;
 *   - return 0 on success, a negative value for an argument error detected before launch, a positive
 *     hipError_t otherwise; mx_last_error() returns a thread-local message;
 *   - "+=" outputs accumulate into what the caller hands in (parameter gradients); every element has ONE adder.
 *   - the training step is run-to-run deterministic: no result is joined through floating-point atomics.  Reductions
 *     that span workgroups use one of three schemes: (i) per-channel BatchNorm statistics: producers write one partial
 *     row per workgroup into `part[P][2][C]` (P from the matching mx_*_parts() helper, no zeroing needed) and the finalise
 *     entry points add the P rows in fp64 in a fixed order (two levels above 1024 rows: <= 64 row slices into the caller's
 *     acc[64][2C] scratch, then one thread per channel); (ii) "last arriver finishes": workgroups park partials in the
 *     caller's `ws` scratch and the last one to arrive adds them in index order (mx_pool_sum, mx_se_bn1_pool,
 *     mx_dwconv_fwd's squeeze); (iii) 64-bit fixed-point integer atomics where the terms are bounded (ER loss).
 *   - `ws` scratch (entry points that take `void* ws, long ws_bytes`; size from the matching mx_*_ws() helper, 0 = not
 *     needed): 16-byte aligned; for scheme (ii) its first 64 KB hold arrival counters that must be ZERO on entry and are
 *     zero again when the launch has drained, so one zero-initialised buffer per stream can be reused for every call.
 *   - an operand "mode" selects the prologue applied while the operand is loaded:
 *        0 PLAIN   v = x
 *        1 BNACT   v = swish(scale[c]*x + shift[c]) * (gate ? gate[n,c] : 1)     n = row / rows_per_sample
 *        2 AFFINE  v = scale[c]*x + shift[c]
 */
#ifndef MUSCLE_HIP_H
#define MUSCLE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

int mx_version(void);
int mx_abi_hash(void);        /* hash of this header the library was built against (muscle_amd/_lib.py checks it) */
const char* mx_last_error(void);

/* ---- pointwise (1x1) convolutions on fp32 MFMA: model.py:44,63,77,86 ------------------------------ */

/* C[M,N] = A'[M,K] * W[N,K]^T (+bias[N]) (+residual[M,ldc]) (relu); stats (optional) = partial column
 * (sum, sum^2) rows part[mx_pw_fwd_parts(M,N,K)][2][N] of C. */
int mx_pw_fwd_parts(int M, int N, int K);
int mx_pw_fwd(const float* A, int a_mode, const float* a_scale, const float* a_shift, const float* a_gate,
              int rows_per_sample, const float* W, float* C, int M, int K, int N, int lda, int ldc,
              const float* bias, const float* residual, int relu, float* stats, void* stream);

/* Arithmetic of the forward / data-gradient / weight-gradient GEMMs (process-wide; initial value from MX_GEMM_SPLIT, default 1).
 * 0: exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) for every GEMM.
 * 1: (default) "split" arithmetic for the MFMA-bound shapes: each fp32 operand is split exactly into three bf16 terms
 *    (x = h + m + l), six of the nine cross products (each exact in fp32) are accumulated in fp32 on the bf16 matrix pipe; the
 *    dropped terms are <= 3 * 2^-24 of a product - one fp32 rounding.  Operands, accumulation and results are fp32; the error
 *    against fp64 equals the fp32-MFMA kernels'; 2.67x the matrix rate.  The other shapes stay on exact-fp32 MFMA.
 * 2: split arithmetic for every NT GEMM (tests). */
int mx_set_gemm_mode(int mode);
int mx_get_gemm_mode(void);
/* Which kernel takes the split-arithmetic weight gradients with plain operands (backward of model.py:77,86), and an optional fixed
 * number of row groups for them (process-wide; for tests and measurement).  kernel: 0 = wgrad_split_kernel (rounds 3-4), 2 = (default)
 * the wave-specialised persistent kernel of round 5, -1 = leave as is; 1 (the single-stream pipelined kernel, removed) and every
 * other value are MX_EARG and change nothing.  groups: > 0 fixes the row groups of every such launch, 0 = back to the planner's
 * choice, -1 = leave as is.  Same groups of at most 1568 rows each => the two kernels give the same bits: same tiles, same MFMA order
 * per group, same fixed-order sum of the groups.  (A longer group is one accumulation chain in kernel 0, while kernel 2 flushes its
 * accumulators every 1568 rows: the sums then differ in the last bits.) */
int mx_set_wgrad_kernel(int kernel, int groups);
int mx_get_wgrad_kernel(void);
/* 1 if, in the current mode, this GEMM runs in split arithmetic on the bf16 pipe (kind 0: mx_pw_fwd / data gradient
 * C[M,N] = A[M,K] W[N,K]^T; kind 1: weight gradient dW[M=Co,N=Ci] over K=R rows), else 0 - for measurement code. */
int mx_gemm_uses_split(int kind, int M, int N, int K);
/* Which kernel a forward / data-gradient GEMM C[M,N] = A'[M,K] W[N,K]^T would launch in the current mode (tests and measurement;
 * launches nothing, touches no device).  entry 0: the route of mx_pw_fwd and mx_bgemm layout 0 (a_mode 0..2; 3 is MX_EARG there);
 * entry 1: the planes route, mx_pw_fwd_planes (a_mode 0), mx_pw_fwd_planes_act (a_mode 1), mx_pw_dgrad_bnbwd_planes (a_mode 3).
 * Answer = family * 10000 + tile width * 10 + grid form.  family: 1 gemm_nt_kernel (exact fp32), 2 gemm_nt_split_kernel (first
 * split generation), 3 gemm_nt_split3_kernel (weight planes).  Tile width: the columns of the 128-row tile.  Grid form: 0 = 3-D
 * grid, 1 = 1-D XCD-ordered ids, 2 = XCD-ordered in chunks of N tiles.  MX_EARG for extents the entry point would refuse.  The
 * launchers run the same planning functions, so the answer is the launch. */
int mx_pw_fwd_plan(int entry, int a_mode, int M, int K, int N, int batch);

/* Second-generation split kernel (round 4): the weight of a 1x1 convolution (model.py:44,63: `_expand_conv`, `_project_conv`) is
 * split ONCE per optimizer step into three bf16 planes laid out as the kernel's LDS image (bytes: mx_pw_planes_bytes; K % 32 == 0,
 * else MX_EARG = no image for this shape), and mx_pw_fwd_planes runs C[M,N] = A[M,K] * W[N,K]^T (+bias) (+residual) (relu)
 * (+stats as mx_pw_fwd) on a PLAIN fp32 A against that image - same split arithmetic as mode 1 of mx_set_gemm_mode.
 * mx_pw_planes_batch: n matrices in one launch; table = DEVICE array of n rows of 5 longs {src W[N][K] fp32, dst image, N, K,
 * first_tile}, first_tile = running sum of mx_pw_planes_tiles, total_tiles = the full sum.
 * mx_pw_fwd_uses_planes: 1 if, in the current mode, a GEMM of this shape should take mx_pw_fwd_planes (else call mx_pw_fwd). */
long mx_pw_planes_bytes(int N, int K);
int mx_pw_planes_tiles(int N, int K);
int mx_pw_planes_batch(const long* table, int n, int total_tiles, void* stream);
int mx_pw_fwd_uses_planes(int M, int K, int N);
int mx_pw_fwd_planes(const float* A, const void* Wplanes, float* C, int M, int K, int N, int lda, int ldc,
                     const float* bias, const float* residual, int relu, float* stats, void* stream);

/* dst[cols,rows] = src[rows,cols]^T (conv weights): the data gradient runs as mx_pw_fwd against the transposed weight. */
int mx_transpose(const float* src, float* dst, int rows, int cols, void* stream);
/* n such transposes in one launch (every 1x1 conv weight of the network, once per step).  table: DEVICE array of n rows of 5 longs
 * {src, dst, rows, cols, first_tile}; first_tile = running sum of ceil(rows/32)*ceil(cols/32), total_tiles = the full sum */
int mx_transpose_batch(const long* table, int n, int total_tiles, void* stream);

/* dX[M,N] = G[M,K] * W[K,N] (+residual): data gradient of the 1x1 conv with weight W[K=Cout, N=Cin]. */
int mx_pw_dgrad(const float* G, const float* W, float* dX, int M, int K, int N, int ldg, int ldx,
                const float* residual, void* stream);

/* The project convolution's forward GEMM (model.py:83-86) with its operand prologue in the second-generation split kernel:
 * C[M,N] = (swish(scale[k]*A[m,k] + shift[k]) * gate[m / rows_per_sample, k]) * W[N,K]^T, W given as its pre-split image; statistics as
 * mx_pw_fwd.  K % 32 == 0.  mx_pw_fwd_act_uses_planes: 1 where the engine should take it (narrow outputs of the HBM-bound stages). */
int mx_pw_fwd_act_uses_planes(int M, int K, int N);
int mx_pw_fwd_planes_act(const float* A, const float* scale, const float* shift, const float* gate, int rows_per_sample,
                         const void* Wplanes, float* C, int M, int K, int N, int lda, int ldc, float* stats, void* stream);

/* The BatchNorm-0 backward apply dZ = c1*G + c2*X + c3 (model.py:45 backward; coef = [3][K] as mx_bn_bwd_finalize leaves it) folded into
 * BOTH consumers of dZ, so that dZ is never written, where both are HBM-bound (stages 1-2):
 *   mx_pw_dgrad_bnbwd_planes: dX[M,N] = dZ[M,K] * Wt[N,K]^T (+residual), Wt given as its pre-split image (mx_pw_planes_batch);
 *   mx_pw_wgrad_small_bnbwd:  dW[Co,Ci] += dZ[R,Co]^T X[R,Ci] (G, G2 = the BatchNorm input, [R, ldg]) in the small-output weight-gradient
 *                             kernel (192 x 32, 288 x 48); scratch = mx_pw_wgrad_small_ws(R,Co,Ci,0); shapes: mx_pw_wgrad_small_bnbwd_ok.
 * (The same fold into the first-generation data-gradient GEMM and into the tiled split weight gradient was measured slower and removed.) */
int mx_pw_dgrad_bnbwd_planes(const float* G, const float* X, const float* coef, const void* WtPlanes, float* dX, int M, int K, int N,
                             int ldg, int ldx, const float* residual, void* stream);
int mx_pw_wgrad_small_bnbwd_ok(int R, int Co, int Ci);
int mx_pw_wgrad_small_bnbwd(const float* G, const float* G2, const float* coef, const float* X, float* dW, int R, int Co, int Ci,
                            int ldg, int ldx, void* ws, long ws_bytes, void* stream);

/* dW[Co,Ci] += G[R,Co]^T * X'[R,Ci]: weight gradient, general kernel (the shapes the two below do not take).  The R pixel
 * rows are split into slices; with more than one slice each adds into its own partial matrix in `ws` (mx_pw_wgrad_ws bytes)
 * and the partial matrices are added to dW in slice order. */
long mx_pw_wgrad_ws(int R, int Co, int Ci);
int mx_pw_wgrad(const float* G, const float* X, int x_mode, const float* x_scale, const float* x_shift,
                const float* x_gate, int rows_per_sample, float* dW, int R, int Co, int Ci, int ldg, int ldx,
                void* ws, long ws_bytes, void* stream);

/* The same weight gradient for SMALL outputs and long reductions (Co*Ci <= 40960, R >= 65536: the first four stages): one
 * workgroup owns the whole output over a contiguous range of rows, partial matrices are added in a fixed order -
 * deterministic, both operands read once.  mx_pw_wgrad_small_ws: bytes of scratch needed, 0 = shape not taken. */
long mx_pw_wgrad_small_ws(int R, int Co, int Ci, int x_mode);
int mx_pw_wgrad_small(const float* G, const float* X, int x_mode, const float* x_scale, const float* x_shift,
                      const float* x_gate, int rows_per_sample, float* dW, int R, int Co, int Ci, int ldg, int ldx,
                      void* ws, long ws_bytes, void* stream);

/* The whole backward of the expand convolution (backward of model.py:77) where BOTH of its halves are HBM-bound - (Co, Ci) = (288, 48)
 * and (192, 32) only: the small-output kernel above also multiplies every 16-row slab of dZ it holds into W[Co,Ci] (the parameter itself,
 * row-major) and writes dX[R,Ci] = dZ W (+ residual), so G (and G2) cross the fabric once for both gradients and dZ is never written.
 * dZ = c1*G + c2*G2 + c3 (coef = [3][Co]) or G itself (G2 = coef = null); exact fp32 MFMA in every GEMM mode.  dX and residual share
 * lddx.  Scratch: [groups][Co*Ci] floats, never more than mx_pw_wgrad_small_ws(R,Co,Ci,0) where that is not 0; dW = null leaves the
 * partial matrices there for mx_pw_parts_reduce (same kernel, same order: dW += their sum).  _ok: 1 where the engine takes it (one of
 * the two shapes, R >= 65536); the entry point itself runs any R >= 1 and answers MX_EARG for every other shape before any launch. */
int mx_pw_bwd_small_fused_ok(int R, int Co, int Ci);
int mx_pw_bwd_small_fused_groups(int R, int Co, int Ci);
int mx_pw_bwd_small_fused(const float* G, const float* G2, const float* coef, const float* X, const float* W, float* dW, float* dX,
                          const float* residual, int R, int Co, int Ci, int ldg, int ldx, int lddx, void* ws, long ws_bytes, void* stream);
int mx_pw_parts_reduce(const float* part, int groups, int n, float* dW, void* stream);

/* The whole backward of the project convolution (backward of model.py:87 and of the SE / BN1 pair in front of it) where its GEMMs are
 * HBM-bound - (Cout, Cexp) = (48, 288) and (48, 192) only: the small-output kernel's pass over dp [R, Cout] and d_raw [R, Cexp] leaves
 * dW[Cout,Cexp] += dp^T X' with X' = swish(scale*d_raw + shift)*gate[sample] (bit for bit mx_pw_wgrad_small with MX_BNACT where both cut
 * the rows into the same groups: below 131 072 rows), dA[R,Cexp] = dp Wp (Wp the parameter itself, row-major; exact fp32 MFMA in every
 * GEMM mode) and out5[5][N][Cexp], the sums of mx_se_bn1_pool over (dA, d_raw), formed from dA while it is on chip.  Deterministic: no
 * atomics.  rows_per_sample must be a MULTIPLE OF 16 (other values are not handled) that divides R, with at most 65 535 samples.  Scratch:
 * [groups][Cout*Cexp] + [groups + N - 1][5][Cexp] floats, N = R / rows_per_sample; dW = null leaves the partial matrices at its head for
 * mx_pw_parts_reduce.  _ok: 1 where the engine takes it (an admitted shape, R >= 65536, rows_per_sample as above); _groups: the row
 * groups, 0 = not taken; the entry point itself runs any R >= 1 and answers MX_EARG for everything else before any launch. */
int mx_pw_proj_bwd_fused_ok(int R, int Cout, int Cexp, int rows_per_sample);
int mx_pw_proj_bwd_fused_groups(int R, int Cout, int Cexp, int rows_per_sample);
int mx_pw_proj_bwd_fused(const float* dp, const float* d_raw, const float* scale, const float* shift, const float* gate, int rows_per_sample,
                         const float* Wp, float* dW, float* dA, float* out5, int R, int Cout, int Cexp, int lddp, int ldraw, int ldda,
                         void* ws, long ws_bytes, void* stream);

/* The same weight gradient for LARGE outputs (Co*Ci >= 16384): dW cut into 128/64-wide tiles, the rows into groups, partial
 * tiles per group added in a fixed order - deterministic, no atomics; workgroup ids are XCD-aware so that a row slab crosses
 * the fabric once.  mx_pw_wgrad_tile_ws: bytes of scratch needed for contiguous operands (ldg = Co, ldx = Ci), 0 = shape not taken.
 * Kernels behind it (same results contract, chosen per shape and arithmetic): split arithmetic, plain operands - one persistent
 * workgroup per CU of 4 MFMA waves + 4 loader waves (wgrad_split_ws_kernel; mx_set_wgrad_kernel selects the earlier forms);
 * exact-fp32 arithmetic (mx_set_gemm_mode(0)), plain operands, 128 x 128 tiles - the same workgroup with loader waves that only move
 * rows by LDS-DMA and v_mfma_f32_32x32x2 MFMA waves (wgrad_f32_ws_kernel); operand prologues and the other tile sizes - the first
 * split kernel / the tiled fp32 kernel.  One fp32 accumulation chain is at most 1568 rows in the wave-specialised forms. */
long mx_pw_wgrad_tile_ws(int R, int Co, int Ci, int x_mode);
int mx_pw_wgrad_tile(const float* G, const float* X, int x_mode, const float* x_scale, const float* x_shift,
                     const float* x_gate, int rows_per_sample, float* dW, int R, int Co, int Ci, int ldg, int ldx,
                     void* ws, long ws_bytes, void* stream);

/* batched plain GEMM for the PCM head (MuSCLe.py:213-223): layout 0: C=A*B^T (B [N,K]); 1: C=A*B (B [K,N]). */
int mx_bgemm(int layout, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
             long sa, long sb, long sc, int batch, int relu, void* stream);

/* ---- BatchNorm2d (train / eval), SiLU, SE gate, drop_connect + skip: model.py:45-94, utils.py:36-91 -- */

/* part[mx_colreduce_parts(rows,C)][2][C] = partial (sum x, sum x^2) per channel */
int mx_colreduce_parts(long rows, int C);
int mx_colstats(const float* X, long rows, int C, float* part, void* stream);

/* training: batch mean / biased var from the P partial rows (summed in fp64), running stats updated with
 * `momentum` (unbiased var); eval: running stats.  Writes scale = gamma*rstd, shift = beta - mean*scale, mean, rstd. */
int mx_bn_finalize(const float* part, int P, int C, double count, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, float momentum, float eps, int training, float* scale, float* shift,
                   float* mean, float* rstd, double* acc /* [64][2C] */, void* stream);

/* Inference constants of one MBConv block, one launch (eval-mode BatchNorm, model.py:72-92 under model.eval()):
 * s = gamma * rsqrt(running_var + eps), t = beta - s * running_mean for each of the block's BatchNorms {g,b,m,v};
 * We_f[Cexp,Cin] = We * s0[:,None], be = t0 (We == NULL: the block has no expand conv); s1, t1 = BN1's affine;
 * Wp_f[Cout,Cexp] = Wp * s2[:,None], bp = t2 */
int mx_fold_block(const float* We, const float* g0, const float* b0, const float* m0, const float* v0, float eps0,
                  const float* g1, const float* b1, const float* m1, const float* v1, float eps1,
                  const float* Wp, const float* g2, const float* b2, const float* m2, const float* v2, float eps2,
                  int Cin, int Cexp, int Cout, float* We_f, float* be, float* s1, float* t1, float* Wp_f, float* bp, void* stream);

/* out = (scale[c]*P + shift[c]) [swish if act] [* gate[n,c]] [* row_scale[n]] [+ residual]
 * (BN2 + drop_connect + skip; with act + gate: the activated, SE-gated project-conv input, model.py:78-84) */
int mx_bn_apply(const float* P, const float* scale, const float* shift, const float* row_scale, const float* residual,
                const float* gate, float* out, long rows, int C, int rows_per_sample, int act, void* stream);

/* effective upstream gradient  g = G [* row_scale[n]] ; [g = g*gate[n,c] + gate_add[n,c]] ;
 * [g *= swish'(act_scale[c]*X + act_shift[c])] ;  part[mx_colreduce_parts(rows,C)][2][C] = partial (sum g, sum g*X) */
int mx_bn_bwd_reduce(const float* G, const float* X, const float* row_scale, const float* gate, const float* gate_add,
                     const float* act_scale, const float* act_shift, long rows, int C, int rows_per_sample,
                     float* part, void* stream);

/* dgamma += rstd*(sum gx - mean*sum g); dbeta += sum g; (c1,c2,c3) so that dX = c1*g + c2*X + c3 */
int mx_bn_bwd_finalize(const float* part, int P, int C, double count, const float* gamma, const float* mean, const float* rstd,
                       int training, float* dgamma, float* dbeta, float* c1, float* c2, float* c3, double* acc,
                       void* stream);

/* out = c1[c]*g + c2[c]*X + c3[c] with g as in mx_bn_bwd_reduce (out may alias G) */
int mx_bn_bwd_apply(const float* G, const float* X, const float* row_scale, const float* gate, const float* gate_add,
                    const float* act_scale, const float* act_shift, const float* c1, const float* c2, const float* c3,
                    float* out, long rows, int C, int rows_per_sample, void* stream);

/* out[n,c] = sum_hw f(X[n,hw,c]),  f = [scale*x+shift] [swish if act] [* G]: SE squeeze (model.py:82),
 * head GAP (MuSCLe.py:240) and the gate-gradient reduction of their backward.  Overwrites `out`; ws: mx_pool_ws(.., 1). */
long mx_pool_ws(long rows, int C, int rows_per_sample, int planes);
int mx_pool_sum(const float* X, const float* G, const float* scale, const float* shift, int act, long rows, int C,
                int rows_per_sample, float* out, void* ws, long ws_bytes, void* stream);

/* SE + BN1 backward reductions in one pass over (dA, X = d_raw): out5[5][N][C] = per-(sample,channel) sums of
 * {dA*act, dA*s', s', dA*s'*X, s'*X} with z = scale*X+shift, act = swish(z), s' = swish'(z); out5[0] is dL/dgate
 * (model.py:84).  Overwrites out5; ws: mx_pool_ws(.., 5). */
int mx_se_bn1_pool(const float* dA, const float* X, const float* scale, const float* shift, long rows, int C, int rows_per_sample,
                   float* out5, void* ws, long ws_bytes, void* stream);
/* From those sums, in one launch and without a second pass over the tensors:
 *   add[n,c] = inv_hw * sum_j gh[n,j] W1[j,c]  (WRITTEN: the gradient reaching d_raw through the squeeze path, model.py:82-83;
 *              gh [N,SQ] from mx_se_bwd, W1 = _se_reduce.weight [SQ,C]),
 *   the BatchNorm-1 backward sums for g = (dA*gate + add)*s' and mx_bn_bwd_finalize on them: dgamma/dbeta += and the
 *   coefficients c1, c2, c3 of dX = c1*g + c2*X + c3. */
int mx_bn1_sums_finalize(const float* pooled5, const float* gate, const float* gh, const float* W1, float inv_hw, float* add,
                         int N, int C, int SQ, double count, const float* gamma, const float* mean, const float* rstd, int training,
                         float* dgamma, float* dbeta, float* c1, float* c2, float* c3, void* stream);

/* ---- depthwise k x k convolution, k in {3,5}, stride in {1,2}: model.py:50-52,78; utils.py:122-145 ---- */

/* Y = dwconv(act(X)), act = swish(scale*x+shift) when scale != NULL; stats (optional, training) = partial (sum Y, sum Y^2)
 * rows part[mx_dwconv_fwd_parts(N,Ho,Wo,S)][2][C]; pooled (optional, inference, excludes stats):
 * pooled[n][c] = sum_hw swish(pool_scale[c]*Y + pool_shift[c]), the SE squeeze of model.py:81-82 under eval-mode BN1
 * (ws: mx_dwconv_fwd_ws bytes, only read when pooled is given) */
int mx_dwconv_fwd_parts(int N, int Ho, int Wo, int C, int S);
long mx_dwconv_fwd_ws(int N, int Ho, int Wo, int C, int S);
int mx_dwconv_fwd(const float* X, const float* scale, const float* shift, const float* W, float* Y, float* stats,
                  const float* pool_scale, const float* pool_shift, float* pooled, void* ws, long ws_bytes, int N,
                  int H, int Wd, int C, int K, int S, int pad_lo, int Ho, int Wo, void* stream);

/* dX = dwconv^T(dY) (+residual): gradient w.r.t. the activated input */
int mx_dwconv_bwd_data(const float* dY, const float* W, const float* residual, float* dX, int N, int H, int Wd, int C,
                       int K, int S, int pad_lo, int Ho, int Wo, void* stream);

/* dW[C,1,K,K] += sum dY * act(X).  dw_scratch: [mx_dwconv_bwd_weight_parts(N,Ho,Wo,C,S)][C*K*K] floats for per-workgroup
 * partial rows (added in a fixed order by a second kernel). */
int mx_dwconv_bwd_weight_parts(int N, int Ho, int Wo, int C, int S);
int mx_dwconv_bwd_weight(const float* X, const float* scale, const float* shift, const float* dY, float* dW, float* dw_scratch,
                         int N, int H, int Wd, int C, int K, int S, int pad_lo, int Ho, int Wo, void* stream);

/* Stride-1 backward of [BN0+SiLU] -> dwconv -> BN1 -> SiLU -> SE gate in one pass: the BatchNorm-1 data gradient
 * dd = c1*g + c2*D + c3 with g = (dA*gate + add)*swish'(a1*D + b1) is formed while staging (never stored);
 * gX = dwconv^T(dd) [* swish'(a0*X+b0) when a0] [+ residual]; dW += sum dd*act(X); when a0 is given,
 * part[mx_dwconv_bwd_fused_parts()][2][C] = BatchNorm-0 backward partial sums (sum g, sum g*X) of the written gX.
 * dw_scratch[mx_dwconv_bwd_fused_parts()][C*K*K] is workspace (per-workgroup dW rows, summed into dW by a second launch; with
 * dW == NULL that launch is left to the caller: mx_dw_parts_reduce(dw_scratch, parts, C*K*K, dW) on any stream ordered behind this call -
 * nothing consumes a depthwise weight gradient before the optimizer, so it need not sit on the backward's critical path). */
int mx_dwconv_bwd_fused_parts(int N, int H, int Wd, int C, int K);
int mx_dwconv_bwd_fused(const float* dA, const float* D, const float* gate, const float* add, const float* a1, const float* b1,
                        const float* c1, const float* c2, const float* c3, const float* X, const float* a0, const float* b0,
                        const float* W, const float* residual, float* gX, float* dW, float* dw_scratch, float* part, int N, int H,
                        int Wd, int C, int K, int pad_lo, void* stream);

/* The same fusion for a stride-2 depthwise convolution with the static TF-"same" padding (pad_lo before; Ho, Wo as the forward made them;
 * K = 3: pad_lo 0 or 1, K = 5: 1 or 2), dA / D [N,Ho,Wo,C], X / gX [N,H,Wd,C].  The depthwise input
 * always sits behind BatchNorm-0 + SiLU (a0, b0 required; a plain-input stride-2 block keeps mx_bn_bwd_apply + mx_dwconv_bwd_weight +
 * mx_dwconv_bwd_data): gX = dwconv^T(dd) * swish'(a0*X+b0); dW += sum dd*swish(a0*X+b0) (dW == NULL: left to mx_dw_parts_reduce);
 * part[mx_dwconv_bwd_fused_s2_parts()][2][C] = (sum g, sum g*X) of the written gX, dw_scratch[parts][C*K*K] workspace.  parts <= 1024. */
int mx_dwconv_bwd_fused_s2_parts(int N, int H, int Wd, int C, int K);
int mx_dwconv_bwd_fused_s2(const float* dA, const float* D, const float* gate, const float* add, const float* a1, const float* b1,
                           const float* c1, const float* c2, const float* c3, const float* X, const float* a0, const float* b0,
                           const float* W, float* gX, float* dW, float* dw_scratch, float* part, int N, int H, int Wd, int C, int K,
                           int pad_lo, int Ho, int Wo, void* stream);

int mx_dw_parts_reduce(const float* part, int P, int n, float* dW, void* stream);

/* ---- SE excitation (model.py:83-84) and stem patches (model.py:131,175) -------------------------------- */

/* s = pooled_sum*inv_hw; h = W1 s + b1; gate = sigmoid(W2 swish(h) + b2) */
int mx_se_fwd(const float* pooled_sum, float inv_hw, const float* W1, const float* b1, const float* W2, const float* b2,
              float* s, float* h, float* gate, int N, int C, int SQ, void* stream);

/* given ggate[n,c] = dL/dgate: gh[n,j] = dL/d(se_reduce output) [N,SQ] (WRITTEN; mx_bn1_sums_finalize turns it into the
 * pooled-path gradient `add`); dW1,db1,dW2,db2 += (each element summed over the samples by one thread, in order) */
int mx_se_bwd(const float* ggate, const float* gate, const float* s, const float* h, const float* W2,
              float* dW1, float* db1, float* dW2, float* db2, float* gh, int N, int C,
              int SQ, void* stream);

/* The two halves of mx_se_bwd as separate launches: gh (consumed by mx_bn1_sums_finalize on the data-gradient chain) and the four
 * parameter gradients (no consumer before the optimizer: the engine queues them beside the weight-gradient GEMMs). */
int mx_se_bwd_gh(const float* ggate, const float* gate, const float* h, const float* W2, float* gh, int N, int C, int SQ,
                 void* stream);
int mx_se_bwd_params(const float* ggate, const float* gate, const float* s, const float* h, const float* gh, float* dW1, float* db1,
                     float* dW2, float* db2, int N, int C, int SQ, void* stream);

/* out[(n,oy,ox), ci*9+ky*3+kx] = img[n,ci,oy*2-pad+ky,ox*2-pad+kx] (NCHW image), rows of 28 floats (27 + 0) */
int mx_stem_im2col(const float* img, float* out, int N, int H, int W, int Ho, int Wo, int pad_lo, void* stream);

/* ---- CAM head + PCM support: MuSCLe.py:213-223,237-279 ---------------------------------------------------- */

/* dst[n,y,x,coff+c] = [relu] bilinear_align_corners(src[n,:,:,c]); NHWC -> channel slice of an NHWC tensor of width ldd */
int mx_resize_nhwc(const float* src, float* dst, int N, int Hs, int Ws, int C, int Hd, int Wd, int ldd, int coff, int relu,
                   void* stream);

/* dst[n,k,Y,X] (NCHW) = bilinear_align_corners(src[n,:,:,k]); src NHWC with leading dimension lds (MuSCLe.py:256-257) */
int mx_upsample_to_nchw(const float* src, float* dst, int N, int Hs, int Ws, int lds, int K, int Hd, int Wd, void* stream);

/* ---- infer_mcl.py post-processing, one forward pass of the multi-scale / flip list:
 * acc[k-1,Y,X] += resize_halfpixel( upsample_align_corners(src[:,:,k], Hs x Ws), H x W )[Y, flip ? W-1-X : X]  for k = 1..K-1
 * (infer_mcl.py:124-148: model upsample, cv2.resize to the original size, np.flip of the odd passes, sum over passes).
 * src: ONE sample, NHWC [h,w,lds], channel 0 = background. */
int mx_infer_accum(const float* src, float* acc, int h, int w, int lds, int K, int Hs, int Ws, int H, int W, int flip, void* stream);
/* in place per channel over [channels][HW] (infer_mcl.py:153-158 / :161-166): v = max(v,0); v[v < min+1e-6] = 0;
 * v = (v - min - 1e-6) / (max - min + 1e-6) */
int mx_infer_norm(float* acc, int channels, long HW, void* stream);

/* ---- infer_mcl.py:107-148 for one image in ONE launch: every pass of the multi-scale / flip list, both maps, only the
 * channels the script keeps (:172-174).  passes: device int64 [npass][8] {address of the pass's CAM [h,w,lds], address of
 * its SGC [h,w,lds] (cam='cam_lr', one sample each), h, w, Hs, Ws, flip, 0} in the order of VOC12ClsDatasetMSF; trusted
 * device data, h*w*lds < 2^31.  keep: device int32 [nkeep], foreground indices 0..K-2 ascending (model channel keep[j]+1).
 * out_cam / out_sgc: fp32 [nkeep,H,W], fully written; either may be NULL (that map is neither read nor computed), both
 * NULL is an error.  out[j,Y,X] = sum over passes in table order, from 0.f, of mx_infer_accum's per-pass value for channel
 * keep[j]+1 (bit-equal to mx_infer_accum over the same passes into a zeroed accumulator).  No atomics.  The normalisation
 * of infer_mcl.py:151-164 is mx_infer_norm(out, nkeep, H*W) on the compact buffer. */
int mx_cam_infer(const long* passes, int npass, int lds, int K, int H, int W, const int* keep, int nkeep, float* out_cam,
                 float* out_sgc, void* stream);

/* ---- semantic-segmentation inference (infer_seg.py:101-133 without the dense CRF; src/evaluation.py:36-68) ------------
 * mx_seg_infer: one image, ALL passes of its multi-scale / flip list in one launch.  passes: device int64 [npass][8]
 * {address of the pass's NHWC logits [h,w,lds] (cam='seg_lr', one sample), h, w, Hs, Ws, flip, 0, 0}, in the order of
 * VOC12ClsDatasetMSF; every pass has row stride lds (a multiple of 4; the rows are read 16 bytes at a time, so each
 * address is 16-byte aligned).  The table is trusted device data.  Per output pixel (Y, X) and pass:
 *   p = softmax_K(upsample_align_corners(logits, Hs x Ws))            (MuSCLe.forward(cam='seg') + torch.softmax, :104-106)
 *   v = resize_halfpixel(p, H x W)[Y, flip ? W-1-X : X]               (cv2.resize + np.flip of the odd passes, :109-112)
 * then mean = sum over passes in table order / npass (:117), mean[1..K-1] *= cls_scale[1..K-1] if cls_scale (:125),
 * pred[Y,X] = argmax_k mean (uint8, first maximum as np.argmax, :133), prob[k,Y,X] = mean (fp32 [K,H,W], NULL = not
 * written).  1 <= K <= min(lds, 24).  No atomics: the same bits every run.
 * mx_seg_confusion: over pixels with gt < 255 (uint8 [H,W] both), counts[k] += (TP, P, T) with P counting pred == k,
 * T gt == k, TP both; counts int64 [K][3], accumulated across calls. */
int mx_seg_infer(const long* passes, int npass, int lds, int K, int H, int W, const float* cls_scale, unsigned char* pred,
                 float* prob, void* stream);
int mx_seg_confusion(const unsigned char* pred, const unsigned char* gt, int K, int H, int W, long long* counts, void* stream);

/* mx_seg_infer_batch: mx_seg_infer for B images of one output size (H, W) in one launch (the per-epoch validation of
 * train_muscle.py:224-283, one pass per image).  rows: device int64 [nrow][8] {address of the row's NHWC logits [h,w,lds],
 * h, w, Hs, Ws, flip, image 0..B-1, 0}; every row belongs to one image and every image has at least one row.  Per image the
 * rows are summed in table order and divided by the image's row count: pred uint8 [B,H,W] and prob fp32 [B,K,H,W] (NULL =
 * not written) hold, per image, the bits mx_seg_infer produces over that image's rows; cls_scale fp32 [B,K] or NULL.
 * gt uint8 [B,H,W] with counts int64 [K][3] (both or neither): mx_seg_confusion's (TP, P, T) of src/evaluation.py:36-50
 * over all B images, accumulated across calls with integer atomics (exact). */
int mx_seg_infer_batch(const long* rows, int nrow, int B, int lds, int K, int H, int W, const float* cls_scale, unsigned char* pred,
                       float* prob, const unsigned char* gt, long long* counts, void* stream);

/* ---- input stage (src/data.py:215-332, src/imutils.py:143-181,376-388) ------------------------------
 * mx_input_stage: dst[n,3,Hd,Wd] (fp32, fully written) = color_norm + crop container + flip + RandomErasing + CHW of n
 * uint8 HWC sources inside src (RandomCrop src/imutils.py:143-181, RandomCropWithMask :110-112, the flip of :288-289).
 * jobs: n x 12 int32 {src_off, row_stride, col_step, top, left, h, w, ey | ex<<16, eh | ew<<16, 0, 0, 0}, on the device.
 *   inside the window top <= y < top+h, left <= x < left+w (output coordinates):
 *     dst[c, y, x] = norm(src[src_off + ((y-top) * row_stride + (x-left) * col_step) * 3 + c]);  0 outside it;
 *   then 0 inside the box ey <= y < ey+eh, ex <= x < ex+ew (RandomErasing(value=0) of train_mcl.py:114; 0 = none).
 * src_off is the byte offset of the pixel that lands on (top, left), row_stride is in pixels, col_step is +1 or -1: a
 * crop [ch,cw] at (ct,cl) of a container that is then flipped is the window left = Wd-cl-cw with src_off at the crop's
 * last column and col_step -1.  The jobs are trusted device data (as the tables of mx_irn_input_stage are).
 * norm = (float)(((double)u8 / 255 - mean[c]) / std[c]): bit-exact with the numpy expressions. */
int mx_input_stage(const unsigned char* src, const int* jobs, float* dst, int n, int Hd, int Wd, void* stream);

/* transforms.ColorJitter (train_mcl.py:108, src/data.py:223; torchvision 0.9.0 PIL backend = Pillow's ImagingBlend, rgb2l,
 * rgb2hsv_row / hsv2rgb) in place on n uint8 HWC images inside src, bit-exact with Pillow.  jobs: n x 8 words {byte
 * offset, h, w, order (one nibble per position: 0 brightness, 1 contrast, 2 saturation, 3 hue, 15 none), brightness,
 * contrast, saturation factors (float32), hue shift 0..255}; sums: n uint64 of scratch. */
int mx_color_jitter(unsigned char* src, const int* jobs, unsigned long long* sums, int n, int max_pixels, void* stream);

/* PIL.Image.resize (imutils.RandomResizeLong's bicubic, src/imutils.py:127-141; get_views' bilinear 448x448,
 * src/data.py:274-276) = Pillow's 8-bit ImagingResample: horizontal pass src -> tmp, vertical pass tmp -> dst, 22-bit
 * fixed-point coefficient tables computed by the host as Pillow's precompute_coeffs does.  jobs: n x 8 int32 {src_off, Hin,
 * Win, tmp_off, dst_off, Wout, Hout, tab_off}; tabs (int32): per job ksize_h, ksize_v, bounds_h[Wout][2], kk_h[Wout][ksize_h],
 * bounds_v[Hout][2], kk_v[Hout][ksize_v].  Bit-exact with Pillow. */
int mx_resample(const unsigned char* src, const int* jobs, const int* tabs, unsigned char* tmp, unsigned char* dst, int n,
                int max_pixels, void* stream);

/* ---- input stage of decoder training (VOC12SegDataset.__getitem__, src/data.py:93-123) ----------------------------------
 * mx_mask_stage: dst[n,C,S,S] (fp32, fully written) = the soft pseudo-label of item n after RandomResizeLongWithMask's
 * skimage.transform.resize (src/imutils.py:52: Gaussian anti-alias filter + bilinear warp, 'mirror' boundary),
 * RandomCropWithMask's zero container (src/imutils.py:114-116), RandomHorizontalFlipWithMask (src/imutils.py:288-290) and
 * HWC_to_CHW (src/data.py:122).  The resize is evaluated only inside the crop window, from one weight row per output row
 * and column that the host folds from both operators (muscle_amd/segdata.py:mask_axis_table).
 * src: the shipped source rows of every item, channel-last [sh,sw,C], float16 (what infer_irn --soft_output 1 writes) or
 * float32; jobs: n x 16 int32 {byte offset into src, sh, sw, 1 = float32 source, top, left, ch, cw (the window inside the
 * container), flip, ky, kx (taps per row / column), ty_off, tx_off (int32 words into tabs), 0, 0, 0}; tabs at t*_off:
 * start[ch | cw] (first source row / column, relative to the shipped rows) then [ch | cw][k] float32 weights.
 * span_cap >= the longest run of source columns 64 neighbouring window columns read (start[x+63] + kx - start[x]); it
 * sizes the LDS tile.  fp32 accumulation in a fixed order, no atomics.  The image of the same item goes through
 * mx_input_stage. */
int mx_mask_stage(const void* src, const int* jobs, const int* tabs, float* dst, int n, int C, int S, int span_cap, void* stream);

/* mx_label_stage: the same item when its label is a hard label map (mask_type="label": one class index per pixel, 255 =
 * ignore; ours, the reference's unused 'hard' branch pads with class 0 and has no ignore index).  dst[n,S,S] (uint8, fully
 * written) = the label of item n after a NEAREST resize (what PIL.Image.resize(.., NEAREST) returns), the crop window
 * pasted into a container filled with `fill` (255: padding is ignored by mx_ce_label, not trained as background) and
 * np.fliplr of the container:
 *   window top <= y < top+ch, left <= x < left+cw of the container:  c[y, x] = src[ys[y-top]][xs[x-left]];  fill elsewhere;
 *   dst[n, y, x] = flip ? c[y, S-1-x] : c[y, x].
 * src: the shipped uint8 source rows [sh,sw] of every item at BYTE offsets of any alignment (sw is usually odd: the kernel
 * loads single bytes and assumes no alignment); jobs: n x 16 int32 {byte offset into src, sh, sw, top, left, ch, cw, flip,
 * ty_off, tx_off (int32 words into tabs), 0 x 6}; tabs at ty_off: ys[ch], at tx_off: xs[cw], the int32 source row / column of
 * every window row / column relative to the shipped rows (muscle_amd/segdata.py:nearest_axis_table), clamped to the shipped
 * rows by the kernel.  0 <= fill <= 255.  One launch per batch, every output byte has one writer, no atomics. */
int mx_label_stage(const unsigned char* src, const int* jobs, const int* tabs, unsigned char* dst, int n, int S, int fill,
                   void* stream);

/* ---- input stage of IRN training (VOC12AffinityDataset.__getitem__, src/data.py:659-705) ---------------------------------
 * mx_irn_input_stage: one launch writes both outputs of a batch of n items, S = crop size (S % 16 == 0):
 *   img[n,3,S,S] (fp32, fully written) = TorchvisionNormalize (src/data.py:596-609: fp64 (u8 / 255 - mean) / std, one
 *     rounding to fp32) of the rescaled uint8 HWC image [sh,sw,3] at src + img_off, random_lr_flip applied BEFORE the
 *     crop (the rescaled image is mirrored, not the container), random_crop's container with fill 0, CHW:
 *       img[c, cont_top + y, cont_left + x] = norm(I[img_top + y, flip ? sw-1-(img_left + x) : img_left + x, c]),
 *       0 <= y < ch, 0 <= x < cw; 0 elsewhere.
 *   label[n,S/4,S/4] (uint8, fully written; NULL = the eval view, nothing written) = the ORIGINAL label [lh,lw] at
 *     src + lab_off through pil_rescale(NEAREST) to [sh,sw], the same flip, the container with fill 255 and
 *     pil_rescale(., 0.25, NEAREST) - which reads container pixel (4Y+2, 4X+2) - as one gather:
 *       (y, x) = (4Y+2 - cont_top, 4X+2 - cont_left); inside the window:
 *       label[Y, X] = L[ytab[img_top + y], xtab[flip ? sw-1-(img_left + x) : img_left + x]]; 255 elsewhere.
 *     ytab[sh] / xtab[sw] (int32, at tabs + ytab_off / xtab_off words) are Pillow's NEAREST source indices per axis
 *     (muscle_amd/irndata.py:nearest_table); indices are clamped to the label.  lab_off < 0: no label, all 255.
 * src: one device buffer holding every image and label; jobs: n x 16 int32 {img_off, sh, sw, img_top, img_left, cont_top,
 * cont_left, ch, cw, flip, lab_off, lh, lw, ytab_off, xtab_off, 0}, byte offsets into src; the tables are trusted device
 * data.  Bit-exact with the numpy / PIL expressions.  No atomics; the call only enqueues on the stream. */
int mx_irn_input_stage(const unsigned char* src, const int* jobs, const int* tabs, float* img, unsigned char* label, int n, int S,
                       void* stream);

/* ---- IRN random-walk propagation (src/indexing.py:77-142 as called by infer_irn.py:76).
 * mx_irn_affinity: dense[n4][ld] (zero-filled here) <- symmetric affinity 1 - max(edge along the straight path) for every
 *   pixel pair joined by one of the nd search directions, unit diagonal; edge [h,w]; pcoord = int32 (dy,dx) pairs of all
 *   paths back to back (farthest pixel first = the destination), poff[d] / plen[d] = first pair and length of path d.
 * mx_irn_transition: dense <- dense^beta / column sums (to_transition_matrix :116-118); colsum[n4] is workspace.
 * The matrix powers and the final product are mx_bgemm calls. */
int mx_irn_affinity(const float* edge, int h, int w, int radius, const int* pcoord, const int* poff, const int* plen, int nd,
                    float* dense, int ld, int n4, void* stream);
int mx_irn_transition(float* dense, int n4, int ld, float beta, float* colsum, void* stream);
/* infer_irn.py:78-94 after the walk: rw [C,h,w] -> 4x bilinear (half-pixel) upsample, top-left HxW crop, / global max,
 * label[H,W] (uint8) = argmax over [bg_thres, maps] (first maximum wins); soft_half (optional, fp16 [H,W,C+1]) = the
 * values themselves as the script's --soft_output writes them.  max_scratch: one uint32. */
int mx_irn_finish(const float* rw, int C, int h, int w, int H, int W, float bg_thres, unsigned* max_scratch, unsigned char* label,
                  void* soft_half, void* stream);
/* The compact soft pseudo-label (muscle_amd/softlabel.py) back to rows of the dense array: what infer_irn.py:79-88 saves
 * (np.concatenate([bg_thres plane, rw_up / max]).astype(float16), HWC) and src/data.py:102 np.load's, re-created from the
 * stored walk maps with the arithmetic of mx_irn_finish (csrc/irn_soft.h is included by both kernels), bit for bit.
 * Batched: jobs = n x 16 int32 {rw_off, keys_off, K, h, w, H, W, r0, rows, dst_off, channels, vmax, bg, 0, 0, 0}; *_off are
 * byte offsets from base: rw fp32 [K,h,w] (4-byte aligned), keys uint8 [K] ascending (the map i is channel keys[i] + 1 of
 * the label), dst 16-byte aligned; vmax / bg are float bits: the maximum mx_irn_finish divided by and the threshold.
 * Every item's float16 [rows, W, channels] at dst_off is fully written: rows r0 .. r0 + rows - 1 of the [H,W,channels]
 * label - channel 0 half(bg), channel keys[i] + 1 half(up4(rw_i, r0 + y, x) / vmax), every other channel +0.
 * H <= 4h, W <= 4w, r0 + rows <= H, channels <= 256.  The job table is trusted device data.  No atomics. */
int mx_soft_expand(void* base, const int* jobs, int n, void* stream);

/* ---- class-balanced self-training labels (csrc/selflabel.hip; muscle_amd/selflabel.py; CBST, Zou et al., ECCV 2018)
 * The confidence code.  Per pixel of prob fp32 [K,H,W] (the mean map of mx_seg_infer, or the CRF's Q):
 *   label (uint8): best = prob[0], label = 0; for c = 1..K-1: if (prob[c] > best) { best = prob[c]; label = c; } - the first
 *     maximum, as np.argmax on finite data;   conf = best;
 *   code (uint8): a logarithmic code of the uncertainty u = 1.0f - conf, ONE fp32 subtraction:
 *     conf is NaN -> 255 (never selected);   u <= 0 (conf >= 1) -> 0;   otherwise clamp((bits(u) >> 20) - 823, 1, 193),
 *     bits(u) >> 20 = the sign, the 8 exponent bits and the top 3 mantissa bits.  So u = 2^-24 (the smallest uncertainty a
 *     conf < 1 can give) is code 1, u in [0.5, 1) is 185..192 and u >= 1 is 193; a lower code means more confident, with
 *     12.5 % relative resolution in 1 - conf at every magnitude; codes 194..254 are unused.
 * mx_conf_code: label and code uint8 [H,W], fully written; hist int64 [K][256]: hist[label][code]++ for every pixel; with
 *   gt (uint8 [H,W], 255 = ignore; gt, val and hit come together or all NULL) also val[label][code]++ where gt != 255 and
 *   hit[label][code]++ where gt == label (int64 [K][256] both).  The tables are ADDED to (accumulated across calls):
 *   counted per workgroup in LDS, flushed with 64-bit integer atomics; no floating-point atomics, the same integers
 *   every run.  1 <= K <= 24, H*W < 2^31.  prob is read once.
 * mx_code_hist: the same three tables from a stored (label, code) pair of n pixels (the same counting function); a
 *   label >= K is counted nowhere and never used as an index; a stored code in 194..254 is counted as 255.
 * mx_conf_select: out[i] = (label[i] < K && code[i] <= tcode[label[i]]) ? label[i] : 255; tcode uint8 [K] on the device;
 *   kept int64 [K][2] += (kept, total) per class.  1 <= n < 2^31.
 * All three only enqueue on `stream` and return a negative code for bad arguments before any launch. */
int mx_conf_code(const float* prob, int K, int H, int W, unsigned char* label, unsigned char* code, const unsigned char* gt,
                 long long* hist, long long* val, long long* hit, void* stream);
int mx_code_hist(const unsigned char* label, const unsigned char* code, const unsigned char* gt, long n, int K, long long* hist,
                 long long* val, long long* hit, void* stream);
int mx_conf_select(const unsigned char* label, const unsigned char* code, const unsigned char* tcode, long n, int K,
                   unsigned char* out, long long* kept, void* stream);
/* The same walk without the matrix (csrc/irn_walk.hip): x . T^steps as `steps` stencil applications, O(nd * n) memory.
 * mx_irn_walk_weights (indexing.py:77-93 + :116-118; same path table as mx_irn_affinity, n = h*w):
 *   W[nd][n] fp32, direction-major: W[d][p] = (1 - max of the edge along the straight path p -> p+d)^beta, 0 where p+d lies
 *   outside the image (what the padding with 1.0 of :124 and the crop of :131-133 amount to); the power as mx_irn_transition
 *   forms it, so the non-zero weights are that path's dense^beta entries bit for bit.
 *   cs[n] fp64 = 1 + sum_d (W[d][j] + W[d][j-d]), the column sums of dense^beta, gathered in a fixed order.
 * mx_irn_walk (indexing.py:119-120 + :145-147): state 0 = (double)(x * (1 - edge)) with the product in fp32, then `steps` times
 *   v'[c][j] = (v[c][j] + sum_d (v[c][j+d] W[d][j] + v[c][j-d] W[d][j-d])) / cs[j], fp64 sums in one fixed order per pixel,
 *   taps outside the image skipped; the last step writes rw[C][n] rounded to fp32.  x [C][n] fp32; state_a, state_b: two
 *   distinct fp64 [C][n] buffers of mx_irn_walk_ws(C, n) bytes EACH, contents need not survive between calls.  All `steps`
 *   launches are enqueued by the one call.  1 <= steps <= 4096, radius >= 1. */
int mx_irn_walk_weights(const float* edge, int h, int w, int radius, const int* pcoord, const int* poff, const int* plen, int nd,
                        float beta, float* W, double* cs, void* stream);
long mx_irn_walk_ws(int C, int n);                                       /* < 0: bad arguments */
int mx_irn_walk(const float* x, const float* edge, const float* W, const double* cs, int h, int w, int radius, const int* pcoord,
                const int* poff, const int* plen, int nd, int C, int steps, double* state_a, double* state_b, float* rw, void* stream);
/* mx_irn_walk that also hands out the states it passes through (src/indexing.py:116-147 for several exp_times at the cost of
 * the largest): snap[ns] int32 in HOST memory (read before return), 1 <= snap[0], strictly ascending, snap[ns-1] <= 4096,
 * ns <= 13; snap[ns-1] steps are run and at step snap[i] the fp64 state is written together with its fp32 rounding,
 * rw[i][C][n].  Snapshot i equals mx_irn_walk(..., steps = snap[i]) bit for bit: the same per-pixel arithmetic (one device
 * function), the fp64 quotient rounded once.  Everything else as mx_irn_walk. */
int mx_irn_walk_snap(const float* x, const float* edge, const float* W, const double* cs, int h, int w, int radius, const int* pcoord,
                     const int* poff, const int* plen, int nd, int C, const int* snap, int ns, double* state_a, double* state_b,
                     float* rw, void* stream);
/* The label step of infer_irn.py:76-92 for E walk results and ALL thresholds at once, counted as src/evaluation.py:36-50
 * (input_type='png') counts: counts[e][t][k][0..2] += the (TP, P, T) mx_seg_confusion gives for the label map that
 * mx_irn_finish(rw[e], ..., bg_thres = thresholds[t]) writes, integer for integer; no label map is written.
 * rw fp32 [E][Kp][h][w]: the maps of the Kp channels present, channel keys[j] + 1 of the label (every other channel is exactly
 * 0 and never beats a threshold >= 0); keys int32 [Kp] ascending in 0..K-2; Kp = 0 (rw, keys may be NULL): background
 * everywhere.  gt uint8 [H,W] (255 = ignore, K..254 count towards P only, as mx_seg_confusion); thresholds fp32 [nt] ascending
 * and >= 0, nt <= 64; 2 <= K <= 24; E <= 13; H <= 4h, W <= 4w.  vmax uint32 [E]: the bits of the maximum each rw[e] is divided
 * by - the max_scratch word of mx_irn_up_max / mx_irn_finish run on the full [K-1][h][w] stack (the largest irn_up4 value
 * of csrc/irn_soft.h, taken from that kernel, not recomputed), or a stored CompactSoft vmax; 0 gives NaN values:
 * background at every threshold.  A tie value == threshold is background.  One launch, snapshot = blockIdx.y; per pixel at
 * most three LDS integer atomics whatever nt (the bin #{t < best value}, as mx_camdict_confusion); no floating-point atomics. */
int mx_irn_sweep_confusion(const float* rw, int E, int Kp, const int* keys, int h, int w, const unsigned char* gt, int H, int W,
                           const float* thresholds, int nt, int K, const unsigned* vmax, long long* counts, void* stream);

/* ---- per-epoch rapid evaluation (train_mcl.py:286-318 + src/evaluation.py:19-52), one image:
 * for each threshold t: predict = argmax_k [t, half(pred_k*label_k)] (first maximum wins); over pixels with gt < 255:
 * counts[t][k][0..2] += (TP, P, T).  pred [K,H,W] fp32 (cam_maxnorm'ed), label [K], gt uint8 [H,W], counts int64 [nt][K][3]. */
int mx_eval_confusion(const float* pred, const float* label, const unsigned char* gt, const float* thresholds, int nt, int K, int H,
                      int W, long long* counts, void* stream);

/* ---- the same evaluation for B images of one size from the model's LOW-RESOLUTION SGC maps (train_mcl.py:297-303 +
 * src/evaluation.py:19-52): sgc NHWC [B,h,w,lds] (cam='cam_lr'), label_with_bg [B,K] (entry 0 unused), gt uint8 [B,H,W],
 * thresholds [nt], counts int64 [nt][K][3] accumulated across calls.  Per image and channel the kernel takes the extremes of
 * relu(mx_upsample_to_nchw's value) over the H x W grid, then per pixel recomputes that value, applies cam_maxnorm
 * (train_mcl.py:21-28, mx_maxnorm's expression) and counts as mx_eval_confusion does: the table is the one the chain
 * mx_upsample_to_nchw -> mx_maxnorm -> mx_eval_confusion gives per image, integer for integer, and no [K,H,W] tensor is
 * read or written.  K <= min(lds, 24), lds a multiple of 4, nt <= 64.  ws: mx_rapid_eval_lr_ws(B, K) bytes of scratch (the
 * [B][K][2] extremes; zeroed by the call). */
long mx_rapid_eval_lr_ws(int B, int K);
int mx_rapid_eval_lr(const float* sgc, const float* label_with_bg, const unsigned char* gt, const float* thresholds, int nt, int B,
                     int h, int w, int lds, int K, int H, int W, long long* counts, void* ws, long ws_bytes, void* stream);

/* ---- CAM quality evaluation (src/evaluation.py:25-50, input_type='npy'), one image, ALL thresholds of the curve (:126-133):
 * predict(t) = argmax_k [t, tensor_1..tensor_{K-1}] with tensor_{keys[j]+1} = maps[j] and absent channels 0 (first maximum
 * wins; no fp16 rounding, no label multiply); over pixels with gt < 255: counts[t][k][0..2] += (TP, P, T).
 * maps fp32 [nkeep,H,W]; keys int32 [nkeep] ascending in 0..K-2; gt uint8 [H,W]; thresholds fp32 [nt] ascending and >= 0
 * (so an absent channel never wins); counts int64 [nt][K][3], accumulated across calls with integer atomics (exact).
 * nt <= 64, K <= 24.  Per pixel at most three LDS atomics whatever nt: the pixel is binned by #{t < its best value}. */
int mx_camdict_confusion(const float* maps, const int* keys, int nkeep, const unsigned char* gt, const float* thresholds, int nt,
                         int K, int H, int W, long long* counts, void* stream);

/* adjoint of mx_upsample_to_nchw: gsrc (=|+=) W^T gdst */
int mx_upsample_to_nchw_bwd(const float* gdst, float* gsrc, int N, int Hs, int Ws, int lds, int K, int Hd, int Wd,
                            int accumulate, void* stream);

/* y = x / (||x||_2 + eps) per row, nrm saved (MuSCLe.py:218) and its backward */
int mx_row_l2norm(const float* x, float* y, float* nrm, long R, int C, float eps, void* stream);
int mx_row_l2norm_bwd(const float* x, const float* nrm, const float* gy, float* gx, long R, int C, float eps, void* stream);

/* PCM tail on T = aff * [cam | 1]: fwd rv = T[:, :K] / (T[:, K] + eps) (MuSCLe.py:221-222); bwd gives dL/dT */
int mx_pcm_norm(const float* T, const float* grv, float* out, long rows, int L, int K, float eps, int bwd, void* stream);

/* out[b,i,j] = (gaff[b,i,j] + gaff[b,j,i]) * (aff[b,i,j] > 0): gradient through relu(f^T f) (MuSCLe.py:220);
 * matrices are [b, n, ld] with ld >= n (padding columns -> 0) */
int mx_sym_relu_grad(const float* gaff, const float* aff, float* out, int B, int n, int ld, void* stream);

/* flat elementwise: op 0 out = alpha*a; op 1 out = a + alpha*b; op 2 out = (y > 0) ? a (+ b) : 0 */
int mx_ew(int op, const float* a, const float* b, const float* y, float alpha, float* out, long n, void* stream);

/* X[n,hw,c] += alpha * v[n,c] (backward of the global average pool, MuSCLe.py:240) */
int mx_bcast_add(float* X, const float* v, float alpha, long rows, int C, int rows_per_sample, void* stream);

/* ---- losses of the MCL step and the optimiser ---------------------------------------------------------------- */

/* [N,C] classification losses with d loss / d input for unit upstream gradient:
 * mode 0 focal(p,y) gamma 2 alpha .5 (loss_multilabel.py:68-91) -> loss[0] = ; 1 MultiLabelSoftMargin(x,y)
 * (train_mcl.py:146) -> loss[0] = ; 2 Log_Sum_Exp_Pairwise(p,y) (loss_multilabel.py:24-33) -> loss[n];
 * 3 grad = sigmoid(x); 4 grad = y * x * (1 - x) (sigmoid backward, x = sigmoid output, y = upstream) */
int mx_cls_loss(int mode, const float* x, int ldx, const float* y, int ldy, float* loss, float* grad, int ldg, int N, int C,
                void* stream);

/* image_level_contrast (loss_multilabel.py:36-66): out2 = {loss, #valid anchor rows}; gemb = d loss / d emb;
 * workspace: N*D + 2*N*N + 4*N + 16 floats, 16-byte aligned.  N <= 64, D <= 1024.  The pair matrix exp(e_i . e_j / 0.1) (a dense
 * N x N x D contraction) and the gradient's [N x N] x [N x D] product run on v_mfma_f32_16x16x4_f32 in ceil(N/16) workgroups
 * when D % 16 == 0 (one VALU workgroup otherwise). */
int mx_imc(const float* emb, const float* label, int N, int D, int L, float* out2, float* gemb, float* workspace, void* stream);

/* cam_softmaxnorm (train_mcl.py:30-36) on NCHW [N,K,HW]; bwd != 0: out = d/dx given gy */
int mx_softmaxnorm(const float* x, const float* gy, float* out, int N, int K, long HW, int bwd, void* stream);

/* ER loss (train_mcl.py:185-188): mean over rows of the top-k of |softmaxnorm(cams)-softmaxnorm(sgcs)|*lwb, exact
 * 3-pass radix select.  d [N*K*HW] scratch; krem/prefix/sum_gt/cnt_eq [N] and hcnt/hsum [N*2048] state
 * (prefix and sum_gt zeroed by the caller) are kept for mx_er_bwd.  sum_gt and hsum are 64-bit fixed-point sums
 * (value * 2^36; the terms are <= 1): integer atomics, so the loss has the same bits every run. */
int mx_er_fwd(const float* cams, const float* sgcs, const float* lwb, int N, int K, long HW, long k, float* d, unsigned* krem,
              unsigned* prefix, unsigned long long* sum_gt, unsigned* cnt_eq, unsigned* hcnt, unsigned long long* hsum, float* loss,
              void* stream);
/* gsgcs = d loss / d raw_sgcs * gscale * (gup ? gup[0] : 1): gup is the upstream gradient as a device scalar */
int mx_er_bwd(const float* cams, const float* sgcs, const float* lwb, const unsigned* prefix, const unsigned* krem,
              const unsigned* cnt_eq, const float* gup, float gscale, float* gsgcs, int N, int K, long HW, void* stream);

/* The same ER loss computed straight from the low-resolution NHWC maps cam/sgc [N,h,w,L] (MuSCLe.py:256-257 fused in):
 * no H*W-sized tensor is read or written.  gsgc [N,h,w,L] = d loss / d sgc_lowres. */
/* k_dev (optional, device int32): the top-k count read at run time instead of k / gscale's 1/(N k) - for hipGraph replays
 * of the step, where k = int(0.2 * sum(labels) * H * W) (train_mcl.py:178,188) changes with every batch */
int mx_er_lr_fwd(const float* cam, const float* sgc, const float* lwb, int N, int h, int w, int L, int K, int H, int W, long k,
                 const int* k_dev, unsigned* krem, unsigned* prefix, unsigned long long* sum_gt, unsigned* cnt_eq, unsigned* hcnt,
                 unsigned long long* hsum, float* vals /* optional scratch [N*K*H*W]: see below */, float* loss, void* stream);
/* vals: with it the first digit pass parks |diff|*mask for the planes of the labelled classes (the rest of the buffer is
 * never touched) and the two later passes histogram those 4-byte values instead of re-evaluating upsample + softmaxes per
 * pixel; NULL = three evaluating passes, nothing of size H*W allocated.  Same result bit for bit. */
/* ws: mx_er_lr_bwd_ws bytes (64-bit fixed-point accumulators of the band kernel; plain scratch, no counter header) */
long mx_er_lr_bwd_ws(int N, int h, int w, int L, int K);
int mx_er_lr_bwd(const float* cam, const float* sgc, const float* lwb, const unsigned* prefix, const unsigned* krem,
                 const unsigned* cnt_eq, const float* gup, float gscale, const int* k_dev, float* gsgc, int N, int h, int w, int L,
                 int K, int H, int W, void* ws, long ws_bytes, void* stream);

/* torch.optim.Adam(weight_decay) update on flat arrays (train_mcl.py:134,199,229) */
/* dyn (optional, device float[3] = {lr, bias_corr1, sqrt_bias_corr2}): read at run time instead of the arguments (hipGraph replays) */
int mx_adam(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
            float weight_decay, float bias_corr1, float sqrt_bias_corr2, const float* dyn, void* stream);

/* ---- phase 2 (epochs >= 8 / >= 12): cam_maxnorm, PixPro, crops, Sinkhorn EMD ------------------------------------ */

/* cam_maxnorm (train_mcl.py:21-28) per (n,k) plane of HW elements; stats[nk] = {min, max, argmin, argmax};
 * bwd != 0: out = d/dx given gy (gradient also flows through the min / max elements, as torch's does) */
int mx_maxnorm(const float* x, const float* gy, float* out, float* stats, int NK, long HW, int bwd, void* stream);

/* PixPro (loss_multilabel.py:93-105) on NCHW maps (optionally multiplied by mask[n,k], train_mcl.py:209); coords are
 * int64 [N,4] = (h0,w0,hl,wl).  loss[0] is overwritten; g1 must hold zeros on entry; g1 = d loss / d f1.  ws: N*8 bytes (the
 * per-sample cosine sums are 64-bit fixed-point integers: same bits every run). */
int mx_pixpro(const float* f1, const float* f2, const float* mask, const long* coord1, const long* coord2, float* loss, float* g1,
              int N, int K, int H, int W, void* ws, long ws_bytes, void* stream);

/* F.normalize(x, dim=1) on NCHW (train_mcl.py:218-219) and its backward */
int mx_chan_l2norm(const float* x, const float* gy, float* out, int N, int K, long HW, int bwd, void* stream);

/* torchutils.get_dynamic_crops (torchutils.py:217-291) pieces.  table rows of 8 ints {sample,y0,x0,lh,lw,rh,rw,out_off}:
 * out[out_off + r*rw + c, 0..23] = bilinear_align_corners(src[sample,:,y0:y0+lh,x0:x0+lw] -> (rh,rw)), 21 classes + 0 pad */
int mx_crop_resize(const float* src, const int* table, int ncrops, float* out, int K, int H, int W, void* stream);
/* adjoint: gsrc[nsamples,K,H,W] += ...; ordered gather (one adder per element, crops of a sample in table order) */
int mx_crop_resize_bwd(const float* gout, const int* table, int ncrops, float* gsrc, int nsamples, int K, int H, int W, void* stream);
/* 4x4/stride-4 average pool over packed crops; table rows of 4 ints {in_off,h,w,out_off}; bwd: in = pooled grad */
int mx_avgpool4(const float* in, const int* table, int ncrops, float* out, int bwd, void* stream);

/* EMD.dynamic_matching (loss_multilabel.py:287-326).  pairs rows of 6 ints {x_off,n1,y_off,n2,sample,rank}: one workgroup per
 * row, rows in any order (longest first balances the chip); rank = the pair's position in the reference's enumeration.
 * scores: Sinkhorn distance of every pair; traj (optional): npairs * 11*(maxn1+maxn2) floats that receive the 11 states
 *         (u_t, v_t) of every pair, which mx_emd_grad differentiates;
 * best:   minimal-score pair (row index) per sample, ties to the lower rank (= the first minimal pair of the reference's stable
 *         sort, :318); loss += mean of their scores;
 * grad:   gx[crop-1 pixels of each best pair] = d loss / d x (through the 10 iterations), scaled by gscale*(gup?gup[0]:1);
 *         traj = what mx_emd_scores recorded for the same table */
int mx_emd_scores(const float* feat, const int* pairs, int npairs, int maxn1, int maxn2, float* score, float* traj, void* stream);
int mx_emd_best(const float* score, const int* pairs, int npairs, int nsamples, int* best, float* loss, void* stream);
int mx_emd_grad(const float* feat, const int* pairs, const int* best, int nsamples, int maxn1, int maxn2, const float* traj,
                const float* gup, float gscale, float* gx, void* stream);

/* ---- decoder mode / config 4: BiFPN support, CE, gradient clipping, BEACON FieldLoss ------------------------------ */

/* F.avg_pool2d(k=3,s=2,p=1) on NHWC (MuSCLe.py:51,54); bwd: x = pooled gradient, y = input gradient */
int mx_avgpool3s2(const float* x, float* y, int N, int H, int W, int C, int bwd, void* stream);
/* adjoint of mx_resize_nhwc (no relu): gsrc += W^T gdst */
int mx_resize_nhwc_bwd(const float* gdst, float* gsrc, int N, int Hs, int Ws, int C, int Hd, int Wd, void* stream);   /* ordered gather; C % 4 == 0 */
/* CrossEntropyLoss(seg [N,K,HW], argmax_k mask) (train_muscle.py:189-191): loss[0] += mean; bwd: gseg = gup[0]*dL/dseg */
int mx_ce_argmax(const float* seg, const float* mask, const float* gup, float* loss, float* gseg, int N, int K, long HW, int bwd,
                 void* ws /* forward: 8 bytes, the fixed-point sum */, long ws_bytes, void* stream);
/* F.cross_entropy(seg [N,K,HW], label [N,HW] uint8, ignore_index=ignore) against a hard label map (mask_type="label").  A pixel
 * is VALID when label != ignore and label < K; every other value (ignore itself, and any value >= K, which only the raw ABI
 * can deliver) is ignored and never used as an index.  count = number of valid pixels (an integer).
 *   forward (bwd == 0): loss[0] += sum over valid pixels of (log sum exp(seg) - seg[label]) / count; count == 0: loss[0] is
 *     left unchanged (torch gives NaN there).  The sum is kept in 64-bit fixed point as mx_ce_argmax keeps it.
 *   backward (bwd != 0): gseg = gup[0] * (softmax(seg) - onehot(label)) / count at valid pixels and exactly 0 at ignored
 *     ones (all zeros when count == 0), over whatever gseg held; the call counts the valid pixels itself.
 * ws: 16 bytes, 8-byte aligned, in both directions {uint64 fixed-point sum, uint64 count}; contents on entry do not matter.
 * Integer atomics only: the same bits every run. */
int mx_ce_label(const float* seg, const unsigned char* label, int ignore, const float* gup, float* loss, float* gseg, int N, int K,
                long HW, int bwd, void* ws, long ws_bytes, void* stream);
/* clip_grad_norm_(max_norm, 2) on a flat gradient arena (train_muscle.py:202); norm_out (optional) = total norm;
 * sq_scratch: 2048 doubles (per-workgroup partial square sums, added in a fixed order) */
int mx_clip_grad_norm(float* grads, long n, float max_norm, double* sq_scratch, float* norm_out, void* stream);
/* FieldLoss stage 1 (edge.py:423-440,45-89): softmax(beta*seg)[1:], 5x5 Sobel per labelled class, magnitude,
 * 8-way orientation, per-(n,class) max (float bits), edge_fg = sum over classes */
int mx_field_edges(const float* seg, const float* lab_fg, float beta, float* prob, float* mag, unsigned char* orient, unsigned* mx,
                   float* edge_fg, int N, int K, int H, int W, void* stream);
/* stage 2 (edge.py:196-229,372-375): per slot {n,class}: ordered out / in point lists [S][H*W], counts [S][3] */
int mx_field_select(const float* mag, const unsigned char* orient, const unsigned* mx, const int* slots, int nslots, int step,
                    int* out_list, int* in_list, int* counts, int F, int H, int W, void* stream);
/* stage 3: channel-softmaxed dense features (mode 0 full-res NCHW, mode 1 low-res NHWC upsampled on the fly) and
 * class-softmaxed mask at the sampled points pts {n, pixel}.  mask == NULL: the mask rows are not written (mfeat may be
 * NULL too); mx_field_mask_label writes them from a label map instead */
int mx_field_gather(const float* dense, int mode, int h, int w, const float* mask, const int* pts, int npts, float* feat, float* mfeat,
                    int CH, int K, int ML, int H, int W, void* stream);
/* stage 3 for a hard label map label [N,H,W] uint8 (mask_type="label"): the mask rows mfeat [npts, ML] at pts {n, pixel}.
 * label t < K (and != ignore): softmax over the K classes of onehot(t), i.e. 1 / (1 + (K-1)/e) in column t and
 * (1/e) / (1 + (K-1)/e) in the other K-1; an ignored point (ignore, or any value >= K): uniform 1/K, what the soft path's
 * zero padding gives; columns K..ML-1 are 0.  The three values are rounded once from double.  No [N,K,H,W] tensor exists. */
int mx_field_mask_label(const unsigned char* label, const int* pts, int npts, float* mfeat, int K, int ML, int H, int W, int ignore,
                        void* stream);
/* stage 5 (edge.py:231-261,330-347): loss += terms/nsamples, gsim = d loss / d sim, per slot of k x k similarities */
int mx_field_terms(const float* sim, const float* simm, int nslots, int k, float inv_n, float* loss, float* gsim,
                   float* slot_loss /* nslots floats of scratch */, void* stream);
/* stage 6: softmax backward at the out points, scattered (+=) into the dense-feature gradient */
int mx_field_scatter(const float* feat, const float* gfeat, const int* pts, int npts, int mode, int h, int w, const float* gup,
                     float* gdense, float* gpt /* mode 1: npts*CH floats of scratch */, int nsamples, int CH, int H, int W, void* stream);

/* ---- the device sampler of the BEACON boundary points (edge.FieldLoss(sampler="device")) -------------
 * The sampling rule.
 *   A slot is a pair (n, f), n in 0..N-1, f in 0..F-1, F = K-1; its index is s = n*F + f, the order of the reference's
 *   `for b ... for c` loop (src/edge.py:274-282).  A boundary pixel p of a slot is a positive as mx_field_select decides
 *   it: mag >= 0.8f*m && m > 1.  A positive gives at most one out entry, the target pixel oi(p) when it passes `keep`,
 *   and at most one in entry, ii(p), likewise.  An entry is identified by its source pixel p: targets may repeat,
 *   sources cannot.
 *   Counts.  counts[s] = {n_out, n_in, n_pos} for every slot, the values mx_field_select writes for it; an unlabelled
 *     slot (lab_fg[n,f] == 0) counts {0,0,0}.  One device function decides positives, oi, ii and keep for all kernels.
 *   Active slots.  A slot is active iff the sum over all slots of n_pos >= 10 and n_out > k and n_in > k
 *     (src/edge.py:378 and :297; the elif / else branches of :306-316 both skip the slot).
 *   Keys (uint64 arithmetic, wrapping).
 *     mix(z): z ^= z>>30; z *= 0xBF58476D1CE4E5B9; z ^= z>>27; z *= 0x94D049BB133111EB; z ^= z>>31.
 *     stream = mix(seed + 0x9E3779B97F4A7C15 * (draw + 1)).
 *     key(s, side, p) = (mix(stream ^ ((uint64)(2*s + side) << 32 | p)) >> 32 << 32) | p, side 0 = out, 1 = in.
 *     The key is unique per p; ties in the upper half are broken by p.  This requires H*W < 2^32 and 2*N*F < 2^32;
 *     the entry points refuse H*W >= 2^31 already (pixels are int32) before any launch.
 *   Draw.  For an active slot and each side, the k entries with the smallest keys: a uniform k-subset, because the
 *     keys are independent of the data.
 *   Output.  Point rows {n, target pixel}, [N*F*k, 2] int32 per side; within a slot the rows come in ascending source
 *     pixel.  The k rows of an inactive slot are {n, (s*k + j) mod H*W}: valid indices spread over distinct pixels,
 *     whose similarities mx_field_terms_masked ignores and whose gradient is exactly zero.
 *   Draw counter.  `draw` is a uint64 in device memory; mx_field_sample reads it and increments it exactly once per
 *     call, on the device, so a replayed hipGraph draws fresh points.
 * mx_field_count: counts [N*F][3] for all slots in one launch (mag/orient [N,F,H*W], mx [N,F] as mx_field_edges
 *   leaves them, lab_fg [N,F]); writes no lists. */
int mx_field_count(const float* mag, const unsigned char* orient, const unsigned* mx, const float* lab_fg, int step, int* counts,
                   int N, int F, int H, int W, void* stream);
/* mx_field_sample: active [N*F] (0/1), n_active [1], both point tables, and the counter.  state: two uint64,
 * {draw counter, stream key of the latest draw (scratch the launch fills for its own workgroups)}; seed is read as uint64. */
int mx_field_sample(const float* mag, const unsigned char* orient, const unsigned* mx, const int* counts, int step, int k, long seed,
                    void* state, int* active, int* n_active, int* pts_out, int* pts_in, int N, int F, int H, int W, void* stream);
/* mx_field_terms with active flags [nslots]: an inactive slot contributes exactly +0 to loss[0], gets slot_loss = 0 and
 * exact zeros in its gsim rows (its sim / simm rows are not read) */
int mx_field_terms_masked(const float* sim, const float* simm, const int* active, int nslots, int k, float inv_n, float* loss,
                          float* gsim, float* slot_loss /* nslots floats of scratch */, void* stream);

/* ---- dense CRF of segmentation inference (src/imutils.py:439-456, crf_inference) ---------------------------------- */

/* Mean-field inference of the fully connected CRF that src/imutils.py:439-456 hands to pydensecrf (Gaussian + bilateral
 * Potts terms, diagonal kernels, symmetric normalisation), with the sums over j evaluated EXACTLY over a square window
 * instead of on the permutohedral lattice:
 *   k_m(i,j) = exp(-0.5 |f_m(i) - f_m(j)|^2)   for |x_i-x_j| <= R_m and |y_i-y_j| <= R_m (j == i included), else 0
 *   f_gauss = (x, y) / sxy_g;   f_bilateral = (x / sxy_b, y / sxy_b, r / srgb, g / srgb, b / srgb)
 *   R_m = ceil(trunc * sxy_m);  trunc <= 0, or R_m >= max(H, W) - 1: all pairs
 *   n_m(i) = 1 / sqrt(sum_j k_m(i,j) + 1e-20)
 *   U[l,i] = -log(clip(confidence * prob[l,i] + (1 - confidence) / L, 1e-5, 1));   Q_0 = softmax_l(-U)
 *   Q_{s+1} = softmax_l(-U + sum_m w_m n_m(i) sum_j k_m(i,j) n_m(j) Q_s[l,j])      s = 0 .. t-1
 * fp32, no atomics, fixed summation order.  1 <= L <= 24.  workspace: mx_crf_workspace_bytes(L, H, W) bytes, 16-byte
 * aligned, contents need not survive between calls.  Nothing synchronises with the host. */
long mx_crf_workspace_bytes(int L, int H, int W);                       /* < 0: bad arguments */
/* src/imutils.py:439-456: the two normalisers n_gauss, n_bilateral [H,W] of the uint8 image rgb [H,W,3] */
int mx_crf_normalizers(const unsigned char* rgb, int H, int W, float sxy_g, float sxy_b, float srgb, float trunc, void* workspace,
                       float* n_g, float* n_b, void* stream);
/* src/imutils.py:439-456: the whole inference; t = 0 returns Q_0.  q_out: Q_t fp32 [L,H,W] or NULL; pred: argmax_l Q_t uint8
 * [H,W] (first maximum wins) or NULL; at least one of the two */
int mx_crf_inference(const unsigned char* rgb, const float* prob, int L, int H, int W, int t, float confidence, float sxy_g, float w_g,
                     float sxy_b, float srgb, float w_b, float trunc, void* workspace, float* q_out, unsigned char* pred, void* stream);

/* ---- IR labels from CAMs: the label CRF (src/imutils.py:477-491, crf_inference_label) and IRN's cam_to_ir_label around it;
 * csrc/crf.hip, the message kernel of the section above with the label unary ---------------------------------------------- */

/* The model of the section above (same k_m, n_m, window R_m = ceil(trunc * sxy_m) and update; the window is part of the model, so
 * label maps are not bit-identical with pydensecrf's lattice filter) with the unary of unary_from_labels(zero_unsure=False) for L
 * labels, formed in fp32:
 *   U[l,i] = -log(gt_prob) if l == label(i) else -log((1 - gt_prob) / (L - 1));   Q_0 = softmax_l(-U)
 * and the result argmax_l Q_t (first maximum wins).  src/imutils.py:477-491 fixes t = 10, gt_prob = 0.7, sxy_g = 3, w_g = 3,
 * sxy_b = 50, srgb = 5, w_b = 10; here they are arguments.  cam_to_ir_label runs it twice per image, on
 *   lab_fg = argmax([fg_thres, cams...], axis 0),  lab_bg = argmax([bg_thres, cams...], axis 0)     (first maximum wins: a CAM
 *                                                                                  value equal to the threshold is background)
 * with L = C + 1, maps both results through keys [L] (keys[0] = 0, keys[c+1] = class index of cams[c] + 1) and combines
 *   conf = fg;  conf[fg == 0] = 255;  conf[bg + fg == 0] = 0.
 * The two problems share the image, hence every k_m(i,j), both normalisers and the window walk: with fused = 1 and L <= 16 they run
 * as the columns of ONE stencil-GEMM per pass (problem g in columns g*L .. g*L+L-1 of 32, softmax per problem); otherwise one
 * problem per pass (17 <= L <= 21 always).  Both ways give the same bits.  2 <= L <= 21.  fp32, no atomics, fixed summation
 * order.  ws: mx_ir_label_ws(L, H, W) bytes, 16-byte aligned, contents need not survive between calls. */
long mx_ir_label_ws(int L, int H, int W);                               /* < 0: bad arguments */
/* src/imutils.py:477-491 twice + the combination: rgb uint8 [H,W,3], cams [C,H,W], keys int [C+1] (device) -> conf uint8 [H,W].
 * Optional: pred2 [2,H,W] = the two problems' argmax (label indices 0..C, before keys), q_out [2,L,H,W] = their Q_t.  t = 0
 * returns Q_0 / the thresholded label maps. */
int mx_ir_label(const unsigned char* rgb, const float* cams, const int* keys, int C, int H, int W, float fg_thres, float bg_thres, int t,
                float gt_prob, float sxy_g, float w_g, float sxy_b, float srgb, float w_b, float trunc, int fused, void* ws,
                unsigned char* conf, unsigned char* pred2, float* q_out, void* stream);
/* src/imutils.py:477-491 once: labels int [H,W] (a value outside 0..L-1 has no own label: every entry of its unary is the
 * "other" energy) -> pred uint8 [H,W] = argmax_l Q_t and/or q_out [L,H,W] = Q_t; at least one of the two */
int mx_crf_label(const unsigned char* rgb, const int* labels, int L, int H, int W, int t, float gt_prob, float sxy_g, float w_g,
                 float sxy_b, float srgb, float w_b, float trunc, void* ws, unsigned char* pred, float* q_out, void* stream);

/* ---- dense-CRF energy loss of decoder training (csrc/crf_loss.hip; the message pass is the stencil-GEMM of the sections above).
 * OURS, not the reference's: the regularised loss of Tang et al. 2018 ("On Regularized Losses for Weakly-supervised CNN
 * Segmentation") with the pairwise sums evaluated exactly over a window instead of on a lattice, normalised by the affinity mass. */

/* seg fp32 [N,K,H,W] logits, img fp32 [N,3,H,W] normalised as color_norm leaves it, window int [N,4] = (y0, x0, y1, x1) half-open
 * per item (NULL: the whole map), pooling factor f in {1, 2, 4, 8} with H % f == 0 and W % f == 0, h = H/f, w = W/f; u, v: cells of
 * the [h,w] grid, p: pixels.
 *   P_c(p) = softmax_c(seg[n,:,p]);   in(p) = 1 inside the window of item n, else 0
 *   rgb(p) = clamp(rint((img * std + mean) * 255), 0, 255),  mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225)
 *   r_u = 1/f^2 sum_{p in u} in(p);   S_c(u) = 1/f^2 sum_{p in u} in(p) P_c(p);   I(u) = 1/f^2 sum_{p in u} rgb(p)  (all pixels; exact)
 *   s = sxy / f;  R = ceil(trunc * s);  trunc <= 0, or R >= max(h, w) - 1: all pairs
 *   k(u,v) = exp(-(dx^2 + dy^2) / (2 s^2) - |I(u) - I(v)|^2 / (2 srgb^2))   for |dx| <= R and |dy| <= R (v == u included), else 0
 *   M_c(u) = sum_v k(u,v) S_c(v);   Z(u) = sum_v k(u,v) r_v
 *   D = sum_n sum_u r_u Z(u);   E = D - sum_n sum_u sum_c S_c(u) M_c(u);   loss = E / D,  0 where D == 0 (every window empty)
 *   gseg[n,c,p] = g (-2 / (D f^2)) in(p) P_c(p) (M_c(u(p)) - sum_c' P_c'(p) M_c'(u(p)))          (all zeros where D == 0)
 * fp32 with the two sums of D and E accumulated in double, no atomics, fixed summation order.  2 <= K <= 24, 1 <= N <= 65535,
 * H <= 65535, H*W <= 2^24.  ws: mx_crf_loss_ws(N, K, H, W, f) bytes, 16-byte aligned, contents need not survive between calls.
 * Nothing synchronises with the host. */
long mx_crf_loss_ws(int N, int K, int H, int W, int f);                 /* < 0: bad arguments */
/* forward: M [N,h,w,32] (16-byte aligned) = [M_0 .. M_{K-1} | Z | 0 ..] per cell, sums [2] = (D, sum S . M) in double, loss [1] */
int mx_crf_loss_fwd(const float* seg, const float* img, const int* window, int N, int K, int H, int W, int f, float sxy, float srgb,
                    float trunc, void* ws, float* M, double* sums, float* loss, void* stream);
/* backward: gseg [N,K,H,W] (every element written) from the forward's M and sums and the upstream scalar g [1], all on the device */
int mx_crf_loss_bwd(const float* seg, const int* window, const float* M, const double* sums, const float* g, int N, int K, int H, int W,
                    int f, float* gseg, void* stream);

/* ---- Lovasz-softmax loss of decoder training on a segmented device radix sort (csrc/lovasz.hip).  OURS, not the reference's:
 * the loss of Berman, Triki & Blaschko, "The Lovasz-Softmax loss" (CVPR 2018), for hard label maps.
 *
 * Input.  seg fp32 [N,K,HW] logits, label uint8 [N,HW].  A pixel is VALID when label != ignore and label < K; any other value is
 *   ignored and never used as an index.  p = softmax_k(seg) per pixel, fp32.
 * Groups.  per_image == 0: one group of all N*HW pixels; per_image != 0: N groups of HW pixels.  A segment is a (group, class) pair,
 *   s = group*K + c; S = groups*K segments of P elements each (N*HW or HW).  The flat index j of an element is its pixel order inside
 *   the group (n*HW + hw, or hw).
 * Per segment (group, c), over the valid pixels of the group:  fg_j = (label_j == c);  e_j = |fg_j - p_c(j)| in fp32;  G = sum fg_j;
 *   V = the number of valid pixels.
 * Order.  Descending in e, ties by ascending j: np.argsort(-e, kind="stable") over the valid elements.  rank_j in 0..V-1 is the
 *   element's position in that order; an ignored element has rank -1 and coefficient 0.
 * Jaccard increments.  i = rank + 1, F_i = the foreground count among the first i elements, I_i = G - F_i, U_i = G + i - F_i:
 *     the element at i is foreground:  g_i = 1 / U_i
 *     background and G > 0:            g_i = I_i / (U_i (U_i - 1))
 *     G == 0:                          g_1 = 1, every other g_i = 0
 *   formed in fp64 from the integer counts and rounded to fp32 once (never as a difference of two Jaccard values).
 * Segment loss.  L = sum_j e_j g_{rank_j}: products and sums in fp64, a fixed order.
 * Counted segments.  classes_all == 0 ("present"): G > 0 and V > 0; classes_all != 0 ("all"): V > 0.  C_grp = the number of counted
 *   segments of a group.  loss = (1/groups) sum_grp (1/C_grp) sum_counted L; a group with C_grp == 0 adds 0; nothing counted: the
 *   loss is exactly 0 and the gradient all zeros (the mx_ce_label convention).
 * Gradient.  coef_c(j) = w s g_{rank_j}, w = 1 / (groups C_grp) for a counted segment, else 0; s = -1 for a foreground element with
 *   p_c < 1, +1 for a background element with p_c > 0, else 0 (torch's abs subgradient: 0 at e == 0).
 *   gseg_k = gup p_k (coef_k - sum_c coef_c p_c) at valid pixels, exactly 0 at ignored ones.
 * Sort key.  e in [0,1], so bits(e) <= 0x3F800000 and key = 0x3F800000 - bits(|e|) sorts ascending; a value outside [0,1] (NaN, from
 *   non-finite logits) takes key 0 and sorts as e = 1 (results are then unspecified, but rank stays a permutation and nothing
 *   indexes out of range); an ignored element takes 0x40000000, above every valid key.  Inside the sort bit 31 carries fg and is
 *   no part of any digit.
 * The sort is a stable LSD radix sort of (key, j) pairs, 8-bit digits, 4 passes of three launches (per-block digit histogram,
 *   exclusive scan over (segment, digit, block), stable scatter by wave ballots), S independent segments; F_i is a segmented
 *   scan of the same structure.  Integer atomics for counts only; no workgroup waits for another; the same bits every run.
 * Limits: 1 <= K <= 24, P < 2^31, S * P < 2^32.  ws: mx_lovasz_ws(S, P) bytes, 16-byte aligned, contents need not survive between
 * calls.  Nothing synchronises with the host. */
long mx_lovasz_ws(int S, long P);                                       /* < 0: bad arguments */
/* stage 1: err fp32 [S,P] = e and flag uint8 [S,P] (bit 0: foreground, bit 1: valid; an ignored element has err 0, flag 0) */
int mx_lovasz_errors(const float* seg, const unsigned char* label, int ignore, int N, int K, long HW, int per_image, float* err,
                     unsigned char* flag, void* stream);
/* stages 2 and 3 on GIVEN errors: rank int32 [S,P] (may be NULL), coef_g fp32 [S,P] = g at each element in the original order (0 at
 * an ignored one), seg_loss fp64 [S] = L, seg_counts int32 [S][2] = (G, V) */
int mx_lovasz_core(const float* err, const unsigned char* flag, int S, long P, int* rank, float* coef_g, double* seg_loss,
                   int* seg_counts, void* ws, long ws_bytes, void* stream);
/* the loss: stages 1-3 and the class weighting.  err, flag, coef_g [S,P], seg_loss [S], seg_counts [S][2] as above (all written);
 * segw fp32 [S] = w of each segment; loss fp32 [1] (written, not added) */
int mx_lovasz_fwd(const float* seg, const unsigned char* label, int ignore, int N, int K, long HW, int per_image, int classes_all,
                  float* err, unsigned char* flag, float* coef_g, double* seg_loss, int* seg_counts, float* segw, float* loss, void* ws,
                  long ws_bytes, void* stream);
/* backward: gseg [N,K,HW] (every element written) from the forward's coef_g and segw and the upstream scalar gup [1] */
int mx_lovasz_bwd(const float* seg, const unsigned char* label, int ignore, const float* coef_g, const float* segw, const float* gup,
                  int N, int K, long HW, int per_image, float* gseg, void* stream);

/* ---- the permutohedral-lattice backend of both CRFs (csrc/lattice.hip): the filter pydensecrf evaluates the models of
 * src/imutils.py:439-456 and src/imutils.py:477-491 on (Adams, Baek & Davis 2010).  A DIFFERENT model from the windowed sums above
 * (its messages differ from the exact ones by up to a quarter of their size on sparse lattices), selectable, never the default; its
 * cost per pass does not grow with the kernel width.  What is pinned is the algorithm below against its numpy restatement
 * (tests/lattice_ref.py); parity with pydensecrf itself is not pinned.
 *
 * Features, fp32 with fp32 divisions: D = 2: f = (x / sxy, y / sxy);  D = 5: f = (x / sxy, y / sxy, r / srgb, g / srgb, b / srgb).
 * Construction per pixel, fp32, every operation rounded on its own (no fused multiply-add), in this order:
 *   sf[i] = (D+1) sqrt(2/3) / sqrt((i+1)(i+2))   (double, rounded to fp32 once)
 *   sm = 0;  for j = D..1: cf = f[j-1] * sf[j-1]; el[j] = sm - j * cf; sm += cf;    el[0] = sm
 *   rd[i] = floor(el[i] * fp32(1 / (D+1)) + 0.5);  rem0[i] = rd[i] * (D+1);  sum = sum_i rd[i]
 *   for i < j: if el[i] - rem0[i] < el[j] - rem0[j] then rank[i]++ else rank[j]++
 *   sum > 0: rank >= D+1-sum -> rem0 -= D+1, rank += sum - (D+1); the others rank += sum
 *   sum < 0: rank < -sum     -> rem0 += D+1, rank += D+1 + sum;   the others rank += sum
 *   b[0..D+1] = 0;  for i = 0..D: v = (el[i] - rem0[i]) / (D+1); b[D-rank[i]] += v; b[D+1-rank[i]] -= v;    b[0] += 1 + b[D+1]
 *   vertex r = 0..D: key[i] = rem0[i] + canon[r][rank[i]] for i < D, canon[r][k] = r for k <= D-r, else r - (D+1); weight b[r]
 * Distinct keys get one vertex id each (ids may differ from run to run; no value depends on them).  Blur neighbours of a vertex
 * in direction j = 0..D: n1 = the vertex with key - 1 in every coordinate but key[j] + D in coordinate j (j < D), n2 = key + 1 but
 * key[j] - D; -1 when absent.
 * Filter of C channels: splat val[vertex] += b[r] * in[pixel] (64-bit fixed point, integer atomics: the same bits in every run);
 * blur for j = 0, 1, .., D in this order val' = val + 0.5 (val[n1_j] + val[n2_j]), absent = 0; slice out[pixel] =
 * alpha sum_r b[r] val[vertex_r], alpha = 1 / (1 + 2^-D).  H * W <= 2^24 / 6, 1 <= C <= 32.  Nothing synchronises with the host. */
/* src/imutils.py:439-456: bytes of a lattice workspace for D in {2, 5}: the worst case of H*W*(D+1) vertices and C channels */
long mx_lattice_ws(int D, int H, int W, int C);                         /* < 0: bad arguments */
/* src/imutils.py:439-456: build the lattice of the uint8 image rgb [H,W,3] in ws (16-byte aligned).  srgb <= 0: the spatial
 * kernel, D = 2 (rgb is not read); else the bilateral one, D = 5.  An image whose key range does not fit the packed 64-bit hash
 * key at these widths is refused before any launch. */
int mx_lattice_build(const unsigned char* rgb, int H, int W, float sxy, float srgb, void* ws, void* stream);
/* src/imutils.py:439-456: out [C,H,W] = the filter of in [C,H,W] on the lattice that mx_lattice_build left in ws, which must have
 * been sized for at least C channels */
int mx_lattice_filter(void* ws, const float* in, float* out, int C, void* stream);
/* src/imutils.py:439-456: copies of the structure for tests, M = H*W*(D+1) rows each: vid [H*W][D+1] vertex ids, weight
 * [H*W][D+1], keys [M][D] (the first count rows are vertices), nbr [2(D+1)][M] (row 2j: n1_j, row 2j+1: n2_j), count [1] */
int mx_lattice_export(void* ws, int* vid, float* weight, int* keys, int* nbr, int* count, void* stream);
/* The CRFs with both kernels on lattices, as pydensecrf runs them: n_m = 1 / sqrt(filter_m(1) + 1e-20), message
 * w_m n_m filter_m(n_m Q), and the unary, softmax, argmax and conf rules of the windowed entries above, whose argument lists these
 * keep (without trunc / fused).  ws: mx_crf_lattice_ws(L, H, W) bytes, 16-byte aligned. */
/* src/imutils.py:439-456: workspace bytes of the three entries below for L labels, 1 <= L <= 24 */
long mx_crf_lattice_ws(int L, int H, int W);                            /* < 0: bad arguments */
/* src/imutils.py:439-456: mx_crf_inference on lattices */
int mx_crf_inference_lattice(const unsigned char* rgb, const float* prob, int L, int H, int W, int t, float confidence, float sxy_g,
                             float w_g, float sxy_b, float srgb, float w_b, void* ws, float* q_out, unsigned char* pred, void* stream);
/* src/imutils.py:477-491: mx_crf_label on lattices */
int mx_crf_label_lattice(const unsigned char* rgb, const int* labels, int L, int H, int W, int t, float gt_prob, float sxy_g, float w_g,
                         float sxy_b, float srgb, float w_b, void* ws, unsigned char* pred, float* q_out, void* stream);
/* src/imutils.py:477-491 twice + the combination: mx_ir_label on lattices (both problems as columns of one filter where 2L <= 32) */
int mx_ir_label_lattice(const unsigned char* rgb, const float* cams, const int* keys, int C, int H, int W, float fg_thres, float bg_thres,
                        int t, float gt_prob, float sxy_g, float w_g, float sxy_b, float srgb, float w_b, void* ws, unsigned char* conf,
                        unsigned char* pred2, float* q_out, void* stream);

/* ---- the IRN edge / displacement network of infer_irn.py:66 (src/backbones/resnet50_irn.py:215-232 on src/backbones/resnet50.py),
 * inference only.  Its 1x1 convolutions are mx_pw_fwd calls; these are the pieces the EfficientNet path has no use for.
 * fp32, fixed summation order, no atomics. */

/* resnet50.py:24-25 (`conv2` of a bottleneck), forward: Y[N,Ho,Wo,Co] = [relu](conv3x3(X[N,H,W,Ci], padding 1, stride 1|2) + bias[co]),
 * Ho = (H-1)/stride + 1.  Implicit GEMM on v_mfma_f32_16x16x4_f32 over an LDS-staged halo tile; EXACT fp32 always (does not follow
 * mx_set_gemm_mode).  Wp = the packed weight [9][Co][Ci] (tap = ky*3+kx major, Cin contiguous) that mx_conv3x3_pack writes from the
 * state_dict layout W[Co,Ci,3,3], each output channel multiplied by scale[co] if scale (the folded BatchNorm; pack once per
 * checkpoint load).  Ci % 4 == 0, Co % 4 == 0; bias may be NULL. */
int mx_conv3x3_pack(const float* W, const float* scale, float* Wp, int Co, int Ci, void* stream);
int mx_conv3x3_fwd(const float* X, const float* Wp, const float* bias, float* Y, int N, int H, int W, int Ci, int Co, int stride,
                   int relu, void* stream);

/* resnet50.py:62 (7x7 stride-2 pad-3 stem) as patches for mx_pw_fwd: out[(n,oy,ox), ci*49+ky*7+kx] = img[n,ci,2oy-3+ky,2ox-3+kx]
 * (NCHW image [N,3,H,W]), zero outside the image, rows of 148 floats (147 + 0).  Ho x Wo is the stem's output grid for the
 * crop_size frame the image sits in: the zero padding of resnet50_irn.py:225 is the same bounds test, no padded copy exists. */
int mx_stem7_im2col(const float* img, float* out, int N, int H, int W, int Ho, int Wo, void* stream);
/* resnet50.py:66: MaxPool2d(3, 2, 1) on NHWC, y [N,(H-1)/2+1,(W-1)/2+1,C]; padding never wins.  C % 4 == 0. */
int mx_maxpool3s2(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* resnet50.py:80-84: the rows a stride-2 1x1 convolution reads, y[n,oy,ox,:] = x[n,2oy,2ox,:], y [N,(H-1)/2+1,(W-1)/2+1,C] */
int mx_gather_s2(const float* x, float* y, int N, int H, int W, int C, void* stream);

/* resnet50_irn.py:22-92, nn.GroupNorm(G, C): stat[n][g] = {mean, 1/sqrt(biased var + eps)} over the HW x C/G values of each
 * (sample, group) of X [N,HW,ldx]; fp64 sums in a fixed order.  ws: mx_gn_stats_ws bytes of plain scratch.  (C/G) % 4 == 0. */
long mx_gn_stats_ws(int N, int HW, int G);
int mx_gn_stats(const float* X, int N, int HW, int C, int ldx, int G, float eps, void* ws, long ws_bytes, float* stat, void* stream);
/* The rest of a head in the reference's order GroupNorm -> Upsample -> crop -> ReLU (resnet50_irn.py:32-37,118-120), into a channel
 * slice of the concatenation (:121,129,130):
 * dst[n,y,x,coff+c] = [relu] bilinear_halfpixel(gamma[c]*(src[n,:,:,c] - mean)*rstd + beta[c], x scale)[y,x],  y < Hd <= Hs*scale,
 * x < Wd <= Ws*scale; scale in {1,2,4} (align_corners=False); src [N,Hs,Ws,C] dense, dst rows of ldd floats. */
int mx_gn_resize(const float* src, const float* stat, const float* gamma, const float* beta, float* dst, int N, int Hs, int Ws, int C,
                 int G, int scale, int Hd, int Wd, int ldd, int coff, int relu, void* stream);

/* infer_irn.py:76: dst[c] = F.interpolate(src[c], size=(Hd,Wd), mode='bilinear', align_corners=False) on planar [C,H,W] maps */
int mx_resize_planar_halfpixel(const float* src, float* dst, int C, int Hs, int Ws, int Hd, int Wd, void* stream);

/* resnet50_irn.py:227-230 + :107: e [2,Hf,Wf,lde] (channel 0 = fc_edge6's output), d [2,Hf,Wf,ldd] (channels 0,1 = fc_dp7's last
 * convolution), mean [2] = mean_shift.running_mean: edge[y,x] = sigmoid(e[0,y,x]/2 + e[1,y,w-1-x]/2), dp[c,y,x] = d[0,y,x,c] - mean[c]
 * for the top-left h x w crop; edge [h,w], dp [2,h,w]. */
int mx_irn_net_finish(const float* e, int lde, const float* d, int ldd, const float* mean, int Hf, int Wf, int h, int w, float* edge,
                      float* dp, void* stream);

/* ---- training the IRN heads (src/backbones/resnet50_irn.py:143-212, AffinityDisplacementLoss; csrc/irn_train.hip).  The backbone is
 * frozen (:109-114 detach every stage, :138-140), so only the loss head and the twelve 1x1-conv + GroupNorm heads have a backward.
 * Fixed summation order, fp64 loss sums, no floating-point atomics: two steps from the same state give the same bits. */

/* The loss head, forward (:204-212 + the combination of the public IRN training loop, which the reference does not ship).
 * E [N,H,W] logits with leading dimension lde (fc_edge6's 4-column GEMM output), D [N,H,W,2] with leading dimension ldd, label uint8
 * [N,H,W] (0..20, 255 = ignore): the affinity labels of src/data.py:611-637 are derived per pair, never stored.  Path table of
 * indexing.PathIndex(radius, (H,W)) as offsets: pts[2*(poff[d]+k)] = (dy,dx) of point k of path d (point 0 = the destination,
 * 0 <= dy <= radius-1, |dx| <= radius-1), plen[d] points, nd paths (:153-159, to_affinity :161-174, to_pair_displacement :176-192).
 * Sources are the (H-rf) x (W-2rf) window, rf = radius-1.  amax [N,nd,(H-rf)*(W-2rf)] bytes: position of the path maximum (first wins).
 * res[16] doubles: {pos_aff, neg_aff, dp_fg, dp_bg, total, n_bg, n_fg, n_neg, 5 backward coefficients, 0...} with
 * pos_aff = S(bg*pos)/(n_bg+1e-5)/2 + S(fg*pos)/(n_fg+1e-5)/2, neg_aff = S(neg*neg)/(n_neg+1e-5), dp_fg = S(fg*|pd-dst|)/(2 n_fg+1e-5),
 * dp_bg = S(bg*|pd|)/(2 n_bg+1e-5), total = (pos_aff+neg_aff)/2 + (dp_fg+dp_bg)/2.  ws: mx_irn_loss_ws bytes.  radius <= 16. */
long mx_irn_loss_ws(int N, int H, int W, int radius);
int mx_irn_loss_fwd(const float* E, int lde, const float* D, int ldd, const unsigned char* label, const int* pts, const int* poff,
                    const int* plen, int nd, int radius, int N, int H, int W, unsigned char* amax, void* ws, long ws_bytes, double* res,
                    void* stream);
/* Backward of `total` as a gather: dE [N*H*W,4] (column 0 = d total / d E, columns 1-3 zero), dD [N*H*W,4] (columns 0,1), the
 * operands of the 4-row data- and weight-gradient GEMMs of fc_edge6 and fc_dp7's last convolution. */
int mx_irn_loss_bwd(const float* E, int lde, const float* D, int ldd, const unsigned char* label, const int* pts, const int* poff,
                    const int* plen, int nd, int radius, int N, int H, int W, const unsigned char* amax, const double* res, float* dE,
                    float* dD, void* stream);

/* Adjoint of mx_gn_resize (:32-37,118-120): gdst = gradient of the concatenation [N,Hd,Wd,ldd], fdst = the stored forward
 * concatenation (ReLU mask: > 0), slice [coff, coff+C); dY [N,Hs,Ws,C] = gradient at the GroupNorm output. */
int mx_gn_resize_bwd(const float* gdst, const float* fdst, float* dY, int N, int Hs, int Ws, int C, int scale, int Hd, int Wd, int ldd,
                     int coff, void* stream);
/* nn.GroupNorm(G, C) backward on X [N,HW,C] (the 1x1 convolution's output) with stat from mx_gn_stats: dX (may alias dY), dgamma[C],
 * dbeta[C] (written, not added).  fp64 sums in a fixed order.  ws: mx_gn_bwd_ws bytes.  C % 32 == 0, (C/G) % 4 == 0. */
long mx_gn_bwd_ws(int N, int HW, int C, int G);
int mx_gn_bwd(const float* dY, const float* X, const float* stat, const float* gamma, int N, int HW, int C, int G, void* ws, long ws_bytes,
              float* dX, float* dgamma, float* dbeta, void* stream);

/* ---- instance pseudo-labels from the displacement field (IRN's published make_ins_seg_labels step, as DESIGN.md "Instance
 * pseudo-labels" specifies it in six steps; csrc/irn_ins.hip).  Everything after the network is O(H*W) memory on the device.
 * Only integer atomics (min / max / add): every result is independent of the execution order. */

/* Step 1, centroids.  dp [2,h,w] (plane 0 = dy, plane 1 = dx, finite); cent int32 [2,h,w] (y plane, x plane).  One thread per pixel
 * starts at its own coordinate and moves `iterations` times by the bilinear sample of dp at (ceil, floor) taps, each product and sum one
 * fp32 operation in the written order (no fused multiply-add), clipped to the image; then rounds half to even.  The field is staged in
 * LDS when 8*h*w bytes fit 160 KiB, read through L2 otherwise.  iterations >= 0. */
int mx_irn_centroids(const float* dp, int h, int w, int iterations, int* cent, void* stream);
/* Step 2, first line: weak[h,w] int32 = sqrt(dp[1]^2 + dp[0]^2) < thres ? 1 : 0, fp32, that operation order. */
int mx_irn_weak(const float* dp, int h, int w, float thres, int* weak, void* stream);
/* Steps 2 and 6, connected components: pixels with equal non-zero int32 labels that touch along an edge (4-connectivity) form a
 * component; root[h,w] int32 = the smallest linear index y*w + x of the pixel's component, -1 where label is 0.  Union-find: 16x16
 * tiles in LDS, tile borders merged with atomicMin on the parent array in ws, then every pixel follows its chain to the root.  Three
 * launches whatever the input; nothing is read back.  ws: mx_ccl_ws(h, w) bytes, contents need not survive.  h*w < 2^31. */
long mx_ccl_ws(int h, int w);                                            /* < 0: bad arguments */
int mx_ccl(const int* label, int h, int w, int* root, void* ws, void* stream);
/* Steps 2 and 6, compressing the ids that occur to 0..count-1 in ascending order.  The id of pixel p is root[q], q = p without cent,
 * q = cent[p] * w + cent[n + p] with cent (step 2: the component at the pixel's centroid); ids lie in -1..n-1, n = h*w < 2^30.
 * mx_id_mark: marks int32 [n+1] (zero-filled here), marks[id+1] = 1 for every id that occurs (marks[0]: the background, -1).
 * mx_id_rank: rank[n+1] = exclusive prefix sum of marks (one workgroup), count[0] = the number of distinct ids, count[1] = marks[0].
 * mx_id_apply: out[p] = rank[id(p) + 1] (step 2's cluster map: background first if it occurs). */
int mx_id_mark(const int* root, const int* cent, int h, int w, int* marks, void* stream);
int mx_id_rank(const int* marks, int n1, int* rank, int* count, void* stream);
int mx_id_apply(const int* root, const int* cent, int h, int w, const int* rank, int* out, void* stream);
/* Step 3: x[(k*I + i)*n + p] = cluster[p] == i ? cam[k*n + p] : 0; cam [K,n], cluster int32 [n] in 0..I-1, x [K*I, n] fully written. */
int mx_irn_ins_split(const float* cam, const int* cluster, int K, int I, int n, float* x, void* stream);
/* Step 5.  mx_irn_up_max: max_scratch[0] = the bits of the maximum mx_irn_finish divides by (the same kernel, so the same bits),
 * for any C > 0.  mx_irn_ins_finish: with that maximum and the arithmetic of csrc/irn_soft.h, label[H,W] int32 = argmax over
 * [bg_thres, rw_up_1 / max .. rw_up_C / max] (first maximum wins, 0 = background) and win[H,W] fp32 = the winning value; no [C,H,W]
 * array is written.  A maximum of 0 gives label 0 and win = bg_thres everywhere.  H <= 4h, W <= 4w. */
int mx_irn_up_max(const float* rw, int C, int h, int w, int H, int W, unsigned* max_scratch, void* stream);
int mx_irn_ins_finish(const float* rw, int C, int h, int w, int H, int W, float bg_thres, const unsigned* max_scratch, int* label,
                      float* win, void* stream);
/* Step 6 after mx_ccl + mx_id_mark/rank on the label map (n = H*W pixels): segment s = rank[root+1] - marks[0] numbers the components in
 * the order of their first pixel.  area[s] = pixel count (integer add), score_bits[s] = the bits of max win over the segment (integer
 * max on the bit patterns; win >= 0), seg_label[s] / seg_first[s] = label and index of the first pixel.  area and score_bits hold nseg
 * entries and are zero-filled here.  mx_seg_map: seg_map[p] = order[s] + 1 (order int32 [nseg]: the segment's final number), 0 where
 * root[p] < 0. */
int mx_seg_stats(const int* label, const int* root, const float* win, const int* rank, const int* marks, int n, int nseg, int* area,
                 unsigned* score_bits, int* seg_label, int* seg_first, void* stream);
int mx_seg_map(const int* root, const int* rank, const int* marks, const int* order, int n, int nseg, int* seg_map,
               void* stream);

/* ---- instance-segmentation evaluation (DESIGN.md "Instance evaluation"; csrc/ins_eval.hip): the integer joint-count table of one
 * image's prediction against its ground-truth instance map b (uint8 [n_pix], values 0..B, 0 = no object).  Every mask IoU, at every
 * threshold, follows from the table on the host.  Integer counts and integer atomic adds only, no floating point: the result does not
 * depend on the execution order.  Both entries OVERWRITE table and bad (no zeroing by the caller) and only enqueue on `stream`.
 * A value outside its range (a < 0, a > A, b > B) never indexes the table: the pixel is counted in bad[0] and skipped, so bad[0] is
 * the number of such pixels (each counted once) and the caller decides what a non-zero count means.
 * Limits: 0 < n_pix < 2^31, A >= 0, n >= 0, 0 <= B <= 255, a table of at most 2^26 cells; anything else is an argument error (negative
 * return before any launch).  No alignment is asked of a, b or masks: 16-byte packed loads are used where a group of 16 pixels lies
 * inside the array, byte loads on an unaligned start and a ragged end.
 *
 * mx_label_pair_counts: table[a[i]*(B+1) + b[i]] += 1 for every pixel i; a int32 [n_pix] is a non-overlapping label map with values
 * 0..A (InstanceLabels.seg_map: 0 = none, s = segment s-1); table int32 [(A+1)*(B+1)].  Threads add run lengths, into an LDS tile when
 * the table has at most 8192 cells; a larger table is added to directly, behind a 1024-slot LDS hash of cells per workgroup that
 * takes the adds of the cells many threads share.
 * mx_mask_pair_counts: masks uint8 [n*n_pix] (non-zero = set; masks may overlap or be empty; may be NULL when n = 0); table int32
 * [(n+1)*(B+1)]: row p in 1..n counts the pixels of mask p-1 by their b value, row 0 counts EVERY pixel (the histogram of b: the
 * ground-truth areas).  One row of workgroups per table row, each with an LDS histogram of B+1 bins. */
int mx_label_pair_counts(const int* a, const unsigned char* b, long n_pix, int A, int B, int* table, int* bad, void* stream);
int mx_mask_pair_counts(const unsigned char* masks, const unsigned char* b, long n_pix, int n, int B, int* table, int* bad, void* stream);

/* ---- boundary evaluation (DESIGN.md "Boundary evaluation"; csrc/boundary_eval.hip): trimap mIoU (the band curve of the DenseCRF /
 * DeepLab papers) and Boundary IoU (Cheng et al. 2021) from integer tables.  Integer counts and integer atomic adds only: the result
 * does not depend on the execution order.  Both entries only enqueue on `stream`.
 *
 * mx_label_edge_dist: label uint8 [H,W] (any values; 255 is an ordinary value) -> dist uint8 [H,W],
 *   dist[p] = min(dmax + 1, min over q with label[q] != label[p] of max(|dy|, |dx|)), the Chebyshev distance to the nearest pixel with
 * another label; with edge = 1 q also runs over the positions outside the image (a border pixel has distance 1), with edge = 0 over the
 * image only.  dist lies in 1..dmax+1, dmax+1 = "nothing within dmax".  For every value c and d <= dmax, (label == c) & (dist_edge1 <= d)
 * is mask_c & ~erode(mask_c, 3x3 ones, d times, zero border): the band Boundary IoU takes.  Exact for every H, W >= 1.  The separable
 * form inside one workgroup: a 16 x 64 tile with a halo of dmax labels in LDS, a row pass, a column pass; no scratch.
 * Limits: 1 <= dmax <= 64, edge 0 or 1, H*W < 2^31, H <= 1 048 560 (65 535 tile rows).
 *
 * mx_boundary_counts: pred, gt uint8 [H,W]; dt = dist(gt, edge 0), db = dist(gt, edge 1), dp = dist(pred, edge 1), all for this dmax.
 * Pixels with gt == 255 are skipped (as mx_seg_confusion); with g = gt, p = pred, a value >= K increments nothing.
 * hist int64 [6][K][dmax+2] += (bin 0 stays unused):
 *   0 T_tri [g][dt] (g < K)   1 P_tri [p][dt] (p < K)   2 TP_tri [g][dt] (p == g)
 *   3 T_b   [g][db] (g < K)   4 P_b   [p][dp] (p < K)   5 TP_b   [g][max(db,dp)] (p == g)
 * so a count "within d" is the sum of bins 1..d, and rows 2, 1, 0 summed over all bins are mx_seg_confusion's (TP, P, T).
 * ratio int64 [3][K] += (T_b, P_b, TP_b) within this image's own radius d_img (1..dmax; the caller forms it from the image diagonal).
 * Per-workgroup int32 histograms in LDS, flushed with 64-bit integer atomics.  Limits: 2 <= K <= 32, 1 <= dmax <= 64, H*W < 2^31. */
int mx_label_edge_dist(const unsigned char* label, int H, int W, int dmax, int edge, unsigned char* dist, void* stream);
int mx_boundary_counts(const unsigned char* pred, const unsigned char* gt, const unsigned char* dt, const unsigned char* db,
                       const unsigned char* dp, int K, int H, int W, int dmax, int d_img, long long* hist, long long* ratio, void* stream);

/* ---- pixel-adaptive mask refinement (PAMR; Araslanov & Roth, "Single-Stage Semantic Segmentation from Image Labels", CVPR 2020;
 * csrc/pamr.hip, muscle_amd/pamr.py, DESIGN.md "PAMR").  A local affinity from the image, once per image, then a few fixed-point
 * iterations of a convex 8 D-neighbour stencil on every channel of a mask.  The reference does not ship it; what is pinned is the
 * model below against its numpy restatement (tests/pamr_ref.py); parity with the published PAMR code unpinned.
 *
 * Inputs.  An image I with 3 channels, H x W; a mask m fp32 [C,H,W]; dilations d_0..d_{D-1} (the published default: 1,2,4,8,12,24);
 *   num_iter (default 10).  The published module resizes the mask bilinearly to the image size first; here both have the same H x W.
 * Neighbours.  Offsets o_0..o_7 = (-1,-1),(-1,0),(-1,1),(0,-1),(0,1),(1,-1),(1,0),(1,1) as (dy,dx).  Neighbour p = 8 j + k, P = 8 D in
 *   all, of the pixel (y,x) is the pixel (clamp(y + d_j dy_k, 0, H-1), clamp(x + d_j dx_k, 0, W-1)): replicate padding.
 * std_c(y,x) = the unbiased standard deviation (divide by 9 D - 1) of the 9 D values of channel c at the 9 positions, centre
 *   included, of every dilation: all dilations pooled into one sample (mean first, then the squared deviations; j-major, rows top to
 *   bottom, left to right).
 * a_p(y,x) = (1/3) sum_c -|I_c(y,x) - I_c(nbr_p)| / (1e-8 + 0.1 std_c(y,x))
 * w_p(y,x) = softmax over p of a_p(y,x), the maximum subtracted first; where std = 0 every a_p is 0 and w_p = 1/P.
 * m_{s+1}[c,y,x] = sum_p w_p(y,x) m_s[c, nbr_p],  s = 0..num_iter-1; the sum runs p = 0..P-1 in this order, starting from 0.
 * The result is m_{num_iter}; num_iter = 0 returns the input bits.
 * Arithmetic.  Every stored value (w, every m_s) and every operation of std_c, a_p and exp is fp32.  Two sums are ACCUMULATED in
 *   fp64 and rounded to fp32 once: the softmax normaliser sum_p exp(..), so that the fp32 weights of a pixel sum to 1 within 5e-8, and
 *   the stencil sum (exact products of two fp32 values, an fp64 chain in the order above).  A constant mask repeats the same
 *   roundings at a pixel in every iteration; an fp32 chain moved a constant 1.0 by 3.4e-6 .. 5.2e-6 in 10 iterations (the float32
 *   restatement does the same), this one stays within 6e-7 (the bound asked of it is 1e-6).
 * No atomics: the same inputs give the same bits in every run.  Nothing synchronises with the host.
 * Limits (argument errors, a negative return before any launch): 1 <= D <= 8, every dilation in 1..64, N, C, H, W >= 1,
 *   N max(C,P) H W < 2^31.  There is no cap on C. */
/* w fp32 [N,P,H,W] (planar, every element written) from img: img_kind 0 = uint8 [N,H,W,3] (what the CRFs take), img_kind 1 = fp32
 * [N,3,H,W]; equal values give equal bits.  dil: D ints in HOST memory. */
int mx_pamr_affinity(const void* img, int img_kind, int N, int H, int W, const int* dil, int D, float* w, void* stream);
/* one iteration: m_out [N,C,H,W] from m_in and w.  One thread owns a pixel, holds its P weights in registers and walks the C
 * channels; the gathers are served by the caches.  m_in must not overlap m_out. */
int mx_pamr_step(const float* w, const float* m_in, float* m_out, int N, int C, int H, int W, const int* dil, int D, void* stream);
long mx_pamr_ws(int N, int C, int H, int W, int D);                     /* < 0: bad arguments */
/* the affinity and num_iter iterations: out [N,C,H,W] = m_{num_iter} for odd and even counts alike (the iterations alternate between
 * out and one buffer of the workspace; num_iter = 0 is a device copy); mask is only read and must not overlap out.  The same bits as
 * mx_pamr_affinity followed by num_iter calls of mx_pamr_step.  ws: mx_pamr_ws(N, C, H, W, D) bytes, 16-byte aligned, contents need
 * not survive between calls. */
int mx_pamr(const void* img, int img_kind, const float* mask, float* out, int N, int C, int H, int W, const int* dil, int D, int num_iter,
            void* ws, long ws_bytes, void* stream);
/* pred uint8 [N,H,W] = argmax_c m[n,c,y,x], first maximum wins (np.argmax on finite data); 1 <= C <= 256 */
int mx_planar_argmax(const float* m, int N, int C, int H, int W, unsigned char* pred, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSCLE_HIP_H */
