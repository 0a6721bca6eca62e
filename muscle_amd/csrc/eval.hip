// The evaluation entry points: every kernel whose result is an integer (TP, P, T) table per class (src/evaluation.py:19-52), counted
// with the one core of eval_counts.h.  (mx_seg_infer_batch of head.hip is an inference kernel that also counts, with the same core.)
#include "eval_counts.h"
#include "irn_soft.h"
#include <hip/hip_fp16.h>

// src/evaluation.py:36-50 (input_type='png') for one image: the rule of eval_counts.h on a uint8 prediction.  counts int64 [K][3] =
// (TP, P, T), accumulated across images.
__global__ __launch_bounds__(256) void seg_confusion_kernel(const unsigned char* pred, const unsigned char* gt, int K, long HW,
                                                            long long* counts) {
  extern __shared__ int sc[];                   // [K][3]
  for (int i = threadIdx.x; i < K * 3; i += 256) sc[i] = 0;
  __syncthreads();
  for (long p = blockIdx.x * 256L + threadIdx.x; p < HW; p += (long)gridDim.x * 256) {
    const int g = gt[p], pr = pred[p];
    if (g >= 255) continue;
    eval_count(sc, 0, pr, g, K);
  }
  __syncthreads();
  eval_flush(sc, K * 3, counts);
}

// ---------------------------------------------------------------------------
// Per-epoch rapid evaluation (train_mcl.py:286-318 + src/evaluation.py:19-52): for every threshold t,
//   predict = argmax_k [t, half(pred_1*label_1), ..., half(pred_{K-1}*label_{K-1})]   (first maximum wins, as np.argmax)
// pred: one image, [K,H,W] fp32 (already cam_maxnorm'ed); label: [K] (entry 0 unused); gt: uint8 [H,W].
// counts: int64 [nt][K][3] = (TP, P, T), accumulated across images.  The values go through fp16 exactly as the script's
// np.half files do.  Per workgroup the counts are kept in LDS (nt*K*3 ints) and flushed once.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eval_confusion_kernel(const float* pred, const float* label, const unsigned char* gt,
                                                             const float* thr, int nt, int K, long HW, long long* counts) {
  extern __shared__ int lc[];                   // [nt][K][3]
  for (int i = threadIdx.x; i < nt * K * 3; i += 256) lc[i] = 0;
  __syncthreads();
  for (long p = blockIdx.x * 256L + threadIdx.x; p < HW; p += (long)gridDim.x * 256) {
    const int g = gt[p];
    if (g >= 255) continue;
    float best = -1.f;                          // values are >= 0; strict > keeps the first maximum
    int bk = 0;
    for (int k = 1; k < K; ++k) {
      float v = __half2float(__float2half_rn(pred[(long)k * HW + p] * label[k]));
      if (v > best) { best = v; bk = k; }
    }
    for (int t = 0; t < nt; ++t) {
      const int pr = (thr[t] >= best) ? 0 : bk;  // channel 0 holds the threshold and precedes every other channel
      __builtin_assume(pr < K);                  // 0 or a class of the loop above: the rule's guard costs nothing here
      eval_count(lc, t * K, pr, g, K);
    }
  }
  __syncthreads();
  eval_flush(lc, nt * K * 3, counts);
}

// ---------------------------------------------------------------------------
// mx_rapid_eval_lr: the rapid evaluation of B images of one size straight from the model's low-resolution SGC maps
// (cam='cam_lr', NHWC [B,h,w,lds]): train_mcl.py:297-303 + src/evaluation.py:19-52 without any [K,H,W] tensor.  Every
// full-resolution value is recomputed from its <= 4 low-res neighbours with upsample_ac_value (common.h: the bits of
// mx_upsample_to_nchw), normalised with maxnorm_apply (the bits of mx_maxnorm) and counted as eval_confusion_kernel counts.
// Grid: (row bands, images); a workgroup owns `rows` consecutive rows of one image, one thread one pixel at a time with the
// pixel's coordinates and weights computed once and the channels read 16 bytes at a time.
// Phase (a), rapid_extremes_kernel: ext[b][k] = {~bits(min), bits(max)} of relu(upsample) over the H x W grid.  The values
//   are non-negative floats, whose bit patterns order as the floats do, and min / max do not depend on order: wave reduce,
//   LDS integer atomicMax, one global integer atomicMax per workgroup and entry (the min is kept as the complement, so both
//   are maxima over a zero-filled scratch).  Exact, the same bits every run.
// Phase (b), rapid_count_kernel: per pixel with gt < 255 the first maximum over k = 1..K-1 of half(maxnorm * label_k), then
//   per threshold P[pr]++ and TP[g] += (pr == g) in LDS; T[g] does not depend on the threshold: one LDS counter per class,
//   added to every threshold's column at the flush (its own layout, [nt][K][2] + T[K], for speed at nt = 16; pr < K by construction).
// ---------------------------------------------------------------------------
struct RevPixel { int o00, o01, o10, o11; float wy, wx; };

__device__ __forceinline__ RevPixel rev_pixel(int y, int x, int h, int w, int lds, int H, int W) {
  int y0, y1, x0, x1;
  RevPixel p;
  bil_coord_rn(y, h, H, y0, y1, p.wy);
  bil_coord_rn(x, w, W, x0, x1, p.wx);
  p.o00 = (y0 * w + x0) * lds; p.o01 = (y0 * w + x1) * lds;
  p.o10 = (y1 * w + x0) * lds; p.o11 = (y1 * w + x1) * lds;
  return p;
}
// channels 4q .. 4q+3 of the upsampled map at the pixel
__device__ __forceinline__ float4 rev_quad(const float* src, const RevPixel& p, int q) {
  const float4 a00 = ld4(src + p.o00 + q * 4), a01 = ld4(src + p.o01 + q * 4);
  const float4 a10 = ld4(src + p.o10 + q * 4), a11 = ld4(src + p.o11 + q * 4);
  return make_float4(upsample_ac_value(a00.x, a01.x, a10.x, a11.x, p.wy, p.wx), upsample_ac_value(a00.y, a01.y, a10.y, a11.y, p.wy, p.wx),
                     upsample_ac_value(a00.z, a01.z, a10.z, a11.z, p.wy, p.wx), upsample_ac_value(a00.w, a01.w, a10.w, a11.w, p.wy, p.wx));
}
// bit pattern of relu(v) with the sign of a zero dropped (fmaxf(-0, 0) may be either zero; mx_maxnorm's result does not
// depend on which: the extremes only enter x - mn - 1e-6 and mx - mn + 1e-6)
__device__ __forceinline__ unsigned rev_bits(float v) { return __float_as_uint(fmaxf(v, 0.f)) & 0x7fffffffu; }

__global__ __launch_bounds__(256) void rapid_extremes_kernel(const float* sgc, int h, int w, int lds, int K, int H, int W, int rows,
                                                             unsigned* ext) {
  __shared__ unsigned se[EVAL_MAXK * 2];
  const int b = blockIdx.y, yb = blockIdx.x * rows;
  const int npix = min(rows, H - yb) * W;
  const float* src = sgc + (long)b * h * w * lds;
  if (threadIdx.x < EVAL_MAXK * 2) se[threadIdx.x] = 0u;
  __syncthreads();
  unsigned lo[EVAL_MAXK], hi[EVAL_MAXK];               // lo = ~bits of the running minimum: both are running maxima
#pragma unroll
  for (int k = 0; k < EVAL_MAXK; ++k) { lo[k] = 0u; hi[k] = 0u; }
  for (int p = threadIdx.x; p < npix; p += 256) {
    const RevPixel px = rev_pixel(yb + p / W, p % W, h, w, lds, H, W);
#pragma unroll
    for (int q = 0; q < EVAL_MAXK / 4; ++q) {
      if (q * 4 < K) {                                 // quad q lies inside the row: K <= lds and lds % 4 == 0
        const float4 v = rev_quad(src, px, q);
        const unsigned u[4] = {rev_bits(v.x), rev_bits(v.y), rev_bits(v.z), rev_bits(v.w)};
#pragma unroll
        for (int j = 0; j < 4; ++j) { lo[q * 4 + j] = max(lo[q * 4 + j], ~u[j]); hi[q * 4 + j] = max(hi[q * 4 + j], u[j]); }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < EVAL_MAXK; ++k) {                // (a thread without a pixel still holds 0, the identity of both maxima)
    if (k < K) {
      unsigned a = lo[k], c = hi[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { a = max(a, (unsigned)__shfl_xor((int)a, o, 64)); c = max(c, (unsigned)__shfl_xor((int)c, o, 64)); }
      if ((threadIdx.x & 63) == 0) { atomicMax(&se[k * 2], a); atomicMax(&se[k * 2 + 1], c); }
    }
  }
  __syncthreads();
  if (threadIdx.x < K * 2) atomicMax(&ext[(long)b * K * 2 + threadIdx.x], se[threadIdx.x]);
}

__global__ __launch_bounds__(256) void rapid_count_kernel(const float* sgc, const float* label, const unsigned char* gt, const float* thr,
                                                          int nt, int h, int w, int lds, int K, int H, int W, int rows,
                                                          const unsigned* ext, long long* counts) {
  __shared__ int lc[EVAL_MAXT * EVAL_MAXK * 2];        // [nt][K][2] = (TP, P)
  __shared__ int ht[EVAL_MAXK];                        // T per class
  __shared__ float smn[EVAL_MAXK], sinv[EVAL_MAXK], slab[EVAL_MAXK], sth[EVAL_MAXT];
  const int b = blockIdx.y, yb = blockIdx.x * rows;
  const int npix = min(rows, H - yb) * W;
  const float* src = sgc + (long)b * h * w * lds;
  const unsigned char* g8 = gt + ((long)b * H + yb) * W;
  for (int i = threadIdx.x; i < nt * K * 2; i += 256) lc[i] = 0;
  if (threadIdx.x < EVAL_MAXK) {
    const int k = threadIdx.x;
    ht[k] = 0;
    float mn = 0.f, mx = 0.f, lb = 0.f;
    if (k < K) {
      mn = __uint_as_float(~ext[((long)b * K + k) * 2]);
      mx = __uint_as_float(ext[((long)b * K + k) * 2 + 1]);
      lb = label[(long)b * K + k];
    }
    smn[k] = mn; sinv[k] = maxnorm_inv(mn, mx); slab[k] = lb;
  }
  if (threadIdx.x < nt) sth[threadIdx.x] = thr[threadIdx.x];
  __syncthreads();
  for (int p = threadIdx.x; p < npix; p += 256) {
    const int g = g8[p];
    if (g >= 255) continue;
    const RevPixel px = rev_pixel(yb + p / W, p % W, h, w, lds, H, W);
    float best = -1.f;                                 // values are >= 0; strict > keeps the first maximum
    int bk = 0;
#pragma unroll
    for (int q = 0; q < EVAL_MAXK / 4; ++q) {
      if (q * 4 < K) {
        const float4 u = rev_quad(src, px, q);
        const float v[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = q * 4 + j;
          if (k >= 1 && k < K) {
            const float m = maxnorm_apply(v[j], smn[k], sinv[k]);
            const float hv = __half2float(__float2half_rn(m * slab[k]));
            if (hv > best) { best = hv; bk = k; }
          }
        }
      }
    }
    if (g < K) atomicAdd(&ht[g], 1);
    for (int t = 0; t < nt; ++t) {
      const int pr = (sth[t] >= best) ? 0 : bk;        // channel 0 holds the threshold and precedes every other channel
      atomicAdd(&lc[(t * K + pr) * 2 + 1], 1);
      if (pr == g) atomicAdd(&lc[(t * K + g) * 2], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nt * K; i += 256) eval_flush_entry(counts + (long)i * 3, lc[i * 2], lc[i * 2 + 1], ht[i % K]);
}

// ---------------------------------------------------------------------------
// src/evaluation.py:25-50 (input_type='npy') for one image and ALL thresholds of the curve at once.
//   predict(t) = argmax_k [t, tensor_1 .. tensor_{K-1}]  (first maximum wins), tensor_{key+1} = the dict's float32 map,
//   absent channels 0.
// For t >= 0 an absent channel never beats channel 0, so only the kept maps are compared: (best, bk) = their first
// maximum, which does not depend on t; predict(t) = (t >= best) ? 0 : bk: the bins of EvalBins (eval_counts.h).
// maps fp32 [nkeep,H,W]; keys int32 [nkeep] ascending in 0..K-2; thr fp32 [nt] ascending, >= 0; counts int64 [nt][K][3]
// = (TP, P, T), accumulated with integer atomics: exact.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void camdict_confusion_kernel(const float* maps, const int* keys, int nkeep,
                                                                const unsigned char* gt, const float* thr, int nt, int K, long HW,
                                                                long long* counts) {
  __shared__ EvalBins hb;
  __shared__ int sk[EVAL_MAXK];
  hb.init(thr, nt, K);
  if (threadIdx.x < nkeep) sk[threadIdx.x] = keys[threadIdx.x] + 1;
  __syncthreads();
  for (long p = blockIdx.x * 256L + threadIdx.x; p < HW; p += (long)gridDim.x * 256) {
    const int g = gt[p];
    if (g >= 255) continue;
    float best = maps[p];
    int bk = sk[0];
    for (int j = 1; j < nkeep; ++j) {
      const float v = maps[(long)j * HW + p];
      if (v > best) { best = v; bk = sk[j]; }    // strict: the first maximum wins, as np.argmax
    }
    hb.add(hb.bin(best, nt), bk, g, K);
  }
  hb.flush(nt, K, counts);
}

// ---------------------------------------------------------------------------
// Scoring the random walk's (exp_times, threshold) grid in one pass (infer_irn.py:76-92 + src/evaluation.py:36-50): for every
// snapshot e of the walk (mx_irn_walk_snap) and every threshold t, the (TP, P, T) counts mx_seg_confusion would give for the
// label map mx_irn_finish(rw[e], ..., bg_thres = t) writes - without writing a label map.
//   predict(t) = argmax over [t, v_1 .. v_C],  v_c = irn_soft_value(rw_c) (irn_soft.h, the label kernel's arithmetic), first
//   maximum wins, a channel that is absent from the CAM dict is exactly 0 and never beats a t >= 0.
// The winner among the kept channels, (best, bk) = their first strict maximum, does not depend on t; predict(t) = bk where
// t < best and 0 otherwise (a tie v == t stays background, as `v > best` in irn_label_kernel): the bins of EvalBins.  A maximum
// of 0 makes every value NaN: no channel wins, bin 0, background at every threshold, as irn_label_kernel gives.
// grid (x, E): snapshot blockIdx.y.  rw [E][Kp][h][w]; keys [Kp] ascending in 0..K-2; vmax [E] the bits of the maximum each
// snapshot is divided by; counts [E][nt][K][3].
// ---------------------------------------------------------------------------
#define IRS_MAXE 13

__global__ __launch_bounds__(256) void irn_sweep_confusion_kernel(const float* __restrict__ rw, const int* __restrict__ keys, int Kp,
                                                                  int h, int w, const unsigned char* __restrict__ gt, int H, int W,
                                                                  const float* __restrict__ thr, int nt, int K,
                                                                  const unsigned* __restrict__ vmax, long long* __restrict__ counts) {
  __shared__ EvalBins hb;
  __shared__ int sk[EVAL_MAXK];
  hb.init(thr, nt, K);
  if (threadIdx.x < Kp) sk[threadIdx.x] = keys[threadIdx.x] + 1;
  __syncthreads();
  const int e = blockIdx.y;
  const float* m = rw + (long)e * Kp * h * w;
  const float mx = __uint_as_float(vmax[e]);
  const long HW = (long)H * W;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < HW; p += (long)gridDim.x * 256) {
    const int g = gt[p];
    if (g >= 255) continue;
    const int X = (int)(p % W), Y = (int)(p / W);
    float best = -INFINITY;
    int bk = 0;
    for (int j = 0; j < Kp; ++j) {
      const float v = irn_soft_value(m + (long)j * h * w, h, w, Y, X, mx);
      if (v > best) { best = v; bk = sk[j]; }          // strict: the first maximum wins; a NaN never does
    }
    hb.add(hb.bin(best, nt), bk, g, K);
  }
  hb.flush(nt, K, counts + (long)e * nt * K * 3);
}

// workgroups of the one-image counting kernels: eight pixels per thread, at least one, at most 1024
static int eval_grid(long HW) {
  const long b = (HW + 256 * 8 - 1) / (256 * 8);
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

// rows of one image per workgroup of the rapid-evaluation kernels: about 512 workgroups (two per CU) for the batch
static int rev_rows(int B, int H) {
  int r = (int)(((long)B * H + 511) / 512);
  return r < 1 ? 1 : r;
}

extern "C" {

int mx_eval_confusion(const float* pred, const float* label, const unsigned char* gt, const float* thresholds, int nt, int K, int H,
                      int W, long long* counts, void* stream) {
  MX_CHECK_ARG(pred && label && gt && thresholds && counts && nt > 0 && nt <= 64 && K >= 2 && K <= 256 && H > 0 && W > 0,
               "eval_confusion: bad args");
  const long HW = (long)H * W;
  hipLaunchKernelGGL(eval_confusion_kernel, dim3(eval_grid(HW)), dim3(256), sizeof(int) * nt * K * 3, (hipStream_t)stream, pred, label,
                     gt, thresholds, nt, K, HW, counts);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

long mx_rapid_eval_lr_ws(int B, int K) { return (B > 0 && K > 0) ? (long)B * K * 2 * (long)sizeof(unsigned) : 0; }

int mx_rapid_eval_lr(const float* sgc, const float* label_with_bg, const unsigned char* gt, const float* thresholds, int nt, int B,
                     int h, int w, int lds, int K, int H, int W, long long* counts, void* ws, long ws_bytes, void* stream) {
  MX_CHECK_ARG(sgc && label_with_bg && gt && thresholds && counts && ws, "rapid_eval_lr: NULL argument");
  MX_CHECK_ARG(nt > 0 && nt <= EVAL_MAXT && K >= 2 && K <= EVAL_MAXK && K <= lds && lds % 4 == 0 && B > 0 && B <= 65535 && h > 0 &&
                   w > 0 && H > 0 && W > 0 && (long)h * w * lds < 0x7fffffffL && (long)H * W < 0x7fffffffL,
               "rapid_eval_lr: bad args nt=%d B=%d h=%d w=%d lds=%d K=%d H=%d W=%d", nt, B, h, w, lds, K, H, W);
  MX_CHECK_ARG(ws_bytes >= mx_rapid_eval_lr_ws(B, K), "rapid_eval_lr: ws has %ld bytes, needs %ld", ws_bytes,
               mx_rapid_eval_lr_ws(B, K));
  hipStream_t st = (hipStream_t)stream;
  const int rows = rev_rows(B, H);
  const dim3 grid((H + rows - 1) / rows, B);
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)mx_rapid_eval_lr_ws(B, K), st);
  if (e != hipSuccess) { mx_set_error("rapid_eval_lr: memset failed: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(rapid_extremes_kernel, grid, dim3(256), 0, st, sgc, h, w, lds, K, H, W, rows, (unsigned*)ws);
  MX_LAUNCH_CHECK();
  hipLaunchKernelGGL(rapid_count_kernel, grid, dim3(256), 0, st, sgc, label_with_bg, gt, thresholds, nt, h, w, lds, K, H, W, rows,
                     (const unsigned*)ws, counts);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_seg_confusion(const unsigned char* pred, const unsigned char* gt, int K, int H, int W, long long* counts, void* stream) {
  MX_CHECK_ARG(pred && gt && counts && K >= 1 && K <= 255 && H > 0 && W > 0, "seg_confusion: bad args K=%d H=%d W=%d", K, H, W);
  const long HW = (long)H * W;
  hipLaunchKernelGGL(seg_confusion_kernel, dim3(eval_grid(HW)), dim3(256), sizeof(int) * K * 3, (hipStream_t)stream, pred, gt, K, HW,
                     counts);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_camdict_confusion(const float* maps, const int* keys, int nkeep, const unsigned char* gt, const float* thresholds, int nt,
                         int K, int H, int W, long long* counts, void* stream) {
  MX_CHECK_ARG(maps && keys && gt && thresholds && counts, "camdict_confusion: NULL argument");
  MX_CHECK_ARG(nt > 0 && nt <= EVAL_MAXT && K >= 2 && K <= EVAL_MAXK && nkeep > 0 && nkeep <= K - 1 && H > 0 && W > 0,
               "camdict_confusion: bad args nt=%d K=%d nkeep=%d H=%d W=%d", nt, K, nkeep, H, W);
  const long HW = (long)H * W;
  hipLaunchKernelGGL(camdict_confusion_kernel, dim3(eval_grid(HW)), dim3(256), 0, (hipStream_t)stream, maps, keys, nkeep, gt, thresholds,
                     nt, K, HW, counts);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_irn_sweep_confusion(const float* rw, int E, int Kp, const int* keys, int h, int w, const unsigned char* gt, int H, int W,
                           const float* thresholds, int nt, int K, const unsigned* vmax, long long* counts, void* stream) {
  MX_CHECK_ARG(gt && thresholds && vmax && counts && (Kp == 0 || (rw && keys)), "irn_sweep_confusion: null pointer");
  MX_CHECK_ARG(nt >= 1 && nt <= EVAL_MAXT, "irn_sweep_confusion: nt must be 1..%d (got %d)", EVAL_MAXT, nt);
  MX_CHECK_ARG(K >= 2 && K <= EVAL_MAXK, "irn_sweep_confusion: K must be 2..%d (got %d)", EVAL_MAXK, K);
  MX_CHECK_ARG(E >= 1 && E <= IRS_MAXE && Kp >= 0 && Kp <= K - 1, "irn_sweep_confusion: bad E=%d or Kp=%d (K=%d)", E, Kp, K);
  MX_CHECK_ARG(h > 0 && w > 0 && H > 0 && W > 0 && H <= 4 * h && W <= 4 * w && (long)h * w * (Kp > 0 ? Kp : 1) * E < (1L << 31),
               "irn_sweep_confusion: bad geometry h=%d w=%d H=%d W=%d (the label map is the top-left HxW crop of the 4x upsampled maps)",
               h, w, H, W);
  hipLaunchKernelGGL(irn_sweep_confusion_kernel, dim3(eval_grid((long)H * W), E), dim3(256), 0, (hipStream_t)stream, rw, keys, Kp, h, w,
                     gt, H, W, thresholds, nt, K, vmax, counts);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
