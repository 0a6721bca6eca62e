// Scoring the random walk's (exp_times, threshold) grid in one pass (infer_irn.py:76-92 + src/evaluation.py:36-50): for every
// snapshot e of the walk (mx_irn_walk_snap) and every threshold t, the (TP, P, T) counts mx_seg_confusion would give for the
// label map mx_irn_finish(rw[e], ..., bg_thres = t) writes - without writing a label map.
//   predict(t) = argmax over [t, v_1 .. v_C],  v_c = irn_soft_value(rw_c) (irn_soft.h, the label kernel's arithmetic), first
//   maximum wins, a channel that is absent from the CAM dict is exactly 0 and never beats a t >= 0.
// The winner among the kept channels, (best, bk) = their first strict maximum, does not depend on t; predict(t) = bk where
// t < best and 0 otherwise (a tie v == t stays background, as `v > best` in irn_label_kernel).  With ascending thresholds the
// pixel is described by its bin b = #{t_i < best}: thresholds i < b see bk, thresholds i >= b see 0 - the bin argument of
// camdict_confusion_kernel (head.hip), whose histograms and flush this kernel repeats.  A maximum of 0 makes every value NaN:
// no channel wins, bin 0, background at every threshold, as irn_label_kernel gives.  Integer atomics only: exact.
#include "common.h"
#include "irn_soft.h"

#define IRS_MAXT 64
#define IRS_MAXK 24
#define IRS_MAXE 13

// grid (x, E): snapshot blockIdx.y.  rw [E][Kp][h][w]; keys [Kp] ascending in 0..K-2; vmax [E] the bits of the maximum each
// snapshot is divided by; counts [E][nt][K][3].  Pixels with gt == 255 are skipped, gt in K..254 count towards P only
// (seg_confusion_kernel, head.hip).
__global__ __launch_bounds__(256) void irn_sweep_confusion_kernel(const float* __restrict__ rw, const int* __restrict__ keys, int Kp,
                                                                  int h, int w, const unsigned char* __restrict__ gt, int H, int W,
                                                                  const float* __restrict__ thr, int nt, int K,
                                                                  const unsigned* __restrict__ vmax, long long* __restrict__ counts) {
  __shared__ int hp[(IRS_MAXT + 1) * IRS_MAXK], hq[(IRS_MAXT + 1) * IRS_MAXK], ht[IRS_MAXK], hrow[IRS_MAXT + 1];
  __shared__ float st[IRS_MAXT];
  __shared__ int sk[IRS_MAXK];
  for (int i = threadIdx.x; i < (nt + 1) * K; i += 256) { hp[i] = 0; hq[i] = 0; }
  if (threadIdx.x < K) ht[threadIdx.x] = 0;
  if (threadIdx.x < nt) st[threadIdx.x] = thr[threadIdx.x];
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
    int b = 0;
    for (int t = 0; t < nt; ++t) b += (st[t] < best) ? 1 : 0;
    if (b == 0) bk = 0;                                // background at every threshold, whoever led
    atomicAdd(&hp[b * K + bk], 1);
    if (g < K) {
      atomicAdd(&ht[g], 1);
      if (g == bk || g == 0) atomicAdd(&hq[b * K + g], 1);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b <= nt; b += 256) {           // pixels per bin, any winner
    int s = 0;
    for (int c = 0; c < K; ++c) s += hp[b * K + c];
    hrow[b] = s;
  }
  __syncthreads();
  long long* ce = counts + (long)e * nt * K * 3;
  for (int i = threadIdx.x; i < nt * K; i += 256) {
    const int t = i / K, c = i % K;
    int P = 0, TP = 0;
    if (c == 0) {
      for (int b = 0; b <= t; ++b) { P += hrow[b]; TP += hq[b * K]; }
    } else {
      for (int b = t + 1; b <= nt; ++b) { P += hp[b * K + c]; TP += hq[b * K + c]; }
    }
    unsigned long long* d = (unsigned long long*)&ce[(long)i * 3];
    if (TP) atomicAdd(d + 0, (unsigned long long)TP);
    if (P) atomicAdd(d + 1, (unsigned long long)P);
    if (ht[c]) atomicAdd(d + 2, (unsigned long long)ht[c]);
  }
}

extern "C" {

int mx_irn_sweep_confusion(const float* rw, int E, int Kp, const int* keys, int h, int w, const unsigned char* gt, int H, int W,
                           const float* thresholds, int nt, int K, const unsigned* vmax, long long* counts, void* stream) {
  MX_CHECK_ARG(gt && thresholds && vmax && counts && (Kp == 0 || (rw && keys)), "irn_sweep_confusion: null pointer");
  MX_CHECK_ARG(nt >= 1 && nt <= IRS_MAXT, "irn_sweep_confusion: nt must be 1..%d (got %d)", IRS_MAXT, nt);
  MX_CHECK_ARG(K >= 2 && K <= IRS_MAXK, "irn_sweep_confusion: K must be 2..%d (got %d)", IRS_MAXK, K);
  MX_CHECK_ARG(E >= 1 && E <= IRS_MAXE && Kp >= 0 && Kp <= K - 1, "irn_sweep_confusion: bad E=%d or Kp=%d (K=%d)", E, Kp, K);
  MX_CHECK_ARG(h > 0 && w > 0 && H > 0 && W > 0 && H <= 4 * h && W <= 4 * w && (long)h * w * (Kp > 0 ? Kp : 1) * E < (1L << 31),
               "irn_sweep_confusion: bad geometry h=%d w=%d H=%d W=%d (the label map is the top-left HxW crop of the 4x upsampled maps)",
               h, w, H, W);
  const long HW = (long)H * W;
  int blocks = (int)((HW + 256 * 8 - 1) / (256 * 8));
  if (blocks < 1) blocks = 1;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(irn_sweep_confusion_kernel, dim3(blocks, E), dim3(256), 0, (hipStream_t)stream, rw, keys, Kp, h, w, gt, H, W,
                     thresholds, nt, K, vmax, counts);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
