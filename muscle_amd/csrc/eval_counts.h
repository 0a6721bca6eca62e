// The counting core of the evaluation kernels (eval.hip, and seg_infer_kernel<true> of head.hip).  Device code only.
//
// Every quality number is read from an integer table counts[..][K][3] = (TP, P, T) per class, src/evaluation.py:36-50:
//   a pixel with gt == 255 is skipped (by the caller); otherwise P[predict]++, and where gt < K also T[gt]++ and
//   TP[gt] += (predict == gt).  A gt in K..254 therefore counts towards P only.
// The table is counted per workgroup (256 threads) in LDS and flushed with one 64-bit integer atomic per non-zero entry: exact, the
// same integers every run.  eval_count / eval_flush: a direct LDS table [..][K][3]; EvalBins: all thresholds of an ascending list.
#pragma once
#include "common.h"

// the largest threshold list and class count of the kernels whose LDS tables are static (rapid_count_kernel, EvalBins)
#define EVAL_MAXT 64
#define EVAL_MAXK 24

// one pixel with prediction pr and ground truth g (g != 255) into the K rows of the LDS table tab[..][3] that start at `row`
__device__ __forceinline__ void eval_count(int* tab, int row, int pr, int g, int K) {
  if (pr < K) atomicAdd(&tab[(row + pr) * 3 + 1], 1);
  if (g < K) {
    atomicAdd(&tab[(row + g) * 3 + 2], 1);
    if (pr == g) atomicAdd(&tab[(row + g) * 3 + 0], 1);
  }
}

// one (TP, P, T) entry of a workgroup into the global table
__device__ __forceinline__ void eval_flush_entry(long long* d, int TP, int P, int T) {
  unsigned long long* u = (unsigned long long*)d;
  if (TP) atomicAdd(u + 0, (unsigned long long)TP);
  if (P) atomicAdd(u + 1, (unsigned long long)P);
  if (T) atomicAdd(u + 2, (unsigned long long)T);
}

// the n ints of a direct LDS table into the global table of the same layout (the caller has synchronised)
__device__ __forceinline__ void eval_flush(const int* tab, int n, long long* counts) {
  for (int i = threadIdx.x; i < n; i += 256)
    if (tab[i]) atomicAdd((unsigned long long*)&counts[i], (unsigned long long)tab[i]);
}

// Threshold-bin histograms of one workgroup (declare it __shared__).  For t >= 0 and ascending thresholds a pixel whose kept channels
// have the first strict maximum (best, bk) predicts bk at the thresholds i < b and 0 at the thresholds i >= b, b = bin(best).  Per
// pixel at most three LDS atomics, independent of nt:  hp[b][bk]++;  hq[b][g]++ if g == bk or g == 0;  ht[g]++.  At the flush, per
// threshold i and class c:
//   P[i][c>0] = sum_{b>i} hp[b][c]   P[i][0] = sum_{b<=i} sum_c hp[b][c]   TP[i][c>0] = sum_{b>i} hq[b][c]
//   TP[i][0] = sum_{b<=i} hq[b][0]   T[i][c] = ht[c]
struct EvalBins {
  int hp[(EVAL_MAXT + 1) * EVAL_MAXK], hq[(EVAL_MAXT + 1) * EVAL_MAXK], ht[EVAL_MAXK], hrow[EVAL_MAXT + 1];
  float st[EVAL_MAXT];

  // zero the histograms and load the nt <= EVAL_MAXT thresholds; the caller synchronises before the first bin() / add()
  __device__ __forceinline__ void init(const float* thr, int nt, int K) {
    for (int i = threadIdx.x; i < (nt + 1) * K; i += 256) { hp[i] = 0; hq[i] = 0; }
    if (threadIdx.x < K) ht[threadIdx.x] = 0;
    if (threadIdx.x < nt) st[threadIdx.x] = thr[threadIdx.x];
  }

  // #{t_i < best}: a tie best == t stays background, a NaN lies in bin 0
  __device__ __forceinline__ int bin(float best, int nt) const {
    int b = 0;
    for (int t = 0; t < nt; ++t) b += (st[t] < best) ? 1 : 0;
    return b;
  }

  // One pixel (g != 255) whose winner bk, a class in 1..K-1, lies in bin b.  In bin 0 the pixel is background at every threshold,
  // whoever led, so it is counted under class 0: bin 0 is only ever read through class 0 (P[i][0] and TP[i][0] above), and because a
  // kept channel is never class 0, hp[b][0] is empty in every other bin - which is why hrow may sum a row from class 0 and why
  // hq[b][0] is free for the "predict 0 and gt 0" side of every bin.  A caller that left its winner in place in bin 0 and summed
  // hrow from class 1 got the same integers.  bk >= K (a key the host wrappers refuse) is dropped, never written.
  __device__ __forceinline__ void add(int b, int bk, int g, int K) {
    if (b == 0) bk = 0;
    if (bk < K) atomicAdd(&hp[b * K + bk], 1);
    if (g < K) {
      atomicAdd(&ht[g], 1);
      if (g == bk || g == 0) atomicAdd(&hq[b * K + g], 1);
    }
  }

  // the prefix sums into counts[nt][K][3]; every thread of the workgroup calls it
  __device__ __forceinline__ void flush(int nt, int K, long long* counts) {
    __syncthreads();
    for (int b = threadIdx.x; b <= nt; b += 256) {           // pixels per bin, any winner
      int s = 0;
      for (int c = 0; c < K; ++c) s += hp[b * K + c];
      hrow[b] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nt * K; i += 256) {
      const int t = i / K, c = i % K;
      int P = 0, TP = 0;
      if (c == 0) {
        for (int b = 0; b <= t; ++b) { P += hrow[b]; TP += hq[b * K]; }
      } else {
        for (int b = t + 1; b <= nt; ++b) { P += hp[b * K + c]; TP += hq[b * K + c]; }
      }
      eval_flush_entry(counts + (long)i * 3, TP, P, ht[c]);
    }
  }
};
