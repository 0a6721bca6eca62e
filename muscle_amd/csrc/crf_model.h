// The per-pixel arithmetic of the dense CRFs (include/muscle_hip.h states the models), shared by the windowed kernels (crf.hip)
// and the lattice ones (lattice.hip): one definition of each unary, of the label maps, of the softmax with its argmax and of
// the IR-label combination, so the two backends differ in how they evaluate the pairwise sums and in nothing else.
#pragma once
#include "common.h"
#include <math.h>

// probability unary: U = -log(clip(confidence * p + base, 1e-5, 1)), base = (1 - confidence) / L
__device__ __forceinline__ float crf_prob_unary(float confidence, float p, float base) {
  const float c = fminf(fmaxf(confidence * p + base, 1e-5f), 1.0f);
  return -logf(c);
}

// label unary, unary_from_labels(zero_unsure=False): -log(gt_prob) at the pixel's own label, -log((1 - gt_prob) / (L - 1)) elsewhere
struct CrfLabelU { float own, oth; };
inline CrfLabelU crf_label_unary(float gt_prob, int L) {
  CrfLabelU u;
  u.own = -logf(gt_prob); u.oth = -logf((1.0f - gt_prob) / (float)(L - 1));
  return u;
}

// softmax of the two-valued row -U (L-1 equal entries and the own one): the two numerators, and 1 / sum for a pixel whose own
// label is `own` (255: no own column)
struct CrfLabelE { float own, oth; };
__device__ __forceinline__ CrfLabelE crf_label_exp(float u_own, float u_oth) {
  const float m = fmaxf(-u_own, -u_oth);
  CrfLabelE e;
  e.own = expf(-u_own - m); e.oth = expf(-u_oth - m);
  return e;
}
__device__ __forceinline__ float crf_label_inv(CrfLabelE e, int own, int L) {
  float s = 0.f;
  for (int l = 0; l < L; ++l) s += (l == own) ? e.own : e.oth;
  return 1.0f / s;
}

// the two thresholded argmax maps of pixel i over [threshold, cams...] (first maximum wins: a CAM value equal to the threshold
// is background); cams [C][HW]
__device__ __forceinline__ void crf_cam_labels(const float* cams, int C, int HW, int i, float fg_thres, float bg_thres, int& lf, int& lb) {
  float bf = fg_thres, bb = bg_thres;
  lf = 0; lb = 0;
  for (int c = 0; c < C; ++c) {
    const float v = cams[(long)c * HW + i];
    if (v > bf) { bf = v; lf = c + 1; }
    if (v > bb) { bb = v; lb = c + 1; }
  }
}

// a given label: values outside 0..L-1 have no own column
__device__ __forceinline__ int crf_in_label(int v, int L) { return (v >= 0 && v < L) ? v : 255; }

// softmax over d[0..L-1] (stride 1) in place; returns the index of the first maximum of the RESULT
__device__ __forceinline__ int crf_softmax_row(float* d, int L) {
  float m = d[0];
  for (int l = 1; l < L; ++l) m = fmaxf(m, d[l]);
  float s = 0.f;
  for (int l = 0; l < L; ++l) { const float e = expf(d[l] - m); d[l] = e; s += e; }
  const float inv = 1.0f / s;
  int best = 0; float bv = -1.f;
  for (int l = 0; l < L; ++l) {
    const float q = d[l] * inv;
    d[l] = q;
    if (q > bv) { bv = q; best = l; }
  }
  return best;
}

// the three-line combination of cam_to_ir_label
__device__ __forceinline__ unsigned char crf_combine(int fg_conf, int bg_conf) {
  int c = fg_conf;
  if (fg_conf == 0) c = 255;
  if (bg_conf + fg_conf == 0) c = 0;
  return (unsigned char)c;
}
