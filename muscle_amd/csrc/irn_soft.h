// The value arithmetic of the soft pseudo-label (infer_irn.py:78-88), shared by the kernel that writes the dense label
// (irn_label_kernel, irn.hip) and the kernel that re-creates its rows from the compact form (soft_expand_kernel,
// softlabel.hip): one definition, so the two paths cannot drift apart.
#pragma once
#include "common.h"
#include <hip/hip_fp16.h>

// rw_up = interpolate(rw, x4, bilinear, align_corners=False)[:, :H, :W] at (Y, X) of one map m [h,w]: the four taps and the
// two weights.  (The coordinate is exact in fp32 whether or not the multiply-add is fused: a scaling by 1/4.)
struct IrnUp4 { int i00, i01, i10, i11; float wy, wx; };
__device__ __forceinline__ IrnUp4 irn_up4_taps(int h, int w, int Y, int X) {
  float sy = ((float)Y + 0.5f) * 0.25f - 0.5f, sx = ((float)X + 0.5f) * 0.25f - 0.5f;
  if (sy < 0.f) sy = 0.f;
  if (sx < 0.f) sx = 0.f;
  int y0 = (int)sy, x0 = (int)sx;
  if (y0 > h - 1) y0 = h - 1;
  if (x0 > w - 1) x0 = w - 1;
  const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
  IrnUp4 t;
  t.i00 = y0 * w + x0; t.i01 = y0 * w + x1; t.i10 = y1 * w + x0; t.i11 = y1 * w + x1;
  t.wy = sy - y0; t.wx = sx - x0;
  return t;
}
// The blend (1-wy) * ((1-wx) * m00 + wx * m01) + wy * ((1-wx) * m10 + wx * m11), operation for operation as irn_label_kernel
// has always executed it: rows fma(1-wx, m.0, rn(wx * m.1)), then fma(1-wy, row0, rn(wy * row1)).  hipcc contracts the plain
// expression per kernel (and per loop), so a second kernel written with it rounds differently; here every step is spelt out
// with contraction off (common.h: lerp_b) and any kernel that includes this reproduces the label kernel's bits.
__device__ __forceinline__ float irn_up4(const float* m, int h, int w, int Y, int X) {
  const IrnUp4 t = irn_up4_taps(h, w, Y, X);
  return lerp_b(lerp_b(m[t.i00], m[t.i01], t.wx), lerp_b(m[t.i10], m[t.i11], t.wx), t.wy);
}

// rw_up / max(rw_up): the fp32 value the arg-max compares and the soft label stores
__device__ __forceinline__ float irn_soft_value(const float* m, int h, int w, int Y, int X, float mx) {
  return irn_up4(m, h, w, Y, X) / mx;
}

// .astype(np.float16) of infer_irn.py:88 (and of the threshold plane in front)
__device__ __forceinline__ __half irn_soft_half(float v) { return __float2half_rn(v); }
