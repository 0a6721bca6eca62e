// Input stage of IRN training (reference: VOC12AffinityDataset.__getitem__, src/data.py:659-705; TorchvisionNormalize
// src/data.py:596-609; random_lr_flip / random_crop / pil_rescale of src/imutils.py): what a DataLoader worker does per item
// after the bicubic rescale - normalise in float64, flip, paste into the [S,S] containers (fill 0 / 255), HWC -> CHW, reduce
// the label container by 0.25 with NEAREST - as ONE launch per batch that writes both tensors `irn_step` takes.
//
// The image half is store-bound (12 fp32 bytes written per source byte): a thread owns 4 neighbouring output pixels, reads
// their 12 source bytes once and writes one 16-byte store into each of the three channel planes.  (u8 / 255 - mean) / std
// depends on the byte and the channel only, so every workgroup evaluates the fp64 expression once per (channel, byte) into
// a 3 KB LDS table and the pixels look their fp32 value up: the same bits as evaluating it per pixel, without 6 fp64
// divisions per pixel.  Window edges and the flip are resolved per element; there is no tail launch.
// The label half never forms the rescaled label or its container: output (Y, X) is container pixel (4Y+2, 4X+2) (Pillow's
// NEAREST at scale exactly 1/4), which is either outside the window (255) or one byte of the ORIGINAL label, found through
// the two NEAREST index tables of the rescale.  A thread writes 4 label bytes as one 32-bit store.
#include "common.h"

struct IrnInputJob {
  int img_off, sh, sw, img_top, img_left, cont_top, cont_left, ch, cw, flip, lab_off, lh, lw, ytab_off, xtab_off, pad;
};

__global__ __launch_bounds__(256) void irn_input_stage_kernel(const unsigned char* __restrict__ src, const IrnInputJob* __restrict__ jobs,
                                                              const int* __restrict__ tabs, float* __restrict__ img,
                                                              unsigned char* __restrict__ label, int S) {
  __shared__ float lut[3][256];
  {
    const double mean[3] = {0.485, 0.456, 0.406}, stdv[3] = {0.229, 0.224, 0.225};
    const int v = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c][v] = (float)(((double)v / 255.0 - mean[c]) / stdv[c]);   // src/data.py:603-607
  }
  __syncthreads();
  const IrnInputJob jb = jobs[blockIdx.y];
  const int S4 = S >> 2;
  const long plane = (long)S * S;
  const int img_quads = S * S4;                             // 4 pixels each; S <= 16384 keeps this inside an int
  const int lab_quads = label ? S4 * (S4 >> 2) : 0;         // 4 label bytes each (S % 16 == 0)
  float* out = img + (long)blockIdx.y * 3 * plane;
  const unsigned char* im = src + jb.img_off;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < img_quads + lab_quads; q += gridDim.x * 256) {
    if (q < img_quads) {
      const int y = q / S4, x0 = (q - y * S4) << 2;
      const int wy = y - jb.cont_top, wx0 = x0 - jb.cont_left;
      float4 r = {0.f, 0.f, 0.f, 0.f}, g = r, b = r;        // random_crop's container is zero outside the window
      if (wy >= 0 && wy < jb.ch && wx0 > -4 && wx0 < jb.cw) {
        const unsigned char* row = im + (long)(jb.img_top + wy) * jb.sw * 3;
        float* rp = &r.x; float* gp = &g.x; float* bp = &b.x;
        if (wx0 >= 0 && wx0 + 4 <= jb.cw) {                 // whole quad inside the window: its 12 source bytes are contiguous
          const int fx = jb.img_left + wx0;                 // leftmost column in the (flipped) rescaled image
          unsigned char px[12];
          __builtin_memcpy(px, row + (jb.flip ? jb.sw - 4 - fx : fx) * 3, 12);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int s = jb.flip ? 3 - e : e;
            rp[e] = lut[0][px[3 * s]]; gp[e] = lut[1][px[3 * s + 1]]; bp[e] = lut[2][px[3 * s + 2]];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int wx = wx0 + e;
            if (wx >= 0 && wx < jb.cw) {
              const int fx = jb.img_left + wx;
              const unsigned char* px = row + (jb.flip ? jb.sw - 1 - fx : fx) * 3;
              rp[e] = lut[0][px[0]]; gp[e] = lut[1][px[1]]; bp[e] = lut[2][px[2]];
            }
          }
        }
      }
      float* o = out + (long)y * S + x0;
      st4(o, r); st4(o + plane, g); st4(o + 2 * plane, b);
    } else {
      const int l = q - img_quads;
      const int Y = l / (S4 >> 2), X0 = (l - Y * (S4 >> 2)) << 2;
      const int wy = 4 * Y + 2 - jb.cont_top;
      unsigned v = 0xFFFFFFFFu;                             // the label container's fill is 255
      if (jb.lab_off >= 0 && wy >= 0 && wy < jb.ch) {
        const int sy = min(max(tabs[jb.ytab_off + jb.img_top + wy], 0), jb.lh - 1);
        const unsigned char* lrow = src + jb.lab_off + (long)sy * jb.lw;
        const int* xtab = tabs + jb.xtab_off;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int wx = 4 * (X0 + e) + 2 - jb.cont_left;
          if (wx >= 0 && wx < jb.cw) {
            const int fx = jb.img_left + wx;
            const int sx = min(max(xtab[jb.flip ? jb.sw - 1 - fx : fx], 0), jb.lw - 1);
            v = (v & ~(0xFFu << (8 * e))) | ((unsigned)lrow[sx] << (8 * e));
          }
        }
      }
      *reinterpret_cast<unsigned*>(label + (long)blockIdx.y * S4 * S4 + (long)Y * S4 + X0) = v;
    }
  }
}

extern "C" {

int mx_irn_input_stage(const unsigned char* src, const int* jobs, const int* tabs, float* img, unsigned char* label, int n, int S,
                       void* stream) {
  MX_CHECK_ARG(src && jobs && tabs && img, "irn_input_stage: null pointer");
  MX_CHECK_ARG(n > 0 && n <= 65535 && S > 0 && S <= 16384, "irn_input_stage: bad extents n=%d S=%d", n, S);
  MX_CHECK_ARG(S % 16 == 0, "irn_input_stage: S=%d is not a multiple of 16", S);
  MX_CHECK_ARG(((uintptr_t)img & 15) == 0 && ((uintptr_t)label & 3) == 0, "irn_input_stage: img must be 16-byte and label 4-byte aligned");
  const long quads = (long)S * (S / 4) + (label ? (long)(S / 4) * (S / 16) : 0);
  // 16 pixels per thread at the training shape; about 8 workgroups of 256 threads per CU for a batch of 32
  int bx = cdiv(quads, 256 * 4);
  const int cap = 2048 / n < 16 ? 16 : 2048 / n;
  if (bx > cap) bx = cap;
  hipLaunchKernelGGL(irn_input_stage_kernel, dim3(bx, n), dim3(256), 0, (hipStream_t)stream, src, (const IrnInputJob*)jobs, tabs, img,
                     label, S);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
