// Input stage of the decoder-training loop (reference: src/data.py:93-123, src/imutils.py:35-53, :80-118, :283-292, :383-388):
// what VOC12SegDataset.__getitem__ does per item on the host - skimage.transform.resize of the [H,W,21] soft label (a Gaussian
// anti-alias filter + a bilinear warp over the WHOLE rescaled label in float64), RandomCropWithMask's zero container,
// RandomHorizontalFlipWithMask, HWC -> CHW - as one batched kernel that computes the resized label only inside the crop
// window.  (The image half of the same transforms is mx_input_stage, csrc/input.hip.)
//
// The resize is separable and linear: per axis the host folds `bilinear o gaussian` (both with ndimage's 'mirror' boundary)
// into one row of K = 2 + 2 * radius weights per output coordinate (muscle_amd/segdata.py:mask_axis_table), so
//   out[c, y, x] = sum_i wy[y][i] * sum_j wx[x][j] * src[sy[y] + i, sx[x] + j, c].
// The source is channel-last (a 42-byte pixel for 21 float16 channels) and the output channel-first: a workgroup takes 64
// output pixels of one output row, runs the vertical pass over the contiguous run of source pixels they need (whole pixel
// rows, consecutive lanes on consecutive elements) into LDS, and the horizontal pass reads LDS pixel-major and writes 64
// consecutive floats per channel.  fp32 accumulation in a fixed order, no atomics: the same bits every run.
#include "common.h"
#include <hip/hip_fp16.h>

// src_off: byte offset of the shipped source rows [sh, sw, C] (float16, or float32 when f32 != 0); the crop window
// [ch, cw] of the resized label goes to (top, left) of the [S, S] container, mirrored along X when flip != 0;
// ty_off / tx_off (int32 words into tabs): start[n] (first source row / column of each window row / column, relative to
// the shipped rows) followed by n * k float32 weights.
struct MaskJob { int src_off, sh, sw, f32, top, left, ch, cw, flip, ky, kx, ty_off, tx_off, pad0, pad1, pad2; };

__device__ __forceinline__ float mask_ld(const unsigned char* base, long i, int f32) {
  return f32 ? ((const float*)base)[i] : __half2float(((const __half*)base)[i]);
}

__global__ __launch_bounds__(256) void mask_stage_kernel(const unsigned char* __restrict__ src, const MaskJob* __restrict__ jobs,
                                                         const int* __restrict__ tabs, float* __restrict__ dst, int C, int S,
                                                         int span_cap) {
  extern __shared__ float v[];                              // [span][C | 1]: the vertically filtered source pixels of this tile
  const MaskJob jb = jobs[blockIdx.z];
  const int y = blockIdx.y, x0 = blockIdx.x * 64, tid = threadIdx.x;
  const int stride = C | 1;
  const long plane = (long)S * S;
  float* out = dst + (long)blockIdx.z * C * plane + (long)y * S;
  const int ty = y - jb.top;
  const int xa = max(x0, jb.left), xb = min(min(x0 + 64, S), jb.left + jb.cw);       // window columns inside this tile
  const bool live = ty >= 0 && ty < jb.ch && xa < xb;       // uniform over the workgroup
  const int* sx = tabs + jb.tx_off;
  int span0 = 0, span = 0;
  if (live) {
    span0 = min(max(sx[xa - jb.left], 0), jb.sw);
    const int span1 = min(max(sx[xb - 1 - jb.left] + jb.kx, span0), jb.sw);
    span = min(span1 - span0, span_cap);
    const int* sy = tabs + jb.ty_off;
    const float* wy = (const float*)(sy + jb.ch) + (long)ty * jb.ky;
    const int ys = sy[ty];
    const unsigned char* base = src + jb.src_off;
    for (int e = tid; e < span * C; e += 256) {
      float acc = 0.f;
      for (int i = 0; i < jb.ky; ++i) {
        const int r = min(max(ys + i, 0), jb.sh - 1);
        acc += wy[i] * mask_ld(base, ((long)r * jb.sw + span0) * C + e, jb.f32);
      }
      const int px = e / C;
      v[px * stride + (e - px * C)] = acc;
    }
    __syncthreads();
  }
  const int xo = x0 + (tid & 63);
  if (xo >= S) return;
  const int xw = jb.flip ? S - 1 - xo : xo;                 // np.fliplr of the CONTAINER (src/imutils.py:289-290)
  const int tx = xo - jb.left;
  const bool in = live && tx >= 0 && tx < jb.cw;
  int rel = 0;
  const float* wx = nullptr;
  if (in) {
    rel = sx[tx] - span0;
    wx = (const float*)(sx + jb.cw) + (long)tx * jb.kx;
  }
  for (int c = tid >> 6; c < C; c += 4) {
    float acc = 0.f;                                        // RandomCropWithMask's container is zero outside the window
    if (in)
      for (int j = 0; j < jb.kx; ++j) {
        const int p = rel + j;
        if (p >= 0 && p < span) acc += wx[j] * v[p * stride + c];
      }
    out[c * plane + xw] = acc;
  }
}

// The same stage for a hard label map (mask_type="label"): a NEAREST resize is a gather, so the whole stage is
//   dst[n, y, x] = inside the window ? src[ys[y - top]][xs[xc - left]] : fill,   xc = flip ? S-1-x : x (fliplr of the container).
// A thread owns four neighbouring output bytes of one row: it gathers them with byte loads (the shipped rows start at any byte
// offset and sw is usually odd) and writes them as ONE 32-bit store where the four lie inside the row and the address is
// aligned, as single bytes otherwise (a row tail, S % 4 != 0).  64 lanes cover 256 consecutive output bytes and read runs of
// neighbouring source bytes of one source row.  Every output byte has exactly one writer.
struct LabelJob { int src_off, sh, sw, top, left, ch, cw, flip, ty_off, tx_off, pad[6]; };

__global__ __launch_bounds__(256) void label_stage_kernel(const unsigned char* __restrict__ src, const LabelJob* __restrict__ jobs,
                                                          const int* __restrict__ tabs, unsigned char* __restrict__ dst, int S, int fill) {
  const LabelJob jb = jobs[blockIdx.z];
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6), x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;      // a wave per output row
  if (y >= S || x0 >= S) return;
  const int ty = y - jb.top;
  const bool row_in = ty >= 0 && ty < jb.ch && jb.sh > 0 && jb.sw > 0;
  const unsigned char* row = nullptr;
  if (row_in) row = src + jb.src_off + (long)min(max(tabs[jb.ty_off + ty], 0), jb.sh - 1) * jb.sw;
  const int* xs = tabs + jb.tx_off;
  unsigned v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + j;
    const int tx = (jb.flip ? S - 1 - x : x) - jb.left;
    v[j] = (unsigned)fill;
    if (row_in && x < S && tx >= 0 && tx < jb.cw) v[j] = row[min(max(xs[tx], 0), jb.sw - 1)];
  }
  unsigned char* o = dst + ((long)blockIdx.z * S + y) * S + x0;
  if (x0 + 4 <= S && ((uintptr_t)o & 3) == 0) {
    *reinterpret_cast<unsigned*>(o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  } else {
    for (int j = 0; j < 4 && x0 + j < S; ++j) o[j] = (unsigned char)v[j];
  }
}

extern "C" {

int mx_label_stage(const unsigned char* src, const int* jobs, const int* tabs, unsigned char* dst, int n, int S, int fill, void* stream) {
  MX_CHECK_ARG(src && jobs && tabs && dst, "label_stage: null pointer");
  MX_CHECK_ARG(n > 0 && n <= 65535 && S > 0 && S <= 65535 && fill >= 0 && fill <= 255, "label_stage: bad extents n=%d S=%d fill=%d", n, S, fill);
  hipLaunchKernelGGL(label_stage_kernel, dim3(cdiv(S, 256), cdiv(S, 4), n), dim3(256), 0, (hipStream_t)stream, src, (const LabelJob*)jobs, tabs,
                     dst, S, fill);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_mask_stage(const void* src, const int* jobs, const int* tabs, float* dst, int n, int C, int S, int span_cap, void* stream) {
  MX_CHECK_ARG(src && jobs && tabs && dst, "mask_stage: null pointer");
  MX_CHECK_ARG(n > 0 && n <= 65535 && C > 0 && S > 0 && S <= 65535, "mask_stage: bad extents n=%d C=%d S=%d", n, C, S);
  const long lds = (long)span_cap * (C | 1) * 4;
  MX_CHECK_ARG(span_cap > 0 && lds <= 65536, "mask_stage: span_cap=%d x C=%d does not fit 64 KiB of LDS (a stronger downscale than the stage is built for)",
               span_cap, C);
  hipLaunchKernelGGL(mask_stage_kernel, dim3(cdiv(S, 64), S, n), dim3(256), (size_t)lds, (hipStream_t)stream, (const unsigned char*)src,
                     (const MaskJob*)jobs, tabs, dst, C, S, span_cap);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
