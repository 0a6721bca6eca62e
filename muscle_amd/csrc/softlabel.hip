// Expansion of the compact soft pseudo-label (muscle_amd/softlabel.py) into the rows of the dense float16 [H,W,channels]
// array `infer_irn.py:79-88` saves and `src/data.py:102` loads: channel 0 the background threshold, channel keys[i] + 1 the
// 4x bilinear upsample of the stored walk result rw_i divided by the global maximum, every other channel +0.
// The values come from irn_soft.h, the functions irn_label_kernel (irn.hip) writes the dense array with: the expansion is
// that array bit for bit.
//
// The output of one item is ONE contiguous run of rows * W * channels halves (a pixel is 42 bytes at 21 channels), walked
// flat: consecutive lanes take consecutive pairs of halves and store 32 bits each; a run of odd length ends in one lone
// half.  The low-resolution maps (<= 47 KB per class at 375 x 500) are re-read from cache; the channel -> stored map table
// sits in LDS.  No atomics: the same bits every run.
#include "common.h"
#include <hip/hip_fp16.h>
#include "irn_soft.h"

#define MX_SOFT_MAX_CHANNELS 256        // keys are uint8, so channel keys[i] + 1 <= 256 - 1 after the bound below

// byte offsets from the batch base; vmax / bg: float bits
struct SoftJob { int rw_off, keys_off, K, h, w, H, W, r0, rows, dst_off, channels, vmax, bg, pad0, pad1, pad2; };

// half e = (pixel p, channel c) of the run, as 16 bits
__device__ __forceinline__ unsigned soft_half_bits(const float* rw, const short* slot, const SoftJob& jb, unsigned p, int c, float vmax,
                                                   unsigned bg_bits) {
  if (c == 0) return bg_bits;
  const int s = slot[c];
  if (s < 0) return 0u;
  const unsigned y = p / (unsigned)jb.W, x = p - y * (unsigned)jb.W;
  return (unsigned)__half_as_ushort(irn_soft_half(irn_soft_value(rw + (long)s * jb.h * jb.w, jb.h, jb.w, jb.r0 + (int)y, (int)x, vmax)));
}

__global__ __launch_bounds__(256) void soft_expand_kernel(unsigned char* __restrict__ base, const SoftJob* __restrict__ jobs) {
  __shared__ short slot[MX_SOFT_MAX_CHANNELS];
  const SoftJob jb = jobs[blockIdx.z];
  const int C = min(jb.channels, MX_SOFT_MAX_CHANNELS);
  for (int c = threadIdx.x; c < MX_SOFT_MAX_CHANNELS; c += 256) slot[c] = -1;
  __syncthreads();
  const unsigned char* keys = base + jb.keys_off;
  for (int i = threadIdx.x; i < jb.K; i += 256) {           // keys ascend: every channel has at most one writer
    const int c = (int)keys[i] + 1;
    if (c < C) slot[c] = (short)i;
  }
  __syncthreads();
  const float* rw = (const float*)(base + jb.rw_off);
  const float vmax = __int_as_float(jb.vmax);
  const unsigned bg_bits = (unsigned)__half_as_ushort(irn_soft_half(__int_as_float(jb.bg)));
  const unsigned total = (unsigned)jb.rows * (unsigned)jb.W * (unsigned)C;      // halves; < 2^30 (int32 byte offsets)
  const unsigned pairs = total >> 1;
  unsigned* dst = (unsigned*)(base + jb.dst_off);
  for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < pairs; q += gridDim.x * 256u) {
    const unsigned e = 2u * q;
    const unsigned p0 = e / (unsigned)C;
    const int c0 = (int)(e - p0 * (unsigned)C);
    const bool wrap = c0 + 1 == C;                          // the pair straddles two pixels
    const unsigned lo = soft_half_bits(rw, slot, jb, p0, c0, vmax, bg_bits);
    const unsigned hi = soft_half_bits(rw, slot, jb, wrap ? p0 + 1u : p0, wrap ? 0 : c0 + 1, vmax, bg_bits);
    dst[q] = lo | (hi << 16);
  }
  if ((total & 1u) && blockIdx.x == 0 && threadIdx.x == 0) {           // the lone last half of an odd run
    const unsigned e = total - 1u;
    const unsigned p = e / (unsigned)C;
    ((unsigned short*)dst)[e] = (unsigned short)soft_half_bits(rw, slot, jb, p, (int)(e - p * (unsigned)C), vmax, bg_bits);
  }
}

extern "C" {

int mx_soft_expand(void* base, const int* jobs, int n, void* stream) {
  MX_CHECK_ARG(base && jobs, "soft_expand: null pointer");
  MX_CHECK_ARG(n > 0 && n <= 65535, "soft_expand: n=%d outside 1..65535", n);
  hipLaunchKernelGGL(soft_expand_kernel, dim3(512, 1, n), dim3(256), 0, (hipStream_t)stream, (unsigned char*)base, (const SoftJob*)jobs);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
