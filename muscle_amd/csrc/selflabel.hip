// Class-balanced self-training labels (muscle_amd/selflabel.py): the confidence code of a probability map, its per-class
// histograms, and the selection of the most confident portion of every predicted class (CBST, Zou et al., ECCV 2018).
//
// The rule (DESIGN.md "Self-training labels"; include/muscle_hip.h states it for the entry points).  Per pixel of prob fp32 [K,H,W]:
//   label  best = prob[0], label = 0;  for c = 1..K-1: if (prob[c] > best) { best = prob[c]; label = c; }   - the first maximum, as
//          np.argmax on finite data; a NaN in prob[0] is never displaced, a NaN in another channel never wins
//   conf   = best
//   code   uint8, a logarithmic code of the uncertainty u = 1.0f - conf (ONE fp32 subtraction):
//            conf is NaN            -> 255  (never selected)
//            u <= 0  (conf >= 1)    -> 0
//            otherwise              -> clamp((bits(u) >> 20) - 823, 1, 193)
//          bits(u) >> 20 = the sign, the 8 exponent bits and the top 3 mantissa bits: u = 2^-24 (the smallest uncertainty a conf < 1 can
//          give) is code 1, u in [0.5, 1) is 185..192, u >= 1 is 193.  A lower code is more confident; 194..254 are unused.
// A pure function of fp32 bits: the device and numpy agree exactly.
//
// The tables hist / val / hit int64 [K][256] are counted per workgroup (256 threads) in LDS and flushed with one 64-bit integer atomic per
// non-zero entry, as csrc/eval_counts.h does: exact, the same integers every run, no floating-point atomics.  Only 195 codes occur (0..193
// and 255), so the LDS table of a class has 195 slots, 255 (and any stored code above 193) in the last: three tables of [24][195] int32 are
// 56160 bytes.  The LDS is sized by the launch: K * 195 ints per table, one table without gt.
#include "common.h"

#define CONF_MAXK 24
#define CONF_SLOTS 195          // codes 0..193, and slot 194 for code 255
#define CONF_TOP 193

__device__ __forceinline__ unsigned conf_code_of(float conf) {
#pragma clang fp contract(off)
  if (conf != conf) return 255u;
  const float u = 1.0f - conf;
  if (!(u > 0.f)) return 0u;
  const int c = (int)(__float_as_uint(u) >> 20) - 823;
  return (unsigned)min(max(c, 1), CONF_TOP);
}

// One pixel (lb < K) with code cd and ground truth g into the LDS tables [nt][K][CONF_SLOTS]: hist always; with GT val where g != 255 and
// hit where g == lb.  Shared by conf_code_kernel and code_hist_kernel.
template <bool GT>
__device__ __forceinline__ void conf_count(int* tab, int K, int lb, unsigned cd, int g) {
  const int s = lb * CONF_SLOTS + (int)min(cd, (unsigned)(CONF_SLOTS - 1));
  atomicAdd(&tab[s], 1);
  if (GT) {
    if (g != 255) atomicAdd(&tab[K * CONF_SLOTS + s], 1);
    if (g == lb) atomicAdd(&tab[2 * K * CONF_SLOTS + s], 1);
  }
}

__device__ __forceinline__ void conf_zero(int* tab, int n) {
  for (int i = threadIdx.x; i < n; i += 256) tab[i] = 0;
  __syncthreads();
}

// LDS [nt][K][CONF_SLOTS] -> the global tables [K][256] (every thread of the workgroup calls it)
__device__ __forceinline__ void conf_flush(const int* tab, int K, int nt, long long* hist, long long* val, long long* hit) {
  __syncthreads();
  const int per = K * CONF_SLOTS;
  for (int i = threadIdx.x; i < nt * per; i += 256) {
    const int v = tab[i];
    if (!v) continue;
    const int t = i / per, r = i - t * per, c = r / CONF_SLOTS, s = r - c * CONF_SLOTS;
    long long* dst = t == 0 ? hist : (t == 1 ? val : hit);
    atomicAdd((unsigned long long*)&dst[c * 256 + (s == CONF_SLOTS - 1 ? 255 : s)], (unsigned long long)v);
  }
}

template <bool GT>
__global__ __launch_bounds__(256) void conf_code_kernel(const float* __restrict__ prob, int K, long n, unsigned char* __restrict__ label,
                                                        unsigned char* __restrict__ code, const unsigned char* __restrict__ gt,
                                                        long long* hist, long long* val, long long* hit) {
  extern __shared__ int tab[];
  const int nt = GT ? 3 : 1;
  conf_zero(tab, nt * K * CONF_SLOTS);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float* p = prob + i;                           // lanes walk X: every channel row is read in coalesced runs
    float best = p[0];
    int lb = 0;
#pragma unroll 4
    for (int c = 1; c < K; ++c) {
      const float v = p[(long)c * n];
      if (v > best) { best = v; lb = c; }
    }
    const unsigned cd = conf_code_of(best);
    label[i] = (unsigned char)lb;
    code[i] = (unsigned char)cd;
    conf_count<GT>(tab, K, lb, cd, GT ? (int)gt[i] : 255);
  }
  conf_flush(tab, K, nt, hist, val, hit);
}

template <bool GT>
__global__ __launch_bounds__(256) void code_hist_kernel(const unsigned char* __restrict__ label, const unsigned char* __restrict__ code,
                                                        const unsigned char* __restrict__ gt, long n, int K, long long* hist, long long* val,
                                                        long long* hit) {
  extern __shared__ int tab[];
  const int nt = GT ? 3 : 1;
  conf_zero(tab, nt * K * CONF_SLOTS);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int lb = label[i];
    if (lb < K) conf_count<GT>(tab, K, lb, code[i], GT ? (int)gt[i] : 255);      // a label >= K is counted nowhere, never an index
  }
  conf_flush(tab, K, nt, hist, val, hit);
}

// out = the label where its code is within its class's threshold, else 255; kept[c] += (kept, total).  The per-class sums are taken per
// wave with ballots (lane c keeps class c), then per workgroup in LDS, then one 64-bit integer atomic per non-zero entry.
__global__ __launch_bounds__(256) void conf_select_kernel(const unsigned char* __restrict__ label, const unsigned char* __restrict__ code,
                                                          const unsigned char* __restrict__ tcode, long n, int K,
                                                          unsigned char* __restrict__ out, long long* kept) {
  __shared__ int tab[CONF_MAXK * 2];
  __shared__ int thr[CONF_MAXK];
  if (threadIdx.x < CONF_MAXK * 2) tab[threadIdx.x] = 0;
  if (threadIdx.x < K) thr[threadIdx.x] = tcode[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  int nk = 0, na = 0;
  const long step = (long)gridDim.x * 256;
  for (long i0 = (long)blockIdx.x * 256; i0 < n; i0 += step) {                   // wave-uniform trip count: the ballots see every lane
    const long i = i0 + threadIdx.x;
    int lb = 255;
    bool keep = false;
    if (i < n) {
      lb = label[i];
      keep = lb < K && (int)code[i] <= thr[min(lb, K - 1)];
      out[i] = keep ? (unsigned char)lb : (unsigned char)255;
    }
    for (int c = 0; c < K; ++c) {
      const unsigned long long ma = __ballot(lb == c), mk = __ballot(lb == c && keep);
      if (lane == c) { na += __popcll(ma); nk += __popcll(mk); }
    }
  }
  if (lane < K) {
    if (nk) atomicAdd(&tab[lane * 2], nk);
    if (na) atomicAdd(&tab[lane * 2 + 1], na);
  }
  __syncthreads();
  if (threadIdx.x < K * 2 && tab[threadIdx.x])
    atomicAdd((unsigned long long*)&kept[threadIdx.x], (unsigned long long)tab[threadIdx.x]);
}

// two pixels per thread up to 2048 workgroups, a grid-stride loop beyond: a workgroup zeroes and flushes up to 3 * K * 195 LDS words
static int conf_grid(long n) {
  const long g = (n + 511) / 512;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

extern "C" {

int mx_conf_code(const float* prob, int K, int H, int W, unsigned char* label, unsigned char* code, const unsigned char* gt,
                 long long* hist, long long* val, long long* hit, void* stream) {
  MX_CHECK_ARG(prob && label && code && hist, "conf_code: null pointer");
  MX_CHECK_ARG((gt != nullptr) == (val != nullptr) && (gt != nullptr) == (hit != nullptr), "conf_code: gt, val and hit come together or not at all");
  MX_CHECK_ARG(K >= 1 && K <= CONF_MAXK, "conf_code: K=%d outside 1..%d", K, CONF_MAXK);
  MX_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W < (1L << 31), "conf_code: H=%d W=%d (H*W must lie in 1..2^31-1)", H, W);
  const long n = (long)H * W;
  const size_t lds = (size_t)(gt ? 3 : 1) * K * CONF_SLOTS * sizeof(int);
  if (gt)
    hipLaunchKernelGGL(conf_code_kernel<true>, dim3(conf_grid(n)), dim3(256), lds, (hipStream_t)stream, prob, K, n, label, code, gt, hist, val, hit);
  else
    hipLaunchKernelGGL(conf_code_kernel<false>, dim3(conf_grid(n)), dim3(256), lds, (hipStream_t)stream, prob, K, n, label, code, gt, hist, val, hit);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_code_hist(const unsigned char* label, const unsigned char* code, const unsigned char* gt, long n, int K, long long* hist,
                 long long* val, long long* hit, void* stream) {
  MX_CHECK_ARG(label && code && hist, "code_hist: null pointer");
  MX_CHECK_ARG((gt != nullptr) == (val != nullptr) && (gt != nullptr) == (hit != nullptr), "code_hist: gt, val and hit come together or not at all");
  MX_CHECK_ARG(K >= 1 && K <= CONF_MAXK, "code_hist: K=%d outside 1..%d", K, CONF_MAXK);
  MX_CHECK_ARG(n >= 1 && n < (1L << 31), "code_hist: n=%ld outside 1..2^31-1", n);
  const size_t lds = (size_t)(gt ? 3 : 1) * K * CONF_SLOTS * sizeof(int);
  if (gt)
    hipLaunchKernelGGL(code_hist_kernel<true>, dim3(conf_grid(n)), dim3(256), lds, (hipStream_t)stream, label, code, gt, n, K, hist, val, hit);
  else
    hipLaunchKernelGGL(code_hist_kernel<false>, dim3(conf_grid(n)), dim3(256), lds, (hipStream_t)stream, label, code, gt, n, K, hist, val, hit);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_conf_select(const unsigned char* label, const unsigned char* code, const unsigned char* tcode, long n, int K, unsigned char* out,
                   long long* kept, void* stream) {
  MX_CHECK_ARG(label && code && tcode && out && kept, "conf_select: null pointer");
  MX_CHECK_ARG(K >= 1 && K <= CONF_MAXK, "conf_select: K=%d outside 1..%d", K, CONF_MAXK);
  MX_CHECK_ARG(n >= 1 && n < (1L << 31), "conf_select: n=%ld outside 1..2^31-1", n);
  hipLaunchKernelGGL(conf_select_kernel, dim3(conf_grid(n)), dim3(256), 0, (hipStream_t)stream, label, code, tcode, n, K, out, kept);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
