// Lovasz-softmax loss (muscle_amd/lovasz.py) on a segmented, stable, deterministic LSD radix sort.  include/muscle_hip.h states the
// model (mx_lovasz_ws ..); DESIGN.md "Lovasz-softmax loss" gives the structure, the bytes moved and the workspace.
//
// Stages:
//   1  lv_errors_kernel     seg, label -> err fp32 [S,P], flag uint8 [S,P]; the K logits of a pixel live in registers, lanes walk HW
//   2  4 digit passes of    lv_hist_kernel (per-block digit counts, LDS integer atomics: counts do not depend on order)
//                           lv_scan_kernel (exclusive scan over (digit, block) of a segment: one workgroup per segment)
//                           lv_scatter_kernel (stable: a wave ranks 64 consecutive elements with ballots, its rounds and the four
//                                              waves of a workgroup follow in element order through LDS counters)
//      on (key, j) pairs; the first pass forms the keys from err / flag on the fly, j is implicit there
//   3  lv_fgcount_kernel / lv_scan_kernel / lv_apply_kernel: the segmented scan of the foreground flag along the sorted order, the
//      closed-form increments in fp64 from the integer counts, coef_g and rank back to the original order, fp64 block partials of L
//      lv_segsum_kernel: the partials of a segment in a fixed order
//   4  lv_finish_kernel (class weighting, on the device) and lv_bwd_kernel (softmax adjoint with the stored coefficients)
// No workgroup waits for another; every launch is a plain grid.  A workgroup is 256 threads and owns a tile of 4096 consecutive elements
// of one segment: wave w the elements [1024 w, 1024 w + 1024) of the tile, in 16 rounds of 64.
#include "common.h"

#define LV_MAXK 24
#define LV_ITEMS 16
#define LV_SPAN (LV_ITEMS * 64)          // elements of one wave
#define LV_TILE (4 * LV_SPAN)            // elements of one workgroup
#define LV_ONE 0x3F800000u               // bits(1.0f)
#define LV_INVALID 0x40000000u           // the key of an ignored element: above every valid key
#define LV_PASSES 4

// the public key (lovasz.key_of mirrors it): ascending key = descending e; anything outside [0,1] sorts as e = 1
__device__ __forceinline__ unsigned lv_key_of(float e) {
  return (e >= 0.f && e <= 1.f) ? LV_ONE - (__float_as_uint(e) & 0x7FFFFFFFu) : 0u;
}
// inside the sort bit 31 carries the foreground flag of a valid element; no digit contains it
__device__ __forceinline__ unsigned lv_sort_key(float e, unsigned flag) {
  if (!(flag & 2u)) return LV_INVALID;
  return lv_key_of(e) | ((flag & 1u) << 31);
}
__device__ __forceinline__ unsigned lv_digit(unsigned key, int shift) { return ((key & 0x7FFFFFFFu) >> shift) & 255u; }

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- stage 1 and the backward: softmax of V consecutive pixels, K logits each, in registers ----------------------------------------
template <int V>
__device__ __forceinline__ void lv_softmax(const float* __restrict__ x, int K, long HW, float (&p)[LV_MAXK][V]) {
  float m[V], sum[V];
#pragma unroll
  for (int v = 0; v < V; ++v) { m[v] = -INFINITY; sum[v] = 0.f; }
#pragma unroll
  for (int c = 0; c < LV_MAXK; ++c)
    if (c < K) {
      if (V == 4) {
        const float4 t = ld4(x + (long)c * HW);
        p[c][0] = t.x; p[c][1 % V] = t.y; p[c][2 % V] = t.z; p[c][3 % V] = t.w;
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) p[c][v] = x[(long)c * HW + v];
      }
#pragma unroll
      for (int v = 0; v < V; ++v) m[v] = fmaxf(m[v], p[c][v]);
    }
#pragma unroll
  for (int c = 0; c < LV_MAXK; ++c)
    if (c < K) {
#pragma unroll
      for (int v = 0; v < V; ++v) { p[c][v] = __expf(p[c][v] - m[v]); sum[v] += p[c][v]; }
    }
#pragma unroll
  for (int c = 0; c < LV_MAXK; ++c)
    if (c < K) {
#pragma unroll
      for (int v = 0; v < V; ++v) p[c][v] = p[c][v] / sum[v];
    }
}

template <int V>
__global__ __launch_bounds__(256) void lv_errors_kernel(const float* __restrict__ seg, const unsigned char* __restrict__ label, int ignore,
                                                        int N, int K, long HW, int per_image, float* __restrict__ err,
                                                        unsigned char* __restrict__ flag) {
  const long pix = ((long)blockIdx.x * 256 + threadIdx.x) * V;
  if (pix >= (long)N * HW) return;
  const long n = pix / HW, hw = pix - n * HW;                  // V divides HW: the V pixels share n
  float p[LV_MAXK][V];
  lv_softmax<V>(seg + n * K * HW + hw, K, HW, p);
  int lb[V];
#pragma unroll
  for (int v = 0; v < V; ++v) lb[v] = label[pix + v];
  const long P = per_image ? HW : (long)N * HW;
  const size_t at0 = (size_t)(per_image ? n * K : 0) * (size_t)P + (size_t)(per_image ? hw : pix);
#pragma unroll
  for (int c = 0; c < LV_MAXK; ++c)
    if (c < K) {
      float e[V];
      unsigned char f[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const bool valid = lb[v] != ignore && lb[v] < K, fg = valid && lb[v] == c;
        e[v] = valid ? (fg ? 1.f - p[c][v] : p[c][v]) : 0.f;
        f[v] = (unsigned char)(valid ? (fg ? 3 : 2) : 0);
      }
      const size_t at = at0 + (size_t)c * (size_t)P;
      if (V == 4) {
        st4(err + at, make_float4(e[0], e[1 % V], e[2 % V], e[3 % V]));
        *reinterpret_cast<uchar4*>(flag + at) = make_uchar4(f[0], f[1 % V], f[2 % V], f[3 % V]);
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) { err[at + v] = e[v]; flag[at + v] = f[v]; }
      }
    }
}

__global__ __launch_bounds__(256) void lv_bwd_kernel(const float* __restrict__ seg, const unsigned char* __restrict__ label, int ignore,
                                                     const float* __restrict__ coef_g, const float* __restrict__ segw,
                                                     const float* __restrict__ gup, int N, int K, long HW, int per_image,
                                                     float* __restrict__ gseg) {
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (long)N * HW) return;
  const long n = pix / HW, hw = pix - n * HW;
  float* out = gseg + n * K * HW + hw;
  const int lb = label[pix];
  if (lb == ignore || lb >= K) {                               // ignored: exact zeros, nothing else is read
    for (int c = 0; c < K; ++c) out[(long)c * HW] = 0.f;
    return;
  }
  float p[LV_MAXK][1], cf[LV_MAXK];
  lv_softmax<1>(seg + n * K * HW + hw, K, HW, p);
  const long P = per_image ? HW : (long)N * HW;
  const int s0 = per_image ? (int)n * K : 0;
  const size_t at0 = (size_t)s0 * (size_t)P + (size_t)(per_image ? hw : pix);
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < LV_MAXK; ++c)
    if (c < K) {
      const float g = coef_g[at0 + (size_t)c * (size_t)P], w = segw[s0 + c], pc = p[c][0];
      const float sgn = (lb == c) ? (pc < 1.f ? -1.f : 0.f) : (pc > 0.f ? 1.f : 0.f);
      cf[c] = w * sgn * g;
      dot += cf[c] * pc;
    }
  const float gu = gup[0];
#pragma unroll
  for (int c = 0; c < LV_MAXK; ++c)
    if (c < K) out[(long)c * HW] = gu * p[c][0] * (cf[c] - dot);
}

// ---- stage 2: the digit passes -------------------------------------------------------------------------------------------------------
// hist[s][digit][block] = the count of the digit in the block's tile
template <bool FIRST>
__global__ __launch_bounds__(256) void lv_hist_kernel(const float* __restrict__ err, const unsigned char* __restrict__ flag,
                                                      const unsigned* __restrict__ kin, int shift, long P, int nblk,
                                                      unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  const int s = blockIdx.x / nblk, b = blockIdx.x - s * nblk;
  h[threadIdx.x] = 0u;
  __syncthreads();
  const size_t seg0 = (size_t)s * (size_t)P;
  const long t0 = (long)b * LV_TILE;
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long i = t0 + r * 256 + threadIdx.x;
    if (i < P) {
      const unsigned key = FIRST ? lv_sort_key(err[seg0 + i], flag[seg0 + i]) : kin[seg0 + i];
      atomicAdd(&h[lv_digit(key, shift)], 1u);
    }
  }
  __syncthreads();
  hist[((size_t)s * 256 + threadIdx.x) * (size_t)nblk + b] = h[threadIdx.x];
}

// in-place exclusive scan of n consecutive counts per segment (one workgroup each; 4096 per round - a round is one dependent trip to
// memory, and the table of a 3.2 M-element segment has 200 K entries - with a running carry)
#define LV_SCAN_E 16
__global__ __launch_bounds__(256) void lv_scan_kernel(unsigned* __restrict__ a, long n) {
  __shared__ unsigned wsum[4];
  unsigned* p = a + (size_t)blockIdx.x * (size_t)n;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned carry = 0u;
  for (long c0 = 0; c0 < n; c0 += 256 * LV_SCAN_E) {
    const long i0 = c0 + threadIdx.x * LV_SCAN_E;
    unsigned v[LV_SCAN_E];
    unsigned t = 0u;
#pragma unroll
    for (int k = 0; k < LV_SCAN_E; ++k) v[k] = 0u;
    const bool whole = (n & 3) == 0 && i0 + LV_SCAN_E <= n;          // a and n multiples of 16 bytes: 16-byte accesses
    if (whole) {
#pragma unroll
      for (int k = 0; k < LV_SCAN_E; k += 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(p + i0 + k);
        v[k] = q.x; v[k + 1] = q.y; v[k + 2] = q.z; v[k + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < LV_SCAN_E; ++k)
        if (i0 + k < n) v[k] = p[i0 + k];
    }
#pragma unroll
    for (int k = 0; k < LV_SCAN_E; ++k) t += v[k];
    unsigned inc = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned before = 0u, tot = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < w) before += wsum[k];
      tot += wsum[k];
    }
    unsigned ex = carry + before + inc - t;
#pragma unroll
    for (int k = 0; k < LV_SCAN_E; ++k) { const unsigned x = v[k]; v[k] = ex; ex += x; }
    if (whole) {
#pragma unroll
      for (int k = 0; k < LV_SCAN_E; k += 4) *reinterpret_cast<uint4*>(p + i0 + k) = make_uint4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    } else {
#pragma unroll
      for (int k = 0; k < LV_SCAN_E; ++k)
        if (i0 + k < n) p[i0 + k] = v[k];
    }
    carry += tot;
    __syncthreads();
  }
}

// hist holds the scanned table: the first position of (digit, block) inside the segment
template <bool FIRST>
__global__ __launch_bounds__(256) void lv_scatter_kernel(const float* __restrict__ err, const unsigned char* __restrict__ flag,
                                                         const unsigned* __restrict__ kin, const unsigned* __restrict__ iin, int shift,
                                                         long P, int nblk, const unsigned* __restrict__ hist, unsigned* __restrict__ kout,
                                                         unsigned* __restrict__ iout) {
  __shared__ unsigned wc[4][256];          // per wave: the digit counts of its rounds so far
  __shared__ unsigned base[4][256];        // per wave: the first position of its elements of a digit
  const int s = blockIdx.x / nblk, b = blockIdx.x - s * nblk;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) wc[k][threadIdx.x] = 0u;
  __syncthreads();
  volatile unsigned* mine = wc[w];
  const size_t seg0 = (size_t)s * (size_t)P;
  const long t0 = (long)b * LV_TILE + (long)w * LV_SPAN;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned key[LV_ITEMS], idx[LV_ITEMS], rk[LV_ITEMS];
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long i = t0 + r * 64 + lane;
    const bool in = i < P;
    key[r] = LV_INVALID;
    idx[r] = 0u;
    if (in) {
      if (FIRST) { key[r] = lv_sort_key(err[seg0 + i], flag[seg0 + i]); idx[r] = (unsigned)i; }
      else { key[r] = kin[seg0 + i]; idx[r] = iin[seg0 + i]; }
    }
    const unsigned d = lv_digit(key[r], shift);
    unsigned long long peers = __ballot(in);                   // the lanes of this round with my digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long bal = __ballot(in && on);
      peers &= on ? bal : ~bal;
    }
    const unsigned before = in ? mine[d] : 0u;
    rk[r] = before + (unsigned)__popcll(peers & below);
    __builtin_amdgcn_wave_barrier();
    if (in && (peers >> lane) == 1ull) mine[d] = before + (unsigned)__popcll(peers);     // the highest peer keeps the count
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    const int d = threadIdx.x;
    unsigned run = hist[((size_t)s * 256 + d) * (size_t)nblk + b];
#pragma unroll
    for (int k = 0; k < 4; ++k) { base[k][d] = run; run += wc[k][d]; }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long i = t0 + r * 64 + lane;
    if (i < P) {
      const unsigned dst = base[w][lv_digit(key[r], shift)] + rk[r];
      if ((long)dst < P) { kout[seg0 + dst] = key[r]; iout[seg0 + dst] = idx[r]; }      // (always true: the table counted these keys)
    }
  }
}

// ---- stage 3: increments along the sorted order -------------------------------------------------------------------------------------
// fgc[s][block] = foreground elements of the block's tile; counts[s] += (G, V) (integer atomics)
__global__ __launch_bounds__(256) void lv_fgcount_kernel(const unsigned* __restrict__ keys, long P, int nblk, unsigned* __restrict__ fgc,
                                                         int* __restrict__ counts) {
  __shared__ unsigned sh[2];
  const int s = blockIdx.x / nblk, b = blockIdx.x - s * nblk;
  if (threadIdx.x < 2) sh[threadIdx.x] = 0u;
  __syncthreads();
  const size_t seg0 = (size_t)s * (size_t)P;
  const long t0 = (long)b * LV_TILE;
  unsigned nf = 0u, nv = 0u;
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long i = t0 + r * 256 + threadIdx.x;
    if (i < P) {
      const unsigned k = keys[seg0 + i];
      nf += k >> 31;
      nv += (k & LV_INVALID) ? 0u : 1u;
    }
  }
  nf = wave_sum_u(nf);
  nv = wave_sum_u(nv);
  if ((threadIdx.x & 63) == 0) { atomicAdd(&sh[0], nf); atomicAdd(&sh[1], nv); }
  __syncthreads();
  if (threadIdx.x == 0) {
    fgc[(size_t)s * nblk + b] = sh[0];
    if (sh[0]) atomicAdd(&counts[2 * s], (int)sh[0]);
    if (sh[1]) atomicAdd(&counts[2 * s + 1], (int)sh[1]);
  }
}

// fgx = the scanned fgc: foreground elements before the block.  Valid elements come first in the sorted order, so the position is the rank.
__global__ __launch_bounds__(256) void lv_apply_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ idxs, long P, int nblk,
                                                       const unsigned* __restrict__ fgx, const int* __restrict__ counts,
                                                       int* __restrict__ rank, float* __restrict__ coef, double* __restrict__ part) {
  __shared__ unsigned wf[4];
  __shared__ double wl[4];
  const int s = blockIdx.x / nblk, b = blockIdx.x - s * nblk;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t seg0 = (size_t)s * (size_t)P;
  const long t0 = (long)b * LV_TILE + (long)w * LV_SPAN;
  const long G = counts[2 * s];
  const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
  unsigned key[LV_ITEMS];
  unsigned tot = 0u;
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long i = t0 + r * 64 + lane;
    key[r] = (i < P) ? keys[seg0 + i] : LV_INVALID;
    tot += (unsigned)__popcll(__ballot((key[r] >> 31) != 0u));
  }
  if (lane == 0) wf[w] = tot;
  __syncthreads();
  long F = fgx[(size_t)s * nblk + b];
  for (int k = 0; k < w; ++k) F += wf[k];
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long i = t0 + r * 64 + lane;
    const bool fg = (key[r] >> 31) != 0u;
    const unsigned long long bal = __ballot(fg);
    if (i < P) {
      const unsigned j = idxs[seg0 + i];
      float g = 0.f;
      int rk = -1;
      if (!(key[r] & LV_INVALID)) {
        const long Fi = F + __popcll(bal & upto), pos = i + 1;
        const double U = (double)(G + pos - Fi);
        double gd;
        if (G == 0) gd = (pos == 1) ? 1.0 : 0.0;
        else if (fg) gd = 1.0 / U;
        else gd = (double)(G - Fi) / (U * (U - 1.0));
        g = (float)gd;
        rk = (int)i;
        acc += (double)__uint_as_float(LV_ONE - (key[r] & 0x3FFFFFFFu)) * gd;
      }
      if ((long)j < P) {
        coef[seg0 + j] = g;
        if (rank) rank[seg0 + j] = rk;
      }
    }
    F += __popcll(bal);
  }
  acc = wave_sum_d(acc);
  if (lane == 0) wl[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)s * nblk + b] = (wl[0] + wl[1]) + (wl[2] + wl[3]);
}

__global__ __launch_bounds__(256) void lv_segsum_kernel(const double* __restrict__ part, int nblk, double* __restrict__ seg_loss) {
  __shared__ double sh[4];
  const double* p = part + (size_t)blockIdx.x * nblk;
  double a = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) a += p[b];
  a = wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) seg_loss[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- stage 4: the class weighting (one workgroup; a thread per group, the groups' terms in a fixed order) ------------------------------
__global__ __launch_bounds__(256) void lv_finish_kernel(const double* __restrict__ seg_loss, const int* __restrict__ counts, int groups, int K,
                                                        int all, float* __restrict__ segw, float* __restrict__ loss) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int g = threadIdx.x; g < groups; g += 256) {
    int C = 0;
    double L = 0.0;
    for (int c = 0; c < K; ++c) {
      const int s = g * K + c;
      if (counts[2 * s + 1] > 0 && (all || counts[2 * s] > 0)) { ++C; L += seg_loss[s]; }
    }
    const double wgt = C ? 1.0 / ((double)groups * (double)C) : 0.0;
    for (int c = 0; c < K; ++c) {
      const int s = g * K + c;
      segw[s] = (counts[2 * s + 1] > 0 && (all || counts[2 * s] > 0)) ? (float)wgt : 0.f;
    }
    acc += wgt * L;
  }
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)((sh[0] + sh[1]) + (sh[2] + sh[3]));
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
struct LvPlan { int nblk; size_t key[2], idx[2], hist, fgc, part, total; };

static bool lv_plan(int S, long P, LvPlan* pl) {
  if (S < 1 || P < 1 || P >= (1L << 31) || S > (1 << 24)) return false;
  if ((unsigned long long)S * (unsigned long long)P >= (1ull << 32)) return false;
  pl->nblk = cdiv(P, LV_TILE);
  if ((long)S * pl->nblk >= (1L << 31)) return false;
  const size_t a = (((size_t)S * (size_t)P * 4) + 15) & ~(size_t)15, sb = (size_t)S * pl->nblk;
  size_t o = 0;
  pl->key[0] = o; o += a;
  pl->key[1] = o; o += a;
  pl->idx[0] = o; o += a;
  pl->idx[1] = o; o += a;
  pl->hist = o; o += (sb * 256 * 4 + 15) & ~(size_t)15;
  pl->fgc = o; o += (sb * 4 + 15) & ~(size_t)15;
  pl->part = o; o += sb * 8;
  pl->total = o;
  return true;
}

static int lv_shape(const char* who, int N, int K, long HW, int per_image, int* S, long* P) {
  MX_CHECK_ARG(K >= 1 && K <= LV_MAXK, "%s: K=%d outside 1..%d", who, K, LV_MAXK);
  MX_CHECK_ARG(N >= 1 && HW >= 1 && HW < (1L << 31) && (long)N * HW < (1L << 31), "%s: N=%d HW=%ld (N*HW must lie in 1..2^31-1)", who, N, HW);
  *S = per_image ? N * K : K;
  *P = per_image ? HW : (long)N * HW;
  MX_CHECK_ARG((unsigned long long)*S * (unsigned long long)*P < (1ull << 32), "%s: S*P = %d * %ld must stay below 2^32", who, *S, *P);
  return MX_OK;
}

static int lv_errors_launch(const float* seg, const unsigned char* label, int ignore, int N, int K, long HW, int per_image, float* err,
                            unsigned char* flag, hipStream_t st) {
  const long n = (long)N * HW;
  const bool vec = HW % 4 == 0 && ((uintptr_t)seg | (uintptr_t)err) % 16 == 0 && ((uintptr_t)flag % 4) == 0;
  if (vec)
    hipLaunchKernelGGL(lv_errors_kernel<4>, dim3(cdiv(n / 4, 256)), dim3(256), 0, st, seg, label, ignore, N, K, HW, per_image, err, flag);
  else
    hipLaunchKernelGGL(lv_errors_kernel<1>, dim3(cdiv(n, 256)), dim3(256), 0, st, seg, label, ignore, N, K, HW, per_image, err, flag);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

static int lv_core_launch(const float* err, const unsigned char* flag, int S, long P, int* rank, float* coef_g, double* seg_loss,
                          int* seg_counts, void* ws, const LvPlan& pl, hipStream_t st) {
  char* base = (char*)ws;
  unsigned* key[2] = {(unsigned*)(base + pl.key[0]), (unsigned*)(base + pl.key[1])};
  unsigned* idx[2] = {(unsigned*)(base + pl.idx[0]), (unsigned*)(base + pl.idx[1])};
  unsigned* hist = (unsigned*)(base + pl.hist);
  unsigned* fgc = (unsigned*)(base + pl.fgc);
  double* part = (double*)(base + pl.part);
  const int nblk = pl.nblk;
  const dim3 grid((unsigned)((long)S * nblk)), blk(256);
  hipError_t e = hipMemsetAsync(seg_counts, 0, (size_t)S * 2 * sizeof(int), st);
  if (e != hipSuccess) { mx_set_error("lovasz: memset failed: %s", hipGetErrorString(e)); return (int)e; }
  for (int pass = 0; pass < LV_PASSES; ++pass) {               // (err, flag) -> 0 -> 1 -> 0 -> 1
    const int shift = 8 * pass, dst = pass == 0 ? 0 : (pass & 1), src = dst ^ 1;
    if (pass == 0)
      hipLaunchKernelGGL(lv_hist_kernel<true>, grid, blk, 0, st, err, flag, (const unsigned*)nullptr, shift, P, nblk, hist);
    else
      hipLaunchKernelGGL(lv_hist_kernel<false>, grid, blk, 0, st, err, flag, (const unsigned*)key[src], shift, P, nblk, hist);
    hipLaunchKernelGGL(lv_scan_kernel, dim3(S), blk, 0, st, hist, 256L * nblk);
    if (pass == 0)
      hipLaunchKernelGGL(lv_scatter_kernel<true>, grid, blk, 0, st, err, flag, (const unsigned*)nullptr, (const unsigned*)nullptr, shift, P,
                         nblk, (const unsigned*)hist, key[dst], idx[dst]);
    else
      hipLaunchKernelGGL(lv_scatter_kernel<false>, grid, blk, 0, st, err, flag, (const unsigned*)key[src], (const unsigned*)idx[src], shift,
                         P, nblk, (const unsigned*)hist, key[dst], idx[dst]);
    MX_LAUNCH_CHECK();
  }
  const unsigned* skey = key[(LV_PASSES - 1) & 1];
  const unsigned* sidx = idx[(LV_PASSES - 1) & 1];
  hipLaunchKernelGGL(lv_fgcount_kernel, grid, blk, 0, st, skey, P, nblk, fgc, seg_counts);
  hipLaunchKernelGGL(lv_scan_kernel, dim3(S), blk, 0, st, fgc, (long)nblk);
  hipLaunchKernelGGL(lv_apply_kernel, grid, blk, 0, st, skey, sidx, P, nblk, (const unsigned*)fgc, (const int*)seg_counts, rank, coef_g, part);
  hipLaunchKernelGGL(lv_segsum_kernel, dim3(S), blk, 0, st, (const double*)part, nblk, seg_loss);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

extern "C" {

long mx_lovasz_ws(int S, long P) {
  LvPlan pl;
  if (!lv_plan(S, P, &pl)) {
    mx_set_error("lovasz_ws: S=%d P=%ld (need S >= 1, 1 <= P < 2^31, S*P < 2^32)", S, P);
    return MX_EARG;
  }
  return (long)pl.total;
}

int mx_lovasz_errors(const float* seg, const unsigned char* label, int ignore, int N, int K, long HW, int per_image, float* err,
                     unsigned char* flag, void* stream) {
  MX_CHECK_ARG(seg && label && err && flag, "lovasz_errors: null pointer");
  int S; long P;
  if (int rc = lv_shape("lovasz_errors", N, K, HW, per_image, &S, &P)) return rc;
  return lv_errors_launch(seg, label, ignore, N, K, HW, per_image, err, flag, (hipStream_t)stream);
}

int mx_lovasz_core(const float* err, const unsigned char* flag, int S, long P, int* rank, float* coef_g, double* seg_loss,
                   int* seg_counts, void* ws, long ws_bytes, void* stream) {
  MX_CHECK_ARG(err && flag && coef_g && seg_loss && seg_counts && ws, "lovasz_core: null pointer");
  LvPlan pl;
  MX_CHECK_ARG(lv_plan(S, P, &pl), "lovasz_core: S=%d P=%ld (need S >= 1, 1 <= P < 2^31, S*P < 2^32)", S, P);
  MX_CHECK_ARG(ws_bytes >= (long)pl.total && (uintptr_t)ws % 16 == 0, "lovasz_core: ws of %ld bytes (need %ld, 16-byte aligned)", ws_bytes,
               (long)pl.total);
  return lv_core_launch(err, flag, S, P, rank, coef_g, seg_loss, seg_counts, ws, pl, (hipStream_t)stream);
}

int mx_lovasz_fwd(const float* seg, const unsigned char* label, int ignore, int N, int K, long HW, int per_image, int classes_all,
                  float* err, unsigned char* flag, float* coef_g, double* seg_loss, int* seg_counts, float* segw, float* loss, void* ws,
                  long ws_bytes, void* stream) {
  MX_CHECK_ARG(seg && label && err && flag && coef_g && seg_loss && seg_counts && segw && loss && ws, "lovasz_fwd: null pointer");
  int S; long P;
  if (int rc = lv_shape("lovasz_fwd", N, K, HW, per_image, &S, &P)) return rc;
  LvPlan pl;
  MX_CHECK_ARG(lv_plan(S, P, &pl), "lovasz_fwd: S=%d P=%ld (need S*P < 2^32)", S, P);
  MX_CHECK_ARG(ws_bytes >= (long)pl.total && (uintptr_t)ws % 16 == 0, "lovasz_fwd: ws of %ld bytes (need %ld, 16-byte aligned)", ws_bytes,
               (long)pl.total);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = lv_errors_launch(seg, label, ignore, N, K, HW, per_image, err, flag, st)) return rc;
  if (int rc = lv_core_launch(err, flag, S, P, nullptr, coef_g, seg_loss, seg_counts, ws, pl, st)) return rc;
  hipLaunchKernelGGL(lv_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)seg_loss, (const int*)seg_counts, S / K, K, classes_all, segw,
                     loss);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_lovasz_bwd(const float* seg, const unsigned char* label, int ignore, const float* coef_g, const float* segw, const float* gup,
                  int N, int K, long HW, int per_image, float* gseg, void* stream) {
  MX_CHECK_ARG(seg && label && coef_g && segw && gup && gseg, "lovasz_bwd: null pointer");
  int S; long P;
  if (int rc = lv_shape("lovasz_bwd", N, K, HW, per_image, &S, &P)) return rc;
  hipLaunchKernelGGL(lv_bwd_kernel, dim3(cdiv((long)N * HW, 256)), dim3(256), 0, (hipStream_t)stream, seg, label, ignore, coef_g, segw, gup, N,
                     K, HW, per_image, gseg);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
