// Permutohedral-lattice filter (Adams, Baek & Davis 2010) and the two dense CRFs on it: the approximation pydensecrf evaluates the
// CRFs of src/imutils.py:439-456 (crf_inference) and src/imutils.py:477-491 (crf_inference_label) with.  A selectable backend
// beside the exact windowed kernels of crf.hip: a DIFFERENT model (include/muscle_hip.h states it), whose cost per
// pass is O(N * D) whatever the kernel width.
//
// Build, once per image and kernel (D = 2: (x, y) / sxy;  D = 5: (x / sxy, y / sxy, r / srgb, g / srgb, b / srgb)):
//   lat_build_kernel    one thread per pixel: the enclosing simplex in fp32, every operation rounded on its own in the order the
//                       header states (the vertex set depends on the rounding at simplex borders), the D+1 barycentric weights,
//                       and the D+1 vertex keys inserted into an open-addressing hash table by 64-bit compare-and-swap.
//                       A key is PACKED into one 64-bit word: every key coordinate of vertex r is r + (D+1) m_i, and m_i lies in
//                       a range that follows from the image size and the widths (lat_plan); the word is the mixed-radix number
//                       of the m_i - lo_i, times D+1, plus r.  An image whose ranges do not fit 2^62 is refused before any launch.
//                       A slot is read before it is swapped, so the thousands of pixels of a constant-colour region that share
//                       a vertex issue one atomic between them, not one each (only the first arrivals see the slot empty).
//   lat_assign_kernel   one thread per slot: occupied slots draw consecutive vertex ids (one atomic per wave) and unpack their key
//   lat_resolve_kernel  per (pixel, r): slot -> vertex id
//   lat_nbr_kernel      per (vertex, direction j): the two blur neighbours by hash lookup, -1 when absent
// Vertex ids depend on the arrival order and may differ from run to run; no value below depends on them.
//
// Filter of C <= 32 channels:
//   splat   val[vertex] += b[r] * in[pixel] in 64-bit FIXED POINT with integer atomics (no floating-point atomics anywhere in this
//           library): integer addition is associative, so the sums are the same bits in every arrival order.  The unit of a
//           channel is 2^-k with k = 37 - floor(log2(max|in|)) over that channel (a max-reduction by integer atomicMax on the
//           floats' bits; a channel's result does not depend on the other channels), and b * in is formed exactly in double
//           before it is rounded to the unit: every contribution is off by at most 2^-38 max|in|, a vertex's sum of n
//           contributions by at most n * 2^-38 max|in| (fp32 rounds at 2^-24 relative), and N (D+1) <= 2^24 contributions of at
//           most 2^38 (1 + 2^-22) units stay below 2^63.
//   blur    for j = 0..D in this order: val' = val + 0.5 (val[n1_j] + val[n2_j]), fp32, absent neighbours count 0
//   slice   out[pixel] = alpha * sum_r b[r] val[vertex_r], r ascending, alpha = 1 / (1 + 2^-D)
// All of it gather- and bandwidth-bound; every kernel's grid covers the worst case N (D+1) vertices and exits above the
// vertex count, which stays on the device: nothing synchronises with the host.
#include "common.h"
#include "crf_model.h"
#include <math.h>
#include <string.h>

namespace {

typedef unsigned long long lat_u64;
constexpr lat_u64 LAT_EMPTY = ~0ULL;
constexpr int LAT_MAXC = 32;
constexpr int LAT_MAXL = 24;
constexpr long LAT_MAX_CAND = 1L << 24;      // N * (D+1): the fixed-point headroom of the splat
constexpr int LAT_HDR = 256;                 // bytes: [0] vertex count, [1 + c] the bits of max|in| over channel c

struct LatParams {
  int D, H, W, N;
  int cap;                // N * (D+1): candidates, and the most vertices there can be
  unsigned tsize;         // slots of the hash table, a power of two >= 2 * cap
  int tshift;             // 64 - log2(tsize)
  float sxy, srgb, inv_d1;
  float sf[5];
  int lo[5];
  unsigned n[5];
};

struct LatDesc {
  LatParams p;
  int* hdr; lat_u64* table; int* slot_id; int* vid; float* bary; int* keys; int* nbr;      // the structure
  long long* acc; float* val[2];                                                          // filter scratch (C-dependent)
};

long lat_align(long b) { return (b + 255) / 256 * 256; }

unsigned lat_table_size(long cap) {
  unsigned t = 64;
  while ((long)t < 2 * cap) t <<= 1;
  return t;
}

long lat_struct_bytes(int D, long N) {
  const long cap = N * (D + 1);
  const long T = lat_table_size(cap);
  return LAT_HDR + lat_align(T * 8) + lat_align(T * 4) + 2 * lat_align(cap * 4) + lat_align(cap * D * 4) + lat_align(2L * (D + 1) * cap * 4);
}

long lat_scratch_bytes(long cap, int C) { return lat_align(cap * C * 8) + 2 * lat_align(cap * C * 4); }

// carve the structure at `base`; returns the first byte behind it
char* lat_carve_struct(LatDesc& d, char* base) {
  const long cap = d.p.cap, T = d.p.tsize;
  const int D = d.p.D;
  char* q = base;
  d.hdr = (int*)q; q += LAT_HDR;
  d.table = (lat_u64*)q; q += lat_align(T * 8);
  d.slot_id = (int*)q; q += lat_align(T * 4);
  d.vid = (int*)q; q += lat_align(cap * 4);
  d.bary = (float*)q; q += lat_align(cap * 4);
  d.keys = (int*)q; q += lat_align(cap * D * 4);
  d.nbr = (int*)q; q += lat_align(2L * (D + 1) * cap * 4);
  return q;
}

char* lat_carve_scratch(LatDesc& d, char* base, long cap, int C) {
  char* q = base;
  d.acc = (long long*)q; q += lat_align(cap * C * 8);
  d.val[0] = (float*)q; q += lat_align(cap * C * 4);
  d.val[1] = (float*)q; q += lat_align(cap * C * 4);
  return q;
}

// The key ranges of an image: false when the packed key does not fit (or a coordinate leaves the exact range of fp32 integers).
// Features are >= 0, so el[0] = sum_k cf_k lies in [0, sum_k cfmax_k] and el[i] = sum_{k >= i} cf_k - i cf_{i-1} in
// [-i cfmax_{i-1}, sum_{k >= i} cfmax_k]; m_i = round(el[i] / (D+1)) moved by at most 2 by the wrap and the canonical simplex;
// one more on each side for the rounding of the fp32 operations.
bool lat_plan(int D, int H, int W, float sxy, float srgb, LatParams& p) {
  memset(&p, 0, sizeof(p));
  p.D = D; p.H = H; p.W = W; p.N = H * W;
  p.cap = p.N * (D + 1);
  p.tsize = lat_table_size(p.cap);
  int lg = 0;
  while ((1u << lg) < p.tsize) ++lg;
  p.tshift = 64 - lg;
  p.sxy = sxy; p.srgb = srgb;
  p.inv_d1 = (float)(1.0 / (D + 1));
  double sf[5], cfm[5];
  for (int i = 0; i < D; ++i) {
    sf[i] = (D + 1) * sqrt(2.0 / 3.0) / sqrt((double)(i + 1) * (i + 2));
    p.sf[i] = (float)sf[i];
    const double fmax = i == 0 ? (W - 1) / (double)sxy : i == 1 ? (H - 1) / (double)sxy : 255.0 / (double)srgb;
    cfm[i] = fmax * sf[i];
  }
  double bits = log2((double)(D + 1));
  for (int i = 0; i < D; ++i) {
    double hi = 0.0;
    for (int k = i; k < D; ++k) hi += cfm[k];
    const double lo = i == 0 ? 0.0 : -(double)i * cfm[i - 1];
    const double mlo = floor(lo / (D + 1)) - 3.0, mhi = ceil(hi / (D + 1)) + 3.0;
    if (!(mlo > -2097152.0 && mhi < 2097152.0)) return false;      // (D+1) m stays an exact fp32 integer
    p.lo[i] = (int)mlo;
    p.n[i] = (unsigned)(mhi - mlo + 1.0);
    bits += log2((double)p.n[i]);
  }
  return bits < 62.0;
}

__device__ __forceinline__ unsigned lat_hash(lat_u64 k, int tshift) { return (unsigned)((k * 0x9E3779B97F4A7C15ULL) >> tshift); }

// the word of vertex (r; m[0..D-1]); CLAMP: a coordinate outside its range is clamped (build: cannot happen, and must not reach
// another slot range if it did); otherwise LAT_EMPTY: no vertex of this image has that key
template <int D, bool CLAMP>
__device__ __forceinline__ lat_u64 lat_pack(const LatParams& p, int r, const int* m) {
  lat_u64 a = 0;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    int t = m[i] - p.lo[i];
    if ((unsigned)t >= p.n[i]) {
      if (!CLAMP) return LAT_EMPTY;
      t = t < 0 ? 0 : (int)p.n[i] - 1;
    }
    a = a * p.n[i] + (unsigned)t;
  }
  return a * (D + 1) + (unsigned)r;
}

__device__ __forceinline__ int lat_insert(lat_u64* table, const LatParams& p, lat_u64 k) {
  const unsigned mask = p.tsize - 1;
  unsigned h = lat_hash(k, p.tshift);
  for (unsigned n = 0; n < p.tsize; ++n) {               // at most cap <= tsize / 2 slots are ever taken: an empty one is met
    lat_u64 cur = __hip_atomic_load(table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == k) return (int)h;
    if (cur == LAT_EMPTY) {
      cur = atomicCAS(table + h, LAT_EMPTY, k);
      if (cur == LAT_EMPTY || cur == k) return (int)h;
    }
    h = (h + 1) & mask;
  }
  return (int)h;
}

__device__ __forceinline__ int lat_lookup(const lat_u64* table, const LatParams& p, lat_u64 k) {
  const unsigned mask = p.tsize - 1;
  unsigned h = lat_hash(k, p.tshift);
  for (unsigned n = 0; n < p.tsize; ++n) {
    const lat_u64 cur = table[h];
    if (cur == k) return (int)h;
    if (cur == LAT_EMPTY) return -1;
    h = (h + 1) & mask;
  }
  return -1;
}

// The simplex of one pixel: mi[i] = rem0[i] / (D+1) after the wrap, rank[i], b[0..D].  Every fp32 operation is rounded on its own
// (no contraction), in the order of include/muscle_hip.h.
template <int D>
__device__ __forceinline__ void lat_simplex(const float* f, const LatParams& p, int* mi, int* rank, float* b) {
#pragma clang fp contract(off)
  constexpr int D1 = D + 1;
  float el[D1], rem0[D1], df[D1];
  float sm = 0.f;
#pragma unroll
  for (int j = D; j >= 1; --j) {
    const float cf = f[j - 1] * p.sf[j - 1];
    const float jc = (float)j * cf;
    el[j] = sm - jc;
    sm = sm + cf;
  }
  el[0] = sm;
  int sum = 0;
#pragma unroll
  for (int i = 0; i < D1; ++i) {
    const float q = el[i] * p.inv_d1;
    const float rd = floorf(q + 0.5f);
    rem0[i] = rd * (float)D1;
    sum += (int)rd;
    df[i] = el[i] - rem0[i];
    rank[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < D1; ++i)
#pragma unroll
    for (int j = i + 1; j < D1; ++j) {
      if (df[i] < df[j]) rank[i]++; else rank[j]++;
    }
  if (sum > 0) {
#pragma unroll
    for (int i = 0; i < D1; ++i) {
      if (rank[i] >= D1 - sum) { rem0[i] = rem0[i] - (float)D1; rank[i] += sum - D1; } else rank[i] += sum;
    }
  } else if (sum < 0) {
#pragma unroll
    for (int i = 0; i < D1; ++i) {
      if (rank[i] < -sum) { rem0[i] = rem0[i] + (float)D1; rank[i] += D1 + sum; } else rank[i] += sum;
    }
  }
  float bb[D + 2];
#pragma unroll
  for (int k = 0; k < D + 2; ++k) bb[k] = 0.f;
#pragma unroll
  for (int i = 0; i < D1; ++i) {
    const float d = el[i] - rem0[i];
    const float v = d / (float)D1;
#pragma unroll
    for (int k = 0; k < D + 2; ++k) {                     // static indices: bb stays in registers
      if (k == D - rank[i]) bb[k] = bb[k] + v;
      if (k == D1 - rank[i]) bb[k] = bb[k] - v;
    }
    mi[i] = (int)rem0[i] / D1;                            // rem0 is an exact multiple of D+1
  }
  const float one = 1.f + bb[D1];
  bb[0] = bb[0] + one;
#pragma unroll
  for (int k = 0; k < D1; ++k) b[k] = bb[k];
}

template <int D>
__global__ __launch_bounds__(256) void lat_build_kernel(const unsigned char* rgb, const LatParams p, lat_u64* table, int* slot_of,
                                                        float* bary) {
  constexpr int D1 = D + 1;
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= p.N) return;
  float f[D];
  f[0] = (float)(pix % p.W) / p.sxy;                      // correctly rounded fp32 divisions
  f[1] = (float)(pix / p.W) / p.sxy;
  if constexpr (D == 5) {
#pragma unroll
    for (int c = 0; c < 3; ++c) f[2 + c] = (float)rgb[3L * pix + c] / p.srgb;
  }
  int mi[D1], rank[D1];
  float b[D1];
  lat_simplex<D>(f, p, mi, rank, b);
#pragma unroll
  for (int r = 0; r < D1; ++r) {
    int m[D];
#pragma unroll
    for (int i = 0; i < D; ++i) m[i] = mi[i] - (rank[i] > D - r ? 1 : 0);      // canon[r][k] = r for k <= D-r, else r - (D+1)
    const lat_u64 k = lat_pack<D, true>(p, r, m);
    slot_of[(long)pix * D1 + r] = lat_insert(table, p, k);
    bary[(long)pix * D1 + r] = b[r];
  }
}

template <int D>
__global__ __launch_bounds__(256) void lat_assign_kernel(const LatParams p, const lat_u64* table, int* slot_id, int* keys, int* hdr) {
  constexpr int D1 = D + 1;
  const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;          // tsize is a multiple of 64: whole waves
  const lat_u64 k = s < p.tsize ? table[s] : LAT_EMPTY;
  const bool occ = k != LAT_EMPTY;
  const unsigned long long mask = __ballot(occ);
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0 && mask) base = atomicAdd(hdr, __popcll(mask));
  base = __shfl(base, 0, 64);
  if (!occ) {
    if (s < p.tsize) slot_id[s] = -1;
    return;
  }
  const int id = base + __popcll(mask & ((1ULL << lane) - 1ULL));
  slot_id[s] = id;
  lat_u64 a = k;
  const int r = (int)(a % D1);
  a /= D1;
#pragma unroll
  for (int i = D - 1; i >= 0; --i) {
    const int t = (int)(a % p.n[i]);
    a /= p.n[i];
    keys[(long)id * D + i] = (t + p.lo[i]) * D1 + r;
  }
}

__global__ void lat_resolve_kernel(int* vid, const int* slot_id, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) vid[i] = slot_id[vid[i]];
}

// nbr[(2 j + s) * cap + v]: s = 0: n1 (key - 1, coordinate j: key[j] + D), s = 1: n2 (key + 1, coordinate j: key[j] - D)
template <int D>
__global__ __launch_bounds__(256) void lat_nbr_kernel(const LatParams p, const lat_u64* table, const int* slot_id, const int* keys,
                                                      int* nbr, const int* hdr) {
  constexpr int D1 = D + 1;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int v = (int)(idx / D1), j = (int)(idx % D1);
  if (v >= *hdr || v >= p.cap) return;
  int key[D];
#pragma unroll
  for (int i = 0; i < D; ++i) key[i] = keys[(long)v * D + i];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int step = s == 0 ? -1 : 1;
    int m[D], k0 = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int k = key[i] + (i == j ? -step * D : step);
      if (i == 0) k0 = k;
      m[i] = k;
    }
    const int r = ((k0 % D1) + D1) % D1;
#pragma unroll
    for (int i = 0; i < D; ++i) m[i] = (m[i] - r) / D1;   // exact: every coordinate is congruent to r
    const lat_u64 w = lat_pack<D, false>(p, r, m);
    int id = -1;
    if (w != LAT_EMPTY) {
      const int slot = lat_lookup(table, p, w);
      if (slot >= 0) id = slot_id[slot];
    }
    nbr[(long)(2 * j + s) * p.cap + v] = id;
  }
}

// ---- the filter ------------------------------------------------------------------------------------------------------------
// element (pixel, c) of a map: a[pixel * sp + c * sc]; in == NULL: the constant 1; pre / post: per-pixel factors or NULL
struct LatIO {
  const float* in; long isp, isc; const float* pre;
  float* out; long osp, osc; const float* post;
  float w;                // out = w * post * filter(pre * in)
  int rsqrt;              // out = 1 / sqrt(filter + 1e-20) instead (the normaliser)
};

__device__ __forceinline__ float lat_input(const LatIO& io, int pix, int c) {
  float x = io.in ? io.in[pix * io.isp + c * io.isc] : 1.f;
  if (io.pre) x *= io.pre[pix];
  return x;
}

// blockIdx.y = the channel
__global__ __launch_bounds__(256) void lat_absmax_kernel(const LatIO io, int N, unsigned* amax) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  float a = 0.f;
  if (pix < N) a = fabsf(lat_input(io, pix, c));
  a = wave_max(a);
  if ((threadIdx.x & 63) == 0 && a > 0.f) atomicMax(amax + c, __float_as_uint(a));     // non-negative floats order as their bits
}

__global__ void lat_clear_kernel(long long* acc, const int* hdr, int C, long cap) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (long)*hdr * C && idx < cap * C) acc[idx] = 0;
}

// 2^k units per 1.0 in channel c: k = 37 - floor(log2(max|in|)), so |in| * 2^k < 2^38
__device__ __forceinline__ int lat_unit_exp(const int* hdr, int c) {
  const float m = __uint_as_float((unsigned)hdr[1 + c]);
  return (m > 0.f && m < INFINITY) ? 37 - ilogbf(m) : 0;
}

template <int D>
__global__ __launch_bounds__(256) void lat_splat_kernel(const LatIO io, int N, int C, const int* vid, const float* bary, long long* acc,
                                                        const int* hdr) {
  constexpr int D1 = D + 1;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)N * C) return;
  const int pix = (int)(idx / C), c = (int)(idx % C);
  const double x = (double)lat_input(io, pix, c) * ldexp(1.0, lat_unit_exp(hdr, c));
#pragma unroll
  for (int r = 0; r < D1; ++r) {
    const long long q = __double2ll_rn((double)bary[(long)pix * D1 + r] * x);
    if (q != 0) atomicAdd((lat_u64*)(acc + (long)vid[(long)pix * D1 + r] * C + c), (lat_u64)q);
  }
}

__global__ void lat_convert_kernel(const long long* acc, float* val, const int* hdr, int C, long cap) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (long)hdr[0] * C && idx < cap * C) val[idx] = (float)((double)acc[idx] * ldexp(1.0, -lat_unit_exp(hdr, (int)(idx % C))));
}

__global__ __launch_bounds__(256) void lat_blur_kernel(const float* src, float* dst, const int* n1, const int* n2, const int* hdr, int C,
                                                       long cap) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)hdr[0] * C || idx >= cap * C) return;
  const int v = (int)(idx / C), c = (int)(idx % C);
  const int a = n1[v], b = n2[v];
  const float va = a >= 0 ? src[(long)a * C + c] : 0.f;
  const float vb = b >= 0 ? src[(long)b * C + c] : 0.f;
  dst[idx] = src[idx] + 0.5f * (va + vb);
}

template <int D>
__global__ __launch_bounds__(256) void lat_slice_kernel(const LatIO io, int N, int C, const int* vid, const float* bary, const float* val) {
  constexpr int D1 = D + 1;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)N * C) return;
  const int pix = (int)(idx / C), c = (int)(idx % C);
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < D1; ++r) s += bary[(long)pix * D1 + r] * val[(long)vid[(long)pix * D1 + r] * C + c];
  s *= 1.0f / (1.0f + 1.0f / (float)(1 << D));
  float o;
  if (io.rsqrt) o = 1.0f / sqrtf(s + 1e-20f);
  else o = io.w * (io.post ? io.post[pix] : 1.f) * s;
  io.out[pix * io.osp + c * io.osc] = o;
}

template <int D>
int lat_build_t(const LatDesc& d, const unsigned char* rgb, hipStream_t st) {
  const LatParams& p = d.p;
  hipError_t e = hipMemsetAsync(d.hdr, 0, LAT_HDR, st);
  if (e == hipSuccess) e = hipMemsetAsync(d.table, 0xFF, (size_t)p.tsize * 8, st);
  if (e != hipSuccess) { mx_set_error("lattice build: memset failed: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(lat_build_kernel<D>, dim3(cdiv(p.N, 256)), dim3(256), 0, st, rgb, p, d.table, d.vid, d.bary);
  MX_LAUNCH_CHECK();
  hipLaunchKernelGGL(lat_assign_kernel<D>, dim3(cdiv(p.tsize, 256)), dim3(256), 0, st, p, d.table, d.slot_id, d.keys, d.hdr);
  MX_LAUNCH_CHECK();
  hipLaunchKernelGGL(lat_resolve_kernel, dim3(cdiv(p.cap, 256)), dim3(256), 0, st, d.vid, d.slot_id, p.cap);
  MX_LAUNCH_CHECK();
  hipLaunchKernelGGL(lat_nbr_kernel<D>, dim3(cdiv((long)p.cap * (D + 1), 256)), dim3(256), 0, st, p, d.table, d.slot_id, d.keys, d.nbr,
                     d.hdr);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int lat_build(const LatDesc& d, const unsigned char* rgb, hipStream_t st) {
  return d.p.D == 2 ? lat_build_t<2>(d, rgb, st) : lat_build_t<5>(d, rgb, st);
}

template <int D>
int lat_filter_t(const LatDesc& d, const LatIO& io, int C, hipStream_t st) {
  const LatParams& p = d.p;
  const long NC = (long)p.N * C, VC = (long)p.cap * C;
  hipError_t e = hipMemsetAsync(d.hdr + 1, 0, 4 * LAT_MAXC, st);
  if (e != hipSuccess) { mx_set_error("lattice filter: memset failed: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(lat_absmax_kernel, dim3(cdiv(p.N, 256), C), dim3(256), 0, st, io, p.N, (unsigned*)(d.hdr + 1));
  MX_LAUNCH_CHECK();
  hipLaunchKernelGGL(lat_clear_kernel, dim3(cdiv(VC, 256)), dim3(256), 0, st, d.acc, d.hdr, C, (long)p.cap);
  MX_LAUNCH_CHECK();
  hipLaunchKernelGGL(lat_splat_kernel<D>, dim3(cdiv(NC, 256)), dim3(256), 0, st, io, p.N, C, d.vid, d.bary, d.acc, d.hdr);
  MX_LAUNCH_CHECK();
  hipLaunchKernelGGL(lat_convert_kernel, dim3(cdiv(VC, 256)), dim3(256), 0, st, d.acc, d.val[0], d.hdr, C, (long)p.cap);
  MX_LAUNCH_CHECK();
  int cur = 0;
  for (int j = 0; j <= D; ++j) {
    hipLaunchKernelGGL(lat_blur_kernel, dim3(cdiv(VC, 256)), dim3(256), 0, st, d.val[cur], d.val[cur ^ 1], d.nbr + (long)(2 * j) * p.cap,
                       d.nbr + (long)(2 * j + 1) * p.cap, d.hdr, C, (long)p.cap);
    MX_LAUNCH_CHECK();
    cur ^= 1;
  }
  hipLaunchKernelGGL(lat_slice_kernel<D>, dim3(cdiv(NC, 256)), dim3(256), 0, st, io, p.N, C, d.vid, d.bary, d.val[cur]);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int lat_filter(const LatDesc& d, const LatIO& io, int C, hipStream_t st) {
  return d.p.D == 2 ? lat_filter_t<2>(d, io, C, st) : lat_filter_t<5>(d, io, C, st);
}

// ---- the lattices that mx_lattice_build left in caller workspaces: what the host must know to launch on them (sizes, ranges);
// everything data-dependent stays on the device
struct LatEntry { void* ws; int dev; LatDesc d; };
constexpr int LAT_REG = 64;
std::mutex lat_mu;
LatEntry lat_reg[LAT_REG];
int lat_reg_next = 0;

void lat_register(void* ws, const LatDesc& d) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(lat_mu);
  int at = -1;
  for (int i = 0; i < LAT_REG; ++i)
    if (lat_reg[i].ws == ws && lat_reg[i].dev == dev) at = i;
  if (at < 0) { at = lat_reg_next; lat_reg_next = (lat_reg_next + 1) % LAT_REG; }
  lat_reg[at].ws = ws; lat_reg[at].dev = dev; lat_reg[at].d = d;
}

bool lat_find(void* ws, LatDesc& d) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(lat_mu);
  for (int i = 0; i < LAT_REG; ++i)
    if (lat_reg[i].ws == ws && lat_reg[i].dev == dev && ws) { d = lat_reg[i].d; return true; }
  return false;
}

// ---- the CRFs on two lattices -------------------------------------------------------------------------------------------------
// Maps are pixel-major [N][C], C = G * L columns: problem g in columns g*L .. g*L+L-1.

// U = -log(clip(confidence * p + (1 - confidence) / L, 1e-5, 1)), Q_0 = softmax(-U)
__global__ void lat_unary_prob_kernel(const float* prob, int L, int N, float confidence, float* U, float* q0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float base = (1.0f - confidence) / (float)L;
  for (int l = 0; l < L; ++l) {
    const float u = crf_prob_unary(confidence, prob[(long)l * N + i], base);
    U[(long)i * L + l] = u;
    q0[(long)i * L + l] = -u;
  }
  crf_softmax_row(q0 + (long)i * L, L);
}

// the two thresholded argmax maps
__global__ void lat_cam_labels_kernel(const float* cams, int Cc, int N, float fg_thres, float bg_thres, unsigned char* lab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int lf, lb;
  crf_cam_labels(cams, Cc, N, i, fg_thres, bg_thres, lf, lb);
  lab[i] = (unsigned char)lf;
  lab[(long)N + i] = (unsigned char)lb;
}

__global__ void lat_in_labels_kernel(const int* labels, int L, int N, unsigned char* lab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  lab[i] = (unsigned char)crf_in_label(labels[i], L);
}

// unary_from_labels(zero_unsure=False) of problems g0 .. g0+G-1 and Q_0 = softmax(-U)
__global__ void lat_unary_lab_kernel(const unsigned char* lab, int g0, int G, int L, int N, float u_own, float u_oth, float* U, float* q0) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * G) return;
  const int i = idx / G, g = idx % G;
  const int own = lab[(long)(g0 + g) * N + i];
  const CrfLabelE e = crf_label_exp(u_own, u_oth);
  const float inv = crf_label_inv(e, own, L);
  const long o = (long)i * (G * L) + g * L;
  for (int l = 0; l < L; ++l) {
    U[o + l] = (l == own) ? u_own : u_oth;
    q0[o + l] = ((l == own) ? e.own : e.oth) * inv;
  }
}

// Q_{s+1} = softmax_l((M_g - U) + M_b) per problem (M == NULL: softmax(-U)); on the last step Q_t and its first maximum
__global__ void lat_final_kernel(const float* U, const float* Mg, const float* Mb, int g0, int G, int L, int N, float* q_next, int last,
                                 float* q_out, unsigned char* pred, unsigned char* pred2) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * G) return;
  const int i = idx / G, g = idx % G;
  const long o = (long)i * (G * L) + g * L;
  for (int l = 0; l < L; ++l) q_next[o + l] = Mg ? (Mg[o + l] - U[o + l]) + Mb[o + l] : -U[o + l];
  const int best = crf_softmax_row(q_next + o, L);
  if (!last) return;
  if (q_out)
    for (int l = 0; l < L; ++l) q_out[((long)(g0 + g) * L + l) * N + i] = q_next[o + l];
  if (pred) pred[(long)(g0 + g) * N + i] = (unsigned char)best;
  if (pred2) pred2[(long)(g0 + g) * N + i] = (unsigned char)best;
}

// the IR label out of the two argmax maps
__global__ void lat_conf_kernel(const unsigned char* pred, const int* keys, int N, unsigned char* conf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  conf[i] = crf_combine(keys[pred[i]], keys[pred[(long)N + i]]);
}

int lat_crf_columns(int L) { return 2 * L <= LAT_MAXC ? 2 * L : L; }

long lat_crf_ws_bytes(int C, long N) {
  return lat_struct_bytes(2, N) + lat_struct_bytes(5, N) + lat_scratch_bytes(N * 6, C) + 5 * lat_align(N * C * 4) + 2 * lat_align(N * 4) +
         2 * lat_align(2 * N);
}

struct LatCrf {
  LatDesc g, b;
  float* U; float* Q[2]; float* Mg; float* Mb; float* ng; float* nb; unsigned char* lab; unsigned char* pred;
};

void lat_crf_carve(LatCrf& w, void* ws, int C) {
  const long N = w.g.p.N;
  char* q = lat_carve_struct(w.g, (char*)ws);
  q = lat_carve_struct(w.b, q);
  q = lat_carve_scratch(w.b, q, N * 6, C);
  w.g.acc = w.b.acc; w.g.val[0] = w.b.val[0]; w.g.val[1] = w.b.val[1];      // one filter at a time on the stream
  w.U = (float*)q; q += lat_align(N * C * 4);
  w.Q[0] = (float*)q; q += lat_align(N * C * 4);
  w.Q[1] = (float*)q; q += lat_align(N * C * 4);
  w.Mg = (float*)q; q += lat_align(N * C * 4);
  w.Mb = (float*)q; q += lat_align(N * C * 4);
  w.ng = (float*)q; q += lat_align(N * 4);
  w.nb = (float*)q; q += lat_align(N * 4);
  w.lab = (unsigned char*)q; q += lat_align(2 * N);
  w.pred = (unsigned char*)q;
}

struct LatModel { int t; float sxy_g, w_g, sxy_b, srgb, w_b; };

// both lattices and both normalisers n_m = 1 / sqrt(filter(1) + 1e-20)
int lat_crf_setup(LatCrf& w, const unsigned char* rgb, hipStream_t st) {
  int rc = lat_build(w.g, rgb, st);
  if (rc != MX_OK) return rc;
  rc = lat_build(w.b, rgb, st);
  if (rc != MX_OK) return rc;
  LatIO io = {};
  io.osp = 1; io.osc = 0; io.rsqrt = 1;
  io.out = w.ng;
  rc = lat_filter(w.g, io, 1, st);
  if (rc != MX_OK) return rc;
  io.out = w.nb;
  return lat_filter(w.b, io, 1, st);
}

// t mean-field steps on the C = G * L columns of U / Q[0]
int lat_crf_iterate(LatCrf& w, const LatModel& m, int g0, int G, int L, float* q_out, unsigned char* pred, unsigned char* pred2,
                    hipStream_t st) {
  const int N = w.g.p.N, C = G * L;
  const dim3 grid(cdiv((long)N * G, 128)), block(128);
  if (m.t == 0) {
    hipLaunchKernelGGL(lat_final_kernel, grid, block, 0, st, w.U, (const float*)nullptr, (const float*)nullptr, g0, G, L, N, w.Q[1], 1,
                       q_out, pred, pred2);
    MX_LAUNCH_CHECK();
    return MX_OK;
  }
  for (int s = 0; s < m.t; ++s) {
    LatIO io = {};
    io.in = w.Q[s & 1]; io.isp = C; io.isc = 1; io.osp = C; io.osc = 1;
    io.pre = w.ng; io.post = w.ng; io.w = m.w_g; io.out = w.Mg;
    int rc = lat_filter(w.g, io, C, st);
    if (rc != MX_OK) return rc;
    io.pre = w.nb; io.post = w.nb; io.w = m.w_b; io.out = w.Mb;
    rc = lat_filter(w.b, io, C, st);
    if (rc != MX_OK) return rc;
    hipLaunchKernelGGL(lat_final_kernel, grid, block, 0, st, w.U, w.Mg, w.Mb, g0, G, L, N, w.Q[(s + 1) & 1], s == m.t - 1 ? 1 : 0, q_out,
                       pred, pred2);
    MX_LAUNCH_CHECK();
  }
  return MX_OK;
}

}  // namespace

extern "C" {

#define LAT_CHECK_SIZE(name)                                                                                                        \
  MX_CHECK_ARG(H > 0 && W > 0 && (long)H * W * 6 <= LAT_MAX_CAND, name ": bad size H=%d W=%d (H*W in 1..2^24/6)", H, W)

#define LAT_CHECK_PLAN(name, D, sxy, srgb, p)                                                                                       \
  MX_CHECK_ARG(lat_plan(D, H, W, sxy, srgb, p),                                                                                     \
               name ": the key range of a %d x %d image at sxy=%g srgb=%g does not fit the packed 64-bit key", H, W, (double)(sxy), \
               (double)(srgb))

long mx_lattice_ws(int D, int H, int W, int C) {
  if (!((D == 2 || D == 5) && H > 0 && W > 0 && (long)H * W * 6 <= LAT_MAX_CAND && C >= 1 && C <= LAT_MAXC)) {
    mx_set_error("lattice_ws: bad args D=%d (2 or 5) H=%d W=%d (H*W <= 2^24/6) C=%d (1..%d)", D, H, W, C, LAT_MAXC);
    return MX_EARG;
  }
  const long N = (long)H * W;
  return lat_struct_bytes(D, N) + lat_scratch_bytes(N * (D + 1), C);
}

int mx_lattice_build(const unsigned char* rgb, int H, int W, float sxy, float srgb, void* ws, void* stream) {
  MX_CHECK_ARG(ws, "lattice_build: ws is NULL");
  MX_CHECK_ARG(((uintptr_t)ws & 15) == 0, "lattice_build: ws must be 16-byte aligned");
  LAT_CHECK_SIZE("lattice_build");
  MX_CHECK_ARG(sxy > 0.f, "lattice_build: sxy=%g must be positive", sxy);
  const int D = srgb > 0.f ? 5 : 2;
  MX_CHECK_ARG(D == 2 || rgb, "lattice_build: rgb is NULL (srgb > 0: the bilateral kernel)");
  LatDesc d;
  LAT_CHECK_PLAN("lattice_build", D, sxy, D == 5 ? srgb : 1.f, d.p);
  char* q = lat_carve_struct(d, (char*)ws);
  lat_carve_scratch(d, q, d.p.cap, 1);                    // acc / val are re-carved per filter call for its C
  const int rc = lat_build(d, rgb, (hipStream_t)stream);
  if (rc != MX_OK) return rc;
  lat_register(ws, d);
  return MX_OK;
}

int mx_lattice_filter(void* ws, const float* in, float* out, int C, void* stream) {
  MX_CHECK_ARG(ws && in && out, "lattice_filter: null pointer (ws, in or out)");
  MX_CHECK_ARG(C >= 1 && C <= LAT_MAXC, "lattice_filter: C=%d outside 1..%d", C, LAT_MAXC);
  LatDesc d;
  MX_CHECK_ARG(lat_find(ws, d), "lattice_filter: ws holds no lattice (mx_lattice_build it first)");
  lat_carve_scratch(d, (char*)ws + lat_struct_bytes(d.p.D, d.p.N), d.p.cap, C);
  LatIO io = {};
  io.in = in; io.isp = 1; io.isc = d.p.N; io.out = out; io.osp = 1; io.osc = d.p.N; io.w = 1.f;
  return lat_filter(d, io, C, (hipStream_t)stream);
}

int mx_lattice_export(void* ws, int* vid, float* weight, int* keys, int* nbr, int* count, void* stream) {
  MX_CHECK_ARG(ws && vid && weight && keys && nbr && count, "lattice_export: null pointer");
  LatDesc d;
  MX_CHECK_ARG(lat_find(ws, d), "lattice_export: ws holds no lattice (mx_lattice_build it first)");
  const size_t cap = (size_t)d.p.cap;
  const int D = d.p.D;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(vid, d.vid, cap * 4, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(weight, d.bary, cap * 4, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(keys, d.keys, cap * D * 4, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(nbr, d.nbr, cap * 2 * (D + 1) * 4, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(count, d.hdr, 4, hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) { mx_set_error("lattice_export: copy failed: %s", hipGetErrorString(e)); return (int)e; }
  return MX_OK;
}

long mx_crf_lattice_ws(int L, int H, int W) {
  if (!(L >= 1 && L <= LAT_MAXL && H > 0 && W > 0 && (long)H * W * 6 <= LAT_MAX_CAND)) {
    mx_set_error("crf_lattice_ws: bad args L=%d (1..%d) H=%d W=%d (H*W <= 2^24/6)", L, LAT_MAXL, H, W);
    return MX_EARG;
  }
  return lat_crf_ws_bytes(lat_crf_columns(L), (long)H * W);
}

#define LAT_CHECK_MODEL(name)                                                                                                       \
  LAT_CHECK_SIZE(name);                                                                                                             \
  MX_CHECK_ARG(t >= 0, name ": t=%d is negative", t);                                                                               \
  MX_CHECK_ARG(sxy_g > 0.f && sxy_b > 0.f && srgb > 0.f, name ": sxy_g=%g sxy_b=%g srgb=%g must be positive", sxy_g, sxy_b, srgb);  \
  MX_CHECK_ARG(((uintptr_t)ws & 15) == 0, name ": workspace must be 16-byte aligned");                                              \
  LatCrf w;                                                                                                                         \
  LAT_CHECK_PLAN(name, 2, sxy_g, 1.f, w.g.p);                                                                                       \
  LAT_CHECK_PLAN(name, 5, sxy_b, srgb, w.b.p)

int mx_crf_inference_lattice(const unsigned char* rgb, const float* prob, int L, int H, int W, int t, float confidence, float sxy_g,
                             float w_g, float sxy_b, float srgb, float w_b, void* ws, float* q_out, unsigned char* pred, void* stream) {
  MX_CHECK_ARG(rgb && prob && ws, "crf_inference_lattice: null pointer (rgb, prob or workspace)");
  MX_CHECK_ARG(q_out || pred, "crf_inference_lattice: q_out and pred are both NULL");
  MX_CHECK_ARG(L >= 1 && L <= LAT_MAXL, "crf_inference_lattice: L=%d outside 1..%d", L, LAT_MAXL);
  LAT_CHECK_MODEL("crf_inference_lattice");
  hipStream_t st = (hipStream_t)stream;
  const int N = H * W;
  lat_crf_carve(w, ws, lat_crf_columns(L));
  const LatModel m = {t, sxy_g, w_g, sxy_b, srgb, w_b};
  if (t > 0) {
    const int rc = lat_crf_setup(w, rgb, st);
    if (rc != MX_OK) return rc;
  }
  hipLaunchKernelGGL(lat_unary_prob_kernel, dim3(cdiv(N, 128)), dim3(128), 0, st, prob, L, N, confidence, w.U, w.Q[0]);
  MX_LAUNCH_CHECK();
  return lat_crf_iterate(w, m, 0, 1, L, q_out, pred, (unsigned char*)nullptr, st);
}

int mx_ir_label_lattice(const unsigned char* rgb, const float* cams, const int* keys, int C, int H, int W, float fg_thres, float bg_thres,
                        int t, float gt_prob, float sxy_g, float w_g, float sxy_b, float srgb, float w_b, void* ws, unsigned char* conf,
                        unsigned char* pred2, float* q_out, void* stream) {
  MX_CHECK_ARG(rgb && cams && keys && ws, "ir_label_lattice: null pointer (rgb, cams, keys or ws)");
  MX_CHECK_ARG(conf, "ir_label_lattice: conf is NULL");
  MX_CHECK_ARG(C >= 1 && C + 1 <= 21, "ir_label_lattice: C=%d outside 1..20 (L = C + 1 labels, L >= 2)", C);
  MX_CHECK_ARG(gt_prob > 0.f && gt_prob < 1.f, "ir_label_lattice: gt_prob=%g outside (0, 1)", gt_prob);
  LAT_CHECK_MODEL("ir_label_lattice");
  hipStream_t st = (hipStream_t)stream;
  const int N = H * W, L = C + 1;
  lat_crf_carve(w, ws, lat_crf_columns(L));
  const LatModel m = {t, sxy_g, w_g, sxy_b, srgb, w_b};
  const CrfLabelU u = crf_label_unary(gt_prob, L);
  if (t > 0) {
    const int rc = lat_crf_setup(w, rgb, st);
    if (rc != MX_OK) return rc;
  }
  hipLaunchKernelGGL(lat_cam_labels_kernel, dim3(cdiv(N, 128)), dim3(128), 0, st, cams, C, N, fg_thres, bg_thres, w.lab);
  MX_LAUNCH_CHECK();
  const int G = 2 * L <= LAT_MAXC ? 2 : 1;
  for (int g0 = 0; g0 < 2; g0 += G) {
    hipLaunchKernelGGL(lat_unary_lab_kernel, dim3(cdiv((long)N * G, 128)), dim3(128), 0, st, w.lab, g0, G, L, N, u.own, u.oth, w.U, w.Q[0]);
    MX_LAUNCH_CHECK();
    const int rc = lat_crf_iterate(w, m, g0, G, L, q_out, w.pred, pred2, st);
    if (rc != MX_OK) return rc;
  }
  hipLaunchKernelGGL(lat_conf_kernel, dim3(cdiv(N, 128)), dim3(128), 0, st, w.pred, keys, N, conf);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_crf_label_lattice(const unsigned char* rgb, const int* labels, int L, int H, int W, int t, float gt_prob, float sxy_g, float w_g,
                         float sxy_b, float srgb, float w_b, void* ws, unsigned char* pred, float* q_out, void* stream) {
  MX_CHECK_ARG(rgb && labels && ws, "crf_label_lattice: null pointer (rgb, labels or ws)");
  MX_CHECK_ARG(pred || q_out, "crf_label_lattice: pred and q_out are both NULL");
  MX_CHECK_ARG(L >= 2 && L <= 21, "crf_label_lattice: L=%d outside 2..21", L);
  MX_CHECK_ARG(gt_prob > 0.f && gt_prob < 1.f, "crf_label_lattice: gt_prob=%g outside (0, 1)", gt_prob);
  LAT_CHECK_MODEL("crf_label_lattice");
  hipStream_t st = (hipStream_t)stream;
  const int N = H * W;
  lat_crf_carve(w, ws, lat_crf_columns(L));
  const LatModel m = {t, sxy_g, w_g, sxy_b, srgb, w_b};
  const CrfLabelU u = crf_label_unary(gt_prob, L);
  if (t > 0) {
    const int rc = lat_crf_setup(w, rgb, st);
    if (rc != MX_OK) return rc;
  }
  hipLaunchKernelGGL(lat_in_labels_kernel, dim3(cdiv(N, 128)), dim3(128), 0, st, labels, L, N, w.lab);
  MX_LAUNCH_CHECK();
  hipLaunchKernelGGL(lat_unary_lab_kernel, dim3(cdiv(N, 128)), dim3(128), 0, st, w.lab, 0, 1, L, N, u.own, u.oth, w.U, w.Q[0]);
  MX_LAUNCH_CHECK();
  return lat_crf_iterate(w, m, 0, 1, L, q_out, pred, (unsigned char*)nullptr, st);
}

}  // extern "C"
