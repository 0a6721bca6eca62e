// Pixel-adaptive mask refinement (muscle_amd/pamr.py).  include/muscle_hip.h states the model (mx_pamr_affinity ..); DESIGN.md "PAMR"
// gives the layout, the bytes moved and the measured times.
//
//   pamr_affinity_kernel<D, KIND>  one thread per pixel: three walks over the 9 D taps of the image (mean, squared deviations, a_p), the
//                                  P = 8 D logits of the softmax in registers, w written planar [N,P,H,W]
//   pamr_step_kernel<D>            one thread per pixel: its P weights loaded once into registers (one coalesced load per plane), then
//                                  the C channels in turn, 8 D gathers each from m_in and one fixed fma chain p = 0..P-1 from 0, in fp64
//   planar_argmax_kernel           first maximum over the channels of a planar map
// A workgroup is 256 threads = 64 consecutive x of 4 consecutive rows, so every gather of a wave is one contiguous (clamped) row segment:
// the taps are served by the vector L1 and the L2, no LDS and no barrier (a tile with the 24-pixel halo of the default dilations would
// stage (64+48)(4+48) values for 256 outputs).  D is a template parameter: the weights and the tap offsets index registers statically.
#include "common.h"

#define PAMR_MAXD 8
#define PAMR_MAXDIL 64
#define PAMR_TX 64
#define PAMR_TY 4

struct PamrDil { int d[PAMR_MAXD]; };

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the workgroup's tile and image -> (n, y, x) of this thread; false outside the image
__device__ __forceinline__ bool pamr_pixel(int H, int W, int& n, int& y, int& x) {
  const int tiles_x = (W + PAMR_TX - 1) / PAMR_TX, tiles_y = (H + PAMR_TY - 1) / PAMR_TY;
  const int b = blockIdx.x, t = b / tiles_x;
  n = t / tiles_y;
  x = (b - t * tiles_x) * PAMR_TX + (threadIdx.x & (PAMR_TX - 1));
  y = (t - n * tiles_y) * PAMR_TY + (threadIdx.x >> 6);
  return y < H && x < W;
}

// the three channels of pixel `at` (= y*W + x) of image n
template <int KIND>
__device__ __forceinline__ void pamr_rgb(const void* __restrict__ img, int n, int HW, int at, float (&v)[3]) {
  if (KIND == 0) {
    const unsigned char* p = static_cast<const unsigned char*>(img) + ((size_t)n * HW + at) * 3;
    v[0] = (float)p[0]; v[1] = (float)p[1]; v[2] = (float)p[2];
  } else {
    const float* p = static_cast<const float*>(img) + (size_t)n * 3 * HW + at;
    v[0] = p[0]; v[1] = p[HW]; v[2] = p[2 * (size_t)HW];
  }
}

template <int D, int KIND>
__global__ __launch_bounds__(256) void pamr_affinity_kernel(const void* __restrict__ img, int H, int W, PamrDil dil, float* __restrict__ w) {
  int n, y, x;
  if (!pamr_pixel(H, W, n, y, x)) return;
  const int HW = H * W;
  int row[D][3], col[D][3];                              // the taps of dilation j: rows (pre-multiplied by W) and columns, clamped
#pragma unroll
  for (int j = 0; j < D; ++j) {
    row[j][0] = clampi(y - dil.d[j], H - 1) * W; row[j][1] = y * W; row[j][2] = clampi(y + dil.d[j], H - 1) * W;
    col[j][0] = clampi(x - dil.d[j], W - 1);     col[j][1] = x;     col[j][2] = clampi(x + dil.d[j], W - 1);
  }
  // the pooled sample of 9 D values per channel: mean, then the squared deviations, in one fixed order
  float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      float v[3];
      pamr_rgb<KIND>(img, n, HW, row[j][k / 3] + col[j][k % 3], v);
      s[0] += v[0]; s[1] += v[1]; s[2] += v[2];
    }
  const float cnt = (float)(9 * D);
  const float mean[3] = {s[0] / cnt, s[1] / cnt, s[2] / cnt};
  float q[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      float v[3];
      pamr_rgb<KIND>(img, n, HW, row[j][k / 3] + col[j][k % 3], v);
#pragma unroll
      for (int c = 0; c < 3; ++c) { const float d = v[c] - mean[c]; q[c] = fmaf(d, d, q[c]); }
    }
  float den[3], ctr[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) den[c] = fmaf(0.1f, sqrtf(q[c] / (cnt - 1.f)), 1e-8f);
  pamr_rgb<KIND>(img, n, HW, y * W + x, ctr);
  float a[8 * D], mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int t = k < 4 ? k : k + 1;                   // the 9 positions without the centre
      float v[3];
      pamr_rgb<KIND>(img, n, HW, row[j][t / 3] + col[j][t % 3], v);
      const float e = (-fabsf(ctr[0] - v[0]) / den[0] + -fabsf(ctr[1] - v[1]) / den[1] + -fabsf(ctr[2] - v[2]) / den[2]) / 3.f;
      a[8 * j + k] = e;
      mx = fmaxf(mx, e);
    }
  double sum = 0.0;                                      // the normaliser in fp64: the fp32 weights of a pixel then sum to 1 within 5e-8
#pragma unroll
  for (int p = 0; p < 8 * D; ++p) { a[p] = expf(a[p] - mx); sum += (double)a[p]; }
  const double inv = 1.0 / sum;
  float* wp = w + (size_t)n * (8 * D) * HW + y * W + x;
#pragma unroll
  for (int p = 0; p < 8 * D; ++p) wp[(size_t)p * HW] = (float)((double)a[p] * inv);
}

template <int D>
__global__ __launch_bounds__(256, D <= 2 ? 4 : (D <= 4 ? 3 : 2)) void pamr_step_kernel(const float* __restrict__ w, const float* __restrict__ m_in, float* __restrict__ m_out,
                                                        int C, int H, int W, PamrDil dil) {
  int n, y, x;
  if (!pamr_pixel(H, W, n, y, x)) return;
  const int HW = H * W;
  int row[D][3], col[D][3];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    row[j][0] = clampi(y - dil.d[j], H - 1) * W; row[j][1] = y * W; row[j][2] = clampi(y + dil.d[j], H - 1) * W;
    col[j][0] = clampi(x - dil.d[j], W - 1);     col[j][1] = x;     col[j][2] = clampi(x + dil.d[j], W - 1);
  }
  float wr[8 * D];
  const float* wp = w + (size_t)n * (8 * D) * HW + y * W + x;
#pragma unroll
  for (int p = 0; p < 8 * D; ++p) wr[p] = wp[(size_t)p * HW];
  const float* mi = m_in + (size_t)n * C * HW;
  float* mo = m_out + (size_t)n * C * HW + y * W + x;
  for (int c = 0; c < C; ++c) {
    double acc = 0.0;                                    // exact products, an fp64 chain, ONE rounding to fp32 per output (see the header)
#pragma unroll
    for (int j = 0; j < D; ++j) {                        // the 8 gathers of a dilation are requested together, then its 8 terms of the chain
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int t = k < 4 ? k : k + 1;                 // the 9 positions without the centre
        v[k] = mi[row[j][t / 3] + col[j][t % 3]];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma((double)wr[8 * j + k], (double)v[k], acc);
      __builtin_amdgcn_sched_barrier(0);                 // keeps the scheduler from requesting every dilation's gathers at once (spills)
    }
    *mo = (float)acc;
    mi += HW;
    mo += HW;
  }
}

__global__ __launch_bounds__(256) void planar_argmax_kernel(const float* __restrict__ m, int C, int HW, long total,
                                                            unsigned char* __restrict__ pred) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long n = i / HW, hw = i - n * HW;
  const float* p = m + n * C * HW + hw;
  float best = p[0];
  int arg = 0;
  for (int c = 1; c < C; ++c) {
    const float v = p[(size_t)c * HW];
    if (v > best) { best = v; arg = c; }
  }
  pred[i] = (unsigned char)arg;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static int pamr_check(const char* who, int N, int C, int H, int W, const int* dil, int D, PamrDil* out) {
  MX_CHECK_ARG(D >= 1 && D <= PAMR_MAXD, "%s: 1 <= D <= %d (got %d)", who, PAMR_MAXD, D);
  MX_CHECK_ARG(dil != nullptr, "%s: dil is NULL", who);
  MX_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: N, C, H, W >= 1 (got %d, %d, %d, %d)", who, N, C, H, W);
  for (int j = 0; j < PAMR_MAXD; ++j) {
    if (j < D) MX_CHECK_ARG(dil[j] >= 1 && dil[j] <= PAMR_MAXDIL, "%s: dilation %d is %d, outside 1..%d", who, j, dil[j], PAMR_MAXDIL);
    out->d[j] = j < D ? dil[j] : 1;
  }
  const long wide = C > 8 * D ? C : 8 * D;
  MX_CHECK_ARG((double)N * (double)wide * (double)H * (double)W < 2147483648.0, "%s: N max(C,P) H W must stay below 2^31", who);
  return MX_OK;
}

static inline unsigned pamr_grid(int N, int H, int W) {
  return (unsigned)((long)cdiv(W, PAMR_TX) * cdiv(H, PAMR_TY) * N);
}

static inline long pamr_round(long bytes) { return (bytes + 255) / 256 * 256; }

#define PAMR_FOR_D(D, X)                                                                   \
  switch (D) {                                                                             \
    case 1: X(1); break; case 2: X(2); break; case 3: X(3); break; case 4: X(4); break;    \
    case 5: X(5); break; case 6: X(6); break; case 7: X(7); break; default: X(8); break;   \
  }

static int pamr_affinity_launch(const void* img, int img_kind, int N, int H, int W, const PamrDil& pd, int D, float* w, hipStream_t st) {
  const unsigned grid = pamr_grid(N, H, W);
#define PAMR_AFF(DD)                                                                                          \
  if (img_kind == 0) pamr_affinity_kernel<DD, 0><<<grid, 256, 0, st>>>(img, H, W, pd, w);                     \
  else pamr_affinity_kernel<DD, 1><<<grid, 256, 0, st>>>(img, H, W, pd, w)
  PAMR_FOR_D(D, PAMR_AFF)
#undef PAMR_AFF
  MX_LAUNCH_CHECK();
  return MX_OK;
}

static int pamr_step_launch(const float* w, const float* m_in, float* m_out, int N, int C, int H, int W, const PamrDil& pd, int D,
                            hipStream_t st) {
  const unsigned grid = pamr_grid(N, H, W);
#define PAMR_STEP(DD) pamr_step_kernel<DD><<<grid, 256, 0, st>>>(w, m_in, m_out, C, H, W, pd)
  PAMR_FOR_D(D, PAMR_STEP)
#undef PAMR_STEP
  MX_LAUNCH_CHECK();
  return MX_OK;
}

static bool pamr_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

extern "C" int mx_pamr_affinity(const void* img, int img_kind, int N, int H, int W, const int* dil, int D, float* w, void* stream) {
  PamrDil pd;
  const int rc = pamr_check("mx_pamr_affinity", N, 1, H, W, dil, D, &pd);
  if (rc != MX_OK) return rc;
  MX_CHECK_ARG(img && w, "mx_pamr_affinity: img and w must not be NULL");
  MX_CHECK_ARG(img_kind == 0 || img_kind == 1, "mx_pamr_affinity: img_kind 0 (uint8 [N,H,W,3]) or 1 (fp32 [N,3,H,W]), got %d", img_kind);
  return pamr_affinity_launch(img, img_kind, N, H, W, pd, D, w, (hipStream_t)stream);
}

extern "C" int mx_pamr_step(const float* w, const float* m_in, float* m_out, int N, int C, int H, int W, const int* dil, int D,
                            void* stream) {
  PamrDil pd;
  const int rc = pamr_check("mx_pamr_step", N, C, H, W, dil, D, &pd);
  if (rc != MX_OK) return rc;
  MX_CHECK_ARG(w && m_in && m_out, "mx_pamr_step: w, m_in and m_out must not be NULL");
  MX_CHECK_ARG(!pamr_overlap(m_in, m_out, (size_t)N * C * H * W * 4), "mx_pamr_step: m_in must not overlap m_out");
  return pamr_step_launch(w, m_in, m_out, N, C, H, W, pd, D, (hipStream_t)stream);
}

extern "C" long mx_pamr_ws(int N, int C, int H, int W, int D) {
  const int one[PAMR_MAXD] = {1, 1, 1, 1, 1, 1, 1, 1};
  PamrDil pd;
  if (pamr_check("mx_pamr_ws", N, C, H, W, one, D, &pd) != MX_OK) return -1;
  const long px = (long)N * H * W;
  return pamr_round(px * 8 * D * 4) + pamr_round(px * C * 4);
}

extern "C" int mx_pamr(const void* img, int img_kind, const float* mask, float* out, int N, int C, int H, int W, const int* dil, int D,
                       int num_iter, void* ws, long ws_bytes, void* stream) {
  PamrDil pd;
  const int rc = pamr_check("mx_pamr", N, C, H, W, dil, D, &pd);
  if (rc != MX_OK) return rc;
  MX_CHECK_ARG(img && mask && out, "mx_pamr: img, mask and out must not be NULL");
  MX_CHECK_ARG(img_kind == 0 || img_kind == 1, "mx_pamr: img_kind 0 (uint8 [N,H,W,3]) or 1 (fp32 [N,3,H,W]), got %d", img_kind);
  MX_CHECK_ARG(num_iter >= 0, "mx_pamr: num_iter >= 0 (got %d)", num_iter);
  const size_t bytes = (size_t)N * C * H * W * 4;
  MX_CHECK_ARG(!pamr_overlap(mask, out, bytes), "mx_pamr: mask must not overlap out");
  hipStream_t st = (hipStream_t)stream;
  if (num_iter == 0) {
    hipError_t e = hipMemcpyAsync(out, mask, bytes, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) { mx_set_error("mx_pamr: copy failed: %s", hipGetErrorString(e)); return (int)e; }
    return MX_OK;
  }
  MX_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "mx_pamr: ws must be 16-byte aligned and not NULL");
  MX_CHECK_ARG(ws_bytes >= mx_pamr_ws(N, C, H, W, D), "mx_pamr: ws holds %ld bytes, mx_pamr_ws asks for %ld", ws_bytes,
               mx_pamr_ws(N, C, H, W, D));
  float* w = static_cast<float*>(ws);
  float* tmp = reinterpret_cast<float*>(static_cast<char*>(ws) + pamr_round((long)N * H * W * 8 * D * 4));
  int r = pamr_affinity_launch(img, img_kind, N, H, W, pd, D, w, st);
  if (r != MX_OK) return r;
  const float* src = mask;
  for (int s = 1; s <= num_iter; ++s) {                  // the last iteration writes out, the ones before it alternate backwards from there
    float* dst = ((num_iter - s) & 1) ? tmp : out;
    r = pamr_step_launch(w, src, dst, N, C, H, W, pd, D, st);
    if (r != MX_OK) return r;
    src = dst;
  }
  return MX_OK;
}

extern "C" int mx_planar_argmax(const float* m, int N, int C, int H, int W, unsigned char* pred, void* stream) {
  MX_CHECK_ARG(m && pred, "mx_planar_argmax: m and pred must not be NULL");
  MX_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && C >= 1 && C <= 256, "mx_planar_argmax: N, H, W >= 1 and 1 <= C <= 256 (got %d, %d, %d, %d)",
               N, H, W, C);
  MX_CHECK_ARG((double)N * C * (double)H * W < 2147483648.0, "mx_planar_argmax: N C H W must stay below 2^31");
  const long total = (long)N * H * W;
  planar_argmax_kernel<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(m, C, H * W, total, pred);
  MX_LAUNCH_CHECK();
  return MX_OK;
}
