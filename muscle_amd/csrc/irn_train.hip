// Training the IRN heads (src/backbones/resnet50_irn.py:143-212, AffinityDisplacementLoss): the loss head forward and backward,
// and the backward of a head's GroupNorm -> half-pixel bilinear up-sample -> crop -> ReLU into its concatenation slice.
//
// The loss head.  The reference gathers sigmoid(edge) along every search path with index_select, max-pools along the path, and
// keeps [N, n_dst, n_src] fp32 tensors for the affinity, the two log losses, the pair displacements and the three label
// masks.  Here none of them exists: one thread owns one source pixel of the cropped window, walks all paths over an LDS halo tile,
// derives the pair's label class from the uint8 segmentation map (GetAffinityLabelFromIndices, src/data.py:611-637) and adds
// its terms to seven sums.  The only object of that extent is the arg-max byte map (position of the path maximum, first wins
// like max_pool2d's CPU backward), stored by the forward instead of being recomputed by the backward: the derivation with
// its byte and work counts is in DESIGN.md, "Training the IRN heads".
// Backward is a gather with one owner per output element: the gradient of an edge pixel is a function of its own sigmoid and of
// three INTEGER counts (pairs of each class whose path maximum sits on it); the gradient of a displacement component is two
// integer sums of signs times two coefficients.  No floating-point atomics, no order-dependent float sums: bit-reproducible.
// The loss sums are fp64 partials per workgroup, joined in index order by one workgroup.
#include "common.h"

#define IT_TILE 16
#define IT_MAX_RF 15
#define IT_RES 16                                        // doubles in the result block, see mx_irn_loss_fwd in the header

__device__ __forceinline__ double it_sigmoid(float x) { return 1.0 / (1.0 + exp(-(double)x)); }

// 0 = no pair (an end is >= 21), 1 = bg-pos, 2 = fg-pos, 3 = neg
__device__ __forceinline__ int it_pair_class(int lfrom, int lto) {
  if (lfrom >= 21 || lto >= 21) return 0;
  if (lfrom != lto) return 3;
  return lfrom == 0 ? 1 : 2;
}

__device__ __forceinline__ int it_sign(double v) { return (v > 0.0) - (v < 0.0); }

// grid (tiles, N).  part[(n * tiles + tile) * 8 + {bg*pos, fg*pos, neg*neg, fg*fg_loss, bg*bg_loss, n_bg, n_fg, n_neg}]
__global__ __launch_bounds__(256) void it_loss_fwd_kernel(const float* __restrict__ E, int lde, const float* __restrict__ D, int ldd,
                                                          const unsigned char* __restrict__ L, const int* __restrict__ pts,
                                                          const int* __restrict__ poff, const int* __restrict__ plen, int nd, int H,
                                                          int W, int rf, unsigned char* __restrict__ amax, double* __restrict__ part) {
  const int ch = H - rf, cw = W - 2 * rf;
  const int tiles_x = (cw + IT_TILE - 1) / IT_TILE;
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, n = blockIdx.y;
  const int sy0 = ty * IT_TILE, sx0 = tx * IT_TILE;      // window coordinates; full column = window column + rf
  const int hh = IT_TILE + rf, hw = IT_TILE + 2 * rf;    // halo: full rows sy0.., full columns sx0..
  extern __shared__ float it_smem[];
  float* sg = it_smem;
  float* d0 = sg + hh * hw;
  float* d1 = d0 + hh * hw;
  unsigned char* lb = reinterpret_cast<unsigned char*>(d1 + hh * hw);
  for (int i = tid; i < hh * hw; i += 256) {
    const int r = i / hw, c = i - r * hw;
    const int y = sy0 + r, x = sx0 + c;
    const bool in = y < H && x < W;
    const long p = ((long)n * H + (in ? y : 0)) * W + (in ? x : 0);
    sg[i] = in ? E[p * lde] : -INFINITY;               // the logit: the sigmoid is monotonic, the path maximum is taken on it
    d0[i] = in ? D[p * ldd] : 0.f;
    d1[i] = in ? D[p * ldd + 1] : 0.f;
    lb[i] = in ? L[p] : (unsigned char)255;
  }
  __syncthreads();
  const int lx = tid & (IT_TILE - 1), ly = tid / IT_TILE;
  const int sy = sy0 + ly, sx = sx0 + lx;
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (sy < ch && sx < cw) {
    const int sidx = ly * hw + lx + rf;
    const int ls = lb[sidx];
    const double ds0 = d0[sidx], ds1 = d1[sidx];
    const long plane = (long)ch * cw;
    unsigned char* am = amax + (long)n * nd * plane + (long)sy * cw + sx;
    for (int d = 0; d < nd; ++d) {
      const int o = poff[d], len = plen[d];
      float m = -INFINITY;
      int arg = 0;
      for (int k = 0; k < len; ++k) {
        const float v = sg[sidx + pts[2 * (o + k)] * hw + pts[2 * (o + k) + 1]];
        if (v > m) { m = v; arg = k; }
      }
      am[d * plane] = (unsigned char)arg;
      const int dy0 = pts[2 * o], dx0 = pts[2 * o + 1];
      const int didx = sidx + dy0 * hw + dx0;
      const int cls = it_pair_class(ls, lb[didx]);
      if (cls == 0) continue;
      const double aff = 1.0 - it_sigmoid(m);
      if (cls == 3) {
        a[2] += -log(1.0 + 1e-5 - aff);
        a[7] += 1.0;
      } else {
        const double pos = -log(aff + 1e-5);
        const double p0 = ds0 - (double)d0[didx], p1 = ds1 - (double)d1[didx];
        if (cls == 1) {
          a[0] += pos;
          a[4] += fabs(p0) + fabs(p1);
          a[5] += 1.0;
        } else {
          a[1] += pos;
          a[3] += fabs(p0 - (double)dy0) + fabs(p1 - (double)dx0);
          a[6] += 1.0;
        }
      }
    }
  }
  __shared__ double sh[4][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = wave_sum_d(a[j]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[tid >> 6][j] = a[j];
  }
  __syncthreads();
  if (tid < 8) part[((long)n * gridDim.x + blockIdx.x) * 8 + tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
}

// one workgroup: the partials in index order, then the combination of the public IRN training loop
__global__ __launch_bounds__(256) void it_loss_finalize_kernel(const double* __restrict__ part, int blocks, double* __restrict__ res) {
  __shared__ double sh[256][8];
  const int tid = threadIdx.x;
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = tid; b < blocks; b += 256)
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += part[(long)b * 8 + j];
#pragma unroll
  for (int j = 0; j < 8; ++j) sh[tid][j] = a[j];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int j = 0; j < 8; ++j) sh[tid][j] += sh[tid + s][j];
    __syncthreads();
  }
  if (tid == 0) {
    const double* t = sh[0];
    const double nbg = t[5], nfg = t[6], nng = t[7];
    const double pos_aff = 0.5 * t[0] / (nbg + 1e-5) + 0.5 * t[1] / (nfg + 1e-5);
    const double neg_aff = t[2] / (nng + 1e-5);
    const double dp_fg = t[3] / (2.0 * nfg + 1e-5);
    const double dp_bg = t[4] / (2.0 * nbg + 1e-5);
    res[0] = pos_aff; res[1] = neg_aff; res[2] = dp_fg; res[3] = dp_bg;
    res[4] = (pos_aff + neg_aff) / 2.0 + (dp_fg + dp_bg) / 2.0;
    res[5] = nbg; res[6] = nfg; res[7] = nng;
    res[8] = 0.25 / (nbg + 1e-5);                        // d total / d (one bg-pos log term)
    res[9] = 0.25 / (nfg + 1e-5);
    res[10] = 0.5 / (nng + 1e-5);
    res[11] = 0.5 / (2.0 * nfg + 1e-5);                  // d total / d (one fg |.| term)
    res[12] = 0.5 / (2.0 * nbg + 1e-5);
    res[13] = res[14] = res[15] = 0.0;
  }
}

// grid (ceil(HW / 256), N): one thread per pixel of the full map writes its row of dE [N*H*W, 4] and dD [N*H*W, 4]
__global__ __launch_bounds__(256) void it_loss_bwd_kernel(const float* __restrict__ E, int lde, const float* __restrict__ D, int ldd,
                                                          const unsigned char* __restrict__ L, const int* __restrict__ pts,
                                                          const int* __restrict__ poff, const int* __restrict__ plen, int nd, int H,
                                                          int W, int rf, const unsigned char* __restrict__ amax,
                                                          const double* __restrict__ res, float* __restrict__ dE, float* __restrict__ dD) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int n = blockIdx.y;
  const int py = p / W, px = p - py * W;
  const int ch = H - rf, cw = W - 2 * rf;
  const long plane = (long)ch * cw;
  const unsigned char* Ln = L + (long)n * H * W;
  const float* Dn = D + (long)n * H * W * ldd;
  const unsigned char* An = amax + (long)n * nd * plane;
  const double dp0 = Dn[(long)p * ldd], dp1 = Dn[(long)p * ldd + 1];
  const int lp = Ln[p];
  const bool is_src = py < ch && px >= rf && px < rf + cw;
  int n_bg = 0, n_fg = 0, n_ng = 0;                       // pairs whose path maximum is this pixel, by class
  int sbg0 = 0, sbg1 = 0, sfg0 = 0, sfg1 = 0;
  for (int d = 0; d < nd; ++d) {
    const int o = poff[d], len = plen[d];
    const int dy0 = pts[2 * o], dx0 = pts[2 * o + 1];
    for (int k = 0; k < len; ++k) {
      const int sy = py - pts[2 * (o + k)], sxf = px - pts[2 * (o + k) + 1];
      if (sy < 0 || sy >= ch || sxf < rf || sxf >= rf + cw) continue;
      if (An[d * plane + (long)sy * cw + (sxf - rf)] != k) continue;
      const int cls = it_pair_class(Ln[sy * W + sxf], Ln[(sy + dy0) * W + sxf + dx0]);
      n_bg += cls == 1;
      n_fg += cls == 2;
      n_ng += cls == 3;
    }
    if (is_src) {                                        // this pixel as the source of pair d
      const int q = (py + dy0) * W + px + dx0;
      const int cls = it_pair_class(lp, Ln[q]);
      if (cls == 1 || cls == 2) {
        const double p0 = dp0 - (double)Dn[(long)q * ldd], p1 = dp1 - (double)Dn[(long)q * ldd + 1];
        if (cls == 1) { sbg0 += it_sign(p0); sbg1 += it_sign(p1); }
        else { sfg0 += it_sign(p0 - (double)dy0); sfg1 += it_sign(p1 - (double)dx0); }
      }
    }
    const int sy = py - dy0, sxf = px - dx0;             // this pixel as the destination of pair d
    if (sy >= 0 && sy < ch && sxf >= rf && sxf < rf + cw) {
      const int q = sy * W + sxf;
      const int cls = it_pair_class(Ln[q], lp);
      if (cls == 1 || cls == 2) {
        const double p0 = (double)Dn[(long)q * ldd] - dp0, p1 = (double)Dn[(long)q * ldd + 1] - dp1;
        if (cls == 1) { sbg0 -= it_sign(p0); sbg1 -= it_sign(p1); }
        else { sfg0 -= it_sign(p0 - (double)dy0); sfg1 -= it_sign(p1 - (double)dx0); }
      }
    }
  }
  const double s = it_sigmoid(E[((long)n * H * W + p) * lde]);
  const double ge = s * (1.0 - s) * ((res[8] * n_bg + res[9] * n_fg) / ((1.0 - s) + 1e-5) - res[10] * n_ng / (1.0 + 1e-5 - (1.0 - s)));
  const long row = ((long)n * H * W + p) * 4;
  st4(dE + row, make_float4((float)ge, 0.f, 0.f, 0.f));
  st4(dD + row, make_float4((float)(res[11] * sfg0 + res[12] * sbg0), (float)(res[11] * sfg1 + res[12] * sbg1), 0.f, 0.f));
}

// =====================================================================================================================
// Adjoint of mx_gn_resize: ReLU mask from the stored forward slice, crop, transpose of the half-pixel bilinear up-sample as a
// gather - every source pixel visits the destination pixels that can have it as a tap, in index order.
// =====================================================================================================================
// weight of source index s in destination index d's two taps (halfpixel_tap, common.h: the forward's own)
__device__ __forceinline__ float it_tap_weight(int d, float rs, int n_src, int s) {
  int i0, i1;
  float l1;
  halfpixel_tap(d, rs, n_src, i0, i1, l1);
  return (i0 == s ? 1.f - l1 : 0.f) + (i1 == s ? l1 : 0.f);
}

__global__ __launch_bounds__(256) void it_gn_resize_bwd_kernel(const float* __restrict__ gdst, const float* __restrict__ fdst,
                                                               float* __restrict__ dY, int N, int Hs, int Ws, int C, int scale, int Hd,
                                                               int Wd, int ldd, int coff) {
  const int C4 = C / 4;
  const float rs = 1.f / (float)scale;
  const long total = (long)N * Hs * Ws * C4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const long p = i / C4;
    const int xs = (int)(p % Ws), ys = (int)((p / Ws) % Hs), n = (int)(p / ((long)Ws * Hs));
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int y_lo = scale == 1 ? ys : max(0, ys * scale - scale), y_hi = scale == 1 ? ys : ys * scale + 2 * scale - 1;
    const int x_lo = scale == 1 ? xs : max(0, xs * scale - scale), x_hi = scale == 1 ? xs : xs * scale + 2 * scale - 1;
    for (int yd = y_lo; yd <= min(y_hi, Hd - 1); ++yd) {
      const float wy = scale == 1 ? 1.f : it_tap_weight(yd, rs, Hs, ys);
      if (wy == 0.f) continue;
      for (int xd = x_lo; xd <= min(x_hi, Wd - 1); ++xd) {
        const float wx = scale == 1 ? 1.f : it_tap_weight(xd, rs, Ws, xs);
        if (wx == 0.f) continue;
        const long q = (((long)n * Hd + yd) * Wd + xd) * ldd + coff + c;
        const float4 g = ld4(gdst + q), f = ld4(fdst + q);
        const float w = wy * wx;
        acc.x += f.x > 0.f ? w * g.x : 0.f;
        acc.y += f.y > 0.f ? w * g.y : 0.f;
        acc.z += f.z > 0.f ? w * g.z : 0.f;
        acc.w += f.w > 0.f ? w * g.w : 0.f;
      }
    }
    st4(dY + p * C + c, acc);
  }
}

// =====================================================================================================================
// GroupNorm backward.  One pass forms, per (sample, row slice, channel), the fp64 sums of dY and dY * xhat; the finalisation
// joins them in index order into the per-(n, g) sums (weighted by gamma) and into dgamma / dbeta; the apply writes
// dX = rstd * (gamma dY - (S1 + xhat S2) / m).
// =====================================================================================================================
#define IT_GN_MAX_SLICES 64

static int it_gn_slices(int HW) {
  int s = cdiv(HW, 512);
  return s < 1 ? 1 : (s > IT_GN_MAX_SLICES ? IT_GN_MAX_SLICES : s);
}

// grid (C / 32, slices, N); 256 threads = 32 channels x 8 row lanes
__global__ __launch_bounds__(256) void it_gn_bwd_partial_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                                const float* __restrict__ stat, int HW, int C, int G, int rows_per,
                                                                double* __restrict__ part) {
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl, sl = blockIdx.y, n = blockIdx.z;
  const int g = c / (C / G);
  const float mean = stat[2 * (n * G + g)], rstd = stat[2 * (n * G + g) + 1];
  const int r0 = sl * rows_per, r1 = min(HW, r0 + rows_per);
  double sb = 0.0, sx = 0.0;
  for (int r = r0 + rl; r < r1; r += 8) {
    const long q = ((long)n * HW + r) * C + c;
    const float dy = dY[q], xh = (X[q] - mean) * rstd;
    sb += (double)dy;
    sx += (double)dy * (double)xh;
  }
  __shared__ double sh[8][32][2];
  sh[rl][cl][0] = sb;
  sh[rl][cl][1] = sx;
  __syncthreads();
  if (rl == 0) {
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { t0 += sh[k][cl][0]; t1 += sh[k][cl][1]; }
    double* o = part + (((long)n * gridDim.y + sl) * C + c) * 2;
    o[0] = t0;
    o[1] = t1;
  }
}

// threads [0, N*G): sums[n][g] = {S1, S2}; threads [N*G, N*G + C): dgamma[c], dbeta[c]
__global__ __launch_bounds__(64) void it_gn_bwd_finalize_kernel(const double* __restrict__ part, const float* __restrict__ gamma, int N,
                                                                int S, int C, int G, double* __restrict__ sums,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int cg = C / G;
  if (i < N * G) {
    const int n = i / G, g = i - n * G;
    double s1 = 0.0, s2 = 0.0;
    for (int sl = 0; sl < S; ++sl)
      for (int c = g * cg; c < (g + 1) * cg; ++c) {
        const double* q = part + (((long)n * S + sl) * C + c) * 2;
        s1 += (double)gamma[c] * q[0];
        s2 += (double)gamma[c] * q[1];
      }
    sums[2 * i] = s1;
    sums[2 * i + 1] = s2;
  } else if (i < N * G + C) {
    const int c = i - N * G;
    double db = 0.0, dg = 0.0;
    for (int n = 0; n < N; ++n)
      for (int sl = 0; sl < S; ++sl) {
        const double* q = part + (((long)n * S + sl) * C + c) * 2;
        db += q[0];
        dg += q[1];
      }
    dgamma[c] = (float)dg;
    dbeta[c] = (float)db;
  }
}

__global__ __launch_bounds__(256) void it_gn_bwd_apply_kernel(const float* dY, const float* __restrict__ X, const float* __restrict__ stat,
                                                              const float* __restrict__ gamma, const double* __restrict__ sums, float* dX,
                                                              int N, int HW, int C, int G) {
  const int C4 = C / 4, cg = C / G;
  const double inv_m = 1.0 / ((double)HW * (double)cg);
  const long total = (long)N * HW * C4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const long p = i / C4;
    const int n = (int)(p / HW);
    const int gi = n * G + c / cg;
    const float mean = stat[2 * gi], rstd = stat[2 * gi + 1];
    const float m1 = (float)(sums[2 * gi] * inv_m), m2 = (float)(sums[2 * gi + 1] * inv_m);
    const float4 dy = ld4(dY + p * C + c), x = ld4(X + p * C + c), ga = ld4(gamma + c);
    float4 o;
    o.x = rstd * (ga.x * dy.x - (m1 + (x.x - mean) * rstd * m2));
    o.y = rstd * (ga.y * dy.y - (m1 + (x.y - mean) * rstd * m2));
    o.z = rstd * (ga.z * dy.z - (m1 + (x.z - mean) * rstd * m2));
    o.w = rstd * (ga.w * dy.w - (m1 + (x.w - mean) * rstd * m2));
    st4(dX + p * C + c, o);
  }
}

static unsigned it_ew_blocks(long total) {
  long b = (total + 255) / 256;
  return (unsigned)(b > 65535 ? 65535 : (b < 1 ? 1 : b));
}

static int it_loss_tiles(int H, int W, int rf) { return cdiv(H - rf, IT_TILE) * cdiv(W - 2 * rf, IT_TILE); }

static bool it_loss_geo_ok(int N, int H, int W, int radius, int nd) {
  const int rf = radius - 1;
  return N > 0 && N <= 65535 && radius >= 2 && rf <= IT_MAX_RF && nd > 0 && H - rf > 0 && W - 2 * rf > 0 && (long)H * W < (1L << 24);
}

extern "C" {

long mx_irn_loss_ws(int N, int H, int W, int radius) {
  if (!it_loss_geo_ok(N, H, W, radius, 1)) return -1;
  return (long)N * it_loss_tiles(H, W, radius - 1) * 8 * (long)sizeof(double);
}

int mx_irn_loss_fwd(const float* E, int lde, const float* D, int ldd, const unsigned char* label, const int* pts, const int* poff,
                    const int* plen, int nd, int radius, int N, int H, int W, unsigned char* amax, void* ws, long ws_bytes, double* res,
                    void* stream) {
  MX_CHECK_ARG(E && D && label && pts && poff && plen && amax && ws && res && lde >= 1 && ldd >= 2, "irn_loss_fwd: bad args");
  MX_CHECK_ARG(it_loss_geo_ok(N, H, W, radius, nd), "irn_loss_fwd: geometry N=%d H=%d W=%d radius=%d n_dst=%d", N, H, W, radius, nd);
  MX_CHECK_ARG(ws_bytes >= mx_irn_loss_ws(N, H, W, radius) && ((uintptr_t)ws & 7) == 0, "irn_loss_fwd: scratch too small");
  const int rf = radius - 1, tiles = it_loss_tiles(H, W, rf);
  const int halo = (IT_TILE + rf) * (IT_TILE + 2 * rf);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(it_loss_fwd_kernel, dim3(tiles, N), dim3(256), (size_t)halo * 13, st, E, lde, D, ldd, label, pts, poff, plen, nd, H, W,
                     rf, amax, (double*)ws);
  hipLaunchKernelGGL(it_loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, N * tiles, res);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_irn_loss_bwd(const float* E, int lde, const float* D, int ldd, const unsigned char* label, const int* pts, const int* poff,
                    const int* plen, int nd, int radius, int N, int H, int W, const unsigned char* amax, const double* res, float* dE,
                    float* dD, void* stream) {
  MX_CHECK_ARG(E && D && label && pts && poff && plen && amax && res && dE && dD && lde >= 1 && ldd >= 2, "irn_loss_bwd: bad args");
  MX_CHECK_ARG(it_loss_geo_ok(N, H, W, radius, nd), "irn_loss_bwd: geometry N=%d H=%d W=%d radius=%d n_dst=%d", N, H, W, radius, nd);
  MX_CHECK_ARG((((uintptr_t)dE | (uintptr_t)dD) & 15) == 0, "irn_loss_bwd: dE, dD must be 16-byte aligned");
  hipLaunchKernelGGL(it_loss_bwd_kernel, dim3(cdiv((long)H * W, 256), N), dim3(256), 0, (hipStream_t)stream, E, lde, D, ldd, label, pts,
                     poff, plen, nd, H, W, radius - 1, amax, res, dE, dD);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_gn_resize_bwd(const float* gdst, const float* fdst, float* dY, int N, int Hs, int Ws, int C, int scale, int Hd, int Wd, int ldd,
                     int coff, void* stream) {
  MX_CHECK_ARG(gdst && fdst && dY && N > 0 && Hs > 0 && Ws > 0 && C > 0 && C % 4 == 0, "gn_resize_bwd: bad args");
  MX_CHECK_ARG(scale == 1 || scale == 2 || scale == 4, "gn_resize_bwd: scale %d (1, 2 or 4)", scale);
  MX_CHECK_ARG(Hd > 0 && Wd > 0 && Hd <= Hs * scale && Wd <= Ws * scale, "gn_resize_bwd: the destination is a top-left crop of the up-sampled map");
  MX_CHECK_ARG(ldd % 4 == 0 && coff % 4 == 0 && coff >= 0 && coff + C <= ldd, "gn_resize_bwd: channel slice [%d, %d) of %d", coff, coff + C, ldd);
  hipLaunchKernelGGL(it_gn_resize_bwd_kernel, dim3(it_ew_blocks((long)N * Hs * Ws * (C / 4))), dim3(256), 0, (hipStream_t)stream, gdst,
                     fdst, dY, N, Hs, Ws, C, scale, Hd, Wd, ldd, coff);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

long mx_gn_bwd_ws(int N, int HW, int C, int G) {
  if (N <= 0 || HW <= 0 || C <= 0 || G <= 0) return -1;
  return ((long)N * it_gn_slices(HW) * C * 2 + (long)N * G * 2) * (long)sizeof(double);
}

int mx_gn_bwd(const float* dY, const float* X, const float* stat, const float* gamma, int N, int HW, int C, int G, void* ws, long ws_bytes,
              float* dX, float* dgamma, float* dbeta, void* stream) {
  MX_CHECK_ARG(dY && X && stat && gamma && ws && dX && dgamma && dbeta && N > 0 && HW > 0 && G > 0, "gn_bwd: bad args");
  MX_CHECK_ARG(C > 0 && C % 32 == 0 && C % G == 0 && (C / G) % 4 == 0, "gn_bwd: C %% 32 == 0 and (C / G) %% 4 == 0 (C=%d, G=%d)", C, G);
  MX_CHECK_ARG(N <= 65535, "gn_bwd: N <= 65535");
  MX_CHECK_ARG(ws_bytes >= mx_gn_bwd_ws(N, HW, C, G) && ((uintptr_t)ws & 7) == 0, "gn_bwd: scratch too small");
  const int S = it_gn_slices(HW), rows_per = cdiv(HW, S);
  double* part = (double*)ws;
  double* sums = part + (long)N * S * C * 2;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(it_gn_bwd_partial_kernel, dim3(C / 32, S, N), dim3(256), 0, st, dY, X, stat, HW, C, G, rows_per, part);
  hipLaunchKernelGGL(it_gn_bwd_finalize_kernel, dim3(cdiv(N * G + C, 64)), dim3(64), 0, st, (const double*)part, gamma, N, S, C, G, sums,
                     dgamma, dbeta);
  hipLaunchKernelGGL(it_gn_bwd_apply_kernel, dim3(it_ew_blocks((long)N * HW * (C / 4))), dim3(256), 0, st, dY, X, stat, gamma,
                     (const double*)sums, dX, N, HW, C, G);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
