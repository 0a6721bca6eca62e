// The IRN edge / displacement network of infer_irn.py (src/backbones/resnet50_irn.py:215-232 on src/backbones/resnet50.py): the
// kernels the EfficientNet path never needed.  Dense 3x3 convolution on the fp32 matrix pipe, the 7x7 stem's patch gather,
// max-pool, the strided row gather of the down-sample branches, GroupNorm statistics, GroupNorm + half-pixel bilinear
// up-sampling + crop + ReLU into a channel slice, the CAM down-scaling and the finishing kernel.  Inference only.
// Everything is NHWC fp32, fixed summation order, no atomics: two forwards of the same input give the same bits.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// =====================================================================================================================
// Dense 3x3 convolution, padding 1, stride 1 / 2 (resnet50.py:24-25), implicit GEMM on v_mfma_f32_16x16x4_f32.
//
// rows = output pixels, K = 9 * Cin.  A workgroup owns a PH x 16 patch of output pixels of one sample and BN output channels.
// K is walked in chunks of 16 input channels; per chunk the halo tile of the input ((PH-1)*S+3 rows x 15*S+3 columns x 16
// channels) is staged ONCE in LDS and the nine taps read it at nine offsets - the input crosses HBM -> LDS once per chunk, not
// nine times.  A halo pixel is a row of 16 floats with row stride 20, the layout of gemm.hip's second-generation NT kernel:
// lane (l15, q) reads k = 4q..4q+3 of its pixel with one ds_read_b128 and feeds four consecutive MFMAs; the 16 lanes of a read
// group touch 16 consecutive pixels (stride 20 floats: conflict-free).  With stride 2 consecutive output pixels are two halo
// columns apart (stride 40 floats would be a 2-way conflict), so the even and the odd halo columns are stored as two planes: for a
// fixed tap the 16 pixels of a read group are again consecutive in one plane.
// The packed weight Wp[tap][Cout][Cin] (mx_conv3x3_pack, once per checkpoint load, BatchNorm scale folded in) gives per (chunk, tap)
// a [BN][16] slab with K contiguous, double-buffered through registers exactly like the GEMM's B operand.  The next chunk's halo is
// requested into registers while the nine taps of the current chunk run.
// Summation: one MFMA accumulator per chunk (9 taps x 16 channels = 144 terms), added to a running total per chunk - a blocked sum
// whose rounding error grows with sqrt(144) + Cin/16 instead of 9 Cin.  Exact fp32; does not follow mx_set_gemm_mode.
// The weight rows are the MFMA's first operand (as in gemm.hip), so a lane's four accumulator registers are four consecutive
// output channels of one pixel: bias, ReLU and a 16-byte NHWC store need no exchange.
// =====================================================================================================================
struct ConvArgs {
  const float* x; const float* w; const float* bias; float* y;
  int N, H, W, Ci, Co, Ho, Wo, relu, tiles_x, tiles_y;
};

template <int S, int PH, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void conv3x3_kernel(ConvArgs g) {
  constexpr int PW = 16, LS = 20;
  constexpr int HH = (PH - 1) * S + 3, HW = (PW - 1) * S + 3;       // halo tile
  constexpr int HP = (HW + 1) / 2;                                   // stride 2: columns per parity plane
  constexpr int HROW = S == 1 ? HW : 2 * HP;                         // halo pixels per LDS row
  constexpr int NPIX = HH * HW;
  constexpr int PA = (NPIX * 4 + 255) / 256;
  constexpr int TM = PH / WM, TN = BN / 16 / WN;
  static_assert(WM * WN == 4 && PH % WM == 0 && BN % (16 * WN) == 0 && BN * 4 <= 256, "tile shape");
  __shared__ __attribute__((aligned(16))) float As[HH * HROW * LS];
  __shared__ __attribute__((aligned(16))) float Bs[2 * BN * LS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int wm = wave / WN, wn = wave % WN;
  int sp = blockIdx.x;
  const int tx = sp % g.tiles_x; sp /= g.tiles_x;
  const int ty = sp % g.tiles_y;
  const int n = sp / g.tiles_y;
  const int oy0 = ty * PH, ox0 = tx * PW, n0 = blockIdx.y * BN;
  const int Ci = g.Ci;
  const float* X = g.x + (long)n * g.H * g.W * Ci;

  // halo movers: element e = tid + 256 i -> halo pixel e / 4, 16-byte channel chunk e % 4
  const int ck = (tid & 3) * 4;
  long a_off[PA];                      // offset of the pixel's channel 0 in X, -1 = outside the image (zero padding) or past the tile
  int a_lds[PA];
  float4 ra[PA], rb;
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    const int pix = (tid + 256 * i) >> 2;
    const int r = pix / HW, c = pix - r * HW;
    const int iy = oy0 * S - 1 + r, ix = ox0 * S - 1 + c;
    const bool in = pix < NPIX && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
    a_off[i] = in ? ((long)iy * g.W + ix) * Ci + ck : -1;
    const int pos = S == 1 ? r * HROW + c : r * HROW + (c & 1) * HP + (c >> 1);
    a_lds[i] = pix < NPIX ? pos * LS + ck : -1;
  }
  const int brow = tid >> 2;
  const bool okb = brow < BN && n0 + brow < g.Co;
  const float* pb = g.w + (long)(n0 + (okb ? brow : 0)) * Ci + ck;
  const long tap_stride = (long)g.Co * Ci;

  auto loadA = [&](int c0) {
    const bool kin = c0 + ck < Ci;
#pragma unroll
    for (int i = 0; i < PA; ++i) ra[i] = (a_off[i] >= 0 && kin) ? ld4(X + a_off[i] + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto storeA = [&]() {
#pragma unroll
    for (int i = 0; i < PA; ++i)
      if (a_lds[i] >= 0) st4(As + a_lds[i], ra[i]);
  };
  auto loadB = [&](int it) {
    const int c0 = (it / 9) * 16, t = it % 9;
    rb = (okb && c0 + ck < Ci) ? ld4(pb + t * tap_stride + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto storeB = [&](int buf) {
    if (brow < BN) st4(Bs + buf * BN * LS + brow * LS + ck, rb);
  };

  f32x4 acc[TM][TN], tot[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunk = (Ci + 15) / 16, nit = nchunk * 9;
  loadA(0);
  loadB(0);
  storeA();
  storeB(0);
  if (nit > 1) loadB(1);
  __syncthreads();
  for (int ch = 0; ch < nchunk; ++ch) {
    if (ch + 1 < nchunk) loadA((ch + 1) * 16);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int it = ch * 9 + t, cur = it & 1;
      if (it + 1 < nit) {
        storeB(cur ^ 1);
        if (it + 2 < nit) loadB(it + 2);
      }
      const int ky = t / 3, kx = t % 3;
      const float* bs = Bs + cur * BN * LS + (wn * TN * 16 + l15) * LS + 4 * q;
      f32x4 av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = (wm * TM + i) * S + ky;
        const int pos = S == 1 ? r * HROW + l15 + kx : r * HROW + (kx & 1) * HP + l15 + (kx >> 1);
        av[i] = *reinterpret_cast<const f32x4*>(As + pos * LS + 4 * q);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = *reinterpret_cast<const f32x4*>(bs + 16 * LS * j);
#pragma unroll
      for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[j][st], av[i][st], acc[i][j], 0, 0, 0);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) { tot[i][j] += acc[i][j]; acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if (ch + 1 < nchunk) {
      storeA();
      __syncthreads();
    }
  }

  const int ox = ox0 + l15;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * TN * 16 + 16 * j + 4 * q;
    if (col >= g.Co) continue;                                       // Co % 4 == 0: a lane's four channels are in or out together
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (g.bias) b = *reinterpret_cast<const f32x4*>(g.bias + col);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int oy = oy0 + wm * TM + i;
      if (oy >= g.Ho || ox >= g.Wo) continue;
      f32x4 v = tot[i][j] + b;
      if (g.relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
      *reinterpret_cast<f32x4*>(g.y + (((long)n * g.Ho + oy) * g.Wo + ox) * g.Co + col) = v;
    }
  }
}

template <int S, int PH, int BN, int WM, int WN>
static void conv_launch(ConvArgs g, hipStream_t st) {
  g.tiles_x = cdiv(g.Wo, 16);
  g.tiles_y = cdiv(g.Ho, PH);
  hipLaunchKernelGGL((conv3x3_kernel<S, PH, BN, WM, WN>), dim3((unsigned)(g.N * g.tiles_x * g.tiles_y), (unsigned)cdiv(g.Co, BN)),
                     dim3(256), 0, st, g);
}

// Wp[t][co][ci] = W[co][ci][t] * (scale ? scale[co] : 1)
__global__ __launch_bounds__(256) void conv3x3_pack_kernel(const float* __restrict__ W, const float* __restrict__ scale,
                                                           float* __restrict__ Wp, int Co, int Ci) {
  const long total = 9L * Co * Ci;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ci = (int)(i % Ci), co = (int)((i / Ci) % Co), t = (int)(i / ((long)Ci * Co));
    const float s = scale ? scale[co] : 1.f;
    Wp[i] = W[((long)co * Ci + ci) * 9 + t] * s;
  }
}

// =====================================================================================================================
// stem (resnet50.py:62,66), strided gather (resnet50.py:80-84)
// =====================================================================================================================
// out[(n,oy,ox)][ci*49 + ky*7 + kx] = img[n,ci,2oy-3+ky,2ox-3+kx], zero outside the H x W image: that one test is both the
// convolution's padding and the zero padding of the image up to crop_size (resnet50_irn.py:225); rows of 148 floats (147 + 0)
__global__ __launch_bounds__(256) void stem7_im2col_kernel(const float* __restrict__ img, float* __restrict__ out, int N, int H, int W,
                                                           int Ho, int Wo) {
  const long total = (long)N * Ho * Wo * 37;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int k4 = (int)(i % 37);
    const long row = i / 37;
    const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho), n = (int)(row / ((long)Wo * Ho));
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = k4 * 4 + e;
      const int ci = k / 49, r = k - ci * 49, ky = r / 7, kx = r - ky * 7;
      const int iy = 2 * oy - 3 + ky, ix = 2 * ox - 3 + kx;
      v[e] = (k < 147 && iy >= 0 && iy < H && ix >= 0 && ix < W) ? img[(((long)n * 3 + ci) * H + iy) * W + ix] : 0.f;
    }
    st4(out + row * 148 + k4 * 4, make_float4(v[0], v[1], v[2], v[3]));
  }
}

// MaxPool2d(3, 2, 1) on NHWC; the padding never wins (-inf)
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C,
                                                         int Ho, int Wo) {
  const int C4 = C / 4;
  const long total = (long)N * Ho * Wo * C4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const long p = i / C4;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), n = (int)(p / ((long)Wo * Ho));
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy - 1 + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox - 1 + kx;
        if (ix < 0 || ix >= W) continue;
        const float4 v = ld4(x + (((long)n * H + iy) * W + ix) * C + c);
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
      }
    }
    st4(y + p * C + c, m);
  }
}

// y[n,oy,ox,:] = x[n,2oy,2ox,:]: the rows a stride-2 1x1 convolution reads
__global__ __launch_bounds__(256) void gather_s2_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C,
                                                        int Ho, int Wo) {
  const int C4 = C / 4;
  const long total = (long)N * Ho * Wo * C4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const long p = i / C4;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), n = (int)(p / ((long)Wo * Ho));
    st4(y + p * C + c, ld4(x + (((long)n * H + 2 * oy) * W + 2 * ox) * C + c));
  }
}

// =====================================================================================================================
// GroupNorm (resnet50_irn.py:22-92): statistics, then normalise + half-pixel bilinear + crop + ReLU into a channel slice
// =====================================================================================================================
#define GN_MAX_SLICES 64

// grid (slices, G, N): fp64 sums of x and x^2 over this slice's rows of the group's C/G channels -> part[n][g][slice][2].
// Each thread adds its elements in index order, the wave butterfly and the four waves are added in a fixed order.
__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ X, int HW, int C, int ldx, int G, int rows_per,
                                                         double* __restrict__ part) {
  const int sl = blockIdx.x, gi = blockIdx.y, n = blockIdx.z;
  const int cg = C / G, cg4 = cg / 4;
  const int r0 = sl * rows_per, r1 = min(HW, r0 + rows_per);
  const float* base = X + (long)n * HW * ldx + gi * cg;
  double s = 0.0, ss = 0.0;
  const long total = (long)max(r1 - r0, 0) * cg4;
  for (long e = threadIdx.x; e < total; e += 256) {
    const int c4 = (int)(e % cg4);
    const long r = r0 + e / cg4;
    const float4 v = ld4(base + r * ldx + c4 * 4);
    s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    ss += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
  }
  __shared__ double sh[8];
  s = wave_sum_d(s); ss = wave_sum_d(ss);
  if ((threadIdx.x & 63) == 0) { sh[(threadIdx.x >> 6) * 2] = s; sh[(threadIdx.x >> 6) * 2 + 1] = ss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + (((long)n * G + gi) * gridDim.x + sl) * 2;
    o[0] = ((sh[0] + sh[2]) + sh[4]) + sh[6];
    o[1] = ((sh[1] + sh[3]) + sh[5]) + sh[7];
  }
}

// one thread per (n, g): slices in ascending order; mean and 1/sqrt(biased var + eps) (nn.GroupNorm)
__global__ __launch_bounds__(64) void gn_finalize_kernel(const double* __restrict__ part, int NG, int slices, double count, float eps,
                                                         float* __restrict__ stat) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= NG) return;
  double s = 0.0, ss = 0.0;
  for (int k = 0; k < slices; ++k) { s += part[((long)i * slices + k) * 2]; ss += part[((long)i * slices + k) * 2 + 1]; }
  const double mean = s / count;
  double var = ss / count - mean * mean;
  if (var < 0.0) var = 0.0;
  stat[2 * i] = (float)mean;
  stat[2 * i + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

// dst[n,y,x,coff+c] = [relu] bilinear_halfpixel_{x scale}( gamma*(src - mean)*rstd + beta )[y, x]   for y < Hd, x < Wd (the crop)
__global__ __launch_bounds__(256) void gn_resize_kernel(const float* __restrict__ src, const float* __restrict__ stat,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float* __restrict__ dst, int N, int Hs, int Ws, int C, int G, int scale, int Hd, int Wd,
                                                        int ldd, int coff, int relu) {
  const int C4 = C / 4, cg = C / G;
  const float rs = 1.f / (float)scale;
  const long total = (long)N * Hd * Wd * C4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const long p = i / C4;
    const int x = (int)(p % Wd), y = (int)((p / Wd) % Hd), n = (int)(p / ((long)Wd * Hd));
    const float mean = stat[2 * (n * G + c / cg)], rstd = stat[2 * (n * G + c / cg) + 1];      // cg % 4 == 0: one group per float4
    const float4 ga = ld4(gamma + c), be = ld4(beta + c);
    const float4 a = make_float4(ga.x * rstd, ga.y * rstd, ga.z * rstd, ga.w * rstd);
    auto nrm = [&](int yy, int xx) {
      float4 v = ld4(src + (((long)n * Hs + yy) * Ws + xx) * C + c);
      v.x = (v.x - mean) * a.x + be.x; v.y = (v.y - mean) * a.y + be.y;
      v.z = (v.z - mean) * a.z + be.z; v.w = (v.w - mean) * a.w + be.w;
      return v;
    };
    float4 o;
    if (scale == 1) {
      o = nrm(y, x);
    } else {
      int y0, y1, x0, x1;
      float ly, lx;
      halfpixel_tap(y, rs, Hs, y0, y1, ly);
      halfpixel_tap(x, rs, Ws, x0, x1, lx);
      const float hy = 1.f - ly, hx = 1.f - lx;
      const float4 v00 = nrm(y0, x0), v01 = nrm(y0, x1), v10 = nrm(y1, x0), v11 = nrm(y1, x1);
      o.x = hy * (hx * v00.x + lx * v01.x) + ly * (hx * v10.x + lx * v11.x);
      o.y = hy * (hx * v00.y + lx * v01.y) + ly * (hx * v10.y + lx * v11.y);
      o.z = hy * (hx * v00.z + lx * v01.z) + ly * (hx * v10.z + lx * v11.z);
      o.w = hy * (hx * v00.w + lx * v01.w) + ly * (hx * v10.w + lx * v11.w);
    }
    if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
    st4(dst + p * ldd + coff + c, o);
  }
}

// dst[c,y,x] = bilinear_halfpixel(src[c]) (infer_irn.py:76, F.interpolate(size=..., align_corners=False), no antialiasing)
__global__ __launch_bounds__(256) void planar_resize_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int Hs, int Ws,
                                                            int Hd, int Wd) {
  const float ry = (float)Hs / (float)Hd, rx = (float)Ws / (float)Wd;
  const long total = (long)C * Hd * Wd;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int x = (int)(i % Wd), y = (int)((i / Wd) % Hd), c = (int)(i / ((long)Wd * Hd));
    int y0, y1, x0, x1;
    float ly, lx;
    halfpixel_tap(y, ry, Hs, y0, y1, ly);
    halfpixel_tap(x, rx, Ws, x0, x1, lx);
    const float* s = src + (long)c * Hs * Ws;
    const float hy = 1.f - ly, hx = 1.f - lx;
    dst[i] = hy * (hx * s[(long)y0 * Ws + x0] + lx * s[(long)y0 * Ws + x1]) + ly * (hx * s[(long)y1 * Ws + x0] + lx * s[(long)y1 * Ws + x1]);
  }
}

// resnet50_irn.py:227-230 + :107: crop, edge = sigmoid(e[0]/2 + flip_x(e[1])/2), dp = d[0] - running_mean
__global__ __launch_bounds__(256) void irn_net_finish_kernel(const float* __restrict__ e, int lde, const float* __restrict__ d, int ldd,
                                                             const float* __restrict__ mean, int Hf, int Wf, int h, int w,
                                                             float* __restrict__ edge, float* __restrict__ dp) {
  const long total = (long)h * w;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int x = (int)(i % w), y = (int)(i / w);
    const float e0 = e[((long)y * Wf + x) * lde];
    const float e1 = e[((long)Hf * Wf + (long)y * Wf + (w - 1 - x)) * lde];
    const float z = e0 / 2.f + e1 / 2.f;
    edge[i] = 1.f / (1.f + expf(-z));
    dp[i] = d[((long)y * Wf + x) * ldd] - mean[0];
    dp[total + i] = d[((long)y * Wf + x) * ldd + 1] - mean[1];
  }
}

static unsigned ew_blocks(long total) {
  long b = (total + 255) / 256;
  return (unsigned)(b > 65535 ? 65535 : (b < 1 ? 1 : b));
}

extern "C" {

int mx_conv3x3_pack(const float* W, const float* scale, float* Wp, int Co, int Ci, void* stream) {
  MX_CHECK_ARG(W && Wp && Co > 0 && Ci > 0, "conv3x3_pack: bad args");
  hipLaunchKernelGGL(conv3x3_pack_kernel, dim3(ew_blocks(9L * Co * Ci)), dim3(256), 0, (hipStream_t)stream, W, scale, Wp, Co, Ci);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_conv3x3_fwd(const float* X, const float* Wp, const float* bias, float* Y, int N, int H, int W, int Ci, int Co, int stride,
                   int relu, void* stream) {
  MX_CHECK_ARG(X && Wp && Y && N > 0 && H > 0 && W > 0, "conv3x3_fwd: bad args");
  MX_CHECK_ARG(Ci > 0 && Co > 0 && Ci % 4 == 0 && Co % 4 == 0, "conv3x3_fwd: Cin and Cout must be multiples of 4 (got %d, %d)", Ci, Co);
  MX_CHECK_ARG(stride == 1 || stride == 2, "conv3x3_fwd: stride %d (1 or 2)", stride);
  ConvArgs g;
  g.x = X; g.w = Wp; g.bias = bias; g.y = Y;
  g.N = N; g.H = H; g.W = W; g.Ci = Ci; g.Co = Co; g.relu = relu;
  g.Ho = (H - 1) / stride + 1; g.Wo = (W - 1) / stride + 1;
  g.tiles_x = g.tiles_y = 0;
  hipStream_t st = (hipStream_t)stream;
  // 8 x 16 pixels x 64 channels where that still gives every CU a workgroup, else 4 x 16 x 32 (the 32 x 32 layers: 2 048 pixels)
  const long big = (long)N * cdiv(g.Wo, 16) * cdiv(g.Ho, 8) * cdiv(Co, 64);
  const long mid = (long)N * cdiv(g.Wo, 16) * cdiv(g.Ho, 4) * cdiv(Co, 64);
  if (stride == 1) {
    if (big >= 256) conv_launch<1, 8, 64, 2, 2>(g, st);
    else if (mid >= 256) conv_launch<1, 4, 64, 2, 2>(g, st);
    else conv_launch<1, 4, 32, 2, 2>(g, st);
  } else {
    if (mid >= 256) conv_launch<2, 4, 64, 2, 2>(g, st);
    else conv_launch<2, 4, 32, 2, 2>(g, st);
  }
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_stem7_im2col(const float* img, float* out, int N, int H, int W, int Ho, int Wo, void* stream) {
  MX_CHECK_ARG(img && out && N > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "stem7_im2col: bad args");
  hipLaunchKernelGGL(stem7_im2col_kernel, dim3(ew_blocks((long)N * Ho * Wo * 37)), dim3(256), 0, (hipStream_t)stream, img, out, N, H, W,
                     Ho, Wo);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_maxpool3s2(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  MX_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "maxpool3s2: bad args");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3(ew_blocks((long)N * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W,
                     C, Ho, Wo);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_gather_s2(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  MX_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "gather_s2: bad args");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(gather_s2_kernel, dim3(ew_blocks((long)N * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C,
                     Ho, Wo);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

static int gn_slices(int HW) {
  int s = cdiv(HW, 512);
  return s < 1 ? 1 : (s > GN_MAX_SLICES ? GN_MAX_SLICES : s);
}

long mx_gn_stats_ws(int N, int HW, int G) {
  if (N <= 0 || HW <= 0 || G <= 0) return -1;
  return (long)N * G * gn_slices(HW) * 2 * (long)sizeof(double);
}

int mx_gn_stats(const float* X, int N, int HW, int C, int ldx, int G, float eps, void* ws, long ws_bytes, float* stat, void* stream) {
  MX_CHECK_ARG(X && ws && stat && N > 0 && HW > 0 && C > 0 && G > 0 && ldx >= C && ldx % 4 == 0, "gn_stats: bad args");
  MX_CHECK_ARG(C % G == 0 && (C / G) % 4 == 0, "gn_stats: C / G must be a multiple of 4 (C=%d, G=%d)", C, G);
  MX_CHECK_ARG(N <= 65535 && G <= 65535, "gn_stats: N, G <= 65535");
  MX_CHECK_ARG(ws_bytes >= mx_gn_stats_ws(N, HW, G), "gn_stats: scratch too small");
  const int sl = gn_slices(HW), rows_per = cdiv(HW, sl);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_partial_kernel, dim3(sl, G, N), dim3(256), 0, st, X, HW, C, ldx, G, rows_per, (double*)ws);
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(cdiv(N * G, 64)), dim3(64), 0, st, (const double*)ws, N * G, sl,
                     (double)HW * (double)(C / G), eps, stat);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_gn_resize(const float* src, const float* stat, const float* gamma, const float* beta, float* dst, int N, int Hs, int Ws, int C,
                 int G, int scale, int Hd, int Wd, int ldd, int coff, int relu, void* stream) {
  MX_CHECK_ARG(src && stat && gamma && beta && dst && N > 0 && Hs > 0 && Ws > 0 && C > 0 && G > 0, "gn_resize: bad args");
  MX_CHECK_ARG(C % G == 0 && (C / G) % 4 == 0, "gn_resize: C / G must be a multiple of 4 (C=%d, G=%d)", C, G);
  MX_CHECK_ARG(scale == 1 || scale == 2 || scale == 4, "gn_resize: scale %d (1, 2 or 4)", scale);
  MX_CHECK_ARG(Hd > 0 && Wd > 0 && Hd <= Hs * scale && Wd <= Ws * scale, "gn_resize: the output is a top-left crop of the up-sampled map");
  MX_CHECK_ARG(ldd % 4 == 0 && coff % 4 == 0 && coff >= 0 && coff + C <= ldd, "gn_resize: channel slice [%d, %d) of %d", coff, coff + C, ldd);
  hipLaunchKernelGGL(gn_resize_kernel, dim3(ew_blocks((long)N * Hd * Wd * (C / 4))), dim3(256), 0, (hipStream_t)stream, src, stat, gamma,
                     beta, dst, N, Hs, Ws, C, G, scale, Hd, Wd, ldd, coff, relu);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_resize_planar_halfpixel(const float* src, float* dst, int C, int Hs, int Ws, int Hd, int Wd, void* stream) {
  MX_CHECK_ARG(src && dst && C > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, "resize_planar_halfpixel: bad args");
  hipLaunchKernelGGL(planar_resize_kernel, dim3(ew_blocks((long)C * Hd * Wd)), dim3(256), 0, (hipStream_t)stream, src, dst, C, Hs, Ws, Hd,
                     Wd);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_irn_net_finish(const float* e, int lde, const float* d, int ldd, const float* mean, int Hf, int Wf, int h, int w, float* edge,
                      float* dp, void* stream) {
  MX_CHECK_ARG(e && d && mean && edge && dp && lde >= 1 && ldd >= 2, "irn_net_finish: bad args");
  MX_CHECK_ARG(h > 0 && w > 0 && h <= Hf && w <= Wf, "irn_net_finish: crop %d x %d of a %d x %d frame", h, w, Hf, Wf);
  hipLaunchKernelGGL(irn_net_finish_kernel, dim3(ew_blocks((long)h * w)), dim3(256), 0, (hipStream_t)stream, e, lde, d, ldd, mean, Hf, Wf,
                     h, w, edge, dp);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
