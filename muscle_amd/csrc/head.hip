// CAM head + PCM (pixel-correlation module) support kernels.
//
// Reference: MuSCLe.forward(cam='cam'/'pix') src/MuSCLe.py:237-279 and MuSCLe.PCM :213-223.
// The contractions (fc, CAM 1x1, fuse 1x1, f^T f, cam*aff) run on the MFMA GEMM (gemm.hip); this file
// holds what sits between them: bilinear(align_corners=True) resampling, the per-pixel L2
// normalisation, the affinity column normalisation and their adjoints.  Low-resolution head tensors
// are NHWC with the class dimension padded to a leading dimension that is a multiple of 4.
#include "common.h"
#include "eval_counts.h"

// one component of the bilinear value of the four taps a00 a01 a10 a11 (float4) at the weights wy, wx of bil_coord (common.h), into o
#define BIL(f) o.f = (1.f - wy) * ((1.f - wx) * a00.f + wx * a01.f) + wy * ((1.f - wx) * a10.f + wx * a11.f)

// dst[n,y,x,coff + c] = [relu] bilinear(src[n,:,:,c])   NHWC -> NHWC (channel slice of a wider tensor)
__global__ __launch_bounds__(256) void resize_nhwc_kernel(const float* src, float* dst, int N, int Hs, int Ws, int C, int Hd,
                                                          int Wd, int ldd, int coff, int relu) {
  const int c4n = C / 4;
  const long total = (long)N * Hd * Wd * c4n;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int c = (int)(i % c4n) * 4;
    long p = i / c4n;
    int x = (int)(p % Wd);
    long q = p / Wd;
    int y = (int)(q % Hd), n = (int)(q / Hd);
    int y0, y1, x0, x1;
    float wy, wx;
    bil_coord(y, Hs, Hd, y0, y1, wy);
    bil_coord(x, Ws, Wd, x0, x1, wx);
    const float* b = src + (long)n * Hs * Ws * C + c;
    float4 a00 = ld4(b + ((long)y0 * Ws + x0) * C), a01 = ld4(b + ((long)y0 * Ws + x1) * C);
    float4 a10 = ld4(b + ((long)y1 * Ws + x0) * C), a11 = ld4(b + ((long)y1 * Ws + x1) * C);
    float4 o;
    BIL(x); BIL(y); BIL(z); BIL(w);
    if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
    st4(dst + p * ldd + coff + c, o);
  }
}

// dst[n,k,Y,X] (NCHW, K classes) = bilinear(src[n,:,:,k]) with src NHWC of leading dimension lds
__global__ __launch_bounds__(256) void upsample_to_nchw_kernel(const float* src, float* dst, int N, int Hs, int Ws, int lds,
                                                               int K, int Hd, int Wd) {
  const long total = (long)N * K * Hd * Wd;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int x = (int)(i % Wd);
    long q = i / Wd;
    int y = (int)(q % Hd);
    q /= Hd;
    int k = (int)(q % K), n = (int)(q / K);
    int y0, y1, x0, x1;
    float wy, wx;
    bil_coord_rn(y, Hs, Hd, y0, y1, wy);
    bil_coord_rn(x, Ws, Wd, x0, x1, wx);
    const float* b = src + (long)n * Hs * Ws * lds + k;
    float a00 = b[((long)y0 * Ws + x0) * lds], a01 = b[((long)y0 * Ws + x1) * lds];
    float a10 = b[((long)y1 * Ws + x0) * lds], a11 = b[((long)y1 * Ws + x1) * lds];
    dst[i] = upsample_ac_value(a00, a01, a10, a11, wy, wx);   // common.h: the bits this kernel has always produced
  }
}

// adjoint of the above: gsrc[n,sy,sx,k] (+)= sum over destination pixels of weight * gdst[n,k,Y,X].
// One block per (n,k): separable, first along X into LDS [Hd][Ws], then along Y.
__global__ __launch_bounds__(256) void upsample_to_nchw_bwd_kernel(const float* gdst, float* gsrc, int N, int Hs, int Ws, int lds,
                                                                   int K, int Hd, int Wd, int accumulate) {
  extern __shared__ float t[];   // [Hd][Ws]
  const int nk = blockIdx.x, n = nk / K, k = nk % K;
  const float* g = gdst + (long)nk * Hd * Wd;
  const float sx = (Wd > 1) ? (float)(Ws - 1) / (float)(Wd - 1) : 0.f;
  const float sy = (Hd > 1) ? (float)(Hs - 1) / (float)(Hd - 1) : 0.f;
  // stage 1: gather along X: t[y][sxi] = sum over the destination columns whose footprint names source column sxi (weight 1-f when
  // floor(src) == sxi, f when it is sxi-1).  One owner per element, ascending x: same bits every run (it was an LDS-atomic scatter).
  for (int o = threadIdx.x; o < Hd * Ws; o += 256) {
    const int sxi = o % Ws, y = o / Ws;
    int xlo = 0, xhi = Wd - 1;
    if (sx > 0.f) {
      xlo = max(0, (int)floorf((float)(sxi - 1) / sx) - 1);
      xhi = min(Wd - 1, (int)ceilf((float)(sxi + 1) / sx) + 1);
    }
    float acc = 0.f;
    for (int x = xlo; x <= xhi; ++x) {
      int x0, x1;
      float wx;
      bil_coord(x, Ws, Wd, x0, x1, wx);
      const float v = g[y * Wd + x];
      if (x0 == sxi) acc += (1.f - wx) * v;
      if (x1 == sxi && x1 != x0) acc += wx * v;
    }
    t[o] = acc;
  }
  __syncthreads();
  (void)sx;
  // stage 2: gather along Y: source row i receives from dst rows with floor(src) == i (w 1-f) or i-1 (w f)
  for (int o = threadIdx.x; o < Hs * Ws; o += 256) {
    int sxi = o % Ws, syi = o / Ws;
    float acc = 0.f;
    // only destination rows whose source coordinate y*sy lies in (syi - 1, syi + 1) can name row syi (one row of margin
    // each side for the rounding of bil_coord); the rest of the 448 rows contributed exact zeros
    int ylo = 0, yhi = Hd - 1;
    if (sy > 0.f) {
      ylo = max(0, (int)floorf((float)(syi - 1) / sy) - 1);
      yhi = min(Hd - 1, (int)ceilf((float)(syi + 1) / sy) + 1);
    }
    for (int y = ylo; y <= yhi; ++y) {
      int y0, y1;
      float wy;
      bil_coord(y, Hs, Hd, y0, y1, wy);
      if (y0 == syi) acc += (1.f - wy) * t[y * Ws + sxi];
      if (y1 == syi && y1 != y0) acc += wy * t[y * Ws + sxi];
    }
    float* d = gsrc + (((long)n * Hs + syi) * Ws + sxi) * lds + k;
    *d = accumulate ? (*d + acc) : acc;
  }
}

// rows [R, C]: y = x / (||x||_2 + eps); saves the norm.  One wave per row.
__global__ __launch_bounds__(256) void row_l2norm_kernel(const float* x, float* y, float* nrm, long R, int C, float eps) {
  const int lane = threadIdx.x & 63;
  for (long r = blockIdx.x * 4L + (threadIdx.x >> 6); r < R; r += (long)gridDim.x * 4) {
    const float* p = x + r * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += p[c] * p[c];
    s = sqrtf(wave_sum(s));
    float inv = 1.f / (s + eps);
    for (int c = lane; c < C; c += 64) y[r * C + c] = p[c] * inv;
    if (lane == 0) nrm[r] = s;
  }
}

// backward of y = x/(n+eps): gx = gy/(n+eps) - (x/n) * (gy.x)/(n+eps)^2
__global__ __launch_bounds__(256) void row_l2norm_bwd_kernel(const float* x, const float* nrm, const float* gy, float* gx, long R,
                                                             int C, float eps) {
  const int lane = threadIdx.x & 63;
  for (long r = blockIdx.x * 4L + (threadIdx.x >> 6); r < R; r += (long)gridDim.x * 4) {
    const float* p = x + r * C;
    const float* g = gy + r * C;
    float d = 0.f;
    for (int c = lane; c < C; c += 64) d += p[c] * g[c];
    d = wave_sum(d);
    float n = nrm[r], inv = 1.f / (n + eps);
    float k = (n > 0.f) ? d * inv * inv / n : 0.f;
    for (int c = lane; c < C; c += 64) gx[r * C + c] = g[c] * inv - p[c] * k;
  }
}

// PCM tail.  T[b,j,0..L) = aff * camx with camx[:, :, K] == 1, so T[b,j,K] is the affinity row sum.
//   fwd : rv[b,j,k] = T[b,j,k] / (T[b,j,K] + eps)   (k < K; padding columns -> 0)
//   bwd : gT[b,j,k] = grv[b,j,k]*r ; gT[b,j,K] = -sum_k grv*T*r^2 ; r = 1/(T[b,j,K]+eps)
__global__ __launch_bounds__(256) void pcm_norm_kernel(const float* T, const float* grv, float* out, long rows, int L, int K,
                                                       float eps, int bwd) {
  for (long r = blockIdx.x * 256L + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
    const float* t = T + r * L;
    float inv = 1.f / (t[K] + eps);
    if (!bwd) {
      for (int k = 0; k < L; ++k) out[r * L + k] = (k < K) ? t[k] * inv : 0.f;
    } else {
      const float* g = grv + r * L;
      float acc = 0.f;
      for (int k = 0; k < K; ++k) { out[r * L + k] = g[k] * inv; acc += g[k] * t[k]; }
      out[r * L + K] = -acc * inv * inv;
      for (int k = K + 1; k < L; ++k) out[r * L + k] = 0.f;
    }
  }
}

// G2[b,i,j] = (gaff[b,i,j] + gaff[b,j,i]) * (aff[b,i,j] > 0): gradient of relu(f f^T) w.r.t. the symmetric product
__global__ __launch_bounds__(256) void sym_relu_grad_kernel(const float* gaff, const float* aff, float* out, int B, int n, int ld) {
  const long total = (long)B * n * ld;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int j = (int)(i % ld);
    long q = i / ld;
    int ii = (int)(q % n);
    long b = q / n;
    float v = 0.f;
    if (j < n && aff[i] > 0.f) v = gaff[i] + gaff[(b * n + j) * ld + ii];
    out[i] = v;
  }
}

// small elementwise helpers on flat fp32 arrays
//  op 0: out = alpha*a                 op 1: out = a + alpha*b
//  op 2: out = (y > 0) ? a (+ b) : 0   (relu backward; b optional, y given as third operand)
__global__ __launch_bounds__(256) void ew_kernel(int op, const float* a, const float* b, const float* y, float alpha, float* out,
                                                 long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float v;
    if (op == 0) v = alpha * a[i];
    else if (op == 1) v = a[i] + alpha * b[i];
    else v = (y[i] > 0.f) ? (a[i] + (b ? b[i] : 0.f)) : 0.f;
    out[i] = v;
  }
}

// X[n, hw, c] += alpha * v[n, c]   (backward of the global average pool)
__global__ __launch_bounds__(256) void bcast_add_kernel(float* X, const float* v, float alpha, long rows, int C, int rps) {
  const int c4n = C / 4;
  const long total = rows * c4n;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    long r = i / c4n;
    int c = (int)(i - r * c4n) * 4;
    float4 x = ld4(X + i * 4), a = ld4(v + (r / rps) * C + c);
    x.x += alpha * a.x; x.y += alpha * a.y; x.z += alpha * a.z; x.w += alpha * a.w;
    st4(X + i * 4, x);
  }
}


// ---------------------------------------------------------------------------
// infer_mcl.py:124-148 for one forward pass of the multi-scale / flip list, fused: the model's own
// F.interpolate(align_corners=True) from the 1/16 map to the pass's input size (Hs x Ws), the script's cv2.resize
// (bilinear, half-pixel centres, edge clamp) from there to the original image size (H x W), the un-flip of the odd
// passes and the running sum over passes, for the K-1 foreground channels.  src: one sample, NHWC [h,w,lds], channel 0
// is the background.  acc[k-1,Y,X] += value.  Neither the [21,Hs,Ws] nor the [H,W,21] intermediate exists.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float bil_lr(const float* b, int h, int w, int lds, int Hs, int Ws, int yy, int xx) {
  int y0, y1, x0, x1;
  float wy, wx;
  bil_coord(yy, h, Hs, y0, y1, wy);
  bil_coord(xx, w, Ws, x0, x1, wx);
  float a00 = b[((long)y0 * w + x0) * lds], a01 = b[((long)y0 * w + x1) * lds];
  float a10 = b[((long)y1 * w + x0) * lds], a11 = b[((long)y1 * w + x1) * lds];
  return (1.f - wy) * ((1.f - wx) * a00 + wx * a01) + wy * ((1.f - wx) * a10 + wx * a11);
}

// half-pixel source coordinate (cv2.resize INTER_LINEAR / torch align_corners=False): src = (dst+0.5)*in/out - 0.5, >= 0
__device__ __forceinline__ void hp_coord(int d, int in, int out, int& i0, int& i1, float& w1) {
  float s = ((float)d + 0.5f) * ((float)in / (float)out) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  w1 = s - i0;
}

__global__ __launch_bounds__(256) void infer_accum_kernel(const float* src, float* acc, int h, int w, int lds, int K, int Hs,
                                                          int Ws, int H, int W, int flip) {
  const long total = (long)(K - 1) * H * W;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int X = (int)(i % W);
    long q = i / W;
    int Y = (int)(q % H), k = (int)(q / H) + 1;
    int Xr = flip ? (W - 1 - X) : X;            // np.flip(axis=1) after the resize
    int y0, y1, x0, x1;
    float wy, wx;
    hp_coord(Y, Hs, H, y0, y1, wy);
    hp_coord(Xr, Ws, W, x0, x1, wx);
    const float* b = src + k;
    float a00 = bil_lr(b, h, w, lds, Hs, Ws, y0, x0), a01 = bil_lr(b, h, w, lds, Hs, Ws, y0, x1);
    float a10 = bil_lr(b, h, w, lds, Hs, Ws, y1, x0), a11 = bil_lr(b, h, w, lds, Hs, Ws, y1, x1);
    acc[i] += (1.f - wy) * ((1.f - wx) * a00 + wx * a01) + wy * ((1.f - wx) * a10 + wx * a11);
  }
}

// ---------------------------------------------------------------------------
// infer_seg.py:101-133 (minus the dense CRF) for one image, every pass of the multi-scale / flip list in ONE launch:
// per pass the model's F.interpolate(align_corners=True) of the 1/8 logits to the pass's input size Hs x Ws (the
// seg_map of cam='seg', :104), torch.softmax over the classes (:106), cv2.resize to the original H x W (half-pixel
// centres, edge clamp, :109), np.flip of the odd passes (:112); then np.mean over the passes (:117), the optional
// cls_label scale of channels 1..K-1 (:125) and np.argmax (:133, the first maximum wins).
// One thread per output pixel with the K running sums in registers.  The softmax couples the channels between the two
// resizes, so it is evaluated at each of the <= 4 source pixels of the pixel's half-pixel footprint, on the
// align_corners logits of bil_lr's / mx_upsample_to_nchw's formula, with 16-byte loads of the NHWC rows.
// A footprint corner of weight exactly 0 is skipped (it would add 0 * p).  The sum runs over passes in table order, then
// over corners (fixed order, no atomics: the same bits every run).  prob is stored channel-major, coalesced per channel.
// Measured bound by its arithmetic (<= 4 x npass softmaxes per output pixel), not by memory: 243 us for 12 passes of a
// 500 x 375 image with or without prob (profiles/seg_infer_bench.txt).
// ---------------------------------------------------------------------------
#define SEG_MAXK 24

// p[k] = softmax over k < K of the align_corners bilinear of src[:, :, k] at pixel (sy, sx) of the Hs x Ws map; 0 for k >= K
__device__ __forceinline__ void seg_softmax_at(const float* src, int h, int w, int lds, int K, int Hs, int Ws, int sy, int sx,
                                               float (&p)[SEG_MAXK]) {
  int y0, y1, x0, x1;
  float wy, wx;
  bil_coord(sy, h, Hs, y0, y1, wy);
  bil_coord(sx, w, Ws, x0, x1, wx);
  const float *r00 = src + ((long)y0 * w + x0) * lds, *r01 = src + ((long)y0 * w + x1) * lds;
  const float *r10 = src + ((long)y1 * w + x0) * lds, *r11 = src + ((long)y1 * w + x1) * lds;
#pragma unroll
  for (int q = 0; q < SEG_MAXK / 4; ++q) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q * 4 < K) {                         // quad q lies inside the row: K <= lds and lds % 4 == 0
      float4 a00 = ld4(r00 + q * 4), a01 = ld4(r01 + q * 4), a10 = ld4(r10 + q * 4), a11 = ld4(r11 + q * 4);
      BIL(x); BIL(y); BIL(z); BIL(w);
    }
    p[q * 4 + 0] = o.x; p[q * 4 + 1] = o.y; p[q * 4 + 2] = o.z; p[q * 4 + 3] = o.w;
  }
  float m = p[0];
#pragma unroll
  for (int k = 1; k < SEG_MAXK; ++k)
    if (k < K) m = fmaxf(m, p[k]);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < SEG_MAXK; ++k) {
    p[k] = (k < K) ? expf(p[k] - m) : 0.f;
    s += p[k];
  }
#pragma unroll
  for (int k = 0; k < SEG_MAXK; ++k) p[k] = p[k] / s;
}

// tab: npass x 8 int64 {address of the pass's [h,w,lds] logits, h, w, Hs, Ws, flip, 0, 0}
// BATCH (mx_seg_infer_batch): blockIdx.y is the image; column 6 of the table is the row's image, rows of other images are
// skipped, so an image's passes are summed in table order exactly as the single-image launch sums them; the mean divides by
// the image's own row count; cls / pred / prob are per image; with gt the (TP, P, T) counts of seg_confusion_kernel (eval.hip)
// are taken here with the same rule and flush (eval_counts.h).
template <bool BATCH>
__global__ __launch_bounds__(256) void seg_infer_kernel(const long* tab, int npass, int lds, int K, int H, int W,
                                                        const float* cls, unsigned char* pred, float* prob,
                                                        const unsigned char* gt, long long* counts) {
  const long HW = (long)H * W;
  __shared__ int sc[BATCH ? SEG_MAXK * 3 : 1];
  const int img = BATCH ? blockIdx.y : 0;
  int mine = npass;
  if (BATCH) {
    cls = cls ? cls + (long)img * K : nullptr;
    pred += img * HW;
    prob = prob ? prob + (long)img * K * HW : nullptr;
    gt = gt ? gt + img * HW : nullptr;
    mine = 0;
    for (int n = 0; n < npass; ++n) mine += (tab[n * 8 + 6] == img) ? 1 : 0;
    for (int i = threadIdx.x; i < K * 3; i += 256) sc[i] = 0;
    __syncthreads();
  }
  for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += (long)gridDim.x * 256) {
    const int X = (int)(i % W), Y = (int)(i / W);
    float acc[SEG_MAXK];
#pragma unroll
    for (int k = 0; k < SEG_MAXK; ++k) acc[k] = 0.f;
    for (int n = 0; n < npass; ++n) {
      const long* e = tab + n * 8;
      if (BATCH && e[6] != img) continue;
      const float* src = reinterpret_cast<const float*>(e[0]);
      const int h = (int)e[1], w = (int)e[2], Hs = (int)e[3], Ws = (int)e[4];
      const int Xr = e[5] ? (W - 1 - X) : X;          // np.flip(axis=1) after the resize
      int y0, y1, x0, x1;
      float wy, wx;
      hp_coord(Y, Hs, H, y0, y1, wy);
      hp_coord(Xr, Ws, W, x0, x1, wx);
      for (int c = 0; c < 4; ++c) {
        const float f = ((c & 2) ? wy : 1.f - wy) * ((c & 1) ? wx : 1.f - wx);
        if (f == 0.f) continue;
        float p[SEG_MAXK];
        seg_softmax_at(src, h, w, lds, K, Hs, Ws, (c & 2) ? y1 : y0, (c & 1) ? x1 : x0, p);
#pragma unroll
        for (int k = 0; k < SEG_MAXK; ++k) acc[k] += f * p[k];
      }
    }
    const float fn = (float)mine;
    float best = 0.f;
    int bk = 0;
#pragma unroll
    for (int k = 0; k < SEG_MAXK; ++k) {
      if (k < K) {
        float v = acc[k] / fn;
        if (cls && k > 0) v *= cls[k];
        if (prob) prob[(long)k * HW + i] = v;
        if (k == 0 || v > best) { best = v; bk = k; }
      }
    }
    pred[i] = (unsigned char)bk;
    if (BATCH && gt) {
      const int g = gt[i];
      __builtin_assume(bk < K);                      // a k of the loop above
      if (g < 255) eval_count(sc, 0, bk, g, K);
    }
  }
  if (BATCH && gt) {
    __syncthreads();
    eval_flush(sc, K * 3, counts);
  }
}

// infer_mcl.py:153-158 per channel (one workgroup each): clamp at 0, min / max over the image, zero what is below
// min + 1e-6, then (v - min - 1e-6) / (max - min + 1e-6).  In place.
__global__ __launch_bounds__(256) void infer_norm_kernel(float* acc, long HW) {
  __shared__ float smx[4], smn[4];
  float* a = acc + (long)blockIdx.x * HW;
  float mx = -3.4e38f, mn = 3.4e38f;
  for (long i = threadIdx.x; i < HW; i += 256) {
    float v = fmaxf(a[i], 0.f);
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
  }
  mx = wave_max(mx);
  mn = wave_min(mn);
  if ((threadIdx.x & 63) == 0) { smx[threadIdx.x >> 6] = mx; smn[threadIdx.x >> 6] = mn; }
  __syncthreads();
  mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
  const float lo = mn + 1e-6f, den = mx - mn + 1e-6f;
  for (long i = threadIdx.x; i < HW; i += 256) {
    float v = fmaxf(a[i], 0.f);
    if (v < lo) v = 0.f;
    a[i] = (v - mn - 1e-6f) / den;
  }
}

// ---------------------------------------------------------------------------
// infer_mcl.py:107-148 for one image in ONE launch: every pass of the multi-scale / flip list, both maps (raw CAM and
// SGC), only the channels the script keeps (the image's labels, :172-174).  Per output pixel, pass and kept channel the
// value is exactly infer_accum_kernel's: the hp_coord footprint of (Y, flip ? W-1-X : X), four bil_lr taps, the same
// blend; summed over passes in table order from 0.f in a register.  The footprint, the 4 x 4 low-res offsets and the six
// weights of a pass do not depend on the channel or the map: they are computed once per pixel and pass and shared by
// the CH channels x NMAP maps of the thread (infer_accum_kernel recomputes them per channel and launch).  Channel chunks
// of CH go to blockIdx.y.  No atomics, nothing is read back from out: the same bits every run.
// tab: npass x 8 int64 {address of the pass's CAM [h,w,lds], address of its SGC [h,w,lds], h, w, Hs, Ws, flip, 0};
// col0: table column of map 0 (0 = CAM first, 1 = SGC only).
// ---------------------------------------------------------------------------
// The bits must be infer_accum_kernel's, and hipcc contracts that kernel's a*b + c*d expressions into one rounded product
// and one fma, choosing WHICH product is rounded per expression (and leaving the last blend as two products and an add),
// as its --save-temps ISA shows.  A second kernel written with the same C expressions is contracted differently once the
// coordinates are hoisted, so the arithmetic is spelt out here with contraction off and explicit fmas, operation for
// operation as the old kernel executes it:
//   bil_coord: w1 = fma(scale, d, -i0) (i0 from the rounded product scale*d);   hp_coord: s = fma(d + 0.5, in/out, -0.5)
//   lerp_a(a, b, w) = fma(w, b, rn((1-w)*a)): every x-blend inside a tap, the y-blend of tap (y1,x0), the x-blend of row y0
//   lerp_b(a, b, w) = fma(1-w, a, rn(w*b)):   the y-blend of the other three taps, the x-blend of row y1
//   value = rn((1-wy)*R0) + rn(wy*R1)
// tests/test_gpu_cam_infer.py asserts the equality bit for bit; if a compiler change moves infer_accum_kernel's
// contraction, that test says so and this block is re-derived from the new ISA.
// lerp_a, lerp_b and blend_rows are in common.h (mx_upsample_to_nchw's value is built from the same three).
__device__ __forceinline__ void bil_coord_x(int d, int in, int out, int& i0, int& i1, float& w1) {
#pragma clang fp contract(off)
  float scale = (out > 1) ? (float)(in - 1) / (float)(out - 1) : 0.f;
  float s = scale * (float)d;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  w1 = __builtin_fmaf(scale, (float)d, -(float)i0);
}
__device__ __forceinline__ void hp_coord_x(int d, int in, int out, int& i0, int& i1, float& w1) {
#pragma clang fp contract(off)
  float s = __builtin_fmaf((float)d + 0.5f, (float)in / (float)out, -0.5f);
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  w1 = s - (float)i0;
}
// one align_corners tap of bil_lr from its four low-res corners; LERP_A: the y-blend of the tap at (y1, x0)
template <bool LERP_A>
__device__ __forceinline__ float bil_tap(const float* b, const int (&o)[4], float wy, float wx) {
  float r0 = lerp_a(b[o[0]], b[o[1]], wx), r1 = lerp_a(b[o[2]], b[o[3]], wx);
  return LERP_A ? lerp_a(r0, r1, wy) : lerp_b(r0, r1, wy);
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

template <int CH, int NMAP>
__global__ __launch_bounds__(256) void cam_infer_kernel(const long* tab, int npass, int lds, int H, int W, const int* keep,
                                                        int nkeep, int col0, float* out0, float* out1) {
  const long HW = (long)H * W;
  const int j0 = blockIdx.y * CH;
  int kc[CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) kc[j] = keep[min(j0 + j, nkeep - 1)] + 1;     // model channel (the index is clamped for the tail of the last chunk)
  for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += (long)gridDim.x * 256) {
    const int X = (int)(i % W), Y = (int)(i / W);
    float acc[NMAP][CH];
#pragma unroll
    for (int m = 0; m < NMAP; ++m)
#pragma unroll
      for (int j = 0; j < CH; ++j) acc[m][j] = 0.f;
    for (int n = 0; n < npass; ++n) {
      const long* e = tab + n * 8;
      const int h = (int)e[2], w = (int)e[3], Hs = (int)e[4], Ws = (int)e[5];
      const int Xr = e[6] ? (W - 1 - X) : X;            // np.flip(axis=1) after the resize
      int y0, y1, x0, x1;
      float wy, wx;
      hp_coord_x(Y, Hs, H, y0, y1, wy);
      hp_coord_x(Xr, Ws, W, x0, x1, wx);
      // bil_lr's coordinates of the footprint's two rows and two columns
      int r0[2], r1[2], c0[2], c1[2];
      float wr[2], wc[2];
      bil_coord_x(y0, h, Hs, r0[0], r1[0], wr[0]);
      bil_coord_x(y1, h, Hs, r0[1], r1[1], wr[1]);
      bil_coord_x(x0, w, Ws, c0[0], c1[0], wc[0]);
      bil_coord_x(x1, w, Ws, c0[1], c1[1], wc[1]);
      int o[2][2][4];                                    // [row of the footprint][column][low-res corner]
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          o[a][b][0] = (r0[a] * w + c0[b]) * lds; o[a][b][1] = (r0[a] * w + c1[b]) * lds;
          o[a][b][2] = (r1[a] * w + c0[b]) * lds; o[a][b][3] = (r1[a] * w + c1[b]) * lds;
        }
#pragma unroll
      for (int m = 0; m < NMAP; ++m) {
        const float* src = reinterpret_cast<const float*>(e[col0 + m]);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          if (j0 + j >= nkeep) continue;                 // uniform: the tail of the last chunk does no work
          const float* b = src + kc[j];
          float a00 = bil_tap<false>(b, o[0][0], wr[0], wc[0]), a01 = bil_tap<false>(b, o[0][1], wr[0], wc[1]);
          float a10 = bil_tap<true>(b, o[1][0], wr[1], wc[0]), a11 = bil_tap<false>(b, o[1][1], wr[1], wc[1]);
          acc[m][j] = add_rn(acc[m][j], blend_rows(lerp_a(a00, a01, wx), lerp_b(a10, a11, wx), wy));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (j0 + j < nkeep) {
        out0[(long)(j0 + j) * HW + i] = acc[0][j];
        if (NMAP > 1) out1[(long)(j0 + j) * HW + i] = acc[NMAP - 1][j];
      }
  }
}

static int gs(long n) { long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b)); }

// channels per thread of cam_infer_kernel: see the resource note in DESIGN.md (no scratch at 4 x 2 accumulators)
#define CAM_CH 4
template <int NMAP>
static void cam_infer_launch(const long* passes, int npass, int lds, int H, int W, const int* keep, int nkeep, int col0,
                             float* out0, float* out1, hipStream_t st) {
  const int bx = gs((long)H * W);
  hipLaunchKernelGGL((cam_infer_kernel<CAM_CH, NMAP>), dim3(bx, (nkeep + CAM_CH - 1) / CAM_CH), dim3(256), 0, st, passes, npass,
                     lds, H, W, keep, nkeep, col0, out0, out1);
}

extern "C" {

int mx_resize_nhwc(const float* src, float* dst, int N, int Hs, int Ws, int C, int Hd, int Wd, int ldd, int coff, int relu,
                   void* stream) {
  MX_CHECK_ARG(src && dst && N > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && C % 4 == 0 && ldd % 4 == 0 && coff % 4 == 0 &&
                   coff + C <= ldd, "resize_nhwc: bad args C=%d ldd=%d coff=%d", C, ldd, coff);
  hipLaunchKernelGGL(resize_nhwc_kernel, dim3(gs((long)N * Hd * Wd * (C / 4))), dim3(256), 0, (hipStream_t)stream, src, dst, N,
                     Hs, Ws, C, Hd, Wd, ldd, coff, relu);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_upsample_to_nchw(const float* src, float* dst, int N, int Hs, int Ws, int lds, int K, int Hd, int Wd, void* stream) {
  MX_CHECK_ARG(src && dst && N > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && K > 0 && K <= lds, "upsample_to_nchw: bad args");
  hipLaunchKernelGGL(upsample_to_nchw_kernel, dim3(gs((long)N * K * Hd * Wd)), dim3(256), 0, (hipStream_t)stream, src, dst, N,
                     Hs, Ws, lds, K, Hd, Wd);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_upsample_to_nchw_bwd(const float* gdst, float* gsrc, int N, int Hs, int Ws, int lds, int K, int Hd, int Wd,
                            int accumulate, void* stream) {
  MX_CHECK_ARG(gdst && gsrc && N > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && K > 0 && K <= lds, "upsample_to_nchw_bwd: bad args");
  size_t sh = (size_t)Hd * Ws * sizeof(float);
  MX_CHECK_ARG(sh <= 160 * 1024, "upsample_to_nchw_bwd: Hd*Ws=%d exceeds LDS", Hd * Ws);
  if (sh > 48 * 1024)
    hipFuncSetAttribute((const void*)upsample_to_nchw_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
  hipLaunchKernelGGL(upsample_to_nchw_bwd_kernel, dim3(N * K), dim3(256), sh, (hipStream_t)stream, gdst, gsrc, N, Hs, Ws, lds,
                     K, Hd, Wd, accumulate);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_row_l2norm(const float* x, float* y, float* nrm, long R, int C, float eps, void* stream) {
  MX_CHECK_ARG(x && y && nrm && R > 0 && C > 0, "row_l2norm: bad args");
  hipLaunchKernelGGL(row_l2norm_kernel, dim3(gs(R * 64)), dim3(256), 0, (hipStream_t)stream, x, y, nrm, R, C, eps);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_row_l2norm_bwd(const float* x, const float* nrm, const float* gy, float* gx, long R, int C, float eps, void* stream) {
  MX_CHECK_ARG(x && nrm && gy && gx && R > 0 && C > 0, "row_l2norm_bwd: bad args");
  hipLaunchKernelGGL(row_l2norm_bwd_kernel, dim3(gs(R * 64)), dim3(256), 0, (hipStream_t)stream, x, nrm, gy, gx, R, C, eps);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_pcm_norm(const float* T, const float* grv, float* out, long rows, int L, int K, float eps, int bwd, void* stream) {
  MX_CHECK_ARG(T && out && rows > 0 && K > 0 && K < L && (!bwd || grv), "pcm_norm: bad args");
  hipLaunchKernelGGL(pcm_norm_kernel, dim3(gs(rows)), dim3(256), 0, (hipStream_t)stream, T, grv, out, rows, L, K, eps, bwd);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_sym_relu_grad(const float* gaff, const float* aff, float* out, int B, int n, int ld, void* stream) {
  MX_CHECK_ARG(gaff && aff && out && B > 0 && n > 0 && ld >= n, "sym_relu_grad: bad args");
  hipLaunchKernelGGL(sym_relu_grad_kernel, dim3(gs((long)B * n * ld)), dim3(256), 0, (hipStream_t)stream, gaff, aff, out, B, n, ld);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_ew(int op, const float* a, const float* b, const float* y, float alpha, float* out, long n, void* stream) {
  MX_CHECK_ARG(a && out && n > 0 && op >= 0 && op <= 2, "ew: bad args");
  MX_CHECK_ARG(op != 1 || b, "ew: op 1 needs b");
  MX_CHECK_ARG(op != 2 || y, "ew: op 2 needs y");
  hipLaunchKernelGGL(ew_kernel, dim3(gs(n)), dim3(256), 0, (hipStream_t)stream, op, a, b, y, alpha, out, n);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_bcast_add(float* X, const float* v, float alpha, long rows, int C, int rows_per_sample, void* stream) {
  MX_CHECK_ARG(X && v && rows > 0 && C % 4 == 0 && rows_per_sample > 0, "bcast_add: bad args");
  hipLaunchKernelGGL(bcast_add_kernel, dim3(gs(rows * (C / 4))), dim3(256), 0, (hipStream_t)stream, X, v, alpha, rows, C,
                     rows_per_sample);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_infer_accum(const float* src, float* acc, int h, int w, int lds, int K, int Hs, int Ws, int H, int W, int flip, void* stream) {
  MX_CHECK_ARG(src && acc && h > 0 && w > 0 && K > 1 && K <= lds && Hs > 0 && Ws > 0 && H > 0 && W > 0, "infer_accum: bad args");
  hipLaunchKernelGGL(infer_accum_kernel, dim3(gs((long)(K - 1) * H * W)), dim3(256), 0, (hipStream_t)stream, src, acc, h, w, lds, K,
                     Hs, Ws, H, W, flip);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_infer_norm(float* acc, int channels, long HW, void* stream) {
  MX_CHECK_ARG(acc && channels > 0 && HW > 0, "infer_norm: bad args");
  hipLaunchKernelGGL(infer_norm_kernel, dim3(channels), dim3(256), 0, (hipStream_t)stream, acc, HW);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_seg_infer(const long* passes, int npass, int lds, int K, int H, int W, const float* cls_scale, unsigned char* pred,
                 float* prob, void* stream) {
  MX_CHECK_ARG(passes && pred && npass > 0 && K >= 1 && K <= SEG_MAXK && K <= lds && lds % 4 == 0 && H > 0 && W > 0,
               "seg_infer: bad args npass=%d K=%d lds=%d H=%d W=%d", npass, K, lds, H, W);
  hipLaunchKernelGGL(seg_infer_kernel<false>, dim3(gs((long)H * W)), dim3(256), 0, (hipStream_t)stream, passes, npass, lds, K, H,
                     W, cls_scale, pred, prob, (const unsigned char*)nullptr, (long long*)nullptr);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_seg_infer_batch(const long* rows, int nrow, int B, int lds, int K, int H, int W, const float* cls_scale, unsigned char* pred,
                       float* prob, const unsigned char* gt, long long* counts, void* stream) {
  MX_CHECK_ARG(rows && pred, "seg_infer_batch: NULL table or pred");
  MX_CHECK_ARG((gt == nullptr) == (counts == nullptr), "seg_infer_batch: gt and counts go together");
  MX_CHECK_ARG(B > 0 && B <= 65535 && nrow >= B && nrow <= 4096 && K >= 1 && K <= SEG_MAXK && K <= lds && lds % 4 == 0 && H > 0 &&
                   W > 0 && (long)B * K * H * W < (1L << 40),
               "seg_infer_batch: bad args nrow=%d B=%d K=%d lds=%d H=%d W=%d", nrow, B, K, lds, H, W);
  hipLaunchKernelGGL(seg_infer_kernel<true>, dim3(gs((long)H * W), B), dim3(256), 0, (hipStream_t)stream, rows, nrow, lds, K, H, W,
                     cls_scale, pred, prob, gt, counts);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_cam_infer(const long* passes, int npass, int lds, int K, int H, int W, const int* keep, int nkeep, float* out_cam,
                 float* out_sgc, void* stream) {
  MX_CHECK_ARG(passes && keep && (out_cam || out_sgc), "cam_infer: NULL table, keep list or both outputs NULL");
  MX_CHECK_ARG(npass > 0 && K > 1 && K <= lds && lds % 4 == 0 && H > 0 && W > 0 && nkeep > 0 && nkeep <= K - 1,
               "cam_infer: bad args npass=%d K=%d lds=%d H=%d W=%d nkeep=%d", npass, K, lds, H, W, nkeep);
  if (out_cam && out_sgc)
    cam_infer_launch<2>(passes, npass, lds, H, W, keep, nkeep, 0, out_cam, out_sgc, (hipStream_t)stream);
  else
    cam_infer_launch<1>(passes, npass, lds, H, W, keep, nkeep, out_cam ? 0 : 1, out_cam ? out_cam : out_sgc, nullptr,
                        (hipStream_t)stream);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
