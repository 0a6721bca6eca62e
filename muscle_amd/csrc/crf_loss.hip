// The dense-CRF energy loss of decoder training (include/muscle_hip.h states the model; it is ours, not the reference's): the
// normalised Potts energy of one bilateral kernel on the network's own softmax, pooled to 1/f resolution.
//
//   crf_loss_stage_kernel   one pass over seg and img: per low-resolution cell the softmax over K at its f x f pixels, the windowed
//                           means S and r as the pixel-major row [S_0 .. S_{K-1} | r | 0 ..] of 32 columns, and the mean colour
//   crf_msg_kernel<LOSS>    crf_msg.h: [M | Z] = K . [S | r], one MFMA stream of 32 columns for the whole batch (grid z = item); with r
//                           in column K the normaliser Z costs nothing.  Its epilogue leaves two double partials per workgroup
//   crf_loss_finish_kernel  adds the partials in index order: D, sum S . M, loss = (D - sum S . M) / D.  Nothing is read back
//   crf_loss_bwd_kernel     elementwise over [N,K,H,W]: the softmax again from seg, M at the pixel's cell, gseg
// No atomics anywhere; every sum has a fixed order.
#include "crf_msg.h"

namespace {

constexpr int CL_MAXK = CRF_MAXL;           // r needs column K: K <= 24 leaves it inside the 32
constexpr int CL_TPB = 256;

struct ClStageArgs {
  const float* seg;      // [N,K,H,W] logits
  const float* img;      // [N,3,H,W] normalised image
  const int* window;     // [N,4] (y0, x0, y1, x1) half-open, or NULL: the whole map
  int K, H, W, h, w;
  float* S;              // [N,h,w,32]
  float4* feat;          // [N,h,w]
};

__device__ __forceinline__ void cl_window(const int* window, int n, int H, int W, int& y0, int& x0, int& y1, int& x1) {
  y0 = 0; x0 = 0; y1 = H; x1 = W;
  if (window) { y0 = window[4 * n]; x0 = window[4 * n + 1]; y1 = window[4 * n + 2]; x1 = window[4 * n + 3]; }
}

// softmax over the first K of the logits of pixel p (stride HW) into q; everything stays in registers (K is a predicate)
__device__ __forceinline__ void cl_softmax(const float* seg, long HW, int K, float* q) {
  float m = seg[0];
#pragma unroll
  for (int l = 0; l < CL_MAXK; ++l) {
    q[l] = 0.f;
    if (l < K) { q[l] = seg[l * HW]; m = fmaxf(m, q[l]); }
  }
  float s = 0.f;
#pragma unroll
  for (int l = 0; l < CL_MAXK; ++l) if (l < K) { q[l] = expf(q[l] - m); s += q[l]; }
  const float inv = 1.0f / s;
#pragma unroll
  for (int l = 0; l < CL_MAXK; ++l) q[l] *= inv;
}

// rgb of a normalised value: clamp(rint((v * std + mean) * 255), 0, 255)
__device__ __forceinline__ float cl_rgb(float v, float sd, float mean) {
  return fminf(fmaxf(rintf(fmaf(v, sd, mean) * 255.f), 0.f), 255.f);
}

// A thread owns one full-resolution column of one low-resolution row: it walks the F pixels below each other, then the F lanes of
// a cell add up by xor shuffles (F divides W and 256, so a cell never straddles two workgroups or the map's edge) and the
// cell's first lane writes.  Loads are coalesced along x for every class.
template <int F>
__global__ __launch_bounds__(CL_TPB) void crf_loss_stage_kernel(const ClStageArgs a) {
  const int x = blockIdx.x * CL_TPB + threadIdx.x, Y = blockIdx.y, n = blockIdx.z;
  const int K = a.K, H = a.H, W = a.W;
  const long HW = (long)H * W;
  const bool on = x < W;
  int y0, x0, y1, x1;
  cl_window(a.window, n, H, W, y0, x0, y1, x1);
  float acc[CL_MAXK];
#pragma unroll
  for (int l = 0; l < CL_MAXK; ++l) acc[l] = 0.f;
  float rs = 0.f, cr = 0.f, cg = 0.f, cb = 0.f;
  if (on) {
    const bool inx = x >= x0 && x < x1;
    for (int dy = 0; dy < F; ++dy) {
      const int y = Y * F + dy;
      const long p = (long)y * W + x;
      const float* im = a.img + (long)n * 3 * HW + p;
      cr += cl_rgb(im[0], 0.229f, 0.485f);
      cg += cl_rgb(im[HW], 0.224f, 0.456f);
      cb += cl_rgb(im[2 * HW], 0.225f, 0.406f);
      if (inx && y >= y0 && y < y1) {
        float q[CL_MAXK];
        cl_softmax(a.seg + (long)n * K * HW + p, HW, K, q);
#pragma unroll
        for (int l = 0; l < CL_MAXK; ++l) acc[l] += q[l];
        rs += 1.f;
      }
    }
  }
#pragma unroll
  for (int o = 1; o < F; o <<= 1) {
#pragma unroll
    for (int l = 0; l < CL_MAXK; ++l) acc[l] += __shfl_xor(acc[l], o, 64);
    rs += __shfl_xor(rs, o, 64);
    cr += __shfl_xor(cr, o, 64); cg += __shfl_xor(cg, o, 64); cb += __shfl_xor(cb, o, 64);
  }
  if (!on || (threadIdx.x & (F - 1))) return;
  const float inv = 1.0f / (float)(F * F);                // a power of two: the means of the colours are exact
  const long cell = ((long)n * a.h + Y) * a.w + x / F;
  float row[CRF_LP];
#pragma unroll
  for (int l = 0; l < CRF_LP; ++l) {
    float v = 0.f;
    if (l < CL_MAXK && l < K) v = acc[l] * inv;
    else if (l == K) v = rs * inv;
    row[l] = v;
  }
#pragma unroll
  for (int l = 0; l < CRF_LP; l += 4) st4(a.S + cell * CRF_LP + l, make_float4(row[l], row[l + 1], row[l + 2], row[l + 3]));
  cr *= inv; cg *= inv; cb *= inv;
  a.feat[cell] = make_float4(cr, cg, cb, cr * cr + cg * cg + cb * cb);
}

// sums[0] = D, sums[1] = sum S . M (the partials in index order: 256 strided lane sums, then a fixed tree), loss = (D - sum S . M) / D,
// 0 where D == 0 (every window empty)
__global__ __launch_bounds__(CL_TPB) void crf_loss_finish_kernel(const double* part, long nparts, double* sums, float* loss) {
  __shared__ double sh[2 * CL_TPB];
  const int tid = threadIdx.x;
  double sd = 0.0, sm = 0.0;
  for (long i = tid; i < nparts; i += CL_TPB) { sd += part[2 * i]; sm += part[2 * i + 1]; }
  sh[tid] = sd; sh[CL_TPB + tid] = sm;
  __syncthreads();
  for (int o = CL_TPB / 2; o > 0; o >>= 1) {
    if (tid < o) { sh[tid] += sh[tid + o]; sh[CL_TPB + tid] += sh[CL_TPB + tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    const double D = sh[0], SM = sh[CL_TPB];
    sums[0] = D; sums[1] = SM;
    loss[0] = D > 0.0 ? (float)((D - SM) / D) : 0.f;
  }
}

struct ClBwdArgs {
  const float* seg; const int* window; const float* M; const double* sums; const float* g;
  int K, H, W, f, h, w;
  float* gseg;
};

// gseg[n,c,p] = g (-2 / (D f^2)) in(p) P_c(p) (M_c(u(p)) - sum_c' P_c'(p) M_c'(u(p))); every element is written
__global__ __launch_bounds__(CL_TPB) void crf_loss_bwd_kernel(const ClBwdArgs a) {
  const int x = blockIdx.x * CL_TPB + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  const int K = a.K, H = a.H, W = a.W;
  if (x >= W) return;
  const long HW = (long)H * W;
  const long p = (long)y * W + x;
  int y0, x0, y1, x1;
  cl_window(a.window, n, H, W, y0, x0, y1, x1);
  const double D = a.sums[0];
  const float coef = D > 0.0 ? (float)(-2.0 * (double)a.g[0] / (D * (double)(a.f * a.f))) : 0.f;
  float* out = a.gseg + (long)n * K * HW + p;
  float q[CL_MAXK];
#pragma unroll
  for (int l = 0; l < CL_MAXK; ++l) q[l] = 0.f;
  if (x >= x0 && x < x1 && y >= y0 && y < y1 && D > 0.0) {
    cl_softmax(a.seg + (long)n * K * HW + p, HW, K, q);
    const float* mrow = a.M + (((long)n * a.h + y / a.f) * a.w + x / a.f) * CRF_LP;
    float m[CL_MAXK];
#pragma unroll
    for (int l = 0; l < CL_MAXK; l += 4) {
      const float4 v = ld4(mrow + l);
      m[l] = v.x; m[l + 1] = v.y; m[l + 2] = v.z; m[l + 3] = v.w;
    }
    float dot = 0.f;
#pragma unroll
    for (int l = 0; l < CL_MAXK; ++l) if (l < K) dot = fmaf(q[l], m[l], dot);
#pragma unroll
    for (int l = 0; l < CL_MAXK; ++l) q[l] = coef * q[l] * (m[l] - dot);
  }
#pragma unroll
  for (int l = 0; l < CL_MAXK; ++l) if (l < K) out[l * HW] = q[l];
}

struct ClWs { float* S; float4* feat; double* part; long nparts; };

long cl_parts(int N, int h, int w) { return (long)N * cdiv(w, CRF_TW) * cdiv(h, CRF_TH); }

long cl_ws_bytes(int N, int h, int w) {
  const long cells = (long)N * h * w;
  return cells * CRF_LP * 4 + cells * 16 + cl_parts(N, h, w) * 16;
}

ClWs cl_carve(void* ws, int N, int h, int w) {
  const long cells = (long)N * h * w;
  ClWs c;
  c.S = (float*)ws;
  c.feat = (float4*)(c.S + cells * CRF_LP);
  c.part = (double*)(c.feat + cells);
  c.nparts = cl_parts(N, h, w);
  return c;
}

template <int F>
void cl_launch_stage(const ClStageArgs& a, int N, hipStream_t st) {
  hipLaunchKernelGGL(crf_loss_stage_kernel<F>, dim3(cdiv(a.W, CL_TPB), a.h, N), dim3(CL_TPB), 0, st, a);
}

}  // namespace

extern "C" {

#define CL_MAX_PIXELS (1L << 24)
#define CL_MAX_ITEMS 65535

#define CL_CHECK_SHAPE(name)                                                                                                       \
  MX_CHECK_ARG(N >= 1 && N <= CL_MAX_ITEMS, name ": N=%d outside 1..%d", N, CL_MAX_ITEMS);                                         \
  MX_CHECK_ARG(K >= 2 && K <= CL_MAXK, name ": K=%d outside 2..%d", K, CL_MAXK);                                                   \
  MX_CHECK_ARG(f == 1 || f == 2 || f == 4 || f == 8, name ": f=%d is not 1, 2, 4 or 8", f);                                        \
  MX_CHECK_ARG(H > 0 && W > 0 && H <= 65535 && (long)H * W <= CL_MAX_PIXELS, name ": bad size H=%d W=%d (H <= 65535, H*W in 1..2^24)", \
               H, W);                                                                                                              \
  MX_CHECK_ARG(H % f == 0 && W % f == 0, name ": H=%d W=%d are not multiples of f=%d", H, W, f)

long mx_crf_loss_ws(int N, int K, int H, int W, int f) {
  if (!(N >= 1 && N <= CL_MAX_ITEMS && K >= 2 && K <= CL_MAXK && (f == 1 || f == 2 || f == 4 || f == 8) && H > 0 && W > 0 &&
        H <= 65535 && (long)H * W <= CL_MAX_PIXELS && H % f == 0 && W % f == 0)) {
    mx_set_error("crf_loss_ws: bad args N=%d (1..%d) K=%d (2..%d) H=%d W=%d (H <= 65535, H*W <= 2^24, multiples of f) f=%d (1, 2, 4, 8)", N,
                 CL_MAX_ITEMS, K, CL_MAXK, H, W, f);
    return MX_EARG;
  }
  return cl_ws_bytes(N, H / f, W / f);
}

int mx_crf_loss_fwd(const float* seg, const float* img, const int* window, int N, int K, int H, int W, int f, float sxy, float srgb,
                    float trunc, void* ws, float* M, double* sums, float* loss, void* stream) {
  MX_CHECK_ARG(seg && img && ws && M && sums && loss, "crf_loss_fwd: null pointer (seg, img, ws, M, sums or loss)");
  CL_CHECK_SHAPE("crf_loss_fwd");
  MX_CHECK_ARG(sxy > 0.f && srgb > 0.f, "crf_loss_fwd: sxy=%g srgb=%g must be positive", sxy, srgb);
  MX_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)M & 15) == 0, "crf_loss_fwd: ws and M must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int h = H / f, w = W / f;
  const ClWs c = cl_carve(ws, N, h, w);
  ClStageArgs s = {};
  s.seg = seg; s.img = img; s.window = window; s.K = K; s.H = H; s.W = W; s.h = h; s.w = w; s.S = c.S; s.feat = c.feat;
  if (f == 1) cl_launch_stage<1>(s, N, st);
  else if (f == 2) cl_launch_stage<2>(s, N, st);
  else if (f == 4) cl_launch_stage<4>(s, N, st);
  else cl_launch_stage<8>(s, N, st);
  MX_LAUNCH_CHECK();
  const float sl = sxy / (float)f;                        // the kernel width in cells
  CrfMsgArgs a = {};
  a.feat = c.feat; a.src = c.S; a.H = h; a.W = w; a.L = K; a.G = 1;
  a.R = crf_radius(trunc, sl, h, w); a.s2 = CRF_HALF_LOG2E / (sl * sl); a.cb = CRF_HALF_LOG2E / (srgb * srgb);
  a.msg = M; a.part = c.part;
  hipLaunchKernelGGL((crf_msg_kernel<CRF_LOSS, CRF_U_PROB>), dim3(cdiv(w, CRF_TW), cdiv(h, CRF_TH), N), dim3(256), 0, st, a);
  MX_LAUNCH_CHECK();
  hipLaunchKernelGGL(crf_loss_finish_kernel, dim3(1), dim3(CL_TPB), 0, st, (const double*)c.part, c.nparts, sums, loss);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_crf_loss_bwd(const float* seg, const int* window, const float* M, const double* sums, const float* g, int N, int K, int H, int W,
                    int f, float* gseg, void* stream) {
  MX_CHECK_ARG(seg && M && sums && g && gseg, "crf_loss_bwd: null pointer (seg, M, sums, g or gseg)");
  CL_CHECK_SHAPE("crf_loss_bwd");
  MX_CHECK_ARG(((uintptr_t)M & 15) == 0, "crf_loss_bwd: M must be 16-byte aligned");
  ClBwdArgs b = {};
  b.seg = seg; b.window = window; b.M = M; b.sums = sums; b.g = g; b.K = K; b.H = H; b.W = W; b.f = f; b.h = H / f; b.w = W / f;
  b.gseg = gseg;
  hipLaunchKernelGGL(crf_loss_bwd_kernel, dim3(cdiv(W, CL_TPB), H, N), dim3(CL_TPB), 0, (hipStream_t)stream, b);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
