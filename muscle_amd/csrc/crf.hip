// Dense CRF of segmentation inference (src/imutils.py:439-456, crf_inference): mean-field inference of the fully connected
// CRF of Kraehenbuehl & Koltun (Gaussian + bilateral Potts terms, symmetric normalisation), the model that the reference hands
// to pydensecrf.  pydensecrf filters on a permutohedral lattice; here the sums over j are evaluated exactly over a square
// window of half-width R_m = ceil(trunc * sxy_m) (include/muscle_hip.h states the model).
//
// One kernel does every dense sum: crf_msg_kernel is a tiled stencil-GEMM  D[i, l] = sum_j K[i, j] * B[j, l]  on
// v_mfma_f32_32x32x2_f32.  A workgroup (4 waves) owns 16 x 8 output pixels, a wave 32 of them (the M side of the MFMA);
// the window's source pixels are walked in 32 x 8 tiles staged in LDS: colours (r, g, b, r^2+g^2+b^2) and B[j, 0..31] =
// n(j) * Q_s[0..L-1, j] padded with zeros (pixel-major).  Per MFMA a lane computes ONE K[i, j] directly in the A-operand
// layout (lane -> i = lane & 31, j = pair's pixel lane >> 5):
//     K = exp2(-(s2 * (dx^2 + dy^2) + cb * |c_i - c_j|^2)),     s2 = log2(e) / (2 sxy^2), cb = log2(e) / (2 srgb^2)
// dx, dy and the colour distance are small integers, exact in fp32 (|c_i - c_j|^2 = |c_i|^2 + |c_j|^2 - 2 c_i . c_j), so the
// exponent carries three roundings and one v_exp_f32 per pair remains.  The sum of a source tile (128 chained MFMAs) is
// added to the running total per tile (blocked summation: the rounding error does not grow with the window's area).
// The same kernel with B = (1, 0, ...) gives the normalisers, with the colours switched off the Gaussian term.
// Epilogues: NORM -> n(i); STORE -> the weighted Gaussian message; FINAL -> -U + both messages, softmax over the labels,
// Q_{s+1}, and on the last iteration Q_t [L,H,W] / argmax.  No atomics, fixed order: same bits every run.
#include "common.h"
#include <math.h>

namespace {

constexpr int CRF_LP = 32;                  // labels padded to the MFMA's N
constexpr int CRF_MAXL = 24;
constexpr int CRF_TW = 16, CRF_TH = 8;      // output tile of a workgroup (4 waves x 32 pixels)
constexpr int CRF_SW = 32, CRF_SH = 8;      // source tile staged in LDS
constexpr int CRF_DS = 33;                  // row stride of the epilogue tile (bank-conflict free per-pixel walks)
typedef float crf_f32x16 __attribute__((ext_vector_type(16)));

enum { CRF_NORM = 0, CRF_STORE = 1, CRF_FINAL = 2 };

struct CrfMsgArgs {
  const float4* feat;    // [HW] (r, g, b, r^2+g^2+b^2); NULL: Gaussian kernel (no colour term)
  const float* src;      // [HW][32] Q_s (NORM: unused, B = (1, 0, ...))
  const float* nrm;      // [HW] n_m: scales the rows of src at staging time and the result (NORM: unused)
  int H, W, R, L;
  float s2, cb, w;
  float* n_out;          // NORM
  float* msg;            // STORE: written; FINAL: the Gaussian message, read
  const float* U;        // FINAL
  float* q_next;         // FINAL: [HW][32] or NULL
  float* q_out;          // FINAL: [L,H,W] or NULL
  unsigned char* pred;   // FINAL: [H,W] or NULL
};

// softmax over Dt[0..L-1] (stride 1) in place; returns the index of the first maximum of the RESULT
__device__ __forceinline__ int crf_softmax_row(float* d, int L) {
  float m = d[0];
  for (int l = 1; l < L; ++l) m = fmaxf(m, d[l]);
  float s = 0.f;
  for (int l = 0; l < L; ++l) { const float e = expf(d[l] - m); d[l] = e; s += e; }
  const float inv = 1.0f / s;
  int best = 0; float bv = -1.f;
  for (int l = 0; l < L; ++l) {
    const float q = d[l] * inv;
    d[l] = q;
    if (q > bv) { bv = q; best = l; }
  }
  return best;
}

template <int MODE>
__global__ __launch_bounds__(256) void crf_msg_kernel(const CrfMsgArgs a) {
  __shared__ float4 cs[CRF_SW * CRF_SH];
  __shared__ __attribute__((aligned(16))) float Bs[CRF_SW * CRF_SH * CRF_LP];     // 32 KB; the epilogue tile [128][33] afterwards
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, W = a.W, R = a.R;
  const int X0 = blockIdx.x * CRF_TW, Y0 = blockIdx.y * CRF_TH;
  const int li = lane & 31, kh = lane >> 5;
  const int xi = X0 + (li & 15), yi = Y0 + 2 * wave + (li >> 4);
  float ri = 0.f, gi = 0.f, bi = 0.f, ni = 0.f;
  if (a.feat) {                                           // lanes beyond the image borrow the border pixel (results dropped)
    const float4 f = a.feat[min(yi, H - 1) * W + min(xi, W - 1)];
    ri = -2.f * f.x; gi = -2.f * f.y; bi = -2.f * f.z; ni = f.w;
  }
  const float Rf = (float)R;
  const int xlo = max(0, X0 - R), xhi = min(W - 1, X0 + CRF_TW - 1 + R);
  const int ylo = max(0, Y0 - R), yhi = min(H - 1, Y0 + CRF_TH - 1 + R);

  crf_f32x16 tot;
#pragma unroll
  for (int r = 0; r < 16; ++r) tot[r] = 0.f;

  for (int ys = ylo; ys <= yhi; ys += CRF_SH) {
    for (int xs = xlo; xs <= xhi; xs += CRF_SW) {
      __syncthreads();                                    // the previous tile has been consumed
      {
        const int gx = xs + (tid & (CRF_SW - 1)), gy = ys + (tid >> 5);
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.feat && gx <= xhi && gy <= yhi) f = a.feat[gy * W + gx];
        cs[tid] = f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int idx = tid + 256 * k, p = idx >> 3, q = idx & 7;
        const int gx = xs + (p & (CRF_SW - 1)), gy = ys + (p >> 5);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gx <= xhi && gy <= yhi) {                     // xhi <= W-1, yhi <= H-1: inside the image
          if (MODE == CRF_NORM) {
            if (q == 0) v.x = 1.f;
          } else {
            const int pix = gy * W + gx;
            const float n = a.nrm[pix];
            v = ld4(a.src + (long)pix * CRF_LP + 4 * q);
            v.x *= n; v.y *= n; v.z *= n; v.w *= n;
          }
        }
        st4(Bs + p * CRF_LP + 4 * q, v);
      }
      __syncthreads();

      crf_f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float fdx0 = (float)(xs + kh - xi);
#pragma unroll 1
      for (int sy = 0; sy < CRF_SH; ++sy) {
        const int dy = ys + sy - yi;
        const float ty = (abs(dy) <= R) ? (float)(dy * dy) * a.s2 : INFINITY;      // rows outside the window: exp2(-inf) = 0
        const float4* crow = cs + sy * CRF_SW + kh;
        const float* brow = Bs + (sy * CRF_SW + kh) * CRF_LP + li;
#pragma unroll
        for (int pq = 0; pq < CRF_SW / 2; ++pq) {
          const float4 c = crow[2 * pq];
          const float b = brow[2 * pq * CRF_LP];
          const float fdx = fdx0 + (float)(2 * pq);
          float arg = fmaf(fdx * fdx, a.s2, ty);
          float d2 = ni + c.w;
          d2 = fmaf(ri, c.x, d2);
          d2 = fmaf(gi, c.y, d2);
          d2 = fmaf(bi, c.z, d2);
          arg = fmaf(d2, a.cb, arg);
          float kv = __builtin_amdgcn_exp2f(-arg);
          kv = (fabsf(fdx) <= Rf) ? kv : 0.f;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv, b, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) tot[r] += acc[r];
    }
  }

  // ---- epilogue: the workgroup's D tile [128 pixels][32 labels] through LDS
  __syncthreads();
  float* Dt = Bs;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;      // C/D layout of the 32x32 MFMA: col = lane & 31
    Dt[(wave * 32 + row) * CRF_DS + li] = tot[r];
  }
  __syncthreads();
  // pixel pw of the tile: x = X0 + (pw & 15), y = Y0 + (pw >> 4)
  if (MODE == CRF_NORM) {
    if (tid < 128) {
      const int x = X0 + (tid & 15), y = Y0 + (tid >> 4);
      if (x < W && y < H) a.n_out[y * W + x] = 1.0f / sqrtf(Dt[tid * CRF_DS] + 1e-20f);
    }
    return;
  }
  if (MODE == CRF_STORE) {
    for (int idx = tid; idx < 128 * CRF_LP; idx += 256) {
      const int pw = idx >> 5, l = idx & 31;
      const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
      if (x < W && y < H) {
        const int pix = y * W + x;
        a.msg[(long)pix * CRF_LP + l] = a.w * a.nrm[pix] * Dt[pw * CRF_DS + l];
      }
    }
    return;
  }
  // FINAL
  const int L = a.L;
  for (int idx = tid; idx < 128 * CRF_LP; idx += 256) {
    const int pw = idx >> 5, l = idx & 31;
    const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
    if (x < W && y < H && l < L) {
      const int pix = y * W + x;
      const long o = (long)pix * CRF_LP + l;
      Dt[pw * CRF_DS + l] = (a.msg[o] - a.U[o]) + a.w * a.nrm[pix] * Dt[pw * CRF_DS + l];
    }
  }
  __syncthreads();
  if (tid < 128) {
    const int x = X0 + (tid & 15), y = Y0 + (tid >> 4);
    if (x < W && y < H) {
      const int best = crf_softmax_row(Dt + tid * CRF_DS, L);
      if (a.pred) a.pred[y * W + x] = (unsigned char)best;
    }
  }
  __syncthreads();
  if (a.q_next) {
    for (int idx = tid; idx < 128 * CRF_LP; idx += 256) {
      const int pw = idx >> 5, l = idx & 31;
      const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
      if (x < W && y < H) a.q_next[(long)(y * W + x) * CRF_LP + l] = l < L ? Dt[pw * CRF_DS + l] : 0.f;
    }
  }
  if (a.q_out) {
    const long HW = (long)H * W;
    for (int idx = tid; idx < 128 * L; idx += 256) {
      const int l = idx >> 7, pw = idx & 127;
      const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
      if (x < W && y < H) a.q_out[l * HW + y * W + x] = Dt[pw * CRF_DS + l];
    }
  }
}

// uint8 [HW][3] -> (r, g, b, r^2 + g^2 + b^2), all exact in fp32
__global__ void crf_feat_kernel(const unsigned char* rgb, float4* feat, int HW) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HW) return;
  const float r = (float)rgb[3 * i], g = (float)rgb[3 * i + 1], b = (float)rgb[3 * i + 2];
  feat[i] = make_float4(r, g, b, r * r + g * g + b * b);
}

// U = -log(clip(confidence * p + (1 - confidence) / L, 1e-5, 1)), Q_0 = softmax(-U); U and Q_0 pixel-major [HW][32], zero padded
__global__ void crf_unary_kernel(const float* prob, int L, int HW, int W, float confidence, float* U, float* q0, float* q_out,
                                 unsigned char* pred) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HW) return;
  const float base = (1.0f - confidence) / (float)L;
  float d[CRF_MAXL];
#pragma unroll
  for (int l = 0; l < CRF_MAXL; ++l) {
    float u = 0.f;
    if (l < L) {
      const float c = fminf(fmaxf(confidence * prob[(long)l * HW + i] + base, 1e-5f), 1.0f);
      u = -logf(c);
    }
    U[(long)i * CRF_LP + l] = u;
    d[l] = -u;
  }
#pragma unroll
  for (int l = CRF_MAXL; l < CRF_LP; ++l) U[(long)i * CRF_LP + l] = 0.f;
  // softmax over the first L entries (fully unrolled with predicates: d stays in registers)
  float m = d[0];
#pragma unroll
  for (int l = 1; l < CRF_MAXL; ++l) if (l < L) m = fmaxf(m, d[l]);
  float s = 0.f;
#pragma unroll
  for (int l = 0; l < CRF_MAXL; ++l) if (l < L) { d[l] = expf(d[l] - m); s += d[l]; }
  const float inv = 1.0f / s;
  int best = 0; float bv = -1.f;
#pragma unroll
  for (int l = 0; l < CRF_MAXL; ++l) {
    float q = 0.f;
    if (l < L) {
      q = d[l] * inv;
      if (q > bv) { bv = q; best = l; }
      if (q_out) q_out[(long)l * HW + i] = q;
    }
    q0[(long)i * CRF_LP + l] = q;
  }
#pragma unroll
  for (int l = CRF_MAXL; l < CRF_LP; ++l) q0[(long)i * CRF_LP + l] = 0.f;
  if (pred) pred[i] = (unsigned char)best;
}

struct CrfWs {
  float4* feat; float* ng; float* nb; float* U; float* M; float* Q[2];
};

long crf_ws_floats(long HW) { return 4 * HW + 2 * HW + 4 * (long)CRF_LP * HW; }

CrfWs crf_carve(void* workspace, long HW) {
  CrfWs w;
  float* p = (float*)workspace;
  w.feat = (float4*)p; p += 4 * HW;
  w.U = p; p += CRF_LP * HW;
  w.M = p; p += CRF_LP * HW;
  w.Q[0] = p; p += CRF_LP * HW;
  w.Q[1] = p; p += CRF_LP * HW;
  w.ng = p; p += HW;
  w.nb = p;
  return w;
}

// half-width of the window: ceil(trunc * sxy), everything when trunc <= 0 or the window covers the image
int crf_radius(float trunc, float sxy, int H, int W) {
  const int all = (H > W ? H : W);
  if (!(trunc > 0.f)) return all;
  const double r = ceil((double)trunc * (double)sxy);
  return r >= (double)(all - 1) ? all : (int)r;
}

const float CRF_HALF_LOG2E = 0.72134752044448170368f;     // log2(e) / 2

template <int MODE>
void crf_launch_msg(CrfMsgArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(crf_msg_kernel<MODE>, dim3(cdiv(a.W, CRF_TW), cdiv(a.H, CRF_TH)), dim3(256), 0, st, a);
}

int crf_launch_normalizers(const unsigned char* rgb, int H, int W, float sxy_g, float sxy_b, float srgb, float trunc, const CrfWs& ws,
                           float* n_g, float* n_b, hipStream_t st) {
  const int HW = H * W;
  hipLaunchKernelGGL(crf_feat_kernel, dim3(cdiv(HW, 256)), dim3(256), 0, st, rgb, ws.feat, HW);
  MX_LAUNCH_CHECK();
  CrfMsgArgs a = {};
  a.H = H; a.W = W; a.L = 1;
  a.R = crf_radius(trunc, sxy_g, H, W); a.s2 = CRF_HALF_LOG2E / (sxy_g * sxy_g); a.cb = 0.f; a.n_out = n_g;
  crf_launch_msg<CRF_NORM>(a, st);
  MX_LAUNCH_CHECK();
  a.feat = ws.feat;
  a.R = crf_radius(trunc, sxy_b, H, W); a.s2 = CRF_HALF_LOG2E / (sxy_b * sxy_b); a.cb = CRF_HALF_LOG2E / (srgb * srgb); a.n_out = n_b;
  crf_launch_msg<CRF_NORM>(a, st);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // namespace

extern "C" {

#define CRF_MAX_PIXELS (1L << 24)

long mx_crf_workspace_bytes(int L, int H, int W) {
  if (!(L >= 1 && L <= CRF_MAXL && H > 0 && W > 0 && (long)H * W <= CRF_MAX_PIXELS)) {
    mx_set_error("crf_workspace_bytes: bad args L=%d (1..%d) H=%d W=%d (H*W <= 2^24)", L, CRF_MAXL, H, W);
    return MX_EARG;
  }
  return crf_ws_floats((long)H * W) * 4;
}

int mx_crf_normalizers(const unsigned char* rgb, int H, int W, float sxy_g, float sxy_b, float srgb, float trunc, void* workspace,
                       float* n_g, float* n_b, void* stream) {
  MX_CHECK_ARG(rgb && workspace && n_g && n_b, "crf_normalizers: null pointer");
  MX_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= CRF_MAX_PIXELS, "crf_normalizers: bad size H=%d W=%d (H*W in 1..2^24)", H, W);
  MX_CHECK_ARG(sxy_g > 0.f && sxy_b > 0.f && srgb > 0.f, "crf_normalizers: sxy_g=%g sxy_b=%g srgb=%g must be positive", sxy_g, sxy_b,
               srgb);
  MX_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "crf_normalizers: workspace must be 16-byte aligned");
  const CrfWs ws = crf_carve(workspace, (long)H * W);
  return crf_launch_normalizers(rgb, H, W, sxy_g, sxy_b, srgb, trunc, ws, n_g, n_b, (hipStream_t)stream);
}

int mx_crf_inference(const unsigned char* rgb, const float* prob, int L, int H, int W, int t, float confidence, float sxy_g, float w_g,
                     float sxy_b, float srgb, float w_b, float trunc, void* workspace, float* q_out, unsigned char* pred, void* stream) {
  MX_CHECK_ARG(rgb && prob && workspace, "crf_inference: null pointer (rgb, prob or workspace)");
  MX_CHECK_ARG(q_out || pred, "crf_inference: q_out and pred are both NULL");
  MX_CHECK_ARG(L >= 1 && L <= CRF_MAXL, "crf_inference: L=%d outside 1..%d", L, CRF_MAXL);
  MX_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= CRF_MAX_PIXELS, "crf_inference: bad size H=%d W=%d (H*W in 1..2^24)", H, W);
  MX_CHECK_ARG(t >= 0, "crf_inference: t=%d is negative", t);
  MX_CHECK_ARG(sxy_g > 0.f && sxy_b > 0.f && srgb > 0.f, "crf_inference: sxy_g=%g sxy_b=%g srgb=%g must be positive", sxy_g, sxy_b, srgb);
  MX_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "crf_inference: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  const CrfWs ws = crf_carve(workspace, HW);
  if (t > 0) {
    const int rc = crf_launch_normalizers(rgb, H, W, sxy_g, sxy_b, srgb, trunc, ws, ws.ng, ws.nb, st);
    if (rc != MX_OK) return rc;
  }
  hipLaunchKernelGGL(crf_unary_kernel, dim3(cdiv(HW, 256)), dim3(256), 0, st, prob, L, HW, W, confidence, ws.U, ws.Q[0],
                     t == 0 ? q_out : (float*)nullptr, t == 0 ? pred : (unsigned char*)nullptr);
  MX_LAUNCH_CHECK();
  for (int s = 0; s < t; ++s) {
    const bool last = s == t - 1;
    CrfMsgArgs a = {};
    a.H = H; a.W = W; a.L = L;
    a.src = ws.Q[s & 1];
    a.nrm = ws.ng; a.R = crf_radius(trunc, sxy_g, H, W); a.s2 = CRF_HALF_LOG2E / (sxy_g * sxy_g); a.cb = 0.f; a.w = w_g; a.msg = ws.M;
    crf_launch_msg<CRF_STORE>(a, st);
    MX_LAUNCH_CHECK();
    a.feat = ws.feat;
    a.nrm = ws.nb; a.R = crf_radius(trunc, sxy_b, H, W); a.s2 = CRF_HALF_LOG2E / (sxy_b * sxy_b); a.cb = CRF_HALF_LOG2E / (srgb * srgb);
    a.w = w_b; a.U = ws.U;
    a.q_next = last ? nullptr : ws.Q[(s + 1) & 1];
    a.q_out = last ? q_out : nullptr;
    a.pred = last ? pred : nullptr;
    crf_launch_msg<CRF_FINAL>(a, st);
    MX_LAUNCH_CHECK();
  }
  return MX_OK;
}

}  // extern "C"
