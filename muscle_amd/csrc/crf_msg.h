// crf_msg_kernel, the tiled stencil-GEMM of the windowed dense CRFs (crf.hip describes the tile scheme and the epilogues NORM,
// STORE and FINAL), in a header so that the dense-CRF energy loss (crf_loss.hip) runs its message pass on the same text:
// epilogue LOSS, a batch of images on grid z, no normalisers.  Everything LOSS adds sits behind `MODE == CRF_LOSS`, a template
// constant: the other instantiations compile to the arithmetic they had before the kernel moved here.
#pragma once
#include "common.h"
#include "crf_model.h"
#include <math.h>

namespace {

constexpr int CRF_LP = 32;                  // columns: the MFMA's N
constexpr int CRF_MAXL = 24;                // probability unary
constexpr int CRF_LABEL_MAXL = 21;          // label unary: background + the 20 VOC classes
constexpr int CRF_FUSE_L = 16;              // two problems fit the 32 columns up to here
constexpr int CRF_TW = 16, CRF_TH = 8;      // output tile of a workgroup (4 waves x 32 pixels)
constexpr int CRF_SW = 32, CRF_SH = 8;      // source tile staged in LDS
constexpr int CRF_DS = 33;                  // row stride of the epilogue tile (bank-conflict free per-pixel walks)
typedef float crf_f32x16 __attribute__((ext_vector_type(16)));

enum { CRF_NORM = 0, CRF_STORE = 1, CRF_FINAL = 2, CRF_LOSS = 3 };
enum { CRF_U_PROB = 0, CRF_U_LABEL = 1 };   // the unary of FINAL

struct CrfMsgArgs {
  const float4* feat;    // [HW] (r, g, b, r^2+g^2+b^2); NULL: Gaussian kernel (no colour term)
  const float* src;      // [HW][32] Q_s (NORM: unused, B = (1, 0, ...)); columns >= G*L are zero
  const float* nrm;      // [HW] n_m: scales the rows of src at staging time and the result (NORM: unused)
  int H, W, R, L, G, g0; // this launch carries problems g0 .. g0+G-1 in columns 0 .. G*L-1
  float s2, cb, w;
  float* n_out;          // NORM
  float* msg;            // STORE: written; FINAL: the Gaussian message, read
  const float* U;        // FINAL, U_PROB: [HW][32]
  const unsigned char* lab;   // FINAL, U_LABEL: [2][HW] the problems' label maps (255: a label outside 0..L-1, no own column)
  float u_own, u_oth;    // FINAL, U_LABEL: the two unary energies
  float* q_next;         // FINAL: [HW][32] or NULL
  int last;              // FINAL: the last step, which writes the results below
  float* q_out;          // [2][L][H][W] (one problem: [L,H,W]) or NULL
  unsigned char* pred;   // [2][HW] (one problem: [H,W]) argmax per problem, or NULL
  unsigned char* pred_ws;     // U_LABEL: [2][HW] argmax per problem (workspace; the second pass reads the first's)
  const int* keys;       // U_LABEL: [L] (with conf)
  unsigned char* conf;   // U_LABEL: [HW] or NULL
  // LOSS (grid z = batch item n; feat, src and msg are [N][HW].. and the kernel steps them by n): src = [S | r] with r in column L,
  // unscaled; msg = [M | Z], written; the colours are means over a cell, no integers, so the colour distance is formed from
  // differences; part [blocks][2]: the workgroup's sums of r Z and of S . M, in double
  double* part;
};

template <int MODE, int UNARY>
__global__ __launch_bounds__(256) void crf_msg_kernel(const CrfMsgArgs a) {
  __shared__ float4 cs[CRF_SW * CRF_SH];
  __shared__ __attribute__((aligned(16))) float Bs[CRF_SW * CRF_SH * CRF_LP];     // 32 KB; the epilogue tile [128][33] afterwards
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, W = a.W, R = a.R;
  const int X0 = blockIdx.x * CRF_TW, Y0 = blockIdx.y * CRF_TH;
  const int li = lane & 31, kh = lane >> 5;
  const int xi = X0 + (li & 15), yi = Y0 + 2 * wave + (li >> 4);
  const float4* feat = a.feat;
  const float* src = a.src;
  if (MODE == CRF_LOSS) {                                 // this workgroup's image of the batch
    const long boff = (long)blockIdx.z * H * W;
    feat += boff; src += boff * CRF_LP;
  }
  float ri = 0.f, gi = 0.f, bi = 0.f, ni = 0.f;
  if (feat) {                                             // lanes beyond the image borrow the border pixel (results dropped)
    const float4 f = feat[min(yi, H - 1) * W + min(xi, W - 1)];
    if (MODE == CRF_LOSS) { ri = f.x; gi = f.y; bi = f.z; }
    else { ri = -2.f * f.x; gi = -2.f * f.y; bi = -2.f * f.z; ni = f.w; }
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
        if (feat && gx <= xhi && gy <= yhi) f = feat[gy * W + gx];
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
            if (MODE == CRF_LOSS) {
              v = ld4(src + (long)pix * CRF_LP + 4 * q);
            } else {
              const float n = a.nrm[pix];
              v = ld4(src + (long)pix * CRF_LP + 4 * q);
              v.x *= n; v.y *= n; v.z *= n; v.w *= n;
            }
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
          float d2;
          if (MODE == CRF_LOSS) {                         // multiples of 1/f^2: the differences are exact, their squares are not
            const float dr = c.x - ri, dg = c.y - gi, db = c.z - bi;
            d2 = dr * dr;
            d2 = fmaf(dg, dg, d2);
            d2 = fmaf(db, db, d2);
          } else {
            d2 = ni + c.w;
            d2 = fmaf(ri, c.x, d2);
            d2 = fmaf(gi, c.y, d2);
            d2 = fmaf(bi, c.z, d2);
          }
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

  // ---- epilogue: the workgroup's D tile [128 pixels][32 columns] through LDS
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
  if (MODE == CRF_LOSS) {
    // [M | Z] of the tile, and the tile's share of  sum_u r_u Z(u)  and  sum_u sum_c S_c(u) M_c(u): products and sums in double
    // (E is the difference of two nearly equal sums), lanes by xor shuffles, waves in index order - no atomics, the same bits
    // every run
    __shared__ double red[8];
    float* M = a.msg + (long)blockIdx.z * H * W * CRF_LP;
    const int L = a.L;
    double sd = 0.0, sm = 0.0;
    for (int idx = tid; idx < 128 * CRF_LP; idx += 256) {
      const int pw = idx >> 5, l = idx & 31;
      const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
      if (x < W && y < H) {
        const long o = (long)(y * W + x) * CRF_LP + l;
        const float d = Dt[pw * CRF_DS + l];
        M[o] = d;
        const double t = (double)src[o] * (double)d;
        if (l < L) sm += t;
        else if (l == L) sd += t;
      }
    }
    sd = wave_sum_d(sd); sm = wave_sum_d(sm);
    if (lane == 0) { red[2 * wave] = sd; red[2 * wave + 1] = sm; }
    __syncthreads();
    if (tid == 0) {
      const long b = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
      a.part[2 * b] = (red[0] + red[2]) + (red[4] + red[6]);
      a.part[2 * b + 1] = (red[1] + red[3]) + (red[5] + red[7]);
    }
    return;
  }
  // FINAL
  __shared__ int best_s[2 * 128];                         // U_LABEL only: the argmaxes wait for the combination
  const int L = a.L, G = a.G, GL = G * L;
  const long HW = (long)H * W;
  for (int idx = tid; idx < 128 * CRF_LP; idx += 256) {
    const int pw = idx >> 5, c = idx & 31;
    const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
    if (x < W && y < H && c < GL) {
      const int pix = y * W + x;
      const long o = (long)pix * CRF_LP + c;
      float u;
      if (UNARY == CRF_U_LABEL) {
        const int g = c >= L ? 1 : 0, l = c - g * L;      // G <= 2
        u = ((int)a.lab[(a.g0 + g) * HW + pix] == l) ? a.u_own : a.u_oth;
      } else {
        u = a.U[o];
      }
      Dt[pw * CRF_DS + c] = (a.msg[o] - u) + a.w * a.nrm[pix] * Dt[pw * CRF_DS + c];
    }
  }
  __syncthreads();
  {                                                       // one thread per (problem, pixel): the softmax sees its own L columns only
    const int pw = tid & 127, g = tid >> 7;
    const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
    if (g < G && x < W && y < H) {
      const int best = crf_softmax_row(Dt + pw * CRF_DS + g * L, L);
      if (UNARY == CRF_U_LABEL) best_s[g * 128 + pw] = best;
      else if (a.last && a.pred) a.pred[y * W + x] = (unsigned char)best;
    }
  }
  __syncthreads();
  if (a.q_next) {
    for (int idx = tid; idx < 128 * CRF_LP; idx += 256) {
      const int pw = idx >> 5, c = idx & 31;
      const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
      if (x < W && y < H) a.q_next[(long)(y * W + x) * CRF_LP + c] = c < GL ? Dt[pw * CRF_DS + c] : 0.f;
    }
  }
  if (!a.last) return;
  if (a.q_out) {
    for (int idx = tid; idx < 128 * GL; idx += 256) {
      const int c = idx >> 7, pw = idx & 127;
      const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
      if (x < W && y < H) a.q_out[((long)a.g0 * L + c) * HW + y * W + x] = Dt[pw * CRF_DS + c];
    }
  }
  if (UNARY == CRF_U_LABEL && tid < 128) {
    const int x = X0 + (tid & 15), y = Y0 + (tid >> 4);
    if (x < W && y < H) {
      const int pix = y * W + x;
      int p[2] = {0, 0};
      for (int g = 0; g < G; ++g) {
        const int b = best_s[g * 128 + tid];
        p[a.g0 + g] = b;
        a.pred_ws[(a.g0 + g) * HW + pix] = (unsigned char)b;
        if (a.pred) a.pred[(a.g0 + g) * HW + pix] = (unsigned char)b;
      }
      if (a.conf && a.g0 + G == 2) {                      // this launch finishes the background problem: combine
        if (G == 1) p[0] = a.pred_ws[pix];                // written by the first pass, earlier on the stream
        a.conf[pix] = crf_combine(a.keys[p[0]], a.keys[p[1]]);
      }
    }
  }
}

// half-width of the window: ceil(trunc * sxy), everything when trunc <= 0 or the window covers the image
int crf_radius(float trunc, float sxy, int H, int W) {
  const int all = (H > W ? H : W);
  if (!(trunc > 0.f)) return all;
  const double r = ceil((double)trunc * (double)sxy);
  return r >= (double)(all - 1) ? all : (int)r;
}

const float CRF_HALF_LOG2E = 0.72134752044448170368f;     // log2(e) / 2

}  // namespace
