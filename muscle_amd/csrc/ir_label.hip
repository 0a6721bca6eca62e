// IR labels from CAMs (IRN's cam_to_ir_label around src/imutils.py:477-491, crf_inference_label): two thresholded argmax label
// maps of one image, each refined by the label CRF, combined into one uint8 confidence map.
//
// The label CRF is the model family of crf.hip (Gaussian + bilateral Potts terms, symmetric normalisation, sums over j exact
// over a square window of half-width R_m = ceil(trunc * sxy_m); include/muscle_hip.h states it) with the unary of
// unary_from_labels(zero_unsure=False): -log(gt_prob) at the pixel's own label, -log((1 - gt_prob) / (L - 1)) elsewhere.
//
// The two CRFs of an image share the image, hence every k_m(i,j), both normalisers and the whole window walk.  irl_msg_kernel
// is crf_msg_kernel's stencil-GEMM  D[i, c] = sum_j K[i, j] * B[j, c]  on v_mfma_f32_32x32x2_f32 (same tiles, same K in the
// A-operand layout, same blocked summation) with the 32 columns holding G problems of L labels each (G * L <= 32; problem g
// in columns g*L .. g*L+L-1, zeros above): one K[i,j] serves both problems.  A column's result depends on its own B column and
// on K only, so G = 2 gives the bits of two G = 1 runs.  The unary is not stored: the FINAL epilogue rebuilds it from the
// pixel's label, takes the softmax PER PROBLEM over that problem's L columns, and on the last step takes each problem's
// argmax (first maximum wins), maps it through keys and writes the combined map.  No atomics, fixed order.
#include "common.h"
#include <math.h>

namespace {

constexpr int IRL_LP = 32;                  // columns: the MFMA's N
constexpr int IRL_MAXL = 21;                // background + the 20 VOC classes
constexpr int IRL_FUSE_L = 16;              // two problems fit the 32 columns up to here
constexpr int IRL_TW = 16, IRL_TH = 8;      // output tile of a workgroup (4 waves x 32 pixels)
constexpr int IRL_SW = 32, IRL_SH = 8;      // source tile staged in LDS
constexpr int IRL_DS = 33;                  // row stride of the epilogue tile
typedef float irl_f32x16 __attribute__((ext_vector_type(16)));

enum { IRL_NORM = 0, IRL_STORE = 1, IRL_FINAL = 2 };

struct IrlMsgArgs {
  const float4* feat;    // [HW] (r, g, b, r^2+g^2+b^2); NULL: Gaussian kernel (no colour term)
  const float* src;      // [HW][32] Q_s (NORM: unused, B = (1, 0, ...))
  const float* nrm;      // [HW] n_m: scales the rows of src at staging time and the result (NORM: unused)
  int H, W, R, L, G, g0; // this launch carries problems g0 .. g0+G-1 in columns 0 .. G*L-1
  float s2, cb, w;
  float* n_out;          // NORM
  float* msg;            // STORE: written; FINAL: the Gaussian message, read
  const unsigned char* lab;   // FINAL: [2][HW] the problems' label maps (255: a label outside 0..L-1, no own column)
  float u_own, u_oth;    // FINAL: the two unary energies
  float* q_next;         // FINAL: [HW][32] or NULL
  float* q_out;          // FINAL, last step: [2][L][H][W] or NULL
  unsigned char* pred_ws;     // FINAL, last step: [2][HW] argmax per problem (workspace; the second pass reads the first's)
  unsigned char* pred2;  // FINAL, last step: [2][HW] or NULL
  const int* keys;       // FINAL, last step: [L] (with conf)
  unsigned char* conf;   // FINAL, last step: [HW] or NULL
  int last;
};

// the three-line combination of cam_to_ir_label
__device__ __forceinline__ unsigned char irl_combine(int fg_conf, int bg_conf) {
  int c = fg_conf;
  if (fg_conf == 0) c = 255;
  if (bg_conf + fg_conf == 0) c = 0;
  return (unsigned char)c;
}

// softmax over d[0..L-1] in place; returns the index of the first maximum of the RESULT
__device__ __forceinline__ int irl_softmax_row(float* d, int L) {
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
__global__ __launch_bounds__(256) void irl_msg_kernel(const IrlMsgArgs a) {
  __shared__ float4 cs[IRL_SW * IRL_SH];
  __shared__ __attribute__((aligned(16))) float Bs[IRL_SW * IRL_SH * IRL_LP];     // 32 KB; the epilogue tile [128][33] afterwards
  __shared__ int best_s[2 * 128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, W = a.W, R = a.R;
  const int X0 = blockIdx.x * IRL_TW, Y0 = blockIdx.y * IRL_TH;
  const int li = lane & 31, kh = lane >> 5;
  const int xi = X0 + (li & 15), yi = Y0 + 2 * wave + (li >> 4);
  float ri = 0.f, gi = 0.f, bi = 0.f, ni = 0.f;
  if (a.feat) {                                           // lanes beyond the image borrow the border pixel (results dropped)
    const float4 f = a.feat[min(yi, H - 1) * W + min(xi, W - 1)];
    ri = -2.f * f.x; gi = -2.f * f.y; bi = -2.f * f.z; ni = f.w;
  }
  const float Rf = (float)R;
  const int xlo = max(0, X0 - R), xhi = min(W - 1, X0 + IRL_TW - 1 + R);
  const int ylo = max(0, Y0 - R), yhi = min(H - 1, Y0 + IRL_TH - 1 + R);

  irl_f32x16 tot;
#pragma unroll
  for (int r = 0; r < 16; ++r) tot[r] = 0.f;

  for (int ys = ylo; ys <= yhi; ys += IRL_SH) {
    for (int xs = xlo; xs <= xhi; xs += IRL_SW) {
      __syncthreads();                                    // the previous tile has been consumed
      {
        const int gx = xs + (tid & (IRL_SW - 1)), gy = ys + (tid >> 5);
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.feat && gx <= xhi && gy <= yhi) f = a.feat[gy * W + gx];
        cs[tid] = f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int idx = tid + 256 * k, p = idx >> 3, q = idx & 7;
        const int gx = xs + (p & (IRL_SW - 1)), gy = ys + (p >> 5);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gx <= xhi && gy <= yhi) {                     // xhi <= W-1, yhi <= H-1: inside the image
          if (MODE == IRL_NORM) {
            if (q == 0) v.x = 1.f;
          } else {
            const int pix = gy * W + gx;
            const float n = a.nrm[pix];
            v = ld4(a.src + (long)pix * IRL_LP + 4 * q);  // columns >= G*L are zero in src
            v.x *= n; v.y *= n; v.z *= n; v.w *= n;
          }
        }
        st4(Bs + p * IRL_LP + 4 * q, v);
      }
      __syncthreads();

      irl_f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float fdx0 = (float)(xs + kh - xi);
#pragma unroll 1
      for (int sy = 0; sy < IRL_SH; ++sy) {
        const int dy = ys + sy - yi;
        const float ty = (abs(dy) <= R) ? (float)(dy * dy) * a.s2 : INFINITY;      // rows outside the window: exp2(-inf) = 0
        const float4* crow = cs + sy * IRL_SW + kh;
        const float* brow = Bs + (sy * IRL_SW + kh) * IRL_LP + li;
#pragma unroll
        for (int pq = 0; pq < IRL_SW / 2; ++pq) {
          const float4 c = crow[2 * pq];
          const float b = brow[2 * pq * IRL_LP];
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

  // ---- epilogue: the workgroup's D tile [128 pixels][32 columns] through LDS
  __syncthreads();
  float* Dt = Bs;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;      // C/D layout of the 32x32 MFMA: col = lane & 31
    Dt[(wave * 32 + row) * IRL_DS + li] = tot[r];
  }
  __syncthreads();
  // pixel pw of the tile: x = X0 + (pw & 15), y = Y0 + (pw >> 4)
  if (MODE == IRL_NORM) {
    if (tid < 128) {
      const int x = X0 + (tid & 15), y = Y0 + (tid >> 4);
      if (x < W && y < H) a.n_out[y * W + x] = 1.0f / sqrtf(Dt[tid * IRL_DS] + 1e-20f);
    }
    return;
  }
  if (MODE == IRL_STORE) {
    for (int idx = tid; idx < 128 * IRL_LP; idx += 256) {
      const int pw = idx >> 5, l = idx & 31;
      const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
      if (x < W && y < H) {
        const int pix = y * W + x;
        a.msg[(long)pix * IRL_LP + l] = a.w * a.nrm[pix] * Dt[pw * IRL_DS + l];
      }
    }
    return;
  }
  // FINAL
  const int L = a.L, G = a.G, GL = G * L;
  const long HW = (long)H * W;
  for (int idx = tid; idx < 128 * IRL_LP; idx += 256) {
    const int pw = idx >> 5, c = idx & 31;
    const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
    if (x < W && y < H && c < GL) {
      const int pix = y * W + x;
      const int g = c >= L ? 1 : 0, l = c - g * L;        // G <= 2
      const float u = ((int)a.lab[(a.g0 + g) * HW + pix] == l) ? a.u_own : a.u_oth;
      Dt[pw * IRL_DS + c] = (a.msg[(long)pix * IRL_LP + c] - u) + a.w * a.nrm[pix] * Dt[pw * IRL_DS + c];
    }
  }
  __syncthreads();
  {                                                       // one thread per (problem, pixel): the softmax sees its own L columns only
    const int pw = tid & 127, g = tid >> 7;
    const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
    if (g < G && x < W && y < H) best_s[g * 128 + pw] = irl_softmax_row(Dt + pw * IRL_DS + g * L, L);
  }
  __syncthreads();
  if (a.q_next) {
    for (int idx = tid; idx < 128 * IRL_LP; idx += 256) {
      const int pw = idx >> 5, c = idx & 31;
      const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
      if (x < W && y < H) a.q_next[(long)(y * W + x) * IRL_LP + c] = c < GL ? Dt[pw * IRL_DS + c] : 0.f;
    }
  }
  if (!a.last) return;
  if (a.q_out) {
    for (int idx = tid; idx < 128 * GL; idx += 256) {
      const int c = idx >> 7, pw = idx & 127;
      const int x = X0 + (pw & 15), y = Y0 + (pw >> 4);
      if (x < W && y < H) a.q_out[((long)a.g0 * L + c) * HW + y * W + x] = Dt[pw * IRL_DS + c];
    }
  }
  if (tid < 128) {
    const int x = X0 + (tid & 15), y = Y0 + (tid >> 4);
    if (x < W && y < H) {
      const int pix = y * W + x;
      int p[2] = {0, 0};
      for (int g = 0; g < G; ++g) {
        const int b = best_s[g * 128 + tid];
        p[a.g0 + g] = b;
        a.pred_ws[(a.g0 + g) * HW + pix] = (unsigned char)b;
        if (a.pred2) a.pred2[(a.g0 + g) * HW + pix] = (unsigned char)b;
      }
      if (a.conf && a.g0 + G == 2) {                      // this launch finishes the background problem: combine
        if (G == 1) p[0] = a.pred_ws[pix];                // written by the first pass, earlier on the stream
        a.conf[pix] = irl_combine(a.keys[p[0]], a.keys[p[1]]);
      }
    }
  }
}

// uint8 [HW][3] -> (r, g, b, r^2 + g^2 + b^2), all exact in fp32
__global__ void irl_feat_kernel(const unsigned char* rgb, float4* feat, int HW) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HW) return;
  const float r = (float)rgb[3 * i], g = (float)rgb[3 * i + 1], b = (float)rgb[3 * i + 2];
  feat[i] = make_float4(r, g, b, r * r + g * g + b * b);
}

struct IrlLabelArgs {
  const float* cams;     // [C][HW], or NULL: the label map is given
  const int* labels_in;  // [HW] (cams == NULL), one problem
  int C, L, HW, G, g0;
  float fg_thres, bg_thres, u_own, u_oth;
  unsigned char* lab;    // [2][HW]
  float* q0;             // [HW][32]
  int t0;                // t == 0: Q_0 is the result
  float* q_out; unsigned char* pred_ws; unsigned char* pred2; const int* keys; unsigned char* conf;
};

// The two label maps (argmax of [threshold, cams...], first maximum wins: a CAM value equal to the threshold is background) and
// Q_0 = softmax(-U) of problems g0 .. g0+G-1 in columns 0 .. G*L-1, zeros above.
__global__ void irl_label_kernel(const IrlLabelArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.HW) return;
  const int L = a.L;
  int lab[2] = {0, 0};
  if (a.cams) {
    float bf = a.fg_thres, bb = a.bg_thres;
    for (int c = 0; c < a.C; ++c) {
      const float v = a.cams[(long)c * a.HW + i];
      if (v > bf) { bf = v; lab[0] = c + 1; }
      if (v > bb) { bb = v; lab[1] = c + 1; }
    }
  } else {
    const int v = a.labels_in[i];
    lab[0] = (v >= 0 && v < L) ? v : 255;
  }
  // softmax of the two-valued row -U: L-1 equal entries and the own one
  const float m = fmaxf(-a.u_own, -a.u_oth);
  const float e_own = expf(-a.u_own - m), e_oth = expf(-a.u_oth - m);
  float q[IRL_LP];
#pragma unroll
  for (int c = 0; c < IRL_LP; ++c) q[c] = 0.f;
  for (int g = 0; g < a.G; ++g) {
    const int own = lab[a.g0 + g];
    a.lab[(long)(a.g0 + g) * a.HW + i] = (unsigned char)own;
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += (l == own) ? e_own : e_oth;
    const float inv = 1.0f / s;
#pragma unroll
    for (int c = 0; c < IRL_LP; ++c) {
      const int l = c - g * L;
      if (l >= 0 && l < L) q[c] = ((l == own) ? e_own : e_oth) * inv;
    }
  }
#pragma unroll
  for (int c = 0; c < IRL_LP; c += 4) st4(a.q0 + (long)i * IRL_LP + c, make_float4(q[c], q[c + 1], q[c + 2], q[c + 3]));
  if (!a.t0) return;
  int p[2] = {0, 0};
  for (int g = 0; g < a.G; ++g) {
    const int own = lab[a.g0 + g];
    int best = 0; float bv = -1.f;
#pragma unroll
    for (int c = 0; c < IRL_LP; ++c) {
      const int l = c - g * L;
      if (l >= 0 && l < L) {
        if (q[c] > bv) { bv = q[c]; best = l; }
        if (a.q_out) a.q_out[((long)(a.g0 + g) * L + l) * a.HW + i] = q[c];
      }
    }
    (void)own;
    p[a.g0 + g] = best;
    a.pred_ws[(long)(a.g0 + g) * a.HW + i] = (unsigned char)best;
    if (a.pred2) a.pred2[(long)(a.g0 + g) * a.HW + i] = (unsigned char)best;
  }
  if (a.conf && a.g0 + a.G == 2) {
    if (a.G == 1) p[0] = a.pred_ws[i];                    // this thread's own store of the first pass
    a.conf[i] = irl_combine(a.keys[p[0]], a.keys[p[1]]);
  }
}

struct IrlWs {
  float4* feat; float* M; float* Q[2]; float* ng; float* nb; unsigned char* lab; unsigned char* pred;
};

long irl_ws_bytes(long HW) {
  const long maps = (2 * HW + 15) / 16 * 16;
  return (4 * HW + 3 * (long)IRL_LP * HW + 2 * HW) * 4 + 2 * maps;
}

IrlWs irl_carve(void* workspace, long HW) {
  IrlWs w;
  float* p = (float*)workspace;
  w.feat = (float4*)p; p += 4 * HW;
  w.M = p; p += IRL_LP * HW;
  w.Q[0] = p; p += IRL_LP * HW;
  w.Q[1] = p; p += IRL_LP * HW;
  w.ng = p; p += HW;
  w.nb = p; p += HW;
  w.lab = (unsigned char*)p;
  w.pred = w.lab + (2 * HW + 15) / 16 * 16;
  return w;
}

// half-width of the window: ceil(trunc * sxy), everything when trunc <= 0 or the window covers the image
int irl_radius(float trunc, float sxy, int H, int W) {
  const int all = (H > W ? H : W);
  if (!(trunc > 0.f)) return all;
  const double r = ceil((double)trunc * (double)sxy);
  return r >= (double)(all - 1) ? all : (int)r;
}

const float IRL_HALF_LOG2E = 0.72134752044448170368f;     // log2(e) / 2

template <int MODE>
void irl_launch_msg(IrlMsgArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(irl_msg_kernel<MODE>, dim3(cdiv(a.W, IRL_TW), cdiv(a.H, IRL_TH)), dim3(256), 0, st, a);
}

struct IrlModel {
  int t; float gt_prob, sxy_g, w_g, sxy_b, srgb, w_b, trunc;
};

// nprob problems (2: from the CAMs; 1: from labels_in) of L labels, G per pass
int irl_run(const unsigned char* rgb, const float* cams, const int* labels_in, const int* keys, int C, int L, int H, int W,
            float fg_thres, float bg_thres, const IrlModel& m, int nprob, int G, void* workspace, unsigned char* conf,
            unsigned char* pred2, float* q_out, hipStream_t st) {
  const int HW = H * W;
  const IrlWs ws = irl_carve(workspace, HW);
  const float u_own = -logf(m.gt_prob), u_oth = -logf((1.0f - m.gt_prob) / (float)(L - 1));
  const int Rg = irl_radius(m.trunc, m.sxy_g, H, W), Rb = irl_radius(m.trunc, m.sxy_b, H, W);
  const float s2g = IRL_HALF_LOG2E / (m.sxy_g * m.sxy_g), s2b = IRL_HALF_LOG2E / (m.sxy_b * m.sxy_b);
  const float cb = IRL_HALF_LOG2E / (m.srgb * m.srgb);
  if (m.t > 0) {                                          // once per image: the colours and both normalisers
    hipLaunchKernelGGL(irl_feat_kernel, dim3(cdiv(HW, 256)), dim3(256), 0, st, rgb, ws.feat, HW);
    MX_LAUNCH_CHECK();
    IrlMsgArgs a = {};
    a.H = H; a.W = W; a.L = 1; a.G = 1;
    a.R = Rg; a.s2 = s2g; a.cb = 0.f; a.n_out = ws.ng;
    irl_launch_msg<IRL_NORM>(a, st);
    MX_LAUNCH_CHECK();
    a.feat = ws.feat;
    a.R = Rb; a.s2 = s2b; a.cb = cb; a.n_out = ws.nb;
    irl_launch_msg<IRL_NORM>(a, st);
    MX_LAUNCH_CHECK();
  }
  for (int g0 = 0; g0 < nprob; g0 += G) {
    IrlLabelArgs la = {};
    la.cams = cams; la.labels_in = labels_in; la.C = C; la.L = L; la.HW = HW; la.G = G; la.g0 = g0;
    la.fg_thres = fg_thres; la.bg_thres = bg_thres; la.u_own = u_own; la.u_oth = u_oth;
    la.lab = ws.lab; la.q0 = ws.Q[0]; la.t0 = m.t == 0;
    la.q_out = q_out; la.pred_ws = ws.pred; la.pred2 = pred2; la.keys = keys; la.conf = conf;
    hipLaunchKernelGGL(irl_label_kernel, dim3(cdiv(HW, 128)), dim3(128), 0, st, la);
    MX_LAUNCH_CHECK();
    for (int s = 0; s < m.t; ++s) {
      const bool last = s == m.t - 1;
      IrlMsgArgs a = {};
      a.H = H; a.W = W; a.L = L; a.G = G; a.g0 = g0;
      a.src = ws.Q[s & 1];
      a.nrm = ws.ng; a.R = Rg; a.s2 = s2g; a.cb = 0.f; a.w = m.w_g; a.msg = ws.M;
      irl_launch_msg<IRL_STORE>(a, st);
      MX_LAUNCH_CHECK();
      a.feat = ws.feat;
      a.nrm = ws.nb; a.R = Rb; a.s2 = s2b; a.cb = cb; a.w = m.w_b;
      a.lab = ws.lab; a.u_own = u_own; a.u_oth = u_oth;
      a.q_next = last ? nullptr : ws.Q[(s + 1) & 1];
      a.last = last ? 1 : 0;
      a.q_out = q_out; a.pred_ws = ws.pred; a.pred2 = pred2; a.keys = keys; a.conf = conf;
      irl_launch_msg<IRL_FINAL>(a, st);
      MX_LAUNCH_CHECK();
    }
  }
  return MX_OK;
}

}  // namespace

extern "C" {

#define IRL_MAX_PIXELS (1L << 24)

long mx_ir_label_ws(int L, int H, int W) {
  if (!(L >= 2 && L <= IRL_MAXL && H > 0 && W > 0 && (long)H * W <= IRL_MAX_PIXELS)) {
    mx_set_error("ir_label_ws: bad args L=%d (2..%d) H=%d W=%d (H*W <= 2^24)", L, IRL_MAXL, H, W);
    return MX_EARG;
  }
  return irl_ws_bytes((long)H * W);
}

#define IRL_CHECK_MODEL(name)                                                                                                   \
  MX_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= IRL_MAX_PIXELS, name ": bad size H=%d W=%d (H*W in 1..2^24)", H, W);            \
  MX_CHECK_ARG(t >= 0, name ": t=%d is negative", t);                                                                           \
  MX_CHECK_ARG(gt_prob > 0.f && gt_prob < 1.f, name ": gt_prob=%g outside (0, 1)", gt_prob);                                    \
  MX_CHECK_ARG(sxy_g > 0.f && sxy_b > 0.f && srgb > 0.f, name ": sxy_g=%g sxy_b=%g srgb=%g must be positive", sxy_g, sxy_b, srgb); \
  MX_CHECK_ARG(((uintptr_t)ws & 15) == 0, name ": workspace must be 16-byte aligned")

int mx_ir_label(const unsigned char* rgb, const float* cams, const int* keys, int C, int H, int W, float fg_thres, float bg_thres, int t,
                float gt_prob, float sxy_g, float w_g, float sxy_b, float srgb, float w_b, float trunc, int fused, void* ws,
                unsigned char* conf, unsigned char* pred2, float* q_out, void* stream) {
  MX_CHECK_ARG(rgb && cams && keys && ws, "ir_label: null pointer (rgb, cams, keys or ws)");
  MX_CHECK_ARG(conf, "ir_label: conf is NULL");
  MX_CHECK_ARG(C >= 1 && C + 1 <= IRL_MAXL, "ir_label: C=%d outside 1..%d (L = C + 1 labels, L >= 2)", C, IRL_MAXL - 1);
  IRL_CHECK_MODEL("ir_label");
  const int L = C + 1;
  const IrlModel m = {t, gt_prob, sxy_g, w_g, sxy_b, srgb, w_b, trunc};
  const int G = (fused && L <= IRL_FUSE_L) ? 2 : 1;
  return irl_run(rgb, cams, nullptr, keys, C, L, H, W, fg_thres, bg_thres, m, 2, G, ws, conf, pred2, q_out, (hipStream_t)stream);
}

int mx_crf_label(const unsigned char* rgb, const int* labels, int L, int H, int W, int t, float gt_prob, float sxy_g, float w_g,
                 float sxy_b, float srgb, float w_b, float trunc, void* ws, unsigned char* pred, float* q_out, void* stream) {
  MX_CHECK_ARG(rgb && labels && ws, "crf_label: null pointer (rgb, labels or ws)");
  MX_CHECK_ARG(pred || q_out, "crf_label: pred and q_out are both NULL");
  MX_CHECK_ARG(L >= 2 && L <= IRL_MAXL, "crf_label: L=%d outside 2..%d", L, IRL_MAXL);
  IRL_CHECK_MODEL("crf_label");
  const IrlModel m = {t, gt_prob, sxy_g, w_g, sxy_b, srgb, w_b, trunc};
  return irl_run(rgb, nullptr, labels, nullptr, L - 1, L, H, W, 0.f, 0.f, m, 1, 1, ws, nullptr, pred, q_out, (hipStream_t)stream);
}

}  // extern "C"
