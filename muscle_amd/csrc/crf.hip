// The windowed dense CRFs: mean-field inference of the fully connected CRF of Kraehenbuehl & Koltun (Gaussian + bilateral Potts
// terms, symmetric normalisation), the model family that the reference hands to pydensecrf.  pydensecrf filters on a
// permutohedral lattice; here the sums over j are evaluated exactly over a square window of half-width R_m = ceil(trunc * sxy_m)
// (include/muscle_hip.h states the models).  Two unaries share everything else:
//   - the probability unary of segmentation inference (src/imutils.py:439-456, crf_inference): mx_crf_inference;
//   - the label unary of unary_from_labels(zero_unsure=False) (src/imutils.py:477-491, crf_inference_label): mx_crf_label, and
//     mx_ir_label (IRN's cam_to_ir_label): two thresholded argmax label maps of one image, each refined by the label CRF,
//     combined into one uint8 confidence map.
//
// One kernel does every dense sum: crf_msg_kernel is a tiled stencil-GEMM  D[i, c] = sum_j K[i, j] * B[j, c]  on
// v_mfma_f32_32x32x2_f32.  A workgroup (4 waves) owns 16 x 8 output pixels, a wave 32 of them (the M side of the MFMA);
// the window's source pixels are walked in 32 x 8 tiles staged in LDS: colours (r, g, b, r^2+g^2+b^2) and B[j, 0..31] =
// n(j) * Q_s[j, 0..31] (pixel-major, zeros above the columns in use).  Per MFMA a lane computes ONE K[i, j] directly in the
// A-operand layout (lane -> i = lane & 31, j = pair's pixel lane >> 5):
//     K = exp2(-(s2 * (dx^2 + dy^2) + cb * |c_i - c_j|^2)),     s2 = log2(e) / (2 sxy^2), cb = log2(e) / (2 srgb^2)
// dx, dy and the colour distance are small integers, exact in fp32 (|c_i - c_j|^2 = |c_i|^2 + |c_j|^2 - 2 c_i . c_j), so the
// exponent carries three roundings and one v_exp_f32 per pair remains.  The sum of a source tile (128 chained MFMAs) is
// added to the running total per tile (blocked summation: the rounding error does not grow with the window's area).
// The same kernel with B = (1, 0, ...) gives the normalisers, with the colours switched off the Gaussian term.
//
// The 32 columns hold G problems of L labels each (G * L <= 32; problem g in columns g*L .. g*L+L-1): the two CRFs of an IR
// label share the image, hence every K[i, j], both normalisers and the whole window walk, and a column's result depends on
// its own B column and on K only, so G = 2 gives the bits of two G = 1 runs.  The probability path is G = 1.
// Epilogues: NORM -> n(i); STORE -> the weighted Gaussian message; FINAL -> -U + both messages (U read from the workspace, or
// rebuilt from the pixel's label: the label unary is not stored), softmax PER PROBLEM over that problem's L columns, Q_{s+1},
// and on the last iteration Q_t / each problem's argmax (first maximum wins); the IR label maps the two argmaxes through keys
// and writes the combined map.  No atomics, fixed order: same bits every run.
// The kernel itself is in crf_msg.h: crf_loss.hip instantiates its fourth epilogue (LOSS) from the same text.
#include "crf_msg.h"

namespace {

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
    if (l < L) u = crf_prob_unary(confidence, prob[(long)l * HW + i], base);
    U[(long)i * CRF_LP + l] = u;
    d[l] = -u;
  }
#pragma unroll
  for (int l = CRF_MAXL; l < CRF_LP; ++l) U[(long)i * CRF_LP + l] = 0.f;
  // softmax over the first L entries (crf_softmax_row fully unrolled with predicates: d stays in registers)
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

struct CrfLabelArgs {
  const float* cams;     // [C][HW], or NULL: the label map is given
  const int* labels_in;  // [HW] (cams == NULL), one problem
  int C, L, HW, G, g0;
  float fg_thres, bg_thres, u_own, u_oth;
  unsigned char* lab;    // [2][HW]
  float* q0;             // [HW][32]
  int t0;                // t == 0: Q_0 is the result
  float* q_out; unsigned char* pred_ws; unsigned char* pred2; const int* keys; unsigned char* conf;
};

// The two label maps (from the CAMs, or the given one) and Q_0 = softmax(-U) of problems g0 .. g0+G-1 in columns 0 .. G*L-1,
// zeros above.
__global__ void crf_label_kernel(const CrfLabelArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.HW) return;
  const int L = a.L;
  int lab[2] = {0, 0};
  if (a.cams) crf_cam_labels(a.cams, a.C, a.HW, i, a.fg_thres, a.bg_thres, lab[0], lab[1]);
  else lab[0] = crf_in_label(a.labels_in[i], L);
  const CrfLabelE e = crf_label_exp(a.u_own, a.u_oth);
  float q[CRF_LP];
#pragma unroll
  for (int c = 0; c < CRF_LP; ++c) q[c] = 0.f;
  for (int g = 0; g < a.G; ++g) {
    const int own = lab[a.g0 + g];
    a.lab[(long)(a.g0 + g) * a.HW + i] = (unsigned char)own;
    const float inv = crf_label_inv(e, own, L);
#pragma unroll
    for (int c = 0; c < CRF_LP; ++c) {
      const int l = c - g * L;
      if (l >= 0 && l < L) q[c] = ((l == own) ? e.own : e.oth) * inv;
    }
  }
#pragma unroll
  for (int c = 0; c < CRF_LP; c += 4) st4(a.q0 + (long)i * CRF_LP + c, make_float4(q[c], q[c + 1], q[c + 2], q[c + 3]));
  if (!a.t0) return;
  int p[2] = {0, 0};
  for (int g = 0; g < a.G; ++g) {
    int best = 0; float bv = -1.f;
#pragma unroll
    for (int c = 0; c < CRF_LP; ++c) {
      const int l = c - g * L;
      if (l >= 0 && l < L) {
        if (q[c] > bv) { bv = q[c]; best = l; }
        if (a.q_out) a.q_out[((long)(a.g0 + g) * L + l) * a.HW + i] = q[c];
      }
    }
    p[a.g0 + g] = best;
    a.pred_ws[(long)(a.g0 + g) * a.HW + i] = (unsigned char)best;
    if (a.pred2) a.pred2[(long)(a.g0 + g) * a.HW + i] = (unsigned char)best;
  }
  if (a.conf && a.g0 + a.G == 2) {
    if (a.G == 1) p[0] = a.pred_ws[i];                    // this thread's own store of the first pass
    a.conf[i] = crf_combine(a.keys[p[0]], a.keys[p[1]]);
  }
}

// The two workspaces differ in two places: the probability unary stores U, the label unary stores the label and argmax maps.
struct CrfWs {
  float4* feat; float* U; float* M; float* Q[2]; float* ng; float* nb; unsigned char* lab; unsigned char* pred;
};

long crf_ws_bytes(long HW, bool label) {
  const long maps = (2 * HW + 15) / 16 * 16;
  return (4 * HW + (label ? 3 : 4) * (long)CRF_LP * HW + 2 * HW) * 4 + (label ? 2 * maps : 0);
}

CrfWs crf_carve(void* workspace, long HW, bool label) {
  CrfWs w = {};
  float* p = (float*)workspace;
  w.feat = (float4*)p; p += 4 * HW;
  if (!label) { w.U = p; p += CRF_LP * HW; }
  w.M = p; p += CRF_LP * HW;
  w.Q[0] = p; p += CRF_LP * HW;
  w.Q[1] = p; p += CRF_LP * HW;
  w.ng = p; p += HW;
  w.nb = p; p += HW;
  if (label) {
    w.lab = (unsigned char*)p;
    w.pred = w.lab + (2 * HW + 15) / 16 * 16;
  }
  return w;
}

// the two pairwise kernels as the message kernel takes them
struct CrfKernels {
  int Rg, Rb; float s2g, s2b, cb;
  CrfKernels(float sxy_g, float sxy_b, float srgb, float trunc, int H, int W)
      : Rg(crf_radius(trunc, sxy_g, H, W)), Rb(crf_radius(trunc, sxy_b, H, W)), s2g(CRF_HALF_LOG2E / (sxy_g * sxy_g)),
        s2b(CRF_HALF_LOG2E / (sxy_b * sxy_b)), cb(CRF_HALF_LOG2E / (srgb * srgb)) {}
  void gauss(CrfMsgArgs& a) const { a.feat = nullptr; a.R = Rg; a.s2 = s2g; a.cb = 0.f; }
  void bilateral(CrfMsgArgs& a, const float4* feat) const { a.feat = feat; a.R = Rb; a.s2 = s2b; a.cb = cb; }
};

template <int MODE, int UNARY = CRF_U_PROB>
void crf_launch_msg(const CrfMsgArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((crf_msg_kernel<MODE, UNARY>), dim3(cdiv(a.W, CRF_TW), cdiv(a.H, CRF_TH)), dim3(256), 0, st, a);
}

// once per image: the colours and both normalisers
int crf_launch_normalizers(const unsigned char* rgb, int H, int W, const CrfKernels& k, float4* feat, float* n_g, float* n_b,
                           hipStream_t st) {
  const int HW = H * W;
  hipLaunchKernelGGL(crf_feat_kernel, dim3(cdiv(HW, 256)), dim3(256), 0, st, rgb, feat, HW);
  MX_LAUNCH_CHECK();
  CrfMsgArgs a = {};
  a.H = H; a.W = W; a.L = 1; a.G = 1;
  k.gauss(a); a.n_out = n_g;
  crf_launch_msg<CRF_NORM>(a, st);
  MX_LAUNCH_CHECK();
  k.bilateral(a, feat); a.n_out = n_b;
  crf_launch_msg<CRF_NORM>(a, st);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

// t mean-field steps on Q[0]; a carries the problems (H, W, L, G, g0), the unary and where the last step's results go
template <int UNARY>
int crf_iterate(CrfMsgArgs a, const CrfWs& ws, const CrfKernels& k, int t, float w_g, float w_b, hipStream_t st) {
  a.msg = ws.M;
  for (int s = 0; s < t; ++s) {
    a.src = ws.Q[s & 1];
    k.gauss(a); a.nrm = ws.ng; a.w = w_g;
    crf_launch_msg<CRF_STORE>(a, st);
    MX_LAUNCH_CHECK();
    k.bilateral(a, ws.feat); a.nrm = ws.nb; a.w = w_b;
    a.last = s == t - 1;
    a.q_next = a.last ? nullptr : ws.Q[(s + 1) & 1];
    crf_launch_msg<CRF_FINAL, UNARY>(a, st);
    MX_LAUNCH_CHECK();
  }
  return MX_OK;
}

struct CrfModel {
  int t; float gt_prob, sxy_g, w_g, sxy_b, srgb, w_b, trunc;
};

// the label CRF: nprob problems (2: from the CAMs; 1: from labels_in) of L labels, G per pass
int crf_label_run(const unsigned char* rgb, const float* cams, const int* labels_in, const int* keys, int C, int L, int H, int W,
                  float fg_thres, float bg_thres, const CrfModel& m, int nprob, int G, void* workspace, unsigned char* conf,
                  unsigned char* pred2, float* q_out, hipStream_t st) {
  const int HW = H * W;
  const CrfWs ws = crf_carve(workspace, HW, true);
  const CrfLabelU u = crf_label_unary(m.gt_prob, L);
  const CrfKernels k(m.sxy_g, m.sxy_b, m.srgb, m.trunc, H, W);
  if (m.t > 0) {
    const int rc = crf_launch_normalizers(rgb, H, W, k, ws.feat, ws.ng, ws.nb, st);
    if (rc != MX_OK) return rc;
  }
  for (int g0 = 0; g0 < nprob; g0 += G) {
    CrfLabelArgs la = {};
    la.cams = cams; la.labels_in = labels_in; la.C = C; la.L = L; la.HW = HW; la.G = G; la.g0 = g0;
    la.fg_thres = fg_thres; la.bg_thres = bg_thres; la.u_own = u.own; la.u_oth = u.oth;
    la.lab = ws.lab; la.q0 = ws.Q[0]; la.t0 = m.t == 0;
    la.q_out = q_out; la.pred_ws = ws.pred; la.pred2 = pred2; la.keys = keys; la.conf = conf;
    hipLaunchKernelGGL(crf_label_kernel, dim3(cdiv(HW, 128)), dim3(128), 0, st, la);
    MX_LAUNCH_CHECK();
    CrfMsgArgs a = {};
    a.H = H; a.W = W; a.L = L; a.G = G; a.g0 = g0;
    a.lab = ws.lab; a.u_own = u.own; a.u_oth = u.oth;
    a.q_out = q_out; a.pred = pred2; a.pred_ws = ws.pred; a.keys = keys; a.conf = conf;
    const int rc = crf_iterate<CRF_U_LABEL>(a, ws, k, m.t, m.w_g, m.w_b, st);
    if (rc != MX_OK) return rc;
  }
  return MX_OK;
}

}  // namespace

extern "C" {

#define CRF_MAX_PIXELS (1L << 24)

#define CRF_CHECK_SIZE(name) \
  MX_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= CRF_MAX_PIXELS, name ": bad size H=%d W=%d (H*W in 1..2^24)", H, W)
#define CRF_CHECK_KERNELS(name, ws)                                                                                                \
  MX_CHECK_ARG(sxy_g > 0.f && sxy_b > 0.f && srgb > 0.f, name ": sxy_g=%g sxy_b=%g srgb=%g must be positive", sxy_g, sxy_b, srgb); \
  MX_CHECK_ARG(((uintptr_t)ws & 15) == 0, name ": workspace must be 16-byte aligned")
#define CRF_CHECK_LABEL_MODEL(name)                                                             \
  CRF_CHECK_SIZE(name);                                                                         \
  MX_CHECK_ARG(t >= 0, name ": t=%d is negative", t);                                           \
  MX_CHECK_ARG(gt_prob > 0.f && gt_prob < 1.f, name ": gt_prob=%g outside (0, 1)", gt_prob);    \
  CRF_CHECK_KERNELS(name, ws)

long mx_crf_workspace_bytes(int L, int H, int W) {
  if (!(L >= 1 && L <= CRF_MAXL && H > 0 && W > 0 && (long)H * W <= CRF_MAX_PIXELS)) {
    mx_set_error("crf_workspace_bytes: bad args L=%d (1..%d) H=%d W=%d (H*W <= 2^24)", L, CRF_MAXL, H, W);
    return MX_EARG;
  }
  return crf_ws_bytes((long)H * W, false);
}

long mx_ir_label_ws(int L, int H, int W) {
  if (!(L >= 2 && L <= CRF_LABEL_MAXL && H > 0 && W > 0 && (long)H * W <= CRF_MAX_PIXELS)) {
    mx_set_error("ir_label_ws: bad args L=%d (2..%d) H=%d W=%d (H*W <= 2^24)", L, CRF_LABEL_MAXL, H, W);
    return MX_EARG;
  }
  return crf_ws_bytes((long)H * W, true);
}

int mx_crf_normalizers(const unsigned char* rgb, int H, int W, float sxy_g, float sxy_b, float srgb, float trunc, void* workspace,
                       float* n_g, float* n_b, void* stream) {
  MX_CHECK_ARG(rgb && workspace && n_g && n_b, "crf_normalizers: null pointer");
  CRF_CHECK_SIZE("crf_normalizers");
  CRF_CHECK_KERNELS("crf_normalizers", workspace);
  const CrfWs ws = crf_carve(workspace, (long)H * W, false);
  const CrfKernels k(sxy_g, sxy_b, srgb, trunc, H, W);
  return crf_launch_normalizers(rgb, H, W, k, ws.feat, n_g, n_b, (hipStream_t)stream);
}

int mx_crf_inference(const unsigned char* rgb, const float* prob, int L, int H, int W, int t, float confidence, float sxy_g, float w_g,
                     float sxy_b, float srgb, float w_b, float trunc, void* workspace, float* q_out, unsigned char* pred, void* stream) {
  MX_CHECK_ARG(rgb && prob && workspace, "crf_inference: null pointer (rgb, prob or workspace)");
  MX_CHECK_ARG(q_out || pred, "crf_inference: q_out and pred are both NULL");
  MX_CHECK_ARG(L >= 1 && L <= CRF_MAXL, "crf_inference: L=%d outside 1..%d", L, CRF_MAXL);
  CRF_CHECK_SIZE("crf_inference");
  MX_CHECK_ARG(t >= 0, "crf_inference: t=%d is negative", t);
  CRF_CHECK_KERNELS("crf_inference", workspace);
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  const CrfWs ws = crf_carve(workspace, HW, false);
  const CrfKernels k(sxy_g, sxy_b, srgb, trunc, H, W);
  if (t > 0) {
    const int rc = crf_launch_normalizers(rgb, H, W, k, ws.feat, ws.ng, ws.nb, st);
    if (rc != MX_OK) return rc;
  }
  hipLaunchKernelGGL(crf_unary_kernel, dim3(cdiv(HW, 256)), dim3(256), 0, st, prob, L, HW, W, confidence, ws.U, ws.Q[0],
                     t == 0 ? q_out : (float*)nullptr, t == 0 ? pred : (unsigned char*)nullptr);
  MX_LAUNCH_CHECK();
  CrfMsgArgs a = {};
  a.H = H; a.W = W; a.L = L; a.G = 1;
  a.U = ws.U; a.q_out = q_out; a.pred = pred;
  return crf_iterate<CRF_U_PROB>(a, ws, k, t, w_g, w_b, st);
}

int mx_ir_label(const unsigned char* rgb, const float* cams, const int* keys, int C, int H, int W, float fg_thres, float bg_thres, int t,
                float gt_prob, float sxy_g, float w_g, float sxy_b, float srgb, float w_b, float trunc, int fused, void* ws,
                unsigned char* conf, unsigned char* pred2, float* q_out, void* stream) {
  MX_CHECK_ARG(rgb && cams && keys && ws, "ir_label: null pointer (rgb, cams, keys or ws)");
  MX_CHECK_ARG(conf, "ir_label: conf is NULL");
  MX_CHECK_ARG(C >= 1 && C + 1 <= CRF_LABEL_MAXL, "ir_label: C=%d outside 1..%d (L = C + 1 labels, L >= 2)", C, CRF_LABEL_MAXL - 1);
  CRF_CHECK_LABEL_MODEL("ir_label");
  const int L = C + 1;
  const CrfModel m = {t, gt_prob, sxy_g, w_g, sxy_b, srgb, w_b, trunc};
  const int G = (fused && L <= CRF_FUSE_L) ? 2 : 1;
  return crf_label_run(rgb, cams, nullptr, keys, C, L, H, W, fg_thres, bg_thres, m, 2, G, ws, conf, pred2, q_out, (hipStream_t)stream);
}

int mx_crf_label(const unsigned char* rgb, const int* labels, int L, int H, int W, int t, float gt_prob, float sxy_g, float w_g,
                 float sxy_b, float srgb, float w_b, float trunc, void* ws, unsigned char* pred, float* q_out, void* stream) {
  MX_CHECK_ARG(rgb && labels && ws, "crf_label: null pointer (rgb, labels or ws)");
  MX_CHECK_ARG(pred || q_out, "crf_label: pred and q_out are both NULL");
  MX_CHECK_ARG(L >= 2 && L <= CRF_LABEL_MAXL, "crf_label: L=%d outside 2..%d", L, CRF_LABEL_MAXL);
  CRF_CHECK_LABEL_MODEL("crf_label");
  const CrfModel m = {t, gt_prob, sxy_g, w_g, sxy_b, srgb, w_b, trunc};
  return crf_label_run(rgb, nullptr, labels, nullptr, L - 1, L, H, W, 0.f, 0.f, m, 1, 1, ws, nullptr, pred, q_out, (hipStream_t)stream);
}

}  // extern "C"
