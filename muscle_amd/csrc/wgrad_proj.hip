// Fused backward of the small project convs: dW, dA and the SE / BN1 backward sums from one pass over (dp, d_raw).
// A translation unit of its own: compiled beside the kernels of wgrad.hip it changed THEIR register allocation (the fused expand kernel
// went from 248 VGPRs to 256 and 20 bytes of scratch).  The tiling, the row groups below 131 072 rows and the partial-matrix reduce
// are wgrad.hip's (mx_wgrad_small_plan, mx_launch_parts_reduce); "the small-output kernel" below is its wgrad_small_kernel.
#include "common.h"

typedef float f32x4w __attribute__((ext_vector_type(4)));

// dW[Co, Ci] += dp^T X' with X' = swish(a x + b) gate (x = d_raw: what wgrad_small_kernel<..., MX_BNACT> forms), dA[R, Ci] = dp Wp, and
// the five per-(sample, channel) sums of se_bn1_pool_kernel over (dA, x).  Same tiling, slabs and MFMA order as the small-output kernel,
// with one difference in where the prologue runs: x reaches LDS RAW and the waves form X' as they read their B fragments.  With the
// Co tiles all on one wave (the plan of both shapes) a wave reads each of its x values exactly once, so the
// activation is evaluated as often as before - and the lane that evaluates z, sigmoid(z) for x[4 qd + q][16 n + l15] can hold the
// matching dA value: the data gradient feeds the MFMA rows of dp permuted (A row i = slab row 4 (i & 3) + (i >> 2)), which leaves
// da[n][r] = dA[4 r + q][16 n + l15], the B-fragment coordinates.  The five sums therefore cost no LDS, no second sigmoid and no pass
// over dA: 5 TCI running sums per lane, joined over q by two shuffles when the sample changes and at the end of the workgroup's rows,
// stored as pp[group + sample][5][Ci] (a (group, sample) pair has its own slot: both indices only grow along the rows) and added per
// sample in group order by wgrad_proj_pool_kernel.  Wp[Co, Ci] is the parameter itself: K of dA = dp Wp is Co, permuted inside every
// block of 8 as in wgrad.hip's DKB form (one ds_read_b64 feeds two MFMA steps), 2 KB TCI weight fragments per lane for the whole kernel.
// Every slab lies inside one sample (rows_per_sample % 16 == 0, checked by the entry): gate and sample change between slabs only.
struct WpArgs {
  const float* G;          // [R, ldg] dp
  const float* X;          // [R, ldx] d_raw
  const float* ca;         // [Ci] BN1 scale, shift
  const float* cb;
  const float* gate;       // [N, Ci]
  const float* W;          // [Co, Ci]
  float* part;             // [groups][Co*Ci]
  float* dA;               // [R, ldda]
  float* pp;               // [groups + N - 1][5][Ci]
  int R, ldg, ldx, ldda, rps, rows_per_wg;      // R, rps and rows_per_wg multiples of 16: every slab is whole and inside one sample
};

constexpr int wp_pad16(int c) { return ((c + 15) / 16 * 16) % 32 == 16 ? (c + 15) / 16 * 16 : (c + 15) / 16 * 16 + 16; }      // wg_pad16

// CO, CI: the conv's shape; the tiling is wg_plan's for it (four waves; the CO / 16 Co tiles on every wave, Ci tile wave + 4 j on wave)
template <int CO, int CI>
__global__ __launch_bounds__(256, 2) void wgrad_proj_fused_kernel(WpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int RB = 16, TCO = CO / 16, TCI = (CI / 16 + 3) / 4, KB = CO / 8, GCH = CO / 4, XCH = CI / 4;
  constexpr int SG = wp_pad16(CO), SX = wp_pad16(64 * TCI), SLAB = RB * (SG + SX);
  static_assert(CO % 16 == 0 && CI % 16 == 0, "whole tiles, an even number of K blocks");
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const long r_beg = (long)blockIdx.x * a.rows_per_wg;
  const long r_end = min((long)a.R, r_beg + a.rows_per_wg);

  // The workgroup's rows of dp, d_raw and dA as buffers: one 32-bit lane offset each, the slab in the scalar offset (per-access 64-bit
  // addresses, which the compiler kept as one induction variable per store, cost ~40 registers here, and the kernel has none to spare).
  // A slab reaches LDS by LDS-DMA (buffer_load_dwordx4 ... lds), not through registers - a register-staged slab is 24 more at
  // CI = 288: wave instruction k fills the 64 16-byte units behind unit 64 k of the image [16][SG] [16][SX], lane by lane, each lane
  // asking for the unit's (row, chunk) - or for nothing (an offset past the buffer: zeros land) where the unit is padding.
  typedef __attribute__((address_space(3))) void* wlds_t;
  constexpr int NG = SG / 16, NK = (SG + SX) / 16, NIW = (NK + 3) / 4;      // wave instructions per slab: of G, of both, per wave
  const int rows = (int)(r_end - r_beg);
  const __amdgpu_buffer_rsrc_t rsg = wbuf_rsrc(a.G + r_beg * a.ldg, ((long)(rows - 1) * a.ldg + CO) * 4);
  const __amdgpu_buffer_rsrc_t rsx = wbuf_rsrc(a.X + r_beg * a.ldx, ((long)(rows - 1) * a.ldx + CI) * 4);
  const __amdgpu_buffer_rsrc_t rsa = wbuf_rsrc(a.dA + r_beg * a.ldda, ((long)(rows - 1) * a.ldda + CI) * 4);
  static_assert(NIW <= 8, "lane offsets of the slab copy");
  unsigned vo[8];      // (not vo[NIW]: with an argument of template-dependent type the host pass drops the kernel's stub over the builtin below)
#pragma unroll
  for (int i = 0; i < NIW; ++i) {
    const int k = wave * NIW + i;
    const int u = (k < NG ? k : k - NG) * 64 + lane, upr = (k < NG ? SG : SX) / 4;
    const int row = u / upr, ch = u - row * upr;
    vo[i] = ch < (k < NG ? GCH : XCH) ? (unsigned)(row * (k < NG ? a.ldg : a.ldx) + 4 * ch) * 4u : 0x7f000000u;
  }
  // slab S of the workgroup -> stage S & 1
#define WPF_ISSUE(S)                                                                                                                  \
  { float* const st_ = smem + ((S) & 1) * SLAB;                                                                                        \
    _Pragma("unroll") for (int i_ = 0; i_ < NIW; ++i_) {                                                                               \
      const int k_ = wave * NIW + i_;                                                                                                  \
      if (k_ < NG) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsg, (wlds_t)(st_ + 256 * k_), 16, vo[i_], (unsigned)((S) * RB * a.ldg) * 4u, 0, 0); \
      else if (k_ < NK) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (wlds_t)(st_ + 256 * k_), 16, vo[i_], (unsigned)((S) * RB * a.ldx) * 4u, 0, 0); \
    } }

  // this lane's columns: col0 + 64 j (only the last tile of a wave can lie past CI: skipped wave-uniformly)
  const int col0 = 16 * wave + l15;
  const bool last_tile = 16 * wave + 64 * (TCI - 1) < CI;
  auto tv = [&](int j) { return j < TCI - 1 || last_tile; };
  // BN1 scale and shift and the sample's gate row wait in LDS behind the slabs ([3][64 TCI]; a wave writes and reads its own columns
  // only: no barrier): as registers they are 3 TCI more than the kernel has
  float* const cf = smem + 2 * SLAB + col0;
#pragma unroll
  for (int j = 0; j < TCI; ++j) {
    cf[64 * j] = tv(j) ? a.ca[col0 + 64 * j] : 0.f;
    cf[64 * TCI + 64 * j] = tv(j) ? a.cb[col0 + 64 * j] : 0.f;
  }
  // the weight fragments of the first TCR tiles stay in registers, those of the other TCI - TCR wait in LDS behind the coefficients
  // ([KB / 2][256 lanes] float4: conflict-free ds_read_b128) - at CI = 288 all 2 KB TCI = 60 of them were ~25 registers too many
  constexpr int TCR = TCI > 3 ? 3 : TCI;
  f32x4w* const wl = reinterpret_cast<f32x4w*>(smem + 2 * SLAB + 3 * 64 * TCI) + tid;
  float wf[KB][2][TCR];
#pragma unroll
  for (int j = 0; j < TCI; ++j)
#pragma unroll
    for (int t = 0; t < KB; t += 2) {
      f32x4w w4;
#pragma unroll
      for (int e = 0; e < 4; ++e) w4[e] = tv(j) ? a.W[(8 * t + 2 * q + (e & 1) + 8 * (e >> 1)) * CI + col0 + 64 * j] : 0.f;
      if (j < TCR) { wf[t][0][j] = w4[0]; wf[t][1][j] = w4[1]; wf[t + 1][0][j] = w4[2]; wf[t + 1][1][j] = w4[3]; }
      else wl[((j - TCR) * (KB / 2) + t / 2) * 256] = w4;
    }

  f32x4w acc[TCO][TCI];
#pragma unroll
  for (int i = 0; i < TCO; ++i)
#pragma unroll
    for (int j = 0; j < TCI; ++j) acc[i][j] = f32x4w{0.f, 0.f, 0.f, 0.f};

  const int ns = rows / RB;
  if (ns > 0) WPF_ISSUE(0)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int prow = 4 * (l15 & 3) + (l15 >> 2);               // the slab row behind MFMA row l15 of the data gradient
  const unsigned voa = (unsigned)(q * a.ldda + col0) * 4u;   // dA[4 r + q][col0 + 64 j] of slab s: row 16 s + 4 r in the scalar offset
  int s = 0;
  while (s < ns) {
    // the slabs of one sample: its gate row once, its sums flushed behind them
    const int n = (int)((unsigned long)(r_beg + (long)s * RB) / (unsigned)a.rps);
    const int s_end = min((long)ns, ((long)(n + 1) * a.rps - r_beg) / RB);
    float sum[5][TCI];
#pragma unroll
    for (int j = 0; j < TCI; ++j) {
      cf[128 * TCI + 64 * j] = tv(j) ? a.gate[(long)n * CI + col0 + 64 * j] : 0.f;
#pragma unroll
      for (int i = 0; i < 5; ++i) sum[i][j] = 0.f;
    }
    for (; s < s_end; ++s) {
      const int cur = s & 1;
      if (s + 1 < ns) WPF_ISSUE(s + 1)                       // into the stage every wave left at the last barrier
      // Ci tile by Ci tile: the data gradient da[r] = dA[4 r + q][col] (K = CO through the weight fragments), then - per four slab
      // rows - the prologue and the sums at the fragment read and the small-output kernel's MFMAs (every accumulator in its order)
      const float* dz = smem + cur * SLAB + prow * SG + 2 * q;
      const float* gs = smem + cur * SLAB + q * SG + l15;
      const float* xs = smem + cur * SLAB + RB * SG + q * SX + col0;
#pragma unroll
      for (int j = 0; j < TCI; ++j) {
        if (!tv(j)) continue;
        const float ca = cf[64 * j], cb = cf[64 * TCI + 64 * j], cg = cf[128 * TCI + 64 * j];
        f32x4w da = f32x4w{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < KB; t += 2) {
          const float2 v = *reinterpret_cast<const float2*>(dz + 8 * t), u = *reinterpret_cast<const float2*>(dz + 8 * t + 8);
          f32x4w w4;
          if (j < TCR) w4 = f32x4w{wf[t][0][j < TCR ? j : 0], wf[t][1][j < TCR ? j : 0], wf[t + 1][0][j < TCR ? j : 0], wf[t + 1][1][j < TCR ? j : 0]};
          else w4 = wl[((j - TCR) * (KB / 2) + t / 2) * 256];
          da = __builtin_amdgcn_mfma_f32_16x16x4f32(v.x, w4[0], da, 0, 0, 0);
          da = __builtin_amdgcn_mfma_f32_16x16x4f32(v.y, w4[1], da, 0, 0, 0);
          da = __builtin_amdgcn_mfma_f32_16x16x4f32(u.x, w4[2], da, 0, 0, 0);
          da = __builtin_amdgcn_mfma_f32_16x16x4f32(u.y, w4[3], da, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(da[r]), rsa, voa + 256u * j, (unsigned)((s * RB + 4 * r) * a.ldda) * 4u, 0);
#pragma unroll
        for (int qd = 0; qd < RB / 4; ++qd) {
          const float x = xs[(4 * qd) * SX + 64 * j];
          const float z = ca * x + cb;
          const float sg = sigmoidf_(z);
          const float act = z * sg;
          const float bv = act * cg;
          const float sp = sg * (1.f + z * (1.f - sg)), d = da[qd];
          sum[0][j] += d * act; sum[1][j] += d * sp; sum[2][j] += sp;
          sum[3][j] += d * sp * x; sum[4][j] += sp * x;
#pragma unroll
          for (int i = 0; i < TCO; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(gs[(4 * qd) * SG + 16 * i], bv, acc[i][j], 0, 0, 0);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's share of slab s + 1 has landed (and its dA stores have left)
      __syncthreads();
    }
    // the sums of sample n's rows in this workgroup -> pp[group + n]: the four row quarters of a column joined in a fixed order
    float* dst = a.pp + (long)(blockIdx.x + n) * 5 * CI + col0;
#pragma unroll
    for (int j = 0; j < TCI; ++j) {
      if (!tv(j)) continue;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        float v = sum[i][j];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (q == 0) dst[i * CI + 64 * j] = v;
      }
    }
  }
  // partial matrix of this workgroup: acc[i][j][r] = dW[16 i + 4 q + r][col0 + 64 j]
  float* out = a.part + (long)blockIdx.x * CO * CI + col0;
#pragma unroll
  for (int i = 0; i < TCO; ++i)
#pragma unroll
    for (int j = 0; j < TCI; ++j) {
      if (!tv(j)) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(16 * i + 4 * q + r) * CI + 64 * j] = acc[i][j][r];
    }
}

#undef WPF_ISSUE

// out5[i][n][c] = the partial rows pp[g + n][i][c] of the workgroups g that hold rows of sample n, added in group order (in fp64)
__global__ __launch_bounds__(256) void wgrad_proj_pool_kernel(const float* __restrict__ pp, int rps, int rows_per_wg, int Ci, int N,
                                                              float* __restrict__ out5) {
  const int e = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (e >= 5 * Ci) return;
  const int g0 = (int)((long)n * rps / rows_per_wg), g1 = (int)(((long)(n + 1) * rps - 1) / rows_per_wg);
  double s = 0.0;                          // (a sample of a short launch can lie in > 100 workgroups: a float chain that long shows)
  for (int g = g0; g <= g1; ++g) s += (double)pp[(long)(g + n) * 5 * Ci + e];
  const int i = e / Ci, c = e - i * Ci;
  out5[((long)i * N + n) * Ci + c] = (float)s;
}

static bool wpf_shape(int Co, int Ci) { return Co == 48 && (Ci == 288 || Ci == 192); }

// tiling: wg_plan's; row groups: one round of 512 workgroups (two per CU), wg_plan's own below 131 072 rows - there dW matches
// mx_pw_wgrad_small (BNACT) bit for bit
static bool wpf_plan(int R, int Co, int Ci, int rps, WgPlan* p) {
  if (R < 1 || rps < 16 || rps % 16 || R % rps || R / rps > 65535 || !wpf_shape(Co, Ci) || !mx_wgrad_small_plan(1 << 20, Co, Ci, p) || p->nw != 4) return false;
  int rows = cdiv(cdiv(R, 512), 16) * 16;
  if (rows < 64) rows = 64;
  WgPlan q;
  if (R < 131072 && mx_wgrad_small_plan(R, Co, Ci, &q)) rows = q.rows_per_wg;
  p->rows_per_wg = rows;
  p->groups = cdiv(R, rows);
  p->lds_bytes += 3L * 64 * p->tci * 4;                       // scale, shift and gate row of the waves' columns
  if (p->tci > 3) p->lds_bytes += (p->tci - 3) * (Co / 16) * 256L * 16;      // weight fragments of the tiles behind the third
  return true;
}

typedef int (*WpLaunch)(const WpArgs&, const WgPlan&, hipStream_t);
template <int CO, int CI>
static int wpf_launch_one(const WpArgs& a, const WgPlan& p, hipStream_t st) {
  if (p.lds_bytes > 64 * 1024) {
    const int rc = mx_dyn_lds_optin(reinterpret_cast<const void*>(&wgrad_proj_fused_kernel<CO, CI>), 80 * 1024);
    if (rc != MX_OK) return rc;
  }
  hipLaunchKernelGGL((wgrad_proj_fused_kernel<CO, CI>), dim3(p.groups), dim3(256), p.lds_bytes, st, a);
  return MX_OK;
}

// the kernel's compile-time tiling must be the plan's (LDS strides and bytes included)
template <int CO, int CI>
static WpLaunch wpf_try(const WgPlan& p, int Co, int Ci) {
  constexpr int TCI = (CI / 16 + 3) / 4;
  const bool same = Co == CO && Ci == CI && p.nw == 4 && p.wco == 1 && p.tco == CO / 16 && p.tci == TCI && p.SG == wp_pad16(CO) &&
                    p.SX == wp_pad16(64 * TCI) && p.lds_bytes == 2L * 16 * (p.SG + p.SX) * 4 + 3L * 64 * TCI * 4 + (TCI > 3 ? TCI - 3 : 0) * (CO / 16) * 256L * 16;
  return same ? &wpf_launch_one<CO, CI> : nullptr;
}

static WpLaunch wpf_dispatch(const WgPlan& p, int Co, int Ci) {
  if (WpLaunch l = wpf_try<48, 288>(p, Co, Ci)) return l;
  return wpf_try<48, 192>(p, Co, Ci);
}

extern "C" {

// 1 where the engine should take mx_pw_proj_bwd_fused for a project conv [Cout, Cexp] over R rows: an admitted shape, a reduction as
// long as the small-output kernels ask, whole samples of a multiple of 16 rows
int mx_pw_proj_bwd_fused_ok(int R, int Cout, int Cexp, int rows_per_sample) {
  WgPlan p;
  return R >= 65536 && wpf_plan(R, Cout, Cexp, rows_per_sample, &p) && wpf_dispatch(p, Cout, Cexp) ? 1 : 0;
}

// row groups of mx_pw_proj_bwd_fused (0 = not taken): its scratch is [groups][Cout*Cexp] + [groups + N - 1][5][Cexp] floats
int mx_pw_proj_bwd_fused_groups(int R, int Cout, int Cexp, int rows_per_sample) {
  WgPlan p;
  return wpf_plan(R, Cout, Cexp, rows_per_sample, &p) && wpf_dispatch(p, Cout, Cexp) ? p.groups : 0;
}

// The backward of a small project conv in one pass over dp [R, Cout] and d_raw [R, Cexp]: dW[Cout, Cexp] += dp^T (swish(scale d_raw +
// shift) gate), dA[R, Cexp] = dp Wp, out5[5][N][Cexp] = the sums of mx_se_bn1_pool over (dA, d_raw).  dW = null leaves the partial
// matrices at the head of ws for a later mx_pw_parts_reduce.
int mx_pw_proj_bwd_fused(const float* dp, const float* d_raw, const float* scale, const float* shift, const float* gate, int rows_per_sample,
                         const float* Wp, float* dW, float* dA, float* out5, int R, int Cout, int Cexp, int lddp, int ldraw, int ldda,
                         void* ws, long ws_bytes, void* stream) {
  MX_CHECK_ARG(wpf_shape(Cout, Cexp) && R >= 1, "pw_proj_bwd_fused: shape R=%d Cout=%d Cexp=%d not taken (48 x 288 and 48 x 192 only)", R, Cout, Cexp);
  MX_CHECK_ARG(rows_per_sample >= 16 && rows_per_sample % 16 == 0 && R % rows_per_sample == 0,
               "pw_proj_bwd_fused: rows_per_sample=%d must be a multiple of 16 that divides R=%d", rows_per_sample, R);
  MX_CHECK_ARG(dp && d_raw && scale && shift && gate && Wp && dA && out5 && ws, "pw_proj_bwd_fused: null pointer");
  MX_CHECK_ARG((((uintptr_t)dp | (uintptr_t)d_raw | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)gate | (uintptr_t)Wp | (uintptr_t)dW |
                 (uintptr_t)dA | (uintptr_t)out5 | (uintptr_t)ws) & 15) == 0, "pw_proj_bwd_fused: pointers must be 16-byte aligned");
  MX_CHECK_ARG(lddp % 4 == 0 && ldraw % 4 == 0 && ldda % 4 == 0 && lddp >= Cout && ldraw >= Cexp && ldda >= Cexp,
               "pw_proj_bwd_fused: leading dimensions (%d, %d, %d) must be multiples of 4 and cover the rows", lddp, ldraw, ldda);
  WgPlan p;
  MX_CHECK_ARG(wpf_plan(R, Cout, Cexp, rows_per_sample, &p), "pw_proj_bwd_fused: no plan for R=%d Cout=%d Cexp=%d", R, Cout, Cexp);
  const WpLaunch launch = wpf_dispatch(p, Cout, Cexp);
  MX_CHECK_ARG(launch, "pw_proj_bwd_fused: no kernel for Cout=%d Cexp=%d", Cout, Cexp);
  const int N = R / rows_per_sample;
  const long part_floats = (long)p.groups * Cout * Cexp;
  MX_CHECK_ARG(ws_bytes >= (part_floats + (long)(p.groups + N - 1) * 5 * Cexp) * 4, "pw_proj_bwd_fused: workspace too small");
  WpArgs a{};
  a.G = dp; a.X = d_raw; a.ca = scale; a.cb = shift; a.gate = gate; a.W = Wp;
  a.part = (float*)ws; a.dA = dA; a.pp = (float*)ws + part_floats;
  a.R = R; a.ldg = lddp; a.ldx = ldraw; a.ldda = ldda; a.rps = rows_per_sample; a.rows_per_wg = p.rows_per_wg;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch(a, p, st);
  if (rc != MX_OK) return rc;
  MX_LAUNCH_CHECK();
  hipLaunchKernelGGL(wgrad_proj_pool_kernel, dim3(cdiv(5 * Cexp, 256), N), dim3(256), 0, st, (const float*)a.pp, rows_per_sample, p.rows_per_wg,
                     Cexp, N, out5);
  MX_LAUNCH_CHECK();
  if (dW) {
    mx_launch_parts_reduce((const float*)ws, p.groups, Cout * Cexp, dW, st);
    MX_LAUNCH_CHECK();
  }
  return MX_OK;
}

}  // extern "C"
