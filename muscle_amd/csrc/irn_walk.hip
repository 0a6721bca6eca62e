// Matrix-free IRN random walk (src/indexing.py:116-147 as called by infer_irn.py:76): x . T^steps as `steps` applications of
// the 2 nd + 1 point stencil that T is, instead of squaring the dense n x n matrix.  T = scaled / column sums with
// scaled[i][j] = affinity(i, j)^beta, and affinity(i, j) != 0 only for i == j or j == i +- (one of the nd one-sided search
// directions), so one step of v <- v . T is
//   v'[j] = (v[j] + sum_d (v[j + d] W[d][j] + v[j - d] W[d][j - d])) / cs[j]
// with W[d][p] = scaled[p][p + d] and cs = the column sums.  The weights are fp32 (bit for bit the dense path's scaled
// entries); the column sums, the state and every per-pixel sum are fp64: with fp32 state the 2^exp_times renormalised
// steps accumulate more error than the dense path's exp_times squarings do ("IRN random-walk propagation").
// Every sum runs in one fixed order, contraction off, no atomics: tests/irn_walk_ref.py restates it operation for operation.
// mx_irn_walk_snap is the same walk that also writes the states at listed step counts (muscle_amd/irn_sweep.py): one device
// function holds the per-pixel arithmetic, so a snapshot has the bits of a separate walk of as many steps.
#include "common.h"

#define IRN_WALK_MAX_ND 1024      // directions whose (dy, dx) a step keeps in LDS: radius 5 has 34, radius 16 has 394

// W[d][p] = (1 - max of the edge along the straight path p -> p + d)^beta, 0 where p + d lies outside the image.  Every path
// point lies inside the bounding box of p and p + d, so the reference's padding (1.0 around the image, indexing.py:124)
// only ever zeroes pairs that its crop (:131-133) removes.  The power is irn_pow_colsum_kernel's (irn.hip).
__global__ __launch_bounds__(256) void irn_walk_weights_kernel(const float* __restrict__ edge, int h, int w,
                                                               const int* __restrict__ pcoord, const int* __restrict__ poff,
                                                               const int* __restrict__ plen, float beta, float* __restrict__ W) {
  const int n = h * w;
  const int p = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
  if (p >= n) return;
  const int py = p / w, px = p - py * w;
  const int* pc = pcoord + 2 * poff[d];
  const int ty = py + pc[0], tx = px + pc[1];               // destination = first (farthest) path pixel
  float v = 0.f;
  if (ty >= 0 && ty < h && tx >= 0 && tx < w) {
    float mx = -INFINITY;
    for (int l = 0; l < plen[d]; ++l) {
      const int y = py + pc[2 * l], x = px + pc[2 * l + 1];
      mx = fmaxf(mx, (y >= 0 && y < h && x >= 0 && x < w) ? edge[y * w + x] : 1.0f);
    }
    v = 1.0f - mx;
    const int ib = (beta > 0.f && beta <= 64.f && beta == floorf(beta)) ? (int)beta : 0;
    if (ib > 0) {                                            // integral exponent: exact repeated multiplication
      float r = 1.f, b = v;
      for (int e = ib; e; e >>= 1) { if (e & 1) r *= b; b *= b; }
      v = r;
    } else {
      v = (v == 0.f) ? 0.f : powf(v, beta);
    }
  }
  W[(long)d * n + p] = v;
}

// cs[j] = 1 + sum_d (W[d][j] + W[d][j - d]): the column sum of scaled, gathered in the walk's tap order
__global__ __launch_bounds__(256) void irn_walk_colsum_kernel(const float* __restrict__ W, int h, int w, const int* __restrict__ pcoord,
                                                              const int* __restrict__ poff, int nd, double* __restrict__ cs) {
  const int n = h * w;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int y = j / w, x = j - y * w;
  double s = 1.0;
  for (int d = 0; d < nd; ++d) {
    const int dy = pcoord[2 * poff[d]], dx = pcoord[2 * poff[d] + 1];
    const int by = y - dy, bx = x - dx;
    s += (double)W[(long)d * n + j];                         // 0 where j + d is outside
    if (by >= 0 && by < h && bx >= 0 && bx < w) s += (double)W[(long)d * n + by * w + bx];
  }
  cs[j] = s;
}

// state 0 = (double)(x * (1 - edge)), the product in fp32 as indexing.py:145 forms it
__global__ __launch_bounds__(256) void irn_walk_init_kernel(const float* __restrict__ x, const float* __restrict__ edge, int n,
                                                            double* __restrict__ v) {
  const int j = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (j >= n) return;
  v[(long)c * n + j] = (double)(x[(long)c * n + j] * (1.0f - edge[j]));
}

// One step's value for pixel j of one channel (vc = that channel's state): the per-pixel arithmetic, shared by the two step
// kernels so that a snapshot and a separate walk of as many steps cannot drift apart.  sdy / sdx: the (dy, dx) of every direction.
__device__ __forceinline__ double irn_walk_step_value(const double* __restrict__ vc, const float* __restrict__ W,
                                                      const double* __restrict__ cs, int h, int w, int j, const int* sdy,
                                                      const int* sdx, int nd) {
#pragma clang fp contract(off)
  const int n = h * w;
  const int y = j / w, x = j - y * w;
  double s = vc[j];
  // A tap outside the image reads pixel j instead and is dropped by the select: no branch, so the loads of several directions
  // are in flight together; the additions stay in the one order.
#pragma unroll 4
  for (int d = 0; d < nd; ++d) {
    const int dy = sdy[d], dx = sdx[d];
    const float* Wd = W + (long)d * n;
    const int fy = y + dy, fx = x + dx, by = y - dy, bx = x - dx;
    const bool fok = fy >= 0 && fy < h && fx >= 0 && fx < w, bok = by >= 0 && by < h && bx >= 0 && bx < w;
    const int fi = fok ? fy * w + fx : j, bi = bok ? by * w + bx : j;
    const double vf = vc[fi], wf = (double)Wd[j], vb = vc[bi], wb = (double)Wd[bi];
    const double sf = s + vf * wf;
    s = fok ? sf : s;
    const double sb = s + vb * wb;
    s = bok ? sb : s;
  }
  return s / cs[j];
}

// one step for one (pixel, channel); `out32` != null on the last step.  The (dy, dx) of every direction go to LDS first.
__global__ __launch_bounds__(256) void irn_walk_step_kernel(const double* __restrict__ v, const float* __restrict__ W,
                                                            const double* __restrict__ cs, int h, int w,
                                                            const int* __restrict__ pcoord, const int* __restrict__ poff, int nd,
                                                            double* __restrict__ out, float* __restrict__ out32) {
  __shared__ int sdy[IRN_WALK_MAX_ND], sdx[IRN_WALK_MAX_ND];
  for (int d = threadIdx.x; d < nd; d += 256) { sdy[d] = pcoord[2 * poff[d]]; sdx[d] = pcoord[2 * poff[d] + 1]; }
  __syncthreads();
  const int n = h * w;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double s = irn_walk_step_value(v + (long)blockIdx.y * n, W, cs, h, w, j, sdy, sdx, nd);
  if (out32) out32[(long)blockIdx.y * n + j] = (float)s;
  else out[(long)blockIdx.y * n + j] = s;
}

// a snapshot step: the fp64 state the walk goes on from AND the fp32 rounding of that same value, which is what
// irn_walk_step_kernel would have written had the walk ended here
__global__ __launch_bounds__(256) void irn_walk_snap_kernel(const double* __restrict__ v, const float* __restrict__ W,
                                                            const double* __restrict__ cs, int h, int w,
                                                            const int* __restrict__ pcoord, const int* __restrict__ poff, int nd,
                                                            double* __restrict__ out, float* __restrict__ out32) {
  __shared__ int sdy[IRN_WALK_MAX_ND], sdx[IRN_WALK_MAX_ND];
  for (int d = threadIdx.x; d < nd; d += 256) { sdy[d] = pcoord[2 * poff[d]]; sdx[d] = pcoord[2 * poff[d] + 1]; }
  __syncthreads();
  const int n = h * w;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double s = irn_walk_step_value(v + (long)blockIdx.y * n, W, cs, h, w, j, sdy, sdx, nd);
  out[(long)blockIdx.y * n + j] = s;
  out32[(long)blockIdx.y * n + j] = (float)s;
}

extern "C" {

int mx_irn_walk_weights(const float* edge, int h, int w, int radius, const int* pcoord, const int* poff, const int* plen, int nd,
                        float beta, float* W, double* cs, void* stream) {
  MX_CHECK_ARG(edge && pcoord && poff && plen && W && cs, "irn_walk_weights: null pointer");
  MX_CHECK_ARG(h > 0 && w > 0 && radius >= 1 && nd > 0 && nd <= 65535 && (long)h * w * nd < (1L << 31),
               "irn_walk_weights: bad geometry (h=%d w=%d radius=%d nd=%d)", h, w, radius, nd);
  hipStream_t st = (hipStream_t)stream;
  const int n = h * w;
  hipLaunchKernelGGL(irn_walk_weights_kernel, dim3(cdiv(n, 256), nd), dim3(256), 0, st, edge, h, w, pcoord, poff, plen, beta, W);
  hipLaunchKernelGGL(irn_walk_colsum_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, W, h, w, pcoord, poff, nd, cs);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

long mx_irn_walk_ws(int C, int n) {
  if (C < 1 || n < 1) return -1;
  return (long)sizeof(double) * C * n;
}

int mx_irn_walk(const float* x, const float* edge, const float* W, const double* cs, int h, int w, int radius, const int* pcoord,
                const int* poff, const int* plen, int nd, int C, int steps, double* state_a, double* state_b, float* rw, void* stream) {
  MX_CHECK_ARG(x && edge && W && cs && pcoord && poff && plen && state_a && state_b && rw, "irn_walk: null pointer");
  MX_CHECK_ARG(steps >= 1 && steps <= 4096, "irn_walk: steps must be 1..4096 (got %d)", steps);
  MX_CHECK_ARG(radius >= 1, "irn_walk: radius must be >= 1 (got %d)", radius);
  MX_CHECK_ARG(h > 0 && w > 0 && nd > 0 && nd <= IRN_WALK_MAX_ND && C > 0 && C <= 65535 && (long)h * w * nd < (1L << 31) && (long)h * w * C < (1L << 31),
               "irn_walk: bad geometry (h=%d w=%d nd=%d C=%d)", h, w, nd, C);
  MX_CHECK_ARG(state_a != state_b, "irn_walk: the two state buffers must differ");
  hipStream_t st = (hipStream_t)stream;
  const int n = h * w;
  const dim3 grid(cdiv(n, 256), C);
  hipLaunchKernelGGL(irn_walk_init_kernel, grid, dim3(256), 0, st, x, edge, n, state_a);
  double *src = state_a, *dst = state_b;
  for (int s = 0; s < steps; ++s) {
    hipLaunchKernelGGL(irn_walk_step_kernel, grid, dim3(256), 0, st, (const double*)src, W, cs, h, w, pcoord, poff, nd, dst,
                       s == steps - 1 ? rw : (float*)nullptr);
    double* t = src; src = dst; dst = t;
  }
  MX_LAUNCH_CHECK();
  return MX_OK;
}

#define IRN_WALK_MAX_SNAP 13      // exp_times 0..12

// mx_irn_walk that also hands out the states it passes through: snap[ns] (host memory, read before return) ascending step counts,
// rw [ns][C][n].  Snapshot i has the bits of mx_irn_walk(..., steps = snap[i]): the same fp64 value, rounded once.
int mx_irn_walk_snap(const float* x, const float* edge, const float* W, const double* cs, int h, int w, int radius, const int* pcoord,
                     const int* poff, const int* plen, int nd, int C, const int* snap, int ns, double* state_a, double* state_b,
                     float* rw, void* stream) {
  MX_CHECK_ARG(x && edge && W && cs && pcoord && poff && plen && snap && state_a && state_b && rw, "irn_walk_snap: null pointer");
  MX_CHECK_ARG(ns >= 1 && ns <= IRN_WALK_MAX_SNAP, "irn_walk_snap: ns must be 1..%d (got %d)", IRN_WALK_MAX_SNAP, ns);
  MX_CHECK_ARG(snap[0] >= 1 && snap[ns - 1] <= 4096, "irn_walk_snap: snap must lie in 1..4096 (got %d..%d)", snap[0], snap[ns - 1]);
  for (int i = 1; i < ns; ++i)
    MX_CHECK_ARG(snap[i] > snap[i - 1], "irn_walk_snap: snap must be strictly ascending (snap[%d]=%d after %d)", i, snap[i], snap[i - 1]);
  MX_CHECK_ARG(radius >= 1, "irn_walk_snap: radius must be >= 1 (got %d)", radius);
  MX_CHECK_ARG(h > 0 && w > 0 && nd > 0 && nd <= IRN_WALK_MAX_ND && C > 0 && C <= 65535 && (long)h * w * nd < (1L << 31) &&
                   (long)h * w * C * ns < (1L << 31),
               "irn_walk_snap: bad geometry (h=%d w=%d nd=%d C=%d ns=%d)", h, w, nd, C, ns);
  MX_CHECK_ARG(state_a != state_b, "irn_walk_snap: the two state buffers must differ");
  hipStream_t st = (hipStream_t)stream;
  const int n = h * w;
  const dim3 grid(cdiv(n, 256), C);
  hipLaunchKernelGGL(irn_walk_init_kernel, grid, dim3(256), 0, st, x, edge, n, state_a);
  double *src = state_a, *dst = state_b;
  int i = 0;
  for (int s = 1; s <= snap[ns - 1]; ++s) {
    if (s == snap[i]) {
      hipLaunchKernelGGL(irn_walk_snap_kernel, grid, dim3(256), 0, st, (const double*)src, W, cs, h, w, pcoord, poff, nd, dst,
                         rw + (long)i * C * n);
      ++i;
    } else {
      hipLaunchKernelGGL(irn_walk_step_kernel, grid, dim3(256), 0, st, (const double*)src, W, cs, h, w, pcoord, poff, nd, dst,
                         (float*)nullptr);
    }
    double* t = src; src = dst; dst = t;
  }
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
