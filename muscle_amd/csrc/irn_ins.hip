// Instance pseudo-labels from the IRN displacement field ("Instance pseudo-labels"; include/muscle_hip.h has the six steps).
// Everything here is O(H*W) memory: no [classes x instances, H, W] array exists outside the walk's own [C,h,w] input and output.
// Only integer atomics (min on parents, add on areas, max on the bit patterns of non-negative floats): no result depends on the order
// in which workgroups run.
#include "common.h"
#include "irn_soft.h"

#define INS_LDS_BUDGET (160 * 1024)        // one workgroup may declare all of a CU's LDS on gfx950
#define CCL_T 16                           // tile edge of the LDS union-find

// ---------------------------------------------------------------------------------------------------------------------------
// Step 1: centroids.  m(d) = d[uy,ux]*yc*xc + d[dy,ux]*(1-yc)*xc + d[uy,dx]*yc*(1-xc) + d[dy,dx]*(1-yc)*(1-xc), every product and
// sum rounded on its own, left to right: the iteration amplifies a last-bit difference into another pixel, so a fused multiply-add
// anywhere moves centroids (tests/test_cpu_ins_seg.py: fp64 products move 93 of the 2 961 of the 47x63 test field).
// ---------------------------------------------------------------------------------------------------------------------------
// (the __fmul_rn / __fadd_rn intrinsics are plain operators in this toolchain's headers and would contract after inlining; as in
// common.h, every operation is spelt out in a scope with contraction off.)
__device__ __forceinline__ float ins_bil(const float* d, int iuu, int idu, int iud, int idd, float yc, float xc, float oy, float ox) {
#pragma clang fp contract(off)
  float t1 = d[iuu] * yc; t1 = t1 * xc;
  float t2 = d[idu] * oy; t2 = t2 * xc;
  float t3 = d[iud] * yc; t3 = t3 * ox;
  float t4 = d[idd] * oy; t4 = t4 * ox;
  float s = t1 + t2;
  s = s + t3;
  return s + t4;
}
// one move of (cy, cx); n = h*w, f = the field (global or LDS)
__device__ __forceinline__ void ins_move(const float* f, int n, int w, float ymax, float xmax, float& cy, float& cx) {
#pragma clang fp contract(off)
  // cy, cx stay inside [0, h-1] x [0, w-1] (fmaxf / fminf drop a NaN), so the four taps are in bounds
  const float uyf = ceilf(cy), dyf = floorf(cy), uxf = ceilf(cx), dxf = floorf(cx);
  const float yc = cy - dyf, xc = cx - dxf;
  const float oy = 1.f - yc, ox = 1.f - xc;
  const int uy = (int)uyf, dy = (int)dyf, ux = (int)uxf, dx = (int)dxf;
  const int iuu = uy * w + ux, idu = dy * w + ux, iud = uy * w + dx, idd = dy * w + dx;
  const float my = ins_bil(f, iuu, idu, iud, idd, yc, xc, oy, ox);
  const float mx = ins_bil(f + n, iuu, idu, iud, idd, yc, xc, oy, ox);
  const float ny = cy + my, nx = cx + mx;
  cy = fminf(fmaxf(ny, 0.f), ymax);
  cx = fminf(fmaxf(nx, 0.f), xmax);
}

template <bool STAGE>
__global__ __launch_bounds__(256) void irn_centroids_kernel(const float* dp, int h, int w, int iterations, int* cent) {
  extern __shared__ float ins_field[];
  const int n = h * w;
  const float* f = dp;
  if (STAGE) {
    for (int i = threadIdx.x; i < 2 * n; i += 256) ins_field[i] = dp[i];
    __syncthreads();
    f = ins_field;
  }
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  float cy = (float)(p / w), cx = (float)(p % w);
  const float ymax = (float)(h - 1), xmax = (float)(w - 1);
  for (int it = 0; it < iterations; ++it) ins_move(f, n, w, ymax, xmax, cy, cx);
  cent[p] = (int)rintf(cy);             // round half to even
  cent[n + p] = (int)rintf(cx);
}

// Step 2, first line: sqrt(dx^2 + dy^2), the squares and the sum rounded on their own, sqrtf correctly rounded (hipcc's default)
__device__ __forceinline__ float ins_magnitude(float dy, float dx) {
#pragma clang fp contract(off)
  const float a = dx * dx, b = dy * dy;
  const float s = a + b;
  return sqrtf(s);
}
__global__ __launch_bounds__(256) void irn_weak_kernel(const float* dp, int n, float thres, int* weak) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  weak[p] = ins_magnitude(dp[p], dp[n + p]) < thres ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Connected components by union-find.  parent[i] <= i always, a union hangs the larger root below the smaller with atomicMin, so the
// root of a finished component is its smallest index whatever the order of the unions.  A union that finds its target no longer a root
// (atomicMin returns another value) goes on with that value: the link it displaced is re-made, none is lost.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ccl_find_lds(volatile int* par, int a) {
  int p;
  while ((p = par[a]) != a) a = p;
  return a;
}
__device__ __forceinline__ void ccl_union_lds(int* par, int a, int b) {
  for (;;) {
    a = ccl_find_lds(par, a);
    b = ccl_find_lds(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;
  }
}
// across workgroups: the loads go to L2 (agent scope), where the atomics are performed - a CU's L1 may hold an older parent
__device__ __forceinline__ int ccl_find_g(int* par, int a) {
  int p;
  while ((p = __hip_atomic_load(&par[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != a) a = p;
  return a;
}
__device__ __forceinline__ void ccl_union_g(int* par, int a, int b) {
  for (;;) {
    a = ccl_find_g(par, a);
    b = ccl_find_g(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(CCL_T * CCL_T) void ccl_tile_kernel(const int* label, int h, int w, int* parent) {
  __shared__ int par[CCL_T * CCL_T], lab[CCL_T * CCL_T];
  const int t = threadIdx.x, lx = t % CCL_T, ly = t / CCL_T;
  const int gx = blockIdx.x * CCL_T + lx, gy = blockIdx.y * CCL_T + ly;
  const bool in = gx < w && gy < h;
  const int L = in ? label[gy * w + gx] : 0;
  lab[t] = L;
  par[t] = t;
  __syncthreads();
  if (L != 0) {
    if (lx > 0 && lab[t - 1] == L) ccl_union_lds(par, t, t - 1);
    if (ly > 0 && lab[t - CCL_T] == L) ccl_union_lds(par, t, t - CCL_T);
  }
  __syncthreads();
  if (in) {
    const int r = ccl_find_lds(par, t);           // the tile-local raster order is the global one restricted to the tile
    parent[gy * w + gx] = (blockIdx.y * CCL_T + r / CCL_T) * w + blockIdx.x * CCL_T + r % CCL_T;
  }
}

__global__ __launch_bounds__(256) void ccl_border_kernel(const int* label, int h, int w, int* parent) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int L = label[p];
  if (L == 0) return;
  const int x = p % w, y = p / w;
  if (x > 0 && x % CCL_T == 0 && label[p - 1] == L) ccl_union_g(parent, p, p - 1);
  if (y > 0 && y % CCL_T == 0 && label[p - w] == L) ccl_union_g(parent, p, p - w);
}

__global__ __launch_bounds__(256) void ccl_flatten_kernel(const int* label, int n, const int* parent, int* root) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int a = -1;
  if (label[p] != 0) {
    a = p;
    int q;
    while ((q = parent[a]) != a) a = q;
  }
  root[p] = a;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Compressing the ids that occur.  id(p) = root at the pixel, or at its centroid; a centroid outside the image counts as background.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ins_pixel_id(const int* root, const int* cent, int h, int w, int p) {
  if (!cent) return root[p];
  const int y = cent[p], x = cent[h * w + p];
  if (y < 0 || y >= h || x < 0 || x >= w) return -1;
  return root[y * w + x];
}

__global__ __launch_bounds__(256) void id_mark_kernel(const int* root, const int* cent, int h, int w, int* marks) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int id = ins_pixel_id(root, cent, h, w, p);
  if (id >= -1 && id < h * w) marks[id + 1] = 1;          // the same value from every writer
}

// one workgroup: every thread sums a contiguous chunk, the 1024 chunk sums are scanned in LDS, every thread writes its chunk's prefixes
__global__ __launch_bounds__(1024) void id_rank_kernel(const int* marks, int n1, int* rank, int* count) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int chunk = (n1 + 1023) / 1024;
  const int lo = min(t * chunk, n1), hi = min(lo + chunk, n1);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += marks[i];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int i = lo; i < hi; ++i) {
    const int m = marks[i];
    rank[i] = run;
    run += m;
  }
  if (t == 1023) {
    count[0] = part[1023];
    count[1] = marks[0];
  }
}

__global__ __launch_bounds__(256) void id_apply_kernel(const int* root, const int* cent, int h, int w, const int* rank, int* out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  int id = ins_pixel_id(root, cent, h, w, p);
  if (id < -1 || id >= h * w) id = -1;
  out[p] = rank[id + 1];
}

// Step 3
__global__ __launch_bounds__(256) void ins_split_kernel(const float* cam, const int* cluster, int I, int n, long total, float* x) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long c = i / n;
    const int p = (int)(i - c * n);
    const int k = (int)(c / I), ii = (int)(c - (long)k * I);
    x[i] = cluster[p] == ii ? cam[(long)k * n + p] : 0.f;
  }
}

// Step 5: irn_label_kernel (irn.hip) with an int32 label, the winning value instead of every value, and no limit on C
__global__ __launch_bounds__(256) void ins_finish_kernel(const float* rw, int C, int h, int w, int H, int W, const unsigned* mx_bits,
                                                         float bg_thres, int* label, float* win) {
  const float mx = __uint_as_float(mx_bits[0]);
  const long total = (long)H * W;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
    const int X = (int)(p % W), Y = (int)(p / W);
    float best = bg_thres;
    int bk = 0;
    for (int c = 0; c < C; ++c) {
      const float v = irn_soft_value(rw + (long)c * h * w, h, w, Y, X, mx);
      if (v > best) { best = v; bk = c + 1; }
    }
    label[p] = bk;
    win[p] = best;
  }
}

// Step 6
__global__ __launch_bounds__(256) void seg_stats_kernel(const int* label, const int* root, const float* win, const int* rank,
                                                        const int* marks, int n, int nseg, int* area, unsigned* score_bits,
                                                        int* seg_label, int* seg_first) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int r = root[p];
  if (r < 0 || r >= n) return;
  const int s = rank[r + 1] - marks[0];
  if (s < 0 || s >= nseg) return;
  atomicAdd(&area[s], 1);
  atomicMax(&score_bits[s], __float_as_uint(win[p]));          // win >= 0: bit order == value order
  if (r == p) {
    seg_label[s] = label[p];
    seg_first[s] = p;
  }
}

__global__ __launch_bounds__(256) void seg_map_kernel(const int* root, const int* rank, const int* marks, const int* order, int n,
                                                      int nseg, int* seg_map) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int r = root[p];
  int v = 0;
  if (r >= 0 && r < n) {
    const int s = rank[r + 1] - marks[0];
    if (s >= 0 && s < nseg) v = order[s] + 1;
  }
  seg_map[p] = v;
}

extern "C" {

int mx_irn_centroids(const float* dp, int h, int w, int iterations, int* cent, void* stream) {
  MX_CHECK_ARG(dp && cent && h > 0 && w > 0 && iterations >= 0 && (long)h * w < (1L << 30), "irn_centroids: bad args");
  hipStream_t st = (hipStream_t)stream;
  const int n = h * w;
  const long bytes = 8L * n;
  if (bytes <= INS_LDS_BUDGET) {
    if (bytes > 64 * 1024) {
      const int rc = mx_dyn_lds_optin(reinterpret_cast<const void*>(&irn_centroids_kernel<true>), INS_LDS_BUDGET);
      if (rc != MX_OK) return rc;
    }
    hipLaunchKernelGGL(irn_centroids_kernel<true>, dim3(cdiv(n, 256)), dim3(256), (size_t)bytes, st, dp, h, w, iterations, cent);
  } else {
    hipLaunchKernelGGL(irn_centroids_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, st, dp, h, w, iterations, cent);
  }
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_irn_weak(const float* dp, int h, int w, float thres, int* weak, void* stream) {
  MX_CHECK_ARG(dp && weak && h > 0 && w > 0 && (long)h * w < (1L << 30), "irn_weak: bad args");
  hipLaunchKernelGGL(irn_weak_kernel, dim3(cdiv((long)h * w, 256)), dim3(256), 0, (hipStream_t)stream, dp, h * w, thres, weak);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

long mx_ccl_ws(int h, int w) {
  if (h <= 0 || w <= 0 || (long)h * w >= (1L << 31) - 1) return -1;
  return 4L * h * w;
}

int mx_ccl(const int* label, int h, int w, int* root, void* ws, void* stream) {
  MX_CHECK_ARG(label && root && ws && mx_ccl_ws(h, w) > 0 && cdiv(h, CCL_T) <= 65535, "ccl: bad args");
  hipStream_t st = (hipStream_t)stream;
  int* parent = (int*)ws;
  const int n = h * w;
  hipLaunchKernelGGL(ccl_tile_kernel, dim3(cdiv(w, CCL_T), cdiv(h, CCL_T)), dim3(CCL_T * CCL_T), 0, st, label, h, w, parent);
  hipLaunchKernelGGL(ccl_border_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, label, h, w, parent);
  hipLaunchKernelGGL(ccl_flatten_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, label, n, (const int*)parent, root);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_id_mark(const int* root, const int* cent, int h, int w, int* marks, void* stream) {
  MX_CHECK_ARG(root && marks && h > 0 && w > 0 && (long)h * w < (1L << 30), "id_mark: bad args (h*w < 2^30)");
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)h * w;
  hipMemsetAsync(marks, 0, sizeof(int) * (size_t)(n + 1), st);
  hipLaunchKernelGGL(id_mark_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, root, cent, h, w, marks);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_id_rank(const int* marks, int n1, int* rank, int* count, void* stream) {
  MX_CHECK_ARG(marks && rank && count && n1 > 0 && n1 <= (1 << 30), "id_rank: bad args (n1 <= 2^30: the chunk bounds are int)");
  hipLaunchKernelGGL(id_rank_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, marks, n1, rank, count);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_id_apply(const int* root, const int* cent, int h, int w, const int* rank, int* out, void* stream) {
  MX_CHECK_ARG(root && rank && out && h > 0 && w > 0 && (long)h * w < (1L << 30), "id_apply: bad args (h*w < 2^30)");
  hipLaunchKernelGGL(id_apply_kernel, dim3(cdiv((long)h * w, 256)), dim3(256), 0, (hipStream_t)stream, root, cent, h, w, rank, out);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_irn_ins_split(const float* cam, const int* cluster, int K, int I, int n, float* x, void* stream) {
  MX_CHECK_ARG(cam && cluster && x && K > 0 && I > 0 && n > 0, "irn_ins_split: bad args");
  const long total = (long)K * I * n;
  long blocks = (total + 255) / 256;
  if (blocks > 65535) blocks = 65535;
  hipLaunchKernelGGL(ins_split_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cam, cluster, I, n, total, x);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_irn_ins_finish(const float* rw, int C, int h, int w, int H, int W, float bg_thres, const unsigned* max_scratch, int* label,
                      float* win, void* stream) {
  MX_CHECK_ARG(rw && max_scratch && label && win && C > 0 && h > 0 && w > 0 && H > 0 && W > 0 && H <= 4 * h && W <= 4 * w,
               "irn_ins_finish: bad args (the label map is the top-left HxW crop of the 4x upsampled maps)");
  long b = ((long)H * W + 255) / 256;
  if (b > 65535) b = 65535;
  hipLaunchKernelGGL(ins_finish_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, rw, C, h, w, H, W, max_scratch, bg_thres,
                     label, win);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_seg_stats(const int* label, const int* root, const float* win, const int* rank, const int* marks, int n, int nseg, int* area,
                 unsigned* score_bits, int* seg_label, int* seg_first, void* stream) {
  MX_CHECK_ARG(label && root && win && rank && marks && area && score_bits && seg_label && seg_first && n > 0 && nseg > 0 && nseg <= n,
               "seg_stats: bad args");
  hipStream_t st = (hipStream_t)stream;
  hipMemsetAsync(area, 0, sizeof(int) * (size_t)nseg, st);
  hipMemsetAsync(score_bits, 0, sizeof(unsigned) * (size_t)nseg, st);
  hipLaunchKernelGGL(seg_stats_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, label, root, win, rank, marks, n, nseg, area, score_bits,
                     seg_label, seg_first);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_seg_map(const int* root, const int* rank, const int* marks, const int* order, int n, int nseg, int* seg_map, void* stream) {
  MX_CHECK_ARG(root && rank && marks && order && seg_map && n > 0 && nseg > 0, "seg_map: bad args");
  hipLaunchKernelGGL(seg_map_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, root, rank, marks, order, n, nseg, seg_map);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
