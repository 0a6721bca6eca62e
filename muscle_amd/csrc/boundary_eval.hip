// Boundary evaluation ("Boundary evaluation"): the Chebyshev distance of every pixel of a label map to the nearest pixel
// with another label, cut at dmax + 1, and the integer count table from which trimap mIoU and Boundary IoU follow on the host.
// Integer counts and integer atomic adds only, no floating point: no result depends on the order in which threads arrive.
//
// mx_label_edge_dist runs the SEPARABLE form inside one workgroup: a tile of BD_TH x BD_TW output pixels is staged in LDS with a halo of
// dmax labels on every side, a row pass writes for each of the BD_TH + 2 dmax staged rows the distance to the nearest change in that row,
// and a column pass takes min over dy of (label differs ? |dy| : max(|dy|, row value)).  The work per pixel is O(dmax), where scanning
// the (2 dmax + 1)^2 window directly is O(dmax^2) (16 641 labels at dmax 64); keeping both passes in one workgroup needs no scratch
// buffer between them (the library never allocates) at the price of running the row pass over the 2 dmax halo rows again.
// The staged entries are 16 bits wide, so that the scans need no coordinate test: every byte, 255 included, is an ordinary label, and
//   edge = 1: a position outside the image holds BD_OUT, which differs from every label;
//   edge = 0: a position outside the image holds the label of the nearest pixel inside (clamped coordinates).  Such a copy never offers
//             a smaller distance than the pixel it copies, which lies on the way to it: the minimum is unchanged.
// LDS: 2 (BD_TH + 2 dmax)(BD_TW + 2 dmax) + (BD_TH + 2 dmax) BD_TW bytes: 12 KiB at dmax 16, 63 KiB at dmax 64.
#include "common.h"

#define BD_T 256                   // threads per workgroup
#define BD_TW 64                   // tile width
#define BD_TH 16                   // tile height
#define BD_MAXD 64                 // largest radius
#define BD_OUT 0x100               // staged entry of a position outside the image with edge = 1
#define BD_MAXK 32                 // most classes of the count table

__global__ __launch_bounds__(BD_T) void label_edge_dist_kernel(const unsigned char* label, int H, int W, int dmax, int edge,
                                                               unsigned char* dist) {
  extern __shared__ unsigned short bd_lds[];
  const int LW = BD_TW + 2 * dmax, LH = BD_TH + 2 * dmax;
  unsigned short* lab = bd_lds;                                                  // [LH][LW]: rows y0 - dmax .., columns x0 - dmax ..
  unsigned char* rd = reinterpret_cast<unsigned char*>(bd_lds + LH * LW);        // [LH][BD_TW]: row distances of the tile's columns
  const int x0 = blockIdx.x * BD_TW, y0 = blockIdx.y * BD_TH;
  for (int i = threadIdx.x; i < LH * LW; i += BD_T) {
    const int ly = i / LW, lx = i - ly * LW;
    const int y = y0 - dmax + ly, x = x0 - dmax + lx;
    const int yc = min(max(y, 0), H - 1), xc = min(max(x, 0), W - 1);
    const unsigned short v = label[(long)yc * W + xc];
    lab[i] = (edge && (y != yc || x != xc)) ? BD_OUT : v;
  }
  __syncthreads();
  // row pass: nearest position of the row whose entry differs.  From dmax down to 1, so the nearest hit is the last one written: no early
  // exit and no coordinate test.  Both entries are READ before either is tested (`a != c || b != c` on the array elements makes the second
  // read conditional, and every read then waits for the one before it: a full LDS latency per step with one wave per SIMD).  row[-d] and
  // row[d] lie in the staged row for every d <= dmax.
  for (int i = threadIdx.x; i < LH * BD_TW; i += BD_T) {
    const int ly = i / BD_TW, tx = i - ly * BD_TW;
    const unsigned short* row = lab + ly * LW + dmax + tx;
    const unsigned short c = row[0];
    int best = dmax + 1;
#pragma unroll 8
    for (int d = dmax; d >= 1; --d) {
      const unsigned short a = row[-d], b = row[d];
      best = ((a != c) | (b != c)) ? d : best;
    }
    rd[i] = (unsigned char)best;
  }
  __syncthreads();
  // column pass: the rows y - d and y + d lie in the staged tile for every d <= dmax
  for (int i = threadIdx.x; i < BD_TH * BD_TW; i += BD_T) {
    const int ty = i / BD_TW, tx = i - ty * BD_TW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    const int ly = ty + dmax;
    const unsigned short* lc = lab + ly * LW + dmax + tx;
    const unsigned char* rc = rd + ly * BD_TW + tx;
    const unsigned short c = lc[0];
    int best = rc[0];
#pragma unroll 4
    for (int d = dmax; d >= 1; --d) {
      const unsigned short lu = lc[-d * LW], ld = lc[d * LW];
      const int ru = rc[-d * BD_TW], rdn = rc[d * BD_TW];         // read unconditionally, as in the row pass
      const int up = (lu != c) ? 0 : ru;
      const int dn = (ld != c) ? 0 : rdn;
      best = min(best, max(d, min(up, dn)));
    }
    dist[(long)y * W + x] = (unsigned char)best;
  }
}

// hist int64 [6][K][dmax + 2], ratio int64 [3][K], both accumulated.  Every workgroup counts its pixels into an int32 copy of hist in LDS
// and adds the non-zero cells once; the ratio rows are the sums of bins 1..d_img of this image's rows 3..5, taken from the LDS copy.
// A distance outside 1..dmax + 1 (a map that mx_label_edge_dist did not write) is cut to that range and never leaves the table.
__global__ __launch_bounds__(BD_T) void boundary_counts_kernel(const unsigned char* pred, const unsigned char* gt, const unsigned char* dt,
                                                               const unsigned char* db, const unsigned char* dp, int K, long HW, int dmax,
                                                               int d_img, long long* hist, long long* ratio) {
  extern __shared__ int bc_lds[];                // [6][K][dmax + 2]
  const int NB = dmax + 2, row = K * NB, cells = 6 * row;
  for (int i = threadIdx.x; i < cells; i += BD_T) bc_lds[i] = 0;
  __syncthreads();
  for (long i = blockIdx.x * (long)BD_T + threadIdx.x; i < HW; i += (long)gridDim.x * BD_T) {
    const int g = gt[i];
    if (g == 255) continue;
    const int p = pred[i];
    const int bt = min(max((int)dt[i], 1), dmax + 1), bb = min(max((int)db[i], 1), dmax + 1), bp = min(max((int)dp[i], 1), dmax + 1);
    if (g < K) {
      atomicAdd(&bc_lds[0 * row + g * NB + bt], 1);
      atomicAdd(&bc_lds[3 * row + g * NB + bb], 1);
      if (p == g) {
        atomicAdd(&bc_lds[2 * row + g * NB + bt], 1);
        atomicAdd(&bc_lds[5 * row + g * NB + max(bb, bp)], 1);
      }
    }
    if (p < K) {
      atomicAdd(&bc_lds[1 * row + p * NB + bt], 1);
      atomicAdd(&bc_lds[4 * row + p * NB + bp], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += BD_T) {
    const int v = bc_lds[i];
    if (v) atomicAdd((unsigned long long*)&hist[i], (unsigned long long)v);
  }
  for (int i = threadIdx.x; i < 3 * K; i += BD_T) {
    const int* h = bc_lds + 3 * row + i * NB;    // rows 3..5 are contiguous: i = r * K + k
    int s = 0;
    for (int b = 1; b <= d_img; ++b) s += h[b];
    if (s) atomicAdd((unsigned long long*)&ratio[i], (unsigned long long)s);
  }
}

extern "C" {

int mx_label_edge_dist(const unsigned char* label, int H, int W, int dmax, int edge, unsigned char* dist, void* stream) {
  MX_CHECK_ARG(label && dist, "label_edge_dist: null pointer");
  MX_CHECK_ARG(H > 0 && W > 0 && (long)H * W < (1L << 31) && H <= 65535 * BD_TH,
               "label_edge_dist: H, W must be positive with H*W < 2^31 and H <= %d (got %d x %d)", 65535 * BD_TH, H, W);
  MX_CHECK_ARG(dmax >= 1 && dmax <= BD_MAXD, "label_edge_dist: dmax must be in 1..%d (got %d)", BD_MAXD, dmax);
  MX_CHECK_ARG(edge == 0 || edge == 1, "label_edge_dist: edge must be 0 or 1 (got %d)", edge);
  const size_t lds = 2 * (size_t)(BD_TH + 2 * dmax) * (size_t)(BD_TW + 2 * dmax) + (size_t)(BD_TH + 2 * dmax) * BD_TW;   // <= 64 512 bytes
  hipLaunchKernelGGL(label_edge_dist_kernel, dim3(cdiv(W, BD_TW), cdiv(H, BD_TH)), dim3(BD_T), lds, (hipStream_t)stream, label, H, W, dmax,
                     edge, dist);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_boundary_counts(const unsigned char* pred, const unsigned char* gt, const unsigned char* dt, const unsigned char* db,
                       const unsigned char* dp, int K, int H, int W, int dmax, int d_img, long long* hist, long long* ratio, void* stream) {
  MX_CHECK_ARG(pred && gt && dt && db && dp && hist && ratio, "boundary_counts: null pointer");
  MX_CHECK_ARG(K >= 2 && K <= BD_MAXK, "boundary_counts: K must be in 2..%d (got %d)", BD_MAXK, K);
  MX_CHECK_ARG(H > 0 && W > 0 && (long)H * W < (1L << 31), "boundary_counts: H, W must be positive with H*W < 2^31 (got %d x %d)", H, W);
  MX_CHECK_ARG(dmax >= 1 && dmax <= BD_MAXD, "boundary_counts: dmax must be in 1..%d (got %d)", BD_MAXD, dmax);
  MX_CHECK_ARG(d_img >= 1 && d_img <= dmax, "boundary_counts: d_img must be in 1..dmax (got %d, dmax %d)", d_img, dmax);
  const long HW = (long)H * W;
  long blocks = (HW + BD_T * 8 - 1) / (BD_T * 8);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(boundary_counts_kernel, dim3((unsigned)blocks), dim3(BD_T), sizeof(int) * 6 * (size_t)K * (size_t)(dmax + 2),
                     (hipStream_t)stream, pred, gt, dt, db, dp, K, HW, dmax, d_img, hist, ratio);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
