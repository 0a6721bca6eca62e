// Instance-segmentation evaluation ("Instance evaluation"): the integer joint-count table of a prediction against the
// ground-truth instance map, from which every mask IoU at every threshold follows on the host.  One pass over the pixels.
// Integer counts and integer atomic adds only, no floating point: no result depends on the order in which threads arrive.
//
// Both kernels walk the pixels in groups of 16 that are 16-BYTE ALIGNED IN THE BYTE ARRAY they read packed (b in the label form, the
// mask row or b in the mask form): group g covers the pixels [16 g - mis, 16 g - mis + 16) cut to [0, n_pix), mis = address & 15.  A group
// that lies wholly inside is one 16-byte load; the first and last group of an array (unaligned start, ragged end) are read byte by byte
// under the bounds test.  No load ever leaves [0, n_pix).
// Neighbouring pixels nearly always carry the same pair, so every thread keeps (current cell, run length) and adds only when the cell
// changes: a checkerboard costs one add per pixel, a flat image one add per thread.  The adds go to LDS first (the whole table where it
// has at most PAIR_LDS_CELLS cells, a small hash of cells otherwise) and from there to the table once per workgroup.
// A value outside its range never forms an index: the pixel is counted in bad[0] and skipped.
#include "common.h"

#define PAIR_T 256                 // threads per workgroup
#define PAIR_G 16                  // pixels per group
#define PAIR_LDS_CELLS 8192        // a table up to this many cells (32 KiB) is accumulated in LDS, one global add per non-zero cell and workgroup
#define PAIR_MAX_CELLS (1L << 26)
#define PAIR_HASH 1024             // a larger table: this many (cell, count) slots of LDS in front of the global adds
#define PAIR_ROW_BLOCKS 64         // mask form: at most this many workgroups share one mask row

struct PairRun {
  int cell;                        // -1: no run open
  int count;
};
// LDS = true: `tile` is the table itself (or the mask form's histogram).  LDS = false: `tile` is PAIR_HASH keys followed by PAIR_HASH
// counts; a run whose cell owns or can claim its slot is added there, any other goes to `table` at once.  The cells that many threads hit
// (the background row, a large segment on a large object) thus reach `table` once per workgroup: adds to ONE global address are serial.
template <bool LDS>
__device__ __forceinline__ void pair_flush(const PairRun& r, int* tile, int* table) {
  if (r.cell < 0) return;
  if (LDS) {
    atomicAdd(&tile[r.cell], r.count);
  } else {
    const unsigned slot = ((unsigned)r.cell * 2654435761u) >> 22;             // 10 bits
    const int prev = atomicCAS(&tile[slot], -1, r.cell);
    if (prev == -1 || prev == r.cell) atomicAdd(&tile[PAIR_HASH + slot], r.count);
    else atomicAdd(&table[r.cell], r.count);
  }
}
template <bool LDS>
__device__ __forceinline__ void pair_push(PairRun& r, int cell, int* tile, int* table) {
  if (cell == r.cell) { ++r.count; return; }
  pair_flush<LDS>(r, tile, table);
  r.cell = cell;
  r.count = 1;
}
__device__ __forceinline__ unsigned pair_byte(const uint4& v, int k) {
  const unsigned w = k < 8 ? (k < 4 ? v.x : v.y) : (k < 12 ? v.z : v.w);
  return (w >> (8 * (k & 3))) & 255u;
}

// table[a[i]][b[i]] += 1.  mis = address of b & 15; a_vec: a + (16 g - mis) is 16-byte aligned (the same for every g).
template <bool LDS>
__global__ __launch_bounds__(PAIR_T) void label_pair_kernel(const int* a, const unsigned char* b, long n_pix, int A, int B, int cells, int mis,
                                                            int a_vec, long groups, int* table, int* bad) {
  extern __shared__ int pair_tile[];
  if (LDS) {
    for (int c = threadIdx.x; c < cells; c += PAIR_T) pair_tile[c] = 0;
  } else {
    for (int c = threadIdx.x; c < PAIR_HASH; c += PAIR_T) { pair_tile[c] = -1; pair_tile[PAIR_HASH + c] = 0; }
  }
  __syncthreads();
  const int B1 = B + 1;
  PairRun run = {-1, 0};
  int nbad = 0;
  for (long g = (long)blockIdx.x * PAIR_T + threadIdx.x; g < groups; g += (long)gridDim.x * PAIR_T) {
    const long i0 = g * PAIR_G - mis;
    if (i0 >= 0 && i0 + PAIR_G <= n_pix) {
      const uint4 bv = *reinterpret_cast<const uint4*>(b + i0);
      int av[PAIR_G];
      if (a_vec) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int4 t = *reinterpret_cast<const int4*>(a + i0 + 4 * q);
          av[4 * q] = t.x; av[4 * q + 1] = t.y; av[4 * q + 2] = t.z; av[4 * q + 3] = t.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < PAIR_G; ++k) av[k] = a[i0 + k];
      }
#pragma unroll
      for (int k = 0; k < PAIR_G; ++k) {
        const int x = av[k];
        const int y = (int)pair_byte(bv, k);
        if (x < 0 || x > A || y > B) { ++nbad; continue; }
        pair_push<LDS>(run, x * B1 + y, pair_tile, table);
      }
    } else {
      for (int k = 0; k < PAIR_G; ++k) {
        const long i = i0 + k;
        if (i < 0 || i >= n_pix) continue;
        const int x = a[i];
        const int y = (int)b[i];
        if (x < 0 || x > A || y > B) { ++nbad; continue; }
        pair_push<LDS>(run, x * B1 + y, pair_tile, table);
      }
    }
  }
  pair_flush<LDS>(run, pair_tile, table);
  if (nbad) atomicAdd(bad, nbad);
  __syncthreads();
  if (LDS) {
    for (int c = threadIdx.x; c < cells; c += PAIR_T) {
      const int v = pair_tile[c];
      if (v) atomicAdd(&table[c], v);
    }
  } else {
    for (int c = threadIdx.x; c < PAIR_HASH; c += PAIR_T) {
      const int key = pair_tile[c], v = pair_tile[PAIR_HASH + c];
      if (key >= 0 && key < cells && v) atomicAdd(&table[key], v);
    }
  }
}

// Workgroup row r = blockIdx.x of the table: r = 0 is the histogram of b over every pixel (and the only row that counts bad values, so
// each is counted once); r >= 1 counts b over the set pixels of mask r - 1.  blockIdx.y of gridDim.y workgroups share the row.  The packed
// array is b for row 0 and the mask row otherwise; b under a set mask pixel is a byte load (mask rows start at any alignment against b).
__global__ __launch_bounds__(PAIR_T) void mask_pair_kernel(const unsigned char* masks, const unsigned char* b, long n_pix, int B, int* table,
                                                           int* bad) {
  __shared__ int hist[256];
  hist[threadIdx.x] = 0;                                       // PAIR_T == 256 bins
  __syncthreads();
  const int r = blockIdx.x;
  const unsigned char* src = r ? masks + (size_t)(r - 1) * (size_t)n_pix : b;
  const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 15);
  const long groups = (n_pix + mis + PAIR_G - 1) / PAIR_G;
  PairRun run = {-1, 0};
  int nbad = 0;
  for (long g = (long)blockIdx.y * PAIR_T + threadIdx.x; g < groups; g += (long)gridDim.y * PAIR_T) {
    const long i0 = g * PAIR_G - mis;
    uint4 sv = make_uint4(0u, 0u, 0u, 0u);
    const bool whole = i0 >= 0 && i0 + PAIR_G <= n_pix;
    if (whole) {
      sv = *reinterpret_cast<const uint4*>(src + i0);
      if (r && !(sv.x | sv.y | sv.z | sv.w)) continue;         // 16 unset pixels
    }
#pragma unroll
    for (int k = 0; k < PAIR_G; ++k) {
      const long i = i0 + k;
      unsigned s;
      if (whole) s = pair_byte(sv, k);
      else if (i < 0 || i >= n_pix) continue;
      else s = src[i];
      int y;
      if (r) {
        if (!s) continue;
        y = (int)b[i];
        if (y > B) continue;
      } else {
        y = (int)s;
        if (y > B) { ++nbad; continue; }
      }
      pair_push<true>(run, y, hist, nullptr);
    }
  }
  pair_flush<true>(run, hist, nullptr);
  if (nbad) atomicAdd(bad, nbad);
  __syncthreads();
  const int v = hist[threadIdx.x];
  if ((int)threadIdx.x <= B && v) atomicAdd(&table[(size_t)r * (size_t)(B + 1) + threadIdx.x], v);
}

extern "C" {

int mx_label_pair_counts(const int* a, const unsigned char* b, long n_pix, int A, int B, int* table, int* bad, void* stream) {
  MX_CHECK_ARG(a && b && table && bad, "label_pair_counts: null pointer");
  MX_CHECK_ARG(n_pix > 0 && n_pix < (1L << 31), "label_pair_counts: n_pix must be in 1..2^31-1 (got %ld)", n_pix);
  MX_CHECK_ARG(A >= 0 && B >= 0 && B <= 255, "label_pair_counts: A >= 0 and 0 <= B <= 255 are needed (got A=%d B=%d)", A, B);
  const long cells = ((long)A + 1) * (B + 1);
  MX_CHECK_ARG(cells <= PAIR_MAX_CELLS, "label_pair_counts: the table has %ld cells, at most 2^26 are supported", cells);
  hipStream_t st = (hipStream_t)stream;
  hipMemsetAsync(table, 0, sizeof(int) * (size_t)cells, st);
  hipMemsetAsync(bad, 0, sizeof(int), st);
  const int mis = (int)(reinterpret_cast<uintptr_t>(b) & 15);
  const int a_vec = ((reinterpret_cast<uintptr_t>(a) - 4u * (uintptr_t)mis) & 15) == 0;
  const long groups = (n_pix + mis + PAIR_G - 1) / PAIR_G;
  long blocks = (groups + PAIR_T - 1) / PAIR_T;
  if (blocks > 1024) blocks = 1024;
  if (cells <= PAIR_LDS_CELLS)
    hipLaunchKernelGGL(label_pair_kernel<true>, dim3((unsigned)blocks), dim3(PAIR_T), sizeof(int) * (size_t)cells, st, a, b, n_pix, A, B,
                       (int)cells, mis, a_vec, groups, table, bad);
  else
    hipLaunchKernelGGL(label_pair_kernel<false>, dim3((unsigned)blocks), dim3(PAIR_T), sizeof(int) * 2 * PAIR_HASH, st, a, b, n_pix, A, B, (int)cells, mis, a_vec,
                       groups, table, bad);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

int mx_mask_pair_counts(const unsigned char* masks, const unsigned char* b, long n_pix, int n, int B, int* table, int* bad, void* stream) {
  MX_CHECK_ARG(b && table && bad && (masks || n == 0), "mask_pair_counts: null pointer");
  MX_CHECK_ARG(n_pix > 0 && n_pix < (1L << 31), "mask_pair_counts: n_pix must be in 1..2^31-1 (got %ld)", n_pix);
  MX_CHECK_ARG(n >= 0 && B >= 0 && B <= 255, "mask_pair_counts: n >= 0 and 0 <= B <= 255 are needed (got n=%d B=%d)", n, B);
  const long cells = ((long)n + 1) * (B + 1);
  MX_CHECK_ARG(cells <= PAIR_MAX_CELLS, "mask_pair_counts: the table has %ld cells, at most 2^26 are supported", cells);
  hipStream_t st = (hipStream_t)stream;
  hipMemsetAsync(table, 0, sizeof(int) * (size_t)cells, st);
  hipMemsetAsync(bad, 0, sizeof(int), st);
  long per_row = (n_pix / PAIR_G + 1 + 4 * PAIR_T - 1) / (4 * PAIR_T);      // about four groups per thread
  if (per_row > PAIR_ROW_BLOCKS) per_row = PAIR_ROW_BLOCKS;
  hipLaunchKernelGGL(mask_pair_kernel, dim3((unsigned)(n + 1), (unsigned)per_row), dim3(PAIR_T), 0, st, masks, b, n_pix, B, table, bad);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

}  // extern "C"
