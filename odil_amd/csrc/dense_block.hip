// The dense block of the Newton normal equations on the matrix cores.
//
// `Problem.linearize` gives `Array` / `NeuralNet` unknowns DENSE Jacobian columns (reference
// src/odil/core.py:1189-1203): D is (rows = residual values) x (p = a few dozen parameters).  The normal equations
// (reference src/odil/linsolver.py:17-23) need D^T D, D^T r and, for the Schur complement against the stencil part,
// (S^T D)^T Z -- all products X^T Y of two tall, skinny matrices.  One workgroup of four waves walks a contiguous
// range of rows four at a time: lane l holds X[r + l/16][16 ti + l%16] and Y[r + l/16][16 tj + l%16], which ARE the
// A and B operands of v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 for the 16 x 16 tile (ti, tj) of the result,
// so every pair of column tiles is one MFMA per four rows with no shuffling.  Partial results: waves of a workgroup
// are summed through LDS in wave order, workgroups in index order by a second kernel -- bit-reproducible.
//
// More than 64 columns (odil_dense_block_xty_wide, up to kGramWideMax = 1024 per operand): the operands are cut into
// panels of 64 columns and the grid gets two more dimensions, (row range, X panel, Y panel); a workgroup runs the same
// 4 x 4 tile body on one pair of panels over its row range and a final kernel sums the row ranges of every pair in
// index order, in double.  When both operands are the same matrix (X = Y, same row stride, px <= py: D^T D and D^T [D |
// r]) only the pairs on or above the diagonal are computed and the final kernel writes out[i][j], i > j, from the
// partials of out[j][i], so that the Gram block is symmetric to the bit.  COST: every X panel is read once per Y panel
// (and the reverse), i.e. the operands are read ~ (number of panels) times, not once; the 64-column slice of a wider
// row is also a strided access (128 contiguous bytes per tile and row in f64).  WORKSPACE: the number of row ranges is
// kGramWideGroups / (pairs of panels), at least 1 and at most kGramBlocks, so that the partials never exceed
// kGramWideGroups = 2048 blocks of 64 x 64 doubles = 64 MiB (reached at 1024 x 1024 columns: 256 pairs x 8 ranges),
// whatever the column counts: odil_dense_block_wide_workspace_bytes(px, py) <= 64 MiB.  Two costs of the symmetric
// case: the grid still has its nbx (nbx - 1) / 2 x (row ranges) workgroups below the diagonal, which exit at once, and
// the number of row ranges is taken from ALL pairs although only those on or above the diagonal fill their slots (about
// half the workspace and half the row ranges that the bound would allow).
#include "common.h"

namespace odil {

constexpr int kGramTile = 16;
constexpr int kGramMaxTiles = 4;   // up to 64 columns per operand
constexpr int kGramBlocks = 256;   // workgroups (= partial results)
constexpr int kGramWaves = kBlock / 64;
constexpr int kGramPanel = kGramTile * kGramMaxTiles;  // columns of one panel of the wide entry
constexpr int kGramWideMax = 1024;                     // columns per operand of the wide entry
constexpr int kGramWideGroups = 2048;                  // most (row range, panel pair) partials: 2048 x 32 KB = 64 MiB

template <typename T> struct Acc4 { typedef T type __attribute__((ext_vector_type(4))); };

__device__ inline Acc4<double>::type mfma_16x16x4(double a, double b, Acc4<double>::type c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
__device__ inline Acc4<float>::type mfma_16x16x4(float a, float b, Acc4<float>::type c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// row of accumulator register `reg` held by `lane` (cdna_hip_programming.md, fragment layout): f64 and f32 differ
template <typename T> __device__ inline int acc_row(int lane, int reg);
template <> __device__ inline int acc_row<double>(int lane, int reg) { return (lane >> 4) + 4 * reg; }
template <> __device__ inline int acc_row<float>(int lane, int reg) { return (lane >> 4) * 4 + reg; }

// out[i][j] = sum over the rows of range `b` of `nb` of X[r][i] Y[r][j]   (i < 16 TX, j < 16 TY, zero padded): the work
// of one workgroup
template <typename T, int TX, int TY>
__device__ inline void xty_range(const T* __restrict__ x, const T* __restrict__ y, int64_t n, int px, int py,
                                 int64_t ldx, int64_t ldy, int b, int nb, T* __restrict__ out) {
  typedef typename Acc4<T>::type A4;
  __shared__ T red[kGramWaves][TX * TY][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, krow = lane >> 4;
  // contiguous row range of this workgroup, a multiple of 4 * kGramWaves rows long
  const int64_t quads = (n + 3) / 4;
  const int64_t per = (quads + nb - 1) / nb;
  const int64_t q0 = (int64_t)b * per, q1 = q0 + per < quads ? q0 + per : quads;
  A4 acc[TX][TY];
#pragma unroll
  for (int i = 0; i < TX; ++i)
#pragma unroll
    for (int j = 0; j < TY; ++j) acc[i][j] = A4{T(0), T(0), T(0), T(0)};
  for (int64_t q = q0 + wave; q < q1; q += kGramWaves) {
    const int64_t r = 4 * q + krow;
    T xv[TX], yv[TY];
#pragma unroll
    for (int i = 0; i < TX; ++i) {
      const int c = kGramTile * i + col;
      xv[i] = (r < n && c < px) ? x[r * ldx + c] : T(0);
    }
#pragma unroll
    for (int j = 0; j < TY; ++j) {
      const int c = kGramTile * j + col;
      yv[j] = (r < n && c < py) ? y[r * ldy + c] : T(0);
    }
#pragma unroll
    for (int i = 0; i < TX; ++i)
#pragma unroll
      for (int j = 0; j < TY; ++j) acc[i][j] = mfma_16x16x4(xv[i], yv[j], acc[i][j]);
  }
#pragma unroll
  for (int i = 0; i < TX; ++i)
#pragma unroll
    for (int j = 0; j < TY; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wave][i * TY + j][e][lane] = acc[i][j][e];
  __syncthreads();
  // waves summed in order by the threads of wave 0's shape: every thread takes some (tile, reg, lane) entries
  for (int k = threadIdx.x; k < TX * TY * 4 * 64; k += kBlock) {
    const int l = k & 63, e = (k >> 6) & 3, t = k >> 8;
    T s = red[0][t][e][l];
#pragma unroll
    for (int w = 1; w < kGramWaves; ++w) s = s + red[w][t][e][l];
    const int ti = t / TY, tj = t - ti * TY;
    const int row = kGramTile * ti + acc_row<T>(l, e), cc = kGramTile * tj + (l & 15);
    out[row * (kGramTile * TY) + cc] = s;
  }
}

// partial[b][i][j] = the sum of workgroup b
template <typename T, int TX, int TY>
__global__ __launch_bounds__(kBlock) void k_xty_partial(const T* __restrict__ x, const T* __restrict__ y, int64_t n,
                                                       int px, int py, int64_t ldx, int64_t ldy,
                                                       T* __restrict__ partial) {
  xty_range<T, TX, TY>(x, y, n, px, py, ldx, ldy, blockIdx.x, gridDim.x,
                       partial + (int64_t)blockIdx.x * (kGramTile * TX) * (kGramTile * TY));
}

// Position of the pair (X panel bi, Y panel bj) among the `pairs` that are computed: all of them, or (sym) those with
// bi <= bj, row by row.
__host__ __device__ inline int wide_pairs(int nbx, int nby, bool sym) {
  return nbx * nby - (sym ? nbx * (nbx - 1) / 2 : 0);
}
__host__ __device__ inline int wide_pair(int bi, int bj, int nby, bool sym) {
  return sym ? bi * nby - bi * (bi - 1) / 2 + (bj - bi) : bi * nby + bj;
}

// partial[b][pair][64][64]: grid (row ranges, X panels, Y panels), one pair of 64-column panels per workgroup
template <typename T>
__global__ __launch_bounds__(kBlock) void k_xty_wide_partial(const T* __restrict__ x, const T* __restrict__ y,
                                                            int64_t n, int px, int py, int64_t ldx, int64_t ldy,
                                                            int sym, T* __restrict__ partial) {
  const int bi = blockIdx.y, bj = blockIdx.z, nbx = gridDim.y, nby = gridDim.z;
  if (sym && bj < bi) return;  // (the whole workgroup: no barrier is left waiting)
  const int cx = px - kGramPanel * bi, cy = py - kGramPanel * bj;
  const int64_t slot = (int64_t)blockIdx.x * wide_pairs(nbx, nby, sym) + wide_pair(bi, bj, nby, sym);
  xty_range<T, kGramMaxTiles, kGramMaxTiles>(x + kGramPanel * bi, y + kGramPanel * bj, n,
                                             cx < kGramPanel ? cx : kGramPanel, cy < kGramPanel ? cy : kGramPanel, ldx,
                                             ldy, blockIdx.x, gridDim.x, partial + slot * (kGramPanel * kGramPanel));
}

// out[i][j] = sum_b partial[b][pair of (i, j)][i % 64][j % 64] in index order, accumulated in double; sym: elements
// below the diagonal from the transposed position
template <typename T>
__global__ __launch_bounds__(kBlock) void k_xty_wide_final(const T* __restrict__ partial, int nranges, int nbx, int nby,
                                                          int sym, int px, int py, T* __restrict__ out) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= px * py) return;
  const int i = k / py, j = k - i * py;
  const int a = (sym && i > j) ? j : i, c = (sym && i > j) ? i : j;
  const int pairs = wide_pairs(nbx, nby, sym);
  const int64_t at = ((int64_t)wide_pair(a / kGramPanel, c / kGramPanel, nby, sym) * kGramPanel + a % kGramPanel) *
                         kGramPanel + c % kGramPanel;
  double s = 0.0;
  for (int b = 0; b < nranges; ++b) s += (double)partial[(int64_t)b * pairs * (kGramPanel * kGramPanel) + at];
  out[k] = T(s);
}

// out[i][j] = sum_b partial[b][i][j] in index order, accumulated in double
template <typename T>
__global__ __launch_bounds__(kBlock) void k_xty_final(const T* __restrict__ partial, int nblocks, int ppx, int ppy,
                                                     int px, int py, T* __restrict__ out) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= px * py) return;
  const int i = k / py, j = k - i * py;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += (double)partial[((int64_t)b * ppx + i) * ppy + j];
  out[k] = T(s);
}

template <typename T, int TX>
static int xty_launch_y(const T* x, const T* y, int64_t n, int px, int py, int64_t ldx, int64_t ldy, T* partial,
                        int ty, hipStream_t stream) {
#define ODIL_XTY_CASE(TY)                                                                                          \
  case TY:                                                                                                         \
    hipLaunchKernelGGL((k_xty_partial<T, TX, TY>), dim3(kGramBlocks), dim3(kBlock), 0, stream, x, y, n, px, py, ldx, \
                       ldy, partial);                                                                              \
    break;
  switch (ty) {
    ODIL_XTY_CASE(1) ODIL_XTY_CASE(2) ODIL_XTY_CASE(3) ODIL_XTY_CASE(4)
    default: return ODIL_E_INVAL;
  }
#undef ODIL_XTY_CASE
  return check_launch("k_xty_partial");
}

template <typename T>
static int dense_block_xty(const T* x, const T* y, int64_t n, int px, int py, int64_t ldx, int64_t ldy, T* out,
                           T* workspace, void* stream) {
  if (!x || !y || !out || !workspace || n < 1 || px < 1 || py < 1 || px > kGramTile * kGramMaxTiles ||
      py > kGramTile * kGramMaxTiles || ldx < px || ldy < py) {
    set_error("dense_block_xty: null pointer, n < 1 or column counts (%d, %d) outside 1..%d", px, py,
              kGramTile * kGramMaxTiles);
    return ODIL_E_INVAL;
  }
  const int tx = (px + kGramTile - 1) / kGramTile, ty = (py + kGramTile - 1) / kGramTile;
  hipStream_t s = (hipStream_t)stream;
  int e;
  switch (tx) {
    case 1: e = xty_launch_y<T, 1>(x, y, n, px, py, ldx, ldy, workspace, ty, s); break;
    case 2: e = xty_launch_y<T, 2>(x, y, n, px, py, ldx, ldy, workspace, ty, s); break;
    case 3: e = xty_launch_y<T, 3>(x, y, n, px, py, ldx, ldy, workspace, ty, s); break;
    default: e = xty_launch_y<T, 4>(x, y, n, px, py, ldx, ldy, workspace, ty, s); break;
  }
  if (e) return e;
  hipLaunchKernelGGL(k_xty_final<T>, dim3((px * py + kBlock - 1) / kBlock), dim3(kBlock), 0, s, workspace, kGramBlocks,
                     kGramTile * tx, kGramTile * ty, px, py, out);
  return check_launch("k_xty_final");
}

// row ranges of the wide entry: as many as keep (ranges x pairs) within kGramWideGroups, no more than the narrow
// entry's and no more than there are steps of one workgroup (4 waves x 4 rows)
static int wide_ranges(int pairs, int64_t n) {
  int64_t r = kGramWideGroups / pairs;
  const int64_t steps = (n + 4 * kGramWaves - 1) / (4 * kGramWaves);
  if (r > kGramBlocks) r = kGramBlocks;
  if (r > steps) r = steps;
  return r < 1 ? 1 : (int)r;
}

static size_t wide_workspace_bytes(int px, int py) {
  if (px < 1 || py < 1 || px > kGramWideMax || py > kGramWideMax) return 0;
  const int pairs = ((px + kGramPanel - 1) / kGramPanel) * ((py + kGramPanel - 1) / kGramPanel);
  return (size_t)wide_ranges(pairs, INT64_MAX / 2) * pairs * kGramPanel * kGramPanel * sizeof(double);
}

template <typename T>
static int dense_block_xty_wide(const T* x, const T* y, int64_t n, int px, int py, int64_t ldx, int64_t ldy, T* out,
                                T* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !y || !out || !workspace || n < 1 || px < 1 || py < 1 || px > kGramWideMax || py > kGramWideMax ||
      ldx < px || ldy < py) {
    set_error("dense_block_xty_wide: null pointer, n < 1 or column counts (%d, %d) outside 1..%d", px, py,
              kGramWideMax);
    return ODIL_E_INVAL;
  }
  if (workspace_bytes < wide_workspace_bytes(px, py)) {
    set_error("dense_block_xty_wide: workspace of %zu bytes, %zu needed for (%d, %d) columns", workspace_bytes,
              wide_workspace_bytes(px, py), px, py);
    return ODIL_E_INVAL;
  }
  const int nbx = (px + kGramPanel - 1) / kGramPanel, nby = (py + kGramPanel - 1) / kGramPanel;
  const int sym = x == y && ldx == ldy && px <= py;
  const int nranges = wide_ranges(nbx * nby, n);  // (from ALL pairs: the same bound with and without `sym`)
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_xty_wide_partial<T>, dim3(nranges, nbx, nby), dim3(kBlock), 0, s, x, y, n, px, py, ldx, ldy, sym,
                     workspace);
  if (int e = check_launch("k_xty_wide_partial")) return e;
  hipLaunchKernelGGL(k_xty_wide_final<T>, dim3((px * py + kBlock - 1) / kBlock), dim3(kBlock), 0, s, workspace, nranges,
                     nbx, nby, sym, px, py, out);
  return check_launch("k_xty_wide_final");
}

}  // namespace odil

using namespace odil;

extern "C" {
size_t odil_dense_block_workspace_bytes(void) {
  return (size_t)kGramBlocks * (kGramTile * kGramMaxTiles) * (kGramTile * kGramMaxTiles) * sizeof(double);
}
int odil_dense_block_xty_f64(const double* x, const double* y, int64_t n, int px, int py, int64_t ldx, int64_t ldy,
                             double* out, double* workspace, void* stream) {
  return dense_block_xty<double>(x, y, n, px, py, ldx, ldy, out, workspace, stream);
}
int odil_dense_block_xty_f32(const float* x, const float* y, int64_t n, int px, int py, int64_t ldx, int64_t ldy,
                             float* out, float* workspace, void* stream) {
  return dense_block_xty<float>(x, y, n, px, py, ldx, ldy, out, workspace, stream);
}
size_t odil_dense_block_wide_workspace_bytes(int px, int py) { return wide_workspace_bytes(px, py); }
int odil_dense_block_xty_wide_f64(const double* x, const double* y, int64_t n, int px, int py, int64_t ldx, int64_t ldy,
                                  double* out, double* workspace, size_t workspace_bytes, void* stream) {
  return dense_block_xty_wide<double>(x, y, n, px, py, ldx, ldy, out, workspace, workspace_bytes, stream);
}
int odil_dense_block_xty_wide_f32(const float* x, const float* y, int64_t n, int px, int py, int64_t ldx, int64_t ldy,
                                  float* out, float* workspace, size_t workspace_bytes, void* stream) {
  return dense_block_xty_wide<float>(x, y, n, px, py, ldx, ldy, out, workspace, workspace_bytes, stream);
}
int odil_dense_block_gram_f64(const double* d, int64_t n, int p, int64_t ld, double* out, double* workspace,
                              void* stream) {
  return dense_block_xty<double>(d, d, n, p, p, ld, ld, out, workspace, stream);
}
int odil_dense_block_gram_f32(const float* d, int64_t n, int p, int64_t ld, float* out, float* workspace,
                              void* stream) {
  return dense_block_xty<float>(d, d, n, p, p, ld, ld, out, workspace, stream);
}
}
