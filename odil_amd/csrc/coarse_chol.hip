// The coarsest level of the normal-equation multigrid (block_mg.hip, gmg.NormalGMG(coarse="device")) factorised on the
// device: its generalised inverse B is formed without a transfer to the host and applied by odil_lincomb.
//
//   scatter   the level's coefficient arrays into a dense symmetric float64 matrix (odil_bmg_coarse_dense): one thread
//             per row adds the entries of its field in table order, as gmg.NormalGMG.dense does on the host, then
//             0.5 (A + A^T) as the host route; every element receives at most one coefficient: deterministic
//   factor    right-looking blocked Cholesky A = U^T U on the augmented matrix [A | I] (odil_bmg_coarse_chol): per panel
//             of kCcPanel rows, one launch factors the kCcPanel x kCcPanel diagonal block in LDS (every workgroup
//             the same block, redundantly: no workgroup waits on another) and applies U11^-T to the panel's columns
//             of A and of the identity; a second launch subtracts U12^T X from the trailing rows with the f64 MFMA.
//             The right half ends as Y = U^-T.
//   inverse   B = Y^T Y, one MFMA product over the lower-triangular Y, upper tiles only, mirrored: B is exactly
//             symmetric.
//
// Pivots: a Schur-complement pivot <= tol_rel * max_i A_ii drops its row -- U's row and Y's row are zero, the pivot's
// entry of B is zero.  For a positive-semidefinite A (a field fixed only up to a constant) B = E_S A_SS^-1 E_S^T over
// the kept pivots S: symmetric positive semidefinite, and A B b = b for every b in the range of A (gmg.py).
//
// Layout: n unknowns padded to np = a multiple of kCcPanel (padding rows are zero: their pivots are dropped); the
// work matrix is np x 2 np, row-major (row stride 2 np), the factorisation works on its upper triangle.  No atomics:
// two factorisations are bit-identical.
#include "block_mg.h"

namespace odil {

constexpr int kCcPanel = 64;              // rows per panel = the 64 x 64 block of one wave in the MFMA kernels
constexpr int kCcWaves = kBlock / 64;
constexpr int kCcMaxUnknowns = 8192;

typedef double CcAcc __attribute__((ext_vector_type(4)));

__device__ inline CcAcc cc_mfma(double a, double b, CcAcc c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// [0, np) x [0, np) of out (row stride lda): zero, or the identity (ident = 1)
__global__ __launch_bounds__(kBlock) void k_cc_init(double* __restrict__ out, int64_t np, int64_t lda, int ident) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= np * np) return;
  const int64_t r = k / np, c = k - r * np;
  out[r * lda + c] = (ident && c == r) ? 1.0 : 0.0;
}

// row i of the level's matrix: the entries of i's field in table order (gmg.NormalGMG.dense)
__global__ __launch_bounds__(kBlock) void k_cc_scatter(const double* __restrict__ coef,
                                                      const int64_t* __restrict__ table, BmgLevel L, int64_t lda,
                                                      double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= L.off[L.nf]) return;
  const int a = field_of(L, i);
  const int64_t q = i - L.off[a];
  const int64_t na1 = L.n[a][1], na2 = L.n[a][2];
  const int64_t q2 = q % na2, q1 = (q / na2) % na1, q0 = q / (na1 * na2);
  double* row = out + i * lda;
  for (int e = L.ebeg[a]; e < L.ebeg[a + 1]; ++e) {
    const int64_t* t = table + (int64_t)e * kEnt;
    const int bf = (int)t[1];
    const int64_t t0 = q0 + t[2], t1 = q1 + t[3], t2 = q2 + t[4];
    if (t0 < 0 || t0 >= L.n[bf][0] || t1 < 0 || t1 >= L.n[bf][1] || t2 < 0 || t2 >= L.n[bf][2]) continue;
    const int64_t col = L.off[bf] + (t0 * L.n[bf][1] + t1) * L.n[bf][2] + t2;
    row[col] = row[col] + coef[t[5] + q];
  }
}

// (r, c), r < c < n: both entries become 0.5 (A_rc + A_cr); one thread owns the pair
__global__ __launch_bounds__(kBlock) void k_cc_symmetrize(double* __restrict__ m, int64_t n, int64_t lda) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n * n) return;
  const int64_t r = k / n, c = k - r * n;
  if (r >= c) return;
  const double s = 0.5 * (m[r * lda + c] + m[c * lda + r]);
  m[r * lda + c] = s;
  m[c * lda + r] = s;
}

// thr[0] = tol_rel * max_i A_ii (one workgroup; max is exact in any order)
__global__ __launch_bounds__(kBlock) void k_cc_threshold(const double* __restrict__ m, int64_t n, int64_t lda,
                                                        double tol_rel, double* __restrict__ thr) {
  __shared__ double part[kBlock];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) v = fmax(v, m[i * lda + i]);
  part[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double mx = 0.0;
    for (int t = 0; t < kBlock; ++t) mx = fmax(mx, part[t]);
    thr[0] = tol_rel * mx;
  }
}

// Panel k0: factor the diagonal block (upper triangle of rows / columns [k0, k0 + kCcPanel)) in LDS, then
// x = U11^-T x for every column c in [k0 + kCcPanel, np + k0 + kCcPanel) of the panel's rows, one thread per column.
// drops[k0 / kCcPanel]: the number of dropped pivots of rows below n (workgroup 0).
__global__ __launch_bounds__(kBlock) void k_cc_panel(double* __restrict__ m, int64_t lda, int64_t np, int64_t n,
                                                    int64_t k0, const double* __restrict__ thr,
                                                    int* __restrict__ drops) {
  constexpr int P = kCcPanel;
  __shared__ double s[P][P + 1];
  __shared__ double rd[P];
  const int tid = threadIdx.x;
  for (int k = tid; k < P * P; k += kBlock) {
    const int r = k / P, c = k - r * P;
    s[r][c] = c >= r ? m[(k0 + r) * lda + k0 + c] : 0.0;
  }
  const double th = thr[0];
  __syncthreads();
  for (int j = 0; j < P; ++j) {
    const double p = s[j][j];
    const bool keep = p > th;  // (a NaN pivot is dropped as well)
    const double d = keep ? sqrt(p) : 0.0, inv = keep ? 1.0 / d : 0.0;
    __syncthreads();  // every thread has read the pivot before row j changes
    for (int c = j + tid; c < P; c += kBlock) s[j][c] = c == j ? d : keep ? s[j][c] * inv : 0.0;
    if (tid == 0) rd[j] = inv;
    __syncthreads();
    for (int k = tid; k < P * P; k += kBlock) {
      const int r = k / P, c = k - r * P;
      if (r > j && c >= r) s[r][c] = s[r][c] - s[j][r] * s[j][c];
    }
    __syncthreads();
  }
  if (blockIdx.x == 0 && tid == 0) {
    int cnt = 0;
    for (int j = 0; j < P; ++j) cnt += (rd[j] == 0.0 && k0 + j < n) ? 1 : 0;
    drops[k0 / P] = cnt;
  }
  const int64_t c = k0 + P + (int64_t)blockIdx.x * kBlock + tid;
  if (c >= np + k0 + P) return;
  double x[P];
#pragma unroll
  for (int j = 0; j < P; ++j) x[j] = m[(k0 + j) * lda + c];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    x[j] = x[j] * rd[j];
#pragma unroll
    for (int i = j + 1; i < P; ++i) x[i] = x[i] - s[j][i] * x[j];
  }
#pragma unroll
  for (int j = 0; j < P; ++j) m[(k0 + j) * lda + c] = x[j];
}

// Trailing update after panel k0: rows r in [k1, np), k1 = k0 + kCcPanel, columns c in [r's block, np + k1):
// m[r][c] -= sum_{k in panel} m[k][r] m[k][c].  One wave per 64 x 64 block (4 x 4 MFMA tiles); blocks left of the
// diagonal are skipped.  The accumulator starts from the block itself, the U12^T operand enters negated.
__global__ __launch_bounds__(kBlock) void k_cc_update(double* __restrict__ m, int64_t lda, int64_t np, int64_t k0) {
  constexpr int P = kCcPanel;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k1 = k0 + P;
  const int64_t rb = k1 / P + blockIdx.y, cb = (int64_t)blockIdx.x * kCcWaves + wave;
  if (cb < rb || cb >= (np + k1) / P) return;
  const int64_t r0 = rb * P, c0 = cb * P;
  const int col = lane & 15, kr = lane >> 4;
  CcAcc acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ti][tj][e] = m[(r0 + 16 * ti + kr + 4 * e) * lda + c0 + 16 * tj + col];
  for (int s = 0; s < P / 4; ++s) {
    const double* row = m + (k0 + 4 * s + kr) * lda;
    double a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t] = -row[r0 + 16 * t + col];
      b[t] = row[c0 + 16 * t + col];
    }
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = cc_mfma(a[ti], b[tj], acc[ti][tj]);
  }
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int e = 0; e < 4; ++e) m[(r0 + 16 * ti + kr + 4 * e) * lda + c0 + 16 * tj + col] = acc[ti][tj][e];
}

// B = Y^T Y (Y = columns [np, 2 np) of m, lower triangular): block (ib, jb), ib <= jb, sums k from 64 jb on, writes
// B[i][j] and B[j][i] for i, j < n (on the diagonal blocks only the lane holding i < j writes, i = j once)
__global__ __launch_bounds__(kBlock) void k_cc_gram(const double* __restrict__ m, int64_t lda, int64_t np, int64_t n,
                                                   double* __restrict__ out) {
  constexpr int P = kCcPanel;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ib = blockIdx.y, jb = (int64_t)blockIdx.x * kCcWaves + wave;
  if (jb < ib || jb >= np / P) return;
  const int64_t i0 = ib * P, j0 = jb * P;
  const int col = lane & 15, kr = lane >> 4;
  CcAcc acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = CcAcc{0.0, 0.0, 0.0, 0.0};
  for (int64_t k = j0; k < np; k += 4) {
    const double* row = m + (k + kr) * lda + np;
    double a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t] = row[i0 + 16 * t + col];
      b[t] = row[j0 + 16 * t + col];
    }
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = cc_mfma(a[ti], b[tj], acc[ti][tj]);
  }
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t i = i0 + 16 * ti + kr + 4 * e, j = j0 + 16 * tj + col;
        if (i >= n || j >= n || (ib == jb && i > j)) continue;
        out[i * n + j] = acc[ti][tj][e];
        if (i != j) out[j * n + i] = acc[ti][tj][e];
      }
}

static inline unsigned cc_grid(int64_t count) { return (unsigned)((count + kBlock - 1) / kBlock); }

static int coarse_dense(const double* coef, const int64_t* table, const int64_t* desc, int64_t np, int64_t lda,
                        double* out, void* stream) {
  BmgLevel L;
  if (int e = parse_level(desc, L, "bmg_coarse_dense")) return e;
  const int64_t n = L.off[L.nf];
  if (!coef || !table || !out || n > kCcMaxUnknowns || np < n || lda < np) {
    set_error("bmg_coarse_dense: null pointer, %lld unknowns (at most %d) or padded size %lld / row stride %lld too small",
              (long long)n, kCcMaxUnknowns, (long long)np, (long long)lda);
    return ODIL_E_INVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_cc_init, dim3(cc_grid(np * np)), dim3(kBlock), 0, s, out, np, lda, 0);
  if (int e = check_launch("k_cc_init")) return e;
  hipLaunchKernelGGL(k_cc_scatter, dim3(cc_grid(n)), dim3(kBlock), 0, s, coef, table, L, lda, out);
  if (int e = check_launch("k_cc_scatter")) return e;
  hipLaunchKernelGGL(k_cc_symmetrize, dim3(cc_grid(n * n)), dim3(kBlock), 0, s, out, n, lda);
  return check_launch("k_cc_symmetrize");
}

static int coarse_chol(double* work, int64_t n, int64_t np, double tol_rel, double* thr, int* drops, double* inv,
                       void* stream) {
  if (!work || !thr || !drops || !inv || n < 1 || n > kCcMaxUnknowns || np < n || np % kCcPanel != 0 ||
      np - n >= kCcPanel || !(tol_rel >= 0.0)) {
    set_error("bmg_coarse_chol: null pointer, %lld unknowns (1 to %d), padded size %lld (the next multiple of %d) or "
              "tol_rel %g", (long long)n, kCcMaxUnknowns, (long long)np, kCcPanel, tol_rel);
    return ODIL_E_INVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t lda = 2 * np, nb = np / kCcPanel;
  // the identity half (the matrix half is odil_bmg_coarse_dense's, row stride 2 np)
  hipLaunchKernelGGL(k_cc_init, dim3(cc_grid(np * np)), dim3(kBlock), 0, s, work + np, np, lda, 1);
  if (int e = check_launch("k_cc_init")) return e;
  hipLaunchKernelGGL(k_cc_threshold, dim3(1), dim3(kBlock), 0, s, work, n, lda, tol_rel, thr);
  if (int e = check_launch("k_cc_threshold")) return e;
  for (int64_t p = 0; p < nb; ++p) {
    const int64_t k0 = p * kCcPanel;
    hipLaunchKernelGGL(k_cc_panel, dim3(cc_grid(np)), dim3(kBlock), 0, s, work, lda, np, n, k0, thr, drops);
    if (int e = check_launch("k_cc_panel")) return e;
    if (p + 1 == nb) break;
    const int64_t rows = nb - p - 1, cols = nb + p + 1;
    hipLaunchKernelGGL(k_cc_update, dim3((unsigned)((cols + kCcWaves - 1) / kCcWaves), (unsigned)rows), dim3(kBlock),
                       0, s, work, lda, np, k0);
    if (int e = check_launch("k_cc_update")) return e;
  }
  hipLaunchKernelGGL(k_cc_gram, dim3((unsigned)((nb + kCcWaves - 1) / kCcWaves), (unsigned)nb), dim3(kBlock), 0, s,
                     work, lda, np, n, inv);
  return check_launch("k_cc_gram");
}

}  // namespace odil

using namespace odil;

extern "C" {
int odil_bmg_coarse_dense_f64(const double* coef, const int64_t* table, const int64_t* desc, int64_t np, int64_t lda,
                              double* out, void* stream) {
  return coarse_dense(coef, table, desc, np, lda, out, stream);
}
int odil_bmg_coarse_chol_f64(double* work, int64_t n, int64_t np, double tol_rel, double* thr, int* drops,
                             double* inv, void* stream) {
  return coarse_chol(work, n, np, tol_rel, thr, drops, inv, stream);
}
}
