// GCR(m) around the batched multigrid cycle of an ensemble whose members are too large for one workgroup
// (gmg.EnsembleLaunchKrylovGMG): the vector passes of a GCR step and the decision of every member, all on the device.
//
// Per member b the store S_b = [2 m, cells] holds the directions Z (rows 0 .. m - 1) and their images Q (rows m .. 2 m - 1).
// The pass with the number k works in the rows k mod m: the cycle wrote e there (row slot) and the residual launch
// t = 0 - A e (row m + slot).  A member that keeps have_b directions finds the j-th oldest in the rows
// (slot - have_b + j) mod m -- consecutive passes fill consecutive rows, and have_b never exceeds m.
//   k_gcr_dots      beta_j = <Q_j, q>, q = -t, for j < have_b: one read of q                (partial sums, quantity j)
//   k_gcr_project   q' = q - sum_j beta_j Q_j, z' = e - sum_j beta_j Z_j in place;  <q', q'>, <q', rho>
//                                                                                   (partial sums, quantities m, m + 1)
//   k_gcr_update    q = q' / |q'|, z = z' / |q'| in place, x += a z, rho -= a q;  <rho, rho>      (partial sums, quantity 0)
//   k_gcr_sumsq     <v, v> of a vector (the true residual of a member to verify)                (partial sums, quantity 0)
//   k_gcr_decide    one workgroup per member: the partial sums added in a fixed order, the scalars of the passes, the stop
//                   rules and the masks; k_gcr_count then counts the members of every kind
// A workgroup covers kGcrCells consecutive cells of ONE member (the member on blockIdx.y), whatever nbatch is: workgroup p
// leaves its sums, accumulated in double, in gpart[b, quantity, p].  No workgroup waits for, signals or reads what another
// one of the same launch writes; mask[b] == 0: return before any load or store.
#include "common.h"

namespace odil {

constexpr int kGcrPer = 4;                      // cells per thread
constexpr int kGcrCells = kGcrPer * kBlock;     // cells per workgroup
constexpr int kGcrMaxM = 8;                     // directions kept at most

static int64_t gcr_parts(int64_t cells) {
  if (cells < 1 || cells > (int64_t)1 << 24) return 0;
  return (cells + kGcrCells - 1) / kGcrCells;
}

__device__ inline int gcr_row(int slot, int have, int j, int m) { return (slot - have + j + m) % m; }

template <typename T>
__global__ __launch_bounds__(kBlock) void k_gcr_dots(const T* __restrict__ store, int64_t sstride, int64_t cells, int m,
                                                     int slot, const int* __restrict__ have, int max_have,
                                                     const int* __restrict__ mask, double* __restrict__ gpart,
                                                     int64_t gstride) {
  const int64_t b = blockIdx.y;
  if (mask[b] == 0) return;
  int h = have[b] < max_have ? have[b] : max_have;
  if (h > m - 1) h = m - 1;  // (the row of this pass is never one of the kept ones)
  if (h <= 0) return;
  const T* s = store + b * sstride;
  const int64_t first = (int64_t)blockIdx.x * kGcrCells + threadIdx.x;
  T q[kGcrPer];
#pragma unroll
  for (int u = 0; u < kGcrPer; ++u) {
    const int64_t i = first + (int64_t)u * kBlock;
    q[u] = i < cells ? -s[(int64_t)(m + slot) * cells + i] : T(0);
  }
  for (int j = 0; j < h; ++j) {  // (uniform: every thread of the workgroup arrives at the sums)
    const T* qj = s + (int64_t)(m + gcr_row(slot, h, j, m)) * cells;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kGcrPer; ++u) {
      const int64_t i = first + (int64_t)u * kBlock;
      if (i < cells) acc += (double)qj[i] * (double)q[u];
    }
    const double total = block_sum(acc);
    if (threadIdx.x == 0) gpart[b * gstride + (int64_t)j * gridDim.x + blockIdx.x] = total;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_gcr_project(T* __restrict__ store, int64_t sstride, const T* __restrict__ rho,
                                                        int64_t rstride, int64_t cells, int m, int slot,
                                                        const int* __restrict__ have, int max_have,
                                                        const double* __restrict__ scal, int64_t scstride,
                                                        const int* __restrict__ mask, double* __restrict__ gpart,
                                                        int64_t gstride) {
  const int64_t b = blockIdx.y;
  if (mask[b] == 0) return;
  int h = have[b] < max_have ? have[b] : max_have;
  if (h > m - 1) h = m - 1;
  if (h < 0) h = 0;
  T* s = store + b * sstride;
  const T* r = rho + b * rstride;
  T* qrow = s + (int64_t)(m + slot) * cells;
  T* zrow = s + (int64_t)slot * cells;
  const int64_t first = (int64_t)blockIdx.x * kGcrCells + threadIdx.x;
  T q[kGcrPer], z[kGcrPer];
#pragma unroll
  for (int u = 0; u < kGcrPer; ++u) {
    const int64_t i = first + (int64_t)u * kBlock;
    q[u] = i < cells ? -qrow[i] : T(0);
    z[u] = i < cells ? zrow[i] : T(0);
  }
  for (int j = 0; j < h; ++j) {
    const int row = gcr_row(slot, h, j, m);
    const T beta = (T)scal[b * scstride + j];
    const T* qj = s + (int64_t)(m + row) * cells;
    const T* zj = s + (int64_t)row * cells;
#pragma unroll
    for (int u = 0; u < kGcrPer; ++u) {
      const int64_t i = first + (int64_t)u * kBlock;
      if (i < cells) {
        q[u] = q[u] - beta * qj[i];
        z[u] = z[u] - beta * zj[i];
      }
    }
  }
  double qq = 0.0, qr = 0.0;
#pragma unroll
  for (int u = 0; u < kGcrPer; ++u) {
    const int64_t i = first + (int64_t)u * kBlock;
    if (i < cells) {
      qrow[i] = q[u];
      zrow[i] = z[u];
      qq += (double)q[u] * (double)q[u];
      qr += (double)q[u] * (double)r[i];
    }
  }
  const double tqq = block_sum(qq);
  const double tqr = block_sum(qr);
  if (threadIdx.x == 0) {
    gpart[b * gstride + (int64_t)m * gridDim.x + blockIdx.x] = tqq;
    gpart[b * gstride + (int64_t)(m + 1) * gridDim.x + blockIdx.x] = tqr;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_gcr_update(T* __restrict__ store, int64_t sstride, T* __restrict__ x,
                                                       int64_t xstride, T* __restrict__ rho, int64_t rstride, int64_t cells,
                                                       int m, int slot, const double* __restrict__ scal, int64_t scstride,
                                                       const int* __restrict__ mask, double* __restrict__ gpart,
                                                       int64_t gstride) {
  const int64_t b = blockIdx.y;
  if (mask[b] == 0) return;
  T* qrow = store + b * sstride + (int64_t)(m + slot) * cells;
  T* zrow = store + b * sstride + (int64_t)slot * cells;
  T* xm = x + b * xstride;
  T* r = rho + b * rstride;
  const T inv = (T)scal[b * scstride + m], alpha = (T)scal[b * scstride + m + 1];
  const int64_t first = (int64_t)blockIdx.x * kGcrCells + threadIdx.x;
  double rr = 0.0;
#pragma unroll
  for (int u = 0; u < kGcrPer; ++u) {
    const int64_t i = first + (int64_t)u * kBlock;
    if (i < cells) {
      const T q = qrow[i] * inv, z = zrow[i] * inv;
      qrow[i] = q;
      zrow[i] = z;
      xm[i] = xm[i] + alpha * z;
      const T rn = r[i] - alpha * q;
      r[i] = rn;
      rr += (double)rn * (double)rn;
    }
  }
  const double total = block_sum(rr);
  if (threadIdx.x == 0) gpart[b * gstride + blockIdx.x] = total;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_gcr_sumsq(const T* __restrict__ v, int64_t vstride, int64_t cells,
                                                      const int* __restrict__ mask, double* __restrict__ gpart,
                                                      int64_t gstride) {
  const int64_t b = blockIdx.y;
  if (mask[b] == 0) return;
  const T* vm = v + b * vstride;
  const int64_t first = (int64_t)blockIdx.x * kGcrCells + threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < kGcrPer; ++u) {
    const int64_t i = first + (int64_t)u * kBlock;
    if (i < cells) acc += (double)vm[i] * (double)vm[i];
  }
  const double total = block_sum(acc);
  if (threadIdx.x == 0) gpart[b * gstride + blockIdx.x] = total;
}

// the sum of n partial sums in the order of k_cycle_decide_batch (stencil_mg.hip): thread t adds t, t + kBlock, ..., then
// block_sum; valid on thread 0.  Every thread of the workgroup arrives.
__device__ inline double gcr_ordered_sum(const double* __restrict__ p, int n) {
  double sum = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) sum += p[i];
  return block_sum(sum);
}

struct GcrState {
  int* active;  // stationary members (the mask of the base cycle)
  int* gcr;     // members that run the GCR pass
  int* fresh;   // members whose rho = b - A x is to be formed before the pass
  int* verify;  // members whose true residual decides
  int* have;    // directions kept
};

// mode 0, BEFORE pass k.  A stationary member: k_cycle_decide_batch with the hand-over (the order of
//   odil_stencil_solve_krylov_batch).  A GCR member: history[1 + k] from the update's partial sums, then 3 non-finite,
//   recurrence <= tolerance -> verify (+ fresh, have = 0, out of the GCR mask until mode 3 has looked), 1 k == maxcycles,
//   have == m -> have = 0.
// mode 1, the betas of a GCR member from the products of k_gcr_dots; its fresh flag is cleared (rho has been formed).
// mode 2, 1 / |q'| and a = <q', rho> / |q'| from k_gcr_project; |q'|^2 zero or non-finite: 4 breakdown, (k, 4), the member
//   leaves the GCR mask before the update touches its iterate; else have += 1.
// mode 3, a member to verify: history[1 + k] = the true residual's mean square (k_gcr_sumsq); 0 converged, 1 k == maxcycles,
//   else back into the GCR mask with no directions.
__global__ __launch_bounds__(kBlock) void k_gcr_decide(int mode, const double* __restrict__ partials, int64_t pstride,
                                                      const double* __restrict__ partials0, int64_t p0stride, int nparts,
                                                      const double* __restrict__ gpart, int64_t gstride, int gparts,
                                                      double cells, int k, int maxcycles, double tol2, int m,
                                                      double* __restrict__ history, int64_t hstride,
                                                      int* __restrict__ outcome, GcrState st, double* __restrict__ scal,
                                                      int64_t scstride) {
  const int64_t b = blockIdx.x;
  double* h = history + b * hstride;
  int* out = outcome + 3 * b;
  if (mode == 0 && st.active[b] != 0) {
    const double rsq = gcr_ordered_sum(partials + b * pstride, nparts) / cells;
    double bsq = 0.0;
    if (partials0 != nullptr) bsq = gcr_ordered_sum(partials0 + b * p0stride, nparts) / cells;
    if (threadIdx.x != 0) return;
    if (partials0 != nullptr)
      h[0] = bsq;
    else
      bsq = h[0];
    const double prev = h[k];
    h[1 + k] = rsq;
    int why = -1;
    if (!__builtin_isfinite(rsq) || !__builtin_isfinite(bsq)) why = 3;
    else if (rsq <= tol2 * bsq) why = 0;
    else if (k == maxcycles) why = 1;
    else if (k >= 2 && rsq >= 0.25 * prev && rsq > 1e6 * tol2 * bsq) {
      st.active[b] = 0;
      st.gcr[b] = 1;
      st.fresh[b] = 1;
      st.have[b] = 0;
      out[2] = k;
    } else if (k >= 3 && rsq >= (0.98 * 0.98) * prev) why = 2;
    if (why >= 0) {
      out[0] = k;
      out[1] = why;
      st.active[b] = 0;
    }
    return;
  }
  if (mode == 0 && st.gcr[b] != 0) {
    const double rsq = gcr_ordered_sum(gpart + b * gstride, gparts) / cells;
    if (threadIdx.x != 0) return;
    const double bsq = h[0];
    h[1 + k] = rsq;
    int why = -1;
    if (!__builtin_isfinite(rsq)) why = 3;
    else if (rsq <= tol2 * bsq) {  // (the recurrence says converged: the true residual decides, mode 3)
      st.gcr[b] = 0;
      st.verify[b] = 1;
      st.fresh[b] = 1;
      st.have[b] = 0;
    } else if (k == maxcycles) why = 1;
    else if (st.have[b] >= m) st.have[b] = 0;
    if (why >= 0) {
      out[0] = k;
      out[1] = why;
      st.gcr[b] = 0;
    }
    return;
  }
  if (mode == 1 && st.gcr[b] != 0) {
    const int have = st.have[b] < m - 1 ? st.have[b] : m - 1;
    for (int j = 0; j < have; ++j) {  // (uniform)
      const double beta = gcr_ordered_sum(gpart + b * gstride + (int64_t)j * gparts, gparts);
      if (threadIdx.x == 0) scal[b * scstride + j] = beta;
    }
    if (threadIdx.x == 0) st.fresh[b] = 0;
    return;
  }
  if (mode == 2 && st.gcr[b] != 0) {
    const double qq = gcr_ordered_sum(gpart + b * gstride + (int64_t)m * gparts, gparts);
    const double qr = gcr_ordered_sum(gpart + b * gstride + (int64_t)(m + 1) * gparts, gparts);
    if (threadIdx.x != 0) return;
    if (!(qq > 0.0) || !__builtin_isfinite(qq)) {
      out[0] = k;
      out[1] = 4;
      st.gcr[b] = 0;
      return;
    }
    const double inv = 1.0 / sqrt(qq);
    scal[b * scstride + m] = inv;
    scal[b * scstride + m + 1] = qr * inv;
    st.have[b] = st.have[b] + 1;
    return;
  }
  if (mode == 3 && st.verify[b] != 0) {
    const double rsq = gcr_ordered_sum(gpart + b * gstride, gparts) / cells;
    if (threadIdx.x != 0) return;
    const double bsq = h[0];
    h[1 + k] = rsq;
    st.verify[b] = 0;
    st.fresh[b] = 0;
    int why = -1;
    if (!__builtin_isfinite(rsq)) why = 3;
    else if (rsq <= tol2 * bsq) why = 0;
    else if (k == maxcycles) why = 1;
    if (why >= 0) {
      out[0] = k;
      out[1] = why;
    } else {
      st.gcr[b] = 1;
      st.have[b] = 0;
    }
  }
}

// counts[0 .. 3] = the stationary members, the GCR members, the members to verify, the members whose rho is to be formed:
// ONE workgroup in a launch of its own (the decision has finished); integers, exact in any order
__global__ __launch_bounds__(kBlock) void k_gcr_count(GcrState st, int nbatch, int* __restrict__ counts) {
  const int* which[4] = {st.active, st.gcr, st.verify, st.fresh};
  for (int c = 0; c < 4; ++c) {
    double n = 0.0;
    for (int b = threadIdx.x; b < nbatch; b += kBlock) n += which[c][b] != 0 ? 1.0 : 0.0;
    const double total = block_sum(n);
    if (threadIdx.x == 0) counts[c] = (int)total;
  }
}

// ---- argument checks shared by the vector passes -------------------------------------------------------------------
static int gcr_check(const char* what, int nbatch, int64_t cells, int krylov_m, int slot, int max_have, const void* mask,
                     const void* gpart, int64_t gpart_stride, bool has_store, const void* store, int64_t store_stride) {
  if (nbatch < 1 || nbatch > 65535) {
    set_error("%s: nbatch %d (1..65535: the member is a grid dimension)", what, nbatch);
    return ODIL_E_INVAL;
  }
  if (krylov_m < 1 || krylov_m > kGcrMaxM) {
    set_error("%s: krylov_m %d (1..%d directions)", what, krylov_m, kGcrMaxM);
    return ODIL_E_INVAL;
  }
  const int64_t parts = gcr_parts(cells);
  if (!parts) {
    set_error("%s: cells %lld per member (1..2^24)", what, (long long)cells);
    return ODIL_E_INVAL;
  }
  if (slot < 0 || slot >= krylov_m) {
    set_error("%s: slot %d is not one of the krylov_m = %d rows", what, slot, krylov_m);
    return ODIL_E_INVAL;
  }
  if (max_have < 0 || max_have > krylov_m) {
    set_error("%s: have up to max_have %d is beyond krylov_m = %d", what, max_have, krylov_m);
    return ODIL_E_INVAL;
  }
  if (!mask) {
    set_error("%s: mask is null (int[nbatch] on the device)", what);
    return ODIL_E_INVAL;
  }
  if (!gpart) {
    set_error("%s: gpart is null", what);
    return ODIL_E_INVAL;
  }
  if (gpart_stride < (int64_t)(krylov_m + 2) * parts) {
    set_error("%s: gpart_stride %lld is smaller than a member ((krylov_m + 2) x %lld partial sums)", what,
              (long long)gpart_stride, (long long)parts);
    return ODIL_E_INVAL;
  }
  if (has_store) {
    if (!store) {
      set_error("%s: store is null", what);
      return ODIL_E_INVAL;
    }
    if (store_stride < 2 * (int64_t)krylov_m * cells) {
      set_error("%s: store_stride %lld is smaller than a member (2 krylov_m x %lld cells)", what, (long long)store_stride,
                (long long)cells);
      return ODIL_E_INVAL;
    }
  }
  return 0;
}

static int gcr_vector(const char* what, const char* name, const void* v, int64_t stride, int64_t cells) {
  if (!v) {
    set_error("%s: %s is null", what, name);
    return ODIL_E_INVAL;
  }
  if (stride < cells) {
    set_error("%s: %s_stride %lld is smaller than a member (%lld)", what, name, (long long)stride, (long long)cells);
    return ODIL_E_INVAL;
  }
  return 0;
}

static int gcr_scalars(const char* what, const void* scal, int64_t stride, int krylov_m) {
  if (!scal) {
    set_error("%s: scal is null", what);
    return ODIL_E_INVAL;
  }
  if (stride < krylov_m + 2) {
    set_error("%s: scal_stride %lld is smaller than a member (krylov_m + 2 = %d scalars)", what, (long long)stride,
              krylov_m + 2);
    return ODIL_E_INVAL;
  }
  return 0;
}

template <typename T>
static int gcr_dots(const T* store, int64_t store_stride, int64_t cells, int krylov_m, int slot, const int* have, int max_have,
                    const int* mask, int nbatch, double* gpart, int64_t gpart_stride, void* stream) {
  const char* what = "stencil_gcr_dots_batch";
  if (int e = gcr_check(what, nbatch, cells, krylov_m, slot, max_have, mask, gpart, gpart_stride, true, store, store_stride))
    return e;
  if (!have) {
    set_error("%s: have is null (int[nbatch] on the device)", what);
    return ODIL_E_INVAL;
  }
  if (max_have == 0) return 0;  // (no member keeps a direction: nothing to do)
  const dim3 grid((unsigned)gcr_parts(cells), (unsigned)nbatch);
  hipLaunchKernelGGL((k_gcr_dots<T>), grid, dim3(kBlock), 0, (hipStream_t)stream, store, store_stride, cells, krylov_m, slot,
                     have, max_have, mask, gpart, gpart_stride);
  return check_launch("k_gcr_dots");
}

template <typename T>
static int gcr_project(T* store, int64_t store_stride, const T* rho, int64_t rho_stride, int64_t cells, int krylov_m, int slot,
                       const int* have, int max_have, const double* scal, int64_t scal_stride, const int* mask, int nbatch,
                       double* gpart, int64_t gpart_stride, void* stream) {
  const char* what = "stencil_gcr_project_batch";
  if (int e = gcr_check(what, nbatch, cells, krylov_m, slot, max_have, mask, gpart, gpart_stride, true, store, store_stride))
    return e;
  if (!have) {
    set_error("%s: have is null (int[nbatch] on the device)", what);
    return ODIL_E_INVAL;
  }
  if (int e = gcr_vector(what, "rho", rho, rho_stride, cells)) return e;
  if (int e = gcr_scalars(what, scal, scal_stride, krylov_m)) return e;
  const dim3 grid((unsigned)gcr_parts(cells), (unsigned)nbatch);
  hipLaunchKernelGGL((k_gcr_project<T>), grid, dim3(kBlock), 0, (hipStream_t)stream, store, store_stride, rho, rho_stride,
                     cells, krylov_m, slot, have, max_have, scal, scal_stride, mask, gpart, gpart_stride);
  return check_launch("k_gcr_project");
}

template <typename T>
static int gcr_update(T* store, int64_t store_stride, T* x, int64_t x_stride, T* rho, int64_t rho_stride, int64_t cells,
                      int krylov_m, int slot, const double* scal, int64_t scal_stride, const int* mask, int nbatch,
                      double* gpart, int64_t gpart_stride, void* stream) {
  const char* what = "stencil_gcr_update_batch";
  if (int e = gcr_check(what, nbatch, cells, krylov_m, slot, 0, mask, gpart, gpart_stride, true, store, store_stride)) return e;
  if (int e = gcr_vector(what, "x", x, x_stride, cells)) return e;
  if (int e = gcr_vector(what, "rho", rho, rho_stride, cells)) return e;
  if (int e = gcr_scalars(what, scal, scal_stride, krylov_m)) return e;
  if ((const void*)x == (const void*)rho) {
    set_error("%s: x and rho are one array", what);
    return ODIL_E_INVAL;
  }
  const dim3 grid((unsigned)gcr_parts(cells), (unsigned)nbatch);
  hipLaunchKernelGGL((k_gcr_update<T>), grid, dim3(kBlock), 0, (hipStream_t)stream, store, store_stride, x, x_stride, rho,
                     rho_stride, cells, krylov_m, slot, scal, scal_stride, mask, gpart, gpart_stride);
  return check_launch("k_gcr_update");
}

template <typename T>
static int gcr_sumsq(const T* v, int64_t v_stride, int64_t cells, const int* mask, int nbatch, double* gpart,
                     int64_t gpart_stride, void* stream) {
  const char* what = "stencil_gcr_sumsq_batch";
  if (int e = gcr_check(what, nbatch, cells, 1, 0, 0, mask, gpart, gpart_stride, false, nullptr, 0)) return e;
  if (int e = gcr_vector(what, "v", v, v_stride, cells)) return e;
  const dim3 grid((unsigned)gcr_parts(cells), (unsigned)nbatch);
  hipLaunchKernelGGL((k_gcr_sumsq<T>), grid, dim3(kBlock), 0, (hipStream_t)stream, v, v_stride, cells, mask, gpart,
                     gpart_stride);
  return check_launch("k_gcr_sumsq");
}

static int gcr_decide(int mode, const double* partials, int64_t partials_stride, const double* partials0,
                      int64_t partials0_stride, int nparts, const double* gpart, int64_t gpart_stride, int gparts, int nbatch,
                      int64_t cells, int k, int maxcycles, double tol, int krylov_m, double* history, int64_t history_stride,
                      int* outcome, int* active, int* gcr, int* fresh, int* verify, int* have, double* scal,
                      int64_t scal_stride, int* counts, void* stream) {
  const char* what = "stencil_gcr_decide_batch";
  if (mode < 0 || mode > 3) {
    set_error("%s: mode %d (0: before a pass, 1: betas, 2: scaling and step, 3: verification)", what, mode);
    return ODIL_E_INVAL;
  }
  if (nbatch < 1 || nbatch > 65535) {
    set_error("%s: nbatch %d (1..65535: the member is a grid dimension)", what, nbatch);
    return ODIL_E_INVAL;
  }
  if (krylov_m < 1 || krylov_m > kGcrMaxM) {
    set_error("%s: krylov_m %d (1..%d directions)", what, krylov_m, kGcrMaxM);
    return ODIL_E_INVAL;
  }
  if (!active || !gcr || !fresh || !verify || !have) {
    set_error("%s: a mask is null (active, gcr, fresh, verify, have: int[nbatch] on the device)", what);
    return ODIL_E_INVAL;
  }
  if (!history || !outcome || !gpart || !scal || (mode == 0 && (!partials || !counts)) || (mode == 3 && !counts)) {
    set_error("%s: null pointer (history, outcome, gpart, scal; partials and counts where the mode needs them)", what);
    return ODIL_E_INVAL;
  }
  if (cells < 1) {
    set_error("%s: cells %lld per member (at least 1)", what, (long long)cells);
    return ODIL_E_INVAL;
  }
  if (gparts < 1 || gparts > kMaxPartials) {
    set_error("%s: gparts %d partial sums per quantity (1..%d)", what, gparts, kMaxPartials);
    return ODIL_E_INVAL;
  }
  if (gpart_stride < (int64_t)(krylov_m + 2) * gparts) {
    set_error("%s: gpart_stride %lld is smaller than a member ((krylov_m + 2) x %d partial sums)", what,
              (long long)gpart_stride, gparts);
    return ODIL_E_INVAL;
  }
  if (mode == 0 && (nparts < 1 || nparts > kMaxPartials || partials_stride < nparts || (partials0 && partials0_stride < nparts))) {
    set_error("%s: %d partial sums %lld / %lld apart (partials_stride below one member)", what, nparts,
              (long long)partials_stride, (long long)partials0_stride);
    return ODIL_E_INVAL;
  }
  if (scal_stride < krylov_m + 2) {
    set_error("%s: scal_stride %lld is smaller than a member (krylov_m + 2 = %d scalars)", what, (long long)scal_stride,
              krylov_m + 2);
    return ODIL_E_INVAL;
  }
  if (maxcycles < 0 || k < 0 || k > maxcycles || history_stride < (int64_t)maxcycles + 2 || !(tol >= 0.0)) {
    set_error("%s: pass %d of at most %d, tolerance %g, history_stride %lld (>= maxcycles + 2)", what, k, maxcycles, tol,
              (long long)history_stride);
    return ODIL_E_INVAL;
  }
  const GcrState st{active, gcr, fresh, verify, have};
  hipLaunchKernelGGL(k_gcr_decide, dim3((unsigned)nbatch), dim3(kBlock), 0, (hipStream_t)stream, mode, partials,
                     partials_stride, partials0, partials0_stride, nparts, gpart, gpart_stride, gparts, (double)cells, k,
                     maxcycles, tol * tol, krylov_m, history, history_stride, outcome, st, scal, scal_stride);
  if (int e = check_launch("k_gcr_decide")) return e;
  if (mode == 0 || mode == 3) {
    hipLaunchKernelGGL(k_gcr_count, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, st, nbatch, counts);
    return check_launch("k_gcr_count");
  }
  return 0;
}

}  // namespace odil

using namespace odil;

extern "C" {
int64_t odil_stencil_gcr_batch_parts(int64_t cells) { return gcr_parts(cells); }
int odil_stencil_gcr_dots_batch_f64(const double* store, int64_t store_stride, int64_t cells, int krylov_m, int slot,
                                    const int* have, int max_have, const int* mask, int nbatch, double* gpart,
                                    int64_t gpart_stride, void* stream) {
  return gcr_dots<double>(store, store_stride, cells, krylov_m, slot, have, max_have, mask, nbatch, gpart, gpart_stride, stream);
}
int odil_stencil_gcr_dots_batch_f32(const float* store, int64_t store_stride, int64_t cells, int krylov_m, int slot,
                                    const int* have, int max_have, const int* mask, int nbatch, double* gpart,
                                    int64_t gpart_stride, void* stream) {
  return gcr_dots<float>(store, store_stride, cells, krylov_m, slot, have, max_have, mask, nbatch, gpart, gpart_stride, stream);
}
int odil_stencil_gcr_project_batch_f64(double* store, int64_t store_stride, const double* rho, int64_t rho_stride,
                                       int64_t cells, int krylov_m, int slot, const int* have, int max_have,
                                       const double* scal, int64_t scal_stride, const int* mask, int nbatch, double* gpart,
                                       int64_t gpart_stride, void* stream) {
  return gcr_project<double>(store, store_stride, rho, rho_stride, cells, krylov_m, slot, have, max_have, scal, scal_stride,
                             mask, nbatch, gpart, gpart_stride, stream);
}
int odil_stencil_gcr_project_batch_f32(float* store, int64_t store_stride, const float* rho, int64_t rho_stride, int64_t cells,
                                       int krylov_m, int slot, const int* have, int max_have, const double* scal,
                                       int64_t scal_stride, const int* mask, int nbatch, double* gpart, int64_t gpart_stride,
                                       void* stream) {
  return gcr_project<float>(store, store_stride, rho, rho_stride, cells, krylov_m, slot, have, max_have, scal, scal_stride,
                            mask, nbatch, gpart, gpart_stride, stream);
}
int odil_stencil_gcr_update_batch_f64(double* store, int64_t store_stride, double* x, int64_t x_stride, double* rho,
                                      int64_t rho_stride, int64_t cells, int krylov_m, int slot, const double* scal,
                                      int64_t scal_stride, const int* mask, int nbatch, double* gpart, int64_t gpart_stride,
                                      void* stream) {
  return gcr_update<double>(store, store_stride, x, x_stride, rho, rho_stride, cells, krylov_m, slot, scal, scal_stride, mask,
                            nbatch, gpart, gpart_stride, stream);
}
int odil_stencil_gcr_update_batch_f32(float* store, int64_t store_stride, float* x, int64_t x_stride, float* rho,
                                      int64_t rho_stride, int64_t cells, int krylov_m, int slot, const double* scal,
                                      int64_t scal_stride, const int* mask, int nbatch, double* gpart, int64_t gpart_stride,
                                      void* stream) {
  return gcr_update<float>(store, store_stride, x, x_stride, rho, rho_stride, cells, krylov_m, slot, scal, scal_stride, mask,
                           nbatch, gpart, gpart_stride, stream);
}
int odil_stencil_gcr_sumsq_batch_f64(const double* v, int64_t v_stride, int64_t cells, const int* mask, int nbatch,
                                     double* gpart, int64_t gpart_stride, void* stream) {
  return gcr_sumsq<double>(v, v_stride, cells, mask, nbatch, gpart, gpart_stride, stream);
}
int odil_stencil_gcr_sumsq_batch_f32(const float* v, int64_t v_stride, int64_t cells, const int* mask, int nbatch,
                                     double* gpart, int64_t gpart_stride, void* stream) {
  return gcr_sumsq<float>(v, v_stride, cells, mask, nbatch, gpart, gpart_stride, stream);
}
int odil_stencil_gcr_decide_batch(int mode, const double* partials, int64_t partials_stride, const double* partials0,
                                  int64_t partials0_stride, int nparts, const double* gpart, int64_t gpart_stride, int gparts,
                                  int nbatch, int64_t cells, int k, int maxcycles, double tol, int krylov_m, double* history,
                                  int64_t history_stride, int* outcome, int* active, int* gcr, int* fresh, int* verify,
                                  int* have, double* scal, int64_t scal_stride, int* counts, void* stream) {
  return gcr_decide(mode, partials, partials_stride, partials0, partials0_stride, nparts, gpart, gpart_stride, gparts, nbatch,
                    cells, k, maxcycles, tol, krylov_m, history, history_stride, outcome, active, gcr, fresh, verify, have, scal,
                    scal_stride, counts, stream);
}
}
