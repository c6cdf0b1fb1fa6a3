// Shared tap tables of the multigrid transfer kernels (mg_transfer.hip, mg_fast.hip).
#pragma once
#include "common.h"

namespace odil {

// ------------------------------------------------------------------------------------
// Taps of the 1-D prolongation for one fine index k on an axis of type `loc` with n
// coarse points.  In the reference's (r) order (core.py:675-687): r = 0 first.
// 'c': k = 2i+s reads padded index (i+s)+r-1, weights s ? (3,1) : (1,3), sum 4.
// 'n': k = 2i+s reads i (+ i+1 if s), weights 1, sum 1+s.   '.': identity.
// Out-of-range 'c' indices (-1, n) are ghosts: 2*u[clamp] - u[reflect], evaluated
// JOINTLY over all 'c' axes (core.py:640-643), hence the per-tap clamp/reflect pair.
// ------------------------------------------------------------------------------------
struct Taps {
  int cnt;
  int64_t cl[2], rf[2];
  int w[2];
  bool out[2];
  int sum;
};

__device__ __host__ inline Taps make_taps(int loc, int64_t k, int64_t n) {
  Taps t;
  t.cnt = 1;
  t.cl[0] = t.rf[0] = k;
  t.cl[1] = t.rf[1] = 0;
  t.w[0] = 1;
  t.w[1] = 0;
  t.out[0] = t.out[1] = false;
  t.sum = 1;
  if (loc == kCell) {
    int64_t i = k >> 1;
    int s = (int)(k & 1);
    t.cnt = 2;
    t.sum = 4;
    t.w[0] = s ? 3 : 1;
    t.w[1] = s ? 1 : 3;
    for (int r = 0; r < 2; ++r) {
      int64_t j = i + s + r - 1;
      bool o = j < 0 || j >= n;
      t.out[r] = o;
      t.cl[r] = j < 0 ? 0 : (j >= n ? n - 1 : j);
      t.rf[r] = j < 0 ? 1 : (j >= n ? n - 2 : j);
    }
  } else if (loc == kNode) {
    int64_t i = k >> 1;
    int s = (int)(k & 1);
    t.cl[0] = t.rf[0] = i;
    if (s) {
      t.cnt = 2;
      t.sum = 2;
      t.w[1] = 1;
      t.cl[1] = t.rf[1] = i + 1;
    }
  }
  return t;
}

struct InterpArgs {
  int64_t cn[4];  // coarse array shape (canonical 4-D)
  int64_t fn[4];  // fine array shape
  int loc[4];
  // slab decomposition: array axis 0 (canonical index cut_axis) is cut at its low / high end,
  // i.e. that end is an interior interface with ghost planes, not a physical boundary
  int cut_axis, cut_lo, cut_hi;
  // elements between consecutive LEADING indices of the coarse array when it is a view whose leading stride exceeds
  // its volume (a ghost-extended level array of the slab paths without its outer ghost planes); 0: contiguous
  int64_t coarse_ld;
  RowSched sched;
};

// ------------------------------------------------------------------------------------
// P^T in gather form.  With gpad = (tensor-product transpose onto the padded coarse
// grid), the joint ghost rule upad = 2*u[clamp] - u[reflect] gives
//   gc[J] = 2 * sum_{j: clamp(j)=J} gpad[j] - sum_{j: reflect(j)=J} gpad[j],
// and both sums stay separable: per axis the 1-D weights W(j,k) are summed over
//   C(J) = {J} + {-1 if J==0} + {n if J==n-1}   resp.   R(J) = {J} + {-1 if J==1} + {n if J==n-2}.
// 1-D weights: 'c' W(j,k) = {1,3,3,1}/4 at k-2j = -1..2; 'n' {1/2,1,1/2} at k-2j = -1..1.
// ------------------------------------------------------------------------------------
struct AdjTaps {
  int64_t k0;  // first fine index of the window
  int cnt;     // window length (<= 6)
  float wc[6], wr[6];
  bool special;  // wc != wr somewhere
};

__device__ inline float w_cell(int64_t j, int64_t k, int64_t F) {
  if (k < 0 || k >= F) return 0.f;
  int64_t d = k - 2 * j;
  return (d == 0 || d == 1) ? 0.75f : ((d == -1 || d == 2) ? 0.25f : 0.f);
}
// (the march / tile kernels index with int: a 64-bit compare is several instructions, and the wall paths evaluate
// dozens of these per step)
__device__ inline float w_cell(int j, int k, int F) {
  if (k < 0 || k >= F) return 0.f;
  const int d = k - 2 * j;
  return (d == 0 || d == 1) ? 0.75f : ((d == -1 || d == 2) ? 0.25f : 0.f);
}

__device__ inline AdjTaps make_adj_taps(int loc, int64_t J, int64_t n, int64_t F, bool cut_lo = false,
                                       bool cut_hi = false) {
  AdjTaps t;
  t.special = false;
  if (loc == kCell) {
    const bool c_lo = J == 0 && !cut_lo, c_hi = J == n - 1 && !cut_hi, r_lo = J == 1 && !cut_lo,
               r_hi = J == n - 2 && !cut_hi;
    t.special = c_lo || c_hi || r_lo || r_hi;
    if (t.special) {
      t.k0 = 2 * J - 2;
      t.cnt = 6;
    } else {
      t.k0 = 2 * J - 1;
      t.cnt = 4;
    }
    for (int i = 0; i < 6; ++i) {
      int64_t k = t.k0 + i;
      float w = i < t.cnt ? w_cell(J, k, F) : 0.f;
      float lo = w_cell((int64_t)-1, k, F), hi = w_cell(n, k, F);
      t.wc[i] = i < t.cnt ? w + (c_lo ? lo : 0.f) + (c_hi ? hi : 0.f) : 0.f;
      t.wr[i] = i < t.cnt ? w + (r_lo ? lo : 0.f) + (r_hi ? hi : 0.f) : 0.f;
    }
  } else if (loc == kNode) {
    t.k0 = 2 * J - 1;
    t.cnt = 3;
    for (int i = 0; i < 6; ++i) {
      int64_t k = t.k0 + i;
      float w = (i < 3 && k >= 0 && k < F) ? (i == 1 ? 1.f : 0.5f) : 0.f;
      t.wc[i] = t.wr[i] = w;
    }
  } else {
    t.k0 = J;
    t.cnt = 1;
    for (int i = 0; i < 6; ++i) t.wc[i] = t.wr[i] = i == 0 ? 1.f : 0.f;
  }
  return t;
}

// One coarse value of P^T on a canonical 4-D array: the sums over the windows of the four axes, the leading axis
// outermost, zero-weight taps skipped, the reflect sum only where some axis is special.  gfine: the fine array (of one
// row), fs0 / fs1 / fs2 its strides.  The generic kernel and its row form (mg_transfer.hip) both sum here.
template <typename T>
__device__ __forceinline__ T interp_adj_gather(const AdjTaps& t0, const AdjTaps& t1, const AdjTaps& t2, const AdjTaps& t3,
                                               int64_t fs0, int64_t fs1, int64_t fs2, const T* __restrict__ gfine) {
  const bool special = t0.special || t1.special || t2.special || t3.special;
  T sc = T(0), sr = T(0);
  for (int i0 = 0; i0 < t0.cnt; ++i0) {
    if (t0.wc[i0] == 0.f && t0.wr[i0] == 0.f) continue;
    for (int i1 = 0; i1 < t1.cnt; ++i1) {
      if (t1.wc[i1] == 0.f && t1.wr[i1] == 0.f) continue;
      for (int i2 = 0; i2 < t2.cnt; ++i2) {
        if (t2.wc[i2] == 0.f && t2.wr[i2] == 0.f) continue;
        const T wcl = T(t0.wc[i0] * t1.wc[i1] * t2.wc[i2]);
        const T wrl = T(t0.wr[i0] * t1.wr[i1] * t2.wr[i2]);
        const int64_t base = (t0.k0 + i0) * fs0 + (t1.k0 + i1) * fs1 + (t2.k0 + i2) * fs2;
        for (int i3 = 0; i3 < t3.cnt; ++i3) {
          if (t3.wc[i3] == 0.f && t3.wr[i3] == 0.f) continue;
          const T g = gfine[base + t3.k0 + i3];
          sc = sc + (wcl * T(t3.wc[i3])) * g;
          if (special) sr = sr + (wrl * T(t3.wr[i3])) * g;
        }
      }
    }
  }
  return special ? T(2) * sc - sr : sc;
}

// Fast paths (mg_fast.hip): last axis 'c', second-to-last 'c' or '.', any leading axes.
// Return 1 if they handled the call, 0 if the generic kernel must run, <0 on error.
template <typename T>
int interp_add_fast(const T* coarse, const T* add, T* fine, const InterpArgs& a, T cscale, T ascale,
                    hipStream_t stream);
template <typename T>
int interp_adj_fast(const T* gfine, T* gcoarse, T* gscaled, const InterpArgs& a, T scale, hipStream_t stream,
                    const AdamArgs<T>& ad);

// Would the fast kernels take this layout (the predicate of both functions above, nothing launched)?
bool interp_fast_serves(const InterpArgs& a);

// z-marching variants (mg_march.hip): exactly 'ccc' (3-D, all cell-centred).
template <typename T>
int interp_add_march(const T* coarse, const T* add, T* fine, const InterpArgs& a, T cscale, T ascale,
                     hipStream_t stream);
template <typename T>
int interp_adj_march(const T* gfine, T* gcoarse, T* gscaled, const InterpArgs& a, T scale, hipStream_t stream,
                     const AdamArgs<T>& ad);

// The transposed prolongation interp_adj runs for a layout whose arrays are aligned to 16 bytes (nothing launched):
// the rows / tile / march kernels of mg_march.hip (their summation orders differ), a node-centred marching kernel, the
// fast kernel of mg_fast.hip, or the generic kernel.
enum AdjKind { kAdjGeneric = 0, kAdjFast, kAdjNode, kAdjRows, kAdjTile, kAdjMarch };
template <typename T>
int interp_adj_kind(const InterpArgs& a);

// P^T of `nrows` stacked 'ncc' volumes ([nrows, *shape] arrays) through the node-centred marching kernel ONE volume of
// the layout `one` runs (kAdjNode), row by row on blockIdx.y: 1 when launched, 0 when not that case, < 0 on error.
template <typename T>
int interp_adj_march_n_rows(const T* gfine, T* gcoarse, const InterpArgs& one, int nrows, hipStream_t stream,
                            const AdamArgs<T>& ad);

// P^T of `nrows` stacked rows of FOUR axes ([nrows, *shape] arrays; `one`: the layout of ONE row), the row on a grid
// dimension the single kernel does not use: the fast kernel (kAdjFast) and the 'nccc' marching kernel (kAdjNode with a
// leading axis).  1 when launched, 0 when a single row would not run that kernel, < 0 on error.
template <typename T>
int interp_adj_fast_rows(const T* gfine, T* gcoarse, const InterpArgs& one, int nrows, hipStream_t stream,
                         const AdamArgs<T>& ad);
// P of the same rows through the fast kernel (factors 1): 1 when launched, 0 when the fast kernel does not take the layout.
template <typename T>
int interp_add_fast_rows(const T* coarse, const T* add, T* fine, const InterpArgs& one, int nrows, hipStream_t stream);
template <typename T>
int interp_adj_march_lead_rows(const T* gfine, T* gcoarse, const InterpArgs& one, int nrows, hipStream_t stream,
                               const AdamArgs<T>& ad);

}  // namespace odil
