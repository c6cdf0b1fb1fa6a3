// Geometric multigrid for the damped normal equations A = M^T M (+ damping) of a Newton system whose unknowns are
// several grid fields (any loc per field, 1-3 dimensions): the reference hands any such system to smoothed-aggregation
// AMG on the normal equations (reference src/odil/linsolver.py:61-72); here the hierarchy is geometric.
//
// Representation of one level (gmg.NormalGMG builds it): the unknowns of nf fields concatenated in one flat vector
// (field f at off[f], canonical 3-D shape n[f]); for every field pair (a, b) and integer index offset o a coefficient
// array over a's grid,
//     (A x)_a[q] = sum_b sum_o C_ab,o[q] x_b[q + o]        (terms with q + o outside b's grid are zero),
// all arrays in ONE flat buffer; the entry table (device, int64, kEnt words per entry) holds (a, b, o0, o1, o2, start),
// sorted by a, entries of field a in [ebeg[a], ebeg[a + 1]).  Every kernel takes all fields in one launch, and every
// sum runs in a fixed order: no atomics, results are bit-reproducible.
#include "block_mg.h"

namespace odil {

// ---------------------------------------------------------------------------------------------------------------------
// Apply: y = A x (mode 0), y = b - A x (mode 1), one weighted Jacobi sweep y = x + omega dinv (b - A x) (mode 2), or the
// sweep from the zero vector y = omega dinv b (mode 3: x, coef and the table are not read).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bmg_apply(const T* __restrict__ coef, const int64_t* __restrict__ table,
                                                     BmgLevel L, const T* __restrict__ x, const T* __restrict__ b,
                                                     const T* __restrict__ dinv, T* __restrict__ y, int mode, T omega) {
  const int64_t n = L.off[L.nf];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (mode == 3) {
    y[i] = omega * (dinv[i] * b[i]);
    return;
  }
  const int a = field_of(L, i);
  const int64_t q = i - L.off[a];
  const int64_t na1 = L.n[a][1], na2 = L.n[a][2];
  const int64_t q2 = q % na2, q1 = (q / na2) % na1, q0 = q / (na1 * na2);
  T acc = T(0);
  for (int e = L.ebeg[a]; e < L.ebeg[a + 1]; ++e) {
    const int64_t* t = table + (int64_t)e * kEnt;
    const int bf = (int)t[1];
    const int64_t t0 = q0 + t[2], t1 = q1 + t[3], t2 = q2 + t[4];
    if (t0 < 0 || t0 >= L.n[bf][0] || t1 < 0 || t1 >= L.n[bf][1] || t2 < 0 || t2 >= L.n[bf][2]) continue;
    acc = acc + coef[t[5] + q] * x[L.off[bf] + (t0 * L.n[bf][1] + t1) * L.n[bf][2] + t2];
  }
  if (mode == 0)
    y[i] = acc;
  else if (mode == 1)
    y[i] = b[i] - acc;
  else
    y[i] = x[i] + omega * (dinv[i] * (b[i] - acc));
}

// ---------------------------------------------------------------------------------------------------------------------
// Assemble: out[j] += c1[r(j)] c2[r(j)] over a's grid, for ONE pair of stencil blocks of the same output and ONE
// offset.  rmap holds, per axis of a's grid (concatenated, lengths n_a[0], n_a[1], n_a[2]), the row index of the
// output grid that reads a at j_d AND whose read of b lies at j_d + o_d -- or -1 (gather form: every row reads one
// entry of a per block, so at most one row contributes to j).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bmg_assemble(const T* __restrict__ c1, const T* __restrict__ c2,
                                                        const int64_t* __restrict__ rmap, int64_t na0, int64_t na1,
                                                        int64_t na2, int64_t nr1, int64_t nr2, T* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= na0 * na1 * na2) return;
  const int64_t j2 = j % na2, j1 = (j / na2) % na1, j0 = j / (na1 * na2);
  const int64_t r0 = rmap[j0], r1 = rmap[na0 + j1], r2 = rmap[na0 + na1 + j2];
  if (r0 < 0 || r1 < 0 || r2 < 0) return;
  const int64_t r = (r0 * nr1 + r1) * nr2 + r2;
  out[j] = out[j] + c1[r] * c2[r];
}

// ---------------------------------------------------------------------------------------------------------------------
// Transfers, per axis by code: 0 = not coarsened (identity), 1 = cells (coarse cell I has the fine children 2I, 2I+1;
// a fine cell takes 3/4 of its parent and 1/4 of the parent's neighbour on its side, all of the parent at a wall),
// 2 = nodes (coarse node I on fine node 2I, linear in between).  Restriction is the transpose of the prolongation.
struct BmgTransfer {
  BmgLevel fine, coarse;
  int code[kBmgMaxFields][3];
};

// P[i, I] of one axis (i fine, I coarse; nc coarse extent)
__device__ inline double pw1(int64_t i, int64_t I, int code, int64_t nc) {
  if (code == 0) return i == I ? 1.0 : 0.0;
  if (code == 2) {
    const int64_t d = i - 2 * I;
    return d == 0 ? 1.0 : (d == 1 || d == -1) ? 0.5 : 0.0;
  }
  const int64_t p = i >> 1, nb = (i & 1) ? p + 1 : p - 1;
  const bool wall = nb < 0 || nb >= nc;
  if (I == p) return wall ? 1.0 : 0.75;
  if (I == nb) return 0.25;
  return 0.0;
}

// fine indices i with P[i, I] != 0 (at most 4), within [0, nfine)
__device__ inline int fine_support(int64_t I, int code, int64_t nfine, int64_t (&idx)[4]) {
  int k = 0;
  const int64_t lo = code == 0 ? I : 2 * I - 1, hi = code == 0 ? I : code == 2 ? 2 * I + 1 : 2 * I + 2;
  for (int64_t i = lo; i <= hi; ++i)
    if (i >= 0 && i < nfine) idx[k++] = i;
  return k;
}

// restrict (mode 0): out_c = P^T in_f over all fields; prolong (mode 1): out_f = add_f + P in_c (out may alias add)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bmg_transfer(BmgTransfer tr, const T* __restrict__ in, const T* add,
                                                        T* out, int mode) {
  const BmgLevel& O = mode == 0 ? tr.coarse : tr.fine;
  const BmgLevel& I = mode == 0 ? tr.fine : tr.coarse;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= O.off[O.nf]) return;
  const int f = field_of(O, i);
  const int64_t q = i - O.off[f];
  int64_t id[3];
  id[2] = q % O.n[f][2];
  id[1] = (q / O.n[f][2]) % O.n[f][1];
  id[0] = q / (O.n[f][1] * O.n[f][2]);
  int64_t src[3][4];
  double w[3][4];
  int cnt[3];
  for (int d = 0; d < 3; ++d) {
    const int code = tr.code[f][d];
    const int64_t nc = tr.coarse.n[f][d];
    cnt[d] = 0;
    if (mode == 0) {
      int64_t sup[4];
      const int k = fine_support(id[d], code, tr.fine.n[f][d], sup);
      for (int s = 0; s < k; ++s) {
        src[d][cnt[d]] = sup[s];
        w[d][cnt[d]++] = pw1(sup[s], id[d], code, nc);
      }
    } else {
      const int64_t fi = id[d];
      const int64_t lo = code == 0 ? fi : code == 2 ? (fi - 1) >> 1 : (fi >> 1) - 1;
      const int64_t hi = code == 0 ? fi : code == 2 ? (fi + 1) >> 1 : (fi >> 1) + 1;
      for (int64_t J = lo; J <= hi; ++J) {
        if (J < 0 || J >= nc) continue;
        const double v = pw1(fi, J, code, nc);
        if (v != 0.0) {
          src[d][cnt[d]] = J;
          w[d][cnt[d]++] = v;
        }
      }
    }
  }
  const int64_t n1 = I.n[f][1], n2 = I.n[f][2], base = I.off[f];
  T acc = T(0);
  for (int s0 = 0; s0 < cnt[0]; ++s0)
    for (int s1 = 0; s1 < cnt[1]; ++s1)
      for (int s2 = 0; s2 < cnt[2]; ++s2)
        acc = acc + T(w[0][s0] * w[1][s1] * w[2][s2]) * in[base + (src[0][s0] * n1 + src[1][s1]) * n2 + src[2][s2]];
  out[i] = mode == 0 ? acc : add[i] + acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// Galerkin coarsening: C^c_ab,oc[I] = sum_{fine entries (a, b, o)} sum_i P_a[i, I] C_ab,o[i] P_b[i + o, I + oc], one
// thread per coarse coefficient, gather form (per axis the pairs (i_d, weight) are listed first; an entry with an empty
// list on some axis costs three short loops).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bmg_galerkin(BmgTransfer tr, const T* __restrict__ fcoef,
                                                        const int64_t* __restrict__ ftable,
                                                        const int64_t* __restrict__ ctable, int nce, int64_t total,
                                                        T* __restrict__ ccoef) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= total) return;
  // the coarse entry holding t (starts increase along the table)
  int lo = 0, hi = nce - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (ctable[(int64_t)mid * kEnt + 5] <= t) lo = mid;
    else hi = mid - 1;
  }
  const int64_t* ce = ctable + (int64_t)lo * kEnt;
  const int a = (int)ce[0], bf = (int)ce[1];
  const BmgLevel& F = tr.fine;
  const BmgLevel& C = tr.coarse;
  const int64_t q = t - ce[5];
  int64_t I[3], J[3];
  I[2] = q % C.n[a][2];
  I[1] = (q / C.n[a][2]) % C.n[a][1];
  I[0] = q / (C.n[a][1] * C.n[a][2]);
  for (int d = 0; d < 3; ++d) J[d] = I[d] + ce[2 + d];
  T acc = T(0);
  bool inside = true;
  for (int d = 0; d < 3; ++d) inside = inside && J[d] >= 0 && J[d] < C.n[bf][d];
  if (inside) {
    int64_t sup[3][4];
    int ns[3];
    for (int d = 0; d < 3; ++d) ns[d] = fine_support(I[d], tr.code[a][d], F.n[a][d], sup[d]);
    for (int e = F.ebeg[a]; e < F.ebeg[a + 1]; ++e) {
      const int64_t* fe = ftable + (int64_t)e * kEnt;
      if ((int)fe[1] != bf) continue;
      int64_t idx[3][4];
      double w[3][4];
      int cnt[3];
      bool any = true;
      for (int d = 0; d < 3 && any; ++d) {
        cnt[d] = 0;
        for (int s = 0; s < ns[d]; ++s) {
          const int64_t i = sup[d][s], k = i + fe[2 + d];
          if (k < 0 || k >= F.n[bf][d]) continue;
          const double v = pw1(k, J[d], tr.code[bf][d], C.n[bf][d]);
          if (v == 0.0) continue;
          idx[d][cnt[d]] = i;
          w[d][cnt[d]++] = pw1(i, I[d], tr.code[a][d], C.n[a][d]) * v;
        }
        any = cnt[d] > 0;
      }
      if (!any) continue;
      const T* c = fcoef + fe[5];
      const int64_t n1 = F.n[a][1], n2 = F.n[a][2];
      for (int s0 = 0; s0 < cnt[0]; ++s0)
        for (int s1 = 0; s1 < cnt[1]; ++s1)
          for (int s2 = 0; s2 < cnt[2]; ++s2)
            acc = acc + T(w[0][s0] * w[1][s1] * w[2][s2]) * c[(idx[0][s0] * n1 + idx[1][s1]) * n2 + idx[2][s2]];
    }
  }
  ccoef[t] = acc;
}

static int parse_transfer(const int64_t* fdesc, const int64_t* cdesc, const int* code, BmgTransfer& tr,
                          const char* what) {
  if (int e = parse_level(fdesc, tr.fine, what)) return e;
  if (int e = parse_level(cdesc, tr.coarse, what)) return e;
  if (!code || tr.fine.nf != tr.coarse.nf) {
    set_error("%s: fine and coarse levels differ in their fields", what);
    return ODIL_E_INVAL;
  }
  for (int f = 0; f < tr.fine.nf; ++f)
    for (int d = 0; d < 3; ++d) {
      const int c = code[3 * f + d];
      const int64_t nf = tr.fine.n[f][d], nc = tr.coarse.n[f][d];
      const bool ok = (c == 0 && nc == nf) || (c == 1 && nf == 2 * nc) || (c == 2 && nf == 2 * nc - 1 && nc >= 2);
      if (!ok) {
        set_error("%s: field %d axis %d: extents %lld -> %lld do not match transfer code %d", what, f, d, (long long)nf,
                  (long long)nc, c);
        return ODIL_E_INVAL;
      }
      tr.code[f][d] = c;
    }
  return 0;
}

template <typename T>
static int bmg_apply(const T* coef, const int64_t* table, const int64_t* desc, const T* x, const T* b, const T* dinv,
                     T* y, int mode, T omega, void* stream) {
  BmgLevel L;
  if (int e = parse_level(desc, L, "bmg_apply")) return e;
  const bool need_a = mode != 3, need_b = mode != 0, need_d = mode >= 2;
  if (mode < 0 || mode > 3 || !y || (need_a && (!coef || !table || !x)) || (need_b && !b) || (need_d && !dinv) ||
      (need_a && x == y)) {
    set_error("bmg_apply: invalid mode %d, null pointer or x aliasing y", mode);
    return ODIL_E_INVAL;
  }
  const int64_t n = L.off[L.nf];
  hipLaunchKernelGGL(k_bmg_apply<T>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, coef, table, L, x, b, dinv, y, mode, omega);
  return check_launch("k_bmg_apply");
}

template <typename T>
static int bmg_assemble(const T* c1, const T* c2, const int64_t* rmap, const int64_t* ashape, const int64_t* rshape,
                        T* out, void* stream) {
  if (!c1 || !c2 || !rmap || !ashape || !rshape || !out) {
    set_error("bmg_assemble: null pointer");
    return ODIL_E_INVAL;
  }
  for (int d = 0; d < 3; ++d)
    if (ashape[d] < 1 || rshape[d] < 1) {
      set_error("bmg_assemble: empty extent");
      return ODIL_E_INVAL;
    }
  const int64_t n = ashape[0] * ashape[1] * ashape[2];
  hipLaunchKernelGGL(k_bmg_assemble<T>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, c1, c2, rmap, ashape[0], ashape[1], ashape[2], rshape[1], rshape[2], out);
  return check_launch("k_bmg_assemble");
}

template <typename T>
static int bmg_transfer(const int64_t* fdesc, const int64_t* cdesc, const int* code, const T* in, const T* add, T* out,
                        int mode, void* stream) {
  BmgTransfer tr;
  if (int e = parse_transfer(fdesc, cdesc, code, tr, "bmg_transfer")) return e;
  if ((mode != 0 && mode != 1) || !in || !out || in == out || (mode == 1 && !add)) {
    set_error("bmg_transfer: invalid mode %d, null pointer or in aliasing out", mode);
    return ODIL_E_INVAL;
  }
  const int64_t n = mode == 0 ? tr.coarse.off[tr.coarse.nf] : tr.fine.off[tr.fine.nf];
  hipLaunchKernelGGL(k_bmg_transfer<T>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, tr, in, add, out, mode);
  return check_launch("k_bmg_transfer");
}

template <typename T>
static int bmg_galerkin(const int64_t* fdesc, const int64_t* cdesc, const int* code, const T* fcoef,
                        const int64_t* ftable, const int64_t* ctable, int nce, int64_t total, T* ccoef, void* stream) {
  BmgTransfer tr;
  if (int e = parse_transfer(fdesc, cdesc, code, tr, "bmg_galerkin")) return e;
  if (!fcoef || !ftable || !ctable || !ccoef || nce < 1 || total < 1) {
    set_error("bmg_galerkin: null pointer or empty table");
    return ODIL_E_INVAL;
  }
  hipLaunchKernelGGL(k_bmg_galerkin<T>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, tr, fcoef, ftable, ctable, nce, total, ccoef);
  return check_launch("k_bmg_galerkin");
}

}  // namespace odil

using namespace odil;

extern "C" {
int odil_bmg_apply_f64(const double* coef, const int64_t* table, const int64_t* desc, const double* x, const double* b,
                       const double* dinv, double* y, int mode, double omega, void* stream) {
  return bmg_apply<double>(coef, table, desc, x, b, dinv, y, mode, omega, stream);
}
int odil_bmg_apply_f32(const float* coef, const int64_t* table, const int64_t* desc, const float* x, const float* b,
                       const float* dinv, float* y, int mode, float omega, void* stream) {
  return bmg_apply<float>(coef, table, desc, x, b, dinv, y, mode, omega, stream);
}
int odil_bmg_assemble_f64(const double* c1, const double* c2, const int64_t* rmap, const int64_t* ashape,
                          const int64_t* rshape, double* out, void* stream) {
  return bmg_assemble<double>(c1, c2, rmap, ashape, rshape, out, stream);
}
int odil_bmg_assemble_f32(const float* c1, const float* c2, const int64_t* rmap, const int64_t* ashape,
                          const int64_t* rshape, float* out, void* stream) {
  return bmg_assemble<float>(c1, c2, rmap, ashape, rshape, out, stream);
}
int odil_bmg_transfer_f64(const int64_t* fdesc, const int64_t* cdesc, const int* code, const double* in,
                          const double* add, double* out, int mode, void* stream) {
  return bmg_transfer<double>(fdesc, cdesc, code, in, add, out, mode, stream);
}
int odil_bmg_transfer_f32(const int64_t* fdesc, const int64_t* cdesc, const int* code, const float* in,
                          const float* add, float* out, int mode, void* stream) {
  return bmg_transfer<float>(fdesc, cdesc, code, in, add, out, mode, stream);
}
int odil_bmg_galerkin_f64(const int64_t* fdesc, const int64_t* cdesc, const int* code, const double* fcoef,
                          const int64_t* ftable, const int64_t* ctable, int nce, int64_t total, double* ccoef,
                          void* stream) {
  return bmg_galerkin<double>(fdesc, cdesc, code, fcoef, ftable, ctable, nce, total, ccoef, stream);
}
int odil_bmg_galerkin_f32(const int64_t* fdesc, const int64_t* cdesc, const int* code, const float* fcoef,
                          const int64_t* ftable, const int64_t* ctable, int nce, int64_t total, float* ccoef,
                          void* stream) {
  return bmg_galerkin<float>(fdesc, cdesc, code, fcoef, ftable, ctable, nce, total, ccoef, stream);
}
}
