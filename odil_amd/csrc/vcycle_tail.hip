// The COARSE TAIL of a multigrid V-cycle in ONE launch (gmg.PoissonGMG / gmg.StencilGMG: the Newton solve; the reference
// hands that system to SuperLU / pyamg, src/odil/linsolver.py:17-26, 61-72).
//
// Levels of a few thousand cells cost a launch each for every sweep, residual, restriction and prolongation -- ~7
// dependent launches per level and cycle, 5 - 12 us apiece on a GPU that finishes the work itself in under a microsecond:
// at 512^3 the levels from 16^3 down are 28 of a cycle's 57 launches and ~0.3 of its 3.3 ms.  Here ONE workgroup walks
// the whole tail -- pre-smoothing, residual + restriction, the dense solve on the coarsest grid, prolongation +
// post-smoothing, level after level -- with a workgroup barrier where a launch boundary used to be.
//
// The operator of every level is given by coefficient arrays (the layout of stencil_mg.hip: (2 d + 1) arrays per level,
// order 0, -e_0, +e_0, ...; neighbours wrap periodically, wall rows carry a zero towards the wall), which serves both
// cycles: the constant-coefficient Poisson hierarchy passes odil_poisson_jac_coeffs of its rediscretised levels.
//   sweep         x' = x - w (A x - b) / c0
//   coarse rhs    b_c = mean over the merged children of (b - A x)
//   correction    x += P x_c, P = the multigrid decomposition's prolongation with its joint ghost rule
//                 (reference core.py:606-700, 640-643) on the merged axes, identity on the others
//   coarsest      x = inv b, the (pseudo-)inverse the host built once
// fmg: the nested-iteration start instead of one cycle -- b is restricted to every level, the coarsest problem solved,
// every finer level starts one cycle from the interpolated solution of the level below.
#include "common.h"

namespace odil {

constexpr int kTailMaxLev = 8;
constexpr int kTailThreads = 1024;

struct TailLevel {
  int n[3];       // canonical (Z, Y, X), leading extents 1 for d < 3
  float rn[3];    // 1 / n
  int halve[3];   // the transition to the next coarser level merges pairs of cells of this axis
  int size;
  int64_t c;      // offset of this level's coefficient arrays in `coeffs`
  int64_t x, t, b;  // offsets of its iterate / spare / right-hand side in `work`
};

template <typename T>
struct TailArgs {
  int nlev, ndim;
  int has[3], slot[3];
  TailLevel lv[kTailMaxLev];
  int npre, npost, fmg, ninv;
  T wpre[4], wpost[4];
};

// i / n for 0 <= i < 2^22 without the ~40-instruction integer divide: the float quotient is off by at most one
__device__ __forceinline__ int tail_div(int i, int n, float rn) {
  int q = (int)((float)i * rn);
  q = q * n > i ? q - 1 : q;
  q = (q + 1) * n <= i ? q + 1 : q;
  return q;
}

__device__ __forceinline__ void tail_decode(int i, const TailLevel& L, int (&id)[3]) {
  const int r = tail_div(i, L.n[2], L.rn[2]);
  id[2] = i - r * L.n[2];
  id[0] = tail_div(r, L.n[1], L.rn[1]);
  id[1] = r - id[0] * L.n[1];
}

// (A x)[i]; zero: x is the zero vector (the start of every coarse-grid correction) and is not read
template <typename T>
__device__ __forceinline__ T tail_apply(const T* __restrict__ c, const T* __restrict__ x, bool zero, const TailLevel& L,
                                        const TailArgs<T>& a, int i, const int (&id)[3]) {
  if (zero) return T(0);
  T acc = c[i] * x[i];
  const int stride[3] = {L.n[1] * L.n[2], L.n[2], 1};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (!a.has[d]) continue;
    const int n = L.n[d];
    const int im = id[d] == 0 ? i + (n - 1) * stride[d] : i - stride[d];
    const int ip = id[d] == n - 1 ? i - (n - 1) * stride[d] : i + stride[d];
    acc = acc + c[(int64_t)a.slot[d] * L.size + i] * x[im];
    acc = acc + c[(int64_t)(a.slot[d] + 1) * L.size + i] * x[ip];
  }
  return acc;
}

template <typename T>
__device__ void tail_sweep(const T* __restrict__ c, const T* __restrict__ x, bool zero, const T* __restrict__ b,
                           T* __restrict__ out, T w, const TailLevel& L, const TailArgs<T>& a) {
#pragma unroll 4
  for (int i = threadIdx.x; i < L.size; i += kTailThreads) {
    int id[3];
    tail_decode(i, L, id);
    const T ax = tail_apply<T>(c, x, zero, L, a, i, id);
    out[i] = (zero ? T(0) : x[i]) - w * (ax - b[i]) / c[i];
  }
  __syncthreads();
}

// bc = mean over the merged children of (b - A x)  (x == nullptr: of b itself -- the restriction of a right-hand side)
template <typename T>
__device__ void tail_restrict(const T* __restrict__ c, const T* __restrict__ x, bool zero, const T* __restrict__ b,
                              T* __restrict__ bc, const TailLevel& L, const TailLevel& C, const TailArgs<T>& a, bool residual) {
  const int k0 = L.halve[0] ? 2 : 1, k1 = L.halve[1] ? 2 : 1, k2 = L.halve[2] ? 2 : 1;
  const T scale = T(1) / T(k0 * k1 * k2);
  for (int I = threadIdx.x; I < C.size; I += kTailThreads) {
    int cid[3];
    tail_decode(I, C, cid);
    T sum = T(0);
    for (int p = 0; p < k0; ++p)
      for (int q = 0; q < k1; ++q)
        for (int r = 0; r < k2; ++r) {
          int id[3] = {L.halve[0] ? 2 * cid[0] + p : cid[0], L.halve[1] ? 2 * cid[1] + q : cid[1],
                       L.halve[2] ? 2 * cid[2] + r : cid[2]};
          const int i = (id[0] * L.n[1] + id[1]) * L.n[2] + id[2];
          T v = b[i];
          if (residual) v = v - tail_apply<T>(c, x, zero, L, a, i, id);
          sum = sum + v;
        }
    bc[I] = scale * sum;
  }
  __syncthreads();
}

// P xc (add: + xin) on level L from level C; result to out (not xin)
template <typename T>
__device__ void tail_prolong(const T* __restrict__ xc, const T* __restrict__ xin, bool add, T* __restrict__ out,
                             const TailLevel& L, const TailLevel& C) {
  for (int i = threadIdx.x; i < L.size; i += kTailThreads) {
    int id[3];
    tail_decode(i, L, id);
    // per axis: two taps (clamped, reflected index, weight, beyond a wall) on a merged axis, one on the others
    int cl[3][2], rf[3][2], w[3][2], cnt[3];
    bool out_[3][2];
    int den = 1;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (L.halve[d]) {
        const int j0 = id[d] >> 1, s = id[d] & 1, n = C.n[d];
        cnt[d] = 2;
        den *= 4;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int j = j0 + s + r - 1;
          out_[d][r] = j < 0 || j >= n;
          cl[d][r] = j < 0 ? 0 : (j >= n ? n - 1 : j);
          rf[d][r] = j < 0 ? (n > 1 ? 1 : 0) : (j >= n ? (n > 1 ? n - 2 : 0) : j);
          w[d][r] = (s == r) ? 1 : 3;
        }
      } else {
        cnt[d] = 1;
        cl[d][0] = rf[d][0] = id[d];
        w[d][0] = 1;
        out_[d][0] = false;
        cl[d][1] = rf[d][1] = 0, w[d][1] = 0, out_[d][1] = false;
      }
    }
    T s = T(0);
#pragma unroll
    for (int r0 = 0; r0 < 2; ++r0)
#pragma unroll
      for (int r1 = 0; r1 < 2; ++r1)
#pragma unroll
        for (int r2 = 0; r2 < 2; ++r2) {
          if (r0 >= cnt[0] || r1 >= cnt[1] || r2 >= cnt[2]) continue;
          const bool o = out_[0][r0] || out_[1][r1] || out_[2][r2];
          const T vc = xc[(cl[0][r0] * C.n[1] + cl[1][r1]) * C.n[2] + cl[2][r2]];
          T v = vc;
          if (o) v = T(2) * vc - xc[(rf[0][r0] * C.n[1] + rf[1][r1]) * C.n[2] + rf[2][r2]];
          s = s + T(w[0][r0] * w[1][r1] * w[2][r2]) * v;
        }
    s = s * (T(1) / T(den));
    out[i] = add ? xin[i] + s : s;
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(kTailThreads) void k_vcycle_tail(const T* __restrict__ coeffs, const T* xin,
                                                              const T* __restrict__ btop, T* xout, T* work,
                                                              const T* __restrict__ inv, TailArgs<T> a) {
  const int last = a.nlev - 1;
  // where the iterate of a level lives (uniform bookkeeping: every thread holds the same pointers)
  // (in LDS, every thread writing the same values: indexed by a run-time level, private arrays would live in scratch
  // memory and every phase would start with a chain of scratch loads)
  __shared__ const T* cur[kTailMaxLev];
  __shared__ T* bufA[kTailMaxLev];
  __shared__ T* bufB[kTailMaxLev];
  __shared__ const T* rhs[kTailMaxLev];
  __shared__ T* rhsw[kTailMaxLev];
  for (int l = 0; l < kTailMaxLev; ++l) {
    bufA[l] = l == 0 ? xout : work + a.lv[l].x;
    bufB[l] = work + a.lv[l].t;
    rhsw[l] = work + a.lv[l].b;
    rhs[l] = l == 0 ? btop : rhsw[l];
    cur[l] = nullptr;
  }
  auto other = [&](int l) -> T* { return cur[l] == bufA[l] ? bufB[l] : bufA[l]; };
  auto coarsest = [&]() {
    const TailLevel& L = a.lv[last];
    T* out = bufA[last];
    const T* b = rhs[last];
    for (int r = threadIdx.x; r < L.size; r += kTailThreads) {
      T s = T(0);
      for (int j = 0; j < L.size; ++j) s = s + inv[(int64_t)r * L.size + j] * b[j];
      out[r] = s;
    }
    __syncthreads();
    cur[last] = out;
  };
  // one V-cycle on level `top` of the tail; cur[top] == nullptr: from the zero iterate
  auto vcycle = [&](int top) {
    for (int l = top; l < last; ++l) {
      const TailLevel& L = a.lv[l];
      const T* c = coeffs + L.c;
      if (l > top) cur[l] = nullptr;
      for (int k = 0; k < a.npre; ++k) {
        T* dst = other(l);
        tail_sweep<T>(c, cur[l], cur[l] == nullptr, rhs[l], dst, a.wpre[k], L, a);
        cur[l] = dst;
      }
      tail_restrict<T>(c, cur[l], cur[l] == nullptr, rhs[l], rhsw[l + 1], L, a.lv[l + 1], a, true);
    }
    coarsest();
    for (int l = last - 1; l >= top; --l) {
      const TailLevel& L = a.lv[l];
      const T* c = coeffs + L.c;
      if (cur[l] == nullptr) {
        tail_prolong<T>(cur[l + 1], nullptr, false, bufA[l], L, a.lv[l + 1]);
        cur[l] = bufA[l];
      } else {
        T* dst = other(l);
        tail_prolong<T>(cur[l + 1], cur[l], true, dst, L, a.lv[l + 1]);
        cur[l] = dst;
      }
      for (int k = 0; k < a.npost; ++k) {
        T* dst = other(l);
        tail_sweep<T>(c, cur[l], false, rhs[l], dst, a.wpost[k], L, a);
        cur[l] = dst;
      }
    }
  };
  if (a.fmg) {
    for (int l = 0; l < last; ++l)
      tail_restrict<T>(nullptr, nullptr, true, rhs[l], rhsw[l + 1], a.lv[l], a.lv[l + 1], a, false);
    if (last == 0) {
      coarsest();
    } else {
      // the coarsest problem, then every finer level: the interpolated solution of the level below as the start of one cycle
      coarsest();
      for (int l = last - 1; l >= 0; --l) {
        tail_prolong<T>(cur[l + 1], nullptr, false, bufA[l], a.lv[l], a.lv[l + 1]);
        cur[l] = bufA[l];
        vcycle(l);
      }
    }
  } else {
    cur[0] = xin;
    if (last == 0)
      coarsest();
    else
      vcycle(0);
  }
  if (cur[0] != xout) {
    for (int i = threadIdx.x; i < a.lv[0].size; i += kTailThreads) xout[i] = cur[0][i];
  }
}

template <typename T>
static int vcycle_tail(const T* coeffs, const int64_t* shapes, const int* halve, int nlev, int ndim, const T* xin,
                       const T* b, T* xout, T* work, int64_t work_len, const T* inv, int ninv, const T* wpre, int npre,
                       const T* wpost, int npost, int fmg, void* stream) {
  if (nlev < 1 || nlev > kTailMaxLev || ndim < 1 || ndim > 3 || !shapes || (nlev > 1 && !halve) || !coeffs || !b ||
      !xout || !work || !inv || npre < 0 || npre > 4 || npost < 0 || npost > 4 || (npre && !wpre) || (npost && !wpost)) {
    set_error("stencil_vcycle_tail: bad arguments (1..%d levels, ndim 1..3, at most 4 sweeps per side)", kTailMaxLev);
    return ODIL_E_INVAL;
  }
  if (xin == xout || b == xout) {
    set_error("stencil_vcycle_tail: xout must not alias xin or b");
    return ODIL_E_INVAL;
  }
  TailArgs<T> a;
  a.nlev = nlev, a.ndim = ndim;
  for (int d = 0; d < 3; ++d) {
    const int i = d - (3 - ndim);
    a.has[d] = i >= 0 ? 1 : 0;
    a.slot[d] = i >= 0 ? 1 + 2 * i : 0;
  }
  int64_t coff = 0, woff = 0;
  for (int l = 0; l < kTailMaxLev; ++l) {
    TailLevel& L = a.lv[l];
    L.size = 0, L.c = 0, L.x = L.t = L.b = 0;
    for (int d = 0; d < 3; ++d) L.n[d] = 1, L.halve[d] = 0, L.rn[d] = 1.0f;
    if (l >= nlev) continue;
    int64_t size = 1;
    for (int d = 0; d < 3; ++d) {
      const int i = d - (3 - ndim);
      if (i < 0) continue;
      const int64_t n = shapes[l * ndim + i];
      if (n < 1 || n > 4096) {
        set_error("stencil_vcycle_tail: extent %lld of level %d", (long long)n, l);
        return ODIL_E_INVAL;
      }
      L.n[d] = (int)n;
      L.rn[d] = 1.0f / (float)n;
      size *= n;
      if (l + 1 < nlev) {
        L.halve[d] = halve[l * ndim + i] != 0;
        const int64_t nc = shapes[(l + 1) * ndim + i];
        if ((L.halve[d] && (n % 2 || nc != n / 2)) || (!L.halve[d] && nc != n)) {
          set_error("stencil_vcycle_tail: level %d does not follow from level %d along axis %d", l + 1, l, i);
          return ODIL_E_INVAL;
        }
      }
    }
    if (size > (1 << 20)) {
      set_error("stencil_vcycle_tail: level %d has %lld cells (one workgroup walks the tail)", l, (long long)size);
      return ODIL_E_INVAL;
    }
    L.size = (int)size;
    L.c = coff;
    coff += (int64_t)(2 * ndim + 1) * size;
    L.x = woff, L.t = woff + size, L.b = woff + 2 * size;
    woff += 3 * size;
  }
  if (woff > work_len) {
    set_error("stencil_vcycle_tail: work array of %lld values, %lld needed", (long long)work_len, (long long)woff);
    return ODIL_E_INVAL;
  }
  if (ninv != a.lv[nlev - 1].size) {
    set_error("stencil_vcycle_tail: the coarsest level has %d unknowns, the inverse %d", a.lv[nlev - 1].size, ninv);
    return ODIL_E_INVAL;
  }
  a.ninv = ninv;
  a.npre = npre, a.npost = npost, a.fmg = fmg != 0;
  for (int k = 0; k < 4; ++k) {
    a.wpre[k] = k < npre ? wpre[k] : T(0);
    a.wpost[k] = k < npost ? wpost[k] : T(0);
  }
  hipLaunchKernelGGL((k_vcycle_tail<T>), dim3(1), dim3(kTailThreads), 0, (hipStream_t)stream, coeffs, xin, b, xout, work,
                     inv, a);
  return check_launch("k_vcycle_tail");
}

// ---- whole SOLVES of an ensemble: one workgroup per member ---------------------------------------------------------------
// B small systems A_b x_b = rhs_b (or Newton steps u_b <- u_b - d_b, A_b d_b = A_b u_b - rhs_b) in ONE launch.  Workgroup b
// walks member b's hierarchy from the FINEST level with the phases above (same functions, same order: member b's iterate
// after k cycles is that of k launches of k_vcycle_tail on its arrays, bit for bit), forms the residual's mean square
// before every cycle and stops on its own -- no host read-back inside the solve.  Members never communicate.
constexpr int kSolveMaxCycles = 1000;
// (k_vcycle_tail takes extents up to 4096; a 1-D member of 32768 cells is one row: tail_div is exact for i < 2^22)
constexpr int kSolveMaxExtent = 32768;
// (directions GCR keeps between restarts: their products with the new image are one register pair each)
constexpr int kKrylovMax = 8;

template <typename T>
struct SolveArgs {
  TailArgs<T> t;
  int64_t coeff_stride, x_stride, b_stride, work_stride, inv_stride, history_stride;
  int start, mode, maxcycles;
  double tol2;
};

// the sum of every thread's `s` in a fixed order (lanes of a wave by halving distances, then the 16 waves through LDS),
// returned to every thread; red: 16 doubles of LDS
__device__ __forceinline__ double solve_block_sum(double s, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = s;
  __syncthreads();
  double v[16];
#pragma unroll
  for (int w = 0; w < 16; ++w) v[w] = red[w];
#pragma unroll
  for (int half = 8; half > 0; half >>= 1)
#pragma unroll
    for (int w = 0; w < half; ++w) v[w] = v[w] + v[w + half];
  __syncthreads();  // (red is free for the next sum)
  return v[0];
}

// GCR of k_stencil_solve_batch: rho = rhs - A xk on the finest level, its mean square to every thread (xk complete and
// visible before the call)
template <typename T>
__device__ __forceinline__ double solve_true_residual(const T* __restrict__ c, const T* __restrict__ xk,
                                                      const T* __restrict__ rhs, T* __restrict__ rho, const TailLevel& L,
                                                      const TailArgs<T>& a, double* red, double rcells) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < L.size; i += kTailThreads) {
    int id[3];
    tail_decode(i, L, id);
    const T v = rhs[i] - tail_apply<T>(c, xk, false, L, a, i, id);
    rho[i] = v;
    acc += (double)v * (double)v;
  }
  return solve_block_sum(acc, red) * rcells;
}

// one decision of thread 0 (`why` of the others is ignored) to every thread
__device__ __forceinline__ int solve_publish(int why, int* shared) {
  if (threadIdx.x == 0) *shared = why;
  __syncthreads();
  const int all = *shared;
  __syncthreads();  // (read by all before thread 0 writes the next decision)
  return all;
}

// KRYLOV (odil_stencil_solve_krylov_batch): one more rule in the decision before cycle k -- a member whose cycles contract
// by less than 0.5 well above the tolerance (the hand-over rule of gmg.PoissonGMG.solve, on mean squares) goes on with
// GCR(krylov_m) around the same cycle (the algebra of PoissonGMG.solve_krylov), inside this launch.  A member that never
// meets the rule runs the instruction sequence of the plain kernel on the same buffers.  The (2 m + 2) vectors of GCR --
// the iterate xk, the residual rho, Z[m], Q[m] -- follow the levels' 3 x cells in `work`.  outcome: [B, 3].
template <typename T, bool KRYLOV>
__global__ __launch_bounds__(kTailThreads) void k_stencil_solve_batch(const T* __restrict__ coeffs_all, T* x_all,
                                                                      const T* __restrict__ b_all, T* work_all,
                                                                      const T* __restrict__ inv_all, double* history_all,
                                                                      int* outcome, SolveArgs<T> s, int krylov_m) {
  const TailArgs<T>& a = s.t;
  const int64_t member = blockIdx.x;
  const T* coeffs = coeffs_all + member * s.coeff_stride;
  T* xm = x_all + member * s.x_stride;
  const T* bm = b_all + member * s.b_stride;
  T* work = work_all + member * s.work_stride;
  const T* inv = inv_all + member * s.inv_stride;
  double* history = history_all + member * s.history_stride;
  const int last = a.nlev - 1;
  const TailLevel& L0 = a.lv[0];
  __shared__ double red[16];
  __shared__ int stop_shared;

  // Where the iterate of a level lives: two bits per level in ONE register of every thread, derived from the kernel's
  // arguments and workgroup-uniform control flow alone (no pointers in LDS that one thread writes while another reads).
  // 0: the zero vector (nothing stored), 1 / 2: the level's two buffers in `work`, 3: the member's x (finest level only)
  unsigned where = 0;
  auto get = [&](int l) -> int { return (int)((where >> (2 * l)) & 3u); };
  auto set = [&](int l, int v) { where = (where & ~(3u << (2 * l))) | ((unsigned)v << (2 * l)); };
  auto buf = [&](int l, int v) -> T* { return v == 1 ? work + a.lv[l].x : v == 2 ? work + a.lv[l].t : xm; };
  auto cur = [&](int l) -> const T* { return get(l) == 0 ? nullptr : buf(l, get(l)); };
  auto other = [&](int l) -> int { return get(l) == 1 ? 2 : 1; };
  // the right-hand side of the system solved: b, or in a Newton step r = A u - b (the finest level's third slot of `work`)
  T* rwork = work + L0.b;
  const T* rhs0 = s.mode ? rwork : bm;
  // (KRYLOV: the cycle that preconditions GCR takes the residual rho as its finest right-hand side; workgroup-uniform)
  const T* rhs_top = rhs0;
  auto rhs = [&](int l) -> const T* { return l == 0 ? (KRYLOV ? rhs_top : rhs0) : work + a.lv[l].b; };

  auto coarsest = [&]() {
    const TailLevel& L = a.lv[last];
    T* out = buf(last, 1);
    const T* b = rhs(last);
    for (int r = threadIdx.x; r < L.size; r += kTailThreads) {
      T acc = T(0);
      for (int j = 0; j < L.size; ++j) acc = acc + inv[(int64_t)r * L.size + j] * b[j];
      out[r] = acc;
    }
    __syncthreads();
    set(last, 1);
  };
  // (the body of k_vcycle_tail's vcycle)
  auto vcycle = [&](int top) {
    for (int l = top; l < last; ++l) {
      const TailLevel& L = a.lv[l];
      const T* c = coeffs + L.c;
      if (l > top) set(l, 0);
      for (int k = 0; k < a.npre; ++k) {
        const int dst = other(l);
        tail_sweep<T>(c, cur(l), get(l) == 0, rhs(l), buf(l, dst), a.wpre[k], L, a);
        set(l, dst);
      }
      tail_restrict<T>(c, cur(l), get(l) == 0, rhs(l), work + a.lv[l + 1].b, L, a.lv[l + 1], a, true);
    }
    coarsest();
    for (int l = last - 1; l >= top; --l) {
      const TailLevel& L = a.lv[l];
      const T* c = coeffs + L.c;
      if (get(l) == 0) {
        tail_prolong<T>(cur(l + 1), nullptr, false, buf(l, 1), L, a.lv[l + 1]);
        set(l, 1);
      } else {
        const int dst = other(l);
        tail_prolong<T>(cur(l + 1), cur(l), true, buf(l, dst), L, a.lv[l + 1]);
        set(l, dst);
      }
      for (int k = 0; k < a.npost; ++k) {
        const int dst = other(l);
        tail_sweep<T>(c, cur(l), false, rhs(l), buf(l, dst), a.wpost[k], L, a);
        set(l, dst);
      }
    }
  };

  // 1. Newton step: r = A u - b.  The terms of tail_apply in its order, but accumulated in DOUBLE and rounded once: u is
  // O(1) and r shrinks from step to step, so in float32 the roundings of the products c u (eps |c u|, not eps |r|) would
  // set the floor of the Newton iterate -- the residual of an iterative refinement is formed in the wider type.  (double:
  // the same operations as tail_apply)
  if (s.mode) {
    const T* c = coeffs + L0.c;
    const int stride[3] = {L0.n[1] * L0.n[2], L0.n[2], 1};
    for (int i = threadIdx.x; i < L0.size; i += kTailThreads) {
      int id[3];
      tail_decode(i, L0, id);
      double acc = (double)c[i] * (double)xm[i];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        if (!a.has[d]) continue;
        const int n = L0.n[d];
        const int im = id[d] == 0 ? i + (n - 1) * stride[d] : i - stride[d];
        const int ip = id[d] == n - 1 ? i - (n - 1) * stride[d] : i + stride[d];
        acc = acc + (double)c[(int64_t)a.slot[d] * L0.size + i] * (double)xm[im];
        acc = acc + (double)c[(int64_t)(a.slot[d] + 1) * L0.size + i] * (double)xm[ip];
      }
      rwork[i] = (T)(acc - (double)bm[i]);
    }
    __syncthreads();
  }
  // 2. mean(rhs^2)
  const double rcells = 1.0 / (double)L0.size;
  double sum = 0.0;
  for (int i = threadIdx.x; i < L0.size; i += kTailThreads) {
    const double v = (double)rhs0[i];
    sum += v * v;
  }
  const double bsq = solve_block_sum(sum, red) * rcells;
  if (threadIdx.x == 0) history[0] = bsq;
  // 3. the start iterate
  if (s.start == 2) {
    for (int l = 0; l < last; ++l)
      tail_restrict<T>(nullptr, nullptr, true, rhs(l), work + a.lv[l + 1].b, a.lv[l], a.lv[l + 1], a, false);
    coarsest();
    for (int l = last - 1; l >= 0; --l) {
      tail_prolong<T>(cur(l + 1), nullptr, false, buf(l, 1), a.lv[l], a.lv[l + 1]);
      set(l, 1);
      vcycle(l);
    }
  } else if (s.start == 1) {
    set(0, 3);
  }
  // 4. cycles until a stop rule fires (k <= maxcycles <= kSolveMaxCycles: the loop is bounded whatever the numbers do)
  int k = 0, reason = 1;
  double prev = bsq;
  int handover = -1;
  T* xk = nullptr;
  if constexpr (!KRYLOV) {
    // (this loop has a COPY in the branch below, which adds the hand-over rule and the GCR pass: a change to the residual
    // or to the stop rules here is made there too -- tests/test_newton_ensemble_krylov_gpu.py holds members that never
    // hand over to the same bits from both)
    for (; k <= s.maxcycles; ++k) {
      sum = 0.0;
      {
        const T* xc = cur(0);
        const bool zero = get(0) == 0;
        for (int i = threadIdx.x; i < L0.size; i += kTailThreads) {
          int id[3];
          tail_decode(i, L0, id);
          const double v = (double)(tail_apply<T>(coeffs + L0.c, xc, zero, L0, a, i, id) - rhs0[i]);
          sum += v * v;
        }
      }
      const double rsq = solve_block_sum(sum, red) * rcells;
      // the decision is taken ONCE and read by every thread after a barrier: every exit of this loop is workgroup-uniform
      if (threadIdx.x == 0) {
        history[1 + k] = rsq;
        int why = -1;
        if (!__builtin_isfinite(rsq) || !__builtin_isfinite(bsq)) why = 3;
        else if (rsq <= s.tol2 * bsq) why = 0;
        else if (k == s.maxcycles) why = 1;
        else if (k >= 3 && rsq >= (0.98 * 0.98) * prev) why = 2;
        stop_shared = why;
      }
      __syncthreads();
      const int why = stop_shared;
      __syncthreads();  // (read by all before thread 0 writes the next decision)
      if (why >= 0) {
        reason = why;
        break;
      }
      prev = rsq;
      if (last == 0)
        coarsest();
      else
        vcycle(0);
    }
  } else {
    // The same loop with the hand-over rule (the plain loop above stays as it was, and with it the registers of its
    // instantiation).  GCR(m) with one cycle from the zero start as the preconditioner takes over from the iterate of cycle
    // `handover` (PoissonGMG.solve_krylov); it shares this loop, so the cycle stands once in it.  Every branch below that
    // holds a barrier depends on `handover`, `have`, `k` and on decisions read from stop_shared alone: workgroup-uniform.
    // The sums of solve_block_sum are the same bits in every thread.
    int have = 0;
    const int cells = L0.size;
    xk = work + a.lv[last].b + a.lv[last].size;  // (behind the three arrays of every level)
    T* rho = xk + cells;
    T* zall = rho + cells;
    T* qall = zall + (int64_t)krylov_m * cells;
    for (; k <= s.maxcycles; ++k) {
      if (handover < 0) {
        sum = 0.0;
        {
          const T* xc = cur(0);
          const bool zero = get(0) == 0;
          for (int i = threadIdx.x; i < L0.size; i += kTailThreads) {
            int id[3];
            tail_decode(i, L0, id);
            const double v = (double)(tail_apply<T>(coeffs + L0.c, xc, zero, L0, a, i, id) - rhs0[i]);
            sum += v * v;
          }
        }
        const double rsq = solve_block_sum(sum, red) * rcells;
        // the decision is taken ONCE and read by every thread after a barrier: every exit of this loop is workgroup-uniform
        if (threadIdx.x == 0) {
          history[1 + k] = rsq;
          int why = -1;
          if (!__builtin_isfinite(rsq) || !__builtin_isfinite(bsq)) why = 3;
          else if (rsq <= s.tol2 * bsq) why = 0;
          else if (k == s.maxcycles) why = 1;
          else if (k >= 2 && rsq >= 0.25 * prev && rsq > 1e6 * s.tol2 * bsq) why = -2;  // (hand over to GCR)
          else if (k >= 3 && rsq >= (0.98 * 0.98) * prev) why = 2;
          stop_shared = why;
        }
        __syncthreads();
        const int why = stop_shared;
        __syncthreads();  // (read by all before thread 0 writes the next decision)
        if (why >= 0) {
          reason = why;
          break;
        }
        prev = rsq;
        if (why == -2) {
          // (the cycle rotates its own buffers underneath: the iterate gets a home of its own)
          handover = k;
          const T* x0 = cur(0);
          for (int i = threadIdx.x; i < cells; i += kTailThreads) xk[i] = x0 != nullptr ? x0[i] : T(0);
          __syncthreads();
          solve_true_residual<T>(coeffs + L0.c, xk, rhs0, rho, L0, a, red, rcells);
        }
      }
      if (handover >= 0) {  // e = M^-1 rho: the cycle from the zero start, rho its right-hand side
        rhs_top = rho;
        set(0, 0);
      }
      if (last == 0)
        coarsest();
      else
        vcycle(0);
      {
        if (handover >= 0) {
          // the rest of pass k of GCR; k < maxcycles here, and a pass that goes on raises k
          rhs_top = rhs0;
          const T* e = cur(0);
          T* z = zall + (int64_t)have * cells;
          T* q = qall + (int64_t)have * cells;
          // z = e, q = A z, and the products of q with the stored images in the same pass
          double dot[kKrylovMax];
#pragma unroll
          for (int j = 0; j < kKrylovMax; ++j) dot[j] = 0.0;
          for (int i = threadIdx.x; i < cells; i += kTailThreads) {
            int id[3];
            tail_decode(i, L0, id);
            const T qi = tail_apply<T>(coeffs + L0.c, e, false, L0, a, i, id);
            z[i] = e[i];
            q[i] = qi;
#pragma unroll
            for (int j = 0; j < kKrylovMax; ++j)
              if (j < have) dot[j] += (double)qall[(int64_t)j * cells + i] * (double)qi;
          }
#pragma unroll
          for (int j = 0; j < kKrylovMax; ++j)
            if (j < have) dot[j] = solve_block_sum(dot[j], red);
          // classical Gram-Schmidt: q -= sum beta_j Q_j, z -= sum beta_j Z_j; |q|^2
          double qq = 0.0;
          for (int i = threadIdx.x; i < cells; i += kTailThreads) {
            T qi = q[i], zi = z[i];
#pragma unroll
            for (int j = 0; j < kKrylovMax; ++j)
              if (j < have) {
                const T beta = (T)dot[j];
                qi = qi - beta * qall[(int64_t)j * cells + i];
                zi = zi - beta * zall[(int64_t)j * cells + i];
              }
            q[i] = qi;
            z[i] = zi;
            qq += (double)qi * (double)qi;
          }
          qq = solve_block_sum(qq, red);
          // breakdown: the preconditioner returned nothing useful
          if (solve_publish(!(qq > 0.0) || !__builtin_isfinite(qq) ? 4 : -1, &stop_shared) >= 0) {
            reason = 4;
            break;
          }
          const T scale = (T)(1.0 / sqrt(qq));
          double aq = 0.0;
          for (int i = threadIdx.x; i < cells; i += kTailThreads) {
            const T qi = q[i] * scale;
            q[i] = qi;
            z[i] = z[i] * scale;
            aq += (double)qi * (double)rho[i];
          }
          const T alpha = (T)solve_block_sum(aq, red);
          double rr = 0.0;
          for (int i = threadIdx.x; i < cells; i += kTailThreads) {
            xk[i] = xk[i] + alpha * z[i];
            const T v = rho[i] - alpha * q[i];
            rho[i] = v;
            rr += (double)v * (double)v;
          }
          double rsq = solve_block_sum(rr, red) * rcells;
          const int k1 = k + 1;
          int why = -1;
          if (threadIdx.x == 0) {
            history[1 + k1] = rsq;
            if (!__builtin_isfinite(rsq)) why = 3;
            else if (rsq <= s.tol2 * bsq) why = -3;  // (the recurrence says converged: the true residual decides)
            else if (k1 == s.maxcycles) why = 1;
          }
          why = solve_publish(why, &stop_shared);
          ++have;
          if (why == -3) {
            rsq = solve_true_residual<T>(coeffs + L0.c, xk, rhs0, rho, L0, a, red, rcells);
            why = -1;
            if (threadIdx.x == 0) {
              history[1 + k1] = rsq;
              if (!__builtin_isfinite(rsq)) why = 3;
              else if (rsq <= s.tol2 * bsq) why = 0;
              else if (k1 == s.maxcycles) why = 1;
            }
            why = solve_publish(why, &stop_shared);
            have = 0;  // (the recurrence had drifted: the directions go with it)
          }
          if (why >= 0) {
            reason = why;
            k = k1;
            break;
          }
          if (have == krylov_m) have = 0;  // restart: the stored directions are dropped
        }
      }
    }
  }
  if (threadIdx.x == 0) {
    if constexpr (KRYLOV) {
      outcome[3 * member] = k;
      outcome[3 * member + 1] = reason;
      outcome[3 * member + 2] = handover;
    } else {
      outcome[2 * member] = k;
      outcome[2 * member + 1] = reason;
    }
  }
  // 5. the result: x, or u - d
  const T* res = KRYLOV && handover >= 0 ? xk : cur(0);
  if (s.mode) {
    if (res != nullptr)
      for (int i = threadIdx.x; i < L0.size; i += kTailThreads) xm[i] = xm[i] - res[i];
  } else if (res != xm) {
    for (int i = threadIdx.x; i < L0.size; i += kTailThreads) xm[i] = res != nullptr ? res[i] : T(0);
  }
}

// the level table of `shapes` / `halve` (what vcycle_tail builds); false with the error set
template <typename T>
static bool solve_levels(const char* who, TailArgs<T>& a, const int64_t* shapes, const int* halve, int nlev, int ndim,
                         int64_t* ncoeff, int64_t* nwork) {
  a.nlev = nlev, a.ndim = ndim;
  for (int d = 0; d < 3; ++d) {
    const int i = d - (3 - ndim);
    a.has[d] = i >= 0 ? 1 : 0;
    a.slot[d] = i >= 0 ? 1 + 2 * i : 0;
  }
  int64_t coff = 0, woff = 0;
  for (int l = 0; l < kTailMaxLev; ++l) {
    TailLevel& L = a.lv[l];
    L.size = 0, L.c = 0, L.x = L.t = L.b = 0;
    for (int d = 0; d < 3; ++d) L.n[d] = 1, L.halve[d] = 0, L.rn[d] = 1.0f;
    if (l >= nlev) continue;
    int64_t size = 1;
    for (int d = 0; d < 3; ++d) {
      const int i = d - (3 - ndim);
      if (i < 0) continue;
      const int64_t n = shapes[l * ndim + i];
      if (n < 1 || n > kSolveMaxExtent) {
        set_error("%s: extent %lld of level %d", who, (long long)n, l);
        return false;
      }
      L.n[d] = (int)n;
      L.rn[d] = 1.0f / (float)n;
      size *= n;
      if (l + 1 < nlev) {
        L.halve[d] = halve[l * ndim + i] != 0;
        const int64_t nc = shapes[(l + 1) * ndim + i];
        if ((L.halve[d] && (n % 2 || nc != n / 2)) || (!L.halve[d] && nc != n)) {
          set_error("%s: level %d does not follow from level %d along axis %d", who, l + 1, l, i);
          return false;
        }
      }
    }
    if (size > (1 << 20)) {
      set_error("%s: level %d has %lld cells (one workgroup walks the hierarchy)", who, l, (long long)size);
      return false;
    }
    L.size = (int)size;
    L.c = coff;
    coff += (int64_t)(2 * ndim + 1) * size;
    L.x = woff, L.t = woff + size, L.b = woff + 2 * size;
    woff += 3 * size;
  }
  *ncoeff = coff, *nwork = woff;
  return true;
}

// KRYLOV: odil_stencil_solve_krylov_batch (krylov_m directions, the work of the (2 m + 2) vectors of GCR, outcome [B, 3])
template <typename T, bool KRYLOV = false>
static int stencil_solve_batch(const T* coeffs, int64_t coeff_stride, const int64_t* shapes, const int* halve, int nlev,
                               int ndim, int nbatch, T* x, int64_t x_stride, const T* b, int64_t b_stride, T* work,
                               int64_t work_stride, int64_t work_len, const T* inv, int64_t inv_stride, int ninv,
                               const T* wpre, int npre, const T* wpost, int npost, int start, int mode, int maxcycles,
                               double tol, double* history, int64_t history_stride, int* outcome, void* stream,
                               int krylov_m = 0) {
  const char* who = KRYLOV ? "stencil_solve_krylov_batch" : "stencil_solve_batch";
  if (KRYLOV && (krylov_m < 1 || krylov_m > kKrylovMax)) {
    set_error("%s: krylov_m %d (1..%d directions)", who, krylov_m, kKrylovMax);
    return ODIL_E_INVAL;
  }
  if (nlev < 1 || nlev > kTailMaxLev || ndim < 1 || ndim > 3 || npre < 0 || npre > 4 || npost < 0 || npost > 4) {
    set_error("%s: bad arguments (1..%d levels, ndim 1..3, at most 4 sweeps per side)", who, kTailMaxLev);
    return ODIL_E_INVAL;
  }
  if (!shapes || (nlev > 1 && !halve) || !coeffs || !x || !b || !work || !inv || !history || !outcome ||
      (npre && !wpre) || (npost && !wpost)) {
    set_error("%s: null pointer", who);
    return ODIL_E_INVAL;
  }
  if (nbatch < 1 || nbatch > 65535) {
    set_error("%s: %d members (1..65535: one workgroup each)", who, nbatch);
    return ODIL_E_INVAL;
  }
  if (start < 0 || start > 2 || mode < 0 || mode > 1 || (mode == 1 && start == 1)) {
    set_error("%s: start %d, mode %d (start 0..2, mode 0..1; a Newton step starts from 0 or 2)", who, start, mode);
    return ODIL_E_INVAL;
  }
  if (maxcycles < 0 || maxcycles > kSolveMaxCycles) {
    set_error("%s: maxcycles %d (0..%d)", who, maxcycles, kSolveMaxCycles);
    return ODIL_E_INVAL;
  }
  if (!(tol >= 0.0)) {
    set_error("%s: negative tol", who);
    return ODIL_E_INVAL;
  }
  if (x == b) {
    set_error("%s: x must not alias b", who);
    return ODIL_E_INVAL;
  }
  if (coeff_stride < 0 || x_stride < 0 || b_stride < 0 || work_stride < 0 || inv_stride < 0 || history_stride < 0) {
    set_error("%s: negative stride", who);
    return ODIL_E_INVAL;
  }
  SolveArgs<T> s;
  TailArgs<T>& a = s.t;
  int64_t ncoeff = 0, nwork = 0;
  if (!solve_levels<T>(who, a, shapes, halve, nlev, ndim, &ncoeff, &nwork)) return ODIL_E_INVAL;
  const int64_t cells = a.lv[0].size;
  if (KRYLOV) nwork += (int64_t)(2 * krylov_m + 2) * cells;  // (xk, rho, Z[m], Q[m] behind the levels' arrays)
  if (ninv != a.lv[nlev - 1].size) {
    set_error("%s: the coarsest level has %d unknowns, the inverse %d", who, a.lv[nlev - 1].size, ninv);
    return ODIL_E_INVAL;
  }
  if (x_stride < cells || b_stride < cells || work_stride < nwork) {
    set_error("%s: stride smaller than a member (x %lld, b %lld of %lld cells; work %lld of %lld values)", who,
              (long long)x_stride, (long long)b_stride, (long long)cells, (long long)work_stride, (long long)nwork);
    return ODIL_E_INVAL;
  }
  if (work_len < (int64_t)(nbatch - 1) * work_stride + nwork) {
    set_error("%s: work array of %lld values, %lld needed", who, (long long)work_len,
              (long long)((int64_t)(nbatch - 1) * work_stride + nwork));
    return ODIL_E_INVAL;
  }
  if ((coeff_stride != 0 && coeff_stride < ncoeff) || (inv_stride != 0 && inv_stride < (int64_t)ninv * ninv)) {
    set_error("%s: coeff_stride %lld / inv_stride %lld neither 0 (shared) nor a member's %lld / %lld values", who,
              (long long)coeff_stride, (long long)inv_stride, (long long)ncoeff, (long long)ninv * ninv);
    return ODIL_E_INVAL;
  }
  if (history_stride < (int64_t)maxcycles + 2) {
    set_error("%s: history_stride %lld smaller than maxcycles + 2 = %d", who, (long long)history_stride,
              maxcycles + 2);
    return ODIL_E_INVAL;
  }
  a.ninv = ninv;
  a.npre = npre, a.npost = npost, a.fmg = start == 2;
  for (int k = 0; k < 4; ++k) {
    a.wpre[k] = k < npre ? wpre[k] : T(0);
    a.wpost[k] = k < npost ? wpost[k] : T(0);
  }
  s.coeff_stride = coeff_stride, s.x_stride = x_stride, s.b_stride = b_stride, s.work_stride = work_stride;
  s.inv_stride = inv_stride, s.history_stride = history_stride;
  s.start = start, s.mode = mode, s.maxcycles = maxcycles, s.tol2 = tol * tol;
  hipLaunchKernelGGL((k_stencil_solve_batch<T, KRYLOV>), dim3(nbatch), dim3(kTailThreads), 0, (hipStream_t)stream, coeffs,
                     x, b, work, inv, history, outcome, s, krylov_m);
  return check_launch(KRYLOV ? "k_stencil_solve_krylov_batch" : "k_stencil_solve_batch");
}

}  // namespace odil

using namespace odil;

extern "C" {
int odil_stencil_vcycle_tail_f64(const double* coeffs, const int64_t* shapes, const int* halve, int nlev, int ndim,
                                 const double* xin, const double* b, double* xout, double* work, int64_t work_len,
                                 const double* inv, int ninv, const double* wpre, int npre, const double* wpost,
                                 int npost, int fmg, void* stream) {
  return vcycle_tail<double>(coeffs, shapes, halve, nlev, ndim, xin, b, xout, work, work_len, inv, ninv, wpre, npre,
                             wpost, npost, fmg, stream);
}
int odil_stencil_vcycle_tail_f32(const float* coeffs, const int64_t* shapes, const int* halve, int nlev, int ndim,
                                 const float* xin, const float* b, float* xout, float* work, int64_t work_len,
                                 const float* inv, int ninv, const float* wpre, int npre, const float* wpost, int npost,
                                 int fmg, void* stream) {
  return vcycle_tail<float>(coeffs, shapes, halve, nlev, ndim, xin, b, xout, work, work_len, inv, ninv, wpre, npre, wpost,
                            npost, fmg, stream);
}
int odil_stencil_solve_batch_f64(const double* coeffs, int64_t coeff_stride, const int64_t* shapes, const int* halve, int nlev,
                                 int ndim, int nbatch, double* x, int64_t x_stride, const double* b, int64_t b_stride,
                                 double* work, int64_t work_stride, int64_t work_len, const double* inv, int64_t inv_stride,
                                 int ninv, const double* wpre, int npre, const double* wpost, int npost, int start, int mode,
                                 int maxcycles, double tol, double* history, int64_t history_stride, int* outcome,
                                 void* stream) {
  return stencil_solve_batch<double>(coeffs, coeff_stride, shapes, halve, nlev, ndim, nbatch, x, x_stride, b, b_stride, work,
                                     work_stride, work_len, inv, inv_stride, ninv, wpre, npre, wpost, npost, start, mode,
                                     maxcycles, tol, history, history_stride, outcome, stream);
}
int odil_stencil_solve_batch_f32(const float* coeffs, int64_t coeff_stride, const int64_t* shapes, const int* halve, int nlev,
                                 int ndim, int nbatch, float* x, int64_t x_stride, const float* b, int64_t b_stride,
                                 float* work, int64_t work_stride, int64_t work_len, const float* inv, int64_t inv_stride,
                                 int ninv, const float* wpre, int npre, const float* wpost, int npost, int start, int mode,
                                 int maxcycles, float tol, double* history, int64_t history_stride, int* outcome,
                                 void* stream) {
  return stencil_solve_batch<float>(coeffs, coeff_stride, shapes, halve, nlev, ndim, nbatch, x, x_stride, b, b_stride, work,
                                    work_stride, work_len, inv, inv_stride, ninv, wpre, npre, wpost, npost, start, mode,
                                    maxcycles, (double)tol, history, history_stride, outcome, stream);
}
int64_t odil_stencil_solve_batch_work(const int64_t* shapes, int nlev, int ndim) {
  if (!shapes || nlev < 1 || nlev > kTailMaxLev || ndim < 1 || ndim > 3) return 0;
  int64_t total = 0;
  for (int l = 0; l < nlev; ++l) {
    int64_t size = 1;
    for (int i = 0; i < ndim; ++i) {
      const int64_t n = shapes[l * ndim + i];
      if (n < 1 || n > kSolveMaxExtent) return 0;
      size *= n;
    }
    if (size > (1 << 20)) return 0;
    total += 3 * size;
  }
  return total;
}
int odil_stencil_solve_krylov_batch_f64(const double* coeffs, int64_t coeff_stride, const int64_t* shapes, const int* halve,
                                        int nlev, int ndim, int nbatch, double* x, int64_t x_stride, const double* b,
                                        int64_t b_stride, double* work, int64_t work_stride, int64_t work_len,
                                        const double* inv, int64_t inv_stride, int ninv, const double* wpre, int npre,
                                        const double* wpost, int npost, int start, int mode, int maxcycles, double tol,
                                        double* history, int64_t history_stride, int* outcome, int krylov_m, void* stream) {
  return stencil_solve_batch<double, true>(coeffs, coeff_stride, shapes, halve, nlev, ndim, nbatch, x, x_stride, b, b_stride,
                                           work, work_stride, work_len, inv, inv_stride, ninv, wpre, npre, wpost, npost, start,
                                           mode, maxcycles, tol, history, history_stride, outcome, stream, krylov_m);
}
int odil_stencil_solve_krylov_batch_f32(const float* coeffs, int64_t coeff_stride, const int64_t* shapes, const int* halve,
                                        int nlev, int ndim, int nbatch, float* x, int64_t x_stride, const float* b,
                                        int64_t b_stride, float* work, int64_t work_stride, int64_t work_len,
                                        const float* inv, int64_t inv_stride, int ninv, const float* wpre, int npre,
                                        const float* wpost, int npost, int start, int mode, int maxcycles, float tol,
                                        double* history, int64_t history_stride, int* outcome, int krylov_m, void* stream) {
  return stencil_solve_batch<float, true>(coeffs, coeff_stride, shapes, halve, nlev, ndim, nbatch, x, x_stride, b, b_stride,
                                          work, work_stride, work_len, inv, inv_stride, ninv, wpre, npre, wpost, npost, start,
                                          mode, maxcycles, (double)tol, history, history_stride, outcome, stream, krylov_m);
}
int64_t odil_stencil_solve_krylov_batch_work(const int64_t* shapes, int nlev, int ndim, int krylov_m) {
  const int64_t levels = odil_stencil_solve_batch_work(shapes, nlev, ndim);
  if (!levels || krylov_m < 1 || krylov_m > kKrylovMax) return 0;
  int64_t cells = 1;
  for (int i = 0; i < ndim; ++i) cells *= shapes[i];
  return levels + (int64_t)(2 * krylov_m + 2) * cells;
}
}  // extern "C"
