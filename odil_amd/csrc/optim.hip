// Optimizer updates and flat-vector algebra of the ODIL hot path on gfx950
// (reference src/odil/optimizer.py:256-341; L-BFGS / CG building blocks).
// Pure HBM streaming: 16 B per lane, grid capped at 8 workgroups per CU, grid-stride.
#include "common.h"

namespace odil {

template <typename T>
struct Vec16;
template <>
struct Vec16<double> {
  static constexpr int N = 2;
  typedef double type __attribute__((ext_vector_type(2)));
};
template <>
struct Vec16<float> {
  static constexpr int N = 4;
  typedef float type __attribute__((ext_vector_type(4)));
};

template <typename T>
__device__ inline void adam_one(T& x, T& m, T& v, T g, T alpha, T omb1, T omb2, T eps) {
  // optimizer.py:316-318
  m = m + (g - m) * omb1;
  v = v + (g * g - v) * omb2;
  x = x - (m * alpha) / (sqrt(v) + eps);
}

// NT: the arrays are far larger than the caches (chosen by the launcher): streaming loads and stores, +4-6 % on
// top of the uncapped grid (6.3 / 6.5 TB/s for f32 / f64 at 1 G / 128 M elements).
template <typename T, bool NT>
__global__ __launch_bounds__(kBlock) void k_adam(T* __restrict__ x, T* __restrict__ m, T* __restrict__ v,
                                                const T* __restrict__ g, int64_t n, T alpha, T omb1, T omb2, T eps,
                                                int vec_ok, const T* __restrict__ alpha_dev) {
  if (alpha_dev) alpha = *alpha_dev;
  constexpr int V = Vec16<T>::N;
  typedef typename Vec16<T>::type VT;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  if (vec_ok) {
    const int64_t nv = n / V;
    for (int64_t i = tid; i < nv; i += nthreads) {
      VT xv, mv, vv, gv;
      if constexpr (NT) {
        xv = __builtin_nontemporal_load(reinterpret_cast<VT*>(x) + i);
        mv = __builtin_nontemporal_load(reinterpret_cast<VT*>(m) + i);
        vv = __builtin_nontemporal_load(reinterpret_cast<VT*>(v) + i);
        gv = __builtin_nontemporal_load(reinterpret_cast<const VT*>(g) + i);
      } else {
        xv = reinterpret_cast<VT*>(x)[i], mv = reinterpret_cast<VT*>(m)[i], vv = reinterpret_cast<VT*>(v)[i];
        gv = reinterpret_cast<const VT*>(g)[i];
      }
      T* xp = reinterpret_cast<T*>(&xv);
      T* mp = reinterpret_cast<T*>(&mv);
      T* vp = reinterpret_cast<T*>(&vv);
      const T* gp = reinterpret_cast<const T*>(&gv);
#pragma unroll
      for (int k = 0; k < V; ++k) adam_one<T>(xp[k], mp[k], vp[k], gp[k], alpha, omb1, omb2, eps);
      if constexpr (NT) {
        __builtin_nontemporal_store(xv, reinterpret_cast<VT*>(x) + i);
        __builtin_nontemporal_store(mv, reinterpret_cast<VT*>(m) + i);
        __builtin_nontemporal_store(vv, reinterpret_cast<VT*>(v) + i);
      } else {
        reinterpret_cast<VT*>(x)[i] = xv;
        reinterpret_cast<VT*>(m)[i] = mv;
        reinterpret_cast<VT*>(v)[i] = vv;
      }
    }
    for (int64_t i = nv * V + tid; i < n; i += nthreads) adam_one<T>(x[i], m[i], v[i], g[i], alpha, omb1, omb2, eps);
  } else {
    for (int64_t i = tid; i < n; i += nthreads) adam_one<T>(x[i], m[i], v[i], g[i], alpha, omb1, omb2, eps);
  }
}

static inline int aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
int adam_launch(T* x, T* m, T* v, const T* g, int64_t n, T alpha, T omb1, T omb2, T eps, hipStream_t stream,
                const T* alpha_dev);

template <typename T>
static int adam_step(T* x, T* m, T* v, const T* g, int64_t n, T alpha, T omb1, T omb2, T eps, const T* alpha_dev,
                     void* stream) {
  return adam_launch<T>(x, m, v, g, n, alpha, omb1, omb2, eps, (hipStream_t)stream, alpha_dev);
}

template <typename T>
int adam_launch(T* x, T* m, T* v, const T* g, int64_t n, T alpha, T omb1, T omb2, T eps, hipStream_t stream,
                const T* alpha_dev) {
  if (!x || !m || !v || !g || n < 0) {
    set_error("adam_step: null pointer or n < 0");
    return ODIL_E_INVAL;
  }
  if (n == 0) return 0;
  const int vec_ok = aligned16(x) && aligned16(m) && aligned16(v) && aligned16(g);
  if (7 * n * (int64_t)sizeof(T) > kStreamBytes)
    hipLaunchKernelGGL((k_adam<T, true>), dim3(grid_flat(n, kBlock * Vec16<T>::N)), dim3(kBlock), 0, stream, x, m, v, g,
                       n, alpha, omb1, omb2, eps, vec_ok, alpha_dev);
  else
    hipLaunchKernelGGL((k_adam<T, false>), dim3(grid_flat(n, kBlock * Vec16<T>::N)), dim3(kBlock), 0, stream, x, m, v, g,
                       n, alpha, omb1, omb2, eps, vec_ok, alpha_dev);
  return check_launch("k_adam");
}
template int adam_launch<double>(double*, double*, double*, const double*, int64_t, double, double, double, double,
                                 hipStream_t, const double*);
template int adam_launch<float>(float*, float*, float*, const float*, int64_t, float, float, float, float,
                                hipStream_t, const float*);

// Adam on a strided family of contiguous pieces: elements o * stride + offset + j, o < gridDim.y, j < count (the
// planes next to the slab interfaces of a ghost-extended array whose sharded axis is not the leading one: the rest
// of the array was updated by the launch that formed its gradient, these wait for the neighbour's contribution).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_adam_pieces(T* __restrict__ x, T* __restrict__ m, T* __restrict__ v,
                                                       const T* __restrict__ g, int64_t stride, int64_t offset,
                                                       int64_t count, T alpha, T omb1, T omb2, T eps, int vec_ok,
                                                       const T* __restrict__ alpha_dev) {
  if (alpha_dev) alpha = *alpha_dev;
  constexpr int V = Vec16<T>::N;
  typedef typename Vec16<T>::type VT;
  const int64_t base = (int64_t)blockIdx.y * stride + offset;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  if (vec_ok) {
    for (int64_t i = tid; i < count / V; i += nthreads) {
      const int64_t at = base + i * V;
      VT xv = *reinterpret_cast<VT*>(x + at), mv = *reinterpret_cast<VT*>(m + at), vv = *reinterpret_cast<VT*>(v + at);
      const VT gv = *reinterpret_cast<const VT*>(g + at);
      T* xp = reinterpret_cast<T*>(&xv);
      T* mp = reinterpret_cast<T*>(&mv);
      T* vp = reinterpret_cast<T*>(&vv);
      const T* gp = reinterpret_cast<const T*>(&gv);
#pragma unroll
      for (int k = 0; k < V; ++k) adam_one<T>(xp[k], mp[k], vp[k], gp[k], alpha, omb1, omb2, eps);
      *reinterpret_cast<VT*>(x + at) = xv;
      *reinterpret_cast<VT*>(m + at) = mv;
      *reinterpret_cast<VT*>(v + at) = vv;
    }
  } else {
    for (int64_t i = tid; i < count; i += nthreads)
      adam_one<T>(x[base + i], m[base + i], v[base + i], g[base + i], alpha, omb1, omb2, eps);
  }
}

template <typename T>
static int adam_pieces(T* x, T* m, T* v, const T* g, int64_t npieces, int64_t stride, int64_t offset, int64_t count,
                       T alpha, T omb1, T omb2, T eps, const T* alpha_dev, void* stream) {
  if (!x || !m || !v || !g || npieces < 0 || count < 0 || offset < 0 || npieces > 65535) {
    set_error("adam_step_pieces: null pointer, negative size or more than 65535 pieces");
    return ODIL_E_INVAL;
  }
  if (npieces == 0 || count == 0) return 0;
  constexpr int V = Vec16<T>::N;
  const int vec_ok = aligned16(x) && aligned16(m) && aligned16(v) && aligned16(g) && stride % V == 0 &&
                     offset % V == 0 && count % V == 0;
  const dim3 grid(grid_flat(count, kBlock * V), (unsigned)npieces);
  hipLaunchKernelGGL(k_adam_pieces<T>, grid, dim3(kBlock), 0, (hipStream_t)stream, x, m, v, g, stride, offset, count,
                     alpha, omb1, omb2, eps, vec_ok, alpha_dev);
  return check_launch("k_adam_pieces");
}

// Adam on the B members of [B, n] arrays, member b at b * stride of each array (members may be padded): the level-0
// update of an ensemble whose gradient is formed by a launch that does not apply it.  blockIdx.y counts the members;
// the arithmetic is adam_update of common.h with member b's step size alpha_dev[b * alpha_stride].
template <typename T>
__global__ __launch_bounds__(kBlock) void k_adam_batch(T* __restrict__ x, T* __restrict__ m, T* __restrict__ v,
                                                      const T* __restrict__ g, int64_t n, int64_t xs, int64_t ms,
                                                      int64_t vs, int64_t gs, AdamArgs<T> ad, int vec_ok) {
  constexpr int V = Vec16<T>::N;
  typedef typename Vec16<T>::type VT;
  const int64_t b = blockIdx.y;
  T* xb = x + b * xs;
  T* mb = m + b * ms;
  T* vb = v + b * vs;
  const T* gb = g + b * gs;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  int64_t done = 0;
  if (vec_ok) {
    const int64_t nv = n / V;
    for (int64_t i = tid; i < nv; i += nthreads) {
      VT xv = reinterpret_cast<VT*>(xb)[i], mv = reinterpret_cast<VT*>(mb)[i], vv = reinterpret_cast<VT*>(vb)[i];
      const VT gv = reinterpret_cast<const VT*>(gb)[i];
      T* xp = reinterpret_cast<T*>(&xv);
      T* mp = reinterpret_cast<T*>(&mv);
      T* vp = reinterpret_cast<T*>(&vv);
      const T* gp = reinterpret_cast<const T*>(&gv);
#pragma unroll
      for (int k = 0; k < V; ++k) adam_update<T>(xp[k], mp[k], vp[k], gp[k], ad, b);
      reinterpret_cast<VT*>(xb)[i] = xv;
      reinterpret_cast<VT*>(mb)[i] = mv;
      reinterpret_cast<VT*>(vb)[i] = vv;
    }
    done = nv * V;
  }
  for (int64_t i = done + tid; i < n; i += nthreads) adam_update<T>(xb[i], mb[i], vb[i], gb[i], ad, b);
}

template <typename T>
static int adam_step_batch(T* x, T* m, T* v, const T* g, int nbatch, int64_t n, int64_t xs, int64_t ms, int64_t vs,
                           int64_t gs, T omb1, T omb2, T eps, const T* alpha_dev, int64_t alpha_stride, void* stream) {
  if (!x || !m || !v || !g || !alpha_dev || n < 0 || alpha_stride < 0) {
    set_error("adam_step_batch: null pointer, n < 0 or a negative step-size stride");
    return ODIL_E_INVAL;
  }
  if (nbatch < 1 || nbatch > 65535) {
    set_error("adam_step_batch: %d members (1 ... 65535)", nbatch);
    return ODIL_E_INVAL;
  }
  if (nbatch > 1 && (xs < n || ms < n || vs < n || gs < n)) {
    set_error("adam_step_batch: a member stride is below the %lld elements of a member", (long long)n);
    return ODIL_E_INVAL;
  }
  if (n == 0) return 0;
  constexpr int V = Vec16<T>::N;
  const int vec_ok = aligned16(x) && aligned16(m) && aligned16(v) && aligned16(g) &&
                     (nbatch == 1 || (xs % V == 0 && ms % V == 0 && vs % V == 0 && gs % V == 0));
  AdamArgs<T> ad{nullptr, nullptr, nullptr, T(0), omb1, omb2, eps, alpha_dev, alpha_stride, 0};
  const dim3 grid(grid_flat(n, kBlock * V), (unsigned)nbatch);
  hipLaunchKernelGGL(k_adam_batch<T>, grid, dim3(kBlock), 0, (hipStream_t)stream, x, m, v, g, n, xs, ms, vs, gs, ad,
                     vec_ok);
  return check_launch("k_adam_batch");
}

// The Array unknowns of the B members of an ensemble of traced operators, P packed parameters per member: the
// generated k_loss_batch has left member b's parameter gradients, one per row of its partial sums, in pgrad[b, 0 .. npg);
// map[p] (member b: map[b * map_stride + p]) is the row of packed parameter p, any value outside 0 .. npg - 1 (-1 by
// convention) says that no grid kernel forms a gradient for it: g = 0.  Writes g [B, P] and, unless x is null, applies
// adam_one -- the update of k_adam, which a single run makes on these elements of its packed vector -- with member b's
// step size alpha_dev[b * alpha_stride].  A handful of elements per member: one thread each, blockIdx.y the member.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_adam_params_batch(T* __restrict__ x, T* __restrict__ m, T* __restrict__ v,
                                                             T* __restrict__ g, const T* __restrict__ pgrad,
                                                             const int* __restrict__ map, int64_t np, int npg,
                                                             int64_t pgrad_stride, int64_t map_stride, T omb1, T omb2,
                                                             T eps, const T* __restrict__ alpha_dev,
                                                             int64_t alpha_stride) {
  const int64_t b = blockIdx.y;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < np; p += nthreads) {
    const int row = map[b * map_stride + p];
    const T gp = (row >= 0 && row < npg) ? pgrad[b * pgrad_stride + row] : T(0);
    const int64_t at = b * np + p;
    g[at] = gp;
    if (x) adam_one<T>(x[at], m[at], v[at], gp, alpha_dev[b * alpha_stride], omb1, omb2, eps);
  }
}

template <typename T>
static int adam_step_params_batch(T* x, T* m, T* v, T* g, const T* pgrad, const int* map, int nbatch, int64_t np, int npg,
                                  int64_t pgrad_stride, int64_t map_stride, T omb1, T omb2, T eps, const T* alpha_dev,
                                  int64_t alpha_stride, void* stream) {
  const bool update = x || m || v;
  if (!g || !pgrad || !map || np < 0 || npg < 0 || (update && (!x || !m || !v || !alpha_dev)) || alpha_stride < 0) {
    set_error("adam_step_params_batch: null pointer, negative size or a negative step-size stride");
    return ODIL_E_INVAL;
  }
  if (nbatch < 1 || nbatch > 65535) {
    set_error("adam_step_params_batch: %d members (1 ... 65535)", nbatch);
    return ODIL_E_INVAL;
  }
  if (pgrad_stride < npg || (map_stride != 0 && map_stride < np)) {
    set_error("adam_step_params_batch: a row stride is below the length of its rows");
    return ODIL_E_INVAL;
  }
  if (np == 0) return 0;
  const dim3 grid(grid_flat(np, kBlock), (unsigned)nbatch);
  hipLaunchKernelGGL(k_adam_params_batch<T>, grid, dim3(kBlock), 0, (hipStream_t)stream, x, m, v, g, pgrad, map, np, npg,
                     pgrad_stride, map_stride, omb1, omb2, eps, alpha_dev, alpha_stride);
  return check_launch("k_adam_params_batch");
}

// The same launch for members whose operators also have outputs in PARAMETER space (a weight decay, a prior on an Array):
// the generated k_par_batch has left member b's part of the gradient in extra[b, p] -- ADDED to what stood there where a
// grid kernel forms a gradient too, SET where none does, as k_par adds to or sets the packed gradient of a single run.
// g = pgrad[row] + extra is the sum that single run forms (0 + extra where there is no row: exact), and extra is cleared
// behind the read, so that the next k_par_batch adds to zero again: no launch of its own for that.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_adam_params_extra_batch(T* __restrict__ x, T* __restrict__ m, T* __restrict__ v,
                                                                   T* __restrict__ g, const T* __restrict__ pgrad,
                                                                   T* __restrict__ extra, const int* __restrict__ map,
                                                                   int64_t np, int npg, int64_t pgrad_stride,
                                                                   int64_t map_stride, T omb1, T omb2, T eps,
                                                                   const T* __restrict__ alpha_dev, int64_t alpha_stride) {
  const int64_t b = blockIdx.y;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < np; p += nthreads) {
    const int row = map[b * map_stride + p];
    const int64_t at = b * np + p;
    const T gp = ((row >= 0 && row < npg) ? pgrad[b * pgrad_stride + row] : T(0)) + extra[at];
    extra[at] = T(0);
    g[at] = gp;
    if (x) adam_one<T>(x[at], m[at], v[at], gp, alpha_dev[b * alpha_stride], omb1, omb2, eps);
  }
}

template <typename T>
static int adam_step_params_extra_batch(T* x, T* m, T* v, T* g, const T* pgrad, T* extra, const int* map, int nbatch,
                                        int64_t np, int npg, int64_t pgrad_stride, int64_t map_stride, T omb1, T omb2,
                                        T eps, const T* alpha_dev, int64_t alpha_stride, void* stream) {
  const bool update = x || m || v;
  if (!g || !pgrad || !extra || !map || np < 0 || npg < 0 || (update && (!x || !m || !v || !alpha_dev)) ||
      alpha_stride < 0) {
    set_error("adam_step_params_extra_batch: null pointer, negative size or a negative step-size stride");
    return ODIL_E_INVAL;
  }
  if (nbatch < 1 || nbatch > 65535) {
    set_error("adam_step_params_extra_batch: %d members (1 ... 65535)", nbatch);
    return ODIL_E_INVAL;
  }
  if (pgrad_stride < npg || (map_stride != 0 && map_stride < np)) {
    set_error("adam_step_params_extra_batch: a row stride is below the length of its rows");
    return ODIL_E_INVAL;
  }
  if (np == 0) return 0;
  const dim3 grid(grid_flat(np, kBlock), (unsigned)nbatch);
  hipLaunchKernelGGL(k_adam_params_extra_batch<T>, grid, dim3(kBlock), 0, (hipStream_t)stream, x, m, v, g, pgrad, extra,
                     map, np, npg, pgrad_stride, map_stride, omb1, omb2, eps, alpha_dev, alpha_stride);
  return check_launch("k_adam_params_extra_batch");
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_axpy(T* __restrict__ y, const T* __restrict__ x, int64_t n, T a) {
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) y[i] = y[i] + a * x[i];
}

template <typename T>
static int axpy(T* y, const T* x, int64_t n, T a, void* stream) {
  if (!y || !x || n < 0) {
    set_error("axpy: null pointer or n < 0");
    return ODIL_E_INVAL;
  }
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_axpy<T>, dim3(grid_flat(n, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, y, x, n, a);
  return check_launch("k_axpy");
}

// Mixed-precision iterative refinement (gmg.py: float32 V-cycles inside a float64 residual loop): the two conversions
// with their scalings, one pass each.  narrow: y32 = (a / sqrt(*msq)) * x64 (the residual normalised by its own RMS, read
// from the device scalar the residual kernel just wrote: no host round trip); widen: y64 += (a * sqrt(*msq)) * x32.
__global__ __launch_bounds__(kBlock) void k_narrow_scale(const double* __restrict__ x, float* __restrict__ y, int64_t n,
                                                        double a, const double* __restrict__ msq) {
  const double s = msq ? a / sqrt(*msq > 0.0 ? *msq : 1.0) : a;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) y[i] = (float)(s * x[i]);
}
__global__ __launch_bounds__(kBlock) void k_widen_axpy(double* __restrict__ y, const float* __restrict__ x, int64_t n,
                                                      double a, const double* __restrict__ msq) {
  const double s = msq ? a * sqrt(*msq > 0.0 ? *msq : 1.0) : a;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) y[i] = y[i] + s * (double)x[i];
}

// y = a * (adev ? *adev : 1) * x   (cotangent of mean(x^2): 2/n * gout * x, core.py:1093)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_scale(const T* __restrict__ x, T* __restrict__ y, int64_t n, T a,
                                                 const T* __restrict__ adev) {
  const T f = adev ? a * adev[0] : a;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) y[i] = f * x[i];
}

template <typename T>
static int scale(const T* x, T* y, int64_t n, T a, const T* adev, void* stream) {
  if (!x || !y || n < 0) {
    set_error("scale: null pointer or n < 0");
    return ODIL_E_INVAL;
  }
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_scale<T>, dim3(grid_flat(n, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, x, y, n, a, adev);
  return check_launch("k_scale");
}

// y (+)= a (.) b
template <typename T>
__global__ __launch_bounds__(kBlock) void k_addcmul(T* __restrict__ y, const T* __restrict__ a, const T* __restrict__ b,
                                                   int64_t n, int accumulate) {
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) {
    const T v = a[i] * b[i];
    y[i] = accumulate ? y[i] + v : v;
  }
}

template <typename T>
static int addcmul(T* y, const T* a, const T* b, int64_t n, int accumulate, void* stream) {
  if (!y || !a || !b || n < 0) {
    set_error("addcmul: null pointer or n < 0");
    return ODIL_E_INVAL;
  }
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_addcmul<T>, dim3(grid_flat(n, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, y, a, b, n,
                     accumulate);
  return check_launch("k_addcmul");
}

// out[k] = <a_k, b>: blockIdx.y = k; contiguous chunk per workgroup; fixed order.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dots(const T* __restrict__ a, int64_t lda, const T* __restrict__ b,
                                                int64_t n, double* __restrict__ partials) {
  const T* ak = a + (int64_t)blockIdx.y * lda;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per;
  int64_t hi = lo + per;
  if (hi > n) hi = n;
  double local = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) local += (double)ak[i] * (double)b[i];
  const double total = block_sum(local);
  if (threadIdx.x == 0) partials[(int64_t)blockIdx.y * kDotPartials + blockIdx.x] = total;
}

template <typename T>
static int dots(const T* a, int64_t lda, int nvec, const T* b, int64_t n, double* partials, T* out, void* stream) {
  if (!a || !b || !partials || !out || n < 1 || nvec < 1 || nvec > 65535) {
    set_error("dots: null pointer, n < 1 or nvec=%d out of range", nvec);
    return ODIL_E_INVAL;
  }
  int grid = grid_for(n, kBlock * 8);
  if (grid > kDotPartials) grid = kDotPartials;
  hipLaunchKernelGGL(k_dots<T>, dim3(grid, nvec), dim3(kBlock), 0, (hipStream_t)stream, a, lda, b, n, partials);
  if (int e = check_launch("k_dots")) return e;
  return launch_final_reduce<T>(partials, grid, kDotPartials, nvec, 1.0, out, (hipStream_t)stream);
}

// out[j][k] = <a_k, b_j> for up to three right-hand vectors in ONE pass over the a_k (the L-BFGS
// history is by far the largest operand: S^T y, S^T s and S^T g cost one read of S instead of three).
// (the walk of one workgroup over its chunk of ONE a_k: shared by the single kernel and the ensemble form, which differ
// in where a_k and the three partial sums of the workgroup live)
template <typename T>
__device__ inline void dots3_unit(const T* __restrict__ ak, const T* __restrict__ b0, const T* __restrict__ b1,
                                  const T* __restrict__ b2, int64_t n, int vec_ok, double* __restrict__ p0,
                                  double* __restrict__ p1, double* __restrict__ p2) {
  constexpr int V = Vec16<T>::N;
  typedef typename Vec16<T>::type VT;
  // chunk boundaries on multiples of V so that every block reads whole 16 B packs
  const int64_t per = (((n + gridDim.x - 1) / gridDim.x) + V - 1) / V * V;
  const int64_t lo = (int64_t)blockIdx.x * per;
  int64_t hi = lo + per;
  if (hi > n) hi = n;
  double l0 = 0.0, l1 = 0.0, l2 = 0.0;
  int64_t i = lo;
  if (vec_ok) {
    // 16 B per lane and two packs in flight per stream: the history is read once at HBM speed, the
    // right-hand vectors come from the last-level cache
    const int64_t nv = lo < hi ? (hi - lo) / V : 0;
    for (int64_t p = threadIdx.x; p < nv; p += kBlock) {
      const VT av = *reinterpret_cast<const VT*>(ak + lo + p * V);
      const VT x0 = *reinterpret_cast<const VT*>(b0 + lo + p * V);
      VT x1 = x0, x2 = x0;
      if (b1) x1 = *reinterpret_cast<const VT*>(b1 + lo + p * V);
      if (b2) x2 = *reinterpret_cast<const VT*>(b2 + lo + p * V);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const double ad = (double)av[k];
        l0 += ad * (double)x0[k];
        l1 += ad * (double)x1[k];
        l2 += ad * (double)x2[k];
      }
    }
    i = lo + nv * V;
  }
  for (i += threadIdx.x; i < hi; i += kBlock) {
    const double av = (double)ak[i];
    l0 += av * (double)b0[i];
    if (b1) l1 += av * (double)b1[i];
    if (b2) l2 += av * (double)b2[i];
  }
  if (!b1) l1 = 0.0;
  if (!b2) l2 = 0.0;
  const double t0 = block_sum(l0), t1 = block_sum(l1), t2 = block_sum(l2);
  if (threadIdx.x == 0) {
    *p0 = t0;
    *p1 = t1;
    *p2 = t2;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_dots3(const T* __restrict__ a, int64_t lda, const T* __restrict__ b0,
                                                 const T* __restrict__ b1, const T* __restrict__ b2, int64_t n,
                                                 int nvec, double* __restrict__ partials, int vec_ok) {
  const int64_t base = (int64_t)blockIdx.y * kDotPartials + blockIdx.x;
  dots3_unit<T>(a + (int64_t)blockIdx.y * lda, b0, b1, b2, n, vec_ok, partials + base,
                partials + (int64_t)nvec * kDotPartials + base, partials + (int64_t)2 * nvec * kDotPartials + base);
}

// The same products with the right-hand vectors read ONCE: a workgroup owns a chunk of elements for
// all history vectors, keeps its part of b0 / b1 / b2 in registers and walks the history; per vector
// the three wave sums go to that wave's slot of an LDS table (fixed order, no atomics).  The kernel
// above re-reads b0 / b1 / b2 for every a_k -- four streams per history element, of which three come
// from the last-level cache: 2.2 TB/s on the history of L-BFGS (m = 50, 1.4 M unknowns).
constexpr int kDots3MaxVec = 128;  // S and Y of L-BFGS (m = 50) interleaved in one matrix
// (the unit of the single kernel and of the ensemble form: the partial sum of product j of vector k goes to
// partials[(j * jstride + k) * qstride + blockIdx.x])
template <typename T, int E>
__device__ inline void dots3_once_unit(const T* __restrict__ a, int64_t lda, const T* __restrict__ b0,
                                       const T* __restrict__ b1, const T* __restrict__ b2, int64_t n, int nvec,
                                       double* __restrict__ partials, int jstride, int qstride) {
  constexpr int V = Vec16<T>::N;
  constexpr int NP = E / V;  // 16 B packs per thread and chunk
  typedef typename Vec16<T>::type VT;
  __shared__ double acc[3][kBlock / 64][kDots3MaxVec];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = threadIdx.x; q < 3 * (kBlock / 64) * kDots3MaxVec; q += kBlock) (&acc[0][0][0])[q] = 0.0;
  __syncthreads();
  const int64_t chunk = (int64_t)kBlock * E;
  for (int64_t base = (int64_t)blockIdx.x * chunk; base < n; base += (int64_t)gridDim.x * chunk) {
    VT x0[NP], x1[NP], x2[NP];
    bool ok[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int64_t i = base + ((int64_t)p * kBlock + threadIdx.x) * V;
      ok[p] = i + V <= n;  // n is a multiple of V on this path
      const int64_t j = ok[p] ? i : 0;
      x0[p] = *reinterpret_cast<const VT*>(b0 + j);
      x1[p] = b1 ? *reinterpret_cast<const VT*>(b1 + j) : x0[p];
      x2[p] = b2 ? *reinterpret_cast<const VT*>(b2 + j) : x0[p];
    }
    for (int k = 0; k < nvec; ++k) {
      const T* ak = a + (int64_t)k * lda;
      VT av[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int64_t i = base + ((int64_t)p * kBlock + threadIdx.x) * V;
        av[p] = *reinterpret_cast<const VT*>(ak + (ok[p] ? i : 0));
      }
      double l0 = 0.0, l1 = 0.0, l2 = 0.0;
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const double ad = ok[p] ? (double)av[p][e] : 0.0;
          l0 += ad * (double)x0[p][e];
          l1 += ad * (double)x1[p][e];
          l2 += ad * (double)x2[p][e];
        }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        l0 += __shfl_down(l0, off, 64);
        l1 += __shfl_down(l1, off, 64);
        l2 += __shfl_down(l2, off, 64);
      }
      if (lane == 0) {
        acc[0][wave][k] += l0;
        acc[1][wave][k] += l1;
        acc[2][wave][k] += l2;
      }
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < 3 * nvec; q += kBlock) {
    const int j = q / nvec, k = q - j * nvec;
    double t = 0.0;
    for (int w = 0; w < kBlock / 64; ++w) t += acc[j][w][k];
    if ((j == 1 && !b1) || (j == 2 && !b2)) t = 0.0;
    partials[((int64_t)j * jstride + k) * qstride + blockIdx.x] = t;
  }
}

template <typename T, int E>
__global__ __launch_bounds__(kBlock) void k_dots3_once(const T* __restrict__ a, int64_t lda, const T* __restrict__ b0,
                                                      const T* __restrict__ b1, const T* __restrict__ b2, int64_t n,
                                                      int nvec, double* __restrict__ partials) {
  dots3_once_unit<T, E>(a, lda, b0, b1, b2, n, nvec, partials, nvec, kDotPartials);
}

template <typename T>
static int dots3(const T* a, int64_t lda, int nvec, const T* b0, const T* b1, const T* b2, int64_t n, double* partials,
                 T* out, void* stream) {
  if (!a || !b0 || !partials || !out || n < 1 || nvec < 1 || nvec > 65535) {
    set_error("dots3: null pointer, n < 1 or nvec=%d out of range", nvec);
    return ODIL_E_INVAL;
  }
  // every block ends with three block reductions: give it enough elements (64 per thread) to hide them
  int grid = grid_for(n, kBlock * 64);
  if (grid > kDotPartials) grid = kDotPartials;
  const int vec_ok = aligned16(a) && aligned16(b0) && (!b1 || aligned16(b1)) && (!b2 || aligned16(b2)) &&
                     (lda * (int64_t)sizeof(T)) % 16 == 0;
  if (vec_ok && nvec <= kDots3MaxVec && n % Vec16<T>::N == 0 && n >= (int64_t)kBlock * 64) {
    constexpr int E = 4 * Vec16<T>::N;  // four 16 B packs per thread, stream and chunk
    int chunks = grid_for(n, kBlock * E);
    if (chunks > kDotPartials) chunks = kDotPartials;
    hipLaunchKernelGGL((k_dots3_once<T, E>), dim3(chunks), dim3(kBlock), 0, (hipStream_t)stream, a, lda, b0, b1, b2, n,
                       nvec, partials);
    if (int e = check_launch("k_dots3_once")) return e;
    return launch_final_reduce<T>(partials, chunks, kDotPartials, 3 * nvec, 1.0, out, (hipStream_t)stream);
  }
  hipLaunchKernelGGL(k_dots3<T>, dim3(grid, nvec), dim3(kBlock), 0, (hipStream_t)stream, a, lda, b0, b1, b2, n, nvec,
                     partials, vec_ok);
  if (int e = check_launch("k_dots3")) return e;
  return launch_final_reduce<T>(partials, grid, kDotPartials, 3 * nvec, 1.0, out, (hipStream_t)stream);
}

template <typename T>
__device__ inline void lincomb_unit(T* __restrict__ y, T beta, const T* __restrict__ a, int64_t lda, int nvec,
                                    const T* __restrict__ coef, int64_t n) {
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) {
    T acc = beta == T(0) ? T(0) : beta * y[i];
    for (int k = 0; k < nvec; ++k) acc = acc + coef[k] * a[(int64_t)k * lda + i];
    y[i] = acc;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_lincomb(T* __restrict__ y, T beta, const T* __restrict__ a, int64_t lda,
                                                   int nvec, const T* __restrict__ coef, int64_t n) {
  lincomb_unit<T>(y, beta, a, lda, nvec, coef, n);
}

template <typename T>
static int lincomb(T* y, T beta, const T* a, int64_t lda, int nvec, const T* coef, int64_t n, void* stream) {
  if (!y || n < 0 || nvec < 0 || (nvec > 0 && (!a || !coef))) {
    set_error("lincomb: null pointer or negative size");
    return ODIL_E_INVAL;
  }
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_lincomb<T>, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, y, beta, a, lda,
                     nvec, coef, n);
  return check_launch("k_lincomb");
}

// One pass over the new gradient for everything the L-BFGS line search reads on the host after an
// evaluation: <g, d> (Wolfe test), <g, g> and max |g| (projected-gradient stopping test); fixed
// summation order.
// (units of the single kernels and of the ensemble forms: the partial sums of quantity q at partials[q * qstride + ...])
template <typename T>
__device__ inline void lbfgs_probe_unit(const T* __restrict__ g, const T* __restrict__ d, int64_t n,
                                        double* __restrict__ partials, int qstride) {
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per;
  int64_t hi = lo + per;
  if (hi > n) hi = n;
  double gd = 0.0, gg = 0.0, gm = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
    const double gi = (double)g[i];
    gd += gi * (double)d[i];
    gg += gi * gi;
    const double ai = fabs(gi);
    gm = ai > gm || ai != ai ? ai : gm;  // (a NaN stays visible: fmax would drop it and pass the stopping test)
  }
  const double t0 = block_sum(gd), t1 = block_sum(gg);
  __shared__ double wave_max[kBlock / 64];
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(gm, off, 64);
    gm = o > gm || o != o ? o : gm;
  }
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = gm;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; ++w) gm = wave_max[w] > gm || wave_max[w] != wave_max[w] ? wave_max[w] : gm;
    partials[blockIdx.x] = t0;
    partials[qstride + blockIdx.x] = t1;
    partials[2 * qstride + blockIdx.x] = gm;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_lbfgs_probe(const T* __restrict__ g, const T* __restrict__ d, int64_t n,
                                                       double* __restrict__ partials) {
  lbfgs_probe_unit<T>(g, d, n, partials, kDotPartials);
}

template <typename T>
__device__ inline void lbfgs_probe_final_unit(const double* __restrict__ partials, int count, int qstride,
                                              T* __restrict__ out) {
  double gd = 0.0, gg = 0.0, gm = 0.0;
  for (int i = threadIdx.x; i < count; i += kBlock) {
    gd += partials[i];
    gg += partials[qstride + i];
    const double pm = partials[2 * qstride + i];
    gm = pm > gm || pm != pm ? pm : gm;
  }
  const double t0 = block_sum(gd), t1 = block_sum(gg);
  __shared__ double wave_max[kBlock / 64];
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(gm, off, 64);
    gm = o > gm || o != o ? o : gm;
  }
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = gm;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; ++w) gm = wave_max[w] > gm || wave_max[w] != wave_max[w] ? wave_max[w] : gm;
    out[0] = (T)t0;
    out[1] = (T)t1;
    out[2] = (T)gm;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_lbfgs_probe_final(const double* __restrict__ partials, int count,
                                                             T* __restrict__ out) {
  lbfgs_probe_final_unit<T>(partials, count, kDotPartials, out);
}

template <typename T>
static int lbfgs_probe(const T* g, const T* d, int64_t n, double* partials, T* out, void* stream) {
  if (!g || !d || !partials || !out || n < 1) {
    set_error("lbfgs_probe: null pointer or n < 1");
    return ODIL_E_INVAL;
  }
  int grid = grid_for(n, kBlock * 8);
  if (grid > kDotPartials) grid = kDotPartials;
  hipLaunchKernelGGL(k_lbfgs_probe<T>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, g, d, n, partials);
  if (int e = check_launch("k_lbfgs_probe")) return e;
  hipLaunchKernelGGL(k_lbfgs_probe_final<T>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, partials, grid, out);
  return check_launch("k_lbfgs_probe_final");
}

// ---------------------------------------------------------------------------------------------------------------
// The same algebra for an ENSEMBLE in lock-step (include/odil_hip.h: odil_lbfgs_*_batch): member-major [B, n] vectors,
// a [B, rows, n] history.  blockIdx.y walks a list of members (a device array; null: all), every workgroup runs the
// unit of the single kernel on its member's arrays, the partial sums of member b live in row b of the workspace and
// are summed in the single launch's order.  Scalars and counts of a member: entry b of device arrays.
// ---------------------------------------------------------------------------------------------------------------
__device__ inline int member_of(const int32_t* __restrict__ members, int nbatch) {
  const int b = members ? members[blockIdx.y] : (int)blockIdx.y;
  return b >= 0 && b < nbatch ? b : -1;  // (a list entry that names no member: nothing is touched)
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_lbfgs_probe_batch(const T* __restrict__ g, int64_t gs,
                                                             const T* __restrict__ d, int64_t ds, int64_t n, int nbatch,
                                                             const int32_t* __restrict__ members,
                                                             double* __restrict__ partials, int64_t pstride) {
  const int b = member_of(members, nbatch);
  if (b < 0) return;
  lbfgs_probe_unit<T>(g + b * gs, d + b * ds, n, partials + b * pstride, (int)gridDim.x);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_lbfgs_probe_final_batch(const double* __restrict__ partials, int64_t pstride,
                                                                   int count, int nbatch,
                                                                   const int32_t* __restrict__ members,
                                                                   T* __restrict__ out, int64_t out_stride) {
  const int b = member_of(members, nbatch);
  if (b < 0) return;
  lbfgs_probe_final_unit<T>(partials + b * pstride, count, count, out + b * out_stride);
}

// blockIdx.z = k, the history vector; members with fewer vectors leave the launch at once
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dots3_batch(const T* __restrict__ a, int64_t as, int64_t lda,
                                                       const int32_t* __restrict__ counts, int max_count,
                                                       const T* __restrict__ b0, int64_t s0, const T* __restrict__ b1,
                                                       int64_t s1, const T* __restrict__ b2, int64_t s2, int64_t n,
                                                       int nbatch, const int32_t* __restrict__ members,
                                                       double* __restrict__ partials, int64_t pstride, int vec_ok) {
  const int b = member_of(members, nbatch);
  if (b < 0) return;
  const int count = counts ? min(counts[b], max_count) : max_count;
  const int k = blockIdx.z;
  if (k >= count) return;
  double* p = partials + b * pstride + (int64_t)k * gridDim.x + blockIdx.x;
  const int64_t jump = (int64_t)max_count * gridDim.x;
  dots3_unit<T>(a + b * as + (int64_t)k * lda, b0 + b * s0, b1 ? b1 + b * s1 : nullptr, b2 ? b2 + b * s2 : nullptr, n,
                vec_ok, p, p + jump, p + 2 * jump);
}

template <typename T, int E>
__global__ __launch_bounds__(kBlock) void k_dots3_once_batch(const T* __restrict__ a, int64_t as, int64_t lda,
                                                            const int32_t* __restrict__ counts, int max_count,
                                                            const T* __restrict__ b0, int64_t s0,
                                                            const T* __restrict__ b1, int64_t s1,
                                                            const T* __restrict__ b2, int64_t s2, int64_t n, int nbatch,
                                                            const int32_t* __restrict__ members,
                                                            double* __restrict__ partials, int64_t pstride) {
  const int b = member_of(members, nbatch);
  if (b < 0) return;
  const int count = counts ? min(counts[b], max_count) : max_count;
  if (count < 1) return;
  dots3_once_unit<T, E>(a + b * as, lda, b0 + b * s0, b1 ? b1 + b * s1 : nullptr, b2 ? b2 + b * s2 : nullptr, n, count,
                        partials + b * pstride, max_count, (int)gridDim.x);
}

// k_final_reduce for member blockIdx.y: blockIdx.x = j * max_count + k, `chunks` partial sums each
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dots3_final_batch(const double* __restrict__ partials, int64_t pstride,
                                                             int chunks, const int32_t* __restrict__ counts,
                                                             int max_count, int nbatch,
                                                             const int32_t* __restrict__ members, T* __restrict__ out,
                                                             int64_t out_stride, int64_t ldo) {
  const int b = member_of(members, nbatch);
  if (b < 0) return;
  const int count = counts ? min(counts[b], max_count) : max_count;
  const int j = blockIdx.x / max_count, k = blockIdx.x - j * max_count;
  if (k >= count) return;
  const double* p = partials + b * pstride + (int64_t)blockIdx.x * chunks;
  double local = 0.0;
  for (int i = threadIdx.x; i < chunks; i += kBlock) local += p[i];
  const double total = block_sum(local);
  if (threadIdx.x == 0) out[b * out_stride + j * ldo + k] = T(total / 1.0);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_lincomb_batch(T* __restrict__ y, int64_t ys, T beta, const T* __restrict__ a,
                                                         int64_t as, int64_t lda,
                                                         const int32_t* __restrict__ counts, int max_count,
                                                         const T* __restrict__ coef, int64_t cs, int64_t n, int nbatch,
                                                         const int32_t* __restrict__ members) {
  const int b = member_of(members, nbatch);
  if (b < 0) return;
  const int count = counts ? min(counts[b], max_count) : max_count;
  lincomb_unit<T>(y + b * ys, beta, a + b * as, lda, count < 0 ? 0 : count, coef + b * cs, n);
}

// out = y + alpha[b] * x (k_axpy), out = alpha[b] * x (k_scale), out = x; launch-uniform branches
template <typename T>
__global__ __launch_bounds__(kBlock) void k_axpy_batch(T* out, int64_t os, const T* y, int64_t ys, const T* x,
                                                      int64_t xs, const T* __restrict__ alpha, int64_t n, int nbatch,
                                                      const int32_t* __restrict__ members) {
  const int b = member_of(members, nbatch);
  if (b < 0) return;
  T* ob = out + b * os;
  const T* xb = x + b * xs;
  const T* yb = y ? y + b * ys : nullptr;
  const T a = alpha ? alpha[b] : T(1);
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) {
    if (yb)
      ob[i] = yb[i] + a * xb[i];
    else if (alpha)
      ob[i] = a * xb[i];
    else
      ob[i] = xb[i];
  }
}

// y = g - r as the single run forms it (r = -1 * r, then r = r + 1 * g), s = stp * d, and both into their history rows
template <typename T>
__global__ __launch_bounds__(kBlock) void k_lbfgs_pair_batch(const T* __restrict__ g, int64_t gs, T* __restrict__ r,
                                                            int64_t rs, T* __restrict__ d, int64_t ds,
                                                            T* __restrict__ w, int64_t ws, int64_t lda, int rows,
                                                            const T* __restrict__ stp, const int32_t* __restrict__ slot,
                                                            int64_t n, int nbatch,
                                                            const int32_t* __restrict__ members) {
  const int b = member_of(members, nbatch);
  if (b < 0) return;
  const T* gb = g + b * gs;
  T* rb = r + b * rs;
  T* db = d + b * ds;
  const T f = stp[b];
  const int sl = slot[b];
  const bool store = sl >= 0 && 2 * sl + 1 < rows;
  T* wsb = w + b * ws + (int64_t)(store ? 2 * sl : 0) * lda;
  T* wyb = wsb + lda;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) {
    const T neg = T(-1) * rb[i];
    const T yi = neg + T(1) * gb[i];
    const T si = f * db[i];
    rb[i] = yi;
    db[i] = si;
    if (store) {
      wsb[i] = si;
      wyb[i] = yi;
    }
  }
}

// What every batched launcher refuses first.  -> 0, with *rows_y = the grid's member extent (0: an empty list).
static int batch_list(const char* what, int64_t n, int nbatch, const int32_t* members, int nsel, int* rows_y) {
  if (n < 1) {
    set_error("%s: n=%lld < 1", what, (long long)n);
    return ODIL_E_INVAL;
  }
  if (nbatch < 1 || nbatch > 65535) {
    set_error("%s: %d members (1 ... 65535, one grid row each)", what, nbatch);
    return ODIL_E_INVAL;
  }
  if (members && (nsel < 0 || nsel > nbatch)) {
    set_error("%s: a list of %d members for %d members", what, nsel, nbatch);
    return ODIL_E_INVAL;
  }
  *rows_y = members ? nsel : nbatch;
  return 0;
}

static int batch_stride(const char* what, const char* name, int64_t stride, int64_t extent, int nbatch) {
  if (nbatch > 1 && stride < extent) {
    set_error("%s: member stride %lld of %s is below the %lld elements of a member", what, (long long)stride, name,
              (long long)extent);
    return ODIL_E_INVAL;
  }
  return 0;
}

// rows: history vectors a member HAS; max_count: how many of them a launch may use
static int batch_history(const char* what, int64_t a_stride, int64_t lda, int rows, int max_count, int least, int64_t n,
                         int nbatch) {
  if (rows < 1 || max_count < least || max_count > rows) {
    set_error("%s: count %d outside %d ... %d, the history vectors of a member", what, max_count, least, rows);
    return ODIL_E_INVAL;
  }
  if (lda < n) {
    set_error("%s: lda=%lld is below n=%lld", what, (long long)lda, (long long)n);
    return ODIL_E_INVAL;
  }
  return batch_stride(what, "the history", a_stride, (int64_t)(rows - 1) * lda + n, nbatch);
}

static int dots3_chunks(int64_t n, int elem_size, bool once) {
  const int grid = once ? grid_for(n, kBlock * 4 * (16 / elem_size)) : grid_for(n, kBlock * 64);
  return grid > kDotPartials ? kDotPartials : grid;
}

static int probe_chunks(int64_t n) {
  const int grid = grid_for(n, kBlock * 8);
  return grid > kDotPartials ? kDotPartials : grid;
}

static int64_t batch_partials(int64_t n, int max_count, int elem_size) {
  int chunks = dots3_chunks(n, elem_size, true);
  if (dots3_chunks(n, elem_size, false) > chunks) chunks = dots3_chunks(n, elem_size, false);
  if (probe_chunks(n) > chunks) chunks = probe_chunks(n);
  return (int64_t)3 * (max_count < 1 ? 1 : max_count) * chunks;
}

static int batch_workspace(const char* what, const double* partials, int64_t partials_stride, int64_t partials_len,
                           int64_t need, int nbatch) {
  if (!partials || partials_stride < need || partials_len < (int64_t)(nbatch - 1) * partials_stride + need) {
    set_error("%s: partials workspace too short: %lld doubles in rows of %lld, %d members need %lld each", what,
              (long long)partials_len, (long long)partials_stride, nbatch, (long long)need);
    return ODIL_E_INVAL;
  }
  return 0;
}

template <typename T>
static int lbfgs_probe_batch(const T* g, int64_t g_stride, const T* d, int64_t d_stride, int64_t n, int nbatch,
                             const int32_t* members, int nsel, double* partials, int64_t partials_stride,
                             int64_t partials_len, T* out, int64_t out_stride, void* stream) {
  static const char* what = "lbfgs_probe_batch";
  if (!g || !d || !partials || !out) {
    set_error("%s: null pointer", what);
    return ODIL_E_INVAL;
  }
  int ny;
  if (int e = batch_list(what, n, nbatch, members, nsel, &ny)) return e;
  if (int e = batch_stride(what, "g", g_stride, n, nbatch)) return e;
  if (int e = batch_stride(what, "d", d_stride, n, nbatch)) return e;
  if (int e = batch_stride(what, "out", out_stride, 3, nbatch)) return e;
  const int grid = probe_chunks(n);
  if (int e = batch_workspace(what, partials, partials_stride, partials_len, (int64_t)3 * grid, nbatch)) return e;
  if (ny == 0) return 0;
  hipLaunchKernelGGL(k_lbfgs_probe_batch<T>, dim3(grid, ny), dim3(kBlock), 0, (hipStream_t)stream, g, g_stride, d,
                     d_stride, n, nbatch, members, partials, partials_stride);
  if (int e = check_launch("k_lbfgs_probe_batch")) return e;
  hipLaunchKernelGGL(k_lbfgs_probe_final_batch<T>, dim3(1, ny), dim3(kBlock), 0, (hipStream_t)stream, partials,
                     partials_stride, grid, nbatch, members, out, out_stride);
  return check_launch("k_lbfgs_probe_final_batch");
}

// vec_ok of `dots3` for member b's own arrays
template <typename T>
static int dots3_member_vec_ok(const T* a, int64_t as, int64_t lda, const T* b0, int64_t s0, const T* b1, int64_t s1,
                               const T* b2, int64_t s2, int64_t b) {
  return aligned16(a + b * as) && aligned16(b0 + b * s0) && (!b1 || aligned16(b1 + b * s1)) &&
         (!b2 || aligned16(b2 + b * s2)) && (lda * (int64_t)sizeof(T)) % 16 == 0;
}

template <typename T>
static int lbfgs_dots3_batch(const T* a, int64_t a_stride, int64_t lda, int rows, const int32_t* counts, int max_count,
                             const T* b0, int64_t b0_stride, const T* b1, int64_t b1_stride, const T* b2,
                             int64_t b2_stride, int64_t n, int nbatch, const int32_t* members, int nsel,
                             double* partials, int64_t partials_stride, int64_t partials_len, T* out,
                             int64_t out_stride, int64_t ldo, void* stream) {
  static const char* what = "lbfgs_dots3_batch";
  if (!a || !b0 || !partials || !out) {
    set_error("%s: null pointer", what);
    return ODIL_E_INVAL;
  }
  int ny;
  if (int e = batch_list(what, n, nbatch, members, nsel, &ny)) return e;
  if (int e = batch_history(what, a_stride, lda, rows, max_count, 1, n, nbatch)) return e;
  if (int e = batch_stride(what, "b0", b0_stride, n, nbatch)) return e;
  if (b1)
    if (int e = batch_stride(what, "b1", b1_stride, n, nbatch)) return e;
  if (b2)
    if (int e = batch_stride(what, "b2", b2_stride, n, nbatch)) return e;
  if (ldo < max_count) {
    set_error("%s: ldo=%lld is below the count %d", what, (long long)ldo, max_count);
    return ODIL_E_INVAL;
  }
  if (int e = batch_stride(what, "out", out_stride, 2 * ldo + max_count, nbatch)) return e;
  // the choice of kernel a member's single call makes: one answer for the launch, or none
  const int vec_ok = dots3_member_vec_ok<T>(a, a_stride, lda, b0, b0_stride, b1, b1_stride, b2, b2_stride, 0);
  for (int b = 1; b < nbatch; ++b)
    if (dots3_member_vec_ok<T>(a, a_stride, lda, b0, b0_stride, b1, b1_stride, b2, b2_stride, b) != vec_ok) {
      set_error("%s: member %d is%s aligned to 16 bytes where member 0 is%s (member strides off the 16-byte grid): the "
                "members' single calls would not run the same kernel", what, b, vec_ok ? " not" : "", vec_ok ? "" : " not");
      return ODIL_E_INVAL;
    }
  const bool once_sized = vec_ok && n % Vec16<T>::N == 0 && n >= (int64_t)kBlock * 64;
  if (once_sized && max_count > kDots3MaxVec) {
    set_error("%s: count %d above %d at n=%lld: the kernel a member's single call runs would depend on its own count", what,
              max_count, kDots3MaxVec, (long long)n);
    return ODIL_E_INVAL;
  }
  const int chunks = dots3_chunks(n, (int)sizeof(T), once_sized);
  if (int e = batch_workspace(what, partials, partials_stride, partials_len, (int64_t)3 * max_count * chunks, nbatch))
    return e;
  if (ny == 0) return 0;
  if (once_sized) {
    constexpr int E = 4 * Vec16<T>::N;
    hipLaunchKernelGGL((k_dots3_once_batch<T, E>), dim3(chunks, ny), dim3(kBlock), 0, (hipStream_t)stream, a, a_stride,
                       lda, counts, max_count, b0, b0_stride, b1, b1_stride, b2, b2_stride, n, nbatch, members, partials,
                       partials_stride);
    if (int e = check_launch("k_dots3_once_batch")) return e;
  } else {
    hipLaunchKernelGGL(k_dots3_batch<T>, dim3(chunks, ny, max_count), dim3(kBlock), 0, (hipStream_t)stream, a, a_stride,
                       lda, counts, max_count, b0, b0_stride, b1, b1_stride, b2, b2_stride, n, nbatch, members, partials,
                       partials_stride, vec_ok);
    if (int e = check_launch("k_dots3_batch")) return e;
  }
  hipLaunchKernelGGL(k_dots3_final_batch<T>, dim3(3 * max_count, ny), dim3(kBlock), 0, (hipStream_t)stream, partials,
                     partials_stride, chunks, counts, max_count, nbatch, members, out, out_stride, ldo);
  return check_launch("k_dots3_final_batch");
}

template <typename T>
static int lbfgs_lincomb_batch(T* y, int64_t y_stride, T beta, const T* a, int64_t a_stride, int64_t lda, int rows,
                               const int32_t* counts, int max_count, const T* coef, int64_t coef_stride, int64_t n,
                               int nbatch, const int32_t* members, int nsel, void* stream) {
  static const char* what = "lbfgs_lincomb_batch";
  if (!y || !a || !coef) {
    set_error("%s: null pointer", what);
    return ODIL_E_INVAL;
  }
  int ny;
  if (int e = batch_list(what, n, nbatch, members, nsel, &ny)) return e;
  if (int e = batch_history(what, a_stride, lda, rows, max_count, 0, n, nbatch)) return e;
  if (int e = batch_stride(what, "y", y_stride, n, nbatch)) return e;
  if (int e = batch_stride(what, "coef", coef_stride, max_count, nbatch)) return e;
  if (ny == 0) return 0;
  hipLaunchKernelGGL(k_lincomb_batch<T>, dim3(grid_for(n, kBlock), ny), dim3(kBlock), 0, (hipStream_t)stream, y,
                     y_stride, beta, a, a_stride, lda, counts, max_count, coef, coef_stride, n, nbatch, members);
  return check_launch("k_lincomb_batch");
}

template <typename T>
static int lbfgs_axpy_batch(T* out, int64_t out_stride, const T* y, int64_t y_stride, const T* x, int64_t x_stride,
                            const T* alpha, int64_t n, int nbatch, const int32_t* members, int nsel, void* stream) {
  static const char* what = "lbfgs_axpy_batch";
  if (!out || !x || (y && !alpha)) {
    set_error("%s: null pointer", what);
    return ODIL_E_INVAL;
  }
  int ny;
  if (int e = batch_list(what, n, nbatch, members, nsel, &ny)) return e;
  if (int e = batch_stride(what, "out", out_stride, n, nbatch)) return e;
  if (int e = batch_stride(what, "x", x_stride, n, nbatch)) return e;
  if (y)
    if (int e = batch_stride(what, "y", y_stride, n, nbatch)) return e;
  if (ny == 0) return 0;
  int grid = grid_flat(n, kBlock * 2);
  if (grid > 65535 * 16) grid = 65535 * 16;
  hipLaunchKernelGGL(k_axpy_batch<T>, dim3(grid, ny), dim3(kBlock), 0, (hipStream_t)stream, out, out_stride, y,
                     y_stride, x, x_stride, alpha, n, nbatch, members);
  return check_launch("k_axpy_batch");
}

template <typename T>
static int lbfgs_pair_batch(const T* g, int64_t g_stride, T* r, int64_t r_stride, T* d, int64_t d_stride, T* w,
                            int64_t w_stride, int64_t lda, int rows, const T* stp, const int32_t* slot, int64_t n,
                            int nbatch, const int32_t* members, int nsel, void* stream) {
  static const char* what = "lbfgs_pair_batch";
  if (!g || !r || !d || !w || !stp || !slot) {
    set_error("%s: null pointer", what);
    return ODIL_E_INVAL;
  }
  int ny;
  if (int e = batch_list(what, n, nbatch, members, nsel, &ny)) return e;
  if (rows < 2 || rows % 2) {
    set_error("%s: %d history vectors (an even number: s and y interleaved)", what, rows);
    return ODIL_E_INVAL;
  }
  if (int e = batch_history(what, w_stride, lda, rows, rows, 1, n, nbatch)) return e;
  if (int e = batch_stride(what, "g", g_stride, n, nbatch)) return e;
  if (int e = batch_stride(what, "r", r_stride, n, nbatch)) return e;
  if (int e = batch_stride(what, "d", d_stride, n, nbatch)) return e;
  if (ny == 0) return 0;
  int grid = grid_flat(n, kBlock * 2);
  if (grid > 65535 * 16) grid = 65535 * 16;
  hipLaunchKernelGGL(k_lbfgs_pair_batch<T>, dim3(grid, ny), dim3(kBlock), 0, (hipStream_t)stream, g, g_stride, r,
                     r_stride, d, d_stride, w, w_stride, lda, rows, stp, slot, n, nbatch, members);
  return check_launch("k_lbfgs_pair_batch");
}

}  // namespace odil

using namespace odil;

extern "C" {
int odil_adam_step_f64(double* x, double* m, double* v, const double* g, int64_t n, double alpha,
                       double one_minus_b1, double one_minus_b2, double eps, const double* alpha_dev, void* stream) {
  return adam_step<double>(x, m, v, g, n, alpha, one_minus_b1, one_minus_b2, eps, alpha_dev, stream);
}
int odil_adam_step_f32(float* x, float* m, float* v, const float* g, int64_t n, float alpha, float one_minus_b1,
                       float one_minus_b2, float eps, const float* alpha_dev, void* stream) {
  return adam_step<float>(x, m, v, g, n, alpha, one_minus_b1, one_minus_b2, eps, alpha_dev, stream);
}
int odil_adam_step_pieces_f64(double* x, double* m, double* v, const double* g, int64_t npieces, int64_t stride,
                              int64_t offset, int64_t count, double alpha, double one_minus_b1, double one_minus_b2,
                              double eps, const double* alpha_dev, void* stream) {
  return adam_pieces<double>(x, m, v, g, npieces, stride, offset, count, alpha, one_minus_b1, one_minus_b2, eps, alpha_dev,
                             stream);
}
int odil_adam_step_pieces_f32(float* x, float* m, float* v, const float* g, int64_t npieces, int64_t stride,
                              int64_t offset, int64_t count, float alpha, float one_minus_b1, float one_minus_b2,
                              float eps, const float* alpha_dev, void* stream) {
  return adam_pieces<float>(x, m, v, g, npieces, stride, offset, count, alpha, one_minus_b1, one_minus_b2, eps, alpha_dev,
                            stream);
}
int odil_adam_step_batch_f64(double* x, double* m, double* v, const double* g, int nbatch, int64_t n, int64_t x_stride,
                             int64_t m_stride, int64_t v_stride, int64_t g_stride, double one_minus_b1,
                             double one_minus_b2, double eps, const double* alpha_dev, int64_t alpha_stride,
                             void* stream) {
  return adam_step_batch<double>(x, m, v, g, nbatch, n, x_stride, m_stride, v_stride, g_stride, one_minus_b1,
                                 one_minus_b2, eps, alpha_dev, alpha_stride, stream);
}
int odil_adam_step_batch_f32(float* x, float* m, float* v, const float* g, int nbatch, int64_t n, int64_t x_stride,
                             int64_t m_stride, int64_t v_stride, int64_t g_stride, float one_minus_b1,
                             float one_minus_b2, float eps, const float* alpha_dev, int64_t alpha_stride, void* stream) {
  return adam_step_batch<float>(x, m, v, g, nbatch, n, x_stride, m_stride, v_stride, g_stride, one_minus_b1,
                                one_minus_b2, eps, alpha_dev, alpha_stride, stream);
}
int odil_adam_step_params_batch_f64(double* x, double* m, double* v, double* g, const double* pgrad, const int* map,
                                    int nbatch, int64_t np, int npg, int64_t pgrad_stride, int64_t map_stride,
                                    double one_minus_b1, double one_minus_b2, double eps, const double* alpha_dev,
                                    int64_t alpha_stride, void* stream) {
  return adam_step_params_batch<double>(x, m, v, g, pgrad, map, nbatch, np, npg, pgrad_stride, map_stride, one_minus_b1,
                                        one_minus_b2, eps, alpha_dev, alpha_stride, stream);
}
int odil_adam_step_params_batch_f32(float* x, float* m, float* v, float* g, const float* pgrad, const int* map, int nbatch,
                                    int64_t np, int npg, int64_t pgrad_stride, int64_t map_stride, float one_minus_b1,
                                    float one_minus_b2, float eps, const float* alpha_dev, int64_t alpha_stride,
                                    void* stream) {
  return adam_step_params_batch<float>(x, m, v, g, pgrad, map, nbatch, np, npg, pgrad_stride, map_stride, one_minus_b1,
                                       one_minus_b2, eps, alpha_dev, alpha_stride, stream);
}
int odil_adam_step_params_extra_batch_f64(double* x, double* m, double* v, double* g, const double* pgrad, double* extra,
                                          const int* map, int nbatch, int64_t np, int npg, int64_t pgrad_stride,
                                          int64_t map_stride, double one_minus_b1, double one_minus_b2, double eps,
                                          const double* alpha_dev, int64_t alpha_stride, void* stream) {
  return adam_step_params_extra_batch<double>(x, m, v, g, pgrad, extra, map, nbatch, np, npg, pgrad_stride, map_stride,
                                              one_minus_b1, one_minus_b2, eps, alpha_dev, alpha_stride, stream);
}
int odil_adam_step_params_extra_batch_f32(float* x, float* m, float* v, float* g, const float* pgrad, float* extra,
                                          const int* map, int nbatch, int64_t np, int npg, int64_t pgrad_stride,
                                          int64_t map_stride, float one_minus_b1, float one_minus_b2, float eps,
                                          const float* alpha_dev, int64_t alpha_stride, void* stream) {
  return adam_step_params_extra_batch<float>(x, m, v, g, pgrad, extra, map, nbatch, np, npg, pgrad_stride, map_stride,
                                             one_minus_b1, one_minus_b2, eps, alpha_dev, alpha_stride, stream);
}
int odil_narrow_scale(const double* x, float* y, int64_t n, double a, const double* msq, void* stream) {
  if (!x || !y || n < 0) {
    set_error("narrow_scale: null pointer or n < 0");
    return ODIL_E_INVAL;
  }
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_narrow_scale, dim3(grid_flat(n, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, x, y, n, a, msq);
  return check_launch("k_narrow_scale");
}
int odil_widen_axpy(double* y, const float* x, int64_t n, double a, const double* msq, void* stream) {
  if (!x || !y || n < 0) {
    set_error("widen_axpy: null pointer or n < 0");
    return ODIL_E_INVAL;
  }
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_widen_axpy, dim3(grid_flat(n, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, y, x, n, a, msq);
  return check_launch("k_widen_axpy");
}
int odil_axpy_f64(double* y, const double* x, int64_t n, double a, void* stream) {
  return axpy<double>(y, x, n, a, stream);
}
int odil_axpy_f32(float* y, const float* x, int64_t n, float a, void* stream) {
  return axpy<float>(y, x, n, a, stream);
}
int odil_scale_f64(const double* x, double* y, int64_t n, double a, const double* adev, void* stream) {
  return scale<double>(x, y, n, a, adev, stream);
}
int odil_scale_f32(const float* x, float* y, int64_t n, float a, const float* adev, void* stream) {
  return scale<float>(x, y, n, a, adev, stream);
}
int odil_addcmul_f64(double* y, const double* a, const double* b, int64_t n, int accumulate, void* stream) {
  return addcmul<double>(y, a, b, n, accumulate, stream);
}
int odil_addcmul_f32(float* y, const float* a, const float* b, int64_t n, int accumulate, void* stream) {
  return addcmul<float>(y, a, b, n, accumulate, stream);
}
int odil_dots_f64(const double* a, int64_t lda, int nvec, const double* b, int64_t n, double* partials,
                  double* out, void* stream) {
  return dots<double>(a, lda, nvec, b, n, partials, out, stream);
}
int odil_dots_f32(const float* a, int64_t lda, int nvec, const float* b, int64_t n, double* partials, float* out,
                  void* stream) {
  return dots<float>(a, lda, nvec, b, n, partials, out, stream);
}
int odil_lbfgs_probe_f64(const double* g, const double* d, int64_t n, double* partials, double* out, void* stream) {
  return lbfgs_probe<double>(g, d, n, partials, out, stream);
}
int odil_lbfgs_probe_f32(const float* g, const float* d, int64_t n, double* partials, float* out, void* stream) {
  return lbfgs_probe<float>(g, d, n, partials, out, stream);
}
int odil_dots3_f64(const double* a, int64_t lda, int nvec, const double* b0, const double* b1, const double* b2,
                   int64_t n, double* partials, double* out, void* stream) {
  return dots3<double>(a, lda, nvec, b0, b1, b2, n, partials, out, stream);
}
int odil_dots3_f32(const float* a, int64_t lda, int nvec, const float* b0, const float* b1, const float* b2, int64_t n,
                   double* partials, float* out, void* stream) {
  return dots3<float>(a, lda, nvec, b0, b1, b2, n, partials, out, stream);
}
int64_t odil_lbfgs_batch_partials(int64_t n, int max_count, int elem_size) {
  if (n < 1 || (elem_size != 4 && elem_size != 8)) return 0;
  return batch_partials(n, max_count, elem_size);
}
int odil_lbfgs_probe_batch_f64(const double* g, int64_t g_stride, const double* d, int64_t d_stride, int64_t n,
                               int nbatch, const int32_t* members, int nsel, double* partials,
                               int64_t partials_stride, int64_t partials_len, double* out, int64_t out_stride,
                               void* stream) {
  return lbfgs_probe_batch<double>(g, g_stride, d, d_stride, n, nbatch, members, nsel, partials, partials_stride,
                                   partials_len, out, out_stride, stream);
}
int odil_lbfgs_probe_batch_f32(const float* g, int64_t g_stride, const float* d, int64_t d_stride, int64_t n,
                               int nbatch, const int32_t* members, int nsel, double* partials,
                               int64_t partials_stride, int64_t partials_len, float* out, int64_t out_stride,
                               void* stream) {
  return lbfgs_probe_batch<float>(g, g_stride, d, d_stride, n, nbatch, members, nsel, partials, partials_stride,
                                  partials_len, out, out_stride, stream);
}
int odil_lbfgs_dots3_batch_f64(const double* a, int64_t a_stride, int64_t lda, int rows, const int32_t* counts,
                               int max_count, const double* b0, int64_t b0_stride, const double* b1, int64_t b1_stride,
                               const double* b2, int64_t b2_stride, int64_t n, int nbatch, const int32_t* members,
                               int nsel, double* partials, int64_t partials_stride, int64_t partials_len, double* out,
                               int64_t out_stride, int64_t ldo, void* stream) {
  return lbfgs_dots3_batch<double>(a, a_stride, lda, rows, counts, max_count, b0, b0_stride, b1, b1_stride, b2,
                                   b2_stride, n, nbatch, members, nsel, partials, partials_stride, partials_len, out,
                                   out_stride, ldo, stream);
}
int odil_lbfgs_dots3_batch_f32(const float* a, int64_t a_stride, int64_t lda, int rows, const int32_t* counts,
                               int max_count, const float* b0, int64_t b0_stride, const float* b1, int64_t b1_stride,
                               const float* b2, int64_t b2_stride, int64_t n, int nbatch, const int32_t* members,
                               int nsel, double* partials, int64_t partials_stride, int64_t partials_len, float* out,
                               int64_t out_stride, int64_t ldo, void* stream) {
  return lbfgs_dots3_batch<float>(a, a_stride, lda, rows, counts, max_count, b0, b0_stride, b1, b1_stride, b2, b2_stride,
                                  n, nbatch, members, nsel, partials, partials_stride, partials_len, out, out_stride, ldo,
                                  stream);
}
int odil_lbfgs_lincomb_batch_f64(double* y, int64_t y_stride, double beta, const double* a, int64_t a_stride,
                                 int64_t lda, int rows, const int32_t* counts, int max_count, const double* coef,
                                 int64_t coef_stride, int64_t n, int nbatch, const int32_t* members, int nsel,
                                 void* stream) {
  return lbfgs_lincomb_batch<double>(y, y_stride, beta, a, a_stride, lda, rows, counts, max_count, coef, coef_stride, n,
                                     nbatch, members, nsel, stream);
}
int odil_lbfgs_lincomb_batch_f32(float* y, int64_t y_stride, float beta, const float* a, int64_t a_stride, int64_t lda,
                                 int rows, const int32_t* counts, int max_count, const float* coef, int64_t coef_stride,
                                 int64_t n, int nbatch, const int32_t* members, int nsel, void* stream) {
  return lbfgs_lincomb_batch<float>(y, y_stride, beta, a, a_stride, lda, rows, counts, max_count, coef, coef_stride, n,
                                    nbatch, members, nsel, stream);
}
int odil_lbfgs_axpy_batch_f64(double* out, int64_t out_stride, const double* y, int64_t y_stride, const double* x,
                              int64_t x_stride, const double* alpha, int64_t n, int nbatch, const int32_t* members,
                              int nsel, void* stream) {
  return lbfgs_axpy_batch<double>(out, out_stride, y, y_stride, x, x_stride, alpha, n, nbatch, members, nsel, stream);
}
int odil_lbfgs_axpy_batch_f32(float* out, int64_t out_stride, const float* y, int64_t y_stride, const float* x,
                              int64_t x_stride, const float* alpha, int64_t n, int nbatch, const int32_t* members,
                              int nsel, void* stream) {
  return lbfgs_axpy_batch<float>(out, out_stride, y, y_stride, x, x_stride, alpha, n, nbatch, members, nsel, stream);
}
int odil_lbfgs_pair_batch_f64(const double* g, int64_t g_stride, double* r, int64_t r_stride, double* d,
                              int64_t d_stride, double* w, int64_t w_stride, int64_t lda, int rows, const double* stp,
                              const int32_t* slot, int64_t n, int nbatch, const int32_t* members, int nsel,
                              void* stream) {
  return lbfgs_pair_batch<double>(g, g_stride, r, r_stride, d, d_stride, w, w_stride, lda, rows, stp, slot, n, nbatch,
                                  members, nsel, stream);
}
int odil_lbfgs_pair_batch_f32(const float* g, int64_t g_stride, float* r, int64_t r_stride, float* d, int64_t d_stride,
                              float* w, int64_t w_stride, int64_t lda, int rows, const float* stp, const int32_t* slot,
                              int64_t n, int nbatch, const int32_t* members, int nsel, void* stream) {
  return lbfgs_pair_batch<float>(g, g_stride, r, r_stride, d, d_stride, w, w_stride, lda, rows, stp, slot, n, nbatch,
                                 members, nsel, stream);
}
int odil_lincomb_f64(double* y, double beta, const double* a, int64_t lda, int nvec, const double* coef, int64_t n,
                     void* stream) {
  return lincomb<double>(y, beta, a, lda, nvec, coef, n, stream);
}
int odil_lincomb_f32(float* y, float beta, const float* a, int64_t lda, int nvec, const float* coef, int64_t n,
                     void* stream) {
  return lincomb<float>(y, beta, a, lda, nvec, coef, n, stream);
}
}
