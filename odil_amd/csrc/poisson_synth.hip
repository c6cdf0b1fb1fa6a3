// One damped-Jacobi sweep of the Poisson operator with the LAST prolongation of a V-cycle fused in:
//   u = x + P x_c   (reference core.py:245-263, last step)   is never written to memory,
//   the sweep of A u = rhs (reference examples/poisson/poisson.py:57-113) is evaluated from it directly.
// (The residual of the Adam epoch with the same prolongation fused in is poisson_synth_tile.hip.)
//
// The walk is the one of k_interp_add_march: a thread owns a coarse column (jy, jx), keeps the
// 3 x 3 x 3 ghosted coarse neighbourhood in registers and steps through the coarse planes.  That
// neighbourhood determines u on the 4 x 4 x 4 fine patch around the thread's 2 x 2 x 2 fine cells,
// which is everything the 7-point stencil of those cells reads: own values for the planes below and
// above slide through registers, edge neighbours are recomputed (P costs 8 multiply-adds per
// value; the kernel stays HBM-bound), and only x is loaded at those positions.  Every u is formed
// by exactly the arithmetic of the transfer kernel (same order, same constants), so the result is
// bit-identical to the two-kernel path.
#include "poisson_synth.h"

namespace odil {

// The same value in every lane, kept in scalar registers.
__device__ __forceinline__ double uniform_value(double x) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float uniform_value(float x) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// omega / diag by walls touched, w[z wall][y wall][x wall] (k_poisson_jacobi: the diagonal is the sum over the axes of
// (-2 / h^2) (1 + walls touched)): eight values that are the same in every lane -- scalar registers; one set per own
// cell in vector registers pushed this kernel over its register budget (255 + 20 spilled).
template <typename T>
__device__ __forceinline__ void jacobi_weight_table(const H2<T>& h, T omega, T (&w)[2][2][2]) {
#pragma unroll
  for (int zw = 0; zw < 2; ++zw)
#pragma unroll
    for (int yw = 0; yw < 2; ++yw)
#pragma unroll
      for (int xw = 0; xw < 2; ++xw) {
        const T dz = div_h2<T>(T(-2), h, 0) * T(1 + zw), dy = div_h2<T>(T(-2), h, 1) * T(1 + yw);
        w[zw][yw][xw] = uniform_value(omega / ((dz + dy) + div_h2<T>(T(-2), h, 2) * T(1 + xw)));
      }
}

// The first post-smoothing sweep of a V-cycle with the coarse-grid correction formed in registers: u = w0 + P coarse
// is never stored, 3 1/8 words per cell instead of 5 1/8; fu receives the new iterate.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_poisson_jacobi_synth(const T* __restrict__ coarse,
                                                                 const T* __restrict__ w0,
                                                                 const T* __restrict__ rhs, T* __restrict__ fu,
                                                                 MarchArgs a, H2<T> h, T omega) {
  const int cnz = a.cn[0], cny = a.cn[1], cnx = a.cn[2];
  const int FZ = a.fn[0], FY = a.fn[1], FX = a.fn[2];
  const int64_t cplane = (int64_t)cny * cnx, fplane = (int64_t)FY * FX;
  int zc, yt, xt;
  const bool have = unit_decode(a.usched, zc, yt, xt);
  const int lx = threadIdx.x % a.tx, ly = threadIdx.x / a.tx;
  const int jy = yt * a.ty + ly, jx = xt * a.tx + lx;
  if (have && jy < cny && jx < cnx) {
    const int z0 = zc * a.usched.ZC;
    const int z1 = z0 + a.usched.ZC < cnz ? z0 + a.usched.ZC : cnz;
    const TapN<3> tx = tapn<3>(jx, cnx), ty = tapn<3>(jy, cny);
    const int fy0 = 2 * jy, fx0 = 2 * jx;
    // clamped positions of the edge neighbours (values beyond a wall are discarded by axis_term)
    const int64_t row0 = (int64_t)fy0 * FX + fx0, row1 = row0 + FX;
    const int64_t rowm = (int64_t)(fy0 == 0 ? 0 : fy0 - 1) * FX + fx0;
    const int64_t rowp = (int64_t)(fy0 + 2 >= FY ? FY - 1 : fy0 + 2) * FX + fx0;
    const int xm = fx0 == 0 ? 0 : -1, xp = fx0 + 2 >= FX ? 1 : 2;
    // omega / diag of the four own cells on a plane away from the z walls (k_poisson_jacobi: the diagonal is
    // sum over axes of (-2 / h^2) (1 + walls touched)); the two wall planes of the array form theirs where needed
    T wdt[2][2][2];
    jacobi_weight_table<T>(h, omega, wdt);
    T v[3][3][3];
    load_plane<T, 1>(coarse, z0 - 1, cnz, cplane, cnx, ty, tx, T(1), v[0]);
    load_plane<T, 1>(coarse, z0, cnz, cplane, cnx, ty, tx, T(1), v[1]);
    // own values of the fine planes 2 z0 - 1 and 2 z0 (the first is beyond the wall when z0 == 0)
    T uA[2][2], uB[2][2];
    {
      // relative to coarse plane z0 these planes have offsets -1 and 0: both read the window rows
      // 0 and 1 (coarse planes z0 - 1, z0), which are loaded; row 2 is not touched yet
      PackN<T, 2> wa[2], wb[2];
      const int64_t pa = (int64_t)(z0 == 0 ? 0 : 2 * z0 - 1) * fplane, pb = (int64_t)(2 * z0) * fplane;
      wa[0] = stream_ld<T, 2>(w0 + pa + row0, false);
      wa[1] = stream_ld<T, 2>(w0 + pa + row1, false);
      wb[0] = stream_ld<T, 2>(w0 + pb + row0, false);
      wb[1] = stream_ld<T, 2>(w0 + pb + row1, false);
      synth_own<T, -1>(v, wa, uA);
      synth_own<T, 0>(v, wb, uB);
    }
    for (int jz = z0; jz < z1; ++jz) {
      const int fzB = 2 * jz, fzC = 2 * jz + 1, fzD = 2 * jz + 2;
      const int64_t pB = (int64_t)fzB * fplane, pC = (int64_t)fzC * fplane;
      const int64_t pD = (int64_t)(fzD >= FZ ? FZ - 1 : fzD) * fplane;
      // the HBM streams of this step first: w0 of the two new own planes, the edge rows / columns of
      // the two planes that are finalised, rhs
      PackN<T, 2> wC[2], wD[2], wyB[2], wyC[2], rB[2], rC[2];
      T wxB[2][2], wxC[2][2];
      // (w0 rows are re-read as edge rows by the neighbouring threads of the XCD: cached loads;
      // rhs and fu are touched once: streamed)
      wC[0] = stream_ld<T, 2>(w0 + pC + row0, false);
      wC[1] = stream_ld<T, 2>(w0 + pC + row1, false);
      wD[0] = stream_ld<T, 2>(w0 + pD + row0, false);
      wD[1] = stream_ld<T, 2>(w0 + pD + row1, false);
      wyB[0] = stream_ld<T, 2>(w0 + pB + rowm, false);
      wyB[1] = stream_ld<T, 2>(w0 + pB + rowp, false);
      wyC[0] = stream_ld<T, 2>(w0 + pC + rowm, false);
      wyC[1] = stream_ld<T, 2>(w0 + pC + rowp, false);
      rB[0] = stream_ld<T, 2>(rhs + pB + row0, true);
      rB[1] = stream_ld<T, 2>(rhs + pB + row1, true);
      rC[0] = stream_ld<T, 2>(rhs + pC + row0, true);
      rC[1] = stream_ld<T, 2>(rhs + pC + row1, true);
#pragma unroll
      for (int iy = 0; iy < 2; ++iy) {
        wxB[iy][0] = w0[pB + row0 + iy * FX + xm];
        wxB[iy][1] = w0[pB + row0 + iy * FX + xp];
        wxC[iy][0] = w0[pC + row0 + iy * FX + xm];
        wxC[iy][1] = w0[pC + row0 + iy * FX + xp];
      }
      load_plane<T, 1>(coarse, jz + 1, cnz, cplane, cnx, ty, tx, T(1), v[2]);
      T uC[2][2], uD[2][2];
      synth_own<T, 1>(v, wC, uC);
      synth_own<T, 2>(v, wD, uD);
      T fB[2][2], fC[2][2];
      residual_plane<T, 0, true>(v, uB, uA, uC, wyB, wxB, rB, fzB, fy0, fx0, FZ, FY, FX, h, fB, wdt);
      residual_plane<T, 1, true>(v, uC, uB, uD, wyC, wxC, rC, fzC, fy0, fx0, FZ, FY, FX, h, fC, wdt);
#pragma unroll
      for (int iy = 0; iy < 2; ++iy) {
        PackN<T, 2> o;
        o.e[0] = fB[iy][0], o.e[1] = fB[iy][1];
        stream_st<T, 2>(fu + pB + row0 + iy * FX, o, true);
        o.e[0] = fC[iy][0], o.e[1] = fC[iy][1];
        stream_st<T, 2>(fu + pC + row0 + iy * FX, o, true);
      }
#pragma unroll
      for (int iy = 0; iy < 2; ++iy)
#pragma unroll
        for (int ix = 0; ix < 2; ++ix) {
          uA[iy][ix] = uC[iy][ix];
          uB[iy][ix] = uD[iy][ix];
        }
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          v[0][dy][dx] = v[1][dy][dx];
          v[1][dy][dx] = v[2][dy][dx];
        }
    }
  }
}

template <typename T>
static int poisson_jacobi_synth(const T* coarse, const T* x, const T* rhs, T* xout, const int64_t* cshape, const T* h2,
                                T omega, void* stream) {
  if (!coarse || !x || !rhs || !xout || xout == x) {
    set_error("poisson_jacobi_synth: null pointer (or the sweep in place)");
    return ODIL_E_INVAL;
  }
  SynthArgs sa;
  if (int e = synth_geometry<T>(x, rhs, xout, cshape, sa)) return e;
  T hh[3] = {h2[0], h2[1], h2[2]};
  hipLaunchKernelGGL((k_poisson_jacobi_synth<T>), dim3(unit_grid(sa.m.usched)), dim3(kBlock), 0, (hipStream_t)stream,
                     coarse, x, rhs, xout, sa.m, make_h2<T>(hh), omega);
  return check_launch("k_poisson_jacobi_synth");
}

}  // namespace odil

using namespace odil;

extern "C" {
int odil_poisson_jacobi_synth_f64(const double* coarse, const double* x, const double* rhs, double* xout,
                                  const int64_t* cshape, const double* h2, double omega, void* stream) {
  return poisson_jacobi_synth<double>(coarse, x, rhs, xout, cshape, h2, omega, stream);
}
int odil_poisson_jacobi_synth_f32(const float* coarse, const float* x, const float* rhs, float* xout,
                                  const int64_t* cshape, const float* h2, float omega, void* stream) {
  return poisson_jacobi_synth<float>(coarse, x, rhs, xout, cshape, h2, omega, stream);
}
}  // extern "C"
