// Device pieces shared by the kernels that fuse the last prolongation of the multigrid synthesis into the Poisson
// stencil (poisson_synth.hip: the marching Jacobi sweep; poisson_synth_tile.hip: the tiled residual), and the host
// geometry of their launches.
#pragma once
#include "mg_march.h"
#include "poisson.h"

namespace odil {

// Interpolated coarse contribution at fine offset (ez, ey, ex) in {-1, 0, 1, 2}^3 relative to the
// fine cell (2jz, 2jy, 2jx): coarse base (e + 2) / 2 - 1 and parity e & 1 per axis; reference
// order (rz, ry, rx), weights parity == r ? 1 : 3, scaled by the exact 1/64.
template <typename T, int EZ, int EY, int EX>
__device__ inline T synth_val(const T (&v)[3][3][3]) {
  constexpr int bz = (EZ + 2) / 2 - 1, by = (EY + 2) / 2 - 1, bx = (EX + 2) / 2 - 1;
  constexpr int sz = EZ & 1, sy = EY & 1, sx = EX & 1;
  T s = T(0);
#pragma unroll
  for (int rz = 0; rz < 2; ++rz)
#pragma unroll
    for (int ry = 0; ry < 2; ++ry)
#pragma unroll
      for (int rx = 0; rx < 2; ++rx) {
        const int w = (sz == rz ? 1 : 3) * (sy == ry ? 1 : 3) * (sx == rx ? 1 : 3);
        s = s + T(w) * v[bz + sz + rz][by + sy + ry][bx + sx + rx];  // window index 0..2 <-> coarse j-1..j+1
      }
  return s * (T(1) / T(64));
}

// own 2 x 2 of fine plane 2jz + EZ: u = w0 + P
template <typename T, int EZ>
__device__ inline void synth_own(const T (&v)[3][3][3], const PackN<T, 2> (&w)[2], T (&u)[2][2]) {
  u[0][0] = T(1) * w[0].e[0] + synth_val<T, EZ, 0, 0>(v);
  u[0][1] = T(1) * w[0].e[1] + synth_val<T, EZ, 0, 1>(v);
  u[1][0] = T(1) * w[1].e[0] + synth_val<T, EZ, 1, 0>(v);
  u[1][1] = T(1) * w[1].e[1] + synth_val<T, EZ, 1, 1>(v);
}

struct SynthArgs {
  MarchArgs m;
  int64_t loss_z0, loss_z1;  // fine planes that enter the loss
};

// Residual of the four own cells of fine plane fz from their neighbour values:
//   uc: own values, ub / ua: own values of the planes below / above, ylo / yhi[ix]: rows 2jy-1 / 2jy+2 at the own x,
//   xlo / xhi[iy]: columns 2jx-1 / 2jx+2 at the own rows (values beyond a wall are discarded by axis_term).
// JAC: f is the damped-Jacobi update q - (A u - rhs) wd instead of the residual, wd[iy][ix] = omega / diag of the plane.
template <typename T, bool JAC = false>
__device__ inline void residual_cells(const T (&uc)[2][2], const T (&ub)[2][2], const T (&ua)[2][2], const T (&ylo)[2],
                                      const T (&yhi)[2], const T (&xlo)[2], const T (&xhi)[2],
                                      const PackN<T, 2> (&r)[2], int fz, int fy0, int fx0, int FZ, int FY, int FX,
                                      const H2<T>& h, T (&f)[2][2], const T (*wd)[2][2] = nullptr) {
#pragma unroll
  for (int iy = 0; iy < 2; ++iy)
#pragma unroll
    for (int ix = 0; ix < 2; ++ix) {
      const int y = fy0 + iy, x = fx0 + ix;
      const T q = uc[iy][ix];
      const T ym = iy == 0 ? ylo[ix] : uc[0][ix], yp = iy == 0 ? uc[1][ix] : yhi[ix];
      const T xm = ix == 0 ? xlo[iy] : uc[iy][0], xp = ix == 0 ? uc[iy][1] : xhi[iy];
      T acc = axis_term<T>(q, ub[iy][ix], ua[iy][ix], fz == 0, fz == FZ - 1, h, 0);
      acc = acc + axis_term<T>(q, ym, yp, y == 0, y == FY - 1, h, 1);
      acc = acc + axis_term<T>(q, xm, xp, x == 0, x == FX - 1, h, 2);
      if constexpr (JAC) {  // k_poisson_jacobi's expression
        const bool zw = fz == 0 || fz == FZ - 1, yw = y == 0 || y == FY - 1, xw = x == 0 || x == FX - 1;
        const T w = zw ? (yw ? (xw ? wd[1][1][1] : wd[1][1][0]) : (xw ? wd[1][0][1] : wd[1][0][0]))
                       : (yw ? (xw ? wd[0][1][1] : wd[0][1][0]) : (xw ? wd[0][0][1] : wd[0][0][0]));
        f[iy][ix] = q - (acc - r[iy].e[ix]) * w;
      }
      else
        f[iy][ix] = acc - r[iy].e[ix];
    }
}

// Residual of the four own cells of fine plane fz = 2jz + EZ (EZ in {0, 1}).
//   uc: own values, ub / ua: own values of the planes below / above,
//   wy[2]: w0 packs of rows 2jy-1 and 2jy+2, wx[2][2]: w0 at x = 2jx-1 / 2jx+2 of the two own rows.
// The edge neighbours are recomputed from the thread's own coarse window.
template <typename T, int EZ, bool JAC = false>
__device__ inline void residual_plane(const T (&v)[3][3][3], const T (&uc)[2][2], const T (&ub)[2][2],
                                      const T (&ua)[2][2], const PackN<T, 2> (&wy)[2], const T (&wx)[2][2],
                                      const PackN<T, 2> (&r)[2], int fz, int fy0, int fx0, int FZ, int FY, int FX,
                                      const H2<T>& h, T (&f)[2][2], const T (*wd)[2][2] = nullptr) {
  // edge neighbours: rows 2jy-1 and 2jy+2 at the own x, columns 2jx-1 and 2jx+2 at the own rows
  T ylo[2], yhi[2], xlo[2], xhi[2];
  ylo[0] = T(1) * wy[0].e[0] + synth_val<T, EZ, -1, 0>(v);
  ylo[1] = T(1) * wy[0].e[1] + synth_val<T, EZ, -1, 1>(v);
  yhi[0] = T(1) * wy[1].e[0] + synth_val<T, EZ, 2, 0>(v);
  yhi[1] = T(1) * wy[1].e[1] + synth_val<T, EZ, 2, 1>(v);
  xlo[0] = T(1) * wx[0][0] + synth_val<T, EZ, 0, -1>(v);
  xlo[1] = T(1) * wx[1][0] + synth_val<T, EZ, 1, -1>(v);
  xhi[0] = T(1) * wx[0][1] + synth_val<T, EZ, 0, 2>(v);
  xhi[1] = T(1) * wx[1][1] + synth_val<T, EZ, 1, 2>(v);
  residual_cells<T, JAC>(uc, ub, ua, ylo, yhi, xlo, xhi, r, fz, fy0, fx0, FZ, FY, FX, h, f, wd);
}

// Host side of both launches: the refusals, and the layout in which a thread owns the coarse column (jy, jx) --
// tx lanes along x (the power of two that covers the row, at most the workgroup), ty rows, z-chunks by UnitSched.
// The marching sweep runs in this layout; the tiled residual runs in tiles of its own and sums its loss in this one.
template <typename T>
inline int synth_geometry(const T* w0, const T* rhs, const T* fu, const int64_t* cshape, SynthArgs& sa) {
  MarchArgs& m = sa.m;
  for (int i = 0; i < 3; ++i) {
    if (cshape[i] < 2 || cshape[i] >= (1 << 29)) {
      set_error("poisson_residual_synth: coarse extent %lld on axis %d", (long long)cshape[i], i);
      return ODIL_E_INVAL;
    }
    m.cn[i] = (int)cshape[i];
    m.fn[i] = 2 * m.cn[i];
  }
  if (!((reinterpret_cast<uintptr_t>(w0) | reinterpret_cast<uintptr_t>(rhs) | reinterpret_cast<uintptr_t>(fu)) %
            (2 * sizeof(T)) ==
        0)) {
    set_error("poisson_residual_synth: arrays must be aligned to %d bytes", (int)(2 * sizeof(T)));
    return ODIL_E_INVAL;
  }
  m.cut_lo = m.cut_hi = 0;
  m.lead_loc = 0;
  m.lead_cn = m.lead_fn = 1;
  m.lead_cstride = 0;
  m.nt = (int64_t)m.fn[0] * m.fn[1] * m.fn[2] * (int64_t)sizeof(T) > kStreamBytes;
  int tx = 1;
  while (tx < m.cn[2] && tx < kBlock) tx *= 2;
  m.tx = tx;
  m.ty = kBlock / tx;
  const int64_t ytiles = (m.cn[1] + m.ty - 1) / m.ty, xtiles = (m.cn[2] + m.tx - 1) / m.tx;
  if ((int64_t)m.cn[0] * ytiles * xtiles >= ((int64_t)1 << 31)) {
    set_error("poisson_residual_synth: grid too large for one launch");
    return ODIL_E_INVAL;
  }
  m.usched = make_unit_sched(m.cn[0], ytiles, xtiles);
  return 0;
}

}  // namespace odil
