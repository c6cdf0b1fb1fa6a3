// Poisson residual with the LAST prolongation of the multigrid synthesis fused in:
//   u = w_0 + P s_1   (reference core.py:245-263, last step)   is never written to memory,
//   fu = Lap(u) - rhs (reference examples/poisson/poisson.py:57-113) is evaluated from it directly.
//
// A workgroup owns a tile of kTileY x kTileX coarse columns and marches a z-chunk; a thread owns one coarse column,
// that is its 2 x 2 fine cells on two fine planes per step, keeps the 3 x 3 x 3 ghosted coarse neighbourhood in
// registers and forms only its OWN u (synth_own).  What the marching body (poisson_synth.hip) fetched or recomputed
// per thread is shared through LDS instead:
//   * the ghosted coarse plane (tile + halo 1) is staged once per step by the workgroup -- 2 x 2 one-element loads per
//     thread instead of 18 -- and every thread reads its 3 x 3 window of the new plane from there;
//   * the y+-1 / x+-1 neighbours of the own cells are the OWN values of the neighbouring threads, published to an LDS
//     plane: the same expression on the same operands as the edge value the marching body recomputed
//     (synth_val<EZ, 0, -1> of column j is synth_val<EZ, 0, 1> of column j - 1: same coarse values, order, weights),
//     so fu stays bit-identical to odil_interp_add + odil_poisson_residual;
//   * only the ring of fine cells around the tile is formed by the workgroup itself, from w0 and the staged coarse
//     planes, by the first kHaloTasks threads as a phase of its own.
// The HBM streams of a step (w0, rhs, the ring's w0) and the coarse plane of the next step are requested at the top of
// the step, before its barriers and arithmetic.
//
// Loss: a thread sums the squares of its cells in the order of the marching body, over the z-chunks of the marching
// layout (synth_geometry), and writes that double to column_sums[chunk][jy][jx]; k_synth_loss_replay then runs the
// marching layout's workgroup reduction over those values, so the loss keeps every bit it had when one launch did both.
#include "poisson_synth.h"

namespace odil {

// coarse columns of a workgroup: 8 x 32 measured against 16 x 16 (0.67 against 0.69 ms for the three launches at 512^3
// f64); 4 x 64 has a ring of 272 pairs, more than the workgroup has threads
constexpr int kTileY = 8, kTileX = 32;
static_assert(kTileY * kTileX == kBlock, "one thread per coarse column");
constexpr int kCoarseRows = kTileY + 2, kCoarsePitch = kTileX + 2;  // ghosted tile + halo 1
constexpr int kCoarseCells = kCoarseRows * kCoarsePitch;
constexpr int kStageRounds = (kCoarseCells + kBlock - 1) / kBlock;
// fine tile + halo 1: fine row r of the tile in LDS row 1 + r, fine column c in LDS column 2 + c (own pairs start at
// even columns: one 16-byte access)
constexpr int kFineRows = 2 * kTileY + 2, kFinePitch = 2 * kTileX + 4;
// the ring around the fine tile in pairs of cells, per fine plane of a step: kTileX above, kTileX below, kTileY left,
// kTileY right (the corners are not read by a 7-point stencil)
constexpr int kRingPairs = 2 * kTileX + 2 * kTileY, kHaloTasks = 2 * kRingPairs;
static_assert(kHaloTasks <= kBlock, "one ring pair per thread");

struct SynthTileArgs {
  int cn[3];         // (z, y, x) coarse extents
  UnitSched usched;  // (z-chunk, tile row, tile column); the chunks are those of the marching layout
  int64_t loss_z0, loss_z1;  // fine planes that enter the loss
};

// LDS slot of the ghosted coarse plane q >= -1 in the ring of three
__device__ __forceinline__ int coarse_slot(int q) { return (q + 1) % 3; }

// synth_val for a fine cell whose parities are known at run time, from the staged planes: c0 / c1 are the coarse planes
// of rz = 0 / 1, base the staged position of (ry, rx) = (0, 0).  The order (rz, ry, rx), the weights and the scaling of
// synth_val.
template <typename T>
__device__ inline T synth_val_staged(const T* c0, const T* c1, int sz, int sy, int sx, int base) {
  T s = T(0);
#pragma unroll
  for (int rz = 0; rz < 2; ++rz) {
    const T* c = rz ? c1 : c0;
#pragma unroll
    for (int ry = 0; ry < 2; ++ry)
#pragma unroll
      for (int rx = 0; rx < 2; ++rx) {
        const int w = (sz == rz ? 1 : 3) * (sy == ry ? 1 : 3) * (sx == rx ? 1 : 3);
        s = s + T(w) * c[base + ry * kCoarsePitch + rx];
      }
  }
  return s * (T(1) / T(64));
}

// The HBM streams of one step that a thread consumes in registers.
template <typename T>
struct StepLoads {
  PackN<T, 2> wC[2], wD[2], rB[2], rC[2];  // w0 of the two new own planes, rhs of the two planes that are finalised
  T ring[2];                               // w0 of the thread's pair of ring cells
};

// The walk of one workgroup over its tile and z-chunk of ONE volume (the single launch, and member blockIdx.y of the
// ensemble launch on its own pointers).
template <typename T>
__device__ __forceinline__ void residual_tile_walk(const T* __restrict__ coarse, const T* __restrict__ w0,
                                                   const T* __restrict__ rhs, T* __restrict__ fu,
                                                   const SynthTileArgs& a, const H2<T>& h,
                                                   double* __restrict__ column_sums) {
  __shared__ T cs[3][kCoarseCells];
  __shared__ T fs[2][kFineRows * kFinePitch];
  const int cnz = a.cn[0], cny = a.cn[1], cnx = a.cn[2];
  const int FZ = 2 * cnz, FY = 2 * cny, FX = 2 * cnx;
  const int64_t cplane = (int64_t)cny * cnx, fplane = (int64_t)FY * FX;
  int zc, yt, xt;
  if (!unit_decode(a.usched, zc, yt, xt)) return;  // (the whole workgroup)
  const int tid = threadIdx.x, lx = tid % kTileX, ly = tid / kTileX;
  const int jy0 = yt * kTileY, jx0 = xt * kTileX;
  const int jy = jy0 + ly, jx = jx0 + lx;
  // threads beyond a ragged end of the array take part in the staging, the ring and the barriers; their own loads are
  // those of the last column inside, their values are read by nobody (the neighbour inside sits on a wall)
  const bool valid = jy < cny && jx < cnx;
  const int z0 = zc * a.usched.ZC;
  const int z1 = z0 + a.usched.ZC < cnz ? z0 + a.usched.ZC : cnz;
  const int fy0 = 2 * jy, fx0 = 2 * jx;
  const int64_t row0 = (int64_t)(2 * (jy < cny ? jy : cny - 1)) * FX + 2 * (jx < cnx ? jx : cnx - 1), row1 = row0 + FX;

  // ---- staging of the ghosted coarse plane: position tid (+ kBlock) of the (tile + halo) plane
  int64_t scl[kStageRounds], srf[kStageRounds];
  bool sout[kStageRounds];
#pragma unroll
  for (int k = 0; k < kStageRounds; ++k) {
    const int p = tid + k * kBlock < kCoarseCells ? tid + k * kBlock : kCoarseCells - 1;
    const int qy = jy0 - 1 + p / kCoarsePitch, qx = jx0 - 1 + p % kCoarsePitch;
    const int ycl = qy < 0 ? 0 : (qy >= cny ? cny - 1 : qy), yrf = qy < 0 ? 1 : (qy >= cny ? cny - 2 : qy);
    const int xcl = qx < 0 ? 0 : (qx >= cnx ? cnx - 1 : qx), xrf = qx < 0 ? 1 : (qx >= cnx ? cnx - 2 : qx);
    scl[k] = (int64_t)ycl * cnx + xcl;
    srf[k] = (int64_t)yrf * cnx + xrf;
    sout[k] = qy < 0 || qy >= cny || qx < 0 || qx >= cnx;
  }
  // load_plane's loads and its expression, one position per round instead of a 3 x 3 window
  auto stage_load = [&](int q, T (&cl)[kStageRounds], T (&rf)[kStageRounds]) {
    const int zcl = q < 0 ? 0 : (q >= cnz ? cnz - 1 : q);
    const int zrf = q < 0 ? 1 : (q >= cnz ? cnz - 2 : q);
    const T* ccl = coarse + zcl * cplane;
    const T* crf = coarse + zrf * cplane;
#pragma unroll
    for (int k = 0; k < kStageRounds; ++k) {
      cl[k] = ccl[scl[k]];
      rf[k] = crf[srf[k]];
    }
  };
  auto stage_store = [&](int q, const T (&cl)[kStageRounds], const T (&rf)[kStageRounds]) {
    const bool oz = q < 0 || q >= cnz;
    const T cscale = T(1);
    T* plane = cs[coarse_slot(q)];
#pragma unroll
    for (int k = 0; k < kStageRounds; ++k) {
      const T val = cscale * cl[k];
      const T ghost = T(2) * val - cscale * rf[k];
      if (tid + k * kBlock < kCoarseCells) plane[tid + k * kBlock] = (oz || sout[k]) ? ghost : val;
    }
  };

  // ---- the thread's pair of ring cells (tid < kHaloTasks): fine plane hz of the step, tile-local fine position
  // (hy, hx) of the first cell, the second one step along the ring
  const int hz = tid / kRingPairs, hs = tid % kRingPairs;
  int hy, hx, hdy, hdx;
  if (hs < kTileX)
    hy = -1, hx = 2 * hs, hdy = 0, hdx = 1;
  else if (hs < 2 * kTileX)
    hy = 2 * kTileY, hx = 2 * (hs - kTileX), hdy = 0, hdx = 1;
  else if (hs < 2 * kTileX + kTileY)
    hy = 2 * (hs - 2 * kTileX), hx = -1, hdy = 1, hdx = 0;
  else
    hy = 2 * (hs - 2 * kTileX - kTileY), hx = 2 * kTileX, hdy = 1, hdx = 0;
  int64_t hoff[2];     // position in the fine plane, clamped into the array (values beyond a wall are discarded)
  int hfine[2];        // position in the LDS fine plane
  int hbase[2], hsy[2], hsx[2];  // staged coarse position of (ry, rx) = (0, 0) and the parities
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int y = hy + c * hdy, x = hx + c * hdx;
    int gy = 2 * jy0 + y, gx = 2 * jx0 + x;
    gy = gy < 0 ? 0 : (gy >= FY ? FY - 1 : gy);
    gx = gx < 0 ? 0 : (gx >= FX ? FX - 1 : gx);
    hoff[c] = (int64_t)gy * FX + gx;
    hfine[c] = (1 + y) * kFinePitch + 2 + x;
    hsy[c] = y & 1, hsx[c] = x & 1;
    // fine y = 2 j + s reads the coarse rows j + s - 1 and j + s, staged one row further down
    hbase[c] = ((y >> 1) + hsy[c]) * kCoarsePitch + (x >> 1) + hsx[c];
  }

  auto step_loads = [&](int jz, StepLoads<T>& s) {
    const int fzB = 2 * jz, fzC = 2 * jz + 1, fzD = 2 * jz + 2;
    const int64_t pB = (int64_t)fzB * fplane, pC = (int64_t)fzC * fplane;
    const int64_t pD = (int64_t)(fzD >= FZ ? FZ - 1 : fzD) * fplane;
    // (w0 is re-read as ring cells by the neighbouring workgroups of the XCD: cached loads; rhs and fu are touched
    // once: streamed)
    s.wC[0] = stream_ld<T, 2>(w0 + pC + row0, false);
    s.wC[1] = stream_ld<T, 2>(w0 + pC + row1, false);
    s.wD[0] = stream_ld<T, 2>(w0 + pD + row0, false);
    s.wD[1] = stream_ld<T, 2>(w0 + pD + row1, false);
    s.rB[0] = stream_ld<T, 2>(rhs + pB + row0, true);
    s.rB[1] = stream_ld<T, 2>(rhs + pB + row1, true);
    s.rC[0] = stream_ld<T, 2>(rhs + pC + row0, true);
    s.rC[1] = stream_ld<T, 2>(rhs + pC + row1, true);
    if (tid < kHaloTasks) {
      const T* wp = w0 + (hz ? pC : pB);
      s.ring[0] = wp[hoff[0]];
      s.ring[1] = wp[hoff[1]];
    }
  };

  // ---- prologue: coarse planes z0 - 1, z0, z0 + 1 staged, own values of the fine planes 2 z0 - 1 and 2 z0 (the
  // first is beyond the wall when z0 == 0)
  StepLoads<T> cur;
  cur.ring[0] = cur.ring[1] = T(0);
  PackN<T, 2> wa[2], wb[2];
  {
    T cl[3][kStageRounds], rf[3][kStageRounds];
#pragma unroll
    for (int d = 0; d < 3; ++d) stage_load(z0 - 1 + d, cl[d], rf[d]);
    const int64_t pa = (int64_t)(z0 == 0 ? 0 : 2 * z0 - 1) * fplane, pb = (int64_t)(2 * z0) * fplane;
    wa[0] = stream_ld<T, 2>(w0 + pa + row0, false);
    wa[1] = stream_ld<T, 2>(w0 + pa + row1, false);
    wb[0] = stream_ld<T, 2>(w0 + pb + row0, false);
    wb[1] = stream_ld<T, 2>(w0 + pb + row1, false);
#pragma unroll
    for (int d = 0; d < 3; ++d) stage_store(z0 - 1 + d, cl[d], rf[d]);
  }
  __syncthreads();
  T v[3][3][3];
  auto read_window = [&](int q, T (&w)[3][3]) {
    const T* plane = cs[coarse_slot(q)];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) w[dy][dx] = plane[(ly + dy) * kCoarsePitch + lx + dx];
  };
  read_window(z0 - 1, v[0]);
  read_window(z0, v[1]);
  T uA[2][2], uB[2][2];
  // relative to coarse plane z0 these planes have offsets -1 and 0: both read the window rows 0 and 1 only
  synth_own<T, -1>(v, wa, uA);
  synth_own<T, 0>(v, wb, uB);

  double local = 0.0;
  const int own = (1 + 2 * ly) * kFinePitch + 2 + 2 * lx;  // the thread's first own cell in an LDS fine plane
  for (int jz = z0; jz < z1; ++jz) {
    const int fzB = 2 * jz, fzC = 2 * jz + 1;
    // the HBM streams of this step first, in one basic block, and the coarse plane of the NEXT step, which stays in
    // flight until the end of this one.  (w0 and rhs requested a whole step ahead as well: 238 instead of 211 VGPRs,
    // two waves per SIMD either way, 0.70 against 0.67 ms.)
    const bool more = jz + 1 < z1;
    T ncl[kStageRounds], nrf[kStageRounds];
    step_loads(jz, cur);
    if (more) stage_load(jz + 2, ncl, nrf);
    read_window(jz + 1, v[2]);
    T uC[2][2], uD[2][2];
    synth_own<T, 1>(v, cur.wC, uC);
    synth_own<T, 2>(v, cur.wD, uD);
    // publish the own values of the two planes that are finalised
#pragma unroll
    for (int iy = 0; iy < 2; ++iy)
#pragma unroll
      for (int ix = 0; ix < 2; ++ix) {
        fs[0][own + iy * kFinePitch + ix] = uB[iy][ix];
        fs[1][own + iy * kFinePitch + ix] = uC[iy][ix];
      }
    // the ring around the tile: plane 2 jz reads the coarse planes jz - 1 and jz, plane 2 jz + 1 jz and jz + 1
    if (tid < kHaloTasks) {
      const T* c0 = cs[coarse_slot(jz - 1 + hz)];
      const T* c1 = cs[coarse_slot(jz + hz)];
#pragma unroll
      for (int c = 0; c < 2; ++c)
        fs[hz][hfine[c]] = T(1) * cur.ring[c] + synth_val_staged<T>(c0, c1, hz, hsy[c], hsx[c], hbase[c]);
    }
    __syncthreads();
    T fB[2][2], fC[2][2];
#pragma unroll
    for (int ez = 0; ez < 2; ++ez) {
      const T* f = fs[ez] + own;
      T ylo[2], yhi[2], xlo[2], xhi[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ylo[i] = f[-kFinePitch + i];
        yhi[i] = f[2 * kFinePitch + i];
        xlo[i] = f[i * kFinePitch - 1];
        xhi[i] = f[i * kFinePitch + 2];
      }
      if (ez == 0)
        residual_cells<T>(uB, uA, uC, ylo, yhi, xlo, xhi, cur.rB, fzB, fy0, fx0, FZ, FY, FX, h, fB);
      else
        residual_cells<T>(uC, uB, uD, ylo, yhi, xlo, xhi, cur.rC, fzC, fy0, fx0, FZ, FY, FX, h, fC);
    }
    if (fu && valid) {
      const int64_t pB = (int64_t)fzB * fplane, pC = (int64_t)fzC * fplane;
#pragma unroll
      for (int iy = 0; iy < 2; ++iy) {
        PackN<T, 2> o;
        o.e[0] = fB[iy][0], o.e[1] = fB[iy][1];
        stream_st<T, 2>(fu + pB + row0 + iy * FX, o, true);
        o.e[0] = fC[iy][0], o.e[1] = fC[iy][1];
        stream_st<T, 2>(fu + pC + row0 + iy * FX, o, true);
      }
    }
    const bool inB = fzB >= a.loss_z0 && fzB < a.loss_z1, inC = fzC >= a.loss_z0 && fzC < a.loss_z1;
#pragma unroll
    for (int iy = 0; iy < 2; ++iy)
#pragma unroll
      for (int ix = 0; ix < 2; ++ix) {
        if (inB) local += (double)(fB[iy][ix] * fB[iy][ix]);
        if (inC) local += (double)(fC[iy][ix] * fC[iy][ix]);
      }
    // the coarse plane jz + 2 takes the slot of plane jz - 1, which the ring phase above was the last to read
    if (more) stage_store(jz + 2, ncl, nrf);
    __syncthreads();
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
  if (valid) column_sums[((int64_t)zc * cny + jy) * cnx + jx] = local;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_poisson_residual_tile(const T* __restrict__ coarse,
                                                                  const T* __restrict__ w0,
                                                                  const T* __restrict__ rhs, T* __restrict__ fu,
                                                                  SynthTileArgs a, H2<T> h,
                                                                  double* __restrict__ column_sums) {
  residual_tile_walk<T>(coarse, w0, rhs, fu, a, h, column_sums);
}

// The ensemble form: member blockIdx.y on its own arrays (element strides: w0, rhs, fu, coarse, column sums).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_poisson_residual_tile_batch(const T* __restrict__ coarse,
                                                                        const T* __restrict__ w0,
                                                                        const T* __restrict__ rhs, T* __restrict__ fu,
                                                                        BatchStrides st, SynthTileArgs a, H2<T> h,
                                                                        double* __restrict__ column_sums) {
  const int64_t b = blockIdx.y;
  residual_tile_walk<T>(coarse + b * st.s[3], w0 + b * st.s[0], rhs + b * st.s[1], fu + b * st.s[2], a, h,
                        column_sums + b * st.s[4]);
}

// The workgroup reduction of the marching layout over the column sums: workgroup b sums the threads of its unit in
// block_sum's order into partials[b].
__device__ __forceinline__ void synth_loss_replay(const double* __restrict__ column_sums, const MarchArgs& a,
                                                  double* __restrict__ partials) {
  const int cny = a.cn[1], cnx = a.cn[2];
  double local = 0.0;
  int zc, yt, xt;
  const bool have = unit_decode(a.usched, zc, yt, xt);
  const int lx = threadIdx.x % a.tx, ly = threadIdx.x / a.tx;
  const int jy = yt * a.ty + ly, jx = xt * a.tx + lx;
  if (have && jy < cny && jx < cnx) local = column_sums[((int64_t)zc * cny + jy) * cnx + jx];
  const double total = block_sum(local);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_synth_loss_replay(const double* __restrict__ column_sums, MarchArgs a,
                                                              double* __restrict__ partials) {
  synth_loss_replay(column_sums, a, partials);
}

// The ensemble form: member blockIdx.y reduces its own column sums into its own row of the [B, grid] partial sums.
__global__ __launch_bounds__(kBlock) void k_synth_loss_replay_batch(const double* __restrict__ column_sums,
                                                                    int64_t sums_stride, MarchArgs a,
                                                                    double* __restrict__ partials,
                                                                    int64_t partials_stride) {
  const int64_t b = blockIdx.y;
  synth_loss_replay(column_sums + b * sums_stride, a, partials + b * partials_stride);
}

static size_t column_sums_bytes(const SynthArgs& sa) {
  return (size_t)sa.m.usched.ZCH * sa.m.cn[1] * sa.m.cn[2] * sizeof(double);
}

template <typename T>
static int poisson_residual_synth(const T* coarse, const T* w0, const T* rhs, T* fu, const int64_t* cshape,
                                  const T* h2, int64_t z0, int64_t z1, double denom, double* partials,
                                  double* column_sums, size_t column_sums_size, T* loss, void* stream) {
  if (!coarse || !w0 || !rhs || !partials || !column_sums || !loss) {
    set_error("poisson_residual_synth: null pointer");
    return ODIL_E_INVAL;
  }
  SynthArgs sa;
  if (int e = synth_geometry<T>(w0, rhs, fu, cshape, sa)) return e;
  const MarchArgs& m = sa.m;
  const int grid = unit_grid(m.usched);
  if (grid > kMaxPartials) {
    set_error("poisson_residual_synth: %d workgroups exceed the reduction workspace", grid);
    return ODIL_E_INVAL;
  }
  if (column_sums_size < column_sums_bytes(sa)) {
    set_error("poisson_residual_synth: column sums need %lld bytes, %lld given", (long long)column_sums_bytes(sa),
              (long long)column_sums_size);
    return ODIL_E_INVAL;
  }
  SynthTileArgs ta;
  for (int i = 0; i < 3; ++i) ta.cn[i] = m.cn[i];
  const int64_t ytiles = (m.cn[1] + kTileY - 1) / kTileY, xtiles = (m.cn[2] + kTileX - 1) / kTileX;
  if ((int64_t)m.usched.ZCH * (ytiles + kNumXcd) * xtiles >= ((int64_t)1 << 31)) {
    set_error("poisson_residual_synth: grid too large for one launch");
    return ODIL_E_INVAL;
  }
  ta.usched = make_unit_sched_chunked(m.cn[0], ytiles, xtiles, m.usched.ZC);
  ta.loss_z0 = z0;
  ta.loss_z1 = z1 < 0 ? m.fn[0] : z1;
  T hh[3] = {h2[0], h2[1], h2[2]};
  hipLaunchKernelGGL((k_poisson_residual_tile<T>), dim3(unit_grid(ta.usched)), dim3(kBlock), 0, (hipStream_t)stream,
                     coarse, w0, rhs, fu, ta, make_h2<T>(hh), column_sums);
  if (int e = check_launch("k_poisson_residual_tile")) return e;
  hipLaunchKernelGGL(k_synth_loss_replay, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, column_sums, m, partials);
  if (int e = check_launch("k_synth_loss_replay")) return e;
  const double size = denom > 0.0 ? denom : (double)m.fn[0] * m.fn[1] * m.fn[2];
  return launch_final_reduce<T>(partials, grid, 0, 1, size, loss, (hipStream_t)stream);
}

// The ensemble form of poisson_residual_synth: nbatch members of one shape, each launch covering all of them.  Member
// b's loss is summed in the order of its single run: its own column sums, its own row of partial sums, one row of the
// final reduction.
template <typename T>
static int poisson_residual_synth_batch(const T* coarse, const T* w0, const T* rhs, T* fu, int nbatch, int64_t w0_stride,
                                        int64_t rhs_stride, int64_t fu_stride, const int64_t* cshape, int ndim,
                                        const T* h2, double* partials, int64_t partials_stride, int64_t partials_len,
                                        double* column_sums, size_t column_sums_size, T* loss, void* stream) {
  static const char* what = "poisson_residual_synth_batch";
  if (ndim != 3) {
    set_error("%s: ndim %d (this ensemble runs 3-D members)", what, ndim);
    return ODIL_E_INVAL;
  }
  if (!coarse || !w0 || !rhs || !fu || !cshape || !h2 || !partials || !column_sums || !loss) {
    set_error("%s: null pointer", what);
    return ODIL_E_INVAL;
  }
  if (nbatch < 1 || nbatch > 65535) {
    set_error("%s: %d members (1 ... 65535, one grid row each)", what, nbatch);
    return ODIL_E_INVAL;
  }
  SynthArgs sa;
  if (int e = synth_geometry<T>(w0, rhs, fu, cshape, sa)) return e;
  const MarchArgs& m = sa.m;
  const int64_t cells = (int64_t)m.fn[0] * m.fn[1] * m.fn[2];
  const int64_t strides[3] = {w0_stride, rhs_stride, fu_stride};
  for (int k = 0; k < 3; ++k) {
    if (strides[k] < cells) {
      set_error("%s: member stride %lld is smaller than a member (%lld cells)", what, (long long)strides[k],
                (long long)cells);
      return ODIL_E_INVAL;
    }
    // (the 16 B accesses of the own pairs assume member 0's alignment for every member)
    if ((strides[k] * (int64_t)sizeof(T)) % 16 != 0) {
      set_error("%s: member stride %lld is not a multiple of 16 bytes", what, (long long)strides[k]);
      return ODIL_E_INVAL;
    }
  }
  const int grid = unit_grid(m.usched);
  if (grid > kMaxPartials) {
    set_error("%s: %d workgroups exceed the reduction workspace", what, grid);
    return ODIL_E_INVAL;
  }
  if (partials_stride < grid || partials_stride >= ((int64_t)1 << 31)) {
    set_error("%s: partials workspace too small: rows of %lld doubles, a member needs %d", what,
              (long long)partials_stride, grid);
    return ODIL_E_INVAL;
  }
  if (partials_len < (int64_t)(nbatch - 1) * partials_stride + grid) {
    set_error("%s: partials workspace too small: %lld doubles are fewer than %d rows of %lld", what,
              (long long)partials_len, nbatch, (long long)partials_stride);
    return ODIL_E_INVAL;
  }
  const size_t per_member = column_sums_bytes(sa);
  if (column_sums_size / (size_t)nbatch < per_member) {
    set_error("%s: column sums need %lld bytes per member, %lld given for %d members", what, (long long)per_member,
              (long long)column_sums_size, nbatch);
    return ODIL_E_INVAL;
  }
  SynthTileArgs ta;
  for (int i = 0; i < 3; ++i) ta.cn[i] = m.cn[i];
  const int64_t ytiles = (m.cn[1] + kTileY - 1) / kTileY, xtiles = (m.cn[2] + kTileX - 1) / kTileX;
  if ((int64_t)m.usched.ZCH * (ytiles + kNumXcd) * xtiles >= ((int64_t)1 << 31)) {
    set_error("%s: grid too large for one launch", what);
    return ODIL_E_INVAL;
  }
  ta.usched = make_unit_sched_chunked(m.cn[0], ytiles, xtiles, m.usched.ZC);
  ta.loss_z0 = 0;
  ta.loss_z1 = m.fn[0];
  T hh[3] = {h2[0], h2[1], h2[2]};
  const int64_t sums_stride = (int64_t)(per_member / sizeof(double));
  const BatchStrides st = {{w0_stride, rhs_stride, fu_stride, (int64_t)m.cn[0] * m.cn[1] * m.cn[2], sums_stride}};
  hipLaunchKernelGGL((k_poisson_residual_tile_batch<T>), dim3(unit_grid(ta.usched), nbatch), dim3(kBlock), 0,
                     (hipStream_t)stream, coarse, w0, rhs, fu, st, ta, make_h2<T>(hh), column_sums);
  if (int e = check_launch("k_poisson_residual_tile_batch")) return e;
  hipLaunchKernelGGL(k_synth_loss_replay_batch, dim3(grid, nbatch), dim3(kBlock), 0, (hipStream_t)stream, column_sums,
                     sums_stride, m, partials, partials_stride);
  if (int e = check_launch("k_synth_loss_replay_batch")) return e;
  return launch_final_reduce<T>(partials, grid, (int)partials_stride, nbatch, (double)m.fn[0] * m.fn[1] * m.fn[2], loss,
                                (hipStream_t)stream);
}

}  // namespace odil

using namespace odil;

extern "C" {
size_t odil_poisson_residual_synth_workspace_bytes(const int64_t* cshape) {
  SynthArgs sa;
  if (!cshape || synth_geometry<double>(nullptr, nullptr, nullptr, cshape, sa)) return 0;
  return column_sums_bytes(sa);
}
size_t odil_poisson_residual_synth_batch_workspace_bytes(const int64_t* cshape) {
  return odil_poisson_residual_synth_workspace_bytes(cshape);  // per member
}
int64_t odil_poisson_residual_synth_batch_partials(const int64_t* cshape) {
  SynthArgs sa;
  if (!cshape || synth_geometry<double>(nullptr, nullptr, nullptr, cshape, sa)) return 0;
  const int grid = unit_grid(sa.m.usched);
  return grid > kMaxPartials ? 0 : grid;
}
int odil_poisson_residual_synth_batch_f64(const double* coarse, const double* w0, const double* rhs, double* fu,
                                          int nbatch, int64_t w0_stride, int64_t rhs_stride, int64_t fu_stride,
                                          const int64_t* cshape, int ndim, const double* h2, double* partials,
                                          int64_t partials_stride, int64_t partials_len, double* column_sums,
                                          size_t column_sums_size, double* loss, void* stream) {
  return poisson_residual_synth_batch<double>(coarse, w0, rhs, fu, nbatch, w0_stride, rhs_stride, fu_stride, cshape, ndim,
                                              h2, partials, partials_stride, partials_len, column_sums, column_sums_size,
                                              loss, stream);
}
int odil_poisson_residual_synth_batch_f32(const float* coarse, const float* w0, const float* rhs, float* fu, int nbatch,
                                          int64_t w0_stride, int64_t rhs_stride, int64_t fu_stride,
                                          const int64_t* cshape, int ndim, const float* h2, double* partials,
                                          int64_t partials_stride, int64_t partials_len, double* column_sums,
                                          size_t column_sums_size, float* loss, void* stream) {
  return poisson_residual_synth_batch<float>(coarse, w0, rhs, fu, nbatch, w0_stride, rhs_stride, fu_stride, cshape, ndim,
                                             h2, partials, partials_stride, partials_len, column_sums, column_sums_size,
                                             loss, stream);
}
int odil_poisson_residual_synth_f64(const double* coarse, const double* w0, const double* rhs, double* fu,
                                    const int64_t* cshape, const double* h2, int64_t z0, int64_t z1, double denom,
                                    double* partials, double* column_sums, size_t column_sums_size, double* loss,
                                    void* stream) {
  return poisson_residual_synth<double>(coarse, w0, rhs, fu, cshape, h2, z0, z1, denom, partials, column_sums,
                                        column_sums_size, loss, stream);
}
int odil_poisson_residual_synth_f32(const float* coarse, const float* w0, const float* rhs, float* fu,
                                    const int64_t* cshape, const float* h2, int64_t z0, int64_t z1, double denom,
                                    double* partials, double* column_sums, size_t column_sums_size, float* loss,
                                    void* stream) {
  return poisson_residual_synth<float>(coarse, w0, rhs, fu, cshape, h2, z0, z1, denom, partials, column_sums,
                                       column_sums_size, loss, stream);
}
}  // extern "C"
