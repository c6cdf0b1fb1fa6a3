/*
 * odil_hip.h -- C-ABI of the MI355X-native (gfx950) ODIL hot path.
 *
 * The reference (cselab/odil v0.1.8) is pure Python and has no FFI boundary of its
 * own: its device arithmetic goes through the `mod` namespace into XLA / TensorFlow
 * (reference src/odil/backend.py:12-317).  This library is what a ROCm `mod` +
 * `Problem` bind instead.  Each entry point below cites the reference code whose
 * arithmetic it replaces (paths relative to the reference root).
 *
 * Conventions (all entry points):
 *   - `extern "C"`, plain pointers and sizes; no torch / C++ types.
 *   - every data pointer is a DEVICE pointer into caller-owned memory (the Python
 *     host passes torch tensor storage); the library never allocates, frees or
 *     retains device memory; scratch space is passed in explicitly.
 *   - arrays are C-order, contiguous; `shape` is the ARRAY shape (not cells),
 *     `ndim` <= ODIL_MAX_NDIM; `loc` is ODIL's location string, one of 'c' (cell),
 *     'n' (node), '.' (axis not refined) per axis (reference core.py:606-616).
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = default stream).
 *     Kernels are enqueued and the call returns; no host synchronisation inside.
 *   - return value: 0 on success, <0 on error (ODIL_E_*); the message is
 *     available from `odil_last_error()` (thread-local).
 *   - suffix `_f32` / `_f64` selects the arithmetic type (reference runtime.py:77).
 */
#ifndef ODIL_HIP_H
#define ODIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ODIL_MAX_NDIM 4
#define ODIL_MAX_LEVELS 32
#define ODIL_E_INVAL (-1)  /* bad argument */
#define ODIL_E_LAUNCH (-2) /* HIP launch / runtime failure */
#define ODIL_E_NODEV (-3)  /* no usable gfx950 device */

/* ---- library ---------------------------------------------------------------- */
const char* odil_last_error(void);
int odil_version(void);
/* Number of HIP devices visible, or <0.  Does not create a context. */
int odil_device_count(void);
/* Bytes of scratch every reduction-carrying call needs (`partials`). */
size_t odil_reduce_workspace_bytes(void);

/* ---- multigrid transfers (reference core.py:606-755) ------------------------- */
/* fine = add_scale * add + P(coarse_scale * coarse); `add` may be NULL (then fine =
 * P(coarse)).  Replaces `interp_to_finer(method="stack")` (core.py:606-700) and one
 * step of `Domain.multigrid_to_regular` (core.py:258-262).  `cshape` = coarse array
 * shape; fine shape per axis: 'c' 2n, 'n' 2n-1, '.' n. */
int odil_interp_add_f64(const double* coarse, const double* add, double* fine, const int64_t* cshape, int ndim,
                        const char* loc, double coarse_scale, double add_scale, void* stream);
int odil_interp_add_f32(const float* coarse, const float* add, float* fine, const int64_t* cshape, int ndim,
                        const char* loc, float coarse_scale, float add_scale, void* stream);
/* The same with the coarse operand a VIEW: `coarse_ld` elements lie between consecutive indices of its leading axis
 * (>= the product of its other extents; a ghost-extended level array of the slab paths without its outer ghost planes --
 * no reference counterpart).  Served by the marching kernels of the 4-D layouts ('nccc', '.ccc'); returns 1,
 * having launched nothing, for any other layout or size (the caller then passes a contiguous copy to odil_interp_add). */
int odil_interp_add_ld_f64(const double* coarse, int64_t coarse_ld, const double* add, double* fine, const int64_t* cshape,
                           int ndim, const char* loc, double coarse_scale, double add_scale, void* stream);
int odil_interp_add_ld_f32(const float* coarse, int64_t coarse_ld, const float* add, float* fine, const int64_t* cshape,
                           int ndim, const char* loc, float coarse_scale, float add_scale, void* stream);
/* gcoarse = P^T gfine (the cotangent autodiff produces for core.py:606-700);
 * if `gscaled` != NULL also gscaled = scale * gcoarse. */
int odil_interp_adj_f64(const double* gfine, double* gcoarse, double* gscaled, const int64_t* cshape, int ndim,
                        const char* loc, double scale, void* stream);
int odil_interp_adj_f32(const float* gfine, float* gcoarse, float* gscaled, const int64_t* cshape, int ndim,
                        const char* loc, float scale, void* stream);
/* gcoarse = P^T gfine written into a VIEW with `gcoarse_ld` elements between consecutive leading indices (see
 * odil_interp_add_ld; also the time part 'n...' of the two-step transpose of 'nccc' arrays).  Returns 1, having launched
 * nothing, where the layout is not served. */
int odil_interp_adj_ld_f64(const double* gfine, double* gcoarse, int64_t gcoarse_ld, const int64_t* cshape, int ndim,
                           const char* loc, void* stream);
int odil_interp_adj_ld_f32(const float* gfine, float* gcoarse, int64_t gcoarse_ld, const int64_t* cshape, int ndim,
                           const char* loc, void* stream);
/* Slab decomposition (no reference counterpart): the same transpose for an array
 * whose axis 0 is CUT at its low / high end -- that end carries ghost planes of the
 * neighbouring rank instead of being a wall, so the boundary (ghost-rule) weights are not
 * applied there. */
int odil_interp_adj_cut_f64(const double* gfine, double* gcoarse, double* gscaled, const int64_t* cshape, int ndim,
                            const char* loc, double scale, int cut_lo, int cut_hi, void* stream);
int odil_interp_adj_cut_f32(const float* gfine, float* gcoarse, float* gscaled, const int64_t* cshape, int ndim,
                            const char* loc, float scale, int cut_lo, int cut_hi, void* stream);
/* ... and with the Adam update of the coarse array (x, m, v of gcoarse's shape) fused in, as in
 * odil_mg_synth_adj_adam. */
int odil_interp_adj_cut_adam_f64(const double* gfine, double* gcoarse, const int64_t* cshape, int ndim, const char* loc,
                                 int cut_lo, int cut_hi, double* x, double* m, double* v, double alpha,
                                 double one_minus_b1, double one_minus_b2, double eps, const double* alpha_dev,
                                 void* stream);
int odil_interp_adj_cut_adam_f32(const float* gfine, float* gcoarse, const int64_t* cshape, int ndim, const char* loc,
                                 int cut_lo, int cut_hi, float* x, float* m, float* v, float alpha,
                                 float one_minus_b1, float one_minus_b2, float eps, const float* alpha_dev,
                                 void* stream);
/* coarse = R(fine): full weighting `restrict_to_coarser(method="conv")`
 * (core.py:703-755, backend.py:112-126).  `fshape` = fine array shape. */
int odil_restrict_f64(const double* fine, double* coarse, const int64_t* fshape, int ndim, const char* loc,
                      void* stream);
int odil_restrict_f32(const float* fine, float* coarse, const int64_t* fshape, int ndim, const char* loc,
                      void* stream);

/* gfine = R^T gcoarse: the cotangent autodiff routes through `restrict_to_coarser`
 * (`poisson --mgloss`, examples/poisson/poisson.py:116-122).  `fshape` = fine array shape. */
int odil_restrict_adj_f64(const double* gcoarse, double* gfine, const int64_t* fshape, int ndim, const char* loc,
                          void* stream);
int odil_restrict_adj_f32(const float* gcoarse, float* gfine, const int64_t* fshape, int ndim, const char* loc,
                          void* stream);

/* Strided VALID correlations with a small dense kernel: `mod.convolution` (backend.py:112-126 -> jax.lax.conv; called by
 * restrict_to_coarser, core.py:744-751) and `mod.conv_transpose` (backend.py:165-172 -> jax.lax.conv_transpose; called
 * by interp_to_finer(method="conv"), core.py:656-662) for user operators that call them directly (the framework's own
 * transfers use the dedicated kernels above).  Kernel extents and strides 1..4 per axis, ndim <= 4, taps summed in C
 * order of the kernel.
 *   transposed == 0:  out[o] = sum_k w[k] in[o * s + k],                 oshape = (ishape - wshape) / s + 1
 *   transposed != 0:  out[p] = sum_k w[k] in[(p - k) / s] over the taps with s | (p - k) and the quotient inside `in`
 *                     (the transpose of the above; oshape >= (ishape - 1) s + wshape, zeros beyond). */
int odil_conv_valid_f64(const double* in, const double* w, double* out, const int64_t* ishape, const int64_t* wshape,
                        const int64_t* strides, const int64_t* oshape, int ndim, int transposed, void* stream);
int odil_conv_valid_f32(const float* in, const float* w, float* out, const int64_t* ishape, const int64_t* wshape,
                        const int64_t* strides, const int64_t* oshape, int ndim, int transposed, void* stream);

/* u = sum_l P^l (factor_l * w_l): `Domain.multigrid_to_regular` (core.py:245-263).
 * terms / work / grads are HOST arrays of device pointers, factors / shapes HOST arrays.
 * terms[l]: level arrays fine->coarse, shapes[l*ndim..]: their array shapes,
 * work[l] (1 <= l <= nlvl-2): scratch of level l's size for the partial sums
 * (work[0] and work[nlvl-1] are ignored); `u` has level 0's shape. */
int odil_mg_synth_f64(const double* const* terms, const double* factors, double* const* work, double* u,
                      const int64_t* shapes, int nlvl, int ndim, const char* loc, void* stream);
int odil_mg_synth_f32(const float* const* terms, const float* factors, float* const* work, float* u,
                      const int64_t* shapes, int nlvl, int ndim, const char* loc, void* stream);
/* grads[l] = factor_l * (P^T)^l gu: transpose of the above (what jax.value_and_grad /
 * tf.GradientTape return for the level arrays, core.py:1100 / :1062).  work[l]
 * (1 <= l <= nlvl-1) is needed only for levels whose factor != 1. */
int odil_mg_synth_adj_f64(const double* gu, double* const* grads, const double* factors, double* const* work,
                          const int64_t* shapes, int nlvl, int ndim, const char* loc, void* stream);
int odil_mg_synth_adj_f32(const float* gu, float* const* grads, const float* factors, float* const* work,
                          const int64_t* shapes, int nlvl, int ndim, const char* loc, void* stream);

/* The same chain with the Adam update (optimizer.py:316-318) of every level l >= 1 whose x[l] is
 * non-NULL applied by the lane that forms grads[l][i] (x, m, v: HOST arrays of device pointers,
 * entry 0 ignored): the optimizer launch over the coarse levels and its re-read of the
 * gradients disappear.  grads are still written. */
int odil_mg_synth_adj_adam_f64(const double* gu, double* const* grads, const double* factors, double* const* work,
                               const int64_t* shapes, int nlvl, int ndim, const char* loc, double* const* x,
                               double* const* m, double* const* v, double alpha, double one_minus_b1,
                               double one_minus_b2, double eps, const double* alpha_dev, void* stream);
int odil_mg_synth_adj_adam_f32(const float* gu, float* const* grads, const float* factors, float* const* work,
                               const int64_t* shapes, int nlvl, int ndim, const char* loc, float* const* x,
                               float* const* m, float* const* v, float alpha, float one_minus_b1, float one_minus_b2,
                               float eps, const float* alpha_dev, void* stream);

/* ---- stencil access: Context.field (reference core.py:910-975) ---------------- */
/* out = trim(roll(pad(src), -shift)): 'c'->'n' zero-pad at the low end, periodic roll,
 * 'n'->'c' drop last (core.py:956-969).  `sshape` = source array shape. */
int odil_field_gather_f64(const double* src, double* out, const int64_t* sshape, int ndim, const char* field_loc,
                          const char* loc, const int64_t* shift, void* stream);
int odil_field_gather_f32(const float* src, float* out, const int64_t* sshape, int ndim, const char* field_loc,
                          const char* loc, const int64_t* shift, void* stream);
/* gsrc (+)= transpose of the gather applied to g; accumulate != 0 adds into gsrc. */
int odil_field_scatter_f64(const double* g, double* gsrc, const int64_t* sshape, int ndim, const char* field_loc,
                           const char* loc, const int64_t* shift, int accumulate, void* stream);
int odil_field_scatter_f32(const float* g, float* gsrc, const int64_t* sshape, int ndim, const char* field_loc,
                           const char* loc, const int64_t* shift, int accumulate, void* stream);

/* ---- loss reduction (reference core.py:1093-1095) ----------------------------- */
/* out[0] = mean(x^2) (square != 0) or mean(x) over n elements, accumulated in f64 in
 * a fixed order (deterministic).  `partials`: odil_reduce_workspace_bytes() scratch. */
int odil_mean_reduce_f64(const double* x, int64_t n, int square, double* partials, double* out, void* stream);
int odil_mean_reduce_f32(const float* x, int64_t n, int square, double* partials, float* out, void* stream);

/* ---- Poisson workload (reference examples/poisson/poisson.py:57-113) ---------- */
/* fu = sum_i (u+ - 2u + u-)/h2[i] - rhs with zero-Dirichlet ghosts by extrap_quadh
 * (poisson.py:57-68, core.py:1439-1445); loss[0] = mean(fu^2) (core.py:1093).
 * `fu` may be NULL (loss only).  `shape`: cell shape, ndim <= 3; h2[i] = step_i^2. */
int odil_poisson_residual_f64(const double* u, const double* rhs, double* fu, const int64_t* shape, int ndim,
                              const double* h2, double* partials, double* loss, void* stream);
int odil_poisson_residual_f32(const float* u, const float* rhs, float* fu, const int64_t* shape, int ndim,
                              const float* h2, double* partials, float* loss, void* stream);
/* Slab variant: fu on every plane of the (ghost-extended) local array, but
 * loss[0] = sum_{z0 <= z < z1} fu^2 / denom  (the rank's own planes over the GLOBAL size). */
int odil_poisson_residual_slab_f64(const double* u, const double* rhs, double* fu, const int64_t* shape, int ndim,
                                   const double* h2, int64_t z0, int64_t z1, double denom, double* partials,
                                   double* loss, void* stream);
int odil_poisson_residual_slab_f32(const float* u, const float* rhs, float* fu, const int64_t* shape, int ndim,
                                   const float* h2, int64_t z0, int64_t z1, double denom, double* partials,
                                   float* loss, void* stream);
/* Residual restricted to the next coarser grid in one pass (3-D, even extents, shape[2] a multiple of the
 * 16-byte pack): coarse[K,J,I] = scale * sum over the 2x2x2 fine cells of (A u - rhs), *loss = mean((A u -
 * rhs)^2).  Replaces odil_poisson_residual + odil_restrict in the V-cycle that solves the Newton system
 * (reference linsolver.py:61-72 uses pyamg there); `partials`: odil_reduce_workspace_bytes() scratch.  loss == NULL
 * (coarse levels of a cycle, whose norm nobody reads): the reduction launch is skipped. */
int odil_poisson_residual_restrict_f64(const double* u, const double* rhs, double* coarse, const int64_t* shape,
                                       int ndim, const double* h2, double scale, double* partials, double* loss,
                                       void* stream);
int odil_poisson_residual_restrict_f32(const float* u, const float* rhs, float* coarse, const int64_t* shape, int ndim,
                                       const float* h2, float scale, double* partials, float* loss, void* stream);
/* Slab variant (multi-GPU V-cycles, odil_amd/slab_solvers.py): the same pass over a ghost-extended local array, the
 * convergence measure restricted to the rank's own planes: *loss = sum over planes z0 <= z < z1 of (A u - rhs)^2 / denom
 * (z1 < 0: all planes; denom <= 0: the array size). */
int odil_poisson_residual_restrict_slab_f64(const double* u, const double* rhs, double* coarse, const int64_t* shape,
                                            int ndim, const double* h2, double scale, int64_t z0, int64_t z1,
                                            double denom, double* partials, double* loss, void* stream);
int odil_poisson_residual_restrict_slab_f32(const float* u, const float* rhs, float* coarse, const int64_t* shape,
                                            int ndim, const float* h2, float scale, int64_t z0, int64_t z1, double denom,
                                            double* partials, float* loss, void* stream);
/* Stencil adjoint and the first transposed prolongation in one pass (3-D, even extents >= 4):
 * g0 = scale * A^T fu (stored only when g0 != NULL), g1 = P^T g0 on the grid of half the extents, and the Adam
 * update of the finest level (x0, m0, v0; all NULL: no update, g0 required) and of the next level (x1, m1, v1;
 * optional) by the lanes that form their gradients.  g0 never makes the round trip through memory that
 * odil_poisson_adjoint_adam + odil_mg_synth_adj_adam need (reference core.py:1100 / optimizer.py:311-319);
 * results are bit-identical to that pair.  cut_lo / cut_hi: that end of axis 0 is a slab interface with ghost
 * planes beyond it (multi-GPU), not a wall, as in odil_interp_adj_cut. */
int odil_poisson_adjoint_transpose_adam_f64(const double* fu, double* g0, double* g1, const int64_t* fshape,
                                            const double* h2, double scale, double* x0, double* m0, double* v0,
                                            double* x1, double* m1, double* v1, double alpha, double one_minus_b1,
                                            double one_minus_b2, double eps, const double* alpha_dev, int cut_lo,
                                            int cut_hi, void* stream);
int odil_poisson_adjoint_transpose_adam_f32(const float* fu, float* g0, float* g1, const int64_t* fshape,
                                            const float* h2, float scale, float* x0, float* m0, float* v0, float* x1,
                                            float* m1, float* v1, float alpha, float one_minus_b1, float one_minus_b2,
                                            float eps, const float* alpha_dev, int cut_lo, int cut_hi, void* stream);
/* The same launch with an explicit cut of the coarse z axis (Z = fshape[0] / 2 planes) into units of work: planes
 * [0, Zs) in chunks of L, planes [Zs, Z) in chunks of S, 1 <= S <= L <= 64, 0 <= Zs <= Z; the long chunks are
 * dispatched first.  Every plan gives the same bits; L <= 0 takes the plan the entry points above take, which
 * odil_tile_sched_rule(fshape, 0, plan) writes to plan[0 .. 2] = (L, Zs, S) (Zs == Z: one tier); kind 1: the plan of
 * odil_interp_adj on a 'ccc' array of doubles of that fine shape, where the LDS-tile kernel serves it. */
int odil_poisson_adjoint_transpose_adam_plan_f64(const double* fu, double* g0, double* g1, const int64_t* fshape,
                                                 const double* h2, double scale, double* x0, double* m0, double* v0,
                                                 double* x1, double* m1, double* v1, double alpha, double one_minus_b1,
                                                 double one_minus_b2, double eps, const double* alpha_dev, int cut_lo,
                                                 int cut_hi, int L, int Zs, int S, void* stream);
int odil_poisson_adjoint_transpose_adam_plan_f32(const float* fu, float* g0, float* g1, const int64_t* fshape,
                                                 const float* h2, float scale, float* x0, float* m0, float* v0, float* x1,
                                                 float* m1, float* v1, float alpha, float one_minus_b1,
                                                 float one_minus_b2, float eps, const float* alpha_dev, int cut_lo,
                                                 int cut_hi, int L, int Zs, int S, void* stream);
int odil_tile_sched_rule(const int64_t* fshape, int kind, int* plan);
/* Host only: the units of that schedule for Z planes and Y x XS tiles.  Returns the number of workgroups (-1: not a
 * plan) and writes (z0, z1, y, xs) of workgroup b to units[4 b ..], -1 four times for a workgroup without a unit,
 * for b < capacity.  It walks the kernels' own decode. */
int64_t odil_tile_sched_units(int64_t Z, int64_t Y, int64_t XS, int L, int64_t Zs, int S, int32_t* units,
                              int64_t capacity);
/* One damped-Jacobi sweep of that operator: uout = u - omega (A u - rhs) / diag(A), uout != u.  The
 * smoother of the geometric multigrid that solves the Newton system of the Poisson stencil
 * (reference linsolver.py:61-72 hands that system to pyamg).  u == NULL here and in the two-sweep form below: the sweeps
 * start from the ZERO vector (every coarse level of a V-cycle) -- u is neither read nor need it be zeroed by the caller;
 * the results are those of the same call on an array of zeros, bit for bit. */
int odil_poisson_jacobi_f64(const double* u, const double* rhs, double* uout, const int64_t* shape, int ndim,
                            const double* h2, double omega, void* stream);
int odil_poisson_jacobi_f32(const float* u, const float* rhs, float* uout, const int64_t* shape, int ndim,
                            const float* h2, float omega, void* stream);

/* TWO sweeps of odil_poisson_jacobi, with the weights omega1 and then omega2, in ONE pass over memory: the intermediate iterate
 * stays on the CU (registers along z, lane shifts along x, LDS along y), so a pair of sweeps moves the 3 words per cell
 * of one.  uout != u; bit-identical to two calls of odil_poisson_jacobi.  The last extent must be a multiple of the
 * 16-byte pack (2 doubles / 4 floats).  zc_hint: planes per workgroup chunk, <= 0: automatic.  (Multigrid smoother of
 * the Newton solve; the reference hands that system to SuperLU / pyamg, linsolver.py:17-26, 61-72.) */
int odil_poisson_jacobi2_f64(const double* u, const double* rhs, double* uout, const int64_t* shape, int ndim,
                             const double* h2, double omega1, double omega2, int zc_hint, void* stream);
int odil_poisson_jacobi2_f32(const float* u, const float* rhs, float* uout, const int64_t* shape, int ndim,
                             const float* h2, float omega1, float omega2, int zc_hint, void* stream);

/* The coarse-grid correction of a V-cycle and BOTH post-smoothing sweeps in one pass: two sweeps of odil_poisson_jacobi
 * (weights omega1, omega2) of u = x + P coarse, the prolongation formed on the fly (never stored), the first sweep kept
 * on the CU.  Bit-identical to odil_interp_add followed by odil_poisson_jacobi2.  3-D; coarse: shape cshape, x / rhs /
 * xout: 2 * cshape, xout != x; h2: squared FINE steps.  3 1/8 words per fine cell (separately: 2 1/8 + 6). */
int odil_poisson_jacobi2_synth_f64(const double* coarse, const double* x, const double* rhs, double* xout,
                                   const int64_t* cshape, const double* h2, double omega1, double omega2, int zc_hint,
                                   void* stream);
int odil_poisson_jacobi2_synth_f32(const float* coarse, const float* x, const float* rhs, float* xout,
                                   const int64_t* cshape, const float* h2, float omega1, float omega2, int zc_hint,
                                   void* stream);

/* The same residual with the LAST prolongation of the multigrid synthesis fused in: u = w0 + P coarse
 * (reference core.py:245-263, last step) is formed in registers and never stored.  `coarse`: the
 * synthesised level-1 array of shape cshape (3-D, all axes cell-centred), w0 / rhs / fu: the fine
 * arrays of shape 2 * cshape, h2: squared FINE steps.  fu is bit-identical to
 * odil_interp_add + odil_poisson_residual.  Loss = sum over the fine planes z0 <= z < z1 (z1 < 0:
 * all) of fu^2 / denom (denom <= 0: the array size), as odil_poisson_residual_slab.  fu == NULL: loss only.
 * `partials`: odil_reduce_workspace_bytes() scratch; `column_sums`: scratch of column_sums_size >=
 * odil_poisson_residual_synth_workspace_bytes(cshape) bytes (0: a shape the entry point refuses) -- the sum of squares
 * of every coarse column and z-chunk, which a second launch reduces in a fixed order (deterministic; nothing is
 * allocated by the call). */
size_t odil_poisson_residual_synth_workspace_bytes(const int64_t* cshape);
int odil_poisson_residual_synth_f64(const double* coarse, const double* w0, const double* rhs, double* fu,
                                    const int64_t* cshape, const double* h2, int64_t z0, int64_t z1, double denom,
                                    double* partials, double* column_sums, size_t column_sums_size, double* loss,
                                    void* stream);
int odil_poisson_residual_synth_f32(const float* coarse, const float* w0, const float* rhs, float* fu,
                                    const int64_t* cshape, const float* h2, int64_t z0, int64_t z1, double denom,
                                    double* partials, double* column_sums, size_t column_sums_size, float* loss,
                                    void* stream);

/* One damped-Jacobi sweep (odil_poisson_jacobi) of u = x + P coarse with the prolongation formed in registers:
 * the coarse-grid correction of a V-cycle and its first post-smoothing sweep in one pass, xout != x.  Equal, bit for
 * bit, to odil_interp_add followed by odil_poisson_jacobi.  Shapes as odil_poisson_residual_synth.  (The reference
 * hands the Newton system to pyamg, linsolver.py:61-72.) */
int odil_poisson_jacobi_synth_f64(const double* coarse, const double* x, const double* rhs, double* xout,
                                  const int64_t* cshape, const double* h2, double omega, void* stream);
int odil_poisson_jacobi_synth_f32(const float* coarse, const float* x, const float* rhs, float* xout,
                                  const int64_t* cshape, const float* h2, float omega, void* stream);

/* gu = J^T (scale * fu): cotangent of the operator above; scale = 2/size gives
 * d mean(fu^2)/du (core.py:1093-1101). */
int odil_poisson_adjoint_f64(const double* fu, double* gu, const int64_t* shape, int ndim, const double* h2,
                             double scale, void* stream);
int odil_poisson_adjoint_f32(const float* fu, float* gu, const int64_t* shape, int ndim, const float* h2,
                             float scale, void* stream);
/* The same adjoint with the Adam update of the array that gu is the gradient of fused in
 * (AdamNativeOptimizer._step, optimizer.py:316-318, applied by the lane that forms gu[i]):
 * gu is still written (the P^T chain reads it); x, m, v are updated in place. */
int odil_poisson_adjoint_adam_f64(const double* fu, double* gu, double* x, double* m, double* v, const int64_t* shape,
                                  int ndim, const double* h2, double scale, double alpha, double one_minus_b1,
                                  double one_minus_b2, double eps, const double* alpha_dev, void* stream);
int odil_poisson_adjoint_adam_f32(const float* fu, float* gu, float* x, float* m, float* v, const int64_t* shape,
                                  int ndim, const float* h2, float scale, float alpha, float one_minus_b1,
                                  float one_minus_b2, float eps, const float* alpha_dev, void* stream);
/* Per-shift Jacobian coefficient arrays d(sum fu)/d u_shift as
 * `Problem.eval_operator_grad` returns them under `distinct_shift`
 * (core.py:1313-1361): coeffs holds 2*ndim+1 arrays of `shape`, order
 * [centre, (-1 axis 0), (+1 axis 0), (-1 axis 1), ...]. */
int odil_poisson_jac_coeffs_f64(double* coeffs, const int64_t* shape, int ndim, const double* h2, void* stream);
int odil_poisson_jac_coeffs_f32(float* coeffs, const int64_t* shape, int ndim, const float* h2, void* stream);
/* Are 2 ndim + 1 coefficient arrays (a HOST array of device pointers, the order above) that Jacobian?  One pass over
 * them against the values odil_poisson_jac_coeffs would write, no reference arrays: out[2 k] = max |a_k - e_k|,
 * out[2 k + 1] = max |e_k| (device, 2 (2 ndim + 1) numbers; a NaN stays visible).  The recognition step of the general
 * Newton route (odil_amd/gmg.py: recognise_poisson; the reference has no counterpart: it factorises whatever it is given,
 * linsolver.py:17-26). */
int odil_poisson_jac_match_f64(const double* const* arrays, const int64_t* shape, int ndim, const double* h2,
                               double* partials, double* out, void* stream);
int odil_poisson_jac_match_f32(const float* const* arrays, const int64_t* shape, int ndim, const float* h2, double* partials,
                               float* out, void* stream);

/* ---- optimizers (reference optimizer.py:256-341) ------------------------------ */
/* AdamNativeOptimizer._step (optimizer.py:311-319) on a flat vector:
 *   m += (g-m)*one_minus_b1; v += (g^2-v)*one_minus_b2; x -= (m*alpha)/(sqrt(v)+eps).
 * In this and every *_adam entry point `alpha_dev`, when non-NULL, is a device scalar that replaces
 * `alpha`: the bias-corrected step size changes every epoch, and an epoch captured into a hipGraph
 * must read it from memory (odil_amd/optimizer.py: graph replay of launch-bound epochs). */
int odil_adam_step_f64(double* x, double* m, double* v, const double* g, int64_t n, double alpha,
                       double one_minus_b1, double one_minus_b2, double eps, const double* alpha_dev, void* stream);
int odil_adam_step_f32(float* x, float* m, float* v, const float* g, int64_t n, float alpha, float one_minus_b1,
                       float one_minus_b2, float eps, const float* alpha_dev, void* stream);
/* The same update on `npieces` (<= 65535) contiguous pieces of `count` elements, piece o at o * stride + offset: the
 * planes next to the slab interfaces of a ghost-extended array whose sharded axis is not the leading one (the rest of
 * such an array is updated by the launch that forms its gradient; these planes wait for the neighbour's share). */
int odil_adam_step_pieces_f64(double* x, double* m, double* v, const double* g, int64_t npieces, int64_t stride,
                              int64_t offset, int64_t count, double alpha, double one_minus_b1, double one_minus_b2,
                              double eps, const double* alpha_dev, void* stream);
int odil_adam_step_pieces_f32(float* x, float* m, float* v, const float* g, int64_t npieces, int64_t stride,
                              int64_t offset, int64_t count, float alpha, float one_minus_b1, float one_minus_b2,
                              float eps, const float* alpha_dev, void* stream);
/* The same update on the `nbatch` (1 ... 65535) members of [nbatch, n] arrays, member b at b * stride of each array (the
 * strides, in elements, are at least n: members may be padded): the level-0 update of an ensemble of traced operators,
 * whose gradient a generated gather forms.  Member b reads its step size from the DEVICE array alpha_dev[b *
 * alpha_stride] (alpha_stride 0: one step size for all members) and computes the bits odil_adam_step computes on its
 * own arrays. */
int odil_adam_step_batch_f64(double* x, double* m, double* v, const double* g, int nbatch, int64_t n, int64_t x_stride,
                             int64_t m_stride, int64_t v_stride, int64_t g_stride, double one_minus_b1,
                             double one_minus_b2, double eps, const double* alpha_dev, int64_t alpha_stride,
                             void* stream);
int odil_adam_step_batch_f32(float* x, float* m, float* v, const float* g, int nbatch, int64_t n, int64_t x_stride,
                             int64_t m_stride, int64_t v_stride, int64_t g_stride, float one_minus_b1,
                             float one_minus_b2, float eps, const float* alpha_dev, int64_t alpha_stride, void* stream);
/* The Array unknowns of the `nbatch` (1 ... 65535) members of an ensemble of traced operators, `np` packed parameters
 * per member, in ONE launch.  pgrad[b * pgrad_stride + r], r < npg: the gradient the generated k_loss_batch left for
 * row r of member b's parameter partial sums; map (DEVICE ints): map[b * map_stride + p] is the row of packed parameter
 * p (map_stride 0: one map [np] for all members), any value outside 0 ... npg - 1 (-1 by convention) means that no grid
 * kernel forms a gradient for it.  Writes g[b * np + p] = that gradient (0 where there is none) and applies the update
 * of odil_adam_step -- the same device function -- to x, m, v [nbatch, np] with member b's step size alpha_dev[b *
 * alpha_stride] (alpha_stride 0: one for all).  x, m, v all NULL: only g is formed (the evaluation of an optimizer that
 * is not Adam; alpha_dev may then be NULL). */
int odil_adam_step_params_batch_f64(double* x, double* m, double* v, double* g, const double* pgrad, const int* map,
                                    int nbatch, int64_t np, int npg, int64_t pgrad_stride, int64_t map_stride,
                                    double one_minus_b1, double one_minus_b2, double eps, const double* alpha_dev,
                                    int64_t alpha_stride, void* stream);
int odil_adam_step_params_batch_f32(float* x, float* m, float* v, float* g, const float* pgrad, const int* map, int nbatch,
                                    int64_t np, int npg, int64_t pgrad_stride, int64_t map_stride, float one_minus_b1,
                                    float one_minus_b2, float eps, const float* alpha_dev, int64_t alpha_stride,
                                    void* stream);
/* odil_adam_step_params_batch for members whose operators also have outputs in PARAMETER space (a weight decay, a prior
 * on an Array).  extra [nbatch, np]: what the generated k_par_batch left of member b's gradient -- added to what stood
 * there where a grid kernel forms a gradient too, set where none does.  Forms g[b * np + p] = (the gradient of row
 * map[p], 0 without one) + extra[b * np + p], the sum a single run forms when its k_par adds to its packed gradient,
 * applies the same update (x, m, v all NULL: none), and CLEARS extra, which the next k_par_batch adds to again.  One
 * launch. */
int odil_adam_step_params_extra_batch_f64(double* x, double* m, double* v, double* g, const double* pgrad, double* extra,
                                          const int* map, int nbatch, int64_t np, int npg, int64_t pgrad_stride,
                                          int64_t map_stride, double one_minus_b1, double one_minus_b2, double eps,
                                          const double* alpha_dev, int64_t alpha_stride, void* stream);
int odil_adam_step_params_extra_batch_f32(float* x, float* m, float* v, float* g, const float* pgrad, float* extra,
                                          const int* map, int nbatch, int64_t np, int npg, int64_t pgrad_stride,
                                          int64_t map_stride, float one_minus_b1, float one_minus_b2, float eps,
                                          const float* alpha_dev, int64_t alpha_stride, void* stream);
/* Planes of ghost-extended arrays <-> contiguous message buffers of the slab exchanges (odil_amd/slab.py,
 * slab_traced.py; no reference counterpart).  `descs`: DEVICE array of ndesc (<= 65535) records
 * of five int64 {base, outer, ostride, inner, boff}: plane k of the message is `outer` runs of `inner` contiguous
 * elements of `arr`, run o at base + o * ostride, and the contiguous range [boff, boff + outer * inner) of `buf`.
 * mode 0: buf <- arr (pack); 1: arr <- buf (unpack); 2: arr += buf (halo-add: the transpose of the pack).
 * max_count: the largest outer * inner; vec_ok != 0: every inner is a multiple of 4 (16-byte packs).  One launch. */
int odil_planes_copy_f64(double* arr, double* buf, const int64_t* descs, int ndesc, int64_t max_count, int vec_ok,
                         int mode, void* stream);
int odil_planes_copy_f32(float* arr, float* buf, const int64_t* descs, int ndesc, int64_t max_count, int vec_ok,
                         int mode, void* stream);
/* y += a * x  (GdOptimizer: x -= lr*g, optimizer.py:270; Newton update util.py:177). */
int odil_axpy_f64(double* y, const double* x, int64_t n, double a, void* stream);
int odil_axpy_f32(float* y, const float* x, int64_t n, float a, void* stream);
/* y = a * (adev ? adev[0] : 1) * x: the cotangent of the loss terms, d mean(f^2)/df =
 * (2/n) * gout * f (core.py:1093-1101); `adev` is an optional DEVICE scalar. */
int odil_scale_f64(const double* x, double* y, int64_t n, double a, const double* adev, void* stream);
int odil_scale_f32(const float* x, float* y, int64_t n, float a, const float* adev, void* stream);
/* y = a (.) b (accumulate == 0) or y += a (.) b: one CSR block of the Jacobian applied as
 * coefficient array times gathered field (core.py:1144-1171). */
int odil_addcmul_f64(double* y, const double* a, const double* b, int64_t n, int accumulate, void* stream);
int odil_addcmul_f32(float* y, const float* a, const float* b, int64_t n, int accumulate, void* stream);
/* out[k] = sum_i a[k*lda + i] * b[i], k < nvec, deterministic, f64 accumulation.
 * `partials`: odil_dots_workspace_bytes(nvec) scratch. */
size_t odil_dots_workspace_bytes(int nvec);
int odil_dots_f64(const double* a, int64_t lda, int nvec, const double* b, int64_t n, double* partials,
                  double* out, void* stream);
int odil_dots_f32(const float* a, int64_t lda, int nvec, const float* b, int64_t n, double* partials, float* out,
                  void* stream);
/* out[j*nvec + k] = <a_k, b_j>, j < 3 (b1, b2 may be NULL -> zeros), in one pass over the a_k.
 * `partials`: odil_dots_workspace_bytes(3 * nvec) scratch; `out`: 3 * nvec values. */
int odil_dots3_f64(const double* a, int64_t lda, int nvec, const double* b0, const double* b1, const double* b2,
                   int64_t n, double* partials, double* out, void* stream);
int odil_dots3_f32(const float* a, int64_t lda, int nvec, const float* b0, const float* b1, const float* b2, int64_t n,
                   double* partials, float* out, void* stream);
/* out[0] = <g, d>, out[1] = <g, g>, out[2] = max_i |g[i]| (NaN if any g[i] is NaN) in one pass: what the L-BFGS-B
 * line search and stopping test read after an evaluation (reference optimizer.py:95-105 -> SciPy lnsrlb / projgr).
 * `partials`: odil_dots_workspace_bytes(3) scratch. */
int odil_lbfgs_probe_f64(const double* g, const double* d, int64_t n, double* partials, double* out, void* stream);
int odil_lbfgs_probe_f32(const float* g, const float* d, int64_t n, double* partials, float* out, void* stream);
/* y = beta * y + sum_k coef[k] * a[k*lda + :]  (coef on DEVICE, length nvec). */
int odil_lincomb_f64(double* y, double beta, const double* a, int64_t lda, int nvec, const double* coef, int64_t n,
                     void* stream);
int odil_lincomb_f32(float* y, float beta, const float* a, int64_t lda, int nvec, const float* coef, int64_t n,
                     void* stream);

/* The vector algebra of L-BFGS for an ENSEMBLE of nbatch members in lock-step: member-major [nbatch, n] vectors and a
 * [nbatch, rows, n] history (rows = 2 m: s_k and y_k interleaved), member b of every array at b * <its stride> elements.
 * Every launch covers a LIST of members: `members` is a DEVICE int32 array of nsel member numbers and the member of a
 * workgroup is members[blockIdx.y]; members = NULL means all nbatch members (nsel is ignored).  Members that are not in
 * the list, and the gaps between padded members, are neither read nor written.  Scalars and counts of a member come
 * from DEVICE arrays with one entry per member (entry b, whatever the list), so that one upload serves a round.
 * Member b gets the bits of the single entry point on its own arrays -- the same chunks, the same summation order,
 * both functions of n alone:
 *   odil_lbfgs_probe_batch    out[b * out_stride + 0 .. 2] = odil_lbfgs_probe of g_b, d_b (a NaN in g_b stays visible)
 *   odil_lbfgs_dots3_batch    out[b * out_stride + j * ldo + k] = <a_{b,k}, bj_b> for k < counts[b] (counts = NULL:
 *                             max_count for every member) and j < 3 (b1, b2 may be NULL -> zeros): odil_dots3 with
 *                             nvec = counts[b]; entries k >= counts[b] are left alone.  a_{b,k} at b * a_stride + k * lda.
 *   odil_lbfgs_lincomb_batch  y_b = beta * y_b + sum_{k < counts[b]} coef[b * coef_stride + k] * a_{b,k}, summed in
 *                             the order of odil_lincomb
 *   odil_lbfgs_axpy_batch     out_b = y_b + alpha[b] * x_b (odil_axpy; out may be y); y = NULL: out_b = alpha[b] * x_b
 *                             (odil_scale; out may be x); y = alpha = NULL: out_b = x_b
 *   odil_lbfgs_pair_batch     the correction pair of an accepted step: r_b = g_b - r_b, d_b = stp[b] * d_b and, where
 *                             slot[b] >= 0, rows 2 slot[b] and 2 slot[b] + 1 of w_b = d_b, r_b -- per element what
 *                             odil_scale, odil_axpy and two copies leave behind (no reduction: fusing is free)
 * odil_dots3 picks one of two kernels from n, the alignment of its operands and nvec <= 128.  The batched launcher makes
 * that choice once for the launch, so it refuses, before anything is launched, what would let it differ between
 * members or from a member's single call: member strides or pointers that give members different 16-byte alignment,
 * and max_count > 128 where n and the alignment admit the read-once kernel.  Also refused: null pointers, n < 1, nbatch
 * or nsel outside 1 ... 65535 (nsel = 0 with a list: nothing to do, 0 is returned), nsel > nbatch, max_count outside
 * 1 ... rows (0 ... rows for lincomb), member strides below a member's extent, and a partials workspace shorter than
 * nbatch rows of partials_stride >= odil_lbfgs_batch_partials(n, max_count, elem_size) doubles. */
int64_t odil_lbfgs_batch_partials(int64_t n, int max_count, int elem_size);
int odil_lbfgs_probe_batch_f64(const double* g, int64_t g_stride, const double* d, int64_t d_stride, int64_t n,
                               int nbatch, const int32_t* members, int nsel, double* partials,
                               int64_t partials_stride, int64_t partials_len, double* out, int64_t out_stride,
                               void* stream);
int odil_lbfgs_probe_batch_f32(const float* g, int64_t g_stride, const float* d, int64_t d_stride, int64_t n,
                               int nbatch, const int32_t* members, int nsel, double* partials,
                               int64_t partials_stride, int64_t partials_len, float* out, int64_t out_stride,
                               void* stream);
int odil_lbfgs_dots3_batch_f64(const double* a, int64_t a_stride, int64_t lda, int rows, const int32_t* counts,
                               int max_count, const double* b0, int64_t b0_stride, const double* b1, int64_t b1_stride,
                               const double* b2, int64_t b2_stride, int64_t n, int nbatch, const int32_t* members,
                               int nsel, double* partials, int64_t partials_stride, int64_t partials_len, double* out,
                               int64_t out_stride, int64_t ldo, void* stream);
int odil_lbfgs_dots3_batch_f32(const float* a, int64_t a_stride, int64_t lda, int rows, const int32_t* counts,
                               int max_count, const float* b0, int64_t b0_stride, const float* b1, int64_t b1_stride,
                               const float* b2, int64_t b2_stride, int64_t n, int nbatch, const int32_t* members,
                               int nsel, double* partials, int64_t partials_stride, int64_t partials_len, float* out,
                               int64_t out_stride, int64_t ldo, void* stream);
int odil_lbfgs_lincomb_batch_f64(double* y, int64_t y_stride, double beta, const double* a, int64_t a_stride,
                                 int64_t lda, int rows, const int32_t* counts, int max_count, const double* coef,
                                 int64_t coef_stride, int64_t n, int nbatch, const int32_t* members, int nsel,
                                 void* stream);
int odil_lbfgs_lincomb_batch_f32(float* y, int64_t y_stride, float beta, const float* a, int64_t a_stride, int64_t lda,
                                 int rows, const int32_t* counts, int max_count, const float* coef, int64_t coef_stride,
                                 int64_t n, int nbatch, const int32_t* members, int nsel, void* stream);
int odil_lbfgs_axpy_batch_f64(double* out, int64_t out_stride, const double* y, int64_t y_stride, const double* x,
                              int64_t x_stride, const double* alpha, int64_t n, int nbatch, const int32_t* members,
                              int nsel, void* stream);
int odil_lbfgs_axpy_batch_f32(float* out, int64_t out_stride, const float* y, int64_t y_stride, const float* x,
                              int64_t x_stride, const float* alpha, int64_t n, int nbatch, const int32_t* members,
                              int nsel, void* stream);
int odil_lbfgs_pair_batch_f64(const double* g, int64_t g_stride, double* r, int64_t r_stride, double* d,
                              int64_t d_stride, double* w, int64_t w_stride, int64_t lda, int rows, const double* stp,
                              const int32_t* slot, int64_t n, int nbatch, const int32_t* members, int nsel,
                              void* stream);
int odil_lbfgs_pair_batch_f32(const float* g, int64_t g_stride, float* r, int64_t r_stride, float* d, int64_t d_stride,
                              float* w, int64_t w_stride, int64_t lda, int rows, const float* stp, const int32_t* slot,
                              int64_t n, int nbatch, const int32_t* members, int nsel, void* stream);

/* ---- Newton: matrix-free normal equations (reference core.py:1113-1217,
 *      linsolver.py:17-26) ------------------------------------------------------- */
/* y = M x  where row r of M has coefficients coeffs[s][r] on columns roll(-shift_s):
 * the CSR matrix `field_to_matrix` builds (core.py:1144-1171), kept as coefficient
 * arrays.  `shifts`: nshift*ndim int64. transpose != 0 applies M^T. */
int odil_stencil_apply_f64(const double* coeffs, const int64_t* shifts, int nshift, const double* x, double* y,
                           const int64_t* shape, int ndim, int transpose, void* stream);
int odil_stencil_apply_f32(const float* coeffs, const int64_t* shifts, int nshift, const float* x, float* y,
                           const int64_t* shape, int ndim, int transpose, void* stream);
/* x = M^-1 b for such a matrix when it is triangular along `axis` with the coefficient array `diag` (zero shift)
 * alone on the diagonal block -- the Jacobian of an operator that is explicit in time (wave): every other shift has
 * a negative (direction > 0, forward substitution) or positive (direction < 0) component along `axis`, of size below
 * the extent (other shifts, and direction 0, are refused), and no coefficient that wraps around the ends.  M d = -r
 * then has the solution of the normal equations M^T M d = -M^T r the reference hands to SuperLU (linsolver.py:17-26).
 * One launch per level of `axis`. */
int odil_stencil_march_f64(const double* coeffs, const int64_t* shifts, int nshift, int diag, const double* b, double* x,
                           const int64_t* shape, int ndim, int axis, int direction, void* stream);
int odil_stencil_march_f32(const float* coeffs, const int64_t* shifts, int nshift, int diag, const float* b, float* x,
                           const int64_t* shape, int ndim, int axis, int direction, void* stream);
/* Geometric multigrid for a (2 ndim + 1)-point operator with VARIABLE coefficients on a cell-centred grid, ndim <= 3 (the
 * Newton system of any single-field operator whose Jacobian `Problem.linearize` delivers as per-shift coefficient arrays,
 * core.py:1113-1217; the reference hands M^T M to SuperLU / pyamg, linsolver.py:17-26, 61-72).  `coeffs`: the 2 ndim + 1
 * arrays one after another in the order (0, -e_0, +e_0, -e_1, +e_1, ...), each of `shape`; neighbours wrap periodically
 * (core.py:962-963), a wall row carries a zero coefficient towards the wall.
 *   smooth, mode 0:  out = x - omega (A x - b) / c0   (one damped-Jacobi sweep; out != x).  x == NULL (here and in
 *           odil_stencil_var_smooth2): the sweeps start from the ZERO vector, x is not read -- for finite coefficients the
 *           bits of the same call on an array of zeros
 *           mode 1:  out = b - A x
 *   residual_restrict: coarse = scale * sum over the 2^ndim children of (b - A x), loss = mean((A x - b)^2)
 *           (deterministic two-stage sum; `partials`: odil_reduce_workspace_bytes(); loss == NULL: no reduction launch);
 *           even extents
 *   coarsen: the coarse-grid operator as 2 ndim + 1 arrays of shape / 2: aggregates of 2^ndim cells, piecewise-constant
 *           Galerkin products of the second-order part (x 1/2), the matrix-antisymmetric part and the row sums
 *           (csrc/stencil_mg.hip). */
int odil_stencil_var_smooth_f64(const double* coeffs, const double* x, const double* b, double* out, const int64_t* shape,
                                int ndim, double omega, int mode, void* stream);
int odil_stencil_var_smooth_f32(const float* coeffs, const float* x, const float* b, float* out, const int64_t* shape,
                                int ndim, float omega, int mode, void* stream);
int odil_stencil_var_residual_restrict_f64(const double* coeffs, const double* x, const double* b, double* coarse,
                                           const int64_t* shape, int ndim, double scale, double* partials, double* loss,
                                           void* stream);
int odil_stencil_var_residual_restrict_f32(const float* coeffs, const float* x, const float* b, float* coarse,
                                           const int64_t* shape, int ndim, float scale, double* partials, float* loss,
                                           void* stream);
/* slab variant: the norm over the planes z0 <= z < z1 only, divided by denom (conventions of the Poisson one above) */
int odil_stencil_var_residual_restrict_slab_f64(const double* coeffs, const double* x, const double* b, double* coarse,
                                                const int64_t* shape, int ndim, double scale, int64_t z0, int64_t z1,
                                                double denom, double* partials, double* loss, void* stream);
int odil_stencil_var_residual_restrict_slab_f32(const float* coeffs, const float* x, const float* b, float* coarse,
                                                const int64_t* shape, int ndim, float scale, int64_t z0, int64_t z1,
                                                double denom, double* partials, float* loss, void* stream);
int odil_stencil_var_coarsen_f64(const double* coeffs, double* coarse, const int64_t* shape, int ndim, void* stream);
int odil_stencil_var_coarsen_f32(const float* coeffs, float* coarse, const int64_t* shape, int ndim, void* stream);
/* ... merging two cells along the axes with halve[i] != 0 only (semi-coarsening: the strongly coupled axes of an anisotropic
 * operator; coarse shape = shape / 2 on those axes, shape on the others).  The factor 1/2 of the second-order part goes with
 * the merged axes; with every axis merged this is odil_stencil_var_coarsen. */
int odil_stencil_var_coarsen_axes_f64(const double* coeffs, double* coarse, const int64_t* shape, int ndim, const int* halve,
                                      void* stream);
int odil_stencil_var_coarsen_axes_f32(const float* coeffs, float* coarse, const int64_t* shape, int ndim, const int* halve,
                                      void* stream);
/* The set-up of the hierarchies of an ENSEMBLE (gmg.EnsembleGMG.from_coeffs): `nbatch` (1..65535) operators of one shape,
 * member b's 2 ndim + 1 coefficient arrays starting b * coeff_stride ELEMENTS after member 0's (coeff_stride >= one
 * member), every entry point ONE launch whatever nbatch.  Malformed arguments are refused before any launch.  (No
 * reference counterpart: the reference sets up one solver at a time, linsolver.py:61-72.)
 *   coarsen_batch   the coarse operator of every member, written coarse_stride elements apart: per member bit-identical to
 *                   odil_stencil_var_coarsen where halve is NULL or all ones, to odil_stencil_var_coarsen_axes otherwise
 *                   (the same device code on the member's arrays)
 *   strength_batch  out[b, k] = max |c| of member b's off-centre array 1 + k (k < 2 ndim): the values of odil_max_abs_rows
 *                   on those arrays (a maximum is exact in any order; a NaN propagates), one workgroup per (member, array)
 *   dense_batch     dense[b, r, j] = (A_b e_j)[r], the dense n x n matrix of member b's operator with periodic wrap, n =
 *                   cells <= 512: entry by entry the value mode 1 of odil_stencil_var_smooth gives for the unit vectors */
int odil_stencil_var_coarsen_batch_f64(const double* coeffs, int64_t coeff_stride, double* coarse, int64_t coarse_stride,
                                       const int64_t* shape, int ndim, const int* halve, int nbatch, void* stream);
int odil_stencil_var_coarsen_batch_f32(const float* coeffs, int64_t coeff_stride, float* coarse, int64_t coarse_stride,
                                       const int64_t* shape, int ndim, const int* halve, int nbatch, void* stream);
int odil_stencil_strength_batch_f64(const double* coeffs, int64_t coeff_stride, const int64_t* shape, int ndim, int nbatch,
                                    double* out, void* stream);
int odil_stencil_strength_batch_f32(const float* coeffs, int64_t coeff_stride, const int64_t* shape, int ndim, int nbatch,
                                    float* out, void* stream);
int odil_stencil_dense_batch_f64(const double* coeffs, int64_t coeff_stride, const int64_t* shape, int ndim, int nbatch,
                                 double* dense, void* stream);
int odil_stencil_dense_batch_f32(const float* coeffs, int64_t coeff_stride, const int64_t* shape, int ndim, int nbatch,
                                 float* dense, void* stream);
/* The CYCLE of an ensemble on levels too large for one workgroup (gmg.EnsembleLaunchGMG): the conventions of the set-up
 * entry points above (the member on blockIdx.y, nbatch 1..65535, every *_stride in ELEMENTS and >= one member, malformed
 * arguments refused before any launch).  A member runs the device code of the single entry point on its own arrays: its
 * output is bit-identical to that entry point on them alone.  No workgroup waits for, signals or reads what another one
 * writes: no grid barrier, no counter, no atomic.  `active`: NULL, or int[nbatch] on the device; the workgroups of a member
 * with active[b] == 0 return before any load or store.  (No reference counterpart: the reference solves one system at a
 * time, linsolver.py:17-26, 61-72.)
 *   smooth_batch   odil_stencil_var_smooth for every member: mode 0 the damped Jacobi sweep (x == NULL: from the zero
 *                  vector; out != x), mode 1 out = b - A x.  partials (mode 0 only): NULL, or double[nbatch, P] with P =
 *                  odil_stencil_var_smooth_batch_parts(shape, ndim): workgroup p of member b leaves the sum, in double, of
 *                  (A x - b)^2 over its cells -- the residual of the sweep's INPUT (x == NULL: b^2), which the sweep forms
 *                  anyway.  P and the cells of a workgroup depend on the shape alone, never on nbatch.
 *   smooth_batch_parts   P (one partial sum per 256 cells), 0 for malformed shapes
 *   residual_restrict_batch   coarse = scale * sum over the 2^ndim children of (b - A x) for every member: every axis
 *                  merged, even extents, even strides between members (the two children along the last axis are read as
 *                  one aligned pack); no norm
 *   cycle_decide_batch   the decision before cycle k, one workgroup per member still active: history[b, 1 + k] = (the
 *                  member's nparts partial sums, added in a fixed order) / cells; with partials0 != NULL also history[b, 0]
 *                  from those; then the stop rules of odil_stencil_solve_batch, verbatim -- 0 converged (history[1 + k] <=
 *                  tol^2 history[0]), 1 k == maxcycles, 2 stagnated (k >= 3 and history[1 + k] >= 0.98^2 history[k]), 3 a
 *                  non-finite norm.  A member that stops gets outcome[b] = (k, reason) and active[b] = 0; a member that is
 *                  inactive already is left alone.  A second one-workgroup launch then counts the active members into
 *                  *nactive (device memory).  Everything is double or int: no type suffix. */
int odil_stencil_var_smooth_batch_f64(const double* coeffs, int64_t coeff_stride, const double* x, int64_t x_stride,
                                      const double* b, int64_t b_stride, double* out, int64_t out_stride, const int64_t* shape,
                                      int ndim, int nbatch, double omega, int mode, const int* active, double* partials,
                                      void* stream);
int odil_stencil_var_smooth_batch_f32(const float* coeffs, int64_t coeff_stride, const float* x, int64_t x_stride,
                                      const float* b, int64_t b_stride, float* out, int64_t out_stride, const int64_t* shape,
                                      int ndim, int nbatch, float omega, int mode, const int* active, double* partials,
                                      void* stream);
int64_t odil_stencil_var_smooth_batch_parts(const int64_t* shape, int ndim);
int odil_stencil_var_residual_restrict_batch_f64(const double* coeffs, int64_t coeff_stride, const double* x, int64_t x_stride,
                                                 const double* b, int64_t b_stride, double* coarse, int64_t coarse_stride,
                                                 const int64_t* shape, int ndim, int nbatch, double scale, const int* active,
                                                 void* stream);
int odil_stencil_var_residual_restrict_batch_f32(const float* coeffs, int64_t coeff_stride, const float* x, int64_t x_stride,
                                                 const float* b, int64_t b_stride, float* coarse, int64_t coarse_stride,
                                                 const int64_t* shape, int ndim, int nbatch, float scale, const int* active,
                                                 void* stream);
int odil_stencil_cycle_decide_batch(const double* partials, int64_t partials_stride, const double* partials0,
                                    int64_t partials0_stride, int nparts, int nbatch, int64_t cells, int k, int maxcycles,
                                    double tol, double* history, int64_t history_stride, int* outcome, int* active,
                                    int* nactive, void* stream);

/* WHOLE EPOCHS of the multigrid Poisson problem (1-D or 2-D, all axes cell-centred) in ONE launch: one workgroup walks
 * synthesis, residual + loss, adjoint, transposed prolongations and the Adam update of every level -- the 17 dependent
 * launches of a 1-D N = 256 epoch -- `nepochs` times, the state resident in LDS when it fits.  Every phase repeats the
 * arithmetic of the kernel it replaces and the loss is summed in the order of the two-stage reduction: the trajectory is
 * bit-identical to the multi-launch path.
 *   x, m, v, g   packed vectors of all levels, finest first (unknowns, Adam moments, gradient: all updated)
 *   u            scratch of the same length (the synthesised field of every level; level 0 = the field u)
 *   fu, rhs      residual (out) and right-hand side on the finest level
 *   shapes       nlvl x ndim extents, each level half the one before; h2: squared steps of the finest level
 *   alphas       DEVICE array of nepochs step sizes lr sqrt(1 - b2^t) / (1 - b1^t); losses: DEVICE array, the loss each
 *                epoch evaluated (before its update), norms: their square roots; partials: the reduction workspace
 * Reference: core.py:245-263, 606-700; examples/poisson/poisson.py:57-113; core.py:1093-1100; optimizer.py:311-336. */
/* 1 when odil_poisson_small_epochs keeps the state of these levels in LDS for the whole launch (elem_size 4 / 8 bytes):
 * x, m, v, the gradient (= the synthesis scratch) of all levels, residual and right-hand side of the finest -- 156 KB. */
int odil_poisson_small_epochs_resident(const int64_t* shapes, int nlvl, int ndim, int elem_size);
int odil_poisson_small_epochs_f64(double* x, double* m, double* v, double* g, double* u, double* fu, const double* rhs,
                                  const int64_t* shapes, int nlvl, int ndim, const double* h2, const double* alphas,
                                  int nepochs, double one_minus_b1, double one_minus_b2, double eps, double* losses,
                                  double* norms, double* partials, void* stream);
int odil_poisson_small_epochs_f32(float* x, float* m, float* v, float* g, float* u, float* fu, const float* rhs,
                                  const int64_t* shapes, int nlvl, int ndim, const float* h2, const float* alphas,
                                  int nepochs, float one_minus_b1, float one_minus_b2, float eps, float* losses,
                                  float* norms, double* partials, void* stream);

/* An ENSEMBLE of nbatch such problems in ONE launch: workgroup b runs member b for nepochs epochs -- exactly the
 * per-workgroup code of odil_poisson_small_epochs on pointers offset by the member strides, so every member's result
 * equals its single launch bit for bit.  Members never communicate (no atomics, no grid-wide synchronisation).
 *   x, m, v, g, u   [nbatch] packed vectors, member b at b * state_stride elements (state_stride >= unknowns of a member)
 *   fu, rhs         [nbatch] finest-level arrays, member b at b * field_stride (>= cells of the finest level)
 *   alphas          member b's nepochs step sizes at b * alpha_stride; alpha_stride = 0: one table shared by all members
 *   losses, norms   member b's nepochs values at b * out_stride (>= nepochs)
 *   partials        reduction workspace, member b's at b * partials_stride doubles
 *                   (>= odil_poisson_small_epochs_partials(shapes, ndim, elem_size))
 * Shapes, h2 and the Adam constants are common to the ensemble.  Null pointers, nbatch < 1, strides smaller than a
 * member, levels that do not halve and a partials workspace that is too small are refused before anything is launched. */
int64_t odil_poisson_small_epochs_partials(const int64_t* shapes, int ndim, int elem_size);
int odil_poisson_small_epochs_batch_f64(double* x, double* m, double* v, double* g, double* u, double* fu, const double* rhs,
                                        int nbatch, int64_t state_stride, int64_t field_stride, const int64_t* shapes,
                                        int nlvl, int ndim, const double* h2, const double* alphas, int64_t alpha_stride,
                                        int nepochs, double one_minus_b1, double one_minus_b2, double eps, double* losses,
                                        double* norms, int64_t out_stride, double* partials, int64_t partials_stride,
                                        void* stream);
int odil_poisson_small_epochs_batch_f32(float* x, float* m, float* v, float* g, float* u, float* fu, const float* rhs,
                                        int nbatch, int64_t state_stride, int64_t field_stride, const int64_t* shapes,
                                        int nlvl, int ndim, const float* h2, const float* alphas, int64_t alpha_stride,
                                        int nepochs, float one_minus_b1, float one_minus_b2, float eps, float* losses,
                                        float* norms, int64_t out_stride, double* partials, int64_t partials_stride,
                                        void* stream);

/* An ENSEMBLE of nbatch Poisson problems of ANY 1-D / 2-D size as batched launches: every launch of a single problem's
 * epoch (odil_mg_synth, odil_poisson_residual, odil_poisson_adjoint_adam, odil_mg_synth_adj_adam) covers all members.
 * Member b is blockIdx.y = b of the stencil kernels and runs exactly the single kernel's walk on pointers offset by
 * the member strides; its partial sums go to row b of the partials workspace and are summed in the single launch's
 * order, so losses and states equal the single run's bit for bit.  Members never communicate.
 *   u, rhs, fu, g, x, m, v   member b at b * <its stride> elements (stride >= cells of a member and a multiple of 16
 *                            bytes: every member must start where member 0's 16-byte packs do)
 *   partials                 partials_len doubles, member b's row at b * partials_stride
 *                            (partials_stride >= odil_poisson_batch_partials(shape, ndim, elem_size))
 *   loss                     [nbatch] mean(fu[b]^2)
 *   alpha_dev                DEVICE step sizes, member b's at b * alpha_stride; alpha_stride = 0: one for all members
 * The transfers need no entry points of their own: the synthesis is odil_mg_synth on [nbatch, *shape] arrays with loc
 * '.' + loc, the transposed chain with the updates odil_mg_synth_adj_adam_members, declared below, with nrows = nbatch, loc 'c' or
 * 'cc'; odil_mg_members_levels_ok says from the shapes alone whether a batch may run them, so that a host can refuse
 * it before its first launch.
 * Refused before anything is launched: null pointers, nbatch outside 1 ... 65535, ndim outside 1 ... 2, a member stride
 * below a member's size or off the 16-byte grid, a partials workspace shorter than nbatch rows. */
int64_t odil_poisson_batch_partials(const int64_t* shape, int ndim, int elem_size);
int odil_poisson_residual_batch_f64(const double* u, const double* rhs, double* fu, int nbatch, int64_t u_stride,
                                    int64_t rhs_stride, int64_t fu_stride, const int64_t* shape, int ndim,
                                    const double* h2, double* partials, int64_t partials_stride, int64_t partials_len,
                                    double* loss, void* stream);
int odil_poisson_residual_batch_f32(const float* u, const float* rhs, float* fu, int nbatch, int64_t u_stride,
                                    int64_t rhs_stride, int64_t fu_stride, const int64_t* shape, int ndim, const float* h2,
                                    double* partials, int64_t partials_stride, int64_t partials_len, float* loss,
                                    void* stream);
int odil_poisson_adjoint_adam_batch_f64(const double* fu, double* gu, double* x, double* m, double* v, int nbatch,
                                        int64_t fu_stride, int64_t g_stride, int64_t x_stride, int64_t m_stride,
                                        int64_t v_stride, const int64_t* shape, int ndim, const double* h2, double scale,
                                        double one_minus_b1, double one_minus_b2, double eps, const double* alpha_dev,
                                        int64_t alpha_stride, void* stream);
int odil_poisson_adjoint_adam_batch_f32(const float* fu, float* gu, float* x, float* m, float* v, int nbatch,
                                        int64_t fu_stride, int64_t g_stride, int64_t x_stride, int64_t m_stride,
                                        int64_t v_stride, const int64_t* shape, int ndim, const float* h2, float scale,
                                        float one_minus_b1, float one_minus_b2, float eps, const float* alpha_dev,
                                        int64_t alpha_stride, void* stream);

/* An ENSEMBLE of nbatch 3-D Poisson problems of one shape as batched launches: every launch of a single 3-D problem's
 * epoch (odil_mg_synth on the coarse levels, odil_poisson_residual_synth, odil_poisson_adjoint_adam,
 * odil_mg_synth_adj_adam) covers all members.  Member b is blockIdx.y = b of the residual and stencil kernels and runs
 * exactly the single kernel's walk on pointers offset by the member strides; its column sums and partial sums go to its
 * own part of the workspaces and are reduced in the single launch's order (k_synth_loss_replay, the final reduction),
 * so losses and states equal the single run's bit for bit.  Members never communicate.
 *   coarse                   [nbatch, *cshape] contiguous: the synthesis of the levels 1 ... (level 1 itself when nlvl = 2)
 *   w0, rhs, fu, g, x, m, v  member b at b * <its stride> elements (stride >= cells of a member and a multiple of 16
 *                            bytes); shape = 2 * cshape
 *   partials                 partials_len doubles, member b's row at b * partials_stride
 *                            (partials_stride >= odil_poisson_residual_synth_batch_partials(cshape))
 *   column_sums              nbatch * odil_poisson_residual_synth_batch_workspace_bytes(cshape) bytes (the query: per member)
 *   loss                     [nbatch] mean(fu[b]^2) over the full plane range (there is no slab form)
 *   alpha_dev                DEVICE step sizes, member b's at b * alpha_stride; alpha_stride = 0: one for all members
 * odil_poisson_adjoint_adam_volumes is odil_poisson_adjoint_adam_batch for ndim = 3 (gu = NULL: the gradient is not
 * stored).  The transposed chain with the updates is odil_mg_synth_adj_adam_members, declared below, with nrows = nbatch, loc
 * 'ccc': a level runs the rows, tile, marching or fast kernel that the same level of a single volume runs on the
 * [nbatch, *shape] array as '.ccc', and that kernel reads the step size of its volume.
 * Refused before anything is launched: null pointers, nbatch outside 1 ... 65535, ndim != 3, a member stride below a
 * member's size or off the 16-byte grid, a partials or column-sum workspace that is too short, a grid beyond one launch.
 * odil_interp_adj_kind names the transposed prolongation odil_interp_adj runs for a coarse shape and layout on arrays
 * aligned to 16 bytes, nothing launched: 0 the generic kernel, 1 the fast kernel, 2 a node-centred marching kernel, 3 the
 * row-marching kernel (float), 4 the LDS-tile kernel, 5 the z-marching kernel; negative: an error.  Kernels 3, 4 and 5
 * round differently in float. */
int odil_interp_adj_kind(const int64_t* cshape, int ndim, const char* loc, int elem_size);
size_t odil_poisson_residual_synth_batch_workspace_bytes(const int64_t* cshape);
int64_t odil_poisson_residual_synth_batch_partials(const int64_t* cshape);
int odil_poisson_residual_synth_batch_f64(const double* coarse, const double* w0, const double* rhs, double* fu,
                                          int nbatch, int64_t w0_stride, int64_t rhs_stride, int64_t fu_stride,
                                          const int64_t* cshape, int ndim, const double* h2, double* partials,
                                          int64_t partials_stride, int64_t partials_len, double* column_sums,
                                          size_t column_sums_size, double* loss, void* stream);
int odil_poisson_residual_synth_batch_f32(const float* coarse, const float* w0, const float* rhs, float* fu, int nbatch,
                                          int64_t w0_stride, int64_t rhs_stride, int64_t fu_stride,
                                          const int64_t* cshape, int ndim, const float* h2, double* partials,
                                          int64_t partials_stride, int64_t partials_len, double* column_sums,
                                          size_t column_sums_size, float* loss, void* stream);
int odil_poisson_adjoint_adam_volumes_f64(const double* fu, double* gu, double* x, double* m, double* v, int nbatch,
                                          int64_t fu_stride, int64_t g_stride, int64_t x_stride, int64_t m_stride,
                                          int64_t v_stride, const int64_t* shape, int ndim, const double* h2,
                                          double scale, double one_minus_b1, double one_minus_b2, double eps,
                                          const double* alpha_dev, int64_t alpha_stride, void* stream);
int odil_poisson_adjoint_adam_volumes_f32(const float* fu, float* gu, float* x, float* m, float* v, int nbatch,
                                          int64_t fu_stride, int64_t g_stride, int64_t x_stride, int64_t m_stride,
                                          int64_t v_stride, const int64_t* shape, int ndim, const float* h2, float scale,
                                          float one_minus_b1, float one_minus_b2, float eps, const float* alpha_dev,
                                          int64_t alpha_stride, void* stream);
/* The transposed prolongation chain of EVERY ensemble that runs as batched launches: [nrows, *shape] level arrays
 * (contiguous, layout '.' + loc) of 1-D to 4-D rows with ANY loc of 'c' / 'n' -- the B members of a Poisson ensemble
 * (loc 'c', 'cc', 'ccc'), or the F grid unknowns of B members as nrows = F B rows, row f B + b.  `shapes` are the
 * nlvl x ndim extents of ONE row.  One launch per level for all rows; the Adam update of the
 * levels >= 1 runs in the launch that forms their gradient, row r with the step size alpha_dev[(r % period) *
 * alpha_stride] (period 0: r itself; alpha_stride 0: one step size for all rows).  x = m = v = NULL: the gradients alone
 * (entry 0 of grads, x, m, v is never touched: the chain reads gu).  A level whose single transpose is the fast or a
 * cell-centred marching kernel runs that kernel on all rows; one whose single transpose is the node-centred marching
 * kernel ('ncc' with four coarse planes or more) runs that kernel row by row, the row on a grid dimension; a level whose
 * single transpose is the generic kernel (a node-centred y or x axis: 'nc', 'cn', 'nn', 'n') runs k_interp_adj_members,
 * the generic kernel's sum per coarse value with the row on a grid dimension and the update in the same thread.  Per row
 * the gradients are the bits of odil_mg_synth_adj on that row alone, x, m, v those of odil_adam_step.
 * All-cell rows ('c', 'cc', 'ccc') are generic only beyond the limits of the fast and the marching kernels: an extent of
 * 2^30 or more, or a schedule that cannot be counted in 31 bits (a 3-D level with fewer than 4 coarse planes is fast, not
 * generic).  Such a level is not refused: it runs k_interp_adj_members with the bits of the single run, like any other
 * generic level.  A level that is NOT generic for one row must be of the same kind on the stacked array: 65535 members
 * of (1 << 25,) -> (1 << 24,), fast alone and generic stacked, are refused, not rerouted.
 * A level of 2^31 elements or more per row is refused where a row kernel, which numbers the elements of a row with an
 * int, could meet it: on every level of rows of four axes or with a node-centred axis, and on a generic level of
 * all-cell rows.  Other levels of all-cell rows of up to three axes run the single launch on the '.' + loc array and
 * have no such limit -- for one unknown per member (the Poisson ensembles never had it) and for several alike.
 * Refused before anything is launched: null pointers (the tables and every level array), nrows outside 1 ... 65535,
 * ndim outside 1 ... 4, a loc with '.', fewer than two levels, levels that do not refine, a coarsest extent below 2,
 * gradient arrays off the 16-byte grid, a negative stride or period, and rows one of whose levels would not compute what
 * that level of a single row computes.
 * odil_mg_members_levels_ok answers the last question -- for this chain and for the prolongation odil_mg_synth runs on
 * the same arrays, whose kernels all sum in the reference's order -- from shapes, loc, nrows and the element size alone
 * (0: they do; else the reason is the error text).
 * Rows of FOUR axes (ndim 4, the (t, x, y, z) arrays of the space-time workloads): the canonical view of the transfer
 * kernels has four axes, so the row cannot ride as a leading '.' axis.  A single 4-D array runs one of three transposes,
 * and each has a row variant with the row on a grid dimension the single kernel does not use, base pointers offset by
 * the row, schedule, arithmetic and summation order those of the single launch: the generic kernel
 * (k_interp_adj_members, which has four row axes: a node-centred y or x axis), the fast kernel (the ROWS instantiations of k_interp_adj_fast)
 * and the 'nccc' marching kernel (the ROWS instantiation of k_interp_adj_march_lead, the row on blockIdx.z).
 * odil_mg_members_levels_ok refuses, naming the level, a level whose single kind is none of these and a level of the
 * latter two kinds whose rows are no multiple of 16 bytes (the kernels read packs, and choose their columns per thread,
 * by the alignment of row 0). */
int odil_mg_members_levels_ok(const int64_t* shapes, int nlvl, int ndim, const char* loc, int nrows, int elem_size);
int odil_mg_synth_adj_adam_members_f64(const double* gu, double* const* grads, const int64_t* shapes, int nlvl, int ndim,
                                       const char* loc, int nrows, double* const* x, double* const* m, double* const* v,
                                       double one_minus_b1, double one_minus_b2, double eps, const double* alpha_dev,
                                       int64_t alpha_stride, int64_t period, void* stream);
int odil_mg_synth_adj_adam_members_f32(const float* gu, float* const* grads, const int64_t* shapes, int nlvl, int ndim,
                                       const char* loc, int nrows, float* const* x, float* const* m, float* const* v,
                                       float one_minus_b1, float one_minus_b2, float eps, const float* alpha_dev,
                                       int64_t alpha_stride, int64_t period, void* stream);
/* The synthesis of odil_mg_synth, all factors 1, on the same [nrows, *shape] level arrays of 1-D to 4-D rows:
 * u[r] = sum_l P^l terms[l][r], one launch per level for all rows.  work[l] (1 <= l <= nlvl-2): scratch of the size of
 * terms[l].  Rows of up to three axes are the '.' + loc call of odil_mg_synth; rows of four axes run the fast
 * prolongation where it takes the layout, else the generic one, with the row on blockIdx.y (the ROWS instantiations of
 * k_interp_add_fast and k_interp_add).  Every prolongation kernel sums in
 * the reference's order, so row r gets the bits of odil_mg_synth on that row alone.  Refused before anything is launched:
 * null pointers, nrows outside 1 ... 65535, ndim outside 1 ... 4, a loc with '.', shapes that do not refine. */
int odil_mg_synth_members_f64(const double* const* terms, double* const* work, double* u, const int64_t* shapes, int nlvl,
                              int ndim, const char* loc, int nrows, void* stream);
int odil_mg_synth_members_f32(const float* const* terms, float* const* work, float* u, const int64_t* shapes, int nlvl,
                              int ndim, const char* loc, int nrows, void* stream);
/* The stencil adjoint of all members WITHOUT an update (the gradient of an ensemble whose optimizer is not Adam):
 * gu[b] = odil_poisson_adjoint of fu[b] for nbatch 1-D, 2-D or 3-D members in one launch, member b = blockIdx.y on the
 * single kernel's walk, bit for bit.  Strides as above (>= cells of a member, multiples of 16 bytes).  Refused before
 * anything is launched: null pointers, nbatch outside 1 ... 65535, ndim outside 1 ... 3, such strides.  The transposed
 * prolongations are odil_mg_synth_adj_adam_members with x = m = v = NULL. */
int odil_poisson_adjoint_batch_f64(const double* fu, double* gu, int nbatch, int64_t fu_stride, int64_t g_stride,
                                   const int64_t* shape, int ndim, const double* h2, double scale, void* stream);
int odil_poisson_adjoint_batch_f32(const float* fu, float* gu, int nbatch, int64_t fu_stride, int64_t g_stride,
                                   const int64_t* shape, int ndim, const float* h2, float scale, void* stream);

/* TWO sweeps of odil_stencil_var_smooth in mode 0, with the weights omega1 and then omega2, in ONE pass: the coefficient arrays -- 7 of
 * the 10 words a sweep moves in 3-D -- are read once for both, the intermediate iterate stays on the CU.  out != x;
 * bit-identical to two calls of odil_stencil_var_smooth.  The last extent must be even.  zc_hint: planes per workgroup
 * chunk, <= 0: automatic. */
int odil_stencil_var_smooth2_f64(const double* coeffs, const double* x, const double* b, double* out, const int64_t* shape,
                                 int ndim, double omega1, double omega2, int zc_hint, void* stream);
int odil_stencil_var_smooth2_f32(const float* coeffs, const float* x, const float* b, float* out, const int64_t* shape,
                                 int ndim, float omega1, float omega2, int zc_hint, void* stream);
/* odil_stencil_var_smooth2 for every member of an ensemble in ONE launch (the member on blockIdx.y, the device code and
 * the bits of the single entry point per member).  Arrays and strides (in elements) as in odil_stencil_var_smooth_batch:
 * member m's coefficient arrays at coeffs + m coeff_stride, its vectors at x + m x_stride, b + m b_stride, out +
 * m out_stride.  x == NULL: every member starts from the zero vector (x is not read, x_stride is ignored).  active: NULL,
 * or int[nbatch]: a member with active[m] == 0 is skipped whole (no load, no store).  The unit schedule is that of one
 * member; with zc_hint <= 0 the chunk length counts the workgroups of all members (where a chunk is cut does not enter
 * the arithmetic).  Refused before anything is launched: what odil_stencil_var_smooth2 refuses, nbatch outside
 * 1 ... 65535, more than 2^24 cells per member, null coeffs / b / out, x == out, a stride smaller than a member, an odd
 * stride (a lane loads packs of two cells: every member begins on a pack boundary). */
int odil_stencil_var_smooth2_batch_f64(const double* coeffs, int64_t coeff_stride, const double* x, int64_t x_stride,
                                       const double* b, int64_t b_stride, double* out, int64_t out_stride,
                                       const int64_t* shape, int ndim, int nbatch, double omega1, double omega2, int zc_hint,
                                       const int* active, void* stream);
int odil_stencil_var_smooth2_batch_f32(const float* coeffs, int64_t coeff_stride, const float* x, int64_t x_stride,
                                       const float* b, int64_t b_stride, float* out, int64_t out_stride,
                                       const int64_t* shape, int ndim, int nbatch, float omega1, float omega2, int zc_hint,
                                       const int* active, void* stream);

/* The COARSE TAIL of a multigrid V-cycle in one launch: one workgroup walks `nlev` <= 8 small levels (pre-smoothing,
 * residual + restriction, dense solve on the coarsest, prolongation + post-smoothing) with a workgroup barrier where a
 * launch boundary used to be (levels of a few thousand cells cost ~7 dependent launches per level and cycle otherwise).
 *   coeffs   the (2 ndim + 1) coefficient arrays of every level, finest first, back to back (layout of
 *            odil_stencil_var_smooth; the Poisson hierarchy passes odil_poisson_jac_coeffs of its levels)
 *   shapes   nlev x ndim extents; halve: (nlev - 1) x ndim, 1 where the transition to the next level merges cell pairs
 *   xin      start iterate on the finest of these levels (NULL: zero), b its right-hand side, xout the result (!= xin, b)
 *   work     >= 3 * (cells of all levels) values of scratch;  inv: ninv x ninv (pseudo-)inverse of the coarsest operator
 *   wpre / wpost   HOST arrays of npre / npost (<= 4) Jacobi weights;  sweep: x' = x - w (A x - b) / c0
 *   fmg      0: one V-cycle from xin;  1: the nested-iteration start (b restricted to every level, every level one cycle
 *            from the interpolated solution of the level below), xin ignored
 * Transfers: mean of the merged children down, the multigrid decomposition's prolongation (reference core.py:606-700,
 * joint ghost rule core.py:640-643) up.  (Newton solve; the reference: SuperLU / pyamg, linsolver.py:17-26, 61-72.) */
int odil_stencil_vcycle_tail_f64(const double* coeffs, const int64_t* shapes, const int* halve, int nlev, int ndim,
                                 const double* xin, const double* b, double* xout, double* work, int64_t work_len,
                                 const double* inv, int ninv, const double* wpre, int npre, const double* wpost,
                                 int npost, int fmg, void* stream);
int odil_stencil_vcycle_tail_f32(const float* coeffs, const int64_t* shapes, const int* halve, int nlev, int ndim,
                                 const float* xin, const float* b, float* xout, float* work, int64_t work_len,
                                 const float* inv, int ninv, const float* wpre, int npre, const float* wpost, int npost,
                                 int fmg, void* stream);
/* Whole multigrid SOLVES of an ENSEMBLE in one launch: `nbatch` (1..65535) small systems of one shape, one workgroup per
 * member, every member walking its hierarchy from the FINEST level with the phases of odil_stencil_vcycle_tail: member b's
 * iterate after k cycles equals k launches of that entry point on its arrays alone, bit for bit.  The workgroup forms the
 * residual norm before every cycle and stops on its own: no host read-back inside the solve.  Members never communicate.
 *   coeffs, shapes, halve, nlev, ndim, inv, ninv, wpre, wpost   as odil_stencil_vcycle_tail, per member
 *   *_stride   elements between members;  coeff_stride / inv_stride 0: one operator / one coarsest inverse for all
 *   x, b       per member the unknowns and the right-hand side of the finest level (x != b)
 *   work       per member odil_stencil_solve_batch_work(shapes, nlev, ndim) = 3 * (cells of all levels) values;
 *              work_len >= (nbatch - 1) work_stride + one member
 *   start      0: zero iterate;  1: the content of x;  2: nested iteration (fmg of odil_stencil_vcycle_tail)
 *   mode       0: solve A x = b.  1: Newton step, x holds u: u <- u - d with A d = A u - b (start 0 or 2); A u - b is
 *              accumulated in double and rounded once (_f32: the residual of an iterative refinement in the wider type)
 *   history    per member >= maxcycles + 2 DOUBLES (also _f32): [0] mean(rhs^2) of the system solved, [1 + k]
 *              mean((A x_k - rhs)^2) before cycle k.  Every thread sums the squares of cells tid, tid + 1024, ... in double,
 *              a fixed-order tree combines them (lanes of a wave, then the 16 waves): deterministic, independent of nbatch
 *   outcome    [nbatch, 2]: cycles run, stop reason -- 0 converged (history[1 + k] <= tol^2 history[0]), 1 k == maxcycles
 *              (0..1000), 2 stagnated (k >= 3 and history[1 + k] >= 0.98^2 history[k]), 3 a non-finite norm
 * Malformed arguments are refused before any launch.  (No reference counterpart: the reference solves one system at a time
 * with SuperLU / pyamg, linsolver.py:17-26, 61-72.) */
int odil_stencil_solve_batch_f64(const double* coeffs, int64_t coeff_stride, const int64_t* shapes, const int* halve, int nlev,
                                 int ndim, int nbatch, double* x, int64_t x_stride, const double* b, int64_t b_stride,
                                 double* work, int64_t work_stride, int64_t work_len, const double* inv, int64_t inv_stride,
                                 int ninv, const double* wpre, int npre, const double* wpost, int npost, int start, int mode,
                                 int maxcycles, double tol, double* history, int64_t history_stride, int* outcome,
                                 void* stream);
int odil_stencil_solve_batch_f32(const float* coeffs, int64_t coeff_stride, const int64_t* shapes, const int* halve, int nlev,
                                 int ndim, int nbatch, float* x, int64_t x_stride, const float* b, int64_t b_stride,
                                 float* work, int64_t work_stride, int64_t work_len, const float* inv, int64_t inv_stride,
                                 int ninv, const float* wpre, int npre, const float* wpost, int npost, int start, int mode,
                                 int maxcycles, float tol, double* history, int64_t history_stride, int* outcome,
                                 void* stream);
/* work elements per member of odil_stencil_solve_batch; 0 if the shapes are malformed */
int64_t odil_stencil_solve_batch_work(const int64_t* shapes, int nlev, int ndim);
/* odil_stencil_solve_batch with a KRYLOV HAND-OVER inside the launch: a member whose cycles stop contracting goes on with
 * GCR(krylov_m) around the same cycle, in its own workgroup -- still one launch and one read-back for the whole ensemble.
 * Arguments as odil_stencil_solve_batch, and
 *   krylov_m   1..8 directions kept between restarts (gmg.EnsembleGMG passes 6)
 *   work       per member odil_stencil_solve_krylov_batch_work(shapes, nlev, ndim, krylov_m) = that of
 *              odil_stencil_solve_batch plus (2 krylov_m + 2) finest-level vectors: the iterate xk, the residual rho, the
 *              directions Z[m] and their images Q[m]
 *   outcome    [nbatch, 3]: passes run (cycles + GCR passes), stop reason, the cycle before which the member was handed
 *              over (-1: never)
 * The decision before cycle k, in this order: 3 a non-finite norm; 0 converged; 1 k == maxcycles; HAND-OVER when k >= 2 and
 * history[1 + k] >= 0.25 history[k] and history[1 + k] > 1e6 tol^2 history[0] (the rule of gmg.PoissonGMG.solve on mean
 * squares); 2 stagnated; else one cycle.  A member that never meets the hand-over rule runs the instruction sequence of
 * odil_stencil_solve_batch on the same buffers: iterate, history and (cycles, reason) are its bits, outcome[b, 2] = -1.
 * After the hand-over every pass is that of gmg.PoissonGMG.solve_krylov: e = one cycle from the ZERO start on rho, z = e,
 * q = A z, classical Gram-Schmidt of (q, z) against the stored (Q_j, Z_j), both scaled by 1 / |q|, a = <q, rho>,
 * xk += a z, rho -= a q, history[1 + k] = mean(rho^2); after krylov_m passes the directions are dropped.  Vectors in the
 * working precision, every product and norm accumulated in double in the fixed order of odil_stencil_solve_batch.  Stop
 * reasons inside GCR: 3 non-finite rho; 4 BREAKDOWN, |q|^2 zero or non-finite (not converged); 1 k == maxcycles; 0 only
 * when the TRUE residual rhs - A xk, formed anew once the recurrence passes the tolerance and written over history[1 + k],
 * passes it too (else GCR restarts from that residual).  The loop is bounded by maxcycles whatever the numbers do.
 * Malformed arguments, krylov_m outside 1..8 and a work array too small for the larger work size are refused before any
 * launch.  (No reference counterpart.) */
int odil_stencil_solve_krylov_batch_f64(const double* coeffs, int64_t coeff_stride, const int64_t* shapes, const int* halve,
                                        int nlev, int ndim, int nbatch, double* x, int64_t x_stride, const double* b,
                                        int64_t b_stride, double* work, int64_t work_stride, int64_t work_len,
                                        const double* inv, int64_t inv_stride, int ninv, const double* wpre, int npre,
                                        const double* wpost, int npost, int start, int mode, int maxcycles, double tol,
                                        double* history, int64_t history_stride, int* outcome, int krylov_m, void* stream);
int odil_stencil_solve_krylov_batch_f32(const float* coeffs, int64_t coeff_stride, const int64_t* shapes, const int* halve,
                                        int nlev, int ndim, int nbatch, float* x, int64_t x_stride, const float* b,
                                        int64_t b_stride, float* work, int64_t work_stride, int64_t work_len,
                                        const float* inv, int64_t inv_stride, int ninv, const float* wpre, int npre,
                                        const float* wpost, int npost, int start, int mode, int maxcycles, float tol,
                                        double* history, int64_t history_stride, int* outcome, int krylov_m, void* stream);
/* work elements per member of odil_stencil_solve_krylov_batch; 0 if the shapes are malformed or krylov_m is not 1..8 */
int64_t odil_stencil_solve_krylov_batch_work(const int64_t* shapes, int nlev, int ndim, int krylov_m);
/* The KRYLOV HAND-OVER for members too large for one workgroup (gmg.EnsembleLaunchKrylovGMG): GCR(krylov_m) around the
 * batched cycle of odil_stencil_var_smooth_batch and its companions, run ACROSS launches in lock-step -- pass k is the same
 * pass for every member -- with every decision on the device.  Decision order, pass algebra and stop reasons are those of
 * odil_stencil_solve_krylov_batch above; conventions those of the batched cycle: the member on blockIdx.y, strides in
 * ELEMENTS and >= one member, nbatch 1..65535, malformed arguments refused before any launch, mask[b] == 0: the workgroups
 * of member b return before any load or store; no workgroup waits for, signals or reads what another one of the same
 * launch writes (no grid barrier, no counter, no atomic).  Products and norms: accumulated in double per workgroup of
 * 1024 consecutive cells, workgroup p of member b leaving quantity j in gpart[b gpart_stride + j P + p] with P =
 * odil_stencil_gcr_batch_parts(cells) (a function of the cells alone; 0: cells outside 1..2^24); the decision adds the P
 * sums in a fixed order (thread t the sums t, t + 256, ..., then lanes, then waves).  gpart_stride >= (krylov_m + 2) P.
 *   store     [nbatch, 2 krylov_m, cells]: per member the directions Z (rows 0 .. m - 1) and their images Q (rows m ..).
 *             The pass k works in the rows slot = k mod krylov_m: before it the cycle has written e into row slot and
 *             odil_stencil_var_smooth_batch in mode 1 with b = 0 t = -A e into row m + slot; the sign is taken on reading.
 *             The j-th oldest of the have[b] kept directions is in the rows (slot - have[b] + j) mod krylov_m.
 *   have      DEVICE int[nbatch]; max_have: the host's bound 0..krylov_m on it (a larger entry is cut; the row of the pass
 *             itself is never read as a kept one).  scal: DEVICE double[nbatch, >= krylov_m + 2]: beta_j, 1 / |q'|, a.
 *   dots      quantity j = <Q_j, q> for j < have[b], q = -t: one pass over q (max_have == 0: nothing to do)
 *   project   q' = q - sum_j beta_j Q_j, z' = e - sum_j beta_j Z_j, in place in the rows of the pass (classical
 *             Gram-Schmidt: every beta from the un-projected q); quantities m, m + 1 = <q', q'>, <q', rho>
 *   update    q = q' scal[m], z = z' scal[m] in place, x += scal[m + 1] z, rho -= scal[m + 1] q; quantity 0 = <rho, rho>
 *   sumsq     quantity 0 = <v, v> (the true residual of a member to verify)
 *   decide    one workgroup per member, double / int only; state: active (the stationary members: the mask of the base
 *             cycle), gcr, fresh (rho = b - A x is to be formed, have = 0), verify, have -- DEVICE int[nbatch] each.
 *             mode 0, before pass k.  Stationary member: odil_stencil_cycle_decide_batch on `partials` with the HAND-OVER
 *               in the order of odil_stencil_solve_krylov_batch: active = 0, gcr = fresh = 1, have = 0, outcome[b, 2] = k.
 *               GCR member: history[b, 1 + k] = quantity 0 / cells, then 3 non-finite; recurrence <= tol^2 history[b, 0]:
 *               verify = fresh = 1, gcr = 0, have = 0; 1 k == maxcycles; have == krylov_m: have = 0.
 *             mode 1: scal[b, j] = the products of `dots`; fresh = 0.
 *             mode 2: |q'|^2 = quantity m zero or non-finite: 4 BREAKDOWN, outcome (k, 4), gcr = 0 -- before `update`
 *               touches the iterate; else scal[b, m] = 1 / |q'|, scal[b, m + 1] = quantity (m + 1) / |q'|, have += 1.
 *             mode 3, a member to verify: history[b, 1 + k] = quantity 0 / cells of the true residual; 3 non-finite,
 *               0 converged, 1 k == maxcycles, else gcr = 1 with no directions; verify = fresh = 0.
 *             outcome: [nbatch, 3] (passes, reason, hand-over cycle or -1).  After modes 0 and 3 a one-workgroup launch
 *             writes counts[0 .. 3] = members with active, gcr, verify, fresh set.
 * (No reference counterpart: the reference solves one system at a time, linsolver.py:17-26, 61-72.) */
int64_t odil_stencil_gcr_batch_parts(int64_t cells);
int odil_stencil_gcr_dots_batch_f64(const double* store, int64_t store_stride, int64_t cells, int krylov_m, int slot,
                                    const int* have, int max_have, const int* mask, int nbatch, double* gpart,
                                    int64_t gpart_stride, void* stream);
int odil_stencil_gcr_dots_batch_f32(const float* store, int64_t store_stride, int64_t cells, int krylov_m, int slot,
                                    const int* have, int max_have, const int* mask, int nbatch, double* gpart,
                                    int64_t gpart_stride, void* stream);
int odil_stencil_gcr_project_batch_f64(double* store, int64_t store_stride, const double* rho, int64_t rho_stride,
                                       int64_t cells, int krylov_m, int slot, const int* have, int max_have,
                                       const double* scal, int64_t scal_stride, const int* mask, int nbatch, double* gpart,
                                       int64_t gpart_stride, void* stream);
int odil_stencil_gcr_project_batch_f32(float* store, int64_t store_stride, const float* rho, int64_t rho_stride, int64_t cells,
                                       int krylov_m, int slot, const int* have, int max_have, const double* scal,
                                       int64_t scal_stride, const int* mask, int nbatch, double* gpart, int64_t gpart_stride,
                                       void* stream);
int odil_stencil_gcr_update_batch_f64(double* store, int64_t store_stride, double* x, int64_t x_stride, double* rho,
                                      int64_t rho_stride, int64_t cells, int krylov_m, int slot, const double* scal,
                                      int64_t scal_stride, const int* mask, int nbatch, double* gpart, int64_t gpart_stride,
                                      void* stream);
int odil_stencil_gcr_update_batch_f32(float* store, int64_t store_stride, float* x, int64_t x_stride, float* rho,
                                      int64_t rho_stride, int64_t cells, int krylov_m, int slot, const double* scal,
                                      int64_t scal_stride, const int* mask, int nbatch, double* gpart, int64_t gpart_stride,
                                      void* stream);
int odil_stencil_gcr_sumsq_batch_f64(const double* v, int64_t v_stride, int64_t cells, const int* mask, int nbatch,
                                     double* gpart, int64_t gpart_stride, void* stream);
int odil_stencil_gcr_sumsq_batch_f32(const float* v, int64_t v_stride, int64_t cells, const int* mask, int nbatch,
                                     double* gpart, int64_t gpart_stride, void* stream);
int odil_stencil_gcr_decide_batch(int mode, const double* partials, int64_t partials_stride, const double* partials0,
                                  int64_t partials0_stride, int nparts, const double* gpart, int64_t gpart_stride, int gparts,
                                  int nbatch, int64_t cells, int k, int maxcycles, double tol, int krylov_m, double* history,
                                  int64_t history_stride, int* outcome, int* active, int* gcr, int* fresh, int* verify,
                                  int* have, double* scal, int64_t scal_stride, int* counts, void* stream);
/* Mixed-precision iterative refinement of the multigrid Newton solve (gmg.py; no reference counterpart -- the reference's
 * direct solver is double throughout): float32 V-cycles inside a float64 residual loop.  narrow_scale: y32 = s x64 with
 * s = a / sqrt(*msq) (msq: device scalar, the mean square the residual kernel just wrote; NULL: s = a); widen_axpy:
 * y64 += s x32 with s = a sqrt(*msq). */
int odil_narrow_scale(const double* x, float* y, int64_t n, double a, const double* msq, void* stream);
int odil_widen_axpy(double* y, const float* x, int64_t n, double a, const double* msq, void* stream);
/* out[r] = max |a[r n .. (r + 1) n)| for the nrows <= 64 rows of one array, two launches in all (the multigrid set-up reads
 * the largest coupling of every direction on every level: the 2 d coefficient arrays of a level are rows of one buffer). */
int odil_max_abs_rows_f64(const double* a, int nrows, int64_t n, double* partials, double* out, void* stream);
int odil_max_abs_rows_f32(const float* a, int nrows, int64_t n, double* partials, float* out, void* stream);
/* out[0] = max |a - b|, out[1] = max |b| over n entries in one pass (NaN differences propagate): the comparison by which
 * a linearised operator's coefficient arrays are recognised as a known stencil (gmg.recognise_poisson) -- no reference
 * counterpart.  `partials`: odil_reduce_workspace_bytes(). */
int odil_max_abs_diff_f64(const double* a, const double* b, int64_t n, double* partials, double* out, void* stream);
int odil_max_abs_diff_f32(const float* a, const float* b, int64_t n, double* partials, float* out, void* stream);
/* CSR assembly of the same matrix (core.py:1144-1171, :1214): indptr[n+1], indices,
 * data of nnz = nshift*n entries, columns offset by `col_offset`; rows keep ODIL's
 * order (ascending shift index within a row, not sorted by column). */
int odil_csr_assemble_f64(const double* coeffs, const int64_t* shifts, int nshift, const int64_t* shape, int ndim,
                          int64_t col_offset, int64_t* indptr, int64_t* indices, double* data, void* stream);
int odil_csr_assemble_f32(const float* coeffs, const int64_t* shifts, int nshift, const int64_t* shape, int ndim,
                          int64_t col_offset, int64_t* indptr, int64_t* indices, float* data, void* stream);

/* ---- Newton: the dense block of the normal equations on the matrix cores --------------------------------
 * `Array` / `NeuralNet` unknowns enter `Problem.linearize` as DENSE Jacobian columns (reference core.py:1189-1203);
 * the normal equations (linsolver.py:17-23) need D^T D, D^T r and, for the Schur complement against the
 * matrix-free stencil part, (S^T D)^T Z.  out (px x py, row-major) = X^T Y for row-major X (n x px, row stride
 * ldx) and Y (n x py, row stride ldy), px, py <= 64, by v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 tiles
 * with a fixed-order two-stage reduction (bit-reproducible).  `workspace`: odil_dense_block_workspace_bytes(). */
size_t odil_dense_block_workspace_bytes(void);
int odil_dense_block_xty_f64(const double* x, const double* y, int64_t n, int px, int py, int64_t ldx, int64_t ldy,
                             double* out, double* workspace, void* stream);
int odil_dense_block_xty_f32(const float* x, const float* y, int64_t n, int px, int py, int64_t ldx, int64_t ldy,
                             float* out, float* workspace, void* stream);
/* The same product for 1 <= px, py <= 1024 columns: 64-column panels of X and Y, one pair of panels and one row range
 * per workgroup, row ranges summed in index order in double (bit-reproducible).  X == Y with the same row stride and
 * px <= py (D^T D, D^T [D | r]): only pairs on or above the diagonal are computed and the rest mirrored, so that the
 * p x p block is exactly symmetric.  `workspace`: `workspace_bytes` >= odil_dense_block_wide_workspace_bytes(px, py),
 * which never exceeds 64 MiB (0 for column counts outside the range). */
size_t odil_dense_block_wide_workspace_bytes(int px, int py);
int odil_dense_block_xty_wide_f64(const double* x, const double* y, int64_t n, int px, int py, int64_t ldx,
                                  int64_t ldy, double* out, double* workspace, size_t workspace_bytes, void* stream);
int odil_dense_block_xty_wide_f32(const float* x, const float* y, int64_t n, int px, int py, int64_t ldx, int64_t ldy,
                                  float* out, float* workspace, size_t workspace_bytes, void* stream);
/* The Gram matrix D^T D (p x p) of one block: odil_dense_block_xty with X = Y = D. */
int odil_dense_block_gram_f64(const double* d, int64_t n, int p, int64_t ld, double* out, double* workspace,
                              void* stream);
int odil_dense_block_gram_f32(const float* d, int64_t n, int p, int64_t ld, float* out, float* workspace,
                              void* stream);

/* ---- Newton: multigrid for the normal equations of several grid fields (gmg.NormalGMG) ------------------------------
 * The reference solves any Newton system with --linsolver multigrid by AMG on the normal equations (linsolver.py:61-72).
 * A level: nf <= 8 fields concatenated in one vector; desc = {nf, off[0..nf], n[f][0..2] (canonical 3-D shape of every
 * field, leading axes 1), ebeg[0..nf]}; table: DEVICE int64, 8 words per entry (a, b, o0, o1, o2, start, 0, 0), sorted by
 * a, the entries of field a in [ebeg[a], ebeg[a+1]); coef: the coefficient arrays, entry e over a's grid at coef + start:
 *     (A x)_a[q] = sum_e C_e[q] x_b[q + o]          (terms outside b's grid are zero).
 * apply: mode 0 y = A x, 1 y = b - A x, 2 y = x + omega dinv (b - A x) (one weighted Jacobi sweep), 3 y = omega dinv b
 * (the sweep from zero: x, coef, table not read).  y != x. */
int odil_bmg_apply_f64(const double* coef, const int64_t* table, const int64_t* desc, const double* x, const double* b,
                       const double* dinv, double* y, int mode, double omega, void* stream);
int odil_bmg_apply_f32(const float* coef, const int64_t* table, const int64_t* desc, const float* x, const float* b,
                       const float* dinv, float* y, int mode, float omega, void* stream);
/* One term of A = M^T M: out[j] += c1[r(j)] c2[r(j)] over field a's grid (ashape, canonical 3-D), c1 / c2 the coefficient
 * arrays of two stencil blocks of the same output (row grid rshape); rmap: DEVICE int64, per axis of a's grid
 * (concatenated) the row reading a at j_d whose read of b is at j_d + o_d, or -1 (reference core.py:1144-1171). */
int odil_bmg_assemble_f64(const double* c1, const double* c2, const int64_t* rmap, const int64_t* ashape,
                          const int64_t* rshape, double* out, void* stream);
int odil_bmg_assemble_f32(const float* c1, const float* c2, const int64_t* rmap, const int64_t* ashape,
                          const int64_t* rshape, float* out, void* stream);
/* Transfers between a level (fdesc) and the next coarser one (cdesc); code: HOST, 3 per field, per axis 0 = not coarsened,
 * 1 = cells (3/4, 1/4 linear; all of the parent at a wall), 2 = nodes (coarse node I on fine node 2I, linear).
 * mode 0: out_coarse = P^T in_fine; mode 1: out_fine = add_fine + P in_coarse (out may be add; in != out). */
int odil_bmg_transfer_f64(const int64_t* fdesc, const int64_t* cdesc, const int* code, const double* in,
                          const double* add, double* out, int mode, void* stream);
int odil_bmg_transfer_f32(const int64_t* fdesc, const int64_t* cdesc, const int* code, const float* in,
                          const float* add, float* out, int mode, void* stream);
/* Galerkin coarsening C^c = P^T C P: every coefficient of the coarse table ctable (nce entries, `total` values) from the
 * fine coefficients, one thread per coarse value, fixed summation order. */
int odil_bmg_galerkin_f64(const int64_t* fdesc, const int64_t* cdesc, const int* code, const double* fcoef,
                          const int64_t* ftable, const int64_t* ctable, int nce, int64_t total, double* ccoef,
                          void* stream);
int odil_bmg_galerkin_f32(const int64_t* fdesc, const int64_t* cdesc, const int* code, const float* fcoef,
                          const int64_t* ftable, const int64_t* ctable, int nce, int64_t total, float* ccoef,
                          void* stream);
/* The coarsest level factorised on the device (gmg.NormalGMG(coarse="device"), float64 only, n <= 8192 unknowns; np: n
 * rounded up to a multiple of 64).  coarse_dense: rows / columns [0, np) of out (row stride lda >= np) become the dense
 * symmetric matrix 0.5 (A + A^T) of the level, zero beyond n.  coarse_chol: work is np x 2 np (row stride 2 np) with the
 * matrix of coarse_dense (lda = 2 np) in its left half; blocked Cholesky on [A | I] (f64 MFMA trailing updates), then
 * inv (n x n, row stride n) = the symmetric generalised inverse.  A Schur-complement pivot <= tol_rel * max_i A_ii is
 * dropped (its row and column of inv are zero); drops: DEVICE int[np / 64], the dropped pivots of every panel; thr:
 * DEVICE, one double (scratch).  work is overwritten.  No atomics: bit-reproducible. */
int odil_bmg_coarse_dense_f64(const double* coef, const int64_t* table, const int64_t* desc, int64_t np, int64_t lda,
                              double* out, void* stream);
int odil_bmg_coarse_chol_f64(double* work, int64_t n, int64_t np, double tol_rel, double* thr, int* drops,
                             double* inv, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ODIL_HIP_H */
