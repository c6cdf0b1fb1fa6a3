#!/usr/bin/env python3
"""Fills odil_amd/_jit_cache with the generated kernels of the BASELINE configurations (and of the build / smoke example)
by tracing the example operators on CPU tensors and cross-compiling for gfx950 -- no GPU needed, nothing is launched.
A clean clone then does not spend its first GPU minutes in hipcc.  (The kernels of the GPU test suite's small fixtures --
a few hundred variants of a few seconds each -- are built by the suite's first run and kept in the same cache.)

    python3 tools/prebuild_jit.py [--quick | --all]

--all adds small cases that reach the generator paths the BASELINE configurations do not (SMALL below).  The library name
is the hash of the generated source and the compiler flags, so the printed names of two checkouts are equal exactly when
the generator emits the same bytes for every case: that is how a change of the generator that must not change its output
is checked, without a GPU.
"""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for sub in ("poisson", "heat", "velocity_from_tracer", "wave", "heat_tmax", "infer_constant", "basic", "diffusion"):
    sys.path.insert(0, os.path.join(ROOT, "examples", sub))

CONFIGS = [  # (example module, argv, slab: None or (axis, ranks)[, also emit k_jac: True, or "batch" for k_jac_batch as well])
    ("wave", ["--Nt", "8", "--Nx", "8"], None),                                                      # __graft_entry__.build()
    ("wave", ["--Nt", "8", "--Nx", "16"], None),                                                     # __graft_entry__.smoke()
    ("fields", [], None),                                                                            # one kernel set per field location
    ("heat", ["--Nt", "256", "--Nx", "512", "--infer_k", "1", "--imposed", "stripe"], None),          # config 3
    ("heat2d", ["--Nt", "256", "--Nx", "512", "--Ny", "512", "--infer_k", "1", "--imposed", "stripe"], None),  # config 3 at BASELINE's shape
    ("veltracer", ["--Nt", "128", "--Nx", "256", "--Ny", "256"], None),                                # config 5, reference-native
    ("veltracer3d", ["--Nt", "32", "--Nx", "256"], None),                                            # 5b
    ("veltracer3d", ["--Nt", "128", "--Nx", "32", "--Ny", "256", "--Nz", "256"], (1, 1)),                  # config 5: one rank's slab, world 1
    ("veltracer3d", ["--Nt", "128", "--Nx", "64", "--Ny", "256", "--Nz", "256"], (1, 2)),                  # ... and with interfaces (world >= 2)
]
_HEAT = ["--Nt", "8", "--Nx", "16", "--infer_k", "1"]
SMALL = [  # --all: seconds each
    ("wave", ["--Nt", "8", "--Nx", "8"], None, True),                                                # k_jac
    ("diffusion", ["--ndim", "3", "--N", "16"], (0, 2), True),                                       # k_jac of one slab rank
    ("diffusion", ["--ndim", "2", "--N", "16"], None, "batch"),                                      # k_jac_batch (ensembles)
    ("heat", _HEAT + ["--kwreg", "0.3", "--kwregdecay", "100"], None),                               # k_par (param_expr)
    ("heat", _HEAT + ["--kwreg", "0.3", "--kwregdecay", "100"], (1, 2)),                             # ... of one slab rank
    ("heat_tmax", ["--Nt", "8", "--Nx", "16"], None),                                                # a one-point window, an Array
    ("infer_constant", ["--Nt", "8", "--Nx", "16"], None),                                           # a window of all rows but one
    ("infer_constant", ["--Nt", "8", "--Nx", "10", "--multigrid", "0"], None),                       # ... one point per thread
    ("heat", _HEAT + ["--imposed", "stripe", "--double", "1"], None),                                # float64
    ("veltracer", ["--Nt", "8", "--Nx", "16", "--double", "1"], None),
    ("veltracer", ["--Nt", "8", "--Nx", "16", "--Ny", "10", "--multigrid", "0"], None),              # one point per thread
    ("veltracer3d", ["--Nt", "8", "--Nx", "8", "--Ny", "8", "--Nz", "16"], None),                     # 4-D
    ("veltracer3d", ["--Nt", "8", "--Nx", "8", "--Ny", "8", "--Nz", "16"], (1, 2)),
]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quick", action="store_true", help="the build / smoke kernels only")
    p.add_argument("--all", action="store_true", help="also the small cases of the other generator paths (SMALL)")
    a = p.parse_args()
    import odil_amd
    from odil_amd import runtime, slab_traced, stencil_jit

    runtime._mod = odil_amd.ModRocm(device="cpu")
    odil_amd.util.set_log_file(open(os.devnull, "w"))
    for modname, argv, slab, *jac in CONFIGS[:2] if a.quick else CONFIGS + (SMALL if a.all else []):
        t0 = time.time()
        ex = importlib.import_module(modname)
        problem, state = ex.make_problem(ex.parse_args(argv))
        if slab is not None:
            n = problem.domain.cshape[slab[0]] // slab[1]
            path = slab_traced.HipSlabKernels(problem, state, slab[0], n, "cpu", jac=bool(jac)).lib_path
        elif jac:
            path = stencil_jit.TracedOperator(problem, state, jac=jac[0]).lib_path
        else:
            path = stencil_jit.trace(problem, state).lib_path
            path = path[0] if isinstance(path, list) else path
        what = " ".join(argv) + ("" if slab is None else " [slab {}/{}]".format(*slab)) + (" [k_jac{}]".format("_batch" if jac[0] == "batch" else "") if jac else "")
        print("{:12s} {:60s} {}  {:.1f} s".format(modname, what, os.path.basename(path), time.time() - t0), flush=True)
        del problem, state
    if not a.quick:
        # config 5 with 4 and 8 ranks: the GLOBAL grid would not fit on the host -- the shape-only state bench.py builds
        import argparse as ap
        import numpy as np
        import veltracer3d

        for world in (4, 8):
            t0 = time.time()
            va = veltracer3d.parse_args(["--Nt", "128", "--Nx", str(32 * world), "--Ny", "256", "--Nz", "256"])
            domain = odil_amd.Domain(cshape=(va.Nt, va.Nx, va.Ny, va.Nz), dimnames=("t", "x", "y", "z"), lower=(0, 0, 0, 0),
                                     upper=(1, 1, 1, 1), dtype=np.float32, multigrid=va.multigrid, mg_interp=va.mg_interp,
                                     mg_nlvl=va.nlvl)
            x, y, z = np.meshgrid(*domain.points_1d("x", "y", "z"), indexing="ij")
            extra = ap.Namespace(args=va, u_init=domain.mod.cast(veltracer3d.blob(x, y, z, 0), np.float32),
                                 u_final=domain.mod.cast(veltracer3d.blob(x, y, z, 1), np.float32))
            del x, y, z
            state = odil_amd.State()
            for key in ("u",) + veltracer3d.VEL:
                state.fields[key] = odil_amd.Field(None, loc=veltracer3d.LOC)
            problem = odil_amd.Problem(veltracer3d.operator, domain, extra)
            path = slab_traced.HipSlabKernels(problem, slab_traced.shape_state(domain, state), 1, 32, "cpu").lib_path
            print("{:12s} {:60s} {}  {:.1f} s".format("veltracer3d", "config 5, {} ranks".format(world), os.path.basename(path),
                                                        time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
