"""Set-up of gmg.NormalGMG with the coarsest level inverted on the host (eigh) or on the device (csrc/coarse_chol.hip),
the application of the coarsest inverse, and the `direct` / `multigrid` solves at darcy 1024^2 and 128^3 (DESIGN
section 5).  Run from the repository root: python tools/coarse_chol_timing.py."""
import argparse, os, sys, time, json
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import odil_amd as odil
from odil_amd import gmg, ops

out = {}
def t(fn, reps=1):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): r = fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / reps, r

for name, argv in [("darcy 1024^2", ["--ndim", "2", "--N", "1024"]), ("darcy 128^3", ["--ndim", "3", "--N", "128"])]:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "darcy")); import darcy
    odil.util.set_log_file(open(os.devnull, "w"))
    problem, state = darcy.make_problem(darcy.parse_args(argv))
    vector, op = problem.linearize_device(state)
    rec = {}
    gmg.NormalGMG.create(op, coarse="device")  # warm-up (loads, allocator)
    for coarse in ("host", "device", "host", "device"):
        dt, s = t(lambda: gmg.NormalGMG.create(op, coarse=coarse))
        rec["setup_" + coarse] = dt
        dt2, _ = t(s._coarse_inverse if coarse == "host" else s._coarse_inverse_device)
        rec["coarse_" + coarse] = dt2
    rec["coarsest_unknowns"] = s.offs[-1][-1]; rec["levels"] = s.nlvl
    b = torch.randn(s.offs[-1][-1], dtype=torch.float64, device=op.device)
    x = torch.empty_like(b)
    dt, _ = t(lambda: ops.lincomb(x, 0.0, s.coarse_inv, b), reps=200)
    rec["coarse_apply_lincomb"] = dt
    args = argparse.Namespace(linsolver_tol=1e-12, linsolver_maxiter=None, linsolver_damp=0, linsolver_dampdiag=0)
    for ls in ("direct", "multigrid", "direct"):
        st = {}
        dt, _ = t(lambda: odil.linsolver.solve(op, -vector, args, st, ls))
        rec["solve_" + ls] = dt; rec["status_" + ls] = {k: v for k, v in st.items() if isinstance(v, (int, float, str, bool))}
    out[name] = rec
    print(name, json.dumps(rec), flush=True)
