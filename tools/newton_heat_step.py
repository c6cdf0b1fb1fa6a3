#!/usr/bin/env python3
"""One Newton step of examples/heat as `util.optimize_newton` takes it (linearize_device, linsolver.solve, x - d), with
the solver's status and the wall times of the two phases printed.  --root: the checkout whose package and example are
used (another commit's tree, with its library built, to compare routes); everything else goes to heat.py's parser.

    python tools/newton_heat_step.py --infer_k 1 --arch_k 8 8 --Nt 256 --Nx 512 --optimizer newton --multigrid 0 \
        --linsolver direct
"""

import json
import os
import sys
import time

here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
argv = sys.argv[1:]
if "--root" in argv:
    k = argv.index("--root")
    here = argv[k + 1]
    del argv[k:k + 2]
root = os.path.abspath(here)
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "examples", "heat"))

import torch  # noqa: E402

import heat  # noqa: E402
import odil_amd as odil  # noqa: E402
from odil_amd import linsolver  # noqa: E402

assert os.path.abspath(odil.__file__).startswith(root), odil.__file__
odil.util.set_log_file(sys.stdout)
args = heat.parse_args(argv)
problem, state = heat.make_problem(args)
print("argv", argv, flush=True)
before = float(problem.eval_loss_grad(state)[0])
torch.cuda.synchronize()
t0 = time.perf_counter()
vector, op = problem.linearize_device(state)
torch.cuda.synchronize()
t1 = time.perf_counter()
status = dict()
d = linsolver.solve(op, vector.contiguous(), args, status, args.linsolver)
torch.cuda.synchronize()
t2 = time.perf_counter()
print("unknowns", op.ncols, "rows", op.nrows, flush=True)
print("status", {k: (float(v) if torch.is_tensor(v) else v) for k, v in status.items()}, flush=True)
print(json.dumps(dict(linearize_s=round(t1 - t0, 3), solve_s=round(t2 - t1, 3), total_s=round(t2 - t0, 3),
                      loss_before=before)), flush=True)
problem.domain.unpack_state(problem.domain.pack_state(state) - d.to(vector.dtype), state)
print("loss after", float(problem.eval_loss_grad(state)[0]), flush=True)
