"""Solve the caller's own system on the graded Poisson problem of tests/test_gpu_system_solve.py, both ways, and print
both residuals:
  python examples/solve_system.py [--operator-precision single|double] [--refine] [--stop energy] [n [t [decades]]]
                                                         (defaults 10, 4, 2: S A0 S with S = diag(10^linspace(-2, 2, N)))
The right-hand side, the guess and the solution are in the order and units of the matrix as it is assembled here; the
permutation by parts and the row scaling of the solver stay inside the library (EcgProblem.solve_system).
stop="scaled" is the library's own test, on the scaled system; stop="original" stops on ||b - A x|| <= tol ||b||.
--operator-precision single stores the matrix values of the SpMM in fp32 where the plan allows it (the packed run plan at
up to 4 columns; "spmm_precision" in the output says what the plan in use reads); --refine solves in passes
(solve_system(..., refine=True)), each started from the x before it with a residual formed on the fp64 matrix.
--stop energy adds a third solve that stops on the estimate of the energy-norm error ||x* - x||_A (a delayed lower bound
summed from the drops of the iterations; a heuristic) relative to the same bound of the initial error, and prints the
estimate beside the residuals; not with --refine."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import prealps_amd as pa
from prealps_amd import gen

args = sys.argv[1:]
refine = "--refine" in args
precision = None
if "--operator-precision" in args:
    precision = args[args.index("--operator-precision") + 1]
    del args[args.index("--operator-precision"):args.index("--operator-precision") + 2]
energy = False
if "--stop" in args:
    if args[args.index("--stop") + 1] != "energy":
        sys.exit("--stop takes 'energy' (the scaled and the original stop always run)")
    energy = True
    del args[args.index("--stop"):args.index("--stop") + 2]
if energy and refine:
    sys.exit("--stop energy is not combined with --refine")
args = [a for a in args if a != "--refine"]
n = int(args[0]) if len(args) > 0 else 10
t = int(args[1]) if len(args) > 1 else 4
dec = float(args[2]) if len(args) > 2 else 2.0
TOL = 1e-5
rp, ci, v0 = gen.poisson3d_csr(n)
v = gen.graded_values(rp, ci, v0, -dec, dec)
N = len(rp) - 1
A = sp.csr_matrix((v, ci, rp), shape=(N, N))
b = np.random.default_rng(20260407).standard_normal(N)
prob = pa.EcgProblem(rp, ci, v, 8, None, scale=True, device=0)
prob.create_block_jacobi()
if precision is not None:
    prob.set_operator_precision(precision)
kw = dict(refine=True) if refine else {}
out = dict(n=n, N=N, t=t, decades=2 * dec, tol=TOL, scaling_range=[float(prob.scaling.min()), float(prob.scaling.max())])
for stop in ("scaled", "original") + (("energy",) if energy else ()):
    r = prob.solve_system(b, t, stop=stop, tol=TOL, **kw)
    fresh, normb = prob.system_residuals(b, r.x)
    out[stop] = dict(iters=r.iters,
                     **(dict(passes=r.passes, pass_iters=[int(i) for i in r.pass_iters], refine_status=r.refine_status,
                             pass_relative_residuals=(r.pass_res[:, 0] / r.sys_normb[0]).tolist()) if refine else {}),
                     # what the stopping test saw, in its own metric, and the recurrence residual in the caller's units
                     stopped_at=float(r.sys_res[0] / r.sys_normb[0]),
                     recurrence_relative_residual=float(r.sys_res_original[0] / normb[0]),
                     # formed afresh from b and x: on the device by the library, on the host from the CSR arrays
                     library_relative_residual=float(fresh[0] / normb[0]),
                     host_relative_residual=float(np.linalg.norm(b - A @ r.x) / np.linalg.norm(b)))
    if stop == "energy":
        # the estimate of ||x* - x||_A after iteration err_iter, beside the bound of the initial error it is held against
        out[stop].update(energy_error_estimate=float(r.err_est[0]), estimate_belongs_to_iteration=int(r.err_iter[0]),
                         initial_energy_error_bound=float(r.energy_norm[0]),
                         relative_energy_error_estimate=float(r.err_est[0] / r.energy_norm[0]))
if energy:
    r = prob.solve_system(b, t, stop="original", tol=TOL)      # (the time step below goes on from the caller's own stop)
# a time step: go on from the last solution with a perturbed right-hand side
b2 = b + 1e-3 * np.random.default_rng(1).standard_normal(N)
warm = prob.solve_system(b2, t, x0=r.x, stop="original", tol=TOL, **kw)
cold = prob.solve_system(b2, t, stop="original", tol=TOL, **kw)
out["next_step"] = dict(iters_from_the_last_solution=warm.iters, iters_from_zero=cold.iters)
out["spmm_precision"] = int(prob.stat("spmm_precision"))
prob.close()
print(json.dumps(out))
