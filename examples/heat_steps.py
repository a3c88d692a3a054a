"""An implicit-Euler heat equation on the n^3 Poisson grid, 16 steps on one operator, every step solved twice: cold,
and through the solution history (solve_system(history=True)), which starts from the element of the span of the last
solutions that is closest to the new one in the energy norm:
  python examples/heat_steps.py [--distributed] [n [t [capacity [steps]]]]          (defaults 10, 4, 8, 16)
  python -m torch.distributed.run --nproc_per_node=G examples/heat_steps.py --distributed ...
With --distributed every rank of the process group holds the rows of its parts, of the operator and of the history's
ring alike; b and x stay global arrays, a rank's x holds the rows it owns and zeros elsewhere, and the new u is their sum
over the ranks.  Rank 0 prints.
A = I + 5 K, b_n = u_(n-1) + 5 f(0.2 n), f a travelling sine plus a moving Gaussian; 8 contiguous parts, tol 1e-5 on
||b - A x|| / ||b||.  Prints the iterations of both ways per step and a JSON summary line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import prealps_amd as pa
from prealps_amd import gen

args = sys.argv[1:]
distributed = "--distributed" in args
args = [a for a in args if a != "--distributed"]
rank = 0
if distributed:
    import torch.distributed as dist
    if not dist.is_initialized():
        dist.init_process_group("gloo")
    rank = dist.get_rank()
n = int(args[0]) if len(args) > 0 else 10
t = int(args[1]) if len(args) > 1 else 4
capacity = int(args[2]) if len(args) > 2 else 8
steps = int(args[3]) if len(args) > 3 else 16
DT, TOL = 5.0, 1e-5
rp, ci, v = gen.poisson3d_csr(n)
N = len(rp) - 1
A = (sp.identity(N, format="csr") + DT * sp.csr_matrix((v, ci, rp), shape=(N, N))).tocsr()
A.sort_indices()
g = (np.arange(n) + 0.5) / n
z, y, x = np.meshgrid(g, g, g, indexing="ij")


def source(tm):
    sine = np.sin(2 * np.pi * (x - 0.3 * tm)) * np.sin(np.pi * y) * np.sin(np.pi * z)
    cx, cy = 0.5 + 0.3 * np.cos(0.25 * tm), 0.5 + 0.3 * np.sin(0.25 * tm)
    return (sine + np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - 0.5) ** 2) / 0.02)).ravel()


device = 0
if distributed:      # one device per rank where there are enough of them, otherwise the ranks share
    import torch
    device = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
prob = pa.EcgProblem(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, 8, None, scale=True,
                    device=device, distributed=distributed)
prob.create_block_jacobi()


def whole(x_own):
    """The rows every rank owns, summed into the global vector (one process: x itself)."""
    if not distributed:
        return x_own
    import torch
    full = torch.from_numpy(np.ascontiguousarray(x_own))
    dist.all_reduce(full)
    return full.numpy()


prob.enable_history(capacity)
u = np.zeros(N)
rows = []
for step in range(1, steps + 1):
    b = u + DT * source(0.2 * step)
    cold = prob.solve_system(b, t, tol=TOL)
    warm = prob.solve_system(b, t, tol=TOL, history=True)
    u = whole(warm.x)
    rows.append(dict(step=step, cold=cold.iters, history=warm.iters, rank=warm.history_rank,
                     start_residual=float(warm.sys_res0[0] / warm.sys_normb[0])))
    if rank == 0:
        print("step %2d  cold %3d  history %3d  (rank %d, start residual %.1e of ||b||)"
              % (step, cold.iters, warm.iters, warm.history_rank, rows[-1]["start_residual"]), flush=True)
tail = rows[steps // 2:]
if rank == 0:
    print(json.dumps(dict(n=n, N=N, t=t, capacity=capacity, steps=steps, tol=TOL,
                          cold_iterations=sum(r["cold"] for r in rows), history_iterations=sum(r["history"] for r in rows),
                          second_half_cold=sum(r["cold"] for r in tail), second_half_history=sum(r["history"] for r in tail),
                          ranks=dist.get_world_size() if distributed else 1,
                          gram_refreshes=int(prob.stat("hist_gram_refreshes")), history_bytes=int(prob.stat("hist_bytes")))))
prob.close()
if distributed:
    dist.barrier()
    dist.destroy_process_group()
