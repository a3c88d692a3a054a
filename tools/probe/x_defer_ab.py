"""Same process, the headline problem: 400-iteration solves (tol far below reach) with PREALPS_ECG_X_DEFER (X every second
row pass) alternating off / on, eight times each way, in the style of tools/probe/abs_ab.py.  The switch is read at
every reset, so a solve takes the value the environment holds when it starts.  Prints every window and whether every
on-window is faster than every off-window.  X_DEFER_AB_OUT: also write the lines there."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import prealps_amd
from prealps_amd import gen
rp, ci, v = gen.elasticity3d_csr(70); part, P = gen.box_partition_nodes(70, (2, 4, 8))
prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
rhs = prob.reference_rhs()
ITERS, ALTS = 400, 8
SWITCH = "PREALPS_ECG_X_DEFER"
lines = []
def say(s):
    print(s, flush=True); lines.append(s)
os.environ.pop(SWITCH, None)
prob.solve(rhs, 4, tol=1e-30, max_iter=50)
us = {0: [], 1: []}
for alt in range(ALTS):
    for val in (0, 1):
        os.environ[SWITCH] = str(val)
        r = prob.solve(rhs, 4, tol=1e-30, max_iter=ITERS)
        assert r.iters == ITERS, r.iters
        us[val].append(1e6 * r.seconds / r.iters)
os.environ.pop(SWITCH, None)
say("%s=0: %s us/it" % (SWITCH, " ".join("%.2f" % u for u in us[0])))
say("%s=1: %s us/it" % (SWITCH, " ".join("%.2f" % u for u in us[1])))
say("%s: slowest on %.2f, fastest off %.2f, means %.2f -> %.2f us/it: %s" % (
    SWITCH, max(us[1]), min(us[0]), sum(us[0]) / ALTS, sum(us[1]) / ALTS,
    "every on-window is faster than every off-window" if max(us[1]) < min(us[0]) else "the windows overlap"))
prob.close()
if os.environ.get("X_DEFER_AB_OUT"):
    open(os.environ["X_DEFER_AB_OUT"], "w").write("\n".join(lines) + "\n")
