"""The energy-norm drops on more than one rank: two ranks share the one GPU of the test box and talk through gloo, set up
as in test_gpu_system_ranks.py.  alpha is global behind the Gram all-reduce, so every rank forms the same drops from it
with no collective of their own: the drops are equal on both ranks in bits, equal to the one-process run at 1e-8, and a
solve with them costs the all-reduces per iteration of preAlps_ECGSolve on the same ranks.

The problem is energy_ref's Poisson 10^3 in 40 parts at t = 4; one spawn runs the one-process solves, a second the
two ranks, which receive the former's drops."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
T = 4
CASES = [(1, 4, "odir"), (2, 2, "odir"), (4, 1, "omin")]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _paths():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _single(q):
    try:
        _paths()
        import prealps_amd as pa
        import energy_ref as R
        pb = R.open_problem("P", device=0)
        prob = pb["prob"]
        out = {}
        for k, s, alg in CASES:
            oa = pa.ORTHODIR if alg == "odir" else pa.ORTHOMIN
            got = prob.solve_system(pb["B"][:, :k], T, stop="scaled", tol=TOL, ortho_alg=oa, energy=True)
            out[(k, s, alg)] = (got.iters, got.drop_hist)
        prob.close()
        q.put(("ok", out))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(("fail: %s\n%s" % (e, traceback.format_exc()), None))


def _worker(rank, world, port, single, q):
    try:
        _paths()
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["LOCAL_RANK"] = "0"
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import prealps_amd as pa
        import energy_ref as R
        pb = R.open_problem("P", device=0, distributed=True)
        prob = pb["prob"]
        N = prob.N
        B = pb["B"]
        fails = []

        def gathered(obj):
            box = [None] * world
            dist.all_gather_object(box, obj)
            return box

        def case(name, fn):
            try:
                fn()
            except Exception as e:
                import traceback
                fails.append("case %s: %s\n%s" % (name, e, traceback.format_exc()))

        def drops(k, s, alg):
            oa = pa.ORTHODIR if alg == "odir" else pa.ORTHOMIN
            c0 = prob.stat("ecg_energy_launches")
            base = prob.solve_system(B[:, :k], T, stop="scaled", tol=TOL, ortho_alg=oa)
            got = prob.solve_system(B[:, :k], T, stop="scaled", tol=TOL, ortho_alg=oa, energy=True)
            assert prob.stat("ecg_energy_launches") - c0 == got.iters
            box = gathered((got.iters, got.drop_hist.tobytes(), got.err_hist.tobytes(), got.err_est.tobytes(),
                            got.err_iter.tobytes(), got.energy_norm.tobytes()))
            assert all(b == box[0] for b in box), "the drops or the estimates differ between the ranks"
            # tracking changes no bit of the solve on several ranks either
            assert got.iters == base.iters and np.asarray(got.x).tobytes() == np.asarray(base.x).tobytes()
            assert got.res.tobytes() == base.res.tobytes() and got.sys_hist.tobytes() == base.sys_hist.tobytes()
            it1, d1 = single[(k, s, alg)]
            n = min(it1, got.iters)
            print("rank", rank, (k, s, alg), "iters", got.iters, "one process", it1, "drops / one process - 1",
                  np.abs(got.drop_hist[:n] / d1[:n] - 1.0).max(), flush=True)
            assert got.iters == it1
            np.testing.assert_allclose(got.drop_hist[:n], d1[:n], rtol=1e-8, atol=0.0)

        for k, s, alg in CASES:
            case("drops %s" % ((k, s, alg),), lambda k=k, s=s, alg=alg: drops(k, s, alg))

        def energy_stop():
            got = prob.solve_system(B[:, :2], T, stop="energy", tol=TOL)
            box = gathered((got.iters, got.drop_hist.tobytes(), got.err_est.tobytes()))
            assert all(b == box[0] for b in box), "the energy stop differs between the ranks"
            n, windows = R.stop_iteration(got.drop_hist, TOL)
            assert n == got.iters > R.DMIN
            X = sum(gathered(np.asarray(got.x)))
            xstar = R.exact(pb, 2)
            e0, en = np.sqrt(R.energy2(pb, xstar)), np.sqrt(R.energy2(pb, xstar - X))
            print("rank", rank, "energy stop at", got.iters, "true energy error / initial", en / e0, flush=True)
            assert (en <= TOL * e0).all()

        case("energy stop", energy_stop)

        def collectives(lazy):
            if not lazy:
                os.environ["PREALPS_ECG_LAZY_STOP"] = "0"
            try:
                b = prob.reference_rhs()
                count = {}
                for name, run in (("solve", lambda it: prob.solve(b, T, tol=1e-12, max_iter=it)),
                                  ("tracked", lambda it: prob.solve_system(B[:, :2], T, stop="scaled", tol=1e-12, max_iter=it, energy=True)),
                                  ("tracked, original", lambda it: prob.solve_system(B[:, :2], T, stop="original", tol=1e-12, max_iter=it, energy=True)),
                                  ("energy", lambda it: prob.solve_system(B[:, :2], T, stop="energy", tol=1e-12, max_iter=it))):
                    c = []
                    for it in (4, 12):
                        before = prob.stat("allreduces")
                        r = run(it)
                        assert r.iters == it, (name, r.iters, it)
                        c.append(prob.stat("allreduces") - before)
                    count[name] = (c[1] - c[0]) / 8.0
            finally:
                os.environ.pop("PREALPS_ECG_LAZY_STOP", None)
            print("rank", rank, "lazy" if lazy else "eager", "all-reduces per iteration", count, flush=True)
            assert count["solve"] > 0 and all(v == count["solve"] for v in count.values()), count

        case("collectives, lazy stopping test", lambda: collectives(True))
        case("collectives, eager stopping test", lambda: collectives(False))

        def refusal():
            with pytest.raises(pa.PreAlpsError, match="preAlps_ECGSolveSystemEnergy.*ADAPT_BS"):
                prob.solve_system(B[:, :2], T, stop="energy", bs_red=pa.ADAPT_BS, tol=TOL)
            again = prob.solve_system(B[:, :2], T, stop="energy", tol=TOL)
            assert again.iters > 0

        case("refusal", refusal)

        prob.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok" if not fails else "fail: " + "\n".join(fails)))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "fail: %s\n%s" % (e, traceback.format_exc())))


def test_two_ranks_form_the_drops_of_one_process_without_a_collective():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_single, args=(q,))
    p.start()
    status, single = q.get(timeout=240)
    p.join(timeout=60)
    assert status == "ok", status
    world, port = 2, _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, single, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[1] == "ok", r
