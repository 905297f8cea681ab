"""Equality elimination next to the unreduced solve, on one GPU: per shape (n, neq, m) the times of eliminate, reduced setup + solve and
expand, and of setup + solve of the unreduced batch on the same data, then the warm path of both (update(f) + warm solve).  Device tensors
in, device tensors out; each step timed on the host around a device synchronisation, best of --reps.  eliminate_s is the cold
daqp_batch_eliminate call of a new handle: its device allocations are in the figure.  Prints one JSON line.

--backward: behind the cold solves, the adjoint of both on the same (g_x, g_lam): EliminatedBatchModel.backward (reduce, the adjoint of
the reduced batch, expand) next to BatchModel.backward of the unreduced model -- one untimed call each first (it allocates the
intermediates), then the timed one.

    python tools/bench_eliminate.py [--N 2048] [--reps 3] [--backward]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(60, 40, 160), (200, 140, 460)]


def make(n, neq, m, N, seed):
    """N non-condensed problems: the first neq rows of A are equalities through a planted point, the others leave it 0.1 .. 1 of slack"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((N, n, n)) / np.sqrt(n)
    H = B @ B.transpose(0, 2, 1) + np.eye(n)
    A = rng.standard_normal((N, m, n)) / np.sqrt(n)
    xp = 0.3 * rng.standard_normal((N, n))
    cx = np.einsum("kij,kj->ki", A, xp)
    bu, bl = cx + rng.uniform(0.1, 1.0, (N, m)), cx - rng.uniform(0.1, 1.0, (N, m))
    bu[:, :neq] = bl[:, :neq] = cx[:, :neq]
    sense = np.zeros((N, m), np.int32)
    sense[:, :neq] = 5
    f = rng.standard_normal((N, n))
    return H, f, A, bu, bl, sense


def timed(fn, sync):
    sync()
    t = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t, out


def main():
    import torch
    import daqp_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--backward", action="store_true")
    a = ap.parse_args()
    sync = torch.cuda.synchronize
    rows = []
    for n, neq, m in SHAPES:
        N = a.N if n <= 64 else max(64, a.N // 8)
        dev = [torch.as_tensor(v, device="cuda") for v in make(n, neq, m, N, 7)]
        best = {}
        gen = torch.Generator(device="cuda").manual_seed(11)
        gx = torch.randn(N, n, dtype=torch.float64, device="cuda", generator=gen)
        gl = torch.randn(N, m, dtype=torch.float64, device="cuda", generator=gen)
        derr = None
        for _ in range(a.reps):
            em = daqp_amd.EliminatedBatchModel(N, n, m, 0, np.arange(neq))
            bm = daqp_amd.BatchModel(N, n, m, 0)
            t = {}
            t["eliminate_s"], _ = timed(lambda: em.eliminate(*dev), sync)
            t["reduced_setup_s"], _ = timed(lambda: em.setup_reduced(0), sync)
            t["reduced_solve_s"], r = timed(lambda: em.reduced.solve(out="torch"), sync)
            t["expand_s"], full = timed(lambda: em.expand(r, "torch"), sync)
            t["unreduced_setup_s"], _ = timed(lambda: bm.setup(*dev), sync)
            t["unreduced_solve_s"], ref = timed(lambda: bm.solve(out="torch"), sync)
            if a.backward:
                em.backward(gx, grad_lam=gl), bm.backward(gx, grad_lam=gl)
                t["eliminated_backward_s"], o = timed(lambda: em.backward(gx, grad_lam=gl), sync)
                t["unreduced_backward_s"], oref = timed(lambda: bm.backward(gx, grad_lam=gl), sync)
                derr = float((o["dz"] - oref["dz"]).abs().max() / oref["dz"].abs().max())
                ok_bw = bool((o["status"] == 0).all() and (oref["status"] == 0).all())
            # the warm path: new f on the kept factors (handle and reduced batch / unreduced batch), then a warm solve
            f2 = dev[1] * 1.01
            t["warm_update_s"], _ = timed(lambda: em.update(f=f2), sync)
            t["warm_solve_expand_s"], w = timed(lambda: em.solve(out="torch"), sync)
            t["unreduced_warm_update_s"], _ = timed(lambda: bm.update(f=f2), sync)
            t["unreduced_warm_solve_s"], wref = timed(lambda: bm.solve(out="torch"), sync)
            err = max(float((full["x"] - ref["x"]).abs().max()), float((w["x"] - wref["x"]).abs().max()))
            ok = bool((full["exitflag"] == ref["exitflag"]).all())
            em.close(), bm.close()
            for k, v in t.items():
                best[k] = min(best.get(k, v), v)
        el = sum(best[k] for k in ("eliminate_s", "reduced_setup_s", "reduced_solve_s", "expand_s"))
        un = best["unreduced_setup_s"] + best["unreduced_solve_s"]
        wel, wun = best["warm_update_s"] + best["warm_solve_expand_s"], best["unreduced_warm_update_s"] + best["unreduced_warm_solve_s"]
        rows.append(dict(n=n, neq=neq, m=m, N=N, **{k: round(v, 6) for k, v in best.items()}, eliminated_qps=round(N / el, 1),
                         unreduced_qps=round(N / un, 1), eliminated_warm_qps=round(N / wel, 1), unreduced_warm_qps=round(N / wun, 1),
                         max_abs_dx=err, flags_equal=ok, **(dict(backward_rel_ddz=derr, backward_status_zero=ok_bw) if a.backward else {})))
    print(json.dumps(dict(bench="eliminate", shapes=rows)))


if __name__ == "__main__":
    main()
