#!/usr/bin/env python3
"""Time of BatchModel.backward next to the forward step it follows, at the two headline shapes of BASELINE.md.

  python tools/bench_backward.py [--configs C2,C3] [--soft | --soft-dual | --nullspace | --dual] [--batch N] [--steps K] [--warmup W] [--out profiles/NAME.jsonl]

Per shape: N device-resident QPs (daqp_amd.synthetic.generate_batch_torch), forward = BatchModel.setup + solve with device outputs,
backward = one BatchModel.backward on a device-resident grad_x; both timed with HIP events around K calls after W warm-up calls
(device time, the stream drained before and after).  One JSON line per shape is printed and appended to --out.
--soft: the same shapes with NS_SOFT rows per problem made SOFT and violated at the generator's optimum (rho_soft = RHO_SOFT), the batch
created with ns_max = NS_SOFT: the SOFT instantiations of the adjoint kernel, with qsoft / usoft / usoft_id written.
--nullspace: on the same positive definite batch, BatchModel.backward(nullspace="all") -- every problem through the null-space
kernel (daqp_batch_backward_nullspace, which = 1) -- timed next to the Gram adjoint and the forward step; the largest difference
between the two adjoints, relative to the max norm of the Gram adjoint's [dz; dnu], goes into the record.
--dual: on the same batch, BatchModel.backward(g, grad_lam=g_lam) -- daqp_batch_backward_dual, which = -1: the Gram adjoint with g_lam
on the working set in the second block of its right-hand side -- timed next to the plain adjoint and the forward step.
--soft-dual: the batch of --soft, and BatchModel.backward_soft(g, g_lam, g_slack, lam) -- daqp_batch_backward_soft_dual: the SOFT kernels
with g_lam and the soft_slack term in the second block -- timed next to daqp_batch_backward_soft on the same solved batch.  Only a
right-hand side differs between the two: the pair is a record, not a rate."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NS_SOFT, RHO_SOFT = 2, 0.3
SHAPES = {"C2": (50, 150, 0, 20, 20_000), "C3": (12, 48, 0, 5, 100_000)}     # n, m, ms, n_active, default batch


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--soft", action="store_true")
    ap.add_argument("--soft-dual", action="store_true")
    ap.add_argument("--nullspace", action="store_true")
    ap.add_argument("--dual", action="store_true")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "backward_bench.jsonl"))
    a = ap.parse_args()
    a.soft = a.soft or a.soft_dual
    if a.soft and (a.nullspace or a.dual):
        ap.error("--nullspace and --dual do not take soft rows")
    import torch
    import daqp_amd
    from daqp_amd.synthetic import generate_batch_torch
    for cfg in a.configs.split(","):
        n, m, ms, nact, N = SHAPES[cfg]
        N = a.batch or N
        q = generate_batch_torch(N, n, m, ms, nact, seed=1)
        sense = None
        if a.soft:      # the NS_SOFT general rows furthest from their bounds at the optimum: soft, upper bound 0.2 .. 0.5 below their value there
            ax = torch.einsum("qik,qk->qi", q["A"], q["xref"])
            slack = torch.minimum(q["bupper"][:, ms:] - ax, ax - q["blower"][:, ms:])
            rows = slack.topk(NS_SOFT, dim=1).indices
            sense = torch.zeros((N, m), dtype=torch.int32, device="cuda")
            sense.scatter_(1, rows + ms, 8)
            gen = torch.Generator(device="cuda").manual_seed(2)
            bu = ax.gather(1, rows) - (0.2 + 0.3 * torch.rand((N, NS_SOFT), dtype=torch.float64, device="cuda", generator=gen))
            q["bupper"].scatter_(1, rows + ms, bu)
            q["blower"].scatter_(1, rows + ms, bu - 1.0)
        bm = daqp_amd.BatchModel(N, n, m, ms, NS_SOFT, rho_soft=RHO_SOFT) if a.soft else daqp_amd.BatchModel(N, n, m, ms)

        def forward():
            bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], sense)
            return bm.solve(out="torch")

        r = forward()
        g = torch.randn(N, n, dtype=torch.float64, device="cuda")
        o = bm.backward(g)
        ok = int((o["status"] == 0).sum())
        fwd_ms = timed(forward, a.steps, a.warmup)
        setup_ms, solve_ms = bm.kernel_ms()
        bwd_ms = timed(lambda: bm.backward(g), a.steps, a.warmup)
        extra = {}
        if a.nullspace:
            o2 = bm.backward(g, nullspace="all")
            scale = torch.maximum(o["dz"].abs().amax(1), (o["dbupper"] + o["dblower"]).abs().amax(1))
            diff = torch.maximum((o2["dz"] - o["dz"]).abs().amax(1), (o2["dbupper"] + o2["dblower"] - o["dbupper"] - o["dblower"]).abs().amax(1))
            both = (o["status"] == 0) & (o2["status"] == 0)
            ns_ms = timed(lambda: bm.backward(g, nullspace="all"), a.steps, a.warmup)
            extra = dict(nullspace=True, nullspace_ms=round(ns_ms, 4), nullspace_over_backward=round(ns_ms / bwd_ms, 4),
                         nullspace_over_forward=round(ns_ms / fwd_ms, 4), nullspace_qps_per_s=round(N / ns_ms * 1e3),
                         nullspace_status_ok=int((o2["status"] == 0).sum()), nullspace_max_rel_diff=float((diff / scale)[both].max()))
        if a.dual:
            gl = torch.randn(N, m, dtype=torch.float64, device="cuda")
            o3 = bm.backward(g, grad_lam=gl)
            dual_ms = timed(lambda: bm.backward(g, grad_lam=gl), a.steps, a.warmup)
            extra.update(dual=True, dual_ms=round(dual_ms, 4), dual_over_backward=round(dual_ms / bwd_ms, 4),
                         dual_over_forward=round(dual_ms / fwd_ms, 4), dual_status_ok=int((o3["status"] == 0).sum()))
        if a.soft_dual:
            gl, gs = torch.randn(N, m, dtype=torch.float64, device="cuda"), torch.randn(N, dtype=torch.float64, device="cuda")
            o4 = bm.backward_soft(g, gl, gs, r["lam"])
            sd_ms = timed(lambda: bm.backward_soft(g, gl, gs, r["lam"]), a.steps, a.warmup)
            extra.update(soft_dual=True, soft_dual_ms=round(sd_ms, 4), soft_dual_over_backward=round(sd_ms / bwd_ms, 4),
                         soft_dual_over_forward=round(sd_ms / fwd_ms, 4), soft_dual_status_ok=int((o4["status"] == 0).sum()))
        rec = dict(tool="bench_backward", config=cfg, N=N, n=n, m=m, ms=ms, n_active=nact, steps=a.steps, warmup=a.warmup,
                   forward_ms=round(fwd_ms, 4), forward_setup_kernels_ms=round(setup_ms, 4), forward_solve_kernels_ms=round(solve_ms, 4),
                   backward_ms=round(bwd_ms, 4), backward_over_forward=round(bwd_ms / fwd_ms, 4),
                   backward_qps_per_s=round(N / bwd_ms * 1e3), status_ok=ok, optimal=int((r["exitflag"] == 1).sum()),
                   **(dict(soft=True, ns_max=NS_SOFT, rho_soft=RHO_SOFT, soft_optimal=int((r["exitflag"] == 2).sum()),
                           soft_rows_active=int((o["usoft_id"] >= 0).sum())) if a.soft else {}), **extra,
                   device=torch.cuda.get_device_name(0), version=daqp_amd.lib().daqp_amd_version().decode())
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        bm.close()


if __name__ == "__main__":
    main()
