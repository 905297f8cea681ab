#!/usr/bin/env python3
"""Time of BatchModel.refine (daqp_batch_refine) next to the solve launch of the same batch, at the C2, C3 and C4 shapes of BASELINE.md.

  python tools/bench_refine.py [--configs C2,C3,C4] [--batch N] [--steps K] [--warmup W] [--max-steps S] [--out profiles/TAG_refine_bench.jsonl]

Per shape: N device-resident QPs (daqp_amd.synthetic.generate_batch_torch), solved once by a BatchModel (device outputs); then
BatchModel.refine on (x, lam) of that solve, timed with HIP events around K calls after W warm-up calls (device time, the stream drained
before and after; the time includes the copies of x and lam the wrapper makes) -- the method of tools/bench_certify.py.  Reported per
shape: milliseconds per call, the forward step (setup + solve) and its solve launch alone (BatchModel.kernel_ms), the steps kept and the
merit before and after.  No rate is promised for this kernel: the file records what it costs.  One JSON line per shape, appended to --out.

  python tools/bench_refine.py --nullspace [--configs C2,C3] [--batch N] ...

--nullspace: BatchModel.refine(nullspace=True) (daqp_batch_refine_nullspace, which = 0) on the problems daqp_batch_refine hands back:
per shape (n <= 64 only) a singular-H batch -- the shape's f, A and bounds with H = B'B of rank n / 2 -- and an LP batch (H = None),
both through the proximal loop.  The same timing; next to it the forward step and its solve launches (all of the proximal loop's), the
statuses (-20: the optimum is not locally unique, an LP off a vertex: such a problem is left as it came in), the steps kept and the
merit before and after.  One JSON line per shape and kind."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"C2": (50, 150, 0, 20, 20_000), "C3": (12, 48, 12, 6, 100_000), "C4": (200, 600, 0, 80, 2_048)}     # n, m, ms, n_active, default batch


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
    ap.add_argument("--configs", default="C2,C3,C4")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-steps", type=int, default=3)
    ap.add_argument("--nullspace", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "local_refine_bench.jsonl"))      # (profiles/*_refine_bench.jsonl; committed runs carry their own tag)
    a = ap.parse_args()
    import torch
    import daqp_amd
    from daqp_amd.synthetic import generate_batch_torch
    runs = [(cfg, "definite") for cfg in a.configs.split(",")]
    if a.nullspace:
        runs = [(cfg, kind) for cfg in a.configs.split(",") if SHAPES[cfg][0] <= 64 for kind in ("singular", "lp")]
    for cfg, kind in runs:
        n, m, ms, nact, N = SHAPES[cfg]
        N = a.batch or (min(N, 4_096) if a.nullspace else N)      # (the proximal loop synchronises with the host once per outer iteration)
        q = generate_batch_torch(N, n, m, ms, nact, seed=1)
        if kind == "singular":
            Bm = torch.randn((N, n // 2, n), dtype=torch.float64, device=q["f"].device, generator=torch.Generator(q["f"].device).manual_seed(2))
            q["H"] = Bm.transpose(1, 2) @ Bm
        elif kind == "lp":
            q["H"] = None
        bm = daqp_amd.BatchModel(N, n, m, ms)

        def forward():
            bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], None)
            return bm.solve(out="torch")

        r = forward()
        fwd_ms = timed(forward, a.steps, a.warmup)
        setup_ms, solve_ms = bm.kernel_ms()
        refine = (lambda: bm.refine(r, max_steps=a.max_steps, nullspace=True)) if a.nullspace else (lambda: bm.refine(r, max_steps=a.max_steps))
        o = refine()
        ok = o["status"] == 0
        ref_ms = timed(refine, a.steps, a.warmup)
        extra = {}
        if a.nullspace:
            st = o["status"].cpu().numpy()
            extra = dict(nullspace=True, kind=kind, exit_optimal=int((r["exitflag"] == 1).sum()), n_prox_problems=int((bm.prox_info()["n_prox"] > 0).sum()),
                         status_counts={str(int(v)): int((st == v).sum()) for v in sorted(set(st.tolist()))})
        if not bool(ok.any()):
            ok = torch.ones_like(ok)
        rec = dict(tool="bench_refine", config=cfg, N=N, n=n, m=m, ms=ms, n_active=nact, steps=a.steps, warmup=a.warmup, max_steps=a.max_steps, **extra,
                   refine_ms=round(ref_ms, 4), refine_qps_per_s=round(N / ref_ms * 1e3),
                   forward_ms=round(fwd_ms, 4), forward_setup_kernels_ms=round(setup_ms, 4), forward_solve_kernels_ms=round(solve_ms, 4),
                   refine_over_solve_launch=round(ref_ms / solve_ms, 4) if solve_ms else None, refine_over_forward=round(ref_ms / fwd_ms, 4),
                   status_zero=int(ok.sum()), kept_steps_mean=float(o["steps"][ok].double().mean()), kept_steps_max=int(o["steps"][ok].max()),
                   worst_merit_before=float(o["residual_before"][ok].max()), worst_merit_after=float(o["residual_after"][ok].max()),
                   largest_change_of_x=float((o["x"] - r["x"])[ok].abs().max()),
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
