#!/usr/bin/env python3
"""Time of daqp_amd.certify_batch next to the solve launch of the same batch, at the C2, C3 and C4 shapes of BASELINE.md.

  python tools/bench_certify.py [--configs C2,C3,C4] [--batch N] [--steps K] [--warmup W] [--out profiles/NAME.jsonl]

Per shape: N device-resident QPs (daqp_amd.synthetic.generate_batch_torch), solved once by a BatchModel (device outputs); then
BatchModel.certify on (x, lam) of that solve, timed with HIP events around K calls after W warm-up calls (device time, the stream
drained before and after) -- the method of tools/bench_backward.py.  Reported per shape: milliseconds per certify launch; the bytes the
kernel must read (A, H, f, both bounds, x, lam) over that time as a fraction of the achievable HBM rate (ACHIEVABLE_HBM: the measured
streaming figure for MI355X, not the 8 TB/s of the data sheet); a plain fp64 streaming read of the same arrays (a torch sum over
each: what a kernel that only reads them reaches here, with the same launch overheads) and the certify rate as a fraction of that;
the forward step (setup + solve) and its solve launch alone (BatchModel.kernel_ms).  One JSON line per shape, appended to --out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"C2": (50, 150, 0, 20, 20_000), "C3": (12, 48, 12, 6, 100_000), "C4": (200, 600, 0, 80, 2_048)}     # n, m, ms, n_active, default batch
ACHIEVABLE_HBM = 6.3e12      # bytes / s


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
    ap.add_argument("--out", default=os.path.join("profiles", "certify_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import daqp_amd
    from daqp_amd.synthetic import generate_batch_torch
    for cfg in a.configs.split(","):
        n, m, ms, nact, N = SHAPES[cfg]
        N = a.batch or N
        q = generate_batch_torch(N, n, m, ms, nact, seed=1)
        bm = daqp_amd.BatchModel(N, n, m, ms)

        def forward():
            bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], None)
            return bm.solve(out="torch")

        r = forward()
        fwd_ms = timed(forward, a.steps, a.warmup)
        setup_ms, solve_ms = bm.kernel_ms()
        c = bm.certify(r)
        opt = r["exitflag"] == 1
        cert_ms = timed(lambda: bm.certify(r), a.steps, a.warmup)
        arrays = [q["A"], q["H"], q["f"], q["bupper"], q["blower"], r["x"], r["lam"]]
        nbytes = sum(t.numel() * t.element_size() for t in arrays)
        read_ms = timed(lambda: [t.sum() for t in arrays], a.steps, a.warmup)
        rate, read_rate = nbytes / (cert_ms * 1e-3), nbytes / (read_ms * 1e-3)
        rec = dict(tool="bench_certify", config=cfg, N=N, n=n, m=m, ms=ms, n_active=nact, steps=a.steps, warmup=a.warmup,
                   certify_ms=round(cert_ms, 4), certify_qps_per_s=round(N / cert_ms * 1e3), bytes_read=nbytes,
                   certify_bytes_per_s=round(rate), certify_over_achievable_hbm=round(rate / ACHIEVABLE_HBM, 4), achievable_hbm_bytes_per_s=ACHIEVABLE_HBM,
                   plain_read_ms=round(read_ms, 4), plain_read_bytes_per_s=round(read_rate), certify_over_plain_read=round(rate / read_rate, 4),
                   forward_ms=round(fwd_ms, 4), forward_setup_kernels_ms=round(setup_ms, 4), forward_solve_kernels_ms=round(solve_ms, 4),
                   certify_over_solve_launch=round(cert_ms / solve_ms, 4) if solve_ms else None, optimal=int(opt.sum()),
                   worst_relative_stationarity=float((c["stationarity"] / c["stationarity_scale"])[opt].max()), worst_primal=float(c["primal"][opt].max()),
                   worst_complementarity=float(c["complementarity"][opt].max()), wrong_sign=int(c["wrong_sign"][opt].sum()),
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
