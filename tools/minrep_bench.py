"""tools/minrep_bench.py -- what daqp_minrep_batch costs, next to the reference's daqp_minrep on the same host.

P polyhedra of the fixture's generator (tests/golden/make_golden_minrep.py) at (n, m) = (8, 64), (12, 130), (50, 150), P swept upwards;
inputs resident on the device; setup (image + per-test state + activation) and solve launches timed with the batch's own HIP events
(DAQP_AMD_MINREP_TIMES=1 -> daqp_minrep_batch_info).  The reference (oracle/_ref/libdaqp_ref.so, its own release flags) runs the same
polyhedra through a plain process pool of 1, 4 and 16 workers; its best rate is quoted.  It skips rows it already knows (utils.c:815,
829-830), so it runs fewer than m LDPs per polyhedron: the comparison is per POLYHEDRON, the break-even P is where the GPU call (wall clock,
allocation and copies included) takes as long as the reference takes for P polyhedra on one core / on its best pool.

    python tools/minrep_bench.py [--max-tests 400000] [--ref-polyhedra 64]        -> one JSON line per (shape, P)
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(8, 64, 0), (12, 130, 0), (50, 150, 0)]
REF = os.path.join(ROOT, "oracle", "_ref", "libdaqp_ref.so")
_spec = importlib.util.spec_from_file_location("make_golden_minrep", os.path.join(ROOT, "tests", "golden", "make_golden_minrep.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _ref_chunk(args):
    A, b, ms = args
    L = C.CDLL(REF)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.daqp_minrep.argtypes = [ip, dp, dp, C.c_int, C.c_int, C.c_int]
    L.daqp_minrep.restype = None
    out = np.empty(b.shape, np.int32)
    t0 = time.perf_counter()
    for p in range(A.shape[0]):
        L.daqp_minrep(out[p].ctypes.data_as(ip), A[p].ctypes.data_as(dp), b[p].ctypes.data_as(dp), A.shape[2], b.shape[1], ms)
    return out, time.perf_counter() - t0


def reference_rate(A, b, ms):
    """polyhedra/s of the reference: one core, and the best of pools of 4 and 16 processes"""
    out, t1 = _ref_chunk((A, b, ms))
    rates = {1: A.shape[0] / t1}
    for w in (4, 16):
        if A.shape[0] < w:
            continue
        parts = [(A[i::w].copy(), b[i::w].copy(), ms) for i in range(w)]
        with ProcessPoolExecutor(w) as ex:
            list(ex.map(_ref_chunk, [(a[:1], bb[:1], ms) for a, bb, _ in parts]))      # (start the workers, load the library)
            t0 = time.perf_counter()
            list(ex.map(_ref_chunk, parts))
            rates[w] = A.shape[0] / (time.perf_counter() - t0)
    return out, rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-tests", type=int, default=400000, help="largest P * m of the sweep")
    ap.add_argument("--ref-polyhedra", type=int, default=64)
    a = ap.parse_args()
    os.environ["DAQP_AMD_MINREP_TIMES"] = "1"
    # the reference first, for every shape: its process pools are forked before this process opens the GPU
    refs = {}
    for n, m, ms in SHAPES:
        base = [G.generate(n, m, ms, s) for s in range(a.ref_polyhedra)]
        A0, b0 = np.stack([x[0] for x in base]), np.stack([x[1] for x in base])
        refs[(n, m, ms)] = (A0, b0) + reference_rate(A0, b0, ms)
    import torch
    import daqp_amd
    L = daqp_amd.lib()
    for n, m, ms in SHAPES:
        A0, b0, ref_red, ref_rates = refs[(n, m, ms)]
        P = a.ref_polyhedra
        while P * m <= a.max_tests:
            reps = P // a.ref_polyhedra
            A = torch.from_numpy(np.tile(A0, (reps, 1, 1))).cuda()
            b = torch.from_numpy(np.tile(b0, (reps, 1))).cuda()
            best = None
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                red = daqp_amd.minrep_batch(A, b, ms=ms, out="torch")
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                ts, tv, by = C.c_float(0), C.c_float(0), C.c_ulonglong(0)
                L.daqp_minrep_batch_info(C.byref(ts), C.byref(tv), C.byref(by))
                if best is None or ts.value + tv.value < best["setup_ms"] + best["solve_ms"]:
                    best = dict(setup_ms=ts.value, solve_ms=tv.value, wall_ms=1e3 * wall, device_bytes=by.value)
            same = bool(np.array_equal(red.cpu().numpy()[:a.ref_polyhedra], ref_red))
            ev_s = 1e-3 * (best["setup_ms"] + best["solve_ms"])
            best_ref = max(ref_rates.values())
            print(json.dumps(dict(n=n, m=m, P=P, tests=P * m, **{k: round(v, 3) if isinstance(v, float) else v for k, v in best.items()},
                                  polyhedra_per_s=round(P / ev_s), row_tests_per_s=round(P * m / ev_s), polyhedra_per_s_wall=round(P / (1e-3 * best["wall_ms"])),
                                  ref_polyhedra_per_s={str(k): round(v, 1) for k, v in ref_rates.items()},
                                  speedup_vs_best_ref_events=round(P / ev_s / best_ref, 1), speedup_vs_best_ref_wall=round(P / (1e-3 * best["wall_ms"]) / best_ref, 2),
                                  verdicts_equal_reference=same)), flush=True)
            P *= 4


if __name__ == "__main__":
    main()
