"""tests/golden/make_golden_fval_bound.py -- regenerate golden_fval_bound.npz from the REFERENCE library.

Runs only in the build container (needs oracle/_ref, built by oracle/Makefile from the reference's sources).  The fixture holds
inputs, the fval_bound each case ran with, and the reference's outputs (strict-IEEE build) of daqp_quadprog under that bound
(daqp.c:10,20: a dual-feasible iterate whose |u|^2 + soft slack exceeds 2 fval_bound ends the solve with -1):

  <case>/{H, f, A, bupper, blower, sense, fval_bound, x, lam, fval, exitflag, iter}     the cases of pin_oracle.fval_bound_cases(small=True),
                                                                                        n <= 12; H is empty for an LP
  warm/{n, m, ms, H, f, A, bupper, blower, f2, bounds, x, lam, fval, exitflag, iter}     pin_oracle.fval_bound_warm_sequence: three solves of one
                                                                                        workspace (bound, DAQP_INF, new f + bound)

The bounds come from each problem's own levels as the oracle traces them (between two levels; exactly half a level; the double just
below that); the outputs are the reference's alone.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from oracle.pin_oracle import fval_bound_cases, fval_bound_warm_sequence  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ora, ref = O.Oracle(), O.Reference(strict=True)
    out = {}
    flags = {}
    for name, q, kw in fval_bound_cases(ora, small=True):
        n = q["f"].size
        assert n <= 12
        x, lam, fval, flag, it = ref.quadprog(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q.get("sense"), O.default_settings(**kw))
        sense = q.get("sense")
        for k, v in dict(H=(q["H"] if q["H"] is not None else np.zeros((0, 0))), f=q["f"], A=np.ascontiguousarray(q["A"], dtype=np.float64).reshape(-1, n),
                         bupper=q["bupper"], blower=q["blower"], sense=np.zeros(q["bupper"].size, np.int32) if sense is None else np.asarray(sense, np.int32),
                         fval_bound=np.float64(kw["fval_bound"]), x=x, lam=lam, fval=np.float64(fval), exitflag=np.int32(flag), iter=np.int32(it)).items():
            out[f"{name}/{k}"] = np.asarray(v)
        flags[flag] = flags.get(flag, 0) + 1
    q, outs = fval_bound_warm_sequence(ora, lambda n, m, ms, st: ref.model(n, m, ms, settings=st))
    n, m = q["f"].size, q["bupper"].size
    for k, v in dict(n=n, m=m, ms=m - q["A"].shape[0], H=q["H"], f=q["f"], A=q["A"], bupper=q["bupper"], blower=q["blower"], f2=q["f2"], bounds=q["bounds"],
                     x=np.array([o[0] for o in outs]), lam=np.array([o[1] for o in outs]), fval=np.array([o[2] for o in outs]),
                     exitflag=np.array([o[3] for o in outs], np.int32), iter=np.array([o[4] for o in outs], np.int32)).items():
        out[f"warm/{k}"] = np.asarray(v)
    path = os.path.join(HERE, "golden_fval_bound.npz")
    np.savez_compressed(path, **out)
    print("wrote", len({k.split('/')[0] for k in out}) - 1, "fval_bound cases: exit flags", flags, "; warm flag/iter",
          [(o[3], o[4]) for o in outs], ";", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
