"""tests/golden/make_golden_minrep_truth.py -- golden_minrep_truth.npz: the REFERENCE's daqp_minrep verdicts (strict-IEEE build,
oracle/_ref: build container only; CPU only) on the near-margin polyhedra of tests/minrep_cases.py, rows normalised to unit length
as the GPU path sees them.

Recorded results only: the inputs come from the generator (tests/minrep_cases.py), the truth from its certificates.  Per shape and
near delta, key "n_m_ms_delta":
  red_<key>     (P, m) int8   the reference's verdicts
  stable_<key>  (P, m) int8   1 where the verdict is the same with every b_i pushed by a relative 1e-9 up and down (what a
                              comparison may fall back on where the row normalisation's own rounding decides a verdict)

--measure prints, for every clear and near delta, how often the reference on normalised and on raw rows differs from the truth
(the figures quoted at the top of tests/minrep_cases.py); nothing is written.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import minrep_cases as MC  # noqa: E402

PUSH = 1e-9


def ref_minrep():
    spec = importlib.util.spec_from_file_location("make_golden_minrep", os.path.join(HERE, "make_golden_minrep.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G.RefMinrep()


def record(ref, shape, delta):
    """(red, stable) of the P cases of a shape and a delta, on normalised rows"""
    reds, stables = [], []
    for case in MC.cases(shape, delta):
        An, bn = MC.normalised(case)
        red = ref(An, bn, shape[2])
        up, dn = ref(An, bn + PUSH * np.abs(bn), shape[2]), ref(An, bn - PUSH * np.abs(bn), shape[2])
        reds.append(red)
        stables.append((up == red) & (dn == red))
    return np.stack(reds).astype(np.int8), np.stack(stables).astype(np.int8)


def measure(ref):
    print("delta     rows   | normalised: missed redundant, core called redundant | raw: missed redundant, core called redundant")
    for delta in MC.CLEAR_ALL + MC.NEAR:
        tot = np.zeros(5, np.int64)
        worst = {}
        for shape in MC.SHAPES:
            for case in MC.cases(shape, delta):
                An, bn = MC.normalised(case)
                t = case["truth"]
                rn, rr = ref(An, bn, shape[2]), ref(case["A"], case["b"], shape[2])
                row = np.array([t.size, ((t == 1) & (rn != 1)).sum(), ((t == 0) & (rn != 0)).sum(), ((t == 1) & (rr != 1)).sum(),
                                ((t == 0) & (rr != 0)).sum()])
                tot += row
                if row[1:].any():
                    worst[(shape, case["seed"])] = row[1:].tolist()
        print(f"{delta:7.0e} {tot[0]:6d}   | {tot[1]:5d} {tot[2]:5d} | {tot[3]:5d} {tot[4]:5d}   {worst}")
    nb = np.concatenate([c["b"] for s in MC.SHAPES for d in MC.CLEAR_ALL + MC.NEAR for c in MC.cases(s, d)])
    print(f"negative b: {(nb < 0).mean():.3f} of {nb.size}")


def main():
    ref = ref_minrep()
    if "--measure" in sys.argv:
        return measure(ref)
    out = {}
    for shape in MC.SHAPES:
        for delta in MC.NEAR:
            for case in MC.cases(shape, delta):
                MC.verify(case)
            red, stable = record(ref, shape, delta)
            key = MC.fixture_key(shape, delta)
            out["red_" + key], out["stable_" + key] = red, stable
            truth = MC.stack(MC.cases(shape, delta))[2]
            assert not ((truth == 0) & (red != 0)).any(), f"the reference drops a core row at {key}"
            print(f"{key}: redundant {int((truth == 1).sum())}, missed by the reference {int(((truth == 1) & (red != 1)).sum())}, "
                  f"unstable under a {PUSH:g} push {int((stable == 0).sum())}")
    path = os.path.join(HERE, "golden_minrep_truth.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
