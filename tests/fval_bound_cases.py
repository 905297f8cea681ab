"""Cases of the fval_bound tests (DAQPSettings.fval_bound, daqp.c:10,20: a dual-feasible iterate whose internal objective
|u|^2 + soft slack exceeds 2 fval_bound ends the solve with DAQP_EXIT_INFEASIBLE), as data: for every kernel family and variant of
tests/kkt_cases.py the bounds -- one number per batch -- chosen from the levels the ORACLE passes (OracleModel.enable_levels: w->fval at
every dual-feasible iterate, the value the test compares).  tests/test_cpu_fval_bound.py asserts the conditions below on the oracle alone;
tests/test_gpu_fval_bound.py runs the GPU at the same bounds.

  early   the largest clear bound at which at least one problem stops at its FIRST dual-feasible iterate
  mixed   some problem stops strictly inside its run (not at its first level, not at its last), some problem runs to its unbounded
          result; among such bounds one whose count of stopped problems is no power of two if there is one, and nearest to N - 1 (N a
          power of two: N / 2 + 1, so that the second pass's companion batch, sized to a power of two, has unused slots)
  all     the largest clear bound at which every problem stops (late in its run for the problem with the lowest final level)
  none    above every problem's final level: the unbounded solve
  tight   (exact mode only) problem TIGHT_k and one of its levels l: fval_bound = l / 2 exactly -- the comparison is >, the problem
          does not stop there -- and the double just below, where it does

"clear": no level of any problem of the batch lies within OFFSET = 100 x kkt_cases.BARS["qp"]["fval"][1] = 1e-9 of 2 fval_bound, relative to
max(1, |level|) -- 100 x the project's bar on the default mode's fval error, so the exit cannot flip between the arithmetic modes, and nine
orders of magnitude below an fp32-sized error.  No exclusions: a candidate with any level of any problem inside that band is not taken.

Candidates are the midpoints of neighbouring values of the union of all levels of the batch (and one below the smallest level).

The table RECORDED was printed by `python tests/fval_bound_cases.py` (which runs search() on every family and variant); per entry:
bound, problems stopped / N, smallest .. largest exit iteration of the batch at that bound.  test_cpu_fval_bound.py asserts that search()
still gives these bounds (to 1e-12 relative: see bound()) with exactly these counts and iterations.  Every family and variant meets `mixed`, rows520 and wg130 with their 2 and 3 problems included.
"""
import functools
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kkt_cases as K
from oracle import oracle as O

VARIANTS = ("plain", "sense")
KINDS = ("early", "mixed", "all", "none")
OFFSET = 100.0 * K.BARS["qp"]["fval"][1]
PROX_REL = 1e-6
DAQP_INF = 1e30


@functools.lru_cache(maxsize=None)
def _oracle():
    return O.Oracle()


def settings(bound):
    return O.default_settings(fval_bound=float(bound))


def run(p, bound, init_mask=0):
    """the oracle's solve of every problem of p under fval_bound = bound: K.oracle_solve's dict, with ["levels"] (one array per problem)
    and ["ws"] (the working sets left behind) added"""
    models = []
    for k in range(p["N"]):
        om = _oracle().model(p["n"], p["m"], p["ms"], ns=p["ns_max"], settings=settings(bound))
        om.enable_levels()
        assert om.setup(*K.problem(p, k), init_mask=init_mask) >= 0
        models.append(om)
    out = K.oracle_solve(models)
    out["levels"] = [om.get_levels() for om in models]
    out["ws"] = [om.state()[0] for om in models]
    return out


@functools.lru_cache(maxsize=None)
def unbounded(data, variant):
    """the unbounded oracle solve of a data set (families that differ only in their environment share it), with its levels"""
    return run(K.problems(data, variant), DAQP_INF)


def data_of(name):
    return K.family(name).get("data", name)


def clear(levels, bound, offset=OFFSET):
    lv = np.concatenate(levels)
    return bool(np.all(np.abs(lv - 2.0 * bound) > offset * np.maximum(1.0, np.abs(lv))))


def stop_index(lv, bound):
    """index of the first level above 2 bound (where the solve stops), or -1"""
    over = np.flatnonzero(lv > 2.0 * bound)
    return int(over[0]) if over.size else -1


def classify(levels, bound):
    """per problem: 'first', 'inside', 'last' (the level it stops at) or 'runs'"""
    out = []
    for lv in levels:
        j = stop_index(lv, bound)
        out.append("runs" if j < 0 else "first" if j == 0 else "last" if j == lv.size - 1 else "inside")
    return out


def search(levels):
    """dict(early, mixed, all, none, tight=(problem, level index, bound at, bound below)) for one batch; a kind that no clear candidate meets
    is missing"""
    u = np.unique(np.concatenate(levels))
    cands = [0.5 * (u[0] - 1.0)] + [0.25 * (a + b) for a, b in zip(u[:-1], u[1:])]
    cands = [b for b in cands if clear(levels, b)]
    N = len(levels)
    out = {"none": 0.5 * u[-1] + 1.0}
    best_mixed = None
    target = N - 1 if N & (N - 1) else N // 2 + 1      # (N a power of two: a count whose companion batch is padded, not N - 1)
    for b in cands:
        c = classify(levels, b)
        stopped = N - c.count("runs")
        if "first" in c:
            out["early"] = b
        if stopped == N:
            out["all"] = b
        if "inside" in c and "runs" in c:
            score = (stopped & (stopped - 1) != 0, -abs(stopped - target))
            if best_mixed is None or score > best_mixed[0]:
                best_mixed = (score, b)
    if best_mixed is not None:
        out["mixed"] = best_mixed[1]
    k = int(np.argmax([np.unique(lv).size for lv in levels]))
    uk = np.unique(levels[k])
    uk = uk[uk > 0]
    lvl = uk[uk.size // 2]
    j = int(np.flatnonzero(levels[k] == lvl)[0])
    assert 2.0 * (0.5 * lvl) == lvl
    out["tight"] = (k, j, 0.5 * lvl, float(np.nextafter(0.5 * lvl, -np.inf)))
    return out


# name of the data set -> variant -> kind -> (bound, stopped, N, min exit iteration, max exit iteration); tight -> (problem, level index, bound at)
# printed by `python tests/fval_bound_cases.py`
RECORDED = {
    "tiny": {
        "plain": {"early": (-0.5, 16, 16, 1, 1), "mixed": (7.185278088007117, 9, 16, 2, 17), "all": (2.8730341262788635, 16, 16, 2, 7), "none": (17.019488194661008, 0, 16, 7, 27), "tight": (15, 9, 7.747546022392606)},
        "sense": {"early": (4.481616919957666, 15, 16, 1, 14), "mixed": (6.870450745896587, 9, 16, 2, 18), "all": (4.463002777239282, 16, 16, 1, 14), "none": (15.198789102358036, 0, 16, 8, 22), "tight": (6, 8, 8.663617279735238)},
    },
    "reg20": {
        "plain": {"early": (-0.5, 16, 16, 1, 1), "mixed": (21.405347231957652, 9, 16, 3, 25), "all": (12.06222235292855, 16, 16, 2, 17), "none": (34.22425660239001, 0, 16, 9, 25), "tight": (12, 9, 14.005870992241206)},
        "sense": {"early": (15.200165716875897, 14, 16, 1, 18), "mixed": (21.950138233671147, 9, 16, 2, 28), "all": (9.874293768657747, 16, 16, 1, 13), "none": (90.39094686862124, 0, 16, 13, 33), "tight": (14, 13, 26.33499270485102)},
    },
    "reg21": {
        "plain": {"early": (-0.5, 16, 16, 1, 1), "mixed": (21.290493943817935, 9, 16, 2, 10), "all": (8.586926460397216, 16, 16, 2, 8), "none": (63.47925880657782, 0, 16, 8, 10), "tight": (5, 5, 11.462908933325544)},
        "sense": {"early": (6.253817755599291, 15, 16, 1, 13), "mixed": (18.230796609574305, 9, 16, 2, 24), "all": (6.064474615422898, 16, 16, 1, 13), "none": (48.15922454860335, 0, 16, 11, 33), "tight": (13, 13, 18.512846119545117)},
    },
    "reg26": {
        "plain": {"early": (-0.5, 16, 16, 1, 1), "mixed": (15.33756591266296, 9, 16, 2, 15), "all": (1.8709773227280952, 16, 16, 2, 11), "none": (43.75921323925426, 0, 16, 11, 15), "tight": (12, 7, 13.463111911716245)},
        "sense": {"early": (13.038428950753591, 15, 16, 1, 29), "mixed": (20.658798341864788, 9, 16, 2, 29), "all": (10.063229830794153, 16, 16, 1, 29), "none": (52.00652619644547, 0, 16, 12, 40), "tight": (6, 16, 28.395375493550226)},
    },
    "rows193": {
        "plain": {"early": (-0.5, 12, 12, 1, 1), "mixed": (3.9031797687262726, 11, 12, 2, 35), "all": (3.5971089429804293, 12, 12, 2, 35), "none": (34.38336316949637, 0, 12, 7, 39), "tight": (0, 12, 15.072968489066831)},
        "sense": {"early": (8.160619422793165, 9, 12, 1, 33), "mixed": (3.6527819927769896, 11, 12, 1, 33), "all": (3.6074029307183952, 12, 12, 1, 33), "none": (35.43745949602797, 0, 12, 12, 49), "tight": (5, 16, 27.93366890447045)},
    },
    "blk41": {
        "plain": {"early": (-0.5, 12, 12, 1, 1), "mixed": (24.528713863851358, 11, 12, 2, 13), "all": (24.41047960767554, 12, 12, 2, 13), "none": (97.20507280444261, 0, 12, 13, 13), "tight": (0, 7, 44.84844393920569)},
        "sense": {"early": (4.910387985317334, 12, 12, 1, 2), "mixed": (21.12658800447785, 11, 12, 2, 28), "all": (19.520743316036043, 12, 12, 2, 28), "none": (105.5876314005993, 0, 12, 17, 40), "tight": (8, 19, 104.52884335010471)},
    },
    "blk63": {
        "plain": {"early": (-0.5, 12, 12, 1, 1), "mixed": (65.5861024795996, 11, 12, 3, 21), "all": (65.52676929548225, 12, 12, 3, 21), "none": (142.44615765147088, 0, 12, 21, 23), "tight": (0, 11, 133.58750296579305)},
        "sense": {"early": (8.639843776734756, 12, 12, 1, 2), "mixed": (36.78515238447427, 11, 12, 2, 48), "all": (32.59318542489391, 12, 12, 2, 48), "none": (173.2356039502293, 0, 12, 31, 68), "tight": (8, 31, 111.21135689259681)},
    },
    "reg64": {
        "plain": {"early": (-0.5, 12, 12, 1, 1), "mixed": (179.04416252473231, 11, 12, 2, 31), "all": (177.9377685740461, 12, 12, 2, 31), "none": (727.5253737114191, 0, 12, 31, 85), "tight": (8, 29, 384.06852528758276)},
        "sense": {"early": (21.63097621388885, 12, 12, 1, 2), "mixed": (186.61390658858292, 11, 12, 4, 75), "all": (186.34879505581057, 12, 12, 4, 75), "none": (348.63656794237414, 0, 12, 36, 130), "tight": (0, 45, 267.6443628428924)},
    },
    "img3": {
        "plain": {"early": (-0.5, 12, 12, 1, 1), "mixed": (112.33387051877503, 11, 12, 4, 39), "all": (112.27099211662131, 12, 12, 4, 39), "none": (231.52861366931322, 0, 12, 21, 55), "tight": (0, 19, 187.58678598992395)},
        "sense": {"early": (19.692421880802932, 12, 12, 1, 3), "mixed": (81.6246881398148, 11, 12, 3, 53), "all": (81.37591159461508, 12, 12, 3, 53), "none": (182.4950785767826, 0, 12, 29, 153), "tight": (8, 50, 123.22321752841435)},
    },
    "img2": {
        "plain": {"early": (-0.5, 12, 12, 1, 1), "mixed": (112.60998873910424, 11, 12, 3, 21), "all": (111.61768878817773, 12, 12, 3, 21), "none": (265.47834106563465, 0, 12, 21, 25), "tight": (2, 12, 128.947613537133)},
        "sense": {"early": (18.014845945264547, 12, 12, 1, 3), "mixed": (97.31171788265931, 11, 12, 3, 49), "all": (97.18791338065193, 12, 12, 3, 49), "none": (231.01646309379535, 0, 12, 29, 86), "tight": (2, 36, 229.9593429073501)},
    },
    "spill": {
        "plain": {"early": (-0.5, 12, 12, 1, 1), "mixed": (8.773149215677428, 11, 12, 2, 13), "all": (8.398778015489802, 12, 12, 2, 13), "none": (44.73044307857382, 0, 12, 9, 35), "tight": (0, 11, 41.924644612363025)},
        "sense": {"early": (3.7234990389065628, 12, 12, 1, 3), "mixed": (7.1305817935401254, 11, 12, 2, 14), "all": (6.706034199276374, 12, 12, 2, 14), "none": (40.69999357739394, 0, 12, 12, 33), "tight": (1, 14, 30.06969076046255)},
    },
    "wg70": {
        "plain": {"early": (-0.5, 8, 8, 1, 1), "mixed": (247.81813455296276, 5, 8, 7, 28), "all": (190.8900619313984, 8, 8, 5, 26), "none": (371.0775886151145, 0, 8, 26, 30), "tight": (1, 14, 280.8793972584322)},
        "sense": {"early": (25.44816660216751, 8, 8, 1, 2), "mixed": (288.0836934877451, 5, 8, 11, 73), "all": (236.3573865391222, 8, 8, 7, 35), "none": (340.40032046748047, 0, 8, 34, 134), "tight": (2, 50, 338.8519024425741)},
    },
    "wg130": {
        "plain": {"early": (-0.5, 3, 3, 1, 1), "mixed": (826.4131527857202, 2, 3, 16, 57), "all": (821.9944427538562, 3, 3, 16, 57), "none": (1168.4296473517695, 0, 3, 55, 197), "tight": (1, 62, 1144.243674937767)},
        "sense": {"early": (22.38694630962912, 3, 3, 1, 2), "mixed": (794.5318191842341, 2, 3, 10, 164), "all": (793.7427670891695, 3, 3, 10, 163), "none": (1343.9980984477295, 0, 3, 164, 236), "tight": (0, 86, 1162.1640634558494)},
    },
    "rows520": {
        "plain": {"early": (-0.5, 2, 2, 1, 1), "mixed": (3217.813463678888, 1, 2, 49, 71), "all": (3213.758125635288, 2, 2, 49, 71), "none": (3366.8990356065224, 0, 2, 71, 73), "tight": (0, 36, 2933.720637769816)},
        "sense": {"early": (17.729860736257233, 2, 2, 1, 2), "mixed": (2515.1807591458364, 1, 2, 26, 130), "all": (2504.559951079288, 2, 2, 26, 120), "none": (3218.425599602134, 0, 2, 130, 603), "tight": (0, 215, 3214.238838792721)},
    },
}
# proximal families: bound, problems ending -1 / N at it (found by bisection on the oracle, see prox_search)
PROX_RECORDED = {
    "singular12": (131071.5, 1, 8),
    "singular24": (131071.5, 1, 8),
    "lp12": (511.5, 2, 8),
    "lp24": (16383.5, 2, 8),
}


def bound(name, variant, kind):
    """the recorded bound of a family.  kind 'tight': (problem, level index, bound at, bound just below), taken from the levels as they are
    on this machine -- the generators go through BLAS, whose last bits differ between processors for the larger shapes, and this bound
    has to be exactly half a level; RECORDED keeps the problem, the index and the value it had where the table was printed"""
    if kind == "tight":
        return search(unbounded(data_of(name), variant)["levels"])["tight"]
    return RECORDED[data_of(name)][variant][kind][0]


def split_bound(levels):
    """a clear bound that stops some problems of the batch and not others, the middle one of all such candidates (for batches whose
    levels are only known at test time: warm steps, shared setups); None if there is none"""
    u = np.unique(np.concatenate(levels))
    ok = [b for b in (0.25 * (a + c) for a, c in zip(u[:-1], u[1:]))
          if clear(levels, b) and 0 < sum(stop_index(lv, b) >= 0 for lv in levels) < len(levels)]
    return ok[len(ok) // 2] if ok else None


def _solve_with_levels(models):
    out = K.oracle_solve(models)
    out["levels"] = [om.get_levels() for om in models]
    out["ws"] = [om.state()[0] for om in models]
    return out


@functools.lru_cache(maxsize=None)
def warm_reference(name, variant):
    """the oracle's side of test_warm_and_continue: [cold solve under `mixed`, the solve after fval_bound went back to DAQP_INF (continues
    from the kept working set), the solve after warm_steps' first f update under a finite bound], that bound, the new f.  The last bound
    splits the levels of the warm step (run once without a bound to learn them) and is clear of all of them."""
    p = K.problems(name, variant)
    f2 = K.warm_steps(name, variant)[0][1]["f"]

    def sequence(b3):
        models = []
        for k in range(p["N"]):
            om = _oracle().model(p["n"], p["m"], p["ms"], ns=p["ns_max"], settings=settings(bound(name, variant, "mixed")))
            om.enable_levels()
            assert om.setup(*K.problem(p, k), init_mask=0) >= 0
            models.append(om)
        outs = [_solve_with_levels(models)]
        for om in models:
            om.settings(fval_bound=DAQP_INF)
        outs.append(_solve_with_levels(models))
        for k, om in enumerate(models):
            om.settings(fval_bound=b3)
            assert om.update(O.UPDATE_v, f=f2[k]) == 0
        outs.append(_solve_with_levels(models))
        return outs

    b3 = split_bound(sequence(DAQP_INF)[2]["levels"])
    assert b3 is not None, (name, variant)
    return sequence(b3), b3, f2


@functools.lru_cache(maxsize=None)
def shared_reference(name):
    """test_gpu_kkt.test_kkt_shared's batch (one H and A, per-problem f and bounds) under a bound that splits its own levels:
    dict(H, A, f, bupper, blower, bound, ref = the oracle's solves, levels)"""
    fam, p = K.family(name), K.problems(name, "plain")
    N, n, m, ms = p["N"], p["n"], p["m"], p["ms"]
    H, A = p["H"][0], p["A"][0]
    rng = np.random.default_rng([K.seed_of(fam.get("data", name)), 78])
    f = p["f"][0][None, :] + 0.02 * rng.standard_normal((N, n))
    shift = 0.005 * rng.standard_normal((N, m))
    bu, bl = p["bupper"][0][None, :] + shift, p["blower"][0][None, :] + shift

    def solve(b):
        models = []
        for k in range(N):
            om = _oracle().model(n, m, ms, settings=settings(b))
            om.enable_levels()
            assert om.setup(H, f[k], A, np.full(m, 1e30), np.full(m, -1e30), None) >= 0
            assert om.update(O.UPDATE_v | O.UPDATE_d, f=f[k], bupper=bu[k], blower=bl[k]) == 0
            models.append(om)
        return _solve_with_levels(models)

    b = split_bound(solve(DAQP_INF)["levels"])
    assert b is not None, name
    return dict(H=H, A=A, f=f, bupper=bu, blower=bl, bound=b, ref=solve(b), N=N, n=n, m=m, ms=ms)


def single_bound(name, variant, k=1):
    """problem k of a family on its own: a bound between two of its middle levels (it stops strictly inside its run), clear of all of them"""
    lv = unbounded(data_of(name), variant)["levels"][k]
    u = np.unique(lv)
    for j in range(u.size // 2, u.size - 1):
        b = 0.25 * (u[j - 1] + u[j])
        if clear([lv], b):
            return b
    raise AssertionError((name, variant))


def prox_run(p, bound):
    """daqp_quadprog (init mask 64 + 128) of a proximal family on the oracle under the bound"""
    models = []
    for k in range(p["N"]):
        om = _oracle().model(p["n"], p["m"], p["ms"], settings=settings(bound))
        assert om.setup(*K.problem(p, k), init_mask=64 + 128) >= 0
        models.append(om)
    return K.oracle_solve(models)


def prox_stable(p, b):
    r0 = prox_run(p, b)
    return all(np.array_equal(r[key], r0[key]) for r in (prox_run(p, b * (1 - PROX_REL)), prox_run(p, b * (1 + PROX_REL))) for key in ("exitflag", "iter"))


def prox_search(name):
    """a bound at which some problems of a proximal family end -1 and some do not, stable under a relative +-PROX_REL change: the
    levels belong to the inner subproblems, so the bound is found by bisection between one where every problem stops and one where none does"""
    p = K.prox_problems(name)
    N = p["N"]
    lo, hi = -1.0, 1.0
    while (prox_run(p, hi)["exitflag"] == -1).any():
        hi *= 2.0
    while not (prox_run(p, lo)["exitflag"] == -1).all():
        lo *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        stopped = int((prox_run(p, mid)["exitflag"] == -1).sum())
        if 0 < stopped < N and prox_stable(p, mid):
            return mid, stopped
        if stopped * 2 >= N:
            lo = mid
        else:
            hi = mid
    raise AssertionError(f"{name}: no stable mixed bound found")


def prox_bound(name):
    return PROX_RECORDED[name][0]


def _main():
    print("RECORDED = {")
    for data in K.DATA_SETS:
        print(f'    "{data}": {{')
        for variant in VARIANTS:
            p = K.problems(data, variant)
            levels = unbounded(data, variant)["levels"]
            s = search(levels)
            row = []
            for kind in KINDS:
                r = run(p, s[kind])
                row.append(f'"{kind}": ({float(s[kind])!r}, {int((r["exitflag"] == -1).sum())}, {p["N"]}, {int(r["iter"].min())}, {int(r["iter"].max())})')
            k, j, at, _ = s["tight"]
            row.append(f'"tight": ({k}, {j}, {float(at)!r})')
            print(f'        "{variant}": {{' + ", ".join(row) + "},")
        print("    },")
    print("}")
    print("PROX_RECORDED = {")
    for fam in K.PROX_FAMILIES:
        b, stopped = prox_search(fam["name"])
        print(f'    "{fam["name"]}": ({float(b)!r}, {stopped}, {fam["N"]}),')
    print("}")


if __name__ == "__main__":
    _main()
