"""DAQPSettings.fval_bound (daqp.c:10,20) on every solve kernel family: a dual-feasible iterate whose |u|^2 + soft slack exceeds
2 fval_bound ends the solve with -1.  The bounds are those of tests/fval_bound_cases.py -- chosen from the levels the oracle passes, every
level of every problem at least 1e-9 (relative) away from 2 fval_bound, tests/test_cpu_fval_bound.py -- so flag AND iteration count must
equal the oracle's in both arithmetic modes: a stop one iterate early or late (>= for >, the bound not doubled, the test placed after
the next row is added, fval taken through fp32) changes the iteration count of some problem of some bound.  In the default mode a cold
solve sends every stopped problem through the second pass (recheck.hip.h): all N, one, or a count that is no power of two.

Next to the oracle, a check without solver code (kkt_reference.half_f_hinv_f / dual_value, longdouble) on every stopped problem:
  1. fval + 1/2 f'H^-1 f > fval_bound                              (the stop was due)
  2. fval <= fval_opt + RELTOL max(1, |fval_opt|)                    (weak duality; fval_opt: the unbounded solve, certified by test_gpu_kkt)
  3. the level before the one the GPU stopped at is <= 2 fval_bound  (the stop is not late)
  4. the dual function at lam / sqrt(q_k) equals fval at the fval bar (lam at a negative exit is the least-distance problem's,
     api.c:27 -- established on the oracle by test_cpu_fval_bound.test_lam_at_the_bound_exit_is_in_ldp_units)
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fval_bound_cases as F
import kkt_cases as K
import kkt_reference as R
from oracle import oracle as O
from test_gpu_kkt import FAMILY_NAMES, LAMTOL, RELTOL, XTOL, bits_equal, rel, set_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FVAL_BAR = K.BARS["qp"]["fval"][1]
NEG_KEYS = ("fval", "lam", "soft_slack")      # what the sibling files compare at a negative exit


@functools.lru_cache(maxsize=None)
def oracle_run(data, variant, bound, init_mask):
    return F.run(K.problems(data, variant), bound, init_mask=init_mask)


@functools.lru_cache(maxsize=None)
def problem_constants(data, variant, k):
    """(1/2 f'H^-1 f, q) of problem k in longdouble"""
    p = K.problems(data, variant)
    H, f, A = p["H"][k], p["f"][k], p["A"][k]
    return float(R.half_f_hinv_f(H, f)), R.row_q(H, A, p["ms"])


def model(p, bound, recheck=None):
    import daqp_amd
    bm = daqp_amd.BatchModel(p["N"], p["n"], p["m"], p["ms"], p["ns_max"], fval_bound=float(bound))
    if recheck is not None:
        bm.set_recheck(recheck)
    return bm


def set_bound(bm, bound):
    import daqp_amd
    bm._settings.fval_bound = float(bound)
    daqp_amd.lib().daqp_batch_set_settings(bm._h, C.byref(bm._settings))


def same_verdicts(tag, g, ref):
    assert np.array_equal(g["exitflag"], ref["exitflag"]), (tag, g["exitflag"], ref["exitflag"])
    assert np.array_equal(g["iter"], ref["iter"]), (tag, g["iter"], ref["iter"])


def same_bits(tag, g, ref, rows, keys=NEG_KEYS):
    for key in keys:
        assert bits_equal(g[key][rows], ref[key][rows]), (tag, key)


def close_to(tag, g, ref, exact):
    """every problem of a batch against the oracle: bits in exact mode; default mode: fval to RELTOL, and x, lam to XTOL, LAMTOL where
    the solve ended at an optimum"""
    same_verdicts(tag, g, ref)
    if exact:
        same_bits(tag, g, ref, slice(None))
        ok = ref["exitflag"] > 0
        assert bits_equal(g["x"][ok], ref["x"][ok]), tag
        return
    for k in range(ref["fval"].size):
        assert rel(g["fval"][k], ref["fval"][k]) < RELTOL, (tag, k, g["fval"][k], ref["fval"][k])
        if ref["exitflag"][k] > 0:
            assert np.abs(g["x"][k] - ref["x"][k]).max() < XTOL and np.abs(g["lam"][k] - ref["lam"][k]).max() < LAMTOL, (tag, k)


def certify_stops(tag, data, variant, g, bound, stopped):
    """the four conditions of the module docstring on the stopped problems"""
    p = K.problems(data, variant)
    ub = F.unbounded(data, variant)
    for k in np.flatnonzero(stopped):
        half, q = problem_constants(data, variant, int(k))
        fval = float(g["fval"][k])
        assert fval + half > bound, (tag, k, fval + half, bound)
        assert fval <= ub["fval"][k] + RELTOL * max(1.0, abs(ub["fval"][k])), (tag, k, fval, ub["fval"][k])
        lv = ub["levels"][k]
        j = int(np.argmin(np.abs(0.5 * lv - (fval + half))))
        assert abs(0.5 * lv[j] - (fval + half)) < RELTOL * max(1.0, abs(0.5 * lv[j])), (tag, k, "stopped at no level of the oracle")
        assert j == 0 or lv[j - 1] <= 2.0 * bound, (tag, k, "late", j, lv[j - 1], 2.0 * bound)
        H, f, A, bu, bl, sense = K.problem(p, k)
        dual = float(R.dual_value(H, f, A, bu, bl, sense, p["ms"], np.array(g["lam"][k], dtype=R.LD) / np.sqrt(q), K.RHO_SOFT, q=q))
        assert rel(dual, fval) < FVAL_BAR, (tag, k, dual, fval)


def ws_equal(bm, ref, rows):
    na, ws = bm.working_sets()
    for k in rows:
        assert na[k] == ref["ws"][k].size and np.array_equal(ws[k, : na[k]], ref["ws"][k]), (k, ws[k, : na[k]], ref["ws"][k])


def cold(tag, name, variant, bound, exact, monkeypatch, certify=True):
    """one bound through BatchModel and solve_batch against the oracle; returns the oracle's BatchModel-route run.  certify=False: without
    the longdouble conditions (a bound one double from a level is nearer to it than fval + 1/2 f'H^-1 f can be recomputed)"""
    import daqp_amd
    fam, p = K.family(name), K.problems(name, variant)
    data = F.data_of(name)
    set_env(monkeypatch, fam["env"], exact)
    ref = oracle_run(data, variant, bound, 0)
    stopped = ref["exitflag"] == -1
    args = (p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"])
    bm = model(p, bound)
    g = {k: v.copy() for k, v in bm.setup(*args).solve().items()}
    assert bm.rechecked() == 0
    same_verdicts((tag, "BatchModel"), g, ref)
    print(tag, "stopped", int(stopped.sum()), "of", p["N"], "iter", g["iter"].min(), "..", g["iter"].max())
    close_to((tag, "BatchModel"), g, ref, exact)
    if certify:
        certify_stops((tag, "BatchModel"), data, variant, g, bound, stopped)
    if exact:
        ws_equal(bm, ref, range(p["N"]))
    bm.close()
    refq = oracle_run(data, variant, bound, 64 + 128)
    gq = daqp_amd.solve_batch(*args, ms=p["ms"], fval_bound=float(bound))
    close_to((tag, "solve_batch"), gq, refq, exact)
    if exact:
        return ref
    # the second pass on: every stopped problem is re-solved in the reference's arithmetic, under the same bound
    monkeypatch.delenv("DAQP_AMD_NO_RECHECK")
    bm = model(p, bound)
    g2 = bm.setup(*args).solve()
    assert bm.rechecked() == int(stopped.sum()), (tag, bm.rechecked(), int(stopped.sum()))
    same_verdicts((tag, "second pass"), g2, ref)
    same_bits((tag, "second pass"), g2, ref, stopped)
    ws_equal(bm, ref, np.flatnonzero(stopped))
    for key in ("x", "lam", "fval", "soft_slack"):
        assert bits_equal(g2[key][~stopped], g[key][~stopped]), (tag, "second pass touched a problem that was not stopped", key)
    certify_stops((tag, "second pass"), data, variant, g2, bound, stopped)
    bm.close()
    gq2 = daqp_amd.solve_batch(*args, ms=p["ms"], fval_bound=float(bound))
    same_verdicts((tag, "solve_batch, second pass"), gq2, refq)
    same_bits((tag, "solve_batch, second pass"), gq2, refq, refq["exitflag"] == -1)
    return ref


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("variant", F.VARIANTS)
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_fval_bound_cold(oracle, gpu_lib, monkeypatch, name, variant, kind, exact):
    """cold solves at the bounds early / mixed / all / none.  exact mode: flag, iter, and fval, lam, soft_slack, working sets bit for bit.
    default mode: once with DAQP_AMD_NO_RECHECK=1 (the kernel's own verdict and exit iterate, fval to RELTOL), once with the second
    pass: daqp_batch_rechecked equals the oracle's count of stopped problems, their outputs are bit-equal to the oracle's, the others
    are untouched.  none: equal to the solve without a bound (bit for bit in exact mode, 1e-12 otherwise)."""
    from test_gpu_kkt import same_outputs
    bound = F.bound(name, variant, kind)
    ref = cold((name, variant, kind), name, variant, bound, exact, monkeypatch)
    if kind == "none":
        assert (ref["exitflag"] > 0).all()
        p = K.problems(name, variant)
        set_env(monkeypatch, K.family(name)["env"], exact)
        args = (p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"])
        b0, b1 = model(p, F.DAQP_INF), model(p, bound)
        same_outputs(b1.setup(*args).solve(), b0.setup(*args).solve(), exact)
        b0.close(); b1.close()


@pytest.mark.parametrize("variant", F.VARIANTS)
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_fval_bound_exact_tight(oracle, gpu_lib, monkeypatch, name, variant):
    """exact mode: fval_bound = l / 2 for a level l of one problem -- the comparison is >, it passes that iterate -- and the double
    just below, where it stops there; the other problems of the batch do what the oracle does"""
    k, j, at, below = F.bound(name, variant, "tight")
    data = F.data_of(name)
    cold((name, variant, "at"), name, variant, at, True, monkeypatch, certify=False)
    cold((name, variant, "below"), name, variant, below, True, monkeypatch, certify=False)
    r_at, r_below = oracle_run(data, variant, at, 0), oracle_run(data, variant, below, 0)
    assert r_below["exitflag"][k] == -1 and r_at["iter"][k] > r_below["iter"][k]      # (what the two GPU runs were just held to)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("variant", F.VARIANTS)
@pytest.mark.parametrize("name", K.WARM_FAMILIES)
def test_fval_bound_warm_and_continue(oracle, gpu_lib, monkeypatch, name, variant, exact):
    """solve under `mixed`; fval_bound back to DAQP_INF (daqp_batch_set_settings) and solve again: the stopped problems continue from
    the kept working set, as in the reference; then a new f under a finite bound on the warm solve, where no second pass runs and the
    default mode's verdicts stand on their own.  In the default mode the sequence runs with the second pass off and on (on: the
    continued solve starts from the exact run's iterate)."""
    fam, p = K.family(name), K.problems(name, variant)
    outs, b3, f2 = F.warm_reference(name, variant)
    for recheck in ((None,) if exact else (False, True)):
        set_env(monkeypatch, fam["env"], exact)
        if recheck:
            monkeypatch.delenv("DAQP_AMD_NO_RECHECK")
        bm = model(p, F.bound(name, variant, "mixed"))
        bm.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"])
        g = bm.solve()
        close_to((name, variant, recheck, "cold"), g, outs[0], exact)
        assert bm.rechecked() == (int((outs[0]["exitflag"] == -1).sum()) if recheck else 0)
        set_bound(bm, F.DAQP_INF)
        g = bm.solve()
        assert (outs[1]["exitflag"] > 0).all() and bm.rechecked() == 0
        close_to((name, variant, recheck, "continued"), g, outs[1], exact)
        set_bound(bm, b3)
        bm.update(f=f2)
        g = bm.solve()
        assert bm.rechecked() == 0
        close_to((name, variant, recheck, "warm step"), g, outs[2], exact)
        if exact:
            ws_equal(bm, outs[2], range(p["N"]))
        bm.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("name", K.SHARED_FAMILIES)
def test_fval_bound_shared(oracle, gpu_lib, monkeypatch, name, exact):
    """setup_shared under a bound that stops part of the batch: the second pass does not run after a shared setup (one H and A, nothing
    per problem to gather), with the environment allowing it -- the kernels' own verdicts are held to the oracle"""
    import daqp_amd
    c = F.shared_reference(name)
    set_env(monkeypatch, K.family(name)["env"], exact)
    monkeypatch.delenv("DAQP_AMD_NO_RECHECK", raising=False)
    bm = daqp_amd.BatchModel(c["N"], c["n"], c["m"], c["ms"], fval_bound=float(c["bound"]))
    bm.setup_shared(c["H"], c["f"], c["A"], c["bupper"], c["blower"], None)
    g = bm.solve()
    assert bm.rechecked() == 0
    close_to((name, "shared"), g, c["ref"], exact)
    if exact:
        ws_equal(bm, c["ref"], range(c["N"]))
    bm.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("name,variant", K.SINGLE_CASES)
def test_fval_bound_single_problem(oracle, gpu_lib, monkeypatch, name, variant, exact):
    """daqp_quadprog and setup_daqp / daqp_solve on one problem under a bound that stops it inside its run (N == 1: the second pass is
    the same workspace again in the exact mode); then the bound raised and a second daqp_solve, which continues"""
    import daqp_amd
    fam, p = K.family(name), K.problems(name, variant)
    set_env(monkeypatch, fam["env"], exact)
    monkeypatch.delenv("DAQP_AMD_NO_RECHECK", raising=False)
    n, m, ms = p["n"], p["m"], p["ms"]
    H, f, A, bu, bl, sense = K.problem(p, 1)
    s = np.zeros(m, np.int32) if sense is None else sense
    b = F.single_bound(name, variant)

    def held(tag, got, ref):
        x, fval, flag, info = got
        assert (flag, info["iterations"]) == (ref[3], ref[4]), (tag, flag, info["iterations"], ref[3], ref[4])
        assert (fval == ref[2]) if exact else (rel(fval, ref[2]) < RELTOL), (tag, fval, ref[2])
        if ref[3] > 0:
            assert np.abs(x - ref[0]).max() < XTOL, tag

    om = oracle.model(n, m, ms, ns=p["ns_max"], settings=F.settings(b))
    assert om.setup(H, f, A, bu, bl, sense, init_mask=64 + 128) >= 0
    ref = om.solve()
    assert ref[3] == -1
    held((name, variant, "solve"), daqp_amd.solve(H, f, A, bu, bl, s, fval_bound=float(b)), ref)
    mdl = daqp_amd.Model()
    assert mdl.setup(H, f, A, bu, bl, s, fval_bound=float(b))[0] >= 0
    om = oracle.model(n, m, ms, ns=p["ns_max"], settings=F.settings(b))
    assert om.setup(H, f, A, bu, bl, sense) >= 0
    ref = om.solve()
    assert ref[3] == -1
    held((name, variant, "Model"), mdl.solve(), ref)
    mdl.settings(fval_bound=F.DAQP_INF)
    om.settings(fval_bound=F.DAQP_INF)
    ref = om.solve()
    assert ref[3] > 0
    held((name, variant, "Model, bound raised"), mdl.solve(), ref)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("name", [f["name"] for f in K.PROX_FAMILIES])
def test_fval_bound_prox(oracle, gpu_lib, monkeypatch, name, exact):
    """singular Hessians and LPs: the bound acts inside the proximal loop's inner solves, which run the reference's arithmetic in both
    modes -- flag and total iterations of every problem equal the oracle's, and x, lam, fval bit for bit where the loop ended at an optimum"""
    import daqp_amd
    p = K.prox_problems(name)
    b = F.prox_bound(name)
    set_env(monkeypatch, {}, exact)
    monkeypatch.delenv("DAQP_AMD_NO_RECHECK", raising=False)
    g = daqp_amd.solve_batch(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms=p["ms"], fval_bound=float(b))
    ref = F.prox_run(p, b)
    assert 0 < (ref["exitflag"] == -1).sum() < p["N"]
    same_verdicts((name,), g, ref)
    same_bits((name,), g, ref, ref["exitflag"] > 0, keys=("x", "lam", "fval"))


def test_golden_fval_bound(gpu_lib, monkeypatch):
    """the reference's own outputs under a bound (tests/golden/golden_fval_bound.npz) replayed in exact mode: flag and iter of every case;
    x, lam, fval bit for bit at an optimum; lam and fval bit for bit at the bound exit of a definite QP; then the warm sequence"""
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "1")
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_fval_bound.npz"), allow_pickle=False)
    seen = {}
    for nm in sorted({k.split("/")[0] for k in g.files} - {"warm"}):
        get = lambda key: g[f"{nm}/{key}"]
        H = get("H") if get("H").size else None
        x, fval, flag, info = daqp_amd.solve(H, get("f"), get("A"), get("bupper"), get("blower"), get("sense"), fval_bound=float(get("fval_bound")))
        assert flag == int(get("exitflag")) and info["iterations"] == int(get("iter")), (nm, flag, info["iterations"], int(get("exitflag")), int(get("iter")))
        seen[flag] = seen.get(flag, 0) + 1
        if flag > 0:
            assert bits_equal(x, get("x")) and bits_equal(info["lam"], get("lam")) and fval == float(get("fval")), nm
        elif not nm.startswith(("lp", "singular")):
            assert bits_equal(info["lam"], get("lam")) and fval == float(get("fval")), nm
    assert seen.get(-1, 0) >= 20 and seen.get(1, 0) + seen.get(2, 0) >= 5, seen
    w = lambda key: g[f"warm/{key}"]
    mdl = daqp_amd.Model()
    assert mdl.setup(w("H"), w("f"), w("A"), w("bupper"), w("blower"), None, fval_bound=float(w("bounds")[0]))[0] >= 0
    for t in range(3):
        if t:
            mdl.settings(fval_bound=float(w("bounds")[t]))
        if t == 2:
            assert mdl.update(f=w("f2")) == 0
        x, fval, flag, info = mdl.solve()
        assert flag == int(w("exitflag")[t]) and info["iterations"] == int(w("iter")[t]), (t, flag, info["iterations"])
        assert bits_equal(info["lam"], w("lam")[t]) and fval == float(w("fval")[t]), t
        if flag > 0:
            assert bits_equal(x, w("x")[t]), t
