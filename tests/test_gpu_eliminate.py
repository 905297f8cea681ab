"""Equality elimination on the device (daqp_batch_eliminate / _update / _expand, daqp_amd.EliminatedBatchModel) against the numpy
reference of tests/eliminate_cases.py and against the unreduced BatchModel on the same data."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import eliminate_cases as EC

pytestmark = pytest.mark.gpu

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_eliminated.npz")
# batch sizes 3, 64 and 257, the largest on the smallest problems
N_OF = {(6, 2, 10, 2): 257, (64, 1, 70, 0): 64, (64, 63, 70, 4): 257, (65, 1, 70, 0): 64, (70, 40, 90, 5): 64, (130, 70, 150, 0): 3,
        EC.LP_SHAPE: 64}
IDS = [str(s) for s in EC.SHAPES]
KEYS = ("H", "f", "A", "bupper", "blower", "sense")


@functools.lru_cache(maxsize=None)
def batch(i, lp=False, soft=0):
    shape = EC.LP_SHAPE if lp else EC.SHAPES[i]
    b = EC.make_batch(shape, N_OF[shape], 500 + i, lp=lp, bound_row=(i == 0 and not lp), soft=soft)
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


def eliminated(b, ns=0, **kw):
    import daqp_amd
    n, neq, m, ms = b["shape"]
    em = daqp_amd.EliminatedBatchModel(b["f"].shape[0], n, m, ms, b["eq_rows"], ns_max=ns)
    em.setup(*[b[k] for k in KEYS], **kw)
    return em


@functools.lru_cache(maxsize=None)
def unreduced(i, lp=False, soft=0):
    """(result, certificate) of the unreduced batch"""
    import daqp_amd
    b = batch(i, lp, soft)
    n, neq, m, ms = b["shape"]
    bm = daqp_amd.BatchModel(b["f"].shape[0], n, m, ms, soft)
    bm.setup(*[b[k] for k in KEYS])
    r = bm.solve()
    bm.close()
    return r, daqp_amd.certify_batch(b["H"], b["f"], b["A"], b["bupper"], b["blower"], r["x"], r["lam"], b["sense"], ms=ms)


def agree(r, ref, kept, cert=None, cert_ref=None):
    assert np.array_equal(r["exitflag"], ref["exitflag"])
    ok = ref["exitflag"] > 0
    assert ok.all()
    ex = np.abs(r["x"] - ref["x"]).max(axis=1) / np.maximum(1.0, np.abs(ref["x"]).max(axis=1))
    el = np.abs(r["lam"] - ref["lam"]).max(axis=1) / np.maximum(1.0, np.abs(ref["lam"]).max(axis=1))
    ef = np.abs(r["fval"] - ref["fval"]) / np.maximum(1.0, np.abs(ref["fval"]))
    print("x %.2e lam %.2e fval %.2e" % (ex.max(), el.max(), ef.max()))
    assert ex.max() <= 1e-9 and el.max() <= 1e-7 and ef.max() <= 1e-9
    assert np.array_equal(np.sign(r["lam"][:, kept]), np.sign(ref["lam"][:, kept]))
    if cert is not None:
        for key, a, bb in (("stationarity", cert["stationarity"] / cert["stationarity_scale"], cert_ref["stationarity"] / cert_ref["stationarity_scale"]),
                           ("primal", cert["primal"], cert_ref["primal"]), ("complementarity", cert["complementarity"], cert_ref["complementarity"])):
            print(key, "%.2e vs %.2e" % (a.max(), bb.max()))
            assert (a <= np.maximum(8.0 * bb, 1e-12)).all(), key


# ---- 1: the algebra against the device's own basis ---------------------------------------------------------------------------------
def defects(p, ms, eq, x0, Z, c0, red):
    """the eight defects of one problem's elimination, in longdouble, each relative to its natural scale"""
    n, m = p["f"].size, p["bupper"].size
    kept = EC.kept_rows(m, eq)
    Cm = EC.cmat(p["A"], ms, n).astype(LD)
    E = Cm[eq]
    nrm = np.sqrt((E * E).sum(axis=1))
    x0, Z = np.asarray(x0, dtype=np.float64).astype(LD), np.asarray(Z, dtype=np.float64).astype(LD)
    H, f = p["H"].astype(LD), p["f"].astype(LD)
    e = p["bupper"][eq].astype(LD)
    g = H @ x0 + f
    CI = Cm[kept]
    amax = lambda a: float(np.abs(a).max()) if np.size(a) else 0.0
    d = {"Z'Z-I": amax(Z.T @ Z - np.eye(Z.shape[1], dtype=LD)),
         "EZ": amax((E / nrm[:, None]) @ Z),
         "Ex0-e": amax((E @ x0 - e) / nrm) / max(1.0, amax(e / nrm)),
         "Z'x0": amax(Z.T @ x0) / max(1.0, amax(x0)),
         "Hr": amax(np.asarray(red["H"], dtype=np.float64).astype(LD) - Z.T @ H @ Z) / amax(H),
         "fr": amax(np.asarray(red["f"], dtype=np.float64).astype(LD) - Z.T @ g) / max(1.0, amax(g)),
         "Ar": amax(np.asarray(red["A"], dtype=np.float64).astype(LD) - CI @ Z) / max(1.0, amax(CI)),
         "c0": abs(float(LD(c0) - (LD(0.5) * (x0 @ (H @ x0)) + f @ x0))) / max(1.0, amax(H) * amax(x0) ** 2)}
    shift = CI @ x0
    for name, b in (("bupper", p["bupper"][kept]), ("blower", p["blower"][kept])):
        fin = np.abs(b) < EC.INF
        br = np.asarray(red[name], dtype=np.float64)
        assert np.array_equal(br[~fin], b[~fin])      # open bounds stay as they are
        d[name] = amax(br[fin].astype(LD) - (b[fin].astype(LD) - shift[fin])) / max(1.0, amax(b[fin]))
    return d


@pytest.mark.parametrize("i", range(len(EC.SHAPES)), ids=IDS)
def test_algebra_against_the_devices_own_basis(i):
    """Largest ratio device defect / max(fp64 numpy defect, n 2^-52 / 8) over the ten defects, per shape, measured on an MI355X (the
    bar is 8): (6, 2, 10, 2) 1.55, (64, 1, 70, 0) 1.80, (64, 63, 70, 4) 1.59, (65, 1, 70, 0) 1.50, (70, 40, 90, 5) 0.49,
    (130, 70, 150, 0) 0.37."""
    b = batch(i)
    n, neq, m, ms = b["shape"]
    N = b["f"].shape[0]
    em = eliminated(b)
    assert (em.flags == 1).all()
    bas, red = em.basis(), em.reduced_problem()
    em.close()
    assert np.array_equal(red["H"], red["H"].transpose(0, 2, 1))      # exactly symmetric
    assert np.array_equal(red["sense"], b["sense"][:, EC.kept_rows(m, b["eq_rows"])])
    floor = n * 2.0 ** -52
    worst = {}
    for k in sorted(set(range(0, N, max(1, N // 8))) | {N - 1}):
        p = {key: b[key][k] for key in KEYS}
        dev = defects(p, ms, b["eq_rows"], bas["x0"][k], bas["Z"][k], bas["c0"][k], {key: red[key][k] for key in ("H", "f", "A", "bupper", "blower")})
        ref = EC.eliminate(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms, b["eq_rows"], dtype=np.float64)
        refd = defects(p, ms, b["eq_rows"], ref["x0"], ref["Z"], ref["c0"], ref)
        for key in dev:
            worst[key] = max(worst.get(key, 0.0), dev[key] / max(refd[key], floor / 8.0))
            assert dev[key] <= max(8.0 * refd[key], floor), (k, key, dev[key], refd[key])
    print(b["shape"], "N", N, "worst ratio device / max(reference, floor / 8):", {k: round(v, 3) for k, v in worst.items()})


# ---- 2: end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(EC.SHAPES)), ids=IDS)
def test_solve_agrees_with_the_unreduced_batch(i):
    b = batch(i)
    ref, cert_ref = unreduced(i)
    em = eliminated(b)
    r = em.solve()
    cert = em.certify(r)
    em.close()
    assert set(r) == set(ref) and all(r[k].shape == ref[k].shape and r[k].dtype == ref[k].dtype for k in ref)
    agree(r, ref, EC.kept_rows(b["shape"][2], b["eq_rows"]), cert, cert_ref)


def test_lp_batch():
    b = batch(0, lp=True)
    ref, cert_ref = unreduced(0, lp=True)
    em = eliminated(b)
    assert em.reduced_problem()["H"] is None
    r = em.solve()
    cert = em.certify(r)
    em.close()
    agree(r, ref, EC.kept_rows(b["shape"][2], b["eq_rows"]), cert, cert_ref)


def test_soft_kept_rows():
    b = batch(4, soft=2)
    ref, cert_ref = unreduced(4, soft=2)
    em = eliminated(b, ns=2)
    assert ((em.reduced_problem()["sense"] & 8) != 0).sum(axis=1).max() == 2
    r = em.solve()
    em.close()
    agree(r, ref, EC.kept_rows(b["shape"][2], b["eq_rows"]))
    assert np.abs(r["soft_slack"] - ref["soft_slack"]).max() <= 1e-9 * max(1.0, np.abs(ref["soft_slack"]).max())


def test_active_soft_row_against_the_oracle_on_the_reduced_problem():
    """An ACTIVE soft row is weighted by the reduced Hessian (include/daqp_amd.h), so the comparison point is not the unreduced batch but
    an independent solve of the same reduced problem: the numpy elimination, the oracle on its output, the numpy expansion."""
    from oracle import oracle as O
    ora = O.Oracle()
    shape = EC.SHAPES[4]
    n, neq, m, ms = shape
    N = 16
    b = EC.make_batch(shape, N, 777, soft=2, soft_active=True)
    em = eliminated(b, ns=2)
    r = em.solve()
    em.close()
    for k in range(N):
        p = {key: b[key][k] for key in KEYS}
        el = EC.eliminate(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms, b["eq_rows"])
        om = ora.model(n - neq, m - neq, 0, 2)
        assert om.setup(*[np.ascontiguousarray(el[key], dtype=np.float64) for key in ("H", "f", "A", "bupper", "blower")], el["sense"]) >= 0
        y, lam_r, fval_r, flag, _, slack = om.solve(with_soft=True)
        x, lam, fval = EC.expand(el, y, lam_r, fval_r)
        soft_rows = np.flatnonzero((el["sense"] & 8) != 0)
        assert r["exitflag"][k] == flag > 0 and slack > 0 and np.abs(lam_r[soft_rows]).max() >= 0.1, (k, r["exitflag"][k], flag, slack)
        ex = np.abs(r["x"][k] - x).max() / max(1.0, np.abs(x).max())
        elam = np.abs(r["lam"][k] - lam).max() / max(1.0, np.abs(lam).max())
        es = abs(r["soft_slack"][k] - slack) / abs(slack)      # slack = rho_soft sum q_k lam_k^2 is ~1e-8 here: relative to itself
        ef = abs(r["fval"][k] - fval) / max(1.0, abs(fval))
        if k == 0:
            print("soft_slack %.3e: x %.2e lam %.2e slack %.2e fval %.2e" % (slack, ex, elam, es, ef))
        # (soft_slack is quadratic in lam, which is held to 1e-7: 2e-7 from lam, the rest of 1e-6 for q_k of the two reduced problems)
        assert ex <= 1e-9 and elam <= 1e-7 and es <= 1e-6 and ef <= 1e-9, (k, ex, elam, es, ef)
        assert np.array_equal(np.sign(r["lam"][k][el["kept"]]), np.sign(lam[el["kept"]]))


def test_golden_eliminated_problems_replay():
    import daqp_amd
    for p in EC.golden_problems(GOLDEN):
        n, m = p["f"].size, p["bupper"].size
        em = daqp_amd.EliminatedBatchModel(1, n, m, p["ms"], p["eq_rows"])
        em.setup(*[p[k][None] for k in KEYS])
        r = em.solve()
        em.close()
        kept = EC.kept_rows(m, p["eq_rows"])
        assert r["exitflag"][0] == int(p["exitflag"]) == 1, p["name"]
        assert np.abs(r["x"][0] - p["x"]).max() <= 1e-9, (p["name"], np.abs(r["x"][0] - p["x"]).max())
        assert np.abs(r["lam"][0] - p["lam"]).max() <= 1e-7 * max(1.0, np.abs(p["lam"]).max()), p["name"]
        act = lambda l: np.sign(np.where(np.abs(l) >= 1e-8, l, 0.0))[kept]
        assert np.array_equal(act(r["lam"][0]), act(p["lam"])), p["name"]
        assert abs(r["fval"][0] - float(p["fval"])) <= 1e-9 * max(1.0, abs(float(p["fval"]))), p["name"]


# ---- 3: the warm path -----------------------------------------------------------------------------------------------------------
def moved(b, step):
    """f and the bounds of step `step` of a walk: f drifts, every bound moves with the equality right-hand sides staying equalities"""
    rng = np.random.default_rng(900 + step)
    f = b["f"] + 0.02 * step * rng.standard_normal(b["f"].shape)
    d = 0.01 * step * rng.standard_normal(b["bupper"].shape)
    shift = lambda a: np.where(np.abs(a) >= EC.INF, a, a + d)
    return f, shift(b["bupper"]), shift(b["blower"])


@pytest.mark.parametrize("i", [0, 4], ids=[IDS[0], IDS[4]])
def test_update_is_bit_identical_to_a_fresh_setup(i):
    b = batch(i)
    f, bu, bl = moved(b, 1)
    em = eliminated(b)
    em.update(f=f, bupper=bu, blower=bl)
    got, gb = em.reduced_problem(), em.basis()
    em.close()
    fresh = eliminated(dict(b, f=f, bupper=bu, blower=bl))
    want, wb = fresh.reduced_problem(), fresh.basis()
    fresh.close()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    for k in wb:
        assert np.array_equal(gb[k], wb[k]), k
    with pytest.raises(ValueError, match="setup"):
        em.update(H=b["H"])


def test_three_step_walk_keeps_the_working_sets():
    """f drifts by 1e-3 per step, far inside the planted margins (multipliers and slacks of at least 0.1): the working set of step 0
    stays optimal, so the warm solve only has to confirm it while a cold solve has to find it"""
    import daqp_amd
    b = batch(4)
    n, neq, m, ms = b["shape"]
    kept = EC.kept_rows(m, b["eq_rows"])
    em = eliminated(b)
    bm = daqp_amd.BatchModel(b["f"].shape[0], n, m, ms)
    bm.setup(*[b[k] for k in KEYS])
    em.solve(), bm.solve()
    for step in (1, 2, 3):
        f = b["f"] + 1e-3 * step * np.random.default_rng(950 + step).standard_normal(b["f"].shape)
        em.update(f=f)
        bm.update(f=f)
        r, ref = em.solve(), bm.solve()
        agree(r, ref, kept)
        if step == 2:
            cold = eliminated(dict(b, f=f))
            rc = cold.solve()
            cold.close()
            assert (r["iter"] <= rc["iter"]).all(), (r["iter"], rc["iter"])
    em.close(), bm.close()


# ---- 4: flags and isolation -----------------------------------------------------------------------------------------------------
def test_flags_and_isolation():
    b = batch(4)
    n, neq, m, ms = b["shape"]
    eq = b["eq_rows"]
    bad = {k: b[k].copy() for k in KEYS}
    bad["A"][17, eq[3] - ms] = bad["A"][17, eq[1] - ms]      # a duplicated equality row
    bad["bupper"][17, eq[3]] = bad["blower"][17, eq[3]] = bad["bupper"][17, eq[1]]
    bad["bupper"][40, eq[5]] += 0.5                           # no equality
    em = eliminated(dict(b, **bad))
    want = np.ones(64, np.int32)
    want[17], want[40] = -6, -8
    assert np.array_equal(em.flags, want)
    r = em.solve()
    em.close()
    assert r["exitflag"][17] == -6 and r["exitflag"][40] == -8
    for q in (17, 40):
        assert not r["x"][q].any() and not r["lam"][q].any()
    good = eliminated(b)
    rg = good.solve()
    good.close()
    others = np.setdiff1d(np.arange(64), [17, 40])
    for k in rg:
        assert np.array_equal(r[k][others], rg[k][others]), k


def test_flags_and_isolation_in_an_lp_batch():
    """an LP batch has no H_r: a problem with dependent equality rows is flagged and zeroed without touching its neighbours"""
    b = batch(0, lp=True)
    n, neq, m, ms = b["shape"]
    eq = b["eq_rows"]
    bad = {k: (None if b[k] is None else b[k].copy()) for k in KEYS}
    bad["A"][17, eq[2] - ms] = bad["A"][17, eq[0] - ms]      # a duplicated equality row
    bad["bupper"][17, eq[2]] = bad["blower"][17, eq[2]] = bad["bupper"][17, eq[0]]
    em = eliminated(dict(b, **bad))
    want = np.ones(64, np.int32)
    want[17] = -6
    assert np.array_equal(em.flags, want)
    red = em.reduced_problem()
    assert red["H"] is None and not any(red[k][17].any() for k in ("f", "A", "bupper", "blower", "sense"))
    r = em.solve()
    em.close()
    assert r["exitflag"][17] == -6 and not r["x"][17].any() and not r["lam"][17].any()
    good = eliminated(b)
    redg, rg = good.reduced_problem(), good.solve()
    good.close()
    others = np.setdiff1d(np.arange(64), [17])
    for k in ("f", "A", "bupper", "blower", "sense"):
        assert np.array_equal(red[k][others], redg[k][others]), k
    for k in rg:
        assert np.array_equal(r[k][others], rg[k][others]), k


def test_argument_errors_leave_no_handle():
    import daqp_amd
    from daqp_amd import _lib
    L = daqp_amd.lib()
    b = batch(0)
    n, neq, m, ms = b["shape"]
    N = b["f"].shape[0]
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_lib.c_int_p)
    prob = lambda n_=n, **kw: _lib.DAQPBatchProblem(N, n_, m, ms, *[(kw[k] if k in kw else b[k].ctypes.data) for k in KEYS], kw.get("memory", _lib.MEM_HOST))

    def refused(p, rows, k, word):
        h = C.c_void_p(1)
        assert L.daqp_batch_eliminate(C.byref(h), C.byref(p), None if rows is None else ip(rows), k, None, -1, None) != 0
        assert word in _lib.last_error(), _lib.last_error()
        assert not h.value

    refused(prob(), [0], 0, "neq")
    refused(prob(), list(range(n)), n, "neq")
    refused(prob(), [0, m], 2, "out of range")
    refused(prob(), [3, 2], 2, "ascending")
    refused(prob(), [2, 2], 2, "ascending")
    refused(prob(n_=512), [0, 2], 2, "511")
    refused(prob(), None, 2, "null")
    refused(prob(f=None), [0, 2], 2, "null")
    refused(prob(memory=7), [0, 2], 2, "memory")
    em = eliminated(b)
    r = em.reduced.solve()
    full = {k: np.empty_like(v, shape=(N, n) if k == "x" else ((N, m) if k == "lam" else v.shape)) for k, v in r.items()}
    keys = ("x", "lam", "fval", "soft_slack", "exitflag", "iter")
    rr = _lib.DAQPBatchResult(*[r[k].ctypes.data for k in keys], _lib.MEM_HOST, 0, 0)
    fr = _lib.DAQPBatchResult(*[full[k].ctypes.data for k in keys], _lib.MEM_DEVICE, 0, 0)
    assert L.daqp_batch_expand(em._el, C.byref(rr), C.byref(fr)) != 0 and "mixed" in _lib.last_error()
    assert L.daqp_batch_expand(em._el, None, C.byref(fr)) != 0 and "null" in _lib.last_error()
    assert L.daqp_batch_eliminate_update(None, None, None, None, _lib.MEM_HOST) != 0 and "null" in _lib.last_error()
    assert L.daqp_batch_elimination_bytes(em._el) > 0
    em.close()
    with pytest.raises(ValueError, match="mix"):
        import torch
        eliminated(dict(b, f=torch.as_tensor(b["f"].copy(), device="cuda")))


# ---- 5: solve_batch ---------------------------------------------------------------------------------------------------------------
def test_solve_batch_without_eq_rows_is_what_it_was():
    import daqp_amd
    b = batch(0)
    n, neq, m, ms = b["shape"]
    a = daqp_amd.solve_batch(*[b[k] for k in KEYS], ms=ms)
    c = daqp_amd.solve_batch(*[b[k] for k in KEYS], ms=ms, eq_rows=None)
    bm = daqp_amd.BatchModel(b["f"].shape[0], n, m, ms)
    bm.setup(*[b[k] for k in KEYS], init_mask=daqp_amd.UPDATE_unconstrained | daqp_amd.UPDATE_eliminate)
    d = bm.solve()
    bm.close()
    for k in d:
        assert np.array_equal(a[k], c[k]) and np.array_equal(a[k], d[k]), k
    e = daqp_amd.solve_batch(*[b[k] for k in KEYS], ms=ms, eq_rows=list(b["eq_rows"]))
    agree(e, d, EC.kept_rows(m, b["eq_rows"]))
