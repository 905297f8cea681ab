"""What leaves the solve kernels' epilogues -- x, lam, fval, soft_slack, exitflag -- held to a property of the QP itself: the
extended-precision KKT certificate of tests/kkt_reference.py (no solver code), on every kernel family of tests/kkt_cases.py, in both
arithmetic modes and through every entry route (BatchModel, solve_batch, setup_shared, warm updates, reset, the single-problem calls,
the proximal loop), next to direct comparisons of lam, fval and soft_slack with the oracle.  Bars: kkt_cases.BARS (100 x what the oracle's
own solutions leave, tests/test_cpu_kkt_reference.py); oracle comparisons in the default mode at test_fast_mode_parity's bars."""
import numpy as np
import pytest

import kkt_cases as K
import kkt_reference as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu
XTOL, LAMTOL, RELTOL, GTOL = 1e-9, 1e-8, 1e-8, 1e-7
ENV_KEYS = sorted({k for f in K.FAMILIES for k in f["env"]})
FAMILY_NAMES = [f["name"] for f in K.FAMILIES]


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def rel(a, ref):
    return abs(a - ref) / max(1.0, abs(ref))


def set_env(monkeypatch, env, exact):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DAQP_AMD_EXACT", "1" if exact else "0")
    if exact:
        monkeypatch.delenv("DAQP_AMD_NO_RECHECK", raising=False)
    else:      # the default-mode kernels' own verdicts, as in the sibling files
        monkeypatch.setenv("DAQP_AMD_NO_RECHECK", "1")


def check_one(tag, prob, ms, g, ref, exact, degenerate=False, group="qp", q=None):
    """one problem: prob = (H, f, A, bupper, blower, sense); g, ref = (x, lam, fval, flag, iter, soft_slack) of the GPU and of the oracle"""
    H, f, A, bu, bl, sense = prob
    x, lam, fval, flag, it, ss = g
    xr, lamr, fvalr, flagr, itr, ssr = ref
    assert flag == flagr and it == itr, (tag, flag, flagr, it, itr)
    if exact:
        assert fval == fvalr, (tag, fval, fvalr)
    else:
        assert rel(fval, fvalr) < RELTOL, (tag, fval, fvalr)
    if flag not in (1, 2):      # (no problem of the present families ends here: the oracle gives 1 or 2 everywhere -- kept for draws that do)
        return
    bars = K.BARS[group]
    c = R.certificate(H, f, A, bu, bl, sense, ms, x, lam, K.RHO_SOFT, normalised=(group == "qp"), q=q)
    figures = {k: c[k] for k in bars if k in c}
    figures.update(fval=rel(fval, c["fval_ref"]))
    if group == "qp":
        figures.update(soft_slack=rel(ss, c["soft_slack_ref"]))
    print(tag, " ".join(f"{k}={v:.1e}" for k, v in figures.items()))
    for k, v in figures.items():
        assert v < bars[k][1], (tag, k, v, bars[k][1])
    assert c["wrong_sign"] == 0 and c["nonzero_inactive"] == 0, (tag, c["wrong_sign"], c["nonzero_inactive"])
    if group != "qp":
        return
    if exact:
        assert bits_equal(x, xr) and bits_equal(lam, lamr) and ss == ssr, (tag, np.abs(lam - lamr).max(), ss, ssr)
        return
    assert np.abs(x - xr).max() < XTOL, (tag, np.abs(x - xr).max())
    if degenerate:     # a near-duplicate pair may share its multiplier differently in two arithmetics: compare its effect
        G = R.constraint_matrix(A, ms, f.size).astype(np.float64)
        assert np.abs(G.T @ (lam - lamr)).max() < GTOL, (tag, np.abs(G.T @ (lam - lamr)).max())
    else:
        assert np.array_equal(np.sign(lam), np.sign(lamr)), tag
        assert np.abs(lam - lamr).max() < LAMTOL, (tag, np.abs(lam - lamr).max())
    assert rel(ss, ssr) < RELTOL, (tag, ss, ssr)


def check_batch(tag, p, g, ref, exact, group="qp", data=None, q=None):
    """a batch: p = the family's dict (data: per-problem (f, bupper, blower) overrides), g / ref = dicts of stacked outputs"""
    for k in range(p["N"]):
        prob = list(K.problem(p, k))
        if data is not None:
            prob[1], prob[3], prob[4] = data["f"][k], data["bupper"][k], data["blower"][k]
        check_one((tag, k), prob, p["ms"], tuple(g[key][k] for key in ("x", "lam", "fval", "exitflag", "iter", "soft_slack")),
                  tuple(ref[key][k] for key in ("x", "lam", "fval", "exitflag", "iter", "soft_slack")), exact,
                  degenerate=p["degenerate"], group=group, q=None if q is None else q[k])


def same_outputs(g1, g0, exact):
    """two solves of one batch that must agree: bit for bit in exact mode, to 1e-12 otherwise"""
    assert np.array_equal(g1["exitflag"], g0["exitflag"]) and np.array_equal(g1["iter"], g0["iter"]), (g1["iter"], g0["iter"])
    for key in ("x", "lam", "fval", "soft_slack"):
        if exact:
            assert bits_equal(g1[key], g0[key]), key
        else:
            assert np.abs(g1[key] - g0[key]).max() <= 1e-12 * max(1.0, np.abs(g0[key]).max()), (key, np.abs(g1[key] - g0[key]).max())


def batch_model(p):
    import daqp_amd
    return daqp_amd.BatchModel(p["N"], p["n"], p["m"], p["ms"], p["ns_max"])


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("variant", K.VARIANTS)
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_kkt_cold(oracle, gpu_lib, monkeypatch, name, variant, exact):
    """setup + solve through BatchModel and through solve_batch (the unconstrained shortcut forms d its own way): certificate under
    the bars, fval and soft_slack equal to what the certificate derives from (x, lam), and lam / fval / soft_slack against the oracle --
    bit for bit in exact mode"""
    import daqp_amd
    fam, p = K.family(name), K.problems(name, variant)
    set_env(monkeypatch, fam["env"], exact)
    q = [R.row_q(p["H"][k], p["A"][k], p["ms"]) for k in range(p["N"])]
    bm = batch_model(p)
    bm.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"])
    g = bm.solve()
    bm.close()
    check_batch((name, variant, "BatchModel"), p, g, K.oracle_solve(K.oracle_models(oracle, p, 0)), exact, q=q)
    g = daqp_amd.solve_batch(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms=p["ms"])
    check_batch((name, variant, "solve_batch"), p, g, K.oracle_solve(K.oracle_models(oracle, p, 64 + 128)), exact, q=q)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("variant", ["plain", "sense"])
@pytest.mark.parametrize("name", K.WARM_FAMILIES)
def test_kkt_warm(oracle, gpu_lib, monkeypatch, name, variant, exact):
    """reset() after the cold solve gives the cold solve again; then update(f), update(bounds), update(f) with an OracleModel kept
    alongside: the certificate on the updated data after every step.  reset == cold solve is checked on the plain variant and on soft rows
    without equalities; with equalities only that two resets give the same solve: the reference's
    daqp_deactivate_constraints leaves IMMUTABLE rows marked ACTIVE but reset_daqp_workspace empties the working set, and nothing short
    of a sense update puts an equality back (auxiliary.c:98-101 never adds an ACTIVE or IMMUTABLE row) -- with equalities a solve after a
    reset is not the cold solve, in the reference either."""
    fam, p = K.family(name), K.problems(name, variant)
    set_env(monkeypatch, fam["env"], exact)
    N, n, m = p["N"], p["n"], p["m"]
    q = [R.row_q(p["H"][k], p["A"][k], p["ms"]) for k in range(N)]
    models = K.oracle_models(oracle, p, 0)
    bm = batch_model(p)
    bm.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"])
    g0 = {k: v.copy() for k, v in bm.solve().items()}
    check_batch((name, variant, "cold"), p, g0, K.oracle_solve(models), exact, q=q)
    if variant == "plain":
        bm.reset()
        same_outputs(bm.solve(), g0, exact)
    else:
        # soft rows without equalities (the degenerate variant has none): a reset reproduces the cold solve
        pd = K.problems(name, "degenerate")
        bd = batch_model(pd)
        bd.setup(pd["H"], pd["f"], pd["A"], pd["bupper"], pd["blower"], pd["sense"])
        gd = {k: v.copy() for k, v in bd.solve().items()}
        bd.reset()
        same_outputs(bd.solve(), gd, exact)
        bd.close()
        # with equalities a solve after a reset is another solve (docstring), but the same one every time
        be = batch_model(p)
        be.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"])
        be.solve()
        be.reset()
        ga = {k: v.copy() for k, v in be.solve().items()}
        be.reset()
        same_outputs(be.solve(), ga, exact)
        be.close()
    for step, (what, data) in enumerate(K.warm_steps(name, variant)):
        if what == "d":
            bm.update(bupper=data["bupper"], blower=data["blower"])
            for k in range(N):
                assert models[k].update(O.UPDATE_d, bupper=data["bupper"][k], blower=data["blower"][k]) == 0
        else:
            bm.update(f=data["f"])
            for k in range(N):
                assert models[k].update(O.UPDATE_v, f=data["f"][k]) == 0
        check_batch((name, variant, "step", step), p, bm.solve(), K.oracle_solve(models), exact, data=data, q=q)
    bm.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("name", K.SHARED_FAMILIES)
def test_kkt_shared(oracle, gpu_lib, monkeypatch, name, exact):
    """setup_shared: one H and A (problem 0 of the plain family), per-problem f and bounds; the certificate per problem with the shared
    matrices"""
    import daqp_amd
    fam, p = K.family(name), K.problems(name, "plain")
    set_env(monkeypatch, fam["env"], exact)
    N, n, m, ms = p["N"], p["n"], p["m"], p["ms"]
    H, A = p["H"][0], p["A"][0]
    rng = np.random.default_rng([K.seed_of(fam.get("data", name)), 78])
    f = p["f"][0][None, :] + 0.02 * rng.standard_normal((N, n))
    shift = 0.005 * rng.standard_normal((N, m))
    bu, bl = p["bupper"][0][None, :] + shift, p["blower"][0][None, :] + shift
    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup_shared(H, f, A, bu, bl, None)
    g = bm.solve()
    bm.close()
    q = R.row_q(H, A, ms)
    for k in range(N):
        om = oracle.model(n, m, ms)
        assert om.setup(H, f[k], A, np.full(m, 1e30), np.full(m, -1e30), None) >= 0
        assert om.update(O.UPDATE_v | O.UPDATE_d, f=f[k], bupper=bu[k], blower=bl[k]) == 0
        check_one((name, "shared", k), (H, f[k], A, bu[k], bl[k], None), ms,
                  tuple(g[key][k] for key in ("x", "lam", "fval", "exitflag", "iter", "soft_slack")), om.solve(with_soft=True), exact, q=q)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("name,variant", K.SINGLE_CASES)
def test_kkt_single_problem(oracle, gpu_lib, monkeypatch, name, variant, exact):
    """daqp_quadprog and setup_daqp / daqp_solve / daqp_update_ldp on one problem: the N == 1 mapped output slab and daqp_extract_result"""
    import daqp_amd
    fam, p = K.family(name), K.problems(name, variant)
    set_env(monkeypatch, fam["env"], exact)
    n, m, ms = p["n"], p["m"], p["ms"]
    H, f, A, bu, bl, sense = K.problem(p, 1)
    s = np.zeros(m, np.int32) if sense is None else sense
    q = R.row_q(H, A, ms)
    x, fval, flag, info = daqp_amd.solve(H, f, A, bu, bl, s)
    om = oracle.model(n, m, ms, ns=p["ns_max"])
    assert om.setup(H, f, A, bu, bl, sense, init_mask=64 + 128) >= 0
    check_one((name, variant, "solve"), (H, f, A, bu, bl, sense), ms, (x, info["lam"], fval, flag, info["iterations"], info["soft_slack"]),
              om.solve(with_soft=True), exact, q=q)
    mdl = daqp_amd.Model()
    assert mdl.setup(H, f, A, bu, bl, s)[0] >= 0
    om = oracle.model(n, m, ms, ns=p["ns_max"])
    assert om.setup(H, f, A, bu, bl, sense) >= 0
    f2 = f + 0.05 * np.random.default_rng([K.seed_of(fam.get("data", name)), 79]).standard_normal(n)
    for step, fk in enumerate((f, f2)):
        if step:
            assert mdl.update(f=fk) == om.update(O.UPDATE_v, f=fk)
        x, fval, flag, info = mdl.solve()
        check_one((name, variant, "Model", step), (H, fk, A, bu, bl, sense), ms, (x, info["lam"], fval, flag, info["iterations"], info["soft_slack"]),
                  om.solve(with_soft=True), exact, q=q)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("name", [f["name"] for f in K.PROX_FAMILIES])
def test_kkt_prox(oracle, gpu_lib, monkeypatch, name, exact):
    """singular Hessians and LPs through the proximal loop: the certificate in the problem's own units, fval against f'x + x'Hx / 2 and
    against the oracle"""
    import daqp_amd
    p = K.prox_problems(name)
    set_env(monkeypatch, {}, exact)
    g = daqp_amd.solve_batch(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms=p["ms"])
    ref = K.oracle_solve(K.oracle_models(oracle, p, 64 + 128))
    assert np.isin(ref["exitflag"], (1, 2)).all(), ref["exitflag"]
    check_batch((name,), p, g, ref, exact, group="prox")
