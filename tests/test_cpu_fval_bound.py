"""fval_bound on the oracle alone (no GPU): the oracle's branch against the reference's recorded outputs (tests/golden/golden_fval_bound.npz,
bit for bit), and the conditions that tests/fval_bound_cases.py promises of the bounds tests/test_gpu_fval_bound.py runs the GPU at --
coverage (early / mixed / all / none / tight), clearance of every level of every problem from 2 fval_bound, stability of (flag, iter)
under a move of the bound by that clearance, and the units of lam at the bound exit."""
import os

import numpy as np
import pytest

import fval_bound_cases as F
import kkt_cases as K
import kkt_reference as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(d, v) for d in K.DATA_SETS for v in F.VARIANTS]


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def test_oracle_matches_golden_fval_bound(oracle):
    """the reference's outputs under a bound -- x, lam and fval at the -1 exit included -- bit for bit; then the warm sequence bound ->
    DAQP_INF (continues from the kept working set) -> new f under a bound on one workspace"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_fval_bound.npz"), allow_pickle=False)
    names = sorted({k.split("/")[0] for k in g.files} - {"warm"})
    flags = {}
    for nm in names:
        get = lambda key: g[f"{nm}/{key}"]
        H = get("H") if get("H").size else None
        assert get("f").size <= 12
        x, lam, fval, flag, it = oracle.quadprog(H, get("f"), get("A"), get("bupper"), get("blower"), get("sense"),
                                                 O.default_settings(fval_bound=float(get("fval_bound"))))
        assert flag == int(get("exitflag")) and it == int(get("iter")), (nm, flag, it, int(get("exitflag")), int(get("iter")))
        assert bits_equal(x, get("x")) and bits_equal(lam, get("lam")) and bits_equal(fval, get("fval")), nm
        flags.setdefault(nm.rsplit("_", 1)[1].rstrip("0123456789"), []).append(flag)
    assert len(names) >= 36
    assert set(flags["mid"]) == {-1} and set(flags["below"]) == {-1} and -1 not in flags["none"] and 1 in flags["at"] + flags["none"], flags
    w = lambda key: g[f"warm/{key}"]
    n, m, ms = int(w("n")), int(w("m")), int(w("ms"))
    om = oracle.model(n, m, ms, settings=O.default_settings(fval_bound=float(w("bounds")[0])))
    assert om.setup(w("H"), w("f"), w("A"), w("bupper"), w("blower"), None) >= 0
    for t in range(3):
        if t:
            om.settings(fval_bound=float(w("bounds")[t]))
        if t == 2:
            assert om.update(O.UPDATE_v, f=w("f2")) == 0
        x, lam, fval, flag, it = om.solve()
        assert flag == int(w("exitflag")[t]) and it == int(w("iter")[t]), (t, flag, it)
        assert bits_equal(x, w("x")[t]) and bits_equal(lam, w("lam")[t]) and bits_equal(fval, w("fval")[t]), t
    assert list(w("exitflag")) == [-1, 1, -1]


@pytest.mark.parametrize("data,variant", CASES)
def test_recorded_bounds_are_what_the_search_gives(data, variant):
    p = K.problems(data, variant)
    s = F.search(F.unbounded(data, variant)["levels"])
    rec = F.RECORDED[data][variant]
    for kind in F.KINDS:
        assert kind in s, (data, variant, kind, "no clear bound meets this kind")
        assert abs(rec[kind][0] - s[kind]) <= 1e-12 * max(1.0, abs(s[kind])), (kind, rec[kind][0], s[kind])
        for b in (s[kind], rec[kind][0]):
            r = F.run(p, b)
            assert rec[kind][1:] == (int((r["exitflag"] == -1).sum()), p["N"], int(r["iter"].min()), int(r["iter"].max())), (kind, rec[kind])
    assert rec["tight"][:2] == s["tight"][:2] and abs(rec["tight"][2] - s["tight"][2]) <= 1e-12 * s["tight"][2]


@pytest.mark.parametrize("data,variant", CASES)
def test_coverage_clearance_and_probe(data, variant):
    p = K.problems(data, variant)
    N = p["N"]
    ub = F.unbounded(data, variant)
    levels = ub["levels"]
    assert np.isin(ub["exitflag"], (1, 2)).all()
    for kind in F.KINDS:
        b = F.bound(data, variant, kind)
        c = F.classify(levels, b)
        r = F.run(p, b)
        # the oracle does what the levels say: -1 exactly where a level exceeds 2 b, having passed exactly the levels up to that one
        for k in range(N):
            j = F.stop_index(levels[k], b)
            assert (r["exitflag"][k] == -1) == (j >= 0), (kind, k)
            if j >= 0:
                assert bits_equal(r["levels"][k], levels[k][: j + 1]), (kind, k)
        stopped = int((r["exitflag"] == -1).sum())
        if kind == "early":
            assert "first" in c
        elif kind == "mixed":
            assert "inside" in c and "runs" in c and 0 < stopped < N
        elif kind == "all":
            assert stopped == N
        else:
            assert stopped == 0 and all(2.0 * b > lv.max() for lv in levels)
            for key in ("x", "lam", "fval", "soft_slack"):
                assert bits_equal(r[key], ub[key]), key
            assert np.array_equal(r["iter"], ub["iter"]) and np.array_equal(r["exitflag"], ub["exitflag"])
            continue
        assert F.clear(levels, b), (kind, "a level within OFFSET of 2 fval_bound")      # every problem, no exclusions
        # daqp_quadprog's setup (solve_batch) passes the same levels
        rq = F.run(p, b, init_mask=64 + 128)
        assert np.array_equal(rq["exitflag"], r["exitflag"]) and np.array_equal(rq["iter"], r["iter"]), kind
        # PROBE: the bound moved by the clearance in either direction leaves every (flag, iter) as it is
        for sgn in (-1.0, 1.0):
            rp = F.run(p, b + sgn * 0.5 * F.OFFSET * max(1.0, abs(2.0 * b)))
            assert np.array_equal(rp["exitflag"], r["exitflag"]) and np.array_equal(rp["iter"], r["iter"]), (kind, sgn)
    # tight: at exactly half the level the problem passes it, one double below it stops there; flag -1 or not follows the later levels
    k, j, at, below = F.bound(data, variant, "tight")
    assert 2.0 * at == levels[k][j] and below < at
    r_at, r_below = F.run(p, at), F.run(p, below)
    assert r_below["exitflag"][k] == -1 and r_below["levels"][k].size == j + 1
    assert r_at["levels"][k].size > j + 1 and r_at["iter"][k] > r_below["iter"][k]


@pytest.mark.parametrize("data,variant", [("tiny", "plain"), ("reg21", "sense"), ("img3", "sense"), ("wg70", "plain")])
def test_lam_at_the_bound_exit_is_in_ldp_units(data, variant):
    """the reference skips ldp2qp_solution at a negative exit (api.c:27): lam is the least-distance problem's, lam_qp = lam / sqrt(q_k).
    Converted, the dual function at it equals the reported fval (kkt_cases' fval bar); fval + 1/2 f'H^-1 f is the compared value w->fval / 2;
    unconverted it does not (so the conversion is needed, not incidental)"""
    p = K.problems(data, variant)
    b = F.bound(data, variant, "mixed")
    r = F.run(p, b)
    bar = K.BARS["qp"]["fval"][1]
    seen = 0
    for k in np.flatnonzero(r["exitflag"] == -1):
        H, f, A, bu, bl, sense = K.problem(p, k)
        q = R.row_q(H, A, p["ms"])
        lam_qp = np.array(r["lam"][k], dtype=R.LD) / np.sqrt(q)
        g = R.dual_value(H, f, A, bu, bl, sense, p["ms"], lam_qp, K.RHO_SOFT, q=q)
        assert abs(float(g) - r["fval"][k]) < bar * max(1.0, abs(r["fval"][k])), (k, float(g), r["fval"][k])
        half_level = r["fval"][k] + float(R.half_f_hinv_f(H, f))
        assert abs(half_level - 0.5 * r["levels"][k][-1]) < bar * max(1.0, half_level) and half_level > b
        g_raw = R.dual_value(H, f, A, bu, bl, sense, p["ms"], r["lam"][k], K.RHO_SOFT, q=q)
        seen += int(abs(float(g_raw) - r["fval"][k]) > 1e-6 * max(1.0, abs(r["fval"][k])))
    assert seen > 0


@pytest.mark.parametrize("name", [f["name"] for f in K.PROX_FAMILIES])
def test_prox_bounds(name):
    """proximal families: the recorded bound is the one the bisection finds, some problems end -1 there and some do not, and a relative
    +-1e-6 change of the bound leaves every (flag, iter) as it is"""
    p = K.prox_problems(name)
    b, stopped, N = F.PROX_RECORDED[name]
    assert F.prox_search(name) == (b, stopped)
    r = F.prox_run(p, b)
    assert int((r["exitflag"] == -1).sum()) == stopped and 0 < stopped < N == p["N"]
    assert F.prox_stable(p, b)


@pytest.mark.parametrize("variant", F.VARIANTS)
@pytest.mark.parametrize("name", K.WARM_FAMILIES)
def test_warm_sequence_bounds(name, variant):
    """bound -> DAQP_INF -> new f under a bound: the second solve ends at the unbounded optimum in fewer iterations than a cold solve
    needs for the stopped problems together (it continues), and the last bound splits the warm step's levels and is clear of them"""
    outs, b3, _ = F.warm_reference(name, variant)
    ub = F.unbounded(F.data_of(name), variant)
    stopped = outs[0]["exitflag"] == -1
    assert 0 < stopped.sum() < stopped.size and np.isin(outs[1]["exitflag"], (1, 2)).all()
    assert np.abs(outs[1]["x"] - ub["x"]).max() < 1e-9
    assert (outs[1]["iter"][stopped] + outs[0]["iter"][stopped]).sum() <= (ub["iter"][stopped] + 1).sum()
    assert (outs[1]["iter"][~stopped] == 1).all()
    s3 = outs[2]["exitflag"] == -1
    assert 0 < s3.sum() < s3.size
    lv = F.warm_reference.__wrapped__(name, variant)[0][2]["levels"]
    assert all((l.max() > 2 * b3) == s for l, s in zip(lv, s3))


@pytest.mark.parametrize("name", K.SHARED_FAMILIES)
def test_shared_bounds(name):
    c = F.shared_reference(name)
    st = c["ref"]["exitflag"] == -1
    assert 0 < st.sum() < c["N"] and F.clear(c["ref"]["levels"], c["bound"])


@pytest.mark.parametrize("name,variant", K.SINGLE_CASES)
def test_single_bounds(name, variant):
    b = F.single_bound(name, variant)
    lv = F.unbounded(F.data_of(name), variant)["levels"][1]
    assert 0 < F.stop_index(lv, b) < lv.size - 1
