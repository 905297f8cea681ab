"""The KKT certificate (tests/kkt_reference.py) on the oracle's own solutions of every case family (tests/kkt_cases.py): the bars the GPU
tests import are 100 x what the oracle itself leaves (a), the two derived formulas are the reference's (b), and the families contain
what the GPU tests claim to exercise (c).  `python tests/test_cpu_kkt_reference.py` prints the measured table for kkt_cases.BARS."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):      # (also run as a script: see the module docstring)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import kkt_cases as K            # noqa: E402
import kkt_reference as R        # noqa: E402

QP_KEYS = ("stationarity", "primal", "complementarity", "soft_relation", "fval", "soft_slack")
PROX_KEYS = ("stationarity", "primal", "complementarity", "fval")
_cache = {}


def rel(a, ref):
    return abs(a - ref) / max(1.0, abs(ref))


def run_family(oracle, data, variant):
    """oracle results and certificates of one data set: (problems, results, [certificate or None per problem])"""
    key = (data, variant)
    if key not in _cache:
        p = K.problems(data, variant)
        r = K.oracle_solve(K.oracle_models(oracle, p))
        certs = []
        for k in range(p["N"]):
            H, f, A, bu, bl, s = K.problem(p, k)
            certs.append(R.certificate(H, f, A, bu, bl, s, p["ms"], r["x"][k], r["lam"][k], K.RHO_SOFT) if r["exitflag"][k] in (1, 2) else None)
        _cache[key] = (p, r, certs)
    return _cache[key]


def run_prox(oracle, name):
    if name not in _cache:
        p = K.prox_problems(name)
        r = K.oracle_solve(K.oracle_models(oracle, p))
        certs = []
        for k in range(p["N"]):
            H, f, A, bu, bl, s = K.problem(p, k)
            certs.append(R.certificate(H, f, A, bu, bl, s, p["ms"], r["x"][k], r["lam"][k], K.RHO_SOFT, normalised=False)
                         if r["exitflag"][k] in (1, 2) else None)
        _cache[name] = (p, r, certs)
    return _cache[name]


def worst_of(r, certs, keys):
    w = dict.fromkeys(keys, 0.0)
    for k, c in enumerate(certs):
        if c is None:
            continue
        for key in keys:
            if key == "fval":
                v = rel(r["fval"][k], c["fval_ref"])
            elif key == "soft_slack":
                v = rel(r["soft_slack"][k], c["soft_slack_ref"])
            else:
                v = c[key]
            w[key] = max(w[key], v)
    return w


def measure(oracle):
    worst = {"qp": dict.fromkeys(QP_KEYS, 0.0), "prox": dict.fromkeys(PROX_KEYS, 0.0)}
    for data in K.DATA_SETS:
        for variant in K.VARIANTS:
            _, r, certs = run_family(oracle, data, variant)
            for key, v in worst_of(r, certs, QP_KEYS).items():
                worst["qp"][key] = max(worst["qp"][key], v)
    for fam in K.PROX_FAMILIES:
        _, r, certs = run_prox(oracle, fam["name"])
        for key, v in worst_of(r, certs, PROX_KEYS).items():
            worst["prox"][key] = max(worst["prox"][key], v)
    return worst


def test_bars_are_a_hundred_times_the_oracles_worst(oracle):
    """a: the certificate of the oracle's (x, lam) on every family; BARS records the worst value and the bar derived from it"""
    worst = measure(oracle)
    for group, keys in (("qp", QP_KEYS), ("prox", PROX_KEYS)):
        for key in keys:
            rec_worst, bar = K.BARS[group][key]
            assert worst[group][key] <= 2 * rec_worst, (group, key, worst[group][key], rec_worst)   # (the record is what was measured; another libm may differ a little)
            assert bar == K.bar_from(rec_worst, hi=K.CAPS[group][key]), (group, key, bar)
            assert worst[group][key] < bar, (group, key, worst[group][key], bar)


@pytest.mark.parametrize("variant", K.VARIANTS)
@pytest.mark.parametrize("data", K.DATA_SETS)
def test_certificate_and_formulas_on_the_oracle(oracle, data, variant):
    """a per family (no wrong sign, no multiplier on an inactive row) and b: soft_slack_ref and fval_ref are the oracle's soft_slack and
    fval of the same (x, lam), to 1e-10 max(1, |value|)"""
    p, r, certs = run_family(oracle, data, variant)
    for k, c in enumerate(certs):
        if c is None:
            continue
        for key in ("stationarity", "primal", "complementarity", "soft_relation"):
            assert c[key] < K.BARS["qp"][key][1], (k, key, c[key])
        assert c["wrong_sign"] == 0 and c["nonzero_inactive"] == 0, (k, c["wrong_sign"], c["nonzero_inactive"])
        assert rel(r["fval"][k], c["fval_ref"]) <= 1e-10, (k, r["fval"][k], c["fval_ref"])
        assert rel(r["soft_slack"][k], c["soft_slack_ref"]) <= 1e-10, (k, r["soft_slack"][k], c["soft_slack_ref"])


@pytest.mark.parametrize("name", [f["name"] for f in K.PROX_FAMILIES])
def test_certificate_on_the_oracle_proximal(oracle, name):
    p, r, certs = run_prox(oracle, name)
    assert all(c is not None for c in certs), r["exitflag"]
    for k, c in enumerate(certs):
        for key in ("stationarity", "primal", "complementarity"):
            assert c[key] < K.BARS["prox"][key][1], (k, key, c[key])
        assert c["wrong_sign"] == 0, k
        assert rel(r["fval"][k], c["fval_ref"]) <= 1e-10, (k, r["fval"][k], c["fval_ref"])
        assert r["soft_slack"][k] == 0.0


@pytest.mark.parametrize("variant", K.VARIANTS)
@pytest.mark.parametrize("data", K.DATA_SETS)
def test_coverage(oracle, data, variant):
    """c: what keeps a green GPU test from proving nothing, on the oracle alone"""
    p, r, certs = run_family(oracle, data, variant)
    N, ms, lam, flags = p["N"], p["ms"], r["lam"], r["exitflag"]
    ok = np.isin(flags, (1, 2))
    if variant == "degenerate":
        assert (~ok).sum() <= 0.25 * N, flags
    else:
        assert ok.all(), flags
    lam_ok = lam[ok]
    assert (lam_ok > 0).any() and (lam_ok < 0).any(), "active rows on one side only"
    if ms > 0:
        assert (lam_ok[:, :ms] != 0).any() and (lam_ok[:, ms:] != 0).any(), "no active simple bound / general row"
    if variant != "plain":
        soft = (p["sense"] & R.SOFT) != 0
        with_soft = ((lam != 0) & soft).any(axis=1) & ok
        assert with_soft.sum() >= 0.9 * N, (int(with_soft.sum()), N)
        # soft_slack > primal_tol, i.e. SOFT_OPTIMAL: not on every such problem (kkt_cases.py, "Soft rows", has the share per family and why
        # it cannot be all of them with well-determined multipliers), but on at least one per family and variant
        assert (r["soft_slack"][with_soft] > 0).all() and np.array_equal(flags[ok] == 2, r["soft_slack"][ok] > K.PRIMAL_TOL), r["soft_slack"]
        if (data, variant) != ("rows193", "degenerate"):
            assert (flags[with_soft] == 2).any(), r["soft_slack"]
    # well determined: a change of the data by the default mode's own LDP difference leaves the path alone and lam within a tenth of the
    # bar the GPU's lam is held to (kkt_cases.py, "Conditioning")
    r2 = K.oracle_solve(K.oracle_models(oracle, K.perturbed(p)))
    assert np.array_equal(r2["exitflag"], flags) and np.array_equal(r2["iter"], r["iter"])
    assert np.abs(r2["lam"] - lam).max() < K.PROBE_LAM, np.abs(r2["lam"] - lam).max()
    if variant == "sense":
        eq = (p["sense"] & R.IMMUTABLE) != 0
        le = lam[eq & ok[:, None]]
        assert (le > 0).any() and (le < 0).any(), "equality multipliers of one sign only"


@pytest.mark.parametrize("variant", ["plain", "sense"])
@pytest.mark.parametrize("name", K.WARM_FAMILIES)
def test_warm_steps_on_the_oracle(oracle, name, variant):
    """the warm steps of test_gpu_kkt.test_kkt_warm on the oracle alone: its own certificate under the bars after every step, and every
    step's solution well determined (the probe of test_coverage)"""
    p = K.problems(name, variant)
    models, probes = K.oracle_models(oracle, p), K.oracle_models(oracle, p)
    K.oracle_solve(models), K.oracle_solve(probes)
    for what, data in K.warm_steps(name, variant):
        pert = K.perturbed(dict(p, **data))
        for k in range(p["N"]):
            if what == "d":
                assert models[k].update(K.O.UPDATE_d, bupper=data["bupper"][k], blower=data["blower"][k]) == 0
                assert probes[k].update(K.O.UPDATE_d, bupper=pert["bupper"][k], blower=pert["blower"][k]) == 0
            else:
                assert models[k].update(K.O.UPDATE_v, f=data["f"][k]) == 0 and probes[k].update(K.O.UPDATE_v, f=pert["f"][k]) == 0
        r, r2 = K.oracle_solve(models), K.oracle_solve(probes)
        assert np.isin(r["exitflag"], (1, 2)).all(), r["exitflag"]
        assert np.array_equal(r2["exitflag"], r["exitflag"]) and np.array_equal(r2["iter"], r["iter"])
        assert np.abs(r2["lam"] - r["lam"]).max() < K.PROBE_LAM, np.abs(r2["lam"] - r["lam"]).max()
        for k in range(p["N"]):
            H, f, A, bu, bl, s = K.problem(p, k)
            c = R.certificate(H, data["f"][k], A, data["bupper"][k], data["blower"][k], s, p["ms"], r["x"][k], r["lam"][k], K.RHO_SOFT)
            for key in ("stationarity", "primal", "complementarity", "soft_relation"):
                assert c[key] < K.BARS["qp"][key][1], (k, key, c[key])


if __name__ == "__main__":
    from oracle import oracle as O
    w = measure(O.Oracle())
    for group in ("qp", "prox"):
        print(f'    "{group}": {{')
        for key, v in w[group].items():
            up = float(f"{v:.1e}") if v else 0.0
            up = up if up >= v else float(f"{v * 1.05:.1e}")
            print(f'        "{key}": ({up:.1e}, {K.bar_from(up, hi=K.CAPS[group][key]):.0e}),')
        print("    },")
