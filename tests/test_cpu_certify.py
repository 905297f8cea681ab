"""daqp_certify_batch without a GPU: the interface is there and refuses loudly, the exact reference of tests/certify_cases.py agrees
with tests/kkt_reference.py on the solver's own case families, and the constructed cases have the properties the GPU test relies on."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import certify_cases as CC
import kkt_cases as K
import kkt_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD_EPS = Fraction(1, 2 ** 64)      # unit roundoff of the x87 extended format np.longdouble is on the hosts that run these tests


def test_entry_is_declared_exported_and_reachable():
    import daqp_amd
    from daqp_amd import _lib
    with open(os.path.join(ROOT, "include", "daqp_amd.h")) as fh:
        header = fh.read()
    assert "int daqp_certify_batch(DAQPBatchCertificate *out, const DAQPBatchProblem *p, const c_float *x, const c_float *lam," in header
    assert "} DAQPBatchCertificate;" in header
    for word in ("stationarity_scale", "ray_support", "PROVES NOTHING", "(K + 2)^2 2^-104 S"):
        assert word in header, word
    assert "daqp_certify_batch" in _lib.EXPORTS and hasattr(daqp_amd.lib(), "daqp_certify_batch")
    assert "certify_kernel.hip" in _lib.UNITS and "certify.hip.h" in _lib.UNITS["post_solve.hip"]
    assert callable(daqp_amd.certify_batch) and "certify_batch" in daqp_amd.__all__
    assert callable(daqp_amd.BatchModel.certify)
    assert [k for k, _ in _lib.DAQPBatchCertificate._fields_] == list(CC.REAL_KEYS + CC.INT_KEYS)


def test_kernels_use_no_scratch():
    """the resource report of the build: both kernel variants keep their pairs in registers"""
    from daqp_amd import _lib
    res = {k: v for k, v in _lib.kernel_resources().items() if k.startswith("k_certify")}
    assert {"k_certify_wave<4>", "k_certify_wg<2>", "k_certify_wg<4>", "k_certify_wg<8>"} <= set(res), sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)


def test_refuses_without_a_device():
    import daqp_amd
    from daqp_amd import _lib
    L = daqp_amd.lib()
    q = CC.stack([CC.kkt_point(7, 20, 3, 1)], 2)
    if L.daqp_amd_device_count() < 1:
        with pytest.raises(RuntimeError, match="no HIP device"):
            daqp_amd.certify_batch(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["x"], q["lam"], q["sense"])
        out = np.zeros(2)
        cert = _lib.DAQPBatchCertificate(stationarity=out.ctypes.data)
        p = _lib.DAQPBatchProblem(2, 7, 20, 3, q["H"].ctypes.data, q["f"].ctypes.data, q["A"].ctypes.data, q["bupper"].ctypes.data,
                                  q["blower"].ctypes.data, None, _lib.MEM_HOST)
        assert L.daqp_certify_batch(C.byref(cert), C.byref(p), q["x"].ctypes.data, q["lam"].ctypes.data, 0, -1, None) == -8
        assert "no HIP device" in _lib.last_error()
    # refusals that need no device: they come first
    p = _lib.DAQPBatchProblem(2, 7, 20, 8, q["H"].ctypes.data, q["f"].ctypes.data, q["A"].ctypes.data, q["bupper"].ctypes.data,
                              q["blower"].ctypes.data, None, _lib.MEM_HOST)
    cert = _lib.DAQPBatchCertificate()
    assert L.daqp_certify_batch(C.byref(cert), C.byref(p), q["x"].ctypes.data, q["lam"].ctypes.data, 0, -1, None) != 0
    assert "ms=8" in _lib.last_error()
    assert L.daqp_certify_batch(C.byref(cert), C.byref(p), None, q["lam"].ctypes.data, 0, -1, None) != 0
    assert "null" in _lib.last_error()


def _longdouble_slack(ref, K_, S):
    return (K_ + 2) * LD_EPS * S


def check_against_kkt_reference(tag, prob, ms, x, lam):
    """exact() against kkt_reference.certificate(normalised=False) on one problem; the longdouble reference rounds every product and
    sum once: (K + 2) 2^-64 S with K, S of the sum in question -- S bounded here by the largest row / column sum of absolute terms"""
    H, f, A, bu, bl, sense = prob
    e = CC.exact(H, f, A, bu, bl, sense, ms, x, lam)
    c = R.certificate(H, f, A, bu, bl, sense, ms, x, lam, K.RHO_SOFT, normalised=False)
    n, m = f.size, bu.size
    Cm = np.abs(R.constraint_matrix(A, ms, n).astype(np.float64))
    S_col = (0.0 if H is None else (np.abs(H) @ np.abs(x)).max()) + np.abs(f).max() + (Cm.T @ np.abs(lam)).max()
    finite = np.minimum(np.abs(bu), np.abs(bl))      # the bound a row can be near (the other one may be +-1e30)
    S_row = (Cm @ np.abs(x) + finite).max()
    Kst = n + m + 2
    stat_ref = e["stationarity"][0] / e["stationarity_scale"][0]
    assert abs(Fraction(c["stationarity"]) - stat_ref) <= 2 * _longdouble_slack(stat_ref, Kst, Fraction(S_col)) + Fraction(1, 2 ** 52) * stat_ref, (tag, c["stationarity"], float(stat_ref))
    for key in ("primal", "complementarity"):
        assert abs(Fraction(c[key]) - e[key][0]) <= _longdouble_slack(e[key][0], n + 1, Fraction(S_row)) + Fraction(1, 2 ** 52) * e[key][0], (tag, key, c[key], float(e[key][0]))
    assert c["wrong_sign"] == e["wrong_sign"], (tag, c["wrong_sign"], e["wrong_sign"])
    return e, c


@pytest.mark.parametrize("name", ["tiny", "reg21", "wg70"])
@pytest.mark.parametrize("variant", K.VARIANTS)
def test_exact_reference_agrees_with_kkt_reference(oracle, name, variant):
    """on the oracle's own (x, lam) of the solver's case families: stationarity / stationarity_scale, primal, complementarity,
    wrong_sign, and the objective against fval_ref where no soft row is active"""
    p = K.problems(name, variant)
    ref = K.oracle_solve(K.oracle_models(oracle, p, 0))
    for k in range(min(p["N"], 4)):
        prob = K.problem(p, k)
        e, c = check_against_kkt_reference((name, variant, k), prob, p["ms"], ref["x"][k], ref["lam"][k])
        obj = e["objective"][0]
        assert abs(Fraction(c["fval_ref"]) - obj) <= Fraction(1, 2 ** 50) * max(1, abs(obj)) + e["objective"][1]


@pytest.mark.parametrize("name", ["singular12", "lp24"])
def test_exact_reference_agrees_with_kkt_reference_prox(oracle, name):
    p = K.prox_problems(name)
    ref = K.oracle_solve(K.oracle_models(oracle, p, 0))
    for k in range(min(p["N"], 4)):
        check_against_kkt_reference((name, k), K.problem(p, k), p["ms"], ref["x"][k], ref["lam"][k])


@pytest.mark.parametrize("shape", CC.SHAPES, ids=str)
def test_constructed_cases_are_what_they_claim(shape):
    """(a) is exactly zero, (b) has the planted size, (c) defeats float64 (asserted inside the builder), (d) has residual 0 and the known
    support"""
    n, m, ms = shape
    pool = dict((q["kind"], (q, e)) for q, e in CC.pool(shape))
    q, e = pool["kkt_point"]
    for key in ("stationarity", "primal", "complementarity"):
        assert e[key][0] == 0, key
    assert e["wrong_sign"] == 0 and e["primal_row"] == -1
    d = Fraction(CC.DELTA)
    q, e = pool["defect_sign"]
    if q["planted_row"] >= 0:
        k = q["planted_row"]
        row = np.eye(n)[k] if k < ms else q["A"][k - ms]
        assert e["wrong_sign"] == 1 and e["stationarity"][0] == 2 * abs(Fraction(q["lam"][k])) * Fraction(np.abs(row).max())
    q, e = pool["defect_bound"]
    if q["planted_row"] >= 0:
        assert e["primal"][0] == d and e["primal_row"] == q["planted_row"] and e["stationarity"][0] == 0
    q, e = pool["defect_equality"]
    if q["planted_row"] >= 0:
        assert e["complementarity"][0] == d and e["primal"][0] == d and e["primal_row"] == q["planted_row"]
    q, e = pool["defect_x"]
    assert e["stationarity"][0] > 0
    q, e = pool["cancellation"]
    assert e["stationarity"][0] == Fraction(1, 2 ** 20) and e["stationarity_scale"][0] > 2 ** 38
    for kind in ("ray_parallel", "ray_cycle", "ray_cycle_feasible_twin"):
        if kind in pool:
            q, e = pool[kind]
            assert e["ray_residual"][0] == 0 and e["ray_support"][0] == q["expect_support"], kind      # (ray_scale is C'|lam| with C's signs: 0 for the cycle)
            assert (e["ray_support"][0] < 0) == (kind != "ray_cycle_feasible_twin")
    assert ("ray_parallel" in pool) == (m - ms >= 2) and ("ray_cycle" in pool) == (m - ms >= 3)
