"""daqp_batch_backward_nullspace, what can be checked without a GPU: that the batches tests/test_gpu_backward_nullspace.py runs are what
it needs them to be (on the oracle alone), that its dense reference is the derivative (central differences of a fixed-W KKT solve),
that its checker rejects a wrong answer, and that the entry point is declared, exported and reachable from Python."""
import importlib.util
import inspect
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("backward_nullspace_cases", os.path.join(HERE, "backward_nullspace_cases.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

_oracle_side = {}


def _side(oracle, name):
    if name not in _oracle_side:
        _oracle_side[name] = B.oracle_solve(oracle, name)
    return _oracle_side[name]


@pytest.mark.parametrize("name", list(B.CASES))
def test_case_meets_its_conditions_on_the_oracle(oracle, name):
    """every problem ends OPTIMAL after going through the proximal loop, |lam| >= 1e-8 on W, cond_2(K) <= 1e6, every inactive row at
    least 1e-6 inside its bounds, and the working sets have the sizes the family is about (n for the LPs, strictly between 0 and n
    for dense PSD, 0 for the empty-W case, both equality rows in W)"""
    ref = _side(oracle, name)
    sizes, lam_min, cond, slack = B.check_inputs(name, ref)
    print(f"{name}: |W| {sizes.min()}..{sizes.max()}, min |lam| on W {lam_min:.1e}, max cond_2(K) {cond:.1e}, min slack {slack:.1e}")


def test_every_family_and_size_is_in_the_table():
    assert {c["family"] for c in B.CASES.values()} == set(B.FAMILIES)
    assert {c["shape"][0] for c in B.CASES.values()} >= {2, 5, 16, 33, 64}
    assert all(c["shape"][0] <= 64 for c in B.CASES.values())
    assert B.CASES["lp_n64"]["family"] == 1 and B.CASES["free_n64"]["shape"][0] == 64


def _fixed_w_solve(H, A, ms, W, f, bW):
    n = f.size
    K, _ = B.kkt(H, A, ms, W, n)
    sol = np.linalg.solve(K, np.concatenate([-f, bW]))
    return sol[:n], sol[n:]


@pytest.mark.parametrize("name", ["lp_n5", "psd_n5", "diag_n16"])
def test_dense_reference_against_central_differences(oracle, name):
    """dl/df = -dz, dl/dH = -1/2 (dz x' + x dz'), dl/dA_i = -(lam_i dz + dnu_i x)', dl/db_W = dnu from the dense reference
    (np.linalg.solve on the full KKT matrix) against central differences (step 1e-6) of l = g'x, x from the KKT system with the
    working set fixed and a singular (or zero) H.  Tolerance 1e-8 of max(1, |gradient|_max), as in test_cpu_backward_soft.py: the
    rounding error of a central difference is about |l| 2^-52 / step = 2e-10 per unit of l, fifty times that."""
    n, m, ms = B.CASES[name]["shape"]
    q = B.batch(name)
    ref = _side(oracle, name)
    k = 0
    H, f, A, bu, bl, sense = B.problem(name, q, k)
    H0 = np.zeros((n, n)) if H is None else H
    W = ref["ws"][k]
    bW = np.where(ref["lower"][k][W], bl[W], bu[W])
    g = B.grad(q["f"].shape[0], n)[k]
    x, lamW = _fixed_w_solve(H0, A, ms, W, f, bW)
    assert np.abs(x - ref["x"][k]).max() < 1e-6, "the fixed-W system is not the oracle's optimum"
    dz, dnuW = B.dense_adjoint(H, A, ms, W, g)
    lam, dnu = np.zeros(m), np.zeros(m)
    lam[W], dnu[W] = lamW, dnuW
    gH = -0.5 * (np.outer(dz, x) + np.outer(x, dz))
    gA = -(np.outer(lam[ms:], dz) + np.outer(dnu[ms:], x))
    eps = 1e-6
    base = (H0, f, A, bW)
    loss = lambda Hh, ff, AA, bb: float(g @ _fixed_w_solve(Hh, AA, ms, W, ff, bb)[0])

    def fd(which, E):
        hi, lo = list(base), list(base)
        hi[which] = base[which] + eps * E
        lo[which] = base[which] - eps * E
        return (loss(*hi) - loss(*lo)) / (2 * eps)

    def unit(shape, idx):
        E = np.zeros(shape)
        E[idx] = 1.0
        return E

    mA = m - ms
    rows = sorted({int(i) - ms for i in W if i >= ms})[:3] + [i for i in range(mA) if i + ms not in set(W.tolist())][:1]
    fdf = np.array([fd(1, unit(n, i)) for i in range(n)])
    fdb = np.array([fd(3, unit(len(W), i)) for i in range(len(W))])
    fdH = np.array([[fd(0, 0.5 * (unit((n, n), (i, j)) + unit((n, n), (j, i)))) for j in range(n)] for i in range(n)])
    fdA = np.array([[fd(2, unit((mA, n), (i, j))) for j in range(n)] for i in rows])
    worst = 0.0
    for what, got, want in (("f", -dz, fdf), ("b", dnuW, fdb), ("H", gH, fdH), ("A", gA[rows], fdA)):
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        worst = max(worst, err)
        assert err <= 1e-8, (name, what, err)
    print(f"{name}: max error against central differences: {worst:.2e}")


def test_checker_rejects_a_wrong_answer(oracle):
    """check_adjoint passes the dense reference itself and fails on dz off by 1e-8 of the scale and on a dnu on the wrong side"""
    name = "psd_n16"
    n, m, ms = B.CASES[name]["shape"]
    q = B.batch(name)
    N = q["f"].shape[0]
    ref = _side(oracle, name)
    refsol = B.reference(name, ref, B.grad(N, n))

    def answer():
        o = dict(dz=np.zeros((N, n)), dbupper=np.zeros((N, m)), dblower=np.zeros((N, m)), status=np.zeros(N, np.int32))
        cap = n + 1
        na, ws = np.zeros(N, np.int32), np.full((N, cap), -1, np.int32)
        for k, R in enumerate(refsol):
            W = R["W"]
            o["dz"][k] = R["dz"]
            lower = ref["lower"][k][W]
            o["dblower"][k][W[lower]] = R["dnu"][lower]
            o["dbupper"][k][W[~lower]] = R["dnu"][~lower]
            na[k] = len(W)
            ws[k, :len(W)] = W[::-1]
        return dict(exitflag=ref["flag"]), na, ws, o

    r, na, ws, o = answer()
    assert B.check_adjoint(name, ref, refsol, r, na, ws, o) == 0.0
    r, na, ws, o = answer()
    o["dz"][3, 2] += 1e-8 * refsol[3]["scale"]
    with pytest.raises(AssertionError):
        B.check_adjoint(name, ref, refsol, r, na, ws, o)
    r, na, ws, o = answer()
    i = refsol[5]["W"][0]
    o["dbupper"][5, i], o["dblower"][5, i] = o["dblower"][5, i], o["dbupper"][5, i]
    with pytest.raises(AssertionError):
        B.check_adjoint(name, ref, refsol, r, na, ws, o)
    r, na, ws, o = answer()
    ws[1, 0] = [i for i in range(m) if i not in set(refsol[1]["W"].tolist())][0]
    with pytest.raises(AssertionError):
        B.check_adjoint(name, ref, refsol, r, na, ws, o)


def test_nullspace_entry_declared_exported_and_reachable():
    import daqp_amd
    from daqp_amd import _lib, layer
    from daqp_amd.api import BatchModel
    L = daqp_amd.lib()
    assert "daqp_batch_backward_nullspace" in _lib.EXPORTS and hasattr(L, "daqp_batch_backward_nullspace")
    assert L.daqp_batch_backward_nullspace(None, None, None, None, None, None, 0, 0) != 0      # refused, not dereferenced
    assert "null" in daqp_amd.last_error()
    with open(os.path.join(ROOT, "include", "daqp_amd.h")) as fh:
        header = fh.read()
    assert "int daqp_batch_backward_nullspace(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower, int *status," in header
    for words in ("dz = Z Hr^-1 Z' g", "R_jj^2 < settings->zero_tol", "zero_tol max(1, max_i H_ii)", "n > 64", "ns_max > 0 are refused"):
        assert words in header, words
    assert inspect.signature(layer.qp_layer).parameters["nullspace"].default is False
    assert inspect.signature(BatchModel.backward).parameters["nullspace"].default is False
    assert "nullspace.hip.h" in _lib.UNITS["backward_kernel.hip"]
