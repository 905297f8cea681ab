"""The adjoint of an eliminated batch without a GPU: the reduce -> solve -> expand route of tests/eliminate_adjoint_cases.py against
a dense solve of the full KKT system, the gradients it implies against central differences of the optimum, and the C entry declared,
exported and refusing loudly."""
import os

import numpy as np
import pytest

import eliminate_adjoint_cases as AC
import eliminate_cases as EC

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(s, False, i == 0) for i, s in enumerate(EC.SHAPES)] + [(EC.LP_SHAPE, True, False)]
IDS = [str(c[0]) + (" lp" if c[1] else "") for c in CASES]
WHICH = ("g_x", "g_lam", "both")


def case(shape, lp, bound_row, N=2):
    b = EC.make_batch(shape, N, 5, lp=lp, bound_row=bound_row)
    rng = np.random.default_rng(55)
    return b, rng.standard_normal(b["f"].shape), rng.standard_normal(b["bupper"].shape)


def pick(which, gx, gl):
    return (gx if which != "g_lam" else None), (gl if which != "g_x" else None)


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("shape,lp,bound_row", CASES, ids=IDS)
def test_route_equals_the_dense_solve(shape, lp, bound_row, which):
    """Both sides carry the error of their longdouble products only (every solve is refined on longdouble residuals), amplified by at
    most cond(K): the bar is cond(K) 2^-52 relative to the max norm of the solution, per problem."""
    n, neq, m, ms = shape
    b, GX, GL = case(shape, lp, bound_row)
    for k in range(b["f"].shape[0]):
        p = AC.problem(b, k)
        el = EC.eliminate(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms, b["eq_rows"])
        W, act = AC.working_set(p["lam"], b["eq_rows"])
        gx, gl = pick(which, GX[k], GL[k])
        C = EC.cmat(p["A"], ms, n)
        dz, dnu = AC.route(el, act, gx, gl)
        rz, rnu = AC.dense(p["H"], C, W, gx, gl)
        ref = np.concatenate([rz, rnu])
        err = float(np.abs(np.concatenate([dz, dnu]) - ref).max() / np.abs(ref).max())
        cond = np.linalg.cond(AC.kkt_matrix(p["H"], C, W).astype(np.float64))
        print(shape, which, k, "err %.2e cond %.2e" % (err, cond))
        assert err <= cond * 2.0 ** -52, (k, err, cond)
        assert not dnu[np.setdiff1d(np.arange(m), W)].any()


@pytest.mark.parametrize("shape,lp,bound_row", CASES, ids=IDS)
def test_gradients_equal_central_differences(shape, lp, bound_row):
    """l = g_x'x + g_lam'lam at the planted working set (multipliers and slacks of at least 0.1: a step of 1e-6 keeps it).  The adjoint
    gives dl/df = -dz, dl/de = dnu_E (the equality right-hand side moves bupper and blower together), dl/dA_ij = -(lam_i dz_j + dnu_i
    x_j).  Central differences with h = 1e-6 on refined solves: truncation O(h^2), rounding 2^-64 / h -- far inside the bar of the
    layer's own gradcheck, atol 1e-5 + rtol 1e-4."""
    n, neq, m, ms = shape
    b, GX, GL = case(shape, lp, bound_row, N=1)
    p = AC.problem(b, 0)
    el = EC.eliminate(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms, b["eq_rows"])
    W, act = AC.working_set(p["lam"], b["eq_rows"])
    gx, gl = GX[0].astype(LD), GL[0].astype(LD)
    dz, dnu = AC.route(el, act, gx, gl)
    bW = AC.active_bounds(p, W).astype(LD)
    h = LD(1e-6)

    def loss(f=p["f"], A=p["A"], bW=bW):
        x, lam = AC.optimum(p["H"], f, EC.cmat(A, ms, n).astype(LD), W, bW)
        return gx @ x + gl @ lam

    x, lam = AC.optimum(p["H"], p["f"], EC.cmat(p["A"], ms, n).astype(LD), W, bW)
    assert np.abs(x - p["x"]).max() <= 1e-9 and np.abs(lam - p["lam"]).max() <= 1e-7      # the planted optimum
    rng = np.random.default_rng(7)
    checks = []
    for j in rng.choice(n, 2, replace=False):      # f
        d = np.zeros(n, dtype=LD)
        d[j] = h
        checks.append(("f[%d]" % j, (loss(f=p["f"] + d) - loss(f=p["f"] - d)) / (2 * h), -dz[j]))
    for c in (0, neq - 1):      # the right-hand side of an equality row
        d = np.zeros(len(W), dtype=LD)
        d[c] = h
        checks.append(("e[%d]" % c, (loss(bW=bW + d) - loss(bW=bW - d)) / (2 * h), dnu[b["eq_rows"][c]]))
    gen = [r for r in W if r >= ms]
    for r in (gen[0], gen[-1]):      # one entry of a general equality row and of an active kept row
        j = int(rng.integers(1, n))      # (column 0 of an equality row is kept zero where simple bound 0 is an equality as well)
        d = np.zeros(p["A"].shape, dtype=LD)
        d[r - ms, j] = h
        checks.append(("A[%d,%d]" % (r - ms, j), (loss(A=p["A"] + d) - loss(A=p["A"] - d)) / (2 * h), -(lam[r] * dz[j] + dnu[r] * x[j])))
    for name, fd, an in checks:
        print(shape, name, "fd %.9e adjoint %.9e" % (fd, an))
        assert abs(fd - an) <= 1e-5 + 1e-4 * abs(fd), (name, fd, an)


def test_entry_is_declared_and_exported():
    from daqp_amd import _lib
    with open(os.path.join(ROOT, "include", "daqp_amd.h")) as fh:
        header = fh.read()
    assert "int daqp_batch_eliminate_backward(DAQPBatchElimination *el, DAQPBatch *reduced," in header
    assert "daqp_batch_eliminate_backward" in _lib.EXPORTS


def test_entry_refuses_loudly():
    import daqp_amd
    from daqp_amd import _lib
    L = daqp_amd.lib()
    assert hasattr(L, "daqp_batch_eliminate_backward")
    assert L.daqp_batch_eliminate_backward(None, None, None, None, None, None, None, None, -1, 0) != 0      # refused, not dereferenced
    assert "no HIP device" in _lib.last_error() or "null" in _lib.last_error()
    assert hasattr(daqp_amd.EliminatedBatchModel, "backward")


def test_new_kernels_stay_in_registers():
    """no scratch and no spill at any NV (the figures are in DESIGN.md)"""
    from daqp_amd import _lib
    res = {k: v for k, v in _lib.kernel_resources().items() if k.startswith(("k_adjoint_reduce<", "k_adjoint_expand<"))}
    assert len(res) == 8, sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        assert v["lds"] == 64 * 8 * int(k.split("<")[1].split(">")[0]), (k, v)
