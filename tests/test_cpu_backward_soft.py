"""Soft rows in the adjoint, what can be checked without a GPU: the soft model itself against the reference library, the pure-torch
assembly of the q_k-dependence terms (daqp_amd.layer.soft_gradient_terms) against central differences of the dense system, the
exported entry point, and that the batches test_gpu_backward_soft.py runs are what it needs them to be."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _cases():
    spec = importlib.util.spec_from_file_location("backward_soft_cases", os.path.join(HERE, "backward_soft_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference():
    from oracle import oracle as O
    if not O.reference_available():
        pytest.skip("oracle/_ref is not built here (reference sources not present)")
    return O, O.Reference()


def _ref_solve(O, ref, q, k):
    S = _cases()
    H, Cm, f, bu, bl, sense = S.problem(q, k)
    st = O.default_settings(**q["settings"])
    x, lam, fval, flag, it = ref.quadprog(H, f, Cm[q["ms"]:], bu, bl, sense, settings=st)
    return H, Cm, f, bu, bl, sense, x, lam, flag


SOFT_MODEL_RTOL = 3e-13


def test_soft_model_pinned_against_the_reference():
    """On every active SOFT row of a reference solve:  c_k x - b_k = rho_soft (c_k H^-1 c_k') lam_k  with lam in the caller's units and
    b_k the bound the row is held at -- the relation daqp_batch_backward_soft differentiates.

    Tolerance: the residual |c_k x - b_k| the reference leaves on the ACTIVE HARD rows of the same solves, relative to
    max(1, |c_k x|), times ten.  Measured on these 5 x 48 solves: hard rows 2.76e-14 at worst -- so 3e-13 --, soft relation 1.89e-14
    at worst over 518 active soft rows."""
    S = _cases()
    O, ref = _reference()
    worst_hard = worst_soft = 0.0
    n_soft_rows = 0
    for name in ("one_wave", "cap_beyond_n1", "diag_h", "soft_equality", "shared"):
        q = S.PARITY[name]()
        for k in range(q["f"].shape[0]):
            H, Cm, f, bu, bl, sense, x, lam, flag = _ref_solve(O, ref, q, k)
            assert flag in (1, 2), (name, k, flag)
            cx = Cm @ x
            for i in np.nonzero(lam)[0]:
                b = bu[i] if lam[i] > 0 else bl[i]
                scale = max(1.0, abs(cx[i]))
                if sense[i] & S.SOFT:
                    qk = Cm[i] @ np.linalg.solve(H, Cm[i])
                    err = abs(cx[i] - b - S.RHO * qk * lam[i]) / scale
                    worst_soft = max(worst_soft, err)
                    n_soft_rows += 1
                    assert err <= SOFT_MODEL_RTOL, (name, k, i, err)
                    assert abs(cx[i] - b) > 1e-4, "an active soft row that is not violated tests nothing"
                else:
                    worst_hard = max(worst_hard, abs(cx[i] - b) / scale)
    print(f"hard rows: {worst_hard:.2e}, soft relation: {worst_soft:.2e}, over {n_soft_rows} active soft rows")
    assert n_soft_rows > 200


@pytest.mark.parametrize("name", ["one_wave", "cap_beyond_n1", "diag_h", "soft_equality", "shared", "workgroup", "hbm_scratch"])
def test_gpu_parity_batches_meet_their_conditions_on_the_reference(name):
    """what test_gpu_backward_soft.py asserts about its inputs, on the reference library alone: every problem ends OPTIMAL or
    SOFT_OPTIMAL, and at least half end SOFT_OPTIMAL with an active SOFT row"""
    S = _cases()
    O, ref = _reference()
    q = S.PARITY[name]()
    N = q["f"].shape[0]
    good, most = 0, 0
    for k in range(N):
        *_, sense, x, lam, flag = _ref_solve(O, ref, q, k)
        assert flag in (1, 2), (name, k, flag)
        good += int(flag == 2 and ((lam != 0) & ((sense & S.SOFT) != 0)).any())
        most = max(most, int((lam != 0).sum()))
    assert 2 * good >= N, (name, good, N)
    if name == "cap_beyond_n1":
        assert most > q["f"].shape[1] + 1, "no working set beyond n + 1 rows"


def test_no_soft_active_batch_on_the_reference():
    S = _cases()
    O, ref = _reference()
    q = S.NO_SOFT_ACTIVE()
    for k in range(q["f"].shape[0]):
        *_, sense, x, lam, flag = _ref_solve(O, ref, q, k)
        assert flag == 1 and not ((lam != 0) & ((sense & S.SOFT) != 0)).any(), k


def _fd_system(n=5, seed=4):
    """n = 5, three active rows (ids 0: a simple bound, 3 and 5: general rows), rows 3 and 0 SOFT -- so a soft simple bound and a soft
    general row next to a hard general row; working set fixed"""
    rng = np.random.default_rng(seed)
    ms, mA = 2, 5
    L = np.tril(rng.standard_normal((n, n)))
    H = L @ L.T + np.eye(n)
    return dict(H=H, f=rng.standard_normal(n), A=rng.standard_normal((mA, n)), b=rng.standard_normal(3), W=[3, 0, 5],
                soft=np.array([1.0, 1.0, 0.0]), rho=0.3, g=rng.standard_normal(n), ms=ms, mA=mA, n=n)


def _fd_solve(p, H, f, A, b, rho):
    n, ms, W = p["n"], p["ms"], p["W"]
    Cm = np.vstack([np.eye(n)[:ms], A])
    CW = Cm[W]
    q = np.einsum("kj,kj->k", CW, np.linalg.solve(H, CW.T).T)
    K = np.block([[H, CW.T], [CW, -np.diag(rho * q * p["soft"])]])
    sol = np.linalg.solve(K, np.concatenate([-f, b]))
    return sol[:n], sol[n:]


def test_soft_gradient_assembly_against_central_differences():
    """dl/dH, dl/df, dl/dA, dl/db and dl/drho_soft -- the adjoint's hard terms plus daqp_amd.layer.soft_gradient_terms on CPU tensors --
    against central differences (step 1e-6) of l = g'x, x from the dense system [H C_W'; C_W -S] [x; lam] = [-f; b_W] with the
    working set fixed.  H is perturbed symmetrically.  Tolerance 1e-8 of max(1, |gradient|_max): the rounding error of a central
    difference is about |l| 2^-52 / step = 2e-10 per unit of l, its truncation error step^2 = 1e-12 per unit of the third derivative;
    fifty times that.  Measured: 8.2e-10."""
    import torch
    from daqp_amd.layer import soft_gradient_terms
    S = _cases()
    p = _fd_system()
    n, ms, mA, W, rho, g = p["n"], p["ms"], p["mA"], p["W"], p["rho"], p["g"]
    m = ms + mA
    x, lamW = _fd_solve(p, p["H"], p["f"], p["A"], p["b"], rho)
    Cm = np.vstack([np.eye(n)[:ms], p["A"]])
    dz, dnuW, qW, U = S.dense_adjoint(p["H"], Cm, W, p["soft"], rho, g)
    assert np.abs(p["H"] @ dz + Cm[W].T @ dnuW - g).max() < 1e-12
    # what BatchModel.backward hands over for this problem: two slots more than soft rows, one of them between the used ones left out
    lam, dnu, qsoft = np.zeros(m), np.zeros(m), np.zeros(m)
    lam[W], dnu[W] = lamW, dnuW
    usoft, usoft_id = np.zeros((1, 4, n)), np.full((1, 4), -1, np.int32)
    for slot, k in enumerate(k for k in range(len(W)) if p["soft"][k]):
        qsoft[W[k]], usoft[0, slot], usoft_id[0, slot] = qW[k], U[k], W[k]
    t = lambda a: torch.tensor(a)
    terms = soft_gradient_terms(t(lam[None]), t(dnu[None]), t(qsoft[None]), t(usoft), t(usoft_id), rho, ms)
    gH = -0.5 * (np.outer(dz, x) + np.outer(x, dz)) + terms["dH"][0].numpy()
    gA = -(np.outer(lam[ms:], dz) + np.outer(dnu[ms:], x)) + terms["dA"][0].numpy()
    gf, gb, grho = -dz, dnuW, float(terms["drho"][0])
    assert np.abs(terms["dH"][0].numpy()).max() > 1e-3 and np.abs(terms["dA"][0].numpy()).max() > 1e-3 and abs(grho) > 1e-3
    assert not terms["dA"][0].numpy()[[0, 2, 3, 4]].any(), "only the soft general row of W (id 3: row 1 of A) gets a u term"

    eps = 1e-6
    loss = lambda H, f, A, b, r: float(g @ _fd_solve(p, H, f, A, b, r)[0])
    base = (p["H"], p["f"], p["A"], p["b"], rho)

    def fd(which, E):
        hi, lo = list(base), list(base)
        hi[which] = base[which] + eps * E
        lo[which] = base[which] - eps * E
        return (loss(*hi) - loss(*lo)) / (2 * eps)

    def unit(shape, idx):
        E = np.zeros(shape)
        E[idx] = 1.0
        return E

    worst = 0.0
    fdH = np.array([[fd(0, 0.5 * (unit((n, n), (i, j)) + unit((n, n), (j, i)))) for j in range(n)] for i in range(n)])
    fdf = np.array([fd(1, unit(n, i)) for i in range(n)])
    fdA = np.array([[fd(2, unit((mA, n), (i, j))) for j in range(n)] for i in range(mA)])
    fdb = np.array([fd(3, unit(3, i)) for i in range(3)])
    fdr = fd(4, 1.0)
    for name, got, want in (("H", gH, fdH), ("f", gf, fdf), ("A", gA, fdA), ("b", gb, fdb), ("rho", np.array(grho), np.array(fdr))):
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        worst = max(worst, err)
        assert err <= 1e-8, (name, err)
    print(f"max error against central differences: {worst:.2e}")
    # and without the q_k-dependence terms H and A are wrong: the terms are not a rounding matter
    assert np.abs(gH - terms["dH"][0].numpy() - fdH).max() > 1e-4 and np.abs(gA - terms["dA"][0].numpy() - fdA).max() > 1e-4


def test_backward_soft_symbol_declared_and_exported():
    import daqp_amd
    from daqp_amd import _lib
    L = daqp_amd.lib()
    assert "daqp_batch_backward_soft" in _lib.EXPORTS and hasattr(L, "daqp_batch_backward_soft")
    assert L.daqp_batch_backward_soft(None, None, None, None, None, None, None, None, None, 0) != 0      # refused, not dereferenced
    assert "null" in daqp_amd.last_error()
    with open(os.path.join(ROOT, "include", "daqp_amd.h")) as fh:
        header = fh.read()
    assert "int daqp_batch_backward_soft(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower," in header
    for words in ("S = diag(rho_soft q_k", "dl/drho_soft = sum_k dsig_k q_k", "rho_soft sum_k dsig_k u_k u_k'", "2 rho_soft dsig_i u_i'"):
        assert words in header, words
    import inspect
    from daqp_amd import layer
    sig = inspect.signature(layer.qp_layer)
    assert "sense" in sig.parameters and "rho_soft" in sig.parameters
