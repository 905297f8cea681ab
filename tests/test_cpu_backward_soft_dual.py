"""The soft-row adjoint with a dual right-hand side, what can be checked without a GPU: the gradient formulas of
tests/backward_soft_dual_cases.py (the ones qp_layer(..., soft_returns=True) applies) against central differences of the dense KKT
solve in np.longdouble at working sets taken from the reference library, that those working sets survive the perturbations the GPU
finite-difference test makes, and the new surface's signatures and refusals."""
import importlib.util
import inspect
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LD = np.longdouble
BATCHES = ["one_wave", "cap_beyond_n1", "diag_h", "soft_equality", "shared"]


def _cases():
    spec = importlib.util.spec_from_file_location("backward_soft_dual_cases", os.path.join(HERE, "backward_soft_dual_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference():
    from oracle import oracle as O
    if not O.reference_available():
        pytest.skip("oracle/_ref is not built here (reference sources not present)")
    return O, O.Reference()


def _working_set(O, ref, st, H, Cm, ms, f, bu, bl, sense):
    """(W ascending, upper side per row of W, x, lam, flag) of a reference solve"""
    x, lam, fval, flag, it = ref.quadprog(H, f, Cm[ms:], bu, bl, sense, settings=st)
    W = np.nonzero(lam)[0]
    return W, lam[W] > 0, x, lam, flag


def _entries(n, m, ms):
    """every single-entry perturbation of a problem: (name, index); H entries are symmetric pairs"""
    out = [("H", (i, j)) for i in range(n) for j in range(i, n)] + [("f", (i,)) for i in range(n)]
    out += [("A", (i, j)) for i in range(m - ms) for j in range(n)]
    out += [("bupper", (i,)) for i in range(m)] + [("blower", (i,)) for i in range(m)] + [("rho", ())]
    return out


@pytest.mark.parametrize("name", BATCHES)
def test_gradients_against_central_differences_in_longdouble(name):
    """Every gradient of l = a.x + b.lam + c fval + d soft_slack (random a, b, c, d per problem) from ONE adjoint solve with
    ghat_lam in its second block and the formulas of include/daqp_amd.h, against central differences (step 1e-6) of the dense solve
    of K [x; lam_W] = [-f; b_W] at the fixed working set and sides of the reference library, everything in np.longdouble (64-bit
    mantissa).  Perturbed one entry at a time: symmetric H, the rows of A, both bounds, f and rho.

    Tolerance 1e-7 relative to max(1, |gradient|_inf): the truncation error of the central difference is about step^2 O(1e2) =
    1e-10, its rounding error about 1e-19 / step = 1e-13."""
    C = _cases()
    O, ref = _reference()
    q = C.PARITY[name]()
    N, n = q["f"].shape
    m, ms, rho = q["bupper"].shape[1], q["ms"], q["settings"]["rho_soft"]
    st = O.default_settings(**q["settings"])
    wa, wb, wc, wd = C.weights(q)
    h = LD(C.FD_STEP)
    ents = _entries(n, m, ms)
    P = len(ents)
    worst, seen_soft, big = 0.0, 0, {}
    for k in range(N):
        H, Cm, f, bu, bl, sense = C.problem(q, k)
        W, upper, xr, lamr, flag = _working_set(O, ref, st, H, Cm, ms, f, bu, bl, sense)
        assert flag in (1, 2), (name, k, flag)
        is_soft = ((sense[W] & C.SOFT) != 0).astype(LD)
        seen_soft += int(is_soft.any())
        Hl, Cl, fl, bul, bll = (np.asarray(v, LD) for v in (H, Cm, f, bu, bl))
        a, b, c, d = wa[k].astype(LD), wb[k].astype(LD), LD(wc[k]), LD(wd[k])
        x, lamW, fval, slack = C.forward(Hl, Cl, W, upper, is_soft, LD(rho), fl, bul, bll)
        # the dense solve at that working set IS the reference's optimum (the model of tests/test_cpu_backward_soft.py)
        assert np.abs(np.asarray(x, float) - xr).max() <= 1e-9 * max(1.0, np.abs(xr).max()), (name, k)
        assert np.abs(np.asarray(lamW, float) - lamr[W]).max() <= 1e-8 * max(1.0, np.abs(lamr).max()), (name, k)
        got = C.gradients(Hl, Cl, ms, W, upper, is_soft, LD(rho), x, lamW, a, b, c, d)
        # all 2 P perturbed problems at once
        Hs, Cs, fs = np.tile(Hl, (2 * P, 1, 1)), np.tile(Cl, (2 * P, 1, 1)), np.tile(fl, (2 * P, 1))
        bus, bls, rhos = np.tile(bul, (2 * P, 1)), np.tile(bll, (2 * P, 1)), np.full(2 * P, rho, LD)
        for p, (what, idx) in enumerate(ents):
            for row, sgn in ((2 * p, h), (2 * p + 1, -h)):
                if what == "H":
                    i, j = idx
                    Hs[row, i, j] += 0.5 * sgn
                    Hs[row, j, i] += 0.5 * sgn
                elif what == "f":
                    fs[row, idx[0]] += sgn
                elif what == "A":
                    Cs[row, ms + idx[0], idx[1]] += sgn
                elif what == "bupper":
                    bus[row, idx[0]] += sgn
                elif what == "blower":
                    bls[row, idx[0]] += sgn
                else:
                    rhos[row] += sgn
        xs, ls, fv, sl = C.forward(Hs, Cs, W, upper, is_soft, rhos, fs, bus, bls)
        loss = xs @ a + ls @ b[W] + c * fv + d * sl
        fd = (loss[0::2] - loss[1::2]) / (2 * h)
        want = dict(H=np.zeros((n, n), LD), f=np.zeros(n, LD), A=np.zeros((m - ms, n), LD), bupper=np.zeros(m, LD), blower=np.zeros(m, LD),
                    rho=np.zeros((), LD))
        for p, (what, idx) in enumerate(ents):
            want[what][idx] = fd[p]
            if what == "H":
                want["H"][idx[::-1]] = fd[p]
        for key in want:
            err = float(np.abs(np.asarray(got[key]) - want[key]).max() / max(1.0, float(np.abs(np.asarray(got[key])).max())))
            worst = max(worst, err)
            assert err <= 1e-7, (name, k, key, err)
        big = {key: max(big.get(key, 0.0), float(np.abs(np.asarray(got[key])).max())) for key in got}
    print(f"{name}: worst error against central differences {worst:.2e}; problems with an active SOFT row: {seen_soft}")
    assert 2 * seen_soft >= N, "the soft terms are not exercised"
    assert all(v > 1e-3 for v in big.values()), big      # no gradient of the batch is trivially zero


@pytest.mark.parametrize("name", BATCHES)
def test_working_sets_survive_the_finite_difference_step(name):
    """On the reference library: a perturbation of +-1e-6 in any ONE input entry (H symmetric, f, A, both bounds, rho_soft) leaves the
    working set and its sides unchanged for at least 90 % of the batch's problems -- and so does the direction the GPU test's
    end-to-end central difference takes (backward_soft_dual_cases.fd_direction: f and bupper together, no entry moved by more than
    the step).  This is what allows that test to skip at most 10 % of its problems."""
    C = _cases()
    O, ref = _reference()
    q = C.PARITY[name]()
    N, n = q["f"].shape
    m, ms = q["bupper"].shape[1], q["ms"]
    h = C.FD_STEP
    Ef, Eb = C.fd_direction(q)
    stable = stable_dir = 0
    for k in range(N):
        H, Cm, f, bu, bl, sense = C.problem(q, k)
        st = O.default_settings(**q["settings"])
        W, upper, *_ = _working_set(O, ref, st, H, Cm, ms, f, bu, bl, sense)

        def same(H=H, Cm=Cm, f=f, bu=bu, bl=bl, st=st):
            W2, up2, _, _, flag = _working_set(O, ref, st, H, Cm, ms, f, bu, bl, sense)
            return flag in (1, 2) and np.array_equal(W, W2) and np.array_equal(upper, up2)

        ok = True
        for what, idx in _entries(n, m, ms):
            for sgn in (h, -h):
                if what == "rho":
                    ok = ok and same(st=O.default_settings(**{**q["settings"], "rho_soft": q["settings"]["rho_soft"] + sgn}))
                    continue
                arr = dict(H=H, f=f, A=Cm, bupper=bu, blower=bl)[what].copy()
                if what == "H":
                    i, j = idx
                    arr[i, j] += 0.5 * sgn
                    arr[j, i] += 0.5 * sgn
                elif what == "A":
                    arr[ms + idx[0], idx[1]] += sgn
                else:
                    arr[idx] += sgn
                ok = ok and same(**{dict(H="H", f="f", A="Cm", bupper="bu", blower="bl")[what]: arr})
            if not ok:
                break
        stable += int(ok)
        stable_dir += int(same(f=f + h * Ef[k], bu=bu + h * Eb[k]) and same(f=f - h * Ef[k], bu=bu - h * Eb[k]))
    print(f"{name}: working set unchanged under every single-entry step for {stable} of {N} problems, under the GPU test's direction for {stable_dir}")
    assert 10 * stable >= 9 * N and 10 * stable_dir >= 9 * N, (name, stable, stable_dir, N)


def test_new_surface_signatures_and_refusals_without_a_gpu():
    import torch
    import daqp_amd
    from daqp_amd import _lib, layer
    L = daqp_amd.lib()
    assert "daqp_batch_backward_soft_dual" in _lib.EXPORTS and hasattr(L, "daqp_batch_backward_soft_dual")
    assert L.daqp_batch_backward_soft_dual(*([None] * 12), 0) != 0      # refused, not dereferenced
    assert "null" in daqp_amd.last_error()
    with open(os.path.join(ROOT, "include", "daqp_amd.h")) as fh:
        header = fh.read()
    assert "int daqp_batch_backward_soft_dual(DAQPBatch *b, const c_float *grad_x" in header
    for words in ("const c_float *grad_slack", "ghat_lam[k] = g_lam[WS[k]] + 2 g_s rho_soft q_k lam_k", "dnu_k lam_k - 1/2 g_f lam_k^2 + g_s lam_k^2",
                  "soft_slack = sum_k S_k lam_k^2", "fval = 1/2 x'Hx + f'x + 1/2 soft_slack"):
        assert words in header, words
    sig = inspect.signature(layer.qp_layer)
    assert sig.parameters["soft_returns"].default is False
    assert inspect.signature(layer.soft_gradient_terms).parameters["dsig_extra"].default is None
    bs = inspect.signature(daqp_amd.BatchModel.backward_soft).parameters
    assert list(bs)[1:] == ["grad_x", "grad_lam", "grad_slack", "lam", "out"] and bs["out"].default == "torch"
    assert all(bs[k].default is None for k in ("grad_x", "grad_lam", "grad_slack", "lam"))
    # "soft_slack" is a name of soft_returns=True only; both refusals come before anything touches a device
    t = lambda *s: torch.zeros(*s, dtype=torch.float64)
    H, f, A, bu = torch.eye(3, dtype=torch.float64).expand(2, 3, 3), t(2, 3), t(2, 2, 3), t(2, 2)
    for returns in ("soft_slack", ("x", "soft_slack")):
        with pytest.raises(ValueError, match="returns"):
            daqp_amd.qp_layer(H, f, A, bu, returns=returns)
    with pytest.raises(ValueError, match="returns"):
        daqp_amd.qp_layer(H, f, A, bu, returns=("x", "slack"), soft_returns=True)
    with pytest.raises(ValueError, match="soft_returns"):
        daqp_amd.qp_layer(H, f, A, bu, returns="soft_slack", soft_returns=True, nullspace=True)
    with pytest.raises(ValueError, match="soft_returns"):
        daqp_amd.qp_layer(H, f, A, bu, returns="soft_slack", soft_returns=True, eq_rows=[0])


def test_soft_gradient_terms_unchanged_without_dsig_extra_and_linear_in_it():
    """dsig_extra = None gives the bits of the call without it; a dsig_extra shifts the three outputs by the terms of dsig_extra alone"""
    import torch
    from daqp_amd.layer import soft_gradient_terms
    g = torch.Generator().manual_seed(5)
    N, m, ms, ns, n = 3, 7, 2, 3, 4
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    lam, dnu, usoft = r(N, m), r(N, m), r(N, ns, n)
    ids = torch.tensor([[1, 4, -1], [5, -1, -1], [0, 3, 6]], dtype=torch.int32)
    qsoft = torch.zeros(N, m, dtype=torch.float64)
    for k in range(N):
        for i in ids[k][ids[k] >= 0]:
            qsoft[k, int(i)] = 1.0 + float(i)
    usoft = usoft * (ids >= 0)[:, :, None]
    base = soft_gradient_terms(lam, dnu, qsoft, usoft, ids, 0.3, ms)
    again = soft_gradient_terms(lam, dnu, qsoft, usoft, ids, 0.3, ms, dsig_extra=None)
    ref = dict(dH=-torch.einsum("qsi,qsj->qij", (0.3 * torch.gather(dnu * lam, 1, ids.clamp(min=0).long()) * (ids >= 0))[:, :, None] * usoft, usoft),
               drho=(dnu * lam * qsoft).sum(1))
    for key in base:
        assert torch.equal(base[key], again[key]), key
    assert torch.equal(base["dH"], ref["dH"]) and torch.equal(base["drho"], ref["drho"])      # the expressions of the parent commit
    extra = r(N, m)
    both = soft_gradient_terms(lam, dnu, qsoft, usoft, ids, 0.3, ms, dsig_extra=extra)
    only = soft_gradient_terms(lam, torch.zeros_like(dnu), qsoft, usoft, ids, 0.3, ms, dsig_extra=extra)
    for key in base:
        assert (both[key] - base[key] - only[key]).abs().max() <= 1e-14 * max(1.0, float(both[key].abs().max())), key
        assert only[key].abs().max() > 0, key
