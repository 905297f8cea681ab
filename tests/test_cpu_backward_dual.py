"""daqp_batch_backward_dual, what can be checked without a GPU: a numpy statement of its contract -- the dense solve of
K [dz; dnu] = [g_x; g_lamW], the five gradient formulas (unchanged) and the four objective formulas -- against central differences of
a dense fixed-W KKT solve, for losses l = a'x + c'lam + d fval on planted problems; and that the entry point is declared, exported and
reachable from Python.  This pins the signs: lam is signed (> 0 at an upper bound, < 0 at a lower one), the rows of C_W are not."""
import inspect
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---------------------------------------------------------------------------------------------------------------------------
# the contract, in numpy
# ---------------------------------------------------------------------------------------------------------------------------
def kkt(H, A, ms, W):
    n = H.shape[0]
    Cm = np.vstack([np.eye(n)[:ms], A])
    CW = Cm[W]
    return np.block([[H, CW.T], [CW, np.zeros((len(W), len(W)))]]), Cm


def fixed_w_solve(H, f, A, ms, W, bW):
    """(x, lam on W, fval) of  H x + f + C_W' lam_W = 0,  C_W x = b_W"""
    n = f.size
    K, _ = kkt(H, A, ms, W)
    sol = np.linalg.solve(K, np.concatenate([-f, bW]))
    x = sol[:n]
    return x, sol[n:], 0.5 * x @ H @ x + f @ x


def dual_adjoint(H, A, ms, W, g_x, g_lam):
    """what daqp_batch_backward_dual returns for one problem: (dz, dnu on W) of K [dz; dnu] = [g_x; g_lam[W]]"""
    n = g_x.size
    K, _ = kkt(H, A, ms, W)
    sol = np.linalg.solve(K, np.concatenate([g_x, g_lam[W]]))
    return sol[:n], sol[n:]


def gradients(H, A, ms, W, x, lam, g_x, g_lam, g_fval):
    """dl/dH, dl/df, dl/dA, dl/db (m-vector: the bound each row of W sits at) of a loss with upstream gradients g_x, g_lam, g_fval"""
    m = ms + A.shape[0]
    dz, dnuW = dual_adjoint(H, A, ms, W, g_x, g_lam)
    dnu = np.zeros(m)
    dnu[W] = dnuW
    # the five formulas of daqp_batch_backward, unchanged (dbupper / dblower are dnu split by side)
    gH = -0.5 * (np.outer(dz, x) + np.outer(x, dz))
    gf = -dz
    gA = -(np.outer(lam[ms:], dz) + np.outer(dnu[ms:], x))
    gb = dnu.copy()
    # the objective: fval = 1/2 x'Hx + f'x, envelope theorem, no solve
    gf = gf + g_fval * x
    gH = gH + 0.5 * g_fval * np.outer(x, x)
    gb = gb - g_fval * lam
    gA = gA + g_fval * np.outer(lam[ms:], x)
    return gH, gf, gA, gb


# ---------------------------------------------------------------------------------------------------------------------------
# planted problems: the construction of _planted in tests/test_gpu_backward.py
# ---------------------------------------------------------------------------------------------------------------------------
def planted(seed, n=4, mA=6, ms=2):
    """simple bound 0 held at its upper side, general row 3 (constraint 5) at its lower side, multipliers +-0.5; every other row has
    0.5 of slack on both sides"""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.standard_normal((n, n)))
    A = rng.standard_normal((mA, n))
    H = L @ L.T + np.eye(n)
    xs = rng.standard_normal(n)
    Cm = np.vstack([np.eye(n)[:ms], A])
    cx = Cm @ xs
    lam = np.zeros(ms + mA)
    lam[0], lam[5] = 0.5, -0.5
    f = -(H @ xs + Cm.T @ lam)
    bu, bl = cx + 0.5, cx - 0.5
    bu[0], bl[0] = cx[0], cx[0] - 1.0
    bl[5], bu[5] = cx[5], cx[5] + 1.0
    return dict(H=H, f=f, A=A, bupper=bu, blower=bl, x=xs, lam=lam, W=np.array([0, 5]), lower=np.array([False, True]), ms=ms)


@pytest.mark.parametrize("seed", [2, 3, 4])
@pytest.mark.parametrize("weights", ["x", "lam", "fval", "all"])
def test_contract_against_central_differences(seed, weights):
    """Tolerance 1e-8 of max(1, |gradient|_max), as in test_cpu_backward_nullspace.py: the rounding error of a central difference with
    step 1e-6 is about |l| 2^-52 / step = 2e-10 per unit of l, fifty times that; its truncation error is of order step^2."""
    p = planted(seed)
    H, f, A, ms, W = p["H"], p["f"], p["A"], p["ms"], p["W"]
    n, m, mA = f.size, p["lam"].size, A.shape[0]
    bW = np.where(p["lower"], p["blower"][W], p["bupper"][W])
    x, lamW, fval = fixed_w_solve(H, f, A, ms, W, bW)
    lam = np.zeros(m)
    lam[W] = lamW
    # the planted optimum is what the fixed-W system gives, with the margins the construction promises
    assert np.abs(x - p["x"]).max() < 1e-12 and np.abs(lam - p["lam"]).max() < 1e-12
    assert np.abs(lam[W]).min() >= 1e-3 and (lam[W][p["lower"]] < 0).all() and (lam[W][~p["lower"]] > 0).all()
    _, Cm = kkt(H, A, ms, W)
    off = np.ones(m, bool)
    off[W] = False
    assert min((p["bupper"] - Cm @ x)[off].min(), (Cm @ x - p["blower"])[off].min()) >= 0.01
    rng = np.random.default_rng([seed, 99])
    a, c, d = rng.standard_normal(n), rng.standard_normal(m), float(rng.standard_normal())
    if weights == "x":
        c, d = np.zeros(m), 0.0
    elif weights == "lam":
        a, d = np.zeros(n), 0.0
    elif weights == "fval":
        a, c = np.zeros(n), np.zeros(m)
    gH, gf, gA, gb = gradients(H, A, ms, W, x, lam, a, c, d)
    assert not gb[off].any() and not gA[[i - ms for i in range(ms, m) if off[i]]].any(), "a row off W has no gradient"

    def loss(Hh, ff, AA, bb):
        xx, ll, fv = fixed_w_solve(Hh, ff, AA, ms, W, bb)
        return float(a @ xx + c[W] @ ll + d * fv)

    eps = 1e-6
    base = (H, f, A, bW)

    def fd(which, E):
        hi, lo = list(base), list(base)
        hi[which] = base[which] + eps * E
        lo[which] = base[which] - eps * E
        return (loss(*hi) - loss(*lo)) / (2 * eps)

    def unit(shape, idx):
        E = np.zeros(shape)
        E[idx] = 1.0
        return E

    fdf = np.array([fd(1, unit(n, i)) for i in range(n)])
    fdb = np.array([fd(3, unit(len(W), i)) for i in range(len(W))])
    fdH = np.array([[fd(0, 0.5 * (unit((n, n), (i, j)) + unit((n, n), (j, i)))) for j in range(n)] for i in range(n)])
    fdA = np.array([[fd(2, unit((mA, n), (i, j))) for j in range(n)] for i in range(mA)])
    worst = 0.0
    for what, got, want in (("f", gf, fdf), ("b", gb[W], fdb), ("H", gH, fdH), ("A", gA, fdA)):
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        worst = max(worst, err)
        assert err <= 1e-8, (seed, weights, what, err)
    if weights != "x":
        assert max(np.abs(fdf).max(), np.abs(fdb).max()) > 1e-3, "the loss does not move: nothing was checked"
    print(f"seed {seed}, loss weights on {weights}: max error against central differences: {worst:.2e}")


def test_a_vertex_moves_with_the_multipliers():
    """n rows in W (an LP vertex, H = 0): dz = 0 for g_lam = 0 and dz = C_W^-1 g_lamW otherwise -- x does not move with f, but the loss
    through lam moves with b"""
    rng = np.random.default_rng(5)
    n = 3
    A = rng.standard_normal((n, n))
    W = np.arange(n)
    g_x, g_lam = rng.standard_normal(n), rng.standard_normal(n)
    dz0, _ = dual_adjoint(np.zeros((n, n)), A, 0, W, g_x, np.zeros(n))
    dz1, dnu1 = dual_adjoint(np.zeros((n, n)), A, 0, W, g_x, g_lam)
    assert np.abs(dz0).max() <= 1e-14 * np.abs(g_x).max()
    assert np.abs(dz1 - np.linalg.solve(A, g_lam)).max() <= 1e-12 * np.abs(dz1).max() and np.abs(dz1).max() > 1e-2
    assert np.abs(A.T @ dnu1 - g_x).max() <= 1e-12 * np.abs(dnu1).max()


# ---------------------------------------------------------------------------------------------------------------------------
# the entry point
# ---------------------------------------------------------------------------------------------------------------------------
def test_dual_entry_declared_exported_and_reachable():
    from daqp_amd import _lib
    with open(os.path.join(ROOT, "include", "daqp_amd.h")) as fh:
        header = fh.read()
    assert "int daqp_batch_backward_dual(DAQPBatch *b, const c_float *grad_x" in header
    assert "const c_float *grad_lam" in header
    for words in ("THE FIVE GRADIENT FORMULAS ARE UNCHANGED", "(N_W N_W') dnu = N_W w - g_lamW", "dl/dH += 1/2 g_fval x x'", "dl/dA_i += g_fval lam_i x'",
                  "Not built: soft rows", "soft_slack gradients", "Jacobians and multi-RHS solves", "EliminatedBatchModel", "MultiBatchModel"):
        assert words in header, words
    assert "Not differentiated: lam, fval. */" not in header      # daqp_batch_backward's comment points to the new entry instead
    assert "daqp_batch_backward_dual" in _lib.EXPORTS
    if not os.path.exists(_lib.LIBPATH):      # the export half needs a built library
        return
    import daqp_amd
    from daqp_amd.api import BatchModel
    L = daqp_amd.lib()
    assert hasattr(L, "daqp_batch_backward_dual")
    assert L.daqp_batch_backward_dual(None, None, None, None, None, None, None, -1, 0) != 0      # refused, not dereferenced
    assert "null" in daqp_amd.last_error()
    assert inspect.signature(BatchModel.backward).parameters["grad_lam"].default is None
    res = [k for k in _lib.kernel_resources() if k.startswith("k_backward")]
    if res:      # three mappings of the Gram route and the null-space kernel, each with a dual right-hand side
        assert len([k for k in res if k.startswith("k_backward<") and k.endswith(", true>")]) >= 3, res
        assert "k_backward_nullspace<64, true>" in res, res


def test_layer_takes_returns():
    import torch
    from daqp_amd import layer
    assert inspect.signature(layer.qp_layer).parameters["returns"].default == "x"
    z = torch.zeros(1, 2, dtype=torch.float64)
    for bad in ("y", (), ("x", "x"), ("x", "slack")):
        with pytest.raises(ValueError, match="returns"):
            layer.qp_layer(torch.eye(2, dtype=torch.float64)[None], z, None, z + 1, z - 1, ms=2, returns=bad)
    with pytest.raises(ValueError, match="SOFT"):
        layer.qp_layer(torch.eye(2, dtype=torch.float64)[None], z, None, z + 1, z - 1, ms=2, returns="lam", sense=torch.tensor([8, 0]))
