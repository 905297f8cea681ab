"""The dense oracle and the gradient formulas of the soft-row adjoint with a dual right-hand side (daqp_batch_backward_soft_dual,
BatchModel.backward_soft, qp_layer(..., soft_returns=True)); the batches are those of tests/backward_soft_cases.py.  numpy only; no
test in this file.  test_cpu_backward_soft_dual.py holds gradients() to central differences in np.longdouble;
test_gpu_backward_soft_dual.py holds the GPU to dense_adjoint_dual() and the layer to gradients().

Everything here works in the dtype it is given: np.float64 goes through LAPACK, np.longdouble (which numpy.linalg does not take)
through ld_solve below."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("backward_soft_cases_for_dual", os.path.join(os.path.dirname(os.path.abspath(__file__)), "backward_soft_cases.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

PARITY, NO_SOFT_ACTIVE, problem, SOFT, RHO = S.PARITY, S.NO_SOFT_ACTIVE, S.problem, S.SOFT, S.RHO
FD_STEP = 1e-6


def ld_solve(K, R):
    """K^-1 R for K (..., k, k), R (..., k, p) in the dtype of K: Gaussian elimination WITHOUT pivoting, batched over the leading
    axes.  For the matrices of this file only -- H positive definite and K = [H C'; C -S] with C of full row rank or S > 0 on the
    dependent rows: quasi-definite, so every pivot is a pivot of a definite Schur complement and no row exchange is needed."""
    K, R = np.array(K), np.array(R)
    k = K.shape[-1]
    for c in range(k):
        piv = K[..., c, c]
        l = K[..., c + 1:, c] / piv[..., None]
        K[..., c + 1:, c:] -= l[..., :, None] * K[..., c, None, c:]
        R[..., c + 1:, :] -= l[..., :, None] * R[..., c, None, :]
    for c in range(k - 1, -1, -1):
        R[..., c, :] = (R[..., c, :] - np.einsum("...j,...jp->...p", K[..., c, c + 1:], R[..., c + 1:, :])) / K[..., c, c, None]
    return R


def solve(K, R):
    return ld_solve(K, R) if K.dtype == np.longdouble else np.linalg.solve(K, R)


def kkt(H, CW, is_soft, rho):
    """(K, q, U): K = [H C_W'; C_W -S], q_k = c_k H^-1 c_k', U with rows u_k = H^-1 c_k'; batched over leading axes"""
    n, na = H.shape[-1], CW.shape[-2]
    U = np.swapaxes(solve(H, np.swapaxes(CW, -1, -2)), -1, -2)
    qk = (CW * U).sum(-1)
    K = np.zeros(H.shape[:-2] + (n + na, n + na), H.dtype)
    K[..., :n, :n] = H
    K[..., :n, n:] = np.swapaxes(CW, -1, -2)
    K[..., n:, :n] = CW
    idx = np.arange(na)
    K[..., n + idx, n + idx] = -(rho * qk * is_soft)
    return K, qk, U


def dense_adjoint_dual(H, C, W, is_soft, rho, lam_W, g_x, g_lamW, g_s):
    """K [dz; dnu] = [g_x; ghat_lamW] by a dense solve, K = [H C_W'; C_W -S], S = diag(rho q_k on the SOFT rows of W), ghat_lam_k =
    g_lam_k + 2 g_s rho q_k lam_k on those rows; returns (dz, dnu_W, q_W, U) like backward_soft_cases.dense_adjoint"""
    n = H.shape[0]
    K, qk, U = kkt(H, C[W], is_soft, rho)
    ghat = g_lamW + 2.0 * g_s * rho * qk * lam_W * is_soft
    sol = solve(K, np.concatenate([g_x, ghat])[:, None])[:, 0]
    return sol[:n], sol[n:], qk, U


def forward(H, C, W, upper, is_soft, rho, f, bupper, blower):
    """the optimum at a FIXED working set W with its sides (upper[k]: row W[k] is held at bupper), batched over leading axes of every
    argument but W, upper and is_soft: x, lam_W, fval, soft_slack as tests/kkt_reference.py defines them"""
    n = H.shape[-1]
    CW = C[..., W, :]
    K, qk, _ = kkt(H, CW, is_soft, rho[..., None] if np.ndim(rho) else rho)
    bW = np.where(upper, bupper[..., W], blower[..., W])
    sol = solve(K, np.concatenate([-f, bW], axis=-1)[..., None])[..., 0]
    x, lamW = sol[..., :n], sol[..., n:]
    slack = ((rho[..., None] if np.ndim(rho) else rho) * qk * lamW * lamW * is_soft).sum(-1)
    fval = 0.5 * np.einsum("...i,...ij,...j->...", x, H, x) + (f * x).sum(-1) + 0.5 * slack
    return x, lamW, fval, slack


def gradients(H, C, ms, W, upper, is_soft, rho, x, lam_W, a, b, c, d):
    """every gradient of  l = a.x + b.lam + c fval + d soft_slack  (a (n,), b (m,), c, d scalars) at the working set W, from one
    adjoint solve and the formulas of include/daqp_amd.h: dict(f (n,), H (n, n) -- the symmetric gradient: the change of l per unit
    of a symmetric perturbation E is sum(H_grad * E) --, A (m - ms, n), bupper (m,), blower (m,), rho scalar)"""
    n, m = H.shape[0], C.shape[0]
    W = np.asarray(W, int)
    dz, dnuW, qk, U = dense_adjoint_dual(H, C, W, is_soft, rho, lam_W, a, b[W], d)
    lam, dnu = np.zeros(m, H.dtype), np.zeros(m, H.dtype)
    lam[W], dnu[W] = lam_W, dnuW
    # the five formulas
    gf = -dz
    gH = -0.5 * (np.outer(dz, x) + np.outer(x, dz))
    gC = -(np.outer(lam, dz) + np.outer(dnu, x))
    gbu, gbl = np.zeros(m, H.dtype), np.zeros(m, H.dtype)
    gbu[W[upper]], gbl[W[~upper]] = dnuW[upper], dnuW[~upper]
    # the S-dependence: dsig_k = dl/dS_k, S_k = rho q_k, dq_k = 2 u_k.dc_k - u_k' dH u_k
    dsig = (dnuW * lam_W - 0.5 * c * lam_W * lam_W + d * lam_W * lam_W) * is_soft
    grho = (dsig * qk).sum()
    gH = gH - rho * np.einsum("k,ki,kj->ij", dsig, U, U)
    gC[W] += 2.0 * rho * dsig[:, None] * U
    # the envelope terms of fval
    gf = gf + c * x
    gH = gH + 0.5 * c * np.outer(x, x)
    gC = gC + c * np.outer(lam, x)
    gbu[W[upper]] -= c * lam_W[upper]
    gbl[W[~upper]] -= c * lam_W[~upper]
    return dict(f=gf, H=gH, A=gC[ms:], bupper=gbu, blower=gbl, rho=grho)


def weights(q, seed=31):
    """random a (N, n), b (N, m), c (N,), d (N,) of the linear loss"""
    N, n = q["f"].shape
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, n)), rng.standard_normal((N, q["bupper"].shape[1])), rng.standard_normal(N), rng.standard_normal(N)


def fd_direction(q, seed=37):
    """the direction of the end-to-end central difference of test_gpu_backward_soft_dual.py: E_f (N, n), E_bupper (N, m), entries in
    [-1, 1], so that a step of FD_STEP moves no entry by more than FD_STEP"""
    N, n = q["f"].shape
    rng = np.random.default_rng(seed)
    return 2.0 * rng.random((N, n)) - 1.0, 2.0 * rng.random((N, q["bupper"].shape[1])) - 1.0
