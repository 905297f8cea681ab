"""The adjoint of an eliminated problem in numpy -- the reference of tests/test_cpu_eliminate_backward.py and
tests/test_gpu_eliminate_backward.py -- on top of eliminate_cases.eliminate, next to a dense solve of the full KKT system.

Notation of include/daqp_amd.h (daqp_batch_eliminate_backward): E = C_eq_rows with unit-row QR E' = Q [R; 0], Q = [Q1 Z], row norms s;
I the kept rows; W_I the active kept rows.  For g_x, g_lam

    reduce    y = R^-T (g_lam_E / s),  dz0 = Q1 y,  grad_y = Z'(g_x - H dz0),  grad_lam_r = g_lam_I - C_I dz0
    solve     [H_r A_rW'; A_rW 0] [dz_r; dnu_I] = [grad_y; grad_lam_r on W_I]
    expand    dz = dz0 + Z dz_r,  R dnu~ = Q1'(g_x - H dz - C_WI' dnu_I),  dnu_E = dnu~ / s

Every product is np.longdouble; a linear solve is LU in fp64 followed by two steps of refinement on longdouble residuals, so that the
error of a reference is that of its products, not cond(K) 2^-53."""
import numpy as np

import eliminate_cases as EC

LD = np.longdouble


def solve_refined(K, rhs, steps=2):
    """K^-1 rhs (K, rhs longdouble): fp64 LU, `steps` corrections on longdouble residuals"""
    K, rhs = np.asarray(K, dtype=LD), np.asarray(rhs, dtype=LD)
    if K.shape[0] == 0:
        return np.zeros(0, dtype=LD)
    K64 = K.astype(np.float64)
    x = np.linalg.solve(K64, rhs.astype(np.float64)).astype(LD)
    for _ in range(steps):
        x = x + np.linalg.solve(K64, (rhs - K @ x).astype(np.float64)).astype(LD)
    return x


def working_set(lam, eq_rows):
    """(W, W_I): the rows with a multiplier, equality rows first, then the active kept rows in ascending order"""
    eq = np.asarray(eq_rows)
    act = np.setdiff1d(np.flatnonzero(np.asarray(lam) != 0.0), eq)
    return np.concatenate([eq, act]), act


def kkt_matrix(H, C, W):
    n, k = C.shape[1], len(W)
    K = np.zeros((n + k, n + k), dtype=LD)
    if H is not None:
        K[:n, :n] = H
    K[:n, n:] = C[W].T
    K[n:, :n] = C[W]
    return K


def dense(H, C, W, g_x, g_lam):
    """(dz (n), dnu (m, zero off W)) of the full system K [dz; dnu_W] = [g_x; g_lam_W], solved densely"""
    n, m = C.shape[1], C.shape[0]
    rhs = np.concatenate([np.zeros(n) if g_x is None else g_x, np.zeros(len(W)) if g_lam is None else np.asarray(g_lam)[W]]).astype(LD)
    s = solve_refined(kkt_matrix(H, C, W), rhs)
    dnu = np.zeros(m, dtype=LD)
    dnu[W] = s[n:]
    return s[:n], dnu


def route(el, act, g_x, g_lam):
    """the same (dz, dnu) by reduce -> solve -> expand on el = eliminate_cases.eliminate(...); act: the active kept rows (original ids)"""
    n, m, kept, eq = el["n"], el["m"], el["kept"], el["eq"]
    F = el["full"]
    H = None if F["H"] is None else np.asarray(F["H"], dtype=np.float64).astype(LD)
    C = F["C"].astype(LD)
    Q1, Z, R, s = el["Q1"].astype(LD), el["Z"].astype(LD), el["R"].astype(LD), el["norms"].astype(LD)
    gx = np.zeros(n, dtype=LD) if g_x is None else np.asarray(g_x).astype(LD)
    Hmul = (lambda v: np.zeros(n, dtype=LD)) if H is None else (lambda v: H @ v)
    # reduce
    if g_lam is None:
        dz0 = np.zeros(n, dtype=LD)
        glr = np.zeros(kept.size, dtype=LD)
    else:
        gl = np.asarray(g_lam).astype(LD)
        dz0 = Q1 @ EC._tri_solve_lower(R.T, gl[eq] / s)
        glr = gl[kept] - C[kept] @ dz0
    gy = Z.T @ (gx - Hmul(dz0))
    # solve the reduced system at W_I
    pos = np.searchsorted(kept, act)      # positions of the active rows among the kept ones
    nr = n - eq.size
    Hr = np.zeros((nr, nr), dtype=LD) if H is None else Z.T @ H @ Z
    Ar = C[kept] @ Z
    sol = solve_refined(kkt_matrix(Hr, Ar, pos), np.concatenate([gy, glr[pos]]))
    dzr, dnuI = sol[:nr], sol[nr:]
    # expand
    dz = dz0 + Z @ dzr
    dnu = np.zeros(m, dtype=LD)
    dnu[act] = dnuI
    dnu[eq] = EC._tri_solve_upper(R, Q1.T @ (gx - Hmul(dz) - C[act].T @ dnuI)) / s
    return dz, dnu


def optimum(H, f, C, W, b_W):
    """(x, lam (m)) of the equality-constrained problem at a fixed working set: K [x; lam_W] = [-f; b_W]"""
    n, m = C.shape[1], C.shape[0]
    s = solve_refined(kkt_matrix(H, C, W), np.concatenate([-np.asarray(f), b_W]).astype(LD))
    lam = np.zeros(m, dtype=LD)
    lam[W] = s[n:]
    return s[:n], lam


def active_bounds(p, W):
    """b_W of a planted problem: bupper where the multiplier is positive (and on the equality rows), blower where it is negative"""
    return np.where(p["lam"][W] > 0, p["bupper"][W], p["blower"][W])


def problem(b, k):
    """problem k of a make_batch dict: dict(H, f, A, bupper, blower, sense, x, lam)"""
    return {key: (None if b[key] is None else b[key][k]) for key in ("H", "f", "A", "bupper", "blower", "sense", "x", "lam")}
