"""Equality elimination in numpy -- the reference of tests/test_cpu_eliminate.py and tests/test_gpu_eliminate.py -- and their cases.

With C = [first ms rows of I; A], E = C[eq_rows], e = bupper[eq_rows], I the other rows in their order (include/daqp_amd.h,
daqp_batch_eliminate):  E' = Q [R; 0] of the unit-length rows (np.linalg.qr, complete mode), Z = Q[:, neq:], x0 = Q1 R^-T e,
H_r = Z'HZ, f_r = Z'(H x0 + f), A_r = C_I Z, b_r = b_I - C_I x0 (open bounds kept), c0 = 1/2 x0'Hx0 + f'x0; expansion x = x0 + Z y,
lam_I = lam_r, lam_E = -R^-1 Q1'(H x + f + C_I'lam_I), fval = fval_r + c0.  The QR is fp64, every product np.longdouble.

Cases: cond(H) <= 1e3, equality rows with singular values in [0.3, 3], a planted optimum (so every case is solvable) with active
inequality rows whose multipliers are at least 0.1 in size and inactive rows at least 0.1 away from their bounds."""
import numpy as np

LD = np.longdouble
INF = 1e30


def cmat(A, ms, n):
    C = np.zeros((ms, n))
    C[np.arange(ms), np.arange(ms)] = 1.0
    return C if A is None or np.size(A) == 0 else np.vstack([C, np.asarray(A, dtype=np.float64).reshape(-1, n)])


def kept_rows(m, eq_rows):
    return np.setdiff1d(np.arange(m), np.asarray(eq_rows))


def eliminate(H, f, A, bupper, blower, sense, ms, eq_rows, dtype=LD):
    """one problem.  dict(x0, Z, Q1, R, norms, c0, H (None for an LP), f, A, bupper, blower, sense, kept); dtype: of the products"""
    f = np.asarray(f, dtype=np.float64)
    n, m = f.size, np.size(bupper)
    eq = np.asarray(eq_rows)
    kept = kept_rows(m, eq)
    C = cmat(A, ms, n)
    E = C[eq]
    norms = np.sqrt((E * E).sum(axis=1))
    Q, R = np.linalg.qr((E / norms[:, None]).T, mode="complete")
    neq = eq.size
    Q = Q.astype(dtype)
    R = R[:neq].astype(dtype)
    Q1, Z = Q[:, :neq], Q[:, neq:]
    bu, bl = np.asarray(bupper, dtype=np.float64), np.asarray(blower, dtype=np.float64)
    w = np.linalg.solve(R.T.astype(np.float64), bu[eq] / norms) if dtype is not LD else _tri_solve_lower(R.T, (bu[eq] / norms).astype(LD))
    x0 = Q1 @ w.astype(dtype)
    CI = C[kept].astype(dtype)
    fd = f.astype(dtype)
    if H is None:
        Hx0, Hr = np.zeros(n, dtype=dtype), None
    else:
        Hd = np.asarray(H, dtype=np.float64).astype(dtype)
        Hx0, Hr = Hd @ x0, Z.T @ Hd @ Z
        Hr = np.tril(Hr) + np.tril(Hr, -1).T      # one triangle, mirrored
    shift = CI @ x0
    opened = lambda b: np.abs(b) >= INF
    bur = np.where(opened(bu[kept]), bu[kept], bu[kept].astype(dtype) - shift)
    blr = np.where(opened(bl[kept]), bl[kept], bl[kept].astype(dtype) - shift)
    s = np.zeros(m, np.int32) if sense is None else np.asarray(sense, dtype=np.int32)
    return dict(x0=x0, Z=Z, Q1=Q1, R=R, norms=norms, c0=0.5 * (x0 @ Hx0) + fd @ x0, H=Hr, f=Z.T @ (Hx0 + fd), A=CI @ Z, bupper=bur, blower=blr,
                sense=s[kept].copy(), kept=kept, eq=eq, n=n, m=m, full=dict(H=H, f=f, C=C))


def _tri_solve_lower(L, b):
    y = np.zeros(b.size, dtype=LD)
    for i in range(b.size):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y


def _tri_solve_upper(U, b):
    y = np.zeros(b.size, dtype=LD)
    for i in range(b.size - 1, -1, -1):
        y[i] = (b[i] - U[i, i + 1:] @ y[i + 1:]) / U[i, i]
    return y


def expand(el, y, lam_r, fval_r):
    """(x, lam, fval) of the full problem from a reduced result, as float64"""
    y, lam_r = np.asarray(y, dtype=LD), np.asarray(lam_r, dtype=LD)
    x = el["x0"] + el["Z"] @ y
    F = el["full"]
    C = F["C"].astype(LD)
    g = F["f"].astype(LD) + C[el["kept"]].T @ lam_r
    if F["H"] is not None:
        g = g + np.asarray(F["H"], dtype=np.float64).astype(LD) @ x
    lam = np.zeros(el["m"], dtype=LD)
    lam[el["kept"]] = lam_r
    lam[el["eq"]] = -_tri_solve_upper(el["R"].astype(LD), (el["Q1"].T @ g).astype(LD)) / el["norms"]
    return x.astype(np.float64), lam.astype(np.float64), float(fval_r + el["c0"])


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# (n, neq, m, ms): the shapes of tests/test_gpu_eliminate.py; the first has one equality on a simple-bound row
SHAPES = [(6, 2, 10, 2), (64, 1, 70, 0), (64, 63, 70, 4), (65, 1, 70, 0), (70, 40, 90, 5), (130, 70, 150, 0)]
LP_SHAPE = (12, 4, 30, 0)


def _orth(rng, n):
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


def eq_rows_of(shape, bound_row=False):
    """the batch's equality rows: the first neq general rows -- or, bound_row, simple bound 0 and the first neq - 1 general rows"""
    n, neq, m, ms = shape
    if bound_row:
        return np.concatenate([[0], ms + np.arange(neq - 1)]).astype(np.int32)
    return (ms + np.arange(neq)).astype(np.int32)


def make_batch(shape, N, seed, lp=False, bound_row=False, soft=0, soft_active=False):
    """dict(H (None: LP), f, A, bupper, blower, sense, eq_rows, x, lam, shape): N planted problems; x, lam the planted optimum.
    soft: that many kept general rows carry DAQP_SOFT (they are inactive at the optimum).  soft_active: the upper bound of the first of
    them is pulled 0.02 BELOW the planted point, so that row ends active and violated (soft_slack > 0); x, lam are then no optimum."""
    n, neq, m, ms = shape
    rng = np.random.default_rng(seed)
    eq = eq_rows_of(shape, bound_row)
    kept = kept_rows(m, eq)
    mA = m - ms
    nr = n - neq
    n_act = nr if lp else min(3, nr)
    H = None if lp else np.empty((N, n, n))
    f, A = np.empty((N, n)), np.empty((N, mA, n))
    bu, bl, sense = np.empty((N, m)), np.empty((N, m)), np.zeros((N, m), np.int32)
    X, LAM = np.empty((N, n)), np.zeros((N, m))
    gen_eq = eq[eq >= ms] - ms      # general rows of A that are equalities
    for k in range(N):
        if not lp:
            U = _orth(rng, n)
            B = (U * np.logspace(0, 3, n)[rng.permutation(n)]) @ U.T
            H[k] = 0.5 * (B + B.T)
        Ak = rng.standard_normal((mA, n)) / np.sqrt(n)
        if gen_eq.size:      # singular values in [0.3, 3]; orthogonal to e_0 when bound 0 is an equality too
            g = gen_eq.size
            off = 1 if bound_row else 0
            V = _orth(rng, n - off)[:, :g]
            Eg = (_orth(rng, g) * rng.uniform(0.3, 3.0, g)) @ V.T
            Ak[gen_eq] = 0.0
            Ak[gen_eq, off:] = Eg
        A[k] = Ak
        C = cmat(Ak, ms, n)
        xp = 0.3 * rng.standard_normal(n)
        cx = C @ xp
        bu[k] = cx + rng.uniform(0.1, 1.0, m)
        bl[k] = cx - rng.uniform(0.1, 1.0, m)
        lam = np.zeros(m)
        bu[k, eq] = bl[k, eq] = cx[eq]
        lam[eq] = rng.uniform(0.1, 1.0, neq) * rng.choice([-1.0, 1.0], neq)
        sense[k, eq] = 5
        gen_kept = kept[kept >= ms]
        act = rng.choice(gen_kept, n_act, replace=False)
        for r in act:
            lam[r] = rng.uniform(0.1, 1.0) * rng.choice([-1.0, 1.0])
            if lam[r] > 0:
                bu[k, r] = cx[r]
            else:
                bl[k, r] = cx[r]
        opened = rng.choice(np.setdiff1d(gen_kept, act), 2, replace=False)
        bu[k, opened[0]], bl[k, opened[1]] = INF, -INF
        if soft:
            srows = rng.choice(np.setdiff1d(gen_kept, np.concatenate([act, opened])), soft, replace=False)
            sense[k, srows] = 8
            if soft_active:
                bu[k, srows[0]] = cx[srows[0]] - 0.02
        f[k] = -(C.T @ lam) - (0 if lp else H[k] @ xp)
        X[k], LAM[k] = xp, lam
    return dict(H=H, f=f, A=A, bupper=bu, blower=bl, sense=sense, eq_rows=eq, x=X, lam=LAM, shape=shape)


def golden_problems(path):
    """the 16 problems of tests/golden/golden_eliminated.npz: (dict per problem, with ms and eq_rows = the rows of sense 5)"""
    g = np.load(path, allow_pickle=False)
    out = []
    for k in sorted({key.split("/")[0] for key in g.files}):
        p = {name: g[f"{k}/{name}"] for name in ("H", "f", "A", "bupper", "blower", "sense", "x", "lam", "fval", "exitflag", "iter")}
        p["ms"] = p["bupper"].size - p["A"].shape[0]
        p["eq_rows"] = np.flatnonzero(p["sense"] == 5).astype(np.int32)
        p["name"] = k
        out.append(p)
    return out
