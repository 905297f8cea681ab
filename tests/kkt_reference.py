"""An extended-precision KKT certificate of a dense QP / LP -- no solver code, numpy only.

    min 1/2 x'Hx + f'x   s.t.   blower <= C x <= bupper,   C = [I_ms ; A]

with the reference's sign convention for the multipliers (H x + f + C'lam = 0, lam_k > 0 on an upper bound, lam_k < 0 on a
lower one) and its sense bits: ACTIVE 1, LOWER 2, IMMUTABLE 4 (with ACTIVE and bupper == blower: an equality), SOFT 8 (the row may
be violated; the violation costs 1/(2 rho_soft q_k) per squared unit, so an active soft row sits rho_soft q_k lam_k beyond its bound).

Everything is evaluated in np.longdouble.  q_k = c_k H^-1 c_k' comes from a Cholesky factor and a forward solve written out below;
1/sqrt(q_k) is the scaling the reference gives row k of the least-distance problem -- general rows (utils.c:586-612) and simple
bounds (utils.c:569-585: the norm of row k of R^-1, i.e. sqrt((H^-1)_kk)) alike -- and the unit its primal_tol applies to.

The two derived quantities restate the reference's definitions for a given (x, lam), they are not taken from a run:
  soft_slack_ref = rho_soft * sum over soft rows with lam_k != 0 of q_k lam_k^2     (auxiliary.c:46-88 with lam_qp = lam_ldp * scaling)
  fval_ref       = 1/2 x'Hx + f'x + 1/2 soft_slack_ref                              (api.c:471-477: (fval_ldp - |v|^2) / 2)
tests/test_cpu_kkt_reference.py holds both against the oracle's own soft_slack and fval on every case family (1e-10 relative);
the reference's definition agreed with them as written here, so nothing was corrected.

With normalised=False (an LP, H=None, or a merely semi-definite H: the proximal families) q_k is not defined: every q_k is taken as 1,
the residuals are in the problem's own units, the soft quantities are zero and fval_ref = 1/2 x'Hx + f'x.
"""
import numpy as np

LD = np.longdouble
ACTIVE, LOWER, IMMUTABLE, SOFT = 1, 2, 4, 8


def cholesky(H):
    """lower-triangular L with H = L L' in longdouble (H symmetric positive definite)"""
    H = np.array(H, dtype=LD)
    n = H.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = H[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise ValueError("H is not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (H[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def forward_solve(L, B):
    """Y with L Y = B (B: n x k), longdouble"""
    n = L.shape[0]
    Y = np.zeros(B.shape, dtype=LD)
    for i in range(n):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def constraint_matrix(A, ms, n):
    C = np.zeros((ms, n), dtype=LD)
    C[np.arange(ms), np.arange(ms)] = 1
    if A is not None and np.size(A):
        C = np.vstack([C, np.array(A, dtype=LD).reshape(-1, n)])
    return C


def row_q(H, A, ms):
    """q_k = c_k H^-1 c_k' for every row of C = [I_ms ; A] (longdouble vector of m)"""
    n = np.shape(H)[0]
    Y = forward_solve(cholesky(H), constraint_matrix(A, ms, n).T.copy())
    return (Y * Y).sum(axis=0)


def half_f_hinv_f(H, f):
    """1/2 f'H^-1 f (longdouble): what the reported fval of a QP lacks of the least-distance problem's 1/2 (|u|^2 + soft slack), the
    quantity DAQPSettings.fval_bound is compared with (daqp.c:10,20; api.c:471-477)"""
    y = forward_solve(cholesky(H), np.array(f, dtype=LD).reshape(-1, 1))
    return LD(0.5) * (y * y).sum()


def dual_value(H, f, A, bupper, blower, sense, ms, lam, rho_soft, q=None):
    """the dual function of the QP at multipliers lam (the problem's own units, the reference's sign convention), longdouble:
        g(lam) = -1/2 (f + C'lam)' H^-1 (f + C'lam) - sum_k lam_k b_k - 1/2 rho_soft sum over soft rows of q_k lam_k^2
    with b_k the upper bound where lam_k > 0 and the lower one where lam_k < 0.  A lower bound on the optimal value for every lam
    (weak duality); at a dual-feasible iterate of the active-set method it equals that iterate's reported fval."""
    f = np.array(f, dtype=LD).ravel()
    n = f.size
    lam = np.array(lam, dtype=LD).ravel()
    bu, bl = np.array(bupper, dtype=LD).ravel(), np.array(blower, dtype=LD).ravel()
    sense = np.zeros(lam.size, np.int64) if sense is None else np.asarray(sense, dtype=np.int64).ravel()
    C = constraint_matrix(A, ms, n)
    y = forward_solve(cholesky(H), (f + C.T @ lam).reshape(-1, 1))
    b_side = np.where(lam > 0, bu, bl)
    nz = lam != 0
    soft = ((sense & SOFT) != 0) & nz
    q = row_q(H, A, ms) if q is None else np.array(q, dtype=LD)
    return -LD(0.5) * (y * y).sum() - (lam[nz] * b_side[nz]).sum() - LD(0.5) * LD(rho_soft) * (q * lam * lam)[soft].sum()


def certificate(H, f, A, bupper, blower, sense, ms, x, lam, rho_soft, normalised=True, q=None, bar=1e-6):
    """dict of residuals of (x, lam) for the QP (H, f, A, bupper, blower, sense, ms); H=None: an LP.  q: row_q(H, A, ms) when the
    caller has it already (shared or unchanged matrices); bar: the slack beyond which a row with lam_k != 0 counts as inactive."""
    f = np.array(f, dtype=LD).ravel()
    n = f.size
    x, lam = np.array(x, dtype=LD).ravel(), np.array(lam, dtype=LD).ravel()
    bu, bl = np.array(bupper, dtype=LD).ravel(), np.array(blower, dtype=LD).ravel()
    m = bu.size
    sense = np.zeros(m, np.int64) if sense is None else np.asarray(sense, dtype=np.int64).ravel()
    C = constraint_matrix(A, ms, n)
    if H is None:
        normalised = False
        Hx = np.zeros(n, dtype=LD)
    else:
        Hx = np.array(H, dtype=LD) @ x
    if normalised:
        q = row_q(H, A, ms) if q is None else np.array(q, dtype=LD)
    else:
        q = np.ones(m, dtype=LD)
    sq = np.sqrt(q)
    one = LD(1)

    r = Hx + f + C.T @ lam
    stationarity = np.abs(r).max() / max(one, np.abs(Hx).max(), np.abs(f).max(), np.abs(C.T @ np.abs(lam)).max())

    cx = C @ x
    over, under = cx - bu, bl - cx                       # > 0: beyond the upper / lower bound
    soft = (sense & SOFT) != 0
    equality = ((sense & IMMUTABLE) != 0) & (bu == bl)
    ignored = ((sense & IMMUTABLE) != 0) & ~equality     # the solver never activates such a row
    nz = lam != 0
    upper_side = lam > 0

    # primal: hard rows, and soft rows that claim no violation (lam_k = 0)
    held = ~ignored & ~(soft & nz)
    primal = max(LD(0), (np.maximum(over, under) / sq)[held].max()) if held.any() else LD(0)

    # complementarity: distance of a row with a multiplier from the bound the multiplier names
    dist = np.where(upper_side, np.abs(over), np.abs(under))
    comp_rows = nz & ~soft & ~equality
    comp = np.where(comp_rows, dist / sq, LD(0))
    comp = np.where(equality, np.abs(over) / sq, comp)  # an equality sits on its bound whatever lam is
    complementarity = comp.max() if m else LD(0)

    # soft rows with a multiplier: (c_k x - b_k) = rho_soft q_k lam_k against the bound on the side of sign(lam_k)
    b_side = np.where(upper_side, bu, bl)
    soft_rows = soft & nz & np.bool_(normalised)
    rel = np.abs((cx - b_side) - LD(rho_soft) * q * lam) / np.maximum(one, np.abs(b_side))
    soft_relation = rel[soft_rows].max() if soft_rows.any() else LD(0)
    soft_slack_ref = LD(rho_soft) * (q * lam * lam)[soft_rows].sum()
    fval_ref = LD(0.5) * (x @ Hx) + f @ x + LD(0.5) * soft_slack_ref

    # sign: the bound a row with a multiplier sits on (or beyond) is the nearer one
    on_upper = over >= under
    wrong_sign = int((nz & ~equality & (on_upper != upper_side)).sum())
    slack = np.where(soft_rows, rel, comp)
    nonzero_inactive = int((nz & ~equality & (slack > bar)).sum())

    return dict(stationarity=float(stationarity), primal=float(primal), complementarity=float(complementarity),
                soft_relation=float(soft_relation), soft_slack_ref=float(soft_slack_ref), fval_ref=float(fval_ref),
                wrong_sign=wrong_sign, nonzero_inactive=nonzero_inactive, q_k=q)
