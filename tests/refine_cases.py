"""Cases and a CPU model of the refinement tests (daqp_batch_refine, daqp_amd/csrc/refine.hip.h).  No GPU.

Planted ill-conditioned family.  H = L L' with L unit lower triangular and entries in {-1, 0, 1} ({-3, ..., 3} at n = 12, where nothing smaller reaches the range): H is an exact integer matrix whose
condition number is genuinely large (that of L grows exponentially with its fill; a diagonal scaling would not do -- Cholesky is insensitive
to it).  A has entries in {-2, ..., 2}; x* and lam* are small integers with a chosen active set W that holds upper and lower sides, simple
bounds (where ms > 0), general rows and one equality row; strict complementarity: |lam*| >= 1 on W, slack >= 1 off it (and to the other
bound of a row of W).  f = -(H x* + C' lam*) and the bounds follow, all integers: every datum is exactly representable (verified with
fractions.Fraction in exact()), so (x*, lam*) is the exact optimum and an error is an error of the arithmetic alone.

refine_model(): the algorithm of the kernel in numpy -- residuals in exact rational arithmetic rounded once, the KKT correction solved in
fp64 on a Cholesky factor of H through the Gram matrix of the unit rows of C_W R^-1, the same merit and acceptance rule.

E(x, lam) = max(max|x - x*| / max|x*|, max|lam_W - lam*_W| / max|lam*|).
"""
import functools
from fractions import Fraction

import numpy as np

LOWER = 2      # DAQP_LOWER in a workspace's sense
MU_DONE = 2.0 ** -50

# (n, m, ms), seed, fill of L below the diagonal -> cond(H) as np.linalg.cond gives it, between 1e6 and 1e9.  Found by
# `python tests/refine_cases.py`, which searches fill and seed per shape for: cond in range, the oracle OPTIMAL with the planted W, the
# model at E <= 2^-49; among those, the draw with the largest error of the oracle's own solution.
CASES = [
    dict(shape=(12, 30, 4), seed=8, fill=0.68, cond=1.4e8, amp=3),
    dict(shape=(50, 100, 0), seed=0, fill=0.56, cond=3.3e8),
    dict(shape=(64, 96, 8), seed=5, fill=0.40, cond=2.6e8),
    dict(shape=(80, 120, 0), seed=1, fill=0.32, cond=1.6e8),
    dict(shape=(130, 150, 2), seed=5, fill=0.16, cond=1.1e8),
]
COND_RANGE = (1e6, 1e9)


def make(n, m, ms, seed, fill, amp=1, k=None):
    """dict(H, f, A, bupper, blower, x, lam, W (ids, ascending), lower (bool per row of W), n, m, ms) of one planted problem; k: the rows
    of its working set (default: about n / 4)"""
    rng = np.random.default_rng([9100, n, seed])
    L = np.tril(rng.integers(-amp, amp + 1, (n, n)) * (rng.random((n, n)) < fill), -1).astype(np.float64) + np.eye(n)
    H = L @ L.T
    A = rng.integers(-2, 3, (m - ms, n)).astype(np.float64)
    x = rng.integers(-3, 4, n).astype(np.float64)
    if not x.any():
        x[0] = 1.0
    # the active set: up to two simple bounds, the rest general rows, about n / 4 rows in all
    k = max(4, n // 4) if k is None else k
    nb = min(ms, 2)
    W = np.sort(np.concatenate([rng.choice(ms, nb, replace=False) if nb else np.zeros(0, np.int64),
                                ms + rng.choice(m - ms, k - nb, replace=False)])).astype(np.int64)
    lower = np.arange(k) % 2 == 1      # sides alternate along W: both sides among the simple bounds and among the general rows
    eq = k - 1                         # the last row of W (a general row) is an equality
    Cx = np.concatenate([x[:ms], A @ x])
    bupper = Cx + rng.integers(1, 4, m)
    blower = Cx - rng.integers(1, 4, m)
    lam = np.zeros(m)
    for j, i in enumerate(W):
        mag = float(rng.integers(1, 4))
        if lower[j]:
            blower[i], lam[i] = Cx[i], -mag
        else:
            bupper[i], lam[i] = Cx[i], mag
        if j == eq:
            bupper[i] = blower[i] = Cx[i]
    C = np.vstack([np.eye(n)[:ms], A])
    f = -(H @ x + C.T @ lam)
    return dict(H=H, f=f, A=A, bupper=bupper, blower=blower, x=x, lam=lam, W=W, lower=lower, n=n, m=m, ms=ms)


@functools.lru_cache(maxsize=None)
def case(i):
    c = CASES[i]
    p = make(*c["shape"], c["seed"], c["fill"], c.get("amp", 1))
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def rows(p, ids):
    """rows ids of C = [I_ms; A]"""
    C = np.zeros((len(ids), p["n"]))
    for j, i in enumerate(ids):
        if i < p["ms"]:
            C[j, i] = 1.0
        else:
            C[j] = p["A"][i - p["ms"]]
    return C


def exact(p):
    """every datum is an integer of magnitude < 2^53 (exactly representable), and the planted pair satisfies the KKT conditions with
    strict complementarity in exact rational arithmetic"""
    F = lambda a: [Fraction(float(v)) for v in np.ravel(a)]
    for key in ("H", "f", "A", "bupper", "blower", "x", "lam"):
        for v in F(p[key]):
            if v.denominator != 1 or abs(v.numerator) >= 2 ** 53:
                return False
    n, m, ms = p["n"], p["m"], p["ms"]
    H, A, x, lam, f = (F(p[key]) for key in ("H", "A", "x", "lam", "f"))
    bu, bl = F(p["bupper"]), F(p["blower"])
    Cx = x[:ms] + [sum(A[r * n + j] * x[j] for j in range(n)) for r in range(m - ms)]
    for j in range(n):
        g = sum(H[j * n + i] * x[i] for i in range(n)) + f[j] + (lam[j] if j < ms else 0) + sum(A[r * n + j] * lam[ms + r] for r in range(m - ms))
        if g != 0:
            return False
    inW = set(int(i) for i in p["W"])
    for i in range(m):
        if i in inW:
            side_low = bool(p["lower"][list(p["W"]).index(i)])
            if abs(lam[i]) < 1 or (lam[i] < 0) != side_low or Cx[i] != (bl[i] if side_low else bu[i]):
                return False
            if bu[i] != bl[i] and (bu[i] - Cx[i] if side_low else Cx[i] - bl[i]) < 1:
                return False
        elif lam[i] != 0 or bu[i] - Cx[i] < 1 or Cx[i] - bl[i] < 1:
            return False
    return True


def error(p, x, lam):
    W = p["W"]
    return max(np.abs(x - p["x"]).max() / np.abs(p["x"]).max(), np.abs(lam[W] - p["lam"][W]).max() / np.abs(p["lam"]).max())


def _merit(p, ids, lower, x, lamW):
    """(mu, r1, r2): residuals in exact rational arithmetic, rounded once"""
    n = p["n"]
    Fr = lambda a: [Fraction(float(v)) for v in a]
    xf, lf = Fr(x), Fr(lamW)
    Cw = rows(p, ids)
    Hx = [sum(Fraction(float(h)) * xj for h, xj in zip(p["H"][i], xf) if h != 0.0) for i in range(n)]
    Cl = [sum(Fraction(float(Cw[k, j])) * lf[k] for k in range(len(ids)) if Cw[k, j] != 0.0) for j in range(n)]
    Cla = [sum(Fraction(float(Cw[k, j])) * abs(lf[k]) for k in range(len(ids)) if Cw[k, j] != 0.0) for j in range(n)]
    r1 = np.array([float(-(Hx[j] + Fraction(float(p["f"][j])) + Cl[j])) for j in range(n)])
    b = np.array([p["blower"][i] if lo else p["bupper"][i] for i, lo in zip(ids, lower)])
    cx = [sum(Fraction(float(Cw[k, j])) * xf[j] for j in range(n) if Cw[k, j] != 0.0) for k in range(len(ids))]
    r2 = np.array([float(Fraction(float(bk)) - c) for bk, c in zip(b, cx)])
    s1 = max(1.0, max(abs(float(v)) for v in Hx), np.abs(p["f"]).max(), max(abs(float(v)) for v in Cla))
    mu = np.abs(r1).max() / s1 if n else 0.0
    if len(ids):
        ax = np.abs(Cw * np.asarray(x)[None, :]).sum(axis=1)
        mu = max(mu, (np.abs(r2) / np.maximum(1.0, np.maximum(np.abs(b), ax))).max())
    return mu, r1, r2


def refine_model(p, x, lam, ids=None, lower=None, max_steps=3):
    """(x, lam, steps, mu_before, mu_after): iterative refinement at the working set ids (default: the planted one)"""
    ids = p["W"] if ids is None else np.asarray(ids)
    lower = p["lower"] if lower is None else np.asarray(lower, bool)
    R = np.linalg.cholesky(p["H"]).T                       # H = R'R
    Rinv = np.linalg.solve(R, np.eye(p["n"]))
    Cw = rows(p, ids)
    Nw = Cw @ Rinv
    sn = 1.0 / np.sqrt((Nw * Nw).sum(axis=1))
    Nw = Nw * sn[:, None]
    Lg = np.linalg.cholesky(Nw @ Nw.T) if len(ids) else None
    x, lamW = np.array(x, np.float64), np.array(lam, np.float64)[ids]
    mu, r1, r2 = _merit(p, ids, lower, x, lamW)
    mu_in, kept = mu, 0
    while kept < max_steps and mu > MU_DONE:
        w = Rinv.T @ r1
        if len(ids):
            z = np.linalg.solve(Lg.T, np.linalg.solve(Lg, Nw @ w - r2 * sn))
            dlam = z * sn
            dx = Rinv @ (w - Nw.T @ z)
        else:
            dlam, dx = np.zeros(0), Rinv @ w
        xn, ln = x + dx, lamW + dlam
        mu_n, r1n, r2n = _merit(p, ids, lower, xn, ln)
        if not mu_n < mu:
            break
        gain_small = not mu_n <= 0.5 * mu
        x, lamW, mu, r1, r2, kept = xn, ln, mu_n, r1n, r2n, kept + 1
        if gain_small:
            break
    out = np.zeros(p["m"])
    out[ids] = lamW
    return x, out, kept, mu_in, mu


def oracle_solution(oracle, p):
    """(x, lam, exitflag, ids of the final working set (sorted), their DAQP_LOWER bits) of the oracle's cold solve"""
    om = oracle.model(p["n"], p["m"], p["ms"])
    assert om.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"], None) >= 0
    x, lam, _, flag, _ = om.solve()
    WS, sense, _, _ = om.state()
    order = np.argsort(WS)
    ids = WS[order]
    return x, lam, flag, ids, (sense[ids] & LOWER) != 0


@functools.lru_cache(maxsize=None)
def model_error(i):
    """E of the model's output on case i, started from the oracle's solution: what tests/test_gpu_refine.py takes E_model from"""
    from oracle import oracle as O
    p = case(i)
    x, lam, _, _, _ = oracle_solution(O.Oracle(), p)
    xm, lm, _, _, _ = refine_model(p, x, lam)
    return error(p, xm, lm)


if __name__ == "__main__":      # the search that CASES records
    import sys
    from oracle import oracle as O
    ora = O.Oracle()
    for c in CASES:
        n, m, ms = c["shape"]
        best = None
        for fill in np.linspace(0.02, 1.0, 50):
            for seed in range(6):
                p = make(n, m, ms, seed, float(fill), c.get("amp", 1))
                cond = np.linalg.cond(p["H"])
                if not (3 * COND_RANGE[0] <= cond <= COND_RANGE[1] / 3):
                    continue
                x, lam, flag, ids, low = oracle_solution(ora, p)
                if flag != 1 or not np.array_equal(ids, p["W"]) or not np.array_equal(low[:-1], p["lower"][:-1]):
                    continue
                e0 = error(p, x, lam)
                if best is None or e0 > best[0]:
                    xm, lm, steps, _, _ = refine_model(p, x, lam)
                    if error(p, xm, lm) <= 2.0 ** -49:
                        best = (e0, seed, float(fill), cond, error(p, xm, lm), steps)
        print(c["shape"], best)
        sys.stdout.flush()
