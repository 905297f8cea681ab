"""Cases and a CPU model of the null-space refinement tests (daqp_batch_refine_nullspace, daqp_amd/csrc/refine_nullspace.hip.h).
numpy and the oracle only; no test in this file.

Planted exact families, in the manner of tests/refine_cases.py: every datum is a small integer, (x*, lam*) are small integers with a
chosen working set W (both sides, simple bounds where ms > 0, general rows, one equality where W has a general row to spare), strict
complementarity: |lam*| >= 1 on W, slack >= 1 off it.  f = -(H x* + C' lam*) and the bounds follow, so (x*, lam*) is the exact
optimum (exact(): fractions.Fraction) and an error is an error of the solver's tolerances and arithmetic alone.

    singular    H = B'B, B an integer r x n matrix with entries in {-1, 0, 1}, r < n; W has k >= n - r rows and its KKT matrix
                [H C_W'; C_W 0] is nonsingular (kkt_nonsingular(): fraction-free elimination on Python integers, an exact rational rank)
    lp          H = None, W a vertex: k = n rows with a nonsingular C_W
    free        H = L L' with L unit lower triangular, nothing active (k = 0): Z'HZ is all of H.  Positive definite: for which = 1
    definite    the planted cases of refine_cases.py with n <= 64 (refine_cases.case(i)): for which = 1

Shapes: n over 1, 5, 16, 33 (odd, above half a wavefront) and 64 (the full wavefront, LDS stride 65); k over n - r (the fewest rows
that leave the KKT matrix nonsingular), n - 1 (one null-space column) and n (a vertex, Z empty), 0 for `free`; ms > 0 and ms = 0.

refine_nullspace_model(): the algorithm of the kernel in numpy -- residuals in exact rational arithmetic rounded once
(refine_cases._merit), the unit rows of C_W, their Householder QR, Z'HZ and its Cholesky factor in fp64, the same merit and acceptance
rule.  E(x, lam) = max(max|x - x*| / max|x*|, max|lam_W - lam*_W| / max|lam*|), the second term absent for an empty W.
"""
import functools

import numpy as np

import refine_cases as RC

LOWER = RC.LOWER
MODEL_BAR = 2.0 ** -49      # what the model must reach on every committed case from the oracle's solution

# kind, (n, m, ms), r = rank of H (singular), k = rows of W, seed.  Found by `python tests/refine_nullspace_cases.py`, which walks the
# seeds of each shape for: exact(), kkt_nonsingular(), the oracle OPTIMAL with the planted W and sides, n_prox > 0 (singular, lp), the
# model at E <= MODEL_BAR from the oracle's solution, and from zeros a run whose every trial mu is a factor 2 away from the end
# condition (decisive()); among those, the draw with the largest error of the oracle's own solution.
# From zeros the FIRST step of a well-conditioned system already lands at mu ~ 2^-52 <= 2^-50 and the loop ends there by its own rule,
# with E ~ cond(K) 2^-52 (1e-15 .. 1e-12 here): the model's E from zeros (model_error(i, zeros=True)) is what a run from zeros is
# held to, not MODEL_BAR.
CASES = [
    dict(kind="singular", shape=(1, 3, 1), r=0, k=1, seed=1),
    dict(kind="singular", shape=(5, 14, 2), r=3, k=2, seed=7),
    dict(kind="singular", shape=(5, 14, 0), r=3, k=4, seed=6),
    dict(kind="singular", shape=(16, 40, 4), r=10, k=6, seed=7),
    dict(kind="singular", shape=(16, 40, 4), r=10, k=15, seed=2),
    dict(kind="singular", shape=(33, 80, 5), r=20, k=13, seed=6),
    dict(kind="singular", shape=(33, 80, 0), r=20, k=32, seed=9),
    dict(kind="singular", shape=(33, 80, 5), r=20, k=33, seed=2),
    dict(kind="singular", shape=(64, 140, 10), r=40, k=24, seed=0),
    dict(kind="singular", shape=(64, 140, 0), r=40, k=63, seed=10),
    dict(kind="lp", shape=(1, 3, 1), r=0, k=1, seed=5),
    dict(kind="lp", shape=(5, 14, 2), r=0, k=5, seed=7),
    dict(kind="lp", shape=(16, 40, 0), r=0, k=16, seed=5),
    dict(kind="lp", shape=(33, 80, 5), r=0, k=33, seed=7),
    dict(kind="lp", shape=(64, 140, 10), r=0, k=64, seed=2),
    dict(kind="free", shape=(64, 70, 6), r=64, k=0, seed=6),
]
PROXIMAL = [i for i, c in enumerate(CASES) if c["kind"] in ("singular", "lp")]
SINGULAR = [i for i, c in enumerate(CASES) if c["kind"] == "singular"]
DEFINITE = [i for i, c in enumerate(RC.CASES) if c["shape"][0] <= 64]      # indices into refine_cases.CASES
FREE_FILL = 0.1
_KIND = dict(singular=1, lp=2, free=3)


def label(i):
    c = CASES[i]
    return "%s-n%d-k%d-ms%d" % (c["kind"], c["shape"][0], c["k"], c["shape"][2])


def make(kind, n, m, ms, r, k, seed):
    """dict(H (None for an LP), f, A, bupper, blower, x, lam, W (ids, ascending), lower (bool per row of W), n, m, ms, kind)"""
    rng = np.random.default_rng([9200, _KIND[kind], n, k, seed])
    if kind == "singular":
        B = rng.integers(-1, 2, (r, n)).astype(np.float64)
        H = B.T @ B
    elif kind == "free":
        L = np.tril(rng.integers(-1, 2, (n, n)) * (rng.random((n, n)) < FREE_FILL), -1).astype(np.float64) + np.eye(n)
        H = L @ L.T
    else:
        H = None
    A = rng.integers(-2, 3, (m - ms, n)).astype(np.float64)
    x = rng.integers(-3, 4, n).astype(np.float64)
    if not x.any():
        x[0] = 1.0
    nb = min(ms, 2, k)      # up to two simple bounds, the rest general rows
    W = np.sort(np.concatenate([rng.choice(ms, nb, replace=False) if nb else np.zeros(0, np.int64),
                                ms + rng.choice(m - ms, k - nb, replace=False)])).astype(np.int64)
    lower = np.arange(k) % 2 == 1      # sides alternate along W
    eq = k - 1 if k - nb >= 2 else -1  # the last row of W (a general row) is an equality
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
    f = -((H @ x if H is not None else 0.0) + C.T @ lam)
    return dict(H=H, f=f, A=A, bupper=bupper, blower=blower, x=x, lam=lam, W=W, lower=lower, n=n, m=m, ms=ms, kind=kind)


@functools.lru_cache(maxsize=None)
def case(i):
    c = CASES[i]
    p = make(c["kind"], *c["shape"], c["r"], c["k"], c["seed"])
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def dense(p):
    """p with its Hessian as a matrix (zeros for an LP): what refine_cases' helpers take"""
    return p if p["H"] is not None else dict(p, H=np.zeros((p["n"], p["n"])))


def exact(p):
    """refine_cases.exact (every datum an integer below 2^53, the planted pair satisfies the KKT conditions with strict
    complementarity in exact rational arithmetic) with H = 0 for an LP"""
    return RC.exact(dense(p))


def kkt_nonsingular(p):
    """[H C_W'; C_W 0] has full rank over the rationals: fraction-free (Bareiss) elimination with row pivoting on Python integers --
    every intermediate is an exact integer minor, and the last pivot is the determinant up to sign"""
    n, W = p["n"], p["W"]
    Cw = RC.rows(p, W)
    K = np.block([[dense(p)["H"], Cw.T], [Cw, np.zeros((len(W), len(W)))]])
    M = np.array([[int(v) for v in row] for row in K], dtype=object)
    assert all(float(a) == b for a, b in zip(M.ravel(), K.ravel()))
    N, prev = M.shape[0], 1
    for c in range(N):
        piv = next((r for r in range(c, N) if M[r, c] != 0), None)
        if piv is None:
            return False
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        if c + 1 < N:
            M[c + 1:, c + 1:] = (M[c + 1:, c + 1:] * M[c, c] - np.outer(M[c + 1:, c], M[c, c + 1:])) // prev
        prev = M[c, c]
    return True


def error(p, x, lam):
    W = p["W"]
    e = np.abs(x - p["x"]).max() / np.abs(p["x"]).max()
    return max(e, np.abs(lam[W] - p["lam"][W]).max() / np.abs(p["lam"]).max()) if len(W) else e


def refine_nullspace_model(p, x, lam, ids=None, lower=None, max_steps=3, trials=None):
    """(x, lam, steps, mu_before, mu_after): iterative refinement at the working set ids (default: the planted one), the correction by
    the null-space method on H itself.  trials: a list that receives the mu of every trial pair"""
    ids = p["W"] if ids is None else np.asarray(ids)
    lower = p["lower"] if lower is None else np.asarray(lower, bool)
    pd = dense(p)
    H, n, k = pd["H"], p["n"], len(ids)
    Cw = RC.rows(p, ids)
    s = np.sqrt((Cw * Cw).sum(axis=1))
    Q, R = np.linalg.qr((Cw / s[:, None]).T, mode="complete") if k else (np.eye(n), np.zeros((n, 0)))
    Q1, Z, R = Q[:, :k], Q[:, k:], R[:k]
    Lr = np.linalg.cholesky(Z.T @ H @ Z) if k < n else None      # (raises where H is not positive definite on the null space)
    x, lamW = np.array(x, np.float64), np.array(lam, np.float64)[ids]
    mu, r1, r2 = RC._merit(pd, ids, lower, x, lamW)
    mu_in, kept = mu, 0
    while kept < max_steps and mu > RC.MU_DONE:
        y = np.linalg.solve(R.T, r2 / s) if k else np.zeros(0)
        dx = Q1 @ y
        if k < n:
            t = r1 - H @ dx
            dx = dx + Z @ np.linalg.solve(Lr.T, np.linalg.solve(Lr, Z.T @ t))
        dlam = np.linalg.solve(R, Q1.T @ (r1 - H @ dx)) / s if k else np.zeros(0)
        xn, ln = x + dx, lamW + dlam
        mu_n, r1n, r2n = RC._merit(pd, ids, lower, xn, ln)
        if trials is not None:
            trials.append(mu_n)
        if not mu_n < mu:
            break
        gain_small = not mu_n <= 0.5 * mu
        x, lamW, mu, r1, r2, kept = xn, ln, mu_n, r1n, r2n, kept + 1
        if gain_small:
            break
    out = np.zeros(p["m"])
    out[ids] = lamW
    return x, out, kept, mu_in, mu


def decisive(trials):
    """no trial pair's mu sits within a factor 2 of the end condition mu <= 2^-50: an implementation that sums in another order takes
    the same number of steps"""
    return all(mu <= 0.5 * RC.MU_DONE or mu >= 2.0 * RC.MU_DONE for mu in trials)


def oracle_solution(oracle, p):
    """(x, lam, exitflag, ids of the final working set (sorted), their DAQP_LOWER bits, n_prox) of the oracle's cold solve"""
    om = oracle.model(p["n"], p["m"], p["ms"])
    assert om.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"], None) >= 0
    x, lam, _, flag, _ = om.solve()
    WS, sense, _, _ = om.state()
    ids = np.sort(WS)
    return x, lam, flag, ids, (sense[ids] & LOWER) != 0, int(om.prox()[0])


def planted_working_set(p, ids, low):
    """the oracle's working set is the planted one, side by side (an equality row may sit on either side)"""
    free = p["bupper"][p["W"]] != p["blower"][p["W"]]
    return np.array_equal(ids, p["W"]) and np.array_equal(low[free], p["lower"][free])


@functools.lru_cache(maxsize=None)
def oracle_side(i):
    """(x, lam, exitflag, ids, lower bits, n_prox) of the oracle on case i: computed once, shared, never modified"""
    from oracle import oracle as O
    return oracle_solution(O.Oracle(), case(i))


@functools.lru_cache(maxsize=None)
def model_error(i, zeros=False):
    """E of the model's output on case i, started from the oracle's solution (or from zeros with eight steps): what
    tests/test_gpu_refine_nullspace.py takes E_model from"""
    p = case(i)
    if zeros:
        xm, lm, _, _, _ = refine_nullspace_model(p, np.zeros(p["n"]), np.zeros(p["m"]), max_steps=8)
    else:
        x, lam = oracle_side(i)[:2]
        xm, lm, _, _, _ = refine_nullspace_model(p, x, lam)
    return error(p, xm, lm)


@functools.lru_cache(maxsize=None)
def definite_model_error(i, zeros=False):
    """the same for refine_cases.case(i) (positive definite H: which = 1), with the null-space model"""
    from oracle import oracle as O
    p = RC.case(i)
    if zeros:
        xm, lm, _, _, _ = refine_nullspace_model(p, np.zeros(p["n"]), np.zeros(p["m"]), max_steps=8)
    else:
        x, lam, _, _, _ = RC.oracle_solution(O.Oracle(), p)
        xm, lm, _, _, _ = refine_nullspace_model(p, x, lam)
    return RC.error(p, xm, lm)


if __name__ == "__main__":      # the search that CASES records
    import sys
    from oracle import oracle as O
    ora = O.Oracle()
    for c in CASES:
        best = None
        for seed in range(12):
            p = make(c["kind"], *c["shape"], c["r"], c["k"], seed)
            if not exact(p) or not kkt_nonsingular(p):
                continue
            x, lam, flag, ids, low, n_prox = oracle_solution(ora, p)
            if flag != 1 or not planted_working_set(p, ids, low) or (c["kind"] != "free" and n_prox <= 0):
                continue
            e0 = error(p, x, lam)
            if best is None or e0 > best[0]:
                try:
                    xm, lm, steps, _, _ = refine_nullspace_model(p, x, lam)
                    tz = []
                    xz, lz, stz, _, _ = refine_nullspace_model(p, np.zeros(p["n"]), np.zeros(p["m"]), max_steps=8, trials=tz)
                except np.linalg.LinAlgError:
                    continue
                if error(p, xm, lm) <= MODEL_BAR and decisive(tz):
                    best = (e0, seed, error(p, xm, lm), steps, error(p, xz, lz), stz)
        print(c["kind"], c["shape"], "k", c["k"], best)
        sys.stdout.flush()
