"""Inputs and the dense oracle of the soft-row adjoint tests (test_cpu_backward_soft.py checks every batch here against the
reference library on the CPU; test_gpu_backward_soft.py runs them on the GPU).  numpy only; no test in this file."""
import numpy as np

ACTIVE, LOWER, IMMUTABLE, SOFT = 1, 2, 4, 8
RHO = 0.3          # rho_soft of every batch here: an active soft row then sits O(0.1) beyond its bound and S is O(1) of the Gram matrix
NQ = 48            # problems per batch


def _spd(rng, N, n, diag):
    if diag:
        H = np.zeros((N, n, n))
        H[:, np.arange(n), np.arange(n)] = 1.0 + 9.0 * rng.random((N, n))
        return H
    L = np.tril(rng.standard_normal((N, n, n))) / np.sqrt(n)
    return L @ np.swapaxes(L, 1, 2) + np.eye(n)


def planted_batch(N, n, mA, ms, soft, seed, diag=False, shared=False, fscale=3.0, soft_eq=None, inactive_soft=False):
    """x = 0 satisfies every hard row (|c_i x| <= 0.3 .. 1.0); the rows in `soft` (constraint ids, simple bounds first) carry DAQP_SOFT and
    an upper bound 0.2 .. 0.7 below what the unconstrained optimum gives them, so most of them end up active and violated.
    soft_eq: id of a row turned into a soft equality (ACTIVE | IMMUTABLE | SOFT, bupper == blower) through the same kind of point.
    inactive_soft: the SOFT rows get bounds of +-50 instead (ns_max > 0, no soft row active)."""
    rng = np.random.default_rng(seed)
    m = ms + mA
    H = _spd(rng, 1 if shared else N, n, diag)
    A = rng.standard_normal((1 if shared else N, mA, n))
    f = fscale * rng.standard_normal((N, n))
    Hb, Ab = np.broadcast_to(H, (N, n, n)) if shared else H, np.broadcast_to(A, (N, mA, n)) if shared else A
    xu = -np.linalg.solve(Hb, f[:, :, None])[:, :, 0]
    Cm = np.concatenate([np.broadcast_to(np.eye(n)[:ms], (N, ms, n)), Ab], axis=1)
    cx = np.einsum("qik,qk->qi", Cm, xu)
    w = 0.3 + 0.7 * rng.random((N, m))
    bu, bl = w.copy(), -(0.3 + 0.7 * rng.random((N, m)))
    sense = np.zeros((N, m), np.int32)
    d = 0.2 + 0.5 * rng.random((N, m))
    for k in soft:
        sense[:, k] = SOFT
        if inactive_soft:
            bu[:, k], bl[:, k] = 50.0, -50.0
        else:
            up = cx[:, k] > 0          # the side the unconstrained optimum leans to
            bu[:, k] = np.where(up, cx[:, k] - d[:, k], cx[:, k] + d[:, k] + 1.0)
            bl[:, k] = np.where(up, cx[:, k] - d[:, k] - 1.0, cx[:, k] + d[:, k])
    if soft_eq is not None:
        sense[:, soft_eq] = ACTIVE | IMMUTABLE | SOFT
        bu[:, soft_eq] = bl[:, soft_eq] = cx[:, soft_eq] - np.sign(cx[:, soft_eq]) * d[:, soft_eq]
    return dict(H=H[0] if shared else H, A=A[0] if shared else A, f=f, bupper=bu, blower=bl, sense=sense, ms=ms, shared=shared,
                ns_max=len(set(soft) | ({soft_eq} if soft_eq is not None else set())), settings=dict(rho_soft=RHO))


def generator_batch(N, n, m, na, seed, n_soft=2):
    """a batch of the library's benchmark generator (oracle.generate_batch) with n_soft rows that are inactive at its optimum made SOFT
    and given an upper bound 0.2 .. 0.5 below their value there -- the shapes of the workgroup and HBM-scratch paths of the adjoint"""
    from oracle import oracle as O
    q = O.generate_batch(N, n, m, 0, na, seed)
    rng = np.random.default_rng(seed + 1000)
    ax = np.einsum("qik,qk->qi", q["A"], q["xref"])
    slack = np.minimum(q["bupper"] - ax, ax - q["blower"])
    sense = np.zeros((N, m), np.int32)
    for k in range(N):
        rows = np.argsort(-slack[k])[:n_soft]          # the rows furthest from their bounds
        sense[k, rows] = SOFT
        q["bupper"][k, rows] = ax[k, rows] - (0.2 + 0.3 * rng.random(n_soft))
        q["blower"][k, rows] = q["bupper"][k, rows] - 1.0
    return dict(H=q["H"], A=q["A"], f=q["f"], bupper=q["bupper"], blower=q["blower"], sense=sense, ms=0, shared=False, ns_max=n_soft,
                settings=dict(rho_soft=RHO))


# name -> builder.  Every parity batch: all problems end OPTIMAL / SOFT_OPTIMAL, at least half SOFT_OPTIMAL with an active SOFT row
# (asserted against the reference library in test_cpu_backward_soft.py and against the GPU's own results in test_gpu_backward_soft.py).
PARITY = {
    # one wavefront, everything in LDS: two soft general rows (ids 4, 7) and one soft simple bound (id 1)
    "one_wave": lambda: planted_batch(NQ, 6, 8, 2, [1, 4, 7], seed=21),
    # working sets beyond n + 1 rows: a box on all of x pushed into a corner (fscale) + three soft general rows
    "cap_beyond_n1": lambda: planted_batch(NQ, 4, 4, 4, [4, 5, 6], seed=22, fscale=6.0),
    # diagonal H (rows < ms of R^-1 un-normalised) with a soft simple bound and a soft general row
    "diag_h": lambda: planted_batch(NQ, 6, 4, 6, [2, 7], seed=23, diag=True),
    # a soft equality row next to a soft inequality
    "soft_equality": lambda: planted_batch(NQ, 6, 8, 2, [5], seed=24, soft_eq=3),
    # one H and A for the batch, bounds and sense per problem
    "shared": lambda: planted_batch(NQ, 6, 8, 2, [0, 4, 6], seed=25, shared=True),
    # workgroup path (rows and Gram matrix in LDS) and HBM-scratch path: the smallest shapes tests/test_gpu_backward.py has for them
    "workgroup": lambda: generator_batch(32, 80, 200, 30, seed=7),
    "hbm_scratch": lambda: generator_batch(32, 128, 192, 40, seed=7),
}
NO_SOFT_ACTIVE = lambda: planted_batch(NQ, 6, 8, 2, [4, 7], seed=26, inactive_soft=True)


def problem(q, k):
    """(H, C, f, bupper, blower, sense) of problem k, C = [first ms rows of I; A]"""
    H = q["H"] if q["shared"] else q["H"][k]
    A = q["A"] if q["shared"] else q["A"][k]
    n = H.shape[0]
    return H, np.vstack([np.eye(n)[:q["ms"]], A]), q["f"][k], q["bupper"][k], q["blower"][k], q["sense"][k]


def dense_adjoint(H, Cm, W, is_soft, rho, g):
    """[H C_W'; C_W -S] [dz; dnu] = [g; 0] by a dense solve, S = diag(rho q_k on the SOFT rows of W); also q (per row of W) and
    U (rows u_k = H^-1 c_k')"""
    n, na = H.shape[0], len(W)
    U = np.linalg.solve(H, Cm[W].T).T
    qk = np.einsum("kj,kj->k", Cm[W], U)
    K = np.zeros((n + na, n + na))
    K[:n, :n] = H
    K[:n, n:] = Cm[W].T
    K[n:, :n] = Cm[W]
    K[n:, n:] = -np.diag(rho * qk * is_soft)
    sol = np.linalg.solve(K, np.concatenate([g, np.zeros(na)]))
    return sol[:n], sol[n:], qk, U
