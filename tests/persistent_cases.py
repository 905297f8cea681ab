"""Batches of tests/test_gpu_persistent.py: more problems than a persistent launch has workgroups, so that some workgroups take a
second problem, with the FIRST problem of those workgroups chosen to leave the most behind.  tests/test_cpu_persistent.py holds the
same data to its conditions with numpy and the oracle alone.  No test in this file.

A batch has N = 520 problems for a grid of 512: workgroup b < 8 handles problem b (HEAD) and then problem 512 + b (TAIL).
  HEAD   working sets of BIG rows -- and among them one problem whose adjoint / refinement ends -20 (two nearly parallel active
         equality rows: the Cholesky pivot of the unit-row Gram matrix falls below zero_tol) and one infeasible problem
  TAIL   working sets of SMALL rows: everything beyond row SMALL of the scratch slab still holds HEAD's rows and Gram matrix
The comparison run is the batch of the eight TAIL problems alone: there each of them is the first problem of its workgroup.

The tier arithmetic is restated here from the headers: backward_lds_bytes / backward_scratch_doubles (csrc/backward.hip.h),
refine_lds_bytes / refine_scratch_doubles (csrc/refine.hip.h), pick_tier and scratch_grid (csrc/post_solve.hip), the grid rule of
daqp_batch_eliminate (csrc/post_solve.hip).  The GPU tests hold the grid it gives to the bytes of per-workgroup scratch that the
library reports having allocated."""
import functools

import numpy as np

import eliminate_cases as EC
import refine_cases as RC
from oracle import oracle as O

N, GRID = 520, 512
HEAD, TAIL = np.arange(8), np.arange(GRID, N)
K20, KINF = 2, 5                     # HEAD problems: status -20, infeasible
BIG, MID, SMALL = 60, 30, 10         # rows of the working sets: HEAD, the bulk, TAIL
SINGULAR = -20
ZERO_TOL = 1e-7                      # of the adjoint / refinement batches: between the two pivots of the -20 problem (near_dependent)
EPS_DEP = 3e-5
LDS_MAX = 144 * 1024
SCRATCH_BYTES = 256 << 20


# ---- tier arithmetic -------------------------------------------------------------------------------------------------------------
def tri(k):
    return (k * (k + 1)) >> 1


def backward_lds_bytes(n, cap, rl, nl):
    # dbl = 3 n + 4 cap (+ n (n + 1) / 2 if rl) (+ cap (n | 1) + tri(cap) if nl); bytes = 8 dbl + 4 (2 cap + 2)
    dbl = 3 * n + 4 * cap + (n * (n + 1) // 2 if rl else 0) + (cap * (n | 1) + tri(cap) if nl else 0)
    return 8 * dbl + 4 * (2 * cap + 2)


def refine_lds_bytes(n, cap, rl, nl):
    # dbl = 6 n + 7 cap + kRefineRed (16) (+ ...: as above)
    dbl = 6 * n + 7 * cap + 16 + (n * (n + 1) // 2 if rl else 0) + (cap * (n | 1) + tri(cap) if nl else 0)
    return 8 * dbl + 4 * (2 * cap + 2)


def scratch_doubles(n, cap):
    # backward_scratch_doubles == refine_scratch_doubles
    return cap * (n | 1) + tri(cap)


def pick_tier(n, cap, lds_bytes):
    """(tier, lds): 0 one wavefront, 1 workgroup with rows + Gram matrix in LDS, 2 in scratch, -1 no fit -- pick_tier of post_solve.hip"""
    small = n <= 64 and lds_bytes(n, cap, True, True) <= LDS_MAX
    lds_nl = lds_bytes(n, cap, small, True)
    nl = small or lds_nl <= LDS_MAX
    lds = lds_nl if nl else lds_bytes(n, cap, False, False)
    return (-1 if lds > LDS_MAX else (0 if small else (1 if nl else 2))), lds


def persistent_grid(Nq, bytes_per_wg):
    """scratch_grid of post_solve.hip and the rule of daqp_batch_eliminate: min(N, 512), fewer where 256 MiB / scratch is, never below 16"""
    return min(Nq, max(16, min(512, SCRATCH_BYTES // bytes_per_wg)))


def smallest_scratch_n(lds_bytes, ns=0):
    return next(n for n in range(65, 512) if pick_tier(n, n + ns + 1, lds_bytes)[0] == 2)


ADJOINT_SHAPE = (120, 150, 0)                                   # (n, m, ms)
REFINE_SHAPE = (smallest_scratch_n(refine_lds_bytes), 150, 2)   # n = 106
ELIM_SHAPES = [(65, 1, 70, 0), (70, 40, 90, 5)]                 # (n, neq, m, ms)
NS_MAX = 2


# ---- the adversaries -------------------------------------------------------------------------------------------------------------
def near_dependent(n, m, ms, nact, rng, eps=EPS_DEP):
    """one planted problem (the construction of tests/test_gpu_backward_soft.py::_near_dependent at any shape): general rows 0 and 1
    nearly parallel (relative distance eps), both equalities (sense 5) through the planted point; general rows 2 .. nact - 1 active at
    their upper bounds with multiplier 0.5; every other row 0.5 away.  The solver (sing_tol 3.7e-11) keeps both rows; the pivot of the
    unit-row Gram matrix, ~eps^2 = 1e-9, is below ZERO_TOL."""
    rng = np.random.default_rng(rng)
    mA = m - ms
    L = np.tril(rng.standard_normal((n, n))) / np.sqrt(n)
    H = L @ L.T + np.eye(n)
    A = rng.standard_normal((mA, n))
    A[1] = A[0] + eps * rng.standard_normal(n)
    xs = rng.standard_normal(n)
    C = np.vstack([np.eye(n)[:ms], A])
    cx = C @ xs
    lam = np.zeros(m)
    lam[ms:ms + nact] = 0.5
    f = -(H @ xs + C.T @ lam)
    bu, bl = cx + 0.5, cx - 0.5
    bu[ms:ms + nact] = cx[ms:ms + nact]
    bl[ms:ms + 2] = cx[ms:ms + 2]
    sense = np.zeros(m, np.int32)
    sense[ms:ms + 2] = 5
    return dict(H=0.5 * (H + H.T), f=f, A=A, bupper=bu, blower=bl, sense=sense, x=xs)


def dependent_pivot(p, ms):
    """the smallest Cholesky pivot of the unit-row Gram matrix of C_W H^-1 C_W' with W = the rows at a bound of the planted point"""
    n = p["f"].size
    C = np.vstack([np.eye(n)[:ms], p["A"]])
    cx = C @ p["x"]
    W = np.flatnonzero((np.abs(cx - p["bupper"]) < 1e-12) | (np.abs(cx - p["blower"]) < 1e-12))
    R = np.linalg.cholesky(p["H"]).T
    Nw = np.linalg.solve(R.T, C[W].T).T
    Nw /= np.sqrt((Nw * Nw).sum(axis=1))[:, None]
    G = Nw @ Nw.T
    # right-looking Cholesky until the first pivot below ZERO_TOL (np.linalg.cholesky would raise or not, by rounding)
    piv = []
    for c in range(len(W)):
        piv.append(G[c, c])
        if G[c, c] < ZERO_TOL:
            break
        G[c + 1:, c] /= np.sqrt(G[c, c])
        G[c + 1:, c + 1:] -= np.outer(G[c + 1:, c], G[c + 1:, c])
    return W, min(piv)


def cross(p, ms):
    """two general rows with blower > bupper: infeasible (tests/test_gpu_backward.py::_crossed)"""
    p["blower"][ms] = p["bupper"][ms] + 1.0
    p["blower"][ms + 1] = p["bupper"][ms + 1] + 1.0


def _freeze(b):
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


KEYS = ("H", "f", "A", "bupper", "blower", "sense")


# ---- 1: the adjoint batches ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adjoint_batch(soft=False):
    """dict(H, f, A, bupper, blower, sense) of N problems of ADJOINT_SHAPE drawn by the oracle's generator (generate_qp: planted working
    sets of BIG / MID / SMALL rows), K20 and KINF replaced.  soft: two SOFT rows and one equality per problem (add_sense_variety)."""
    n, m, ms = ADJOINT_SHAPE
    seed = 6200 if soft else 6100
    qs = []
    for k in range(N):
        na = BIG if k < 8 else (SMALL if k >= GRID else MID)
        q = O.generate_qp(n, m, ms, na, rng=[seed, k])
        q = {key: q[key] for key in KEYS}
        if soft:
            q = O.add_sense_variety(q, ms, 1, NS_MAX, [seed + 1, k])
        if k == K20:
            q = {key: v for key, v in near_dependent(n, m, ms, BIG, [seed, k, 1]).items() if key in KEYS}
        if k == KINF:
            cross(q, ms)
        qs.append(q)
    return _freeze({key: np.stack([q[key] for q in qs]) for key in KEYS})


def subset(b, idx):
    """the problems idx of a batch, as a batch of their own"""
    return {key: np.ascontiguousarray(b[key][idx]) for key in KEYS}


# ---- 2: the refinement batch -----------------------------------------------------------------------------------------------------
# planted integer problems of refine_cases.make at REFINE_SHAPE with working sets of BIG, n // 4 and SMALL rows: (seed, fill) found by
# `python tests/persistent_cases.py` under the conditions of refine_cases' own search (cond(H) in COND_RANGE, the oracle OPTIMAL at the
# planted working set, the model at E <= 2^-49)
REFINE_DRAWS = {BIG: (2, 0.2), None: (1, 0.2), SMALL: (1, 0.22)}


@functools.lru_cache(maxsize=None)
def refine_problem(k):
    n, m, ms = REFINE_SHAPE
    seed, fill = REFINE_DRAWS[k]
    return _freeze(RC.make(n, m, ms, seed, fill, k=k))


@functools.lru_cache(maxsize=None)
def refine_batch():
    """N problems: HEAD planted with BIG rows, the bulk with n // 4, TAIL with SMALL; K20 and KINF replaced.  sense is all zero but for K20."""
    n, m, ms = REFINE_SHAPE
    qs = []
    for k in range(N):
        p = refine_problem(BIG if k < 8 else (SMALL if k >= GRID else None))
        q = {key: np.array(p[key]) for key in KEYS[:5]}
        q["sense"] = np.zeros(m, np.int32)
        if k == K20:
            q = {key: v for key, v in near_dependent(n, m, ms, BIG, [6300, k]).items() if key in KEYS}
        if k == KINF:
            cross(q, ms)
        qs.append(q)
    return _freeze({key: np.stack([q[key] for q in qs]) for key in KEYS})


# ---- 3: the elimination batches --------------------------------------------------------------------------------------------------
K6, K8 = 2, 5                        # HEAD problems: dependent equality rows (-6), bupper != blower on an equality row (-8)


@functools.lru_cache(maxsize=None)
def elim_batch(i):
    """eliminate_cases.make_batch at ELIM_SHAPES[i], N problems; K6: the last equality row is a copy of the first (neq = 1: a zero row,
    which depends on nothing less), K8: the bounds of the first equality row differ"""
    shape = ELIM_SHAPES[i]
    n, neq, m, ms = shape
    b = EC.make_batch(shape, N, 6400 + i)
    r = b["eq_rows"] - ms
    if neq == 1:
        b["A"][K6, r[0]] = 0.0
    else:
        b["A"][K6, r[-1]] = b["A"][K6, r[0]]
    b["bupper"][K8, b["eq_rows"][0]] += 0.25
    return _freeze(b)


# ---- 4-6: the solve batches ------------------------------------------------------------------------------------------------------
SOLVE_N, SOLVE_GRID = 24, 8
SOLVE_SHAPES = [(70, 160, 5, 25), (130, 300, 0, 50)]      # (n, m, ms, n_active)
TIER_SHAPE = (129, 200, 10, 30)
K_EMPTY, K_INF = 1, 4                # among the first eight: the unconstrained optimum is feasible; infeasible
# the hand-over: SOLVE_SHAPES[1] with DAQP_AMD_WG_CAPL = 52.  (The planner takes the workgroup kernel only while the packed factor holds
# min(cap, 48) rows or more -- plan_shape, csrc/plan.hip.h -- and the working sets of SOLVE_SHAPES[0] never get there.)
HAND_OVER_SHAPE, HAND_OVER_SEED, HAND_OVER_CAPL = SOLVE_SHAPES[1], 6501, 52


def trace_peak(trace):
    """the largest working set of an add / remove trace (+(id + 1), -(id + 1), branch markers above 0x40000000 dropped), cold start"""
    t = np.asarray(trace)
    t = t[t < 0x40000000]
    return int(np.cumsum(np.sign(t)).max()) if t.size else 0


@functools.lru_cache(maxsize=None)
def solve_batch(shape, seed):
    """generate_batch with problem K_EMPTY's bounds moved to 5 either side of its unconstrained optimum (of the warm step's too) and problem K_INF made infeasible;
    f2: the f of the warm step"""
    n, m, ms, na = shape
    q = O.generate_batch(SOLVE_N, n, m, ms, na, seed)
    xu = -np.linalg.solve(q["H"][K_EMPTY], q["f"][K_EMPTY])
    cx = np.concatenate([xu[:ms], q["A"][K_EMPTY] @ xu])
    q["bupper"][K_EMPTY], q["blower"][K_EMPTY] = cx + 5.0, cx - 5.0
    # general row 1 = -(general row 0) with a x <= b on one and a x >= b + 1 on the other: the bounds of every row are in order, so the
    # setup accepts the problem and the SOLVE kernel is what finds it infeasible (crossed bounds are refused by the setup: iter 0, and
    # nothing is written to x and lam)
    q["A"][K_INF, 1] = -q["A"][K_INF, 0]
    q["bupper"][K_INF, ms + 1] = -q["bupper"][K_INF, ms] - 1.0
    q["blower"][K_INF, ms + 1] = q["bupper"][K_INF, ms + 1] - 1.0
    q["f2"] = q["f"] + 0.02 * np.random.default_rng([seed, 1]).standard_normal((SOLVE_N, n))
    return _freeze(q)


if __name__ == "__main__":      # the search that REFINE_DRAWS records
    ora = O.Oracle()
    n, m, ms = REFINE_SHAPE
    for k in (BIG, None, SMALL):
        best = None
        for fill in np.linspace(0.06, 0.5, 23):
            for seed in range(4):
                p = RC.make(n, m, ms, seed, float(fill), k=k)
                cond = np.linalg.cond(p["H"])
                if not (3 * RC.COND_RANGE[0] <= cond <= RC.COND_RANGE[1] / 3):
                    continue
                x, lam, flag, ids, low = RC.oracle_solution(ora, p)
                if flag != 1 or not np.array_equal(ids, p["W"]) or not np.array_equal(low[:-1], p["lower"][:-1]):
                    continue
                e0 = RC.error(p, x, lam)
                if best is None or e0 > best[0]:
                    xm, lm, steps, _, _ = RC.refine_model(p, x, lam)
                    if RC.error(p, xm, lm) <= 2.0 ** -49:
                        best = (e0, seed, float(fill), cond, RC.error(p, xm, lm), steps)
        print(k, best, flush=True)
