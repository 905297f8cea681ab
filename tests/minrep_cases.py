"""Polyhedra {x : A x <= b} whose redundant rows are known BY CONSTRUCTION, each verdict with a certificate that numpy checks in
np.longdouble -- no solver, no GPU, no reference build is involved in the truth (tests/test_cpu_minrep_truth.py,
tests/test_gpu_minrep_truth.py).

Construction, make_case(n, m, ms, delta, gamma, seed), mA = m - ms general rows:
  * core rows (truth 0): the ms simple bounds e_i and ncore = min(mA, max(n + 1, mA // 2)) unit rows u_j, right-hand side
    b_j = 1 + u_j . c for a centre c.  x_j = c + u_j lies on face j and has slack 1 - u_k . u_j on every other core row k: the
    WITNESS that row j is not redundant.  Rows are drawn by rejection so that u_k . u_j <= 0.95 for every pair, except that every
    fourth core row is a planted near-parallel partner w of the row u before it, u . w = 1 - gamma (and w . u_k <=
    min(0.95, 1 - gamma) for every other k): both rows of a pair are not redundant, with witness slack gamma.
  * redundant rows (truth 1): r = sum_t w_t core[k_t] over three distinct core rows (simple bounds included), w_t in [0.2, 1],
    right-hand side sum_t w_t b_{k_t} + delta |r|.  The combination (k_t, w_t) is the FARKAS certificate: every x of the polyhedron
    has r . x <= rhs - delta |r|.
  * where ms > 0, two of the bounds e_i are also added as general core rows (right-hand side 1 + c_i), and the simple bound itself
    is lifted to 1 + c_i + delta: its truth becomes 1, the certificate is that one general row with weight 1.
  * general rows are scaled by 10**U(-2, 2) and permuted; |c| = CENTRE * sqrt(n), so about a quarter of the b are negative and
    the origin lies outside the polyhedron.

verify(case) checks, in np.longdouble and in normalised units (rows of unit length): every witness lies on its face (|slack| <=
1e-12) with slack >= 0.9 min(gamma, 0.05) on every other core row and >= 0.9 delta on every redundant row (the lifted bound beside
its general twin has slack delta at the twin's witness, by construction: no more can be asked there); every Farkas combination
reproduces its row to 1e-13 |r| with non-negative weights on core rows and clears the bound by >= 0.9 delta.

CPU figures this file rests on (the reference's daqp_minrep, strict-IEEE build, default settings: primal_tol 1e-6):
  measured with |c| = 2, 8 shapes from (3, 12, 0) to (130, 300, 0), gamma in {1e-1, 1e-3, 1e-5}, 2-6 seeds per shape:
    rows normalised, delta >= 3e-5: every verdict equals the truth (0 wrong of about 8000); delta = 1e-6: up to 2 redundant rows per
    shape missed.  Rows raw (scales 1e-2 .. 1e2): correct at delta >= 1e-3, 1 miss in 1200 at (80, 200, 5) and delta = 1e-4, many
    misses at delta <= 3e-5.  A core row was never called redundant, at any delta or gamma, raw or normalised.
  measured with the centre used here, |c| = 1.5 sqrt(n), on exactly the cases of this file (SHAPES x (CLEAR_ALL + NEAR) x SEEDS,
  `python tests/golden/make_golden_minrep_truth.py --measure`), 3360 rows per delta, about 1500 of them redundant:
    rows normalised: every verdict equals the truth at delta = 1e-1, 1e-2, 1e-3, 1e-4, 3e-5, 1e-5 and 3e-6; at 1e-6, 19 redundant
    rows missed (at most 3 per polyhedron).  Rows raw: 0 / 0 / 3 / 0 misses at the four clear deltas (the 3 at (50, 150, 10),
    delta 1e-3), then 82 / 229 / 382 / 515 at the near ones.  No core row called redundant anywhere.  20.8 % of the b are negative.
    So the larger centre costs the reference nothing: CENTRE stays at the 1.5 asked for, and no seed had to be replaced.
So CLEAR_ALL = {1e-1, 1e-2, 1e-3, 1e-4} on normalised rows (>= 100 primal_tol, 3x above where the reference still holds) must be
answered with the truth; NEAR = {3e-5, 1e-5, 3e-6, 1e-6} may miss a redundant row but never drops a core row.
"""
import functools

import numpy as np

# |c| = CENTRE * sqrt(n): the value the construction asks for; the reference answers every clear case with it (figures above), so
# there was no reason to lower it
CENTRE = 1.5
REPLACED_SEEDS = {}       # (n, m, ms, delta, seed) -> replacement seed, with the reason beside each entry; none were needed

GAMMAS = (1e-1, 1e-3, 1e-5)
CLEAR_ALL = (1e-1, 1e-2, 1e-3, 1e-4)      # the reference check on the CPU
CLEAR = (1e-1, 1e-3, 1e-4)                # the GPU tests
NEAR = (3e-5, 1e-5, 3e-6, 1e-6)
SEEDS = (0, 1)                            # P = 2 polyhedra per call
# (n, m, ms): smallest | every variable bounded | one row block | one row past it | four row blocks | simple bounds | image-kernel
# shape | n <= 64 edge with bounds | n = 64 | bounds on every variable at the lane limit | workgroup kernel, with and without bounds
SHAPES = [(3, 12, 0), (6, 40, 6), (8, 64, 0), (8, 65, 0), (16, 193, 4), (12, 130, 12), (50, 150, 10), (63, 140, 63), (64, 256, 0),
          (64, 130, 64), (80, 200, 5), (130, 300, 0)]


def _unit(v):
    return v / np.linalg.norm(v)


def make_case(n, m, ms, delta, gamma, seed):
    """dict: A (mA, n), b (m,) as given to the solver; truth (m,) int32; witness {row: x}; farkas {row: (rows, weights)} in the
    frame of A, b (row indices count the simple bounds first); pairs: list of (row, row) planted near-parallel"""
    rng = np.random.default_rng([1009, n, m, ms, int(round(-np.log10(delta) * 100)), int(round(-np.log10(gamma) * 100)), seed])
    mA = m - ms
    ncore = min(mA, max(n + 1, mA // 2))
    c = _unit(rng.standard_normal(n)) * CENTRE * np.sqrt(n)
    E = np.eye(n)[:ms]
    twins = list(rng.choice(ms, 2, replace=False)) if ms > 0 else []
    core = [E[i].copy() for i in twins]                    # general core rows, unit length
    pairs = []
    while len(core) < ncore:
        j = len(core)
        others = np.vstack([E] + [u[None] for u in core]) if (ms or core) else np.zeros((0, n))
        for _ in range(10000):
            if j % 4 == 3:                                 # partner of the row before it
                u = core[j - 1]
                v = rng.standard_normal(n)
                v = _unit(v - (v @ u) * u)
                w = (1.0 - gamma) * u + np.sqrt(gamma * (2.0 - gamma)) * v
                w = _unit(w)
                dots = others @ w
                # (row j - 1 sits at others[ms + j - 1]; a twin e_i has the simple bound e_i in E at dot 1: the bound is lifted)
                mask = np.ones(len(others), bool)
                mask[ms + j - 1] = False
                if np.all(dots[mask] <= min(0.95, 1.0 - gamma)):
                    pairs.append((j - 1, j))
                    break
            else:
                w = _unit(rng.standard_normal(n))
                if np.all(others @ w <= 0.95):
                    break
        else:
            raise RuntimeError(f"no core row found for {(n, m, ms, delta, gamma, seed)}")
        core.append(w)
    U = np.vstack(core)
    bU = 1.0 + U @ c
    bS = 1.0 + c[:ms]
    truthS = np.zeros(ms, np.int32)
    for i in twins:
        bS[i] += delta
        truthS[i] = 1
    # every truth-0 row in one list: ("s", i) simple bounds that stayed, ("g", j) general core rows
    pool = [("s", i) for i in range(ms) if truthS[i] == 0] + [("g", j) for j in range(ncore)]
    prow = {("s", i): E[i] for i in range(ms)}
    prow.update({("g", j): U[j] for j in range(ncore)})
    prhs = {("s", i): bS[i] for i in range(ms)}
    prhs.update({("g", j): bU[j] for j in range(ncore)})
    rows, rhs, comb = [U], [bU], []
    for _ in range(mA - ncore):
        k = [pool[t] for t in rng.choice(len(pool), 3, replace=False)]
        w = rng.uniform(0.2, 1.0, 3)
        r = sum(wt * prow[kt] for wt, kt in zip(w, k))
        rows.append(r[None])
        rhs.append(np.array([sum(wt * prhs[kt] for wt, kt in zip(w, k)) + delta * np.linalg.norm(r)]))
        comb.append((k, w))
    G, bG = np.vstack(rows), np.concatenate(rhs)
    s = 10.0 ** rng.uniform(-2.0, 2.0, mA)
    perm = rng.permutation(mA)                             # new position t holds old row perm[t]
    pos = np.empty(mA, np.int64)
    pos[perm] = np.arange(mA)
    A, bA = (G * s[:, None])[perm], (bG * s)[perm]
    gid = lambda key: key[1] if key[0] == "s" else ms + int(pos[key[1]])      # noqa: E731
    gscale = lambda key: 1.0 if key[0] == "s" else s[key[1]]                  # noqa: E731
    truth = np.concatenate([truthS, np.zeros(mA, np.int32)])
    witness, farkas = {}, {}
    for i in range(ms):
        if truthS[i] == 0:
            witness[i] = c + E[i]
    for j in range(ncore):
        witness[ms + int(pos[j])] = c + U[j]
    for t, i in enumerate(twins):
        farkas[int(i)] = ([gid(("g", t))], np.array([1.0 / s[t]]))
    for q, (k, w) in enumerate(comb):
        old = ncore + q
        truth[ms + pos[old]] = 1
        farkas[ms + int(pos[old])] = ([gid(kt) for kt in k], np.array([s[old] * wt / gscale(kt) for wt, kt in zip(w, k)]))
    return dict(n=n, m=m, ms=ms, delta=delta, gamma=gamma, seed=seed, A=np.ascontiguousarray(A), b=np.concatenate([bS, bA]),
                truth=truth, witness=witness, farkas=farkas, pairs=[(ms + int(pos[a]), ms + int(pos[bb])) for a, bb in pairs])


def full_rows(case, dtype=np.float64):
    """all m rows (simple bounds as unit vectors first) and b, in dtype"""
    E = np.eye(case["n"], dtype=dtype)[:case["ms"]]
    return np.vstack([E, case["A"].astype(dtype)]), case["b"].astype(dtype)


def normalised(case):
    """(A_i * s_i, b_i * s_i), s_i = 1 / sqrt(sum_k A_ik^2): the rows as the GPU path sees them, in its order of operations (the
    squares summed in column order, one reciprocal of one square root, one multiplication per entry; no fused multiply-add)"""
    A = case["A"]
    ss = np.zeros(A.shape[0])
    for k in range(A.shape[1]):
        ss = ss + A[:, k] * A[:, k]
    scal = 1.0 / np.sqrt(ss)
    b = case["b"].copy()
    b[case["ms"]:] = b[case["ms"]:] * scal
    return np.ascontiguousarray(A * scal[:, None]), b


def verify(case):
    """the certificates, in np.longdouble; raises AssertionError naming the row"""
    L = np.longdouble
    R, b = full_rows(case, L)
    nrm = np.sqrt((R * R).sum(axis=1))
    truth, delta, gamma = case["truth"], L(case["delta"]), L(case["gamma"])
    assert set(case["witness"]) == set(np.flatnonzero(truth == 0).tolist()), "a truth-0 row without a witness"
    assert set(case["farkas"]) == set(np.flatnonzero(truth == 1).tolist()), "a truth-1 row without a Farkas combination"
    core_margin = L(0.9) * min(gamma, L(0.05))
    for j, x in case["witness"].items():
        slack = (b - R @ x.astype(L)) / nrm
        assert abs(slack[j]) <= 1e-12, ("witness off its face", j, float(slack[j]))
        other = np.arange(case["m"]) != j
        lo0 = slack[other & (truth == 0)].min() if (other & (truth == 0)).any() else L(1)
        assert lo0 >= core_margin, ("witness slack on a core row", j, float(lo0))
        if (truth == 1).any():
            lo1 = slack[truth == 1].min()
            assert lo1 >= L(0.9) * delta, ("witness slack on a redundant row", j, float(lo1))
    for j, (k, w) in case["farkas"].items():
        w = w.astype(L)
        assert len(set(k)) == len(k) and j not in k and (truth[k] == 0).all() and (w > 0).all(), ("Farkas rows / weights", j)
        res = R[j] - w @ R[k]
        assert np.sqrt((res * res).sum()) <= 1e-13 * nrm[j], ("Farkas combination does not give the row", j)
        clear = (b[j] - w @ b[k]) / nrm[j]
        assert clear >= L(0.9) * delta, ("Farkas margin", j, float(clear))


def gamma_of(shape, delta, seed):
    """gamma cycles over GAMMAS across seeds, shapes and deltas"""
    deltas = CLEAR_ALL + NEAR
    return GAMMAS[(seed + SHAPES.index(shape) + deltas.index(delta)) % 3]


@functools.lru_cache(maxsize=None)
def cases(shape, delta):
    """the P = len(SEEDS) polyhedra of a shape and a delta"""
    n, m, ms = shape
    out = []
    for seed in SEEDS:
        seed = REPLACED_SEEDS.get((n, m, ms, delta, seed), seed)
        out.append(make_case(n, m, ms, delta, gamma_of(shape, delta, seed % len(SEEDS)), seed))
    return tuple(out)


MIXED_SHAPES = [(8, 65, 0), (50, 150, 10), (80, 200, 5)]
_MIXED = ((1e-1, 1e-5, 11), (1e-3, 1e-1, 12), (1e-4, 1e-3, 13), (1e-2, 1e-5, 14), (1e-4, 1e-1, 15), (1e-3, 1e-3, 16))


@functools.lru_cache(maxsize=None)
def mixed(shape):
    """six unlike polyhedra of one shape for one call: (delta, gamma, seed) all different, every delta clear"""
    return tuple(make_case(*shape, delta, gamma, seed) for delta, gamma, seed in _MIXED)


def with_zero_rows(case, shift=0):
    """the case with three vanishing rows of A inserted (b = 5 there): A, b, the expected verdicts (-1 at the new rows, the truth
    elsewhere).  shift = 0: they end up as the first, a middle and the last general row; shift = 1: one row further inside, so
    that two polyhedra of one call have them at different places"""
    ms, mA = case["ms"], case["A"].shape[0]
    at = np.array([shift, mA // 2, mA - shift])            # positions in the rows as they are
    A = np.insert(case["A"], at, 0.0, axis=0)
    b = np.insert(case["b"], ms + at, 5.0)
    want = np.insert(case["truth"], ms + at, -1)
    assert (np.flatnonzero(want == -1) == ms + np.array([shift, mA // 2 + 1, mA + 2 - shift])).all()
    assert not A[want[ms:] == -1].any() and (np.abs(A[want[ms:] != -1]).sum(axis=1) > 0).all()
    return np.ascontiguousarray(A), b, want


def stack(cs):
    """A (P, mA, n), b (P, m), truth (P, m)"""
    return (np.ascontiguousarray(np.stack([c["A"] for c in cs])), np.ascontiguousarray(np.stack([c["b"] for c in cs])),
            np.stack([c["truth"] for c in cs]))


def fixture_key(shape, delta):
    return f"{shape[0]}_{shape[1]}_{shape[2]}_{delta:.0e}"
