"""Inputs, oracle side and dense reference of tests/test_gpu_backward_nullspace.py (daqp_batch_backward_nullspace: the adjoint of
problems that went through the proximal loop); tests/test_cpu_backward_nullspace.py holds the same inputs to their conditions on
the oracle alone.  numpy and the oracle only; no test in this file.

Reference, per problem, in numpy fp64: np.linalg.solve on  [H C_W'; C_W 0] [dz; dnu] = [g; 0],  C = [I[:ms]; A],  H = 0 for an LP.
W and the side of each of its rows come from the ORACLE model that went through the same setup / solve (its working set and the
LOWER bits of its sense), never from the GPU."""
import numpy as np

from oracle import oracle as O

TOL = 1e-9               # relative to the max norm of [dz; dnu]: the TOL of test_gpu_backward_states.py
LAM_MIN = 1e-8           # every multiplier of a working set is at least this large: W and the sides are unambiguous
COND_MAX = 1e6           # cond_2 of every KKT matrix
SLACK_MIN = 1e-6         # every inactive row is at least this far inside its bounds
GRAD_SEED = 23
KEYS = ("f", "A", "bupper", "blower", "sense")


def _stack(qs, H=True):
    q = {k: np.stack([p[k] for p in qs]) for k in KEYS}
    q["H"] = np.stack([p["H"] for p in qs]) if H else None
    return q


def _lp(n, m, ms, N, seed):
    return _stack([O.generate_lp(n, m, ms, [seed, k]) for k in range(N)], H=False)


def _psd(n, m, ms, rank, N, seed, kind="dense", picks=None):
    """picks: the problem seeds of the batch (default 0 .. N - 1) -- those whose optimum is not a vertex, found on the oracle"""
    return _stack([O.generate_singular_qp(n, m, ms, rank, [seed, k], kind=kind) for k in (picks or range(N))])


def _definite(n, m, ms, na, N, seed):
    q = O.generate_batch(N, n, m, ms, na, seed)
    q["sense"] = np.zeros((N, m), np.int32)
    return {k: q[k] for k in KEYS + ("H",)}


def _equalities(n, m, ms, rank, N, seed):
    qs = []
    for k in range(N):
        q = O.generate_singular_qp(n, m, ms, rank, [seed, k])
        qs.append(O.add_sense_variety(q, ms, 2, 0, [seed + 1, k]))
    return _stack(qs)


def _shared(n, m, ms, rank, N, seed, kind):
    """ONE singular H and ONE A, per-problem f and bounds (the batch of test_gpu_prox.py::test_shared_singular_hessian)"""
    q0 = O.generate_singular_qp(n, m, ms, rank, [seed, n], kind=kind)
    rng = np.random.default_rng([seed + 1, n])
    shift = 0.03 * rng.standard_normal((N, m))
    return dict(H=q0["H"], A=q0["A"], f=q0["f"][None, :] + 0.2 * rng.standard_normal((N, n)), bupper=q0["bupper"][None, :] + shift,
                blower=q0["blower"][None, :] + shift, sense=np.zeros((N, m), np.int32))


def _free_optimum(n, m, ms, N, seed):
    """positive definite H, every bound far from the unconstrained optimum: W is empty, Hr is all of H (n x n)"""
    q = _definite(n, m, ms, 4, N, seed)
    for k in range(N):
        x = -np.linalg.solve(q["H"][k], q["f"][k])
        s = np.concatenate([x[:ms], q["A"][k] @ x])
        q["bupper"][k], q["blower"][k] = s + 1.0, s - 1.0
    return q


FORCED = dict(eps_prox=1e-3)      # eps_prox > 0: every problem is shifted and goes through the proximal loop, definite or not

# name -> dict(family, shape (n, m, ms), make: () -> batch, settings, shared, k: what the sizes of the working sets must be)
CASES = {
    # 1. LPs, box rows plus general rows, the optimum at a vertex
    "lp_n5": dict(family=1, shape=(5, 14, 2), make=lambda: _lp(5, 14, 2, 8, 700), k="n"),
    "lp_n16": dict(family=1, shape=(16, 40, 4), make=lambda: _lp(16, 40, 4, 8, 701), k="n"),
    "lp_n64": dict(family=1, shape=(64, 140, 10), make=lambda: _lp(64, 140, 10, 4, 702), k="n"),
    # 2. dense H = B'B of rank r < n
    "psd_n5": dict(family=2, shape=(5, 14, 2), make=lambda: _psd(5, 14, 2, 3, 8, 710, picks=(0, 3, 4, 10, 13, 16, 17, 18)), k="inner"),
    "psd_n16": dict(family=2, shape=(16, 40, 4), make=lambda: _psd(16, 40, 4, 10, 8, 711, picks=(0, 1, 2, 4, 8, 10, 11, 12)), k="inner"),
    "psd_n33": dict(family=2, shape=(33, 80, 5), make=lambda: _psd(33, 80, 5, 20, 8, 712, picks=(0, 1, 2, 3, 5, 7, 8, 9)), k="inner"),
    # 3. diagonal H with zero entries (the partial shift of the setup)
    "diag_n16": dict(family=3, shape=(16, 40, 16), make=lambda: _psd(16, 40, 16, 0, 8, 720, kind="diag"), k="any"),
    "diag_n33": dict(family=3, shape=(33, 80, 6), make=lambda: _psd(33, 80, 6, 0, 8, 721, kind="diag"), k="any"),
    # 4. positive definite H with eps_prox > 0 forced
    "forced_n2": dict(family=4, shape=(2, 6, 1), make=lambda: _definite(2, 6, 1, 1, 8, 730), settings=FORCED, k="any"),
    "forced_n16": dict(family=4, shape=(16, 40, 4), make=lambda: _definite(16, 40, 4, 6, 8, 731), settings=FORCED, k="any"),
    "forced_n64": dict(family=4, shape=(64, 100, 6), make=lambda: _definite(64, 100, 6, 30, 4, 732), settings=FORCED, k="any"),
    # 5. equality rows (sense 5) in W
    "equalities_n16": dict(family=5, shape=(16, 40, 4), make=lambda: _equalities(16, 40, 4, 10, 8, 740), k="any"),
    # 6. setup_shared with a singular H
    "shared_n12": dict(family=6, shape=(12, 30, 4), make=lambda: _shared(12, 30, 4, 6, 8, 750, "dense"), shared=True, k="any"),
    "shared_diag_n20": dict(family=6, shape=(20, 60, 0), make=lambda: _shared(20, 60, 0, 0, 8, 751, "diag"), shared=True, k="any"),
    # 7. k = 0 at n = 64: Hr is the full 64 x 64
    "free_n64": dict(family=7, shape=(64, 70, 6), make=lambda: _free_optimum(64, 70, 6, 4, 760), settings=FORCED, k="zero"),
}
FAMILIES = {1: "LP at a vertex", 2: "dense PSD", 3: "diagonal with zeros", 4: "definite, forced shift", 5: "equality rows",
            6: "shared singular H", 7: "empty working set, n = 64"}

_cache = {}


def batch(name):
    """the case's arrays (made once, shared, never modified)"""
    if name not in _cache:
        _cache[name] = CASES[name]["make"]()
    return _cache[name]


def problem(name, q, k):
    """(H or None, f, A, bupper, blower, sense) of problem k"""
    shared = CASES[name].get("shared", False)
    H = None if q["H"] is None else (q["H"] if shared else q["H"][k])
    return H, q["f"][k], (q["A"] if shared else q["A"][k]), q["bupper"][k], q["blower"][k], q["sense"][k]


def grad(N, n):
    return np.random.default_rng(GRAD_SEED).standard_normal((N, n))


def oracle_solve(oracle, name):
    """one oracle model per problem through the setup the GPU batch gets; dict(x, lam, flag, n_prox, ws: the oracle's own working
    set per problem, lower: the LOWER bit of its sense per row)"""
    c = CASES[name]
    n, m, ms = c["shape"]
    q = batch(name)
    N = q["f"].shape[0]
    out = dict(x=np.zeros((N, n)), lam=np.zeros((N, m)), flag=np.zeros(N, np.int32), n_prox=np.zeros(N, np.int32), ws=[],
               lower=np.zeros((N, m), bool))
    for k in range(N):
        H, f, A, bu, bl, sense = problem(name, q, k)
        om = oracle.model(n, m, ms, settings=O.default_settings(**c.get("settings", {})))
        if c.get("shared", False):      # the reference's MPC usage: one setup with open bounds, then the problem's own f and bounds
            assert om.setup(H, f, A, np.full(m, 1e30), np.full(m, -1e30), None) >= 0, (name, k)
            assert om.update(O.UPDATE_v | O.UPDATE_d, f=f, bupper=bu, blower=bl) == 0, (name, k)
        else:
            assert om.setup(H, f, A, bu, bl, sense) == 1, (name, k)
        out["x"][k], out["lam"][k], _, out["flag"][k], _ = om.solve()
        ws, osense, _, _ = om.state()
        out["ws"].append(np.sort(ws))
        out["lower"][k] = (osense & O.LOWER) != 0
        out["n_prox"][k] = om.prox()[0]
    return out


def kkt(H, A, ms, W, n):
    Cm = np.vstack([np.eye(n)[:ms], A.reshape(-1, n)])
    CW = Cm[W]
    Hm = np.zeros((n, n)) if H is None else H
    return np.block([[Hm, CW.T], [CW, np.zeros((len(W), len(W)))]]), Cm


def dense_adjoint(H, A, ms, W, g):
    """(dz, dnu on W) of the full KKT system, by np.linalg.solve"""
    n = g.size
    K, _ = kkt(H, A, ms, W, n)
    sol = np.linalg.solve(K, np.concatenate([g, np.zeros(len(W))]))
    return sol[:n], sol[n:]


def reference(name, ref, g):
    """per problem: dict(W sorted, dz, dnu (on W), scale)"""
    c = CASES[name]
    n, m, ms = c["shape"]
    q = batch(name)
    out = []
    for k in range(q["f"].shape[0]):
        H, f, A, bu, bl, sense = problem(name, q, k)
        W = ref["ws"][k]
        dz, dnu = dense_adjoint(H, A, ms, W, g[k])
        out.append(dict(W=W, dz=dz, dnu=dnu, scale=max(np.abs(dz).max(), np.abs(dnu).max() if len(W) else 0.0)))
    return out


def check_inputs(name, ref):
    """the input conditions of one case, on the oracle alone; returns (working-set sizes, smallest |lam| on W, largest cond_2(K),
    smallest slack of an inactive row)"""
    c = CASES[name]
    n, m, ms = c["shape"]
    q = batch(name)
    N = q["f"].shape[0]
    lam_min, cond, slack, sizes = np.inf, 0.0, np.inf, []
    for k in range(N):
        H, f, A, bu, bl, sense = problem(name, q, k)
        assert ref["flag"][k] == 1, (name, k, ref["flag"][k])
        assert ref["n_prox"][k] > 0, (name, k, "did not go through the proximal loop")
        W, lam = ref["ws"][k], ref["lam"][k]
        assert len(set(W.tolist())) == len(W) and set(np.nonzero(lam)[0].tolist()) <= set(W.tolist()), (name, k)
        if len(W):
            lam_min = min(lam_min, np.abs(lam[W]).min())
        K, Cm = kkt(H, A, ms, W, n)
        cond = max(cond, np.linalg.cond(K))
        s = Cm @ ref["x"][k]
        off = np.ones(m, bool)
        off[W] = False
        if off.any():
            slack = min(slack, (bu - s)[off].min(), (s - bl)[off].min())
        sizes.append(len(W))
        if c["family"] == 5:
            assert (sense[W] == 5).sum() == 2, (name, k, "the equality rows are not in W")
    assert lam_min >= LAM_MIN, (name, lam_min)
    assert cond <= COND_MAX, (name, cond)
    assert slack >= SLACK_MIN, (name, slack)
    sizes = np.array(sizes)
    if c["k"] == "n":
        assert (sizes == n).all(), (name, sizes)
    elif c["k"] == "inner":
        assert ((sizes > 0) & (sizes < n)).all(), (name, sizes)
    elif c["k"] == "zero":
        assert (sizes == 0).all(), (name, sizes)
    return sizes, lam_min, cond, slack


def check_adjoint(name, ref, refsol, r, na, ws, o, tag=""):
    """per problem: exit flag and status, the device's working set against the oracle's, dz and dbupper + dblower against the dense
    reference within TOL of the scale, zeros off W, every dnu on the side of its row's LOWER bit; returns the worst relative error"""
    q = batch(name)
    m = q["bupper"].shape[1]
    worst = 0.0
    for k in range(q["f"].shape[0]):
        R = refsol[k]
        W = R["W"]
        assert r["exitflag"][k] == 1 and o["status"][k] == 0, (name, tag, k, r["exitflag"][k], o["status"][k])
        assert na[k] == len(W) and sorted(ws[k, :na[k]].tolist()) == W.tolist(), (name, tag, k, ws[k, :na[k]], W)
        dnu = o["dbupper"][k] + o["dblower"][k]
        e1 = np.abs(o["dz"][k] - R["dz"]).max()
        e2 = np.abs(dnu[W] - R["dnu"]).max() if len(W) else 0.0
        worst = max(worst, e1 / R["scale"], e2 / R["scale"])
        assert e1 <= TOL * R["scale"] and e2 <= TOL * R["scale"], (name, tag, k, e1, e2, R["scale"])
        off = np.ones(m, bool)
        off[W] = False
        assert not o["dbupper"][k][off].any() and not o["dblower"][k][off].any(), (name, tag, k)
        lower = ref["lower"][k][W]
        assert not o["dblower"][k][W[~lower]].any(), (name, tag, k, "a row without the LOWER bit has a value in dblower")
        assert not o["dbupper"][k][W[lower]].any(), (name, tag, k, "a row with the LOWER bit has a value in dbupper")
    return worst


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))
