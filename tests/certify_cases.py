"""Constructed cases and an EXACT reference for the device certificate (daqp_certify_batch, daqp_amd/csrc/certify.hip.h).

exact(...) evaluates every output of the certificate on the float64 inputs as they are, in integer arithmetic (every double is an
integer times a power of two: no rounding anywhere), and returns each real-valued output as a Fraction next to the bound the
accuracy contract of include/daqp_amd.h allows the device for it:

    a sum of K terms with S = sum |terms|:   |computed - exact| <= 2^-52 |exact| + (K + 2)^2 2^-104 S
    a max over rows / columns:               the largest bound among the entries that can decide the max

The builders return problems whose exact certificate is known by construction:
  (a) kkt_point       H, A, x, lam dyadic rationals, f = -Hx - C'lam and the active bounds = c_k x, all exactly representable:
                      every residual is exactly 0, wrong_sign is 0
  (b) DEFECTS         the same with one planted defect of known exact size
  (c) cancellation    the terms of Hx + f + C'lam are of size 2^40 and every component sums to 2^-20 exactly; the builder asserts that
                      plain float64 evaluation misses that by more than the contract's bound
  (d) rays            infeasible polyhedra with a known Farkas ray in lam (two parallel rows with crossed bounds; a three-row cycle) and
                      a feasible twin
"""
import functools
from fractions import Fraction

import numpy as np

ACTIVE, LOWER, IMMUTABLE, SOFT = 1, 2, 4, 8
REAL_KEYS = ("stationarity", "stationarity_scale", "primal", "complementarity", "objective", "ray_residual", "ray_scale", "ray_support")
INT_KEYS = ("wrong_sign", "primal_row")
SHAPES = [(1, 1, 1), (1, 3, 0), (7, 20, 3), (63, 70, 63), (64, 64, 0), (64, 192, 64), (65, 80, 5), (130, 140, 2), (200, 260, 0)]
BATCHES = (1, 3, 67)
DELTA = 2.0 ** -10
U52, U104 = Fraction(1, 2 ** 52), Fraction(1, 2 ** 104)


# ------------------------------------------------------------------------------------------------------------------------------
# exact reference
def _ints(a):
    """(object array of Python ints, E): a == ints / 2^E exactly"""
    a = np.asarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError("the exact reference takes finite inputs")
    fr = [float(v).as_integer_ratio() for v in a.ravel()]
    E = max((d.bit_length() - 1 for _, d in fr), default=0)
    out = np.empty(len(fr), dtype=object)
    out[:] = [nu << (E - (d.bit_length() - 1)) for nu, d in fr]
    return out.reshape(a.shape), E


def _fr(v, E):
    return Fraction(int(v), 1 << E)


def contract_bound(value, K, S):
    return U52 * abs(value) + (K + 2) ** 2 * U104 * S


def _max_with_bound(entries, floor=None):
    """entries: [(exact value, bound)] -> (exact max, bound of the computed max, index of the first largest entry or -1 for the floor).
    |max_k c_k - max_k e_k| <= the largest bound among the entries that can be or beat the maximum."""
    best, arg = (floor, -1) if floor is not None else (None, -1)
    for i, (e, _) in enumerate(entries):
        if best is None or e > best:
            best, arg = e, i
    if best is None:
        return Fraction(0), Fraction(0), -1
    b_arg = entries[arg][1] if arg >= 0 else Fraction(0)
    bound = b_arg
    for e, b in entries:
        if e + b >= best - b_arg and b > bound:
            bound = b
    return best, bound, arg


def exact(H, f, A, bupper, blower, sense, ms, x, lam):
    """dict: REAL_KEYS -> (Fraction exact, Fraction bound), INT_KEYS -> int; the definitions of include/daqp_amd.h"""
    f = np.asarray(f, np.float64).ravel()
    n = f.size
    bu, bl = np.asarray(bupper, np.float64).ravel(), np.asarray(blower, np.float64).ravel()
    m = bu.size
    mA = m - ms
    sense = np.zeros(m, np.int64) if sense is None else np.asarray(sense, np.int64).ravel()
    xi, Ex = _ints(x)
    li, El = _ints(lam)
    fi, Ef = _ints(f)
    bui, Ebu = _ints(bu)
    bli, Ebl = _ints(bl)
    axi, ali = np.abs(xi), np.abs(li)
    zero = Fraction(0)
    # H x and x'Hx
    if H is None:
        hx = [zero] * n
        hx_abs = [zero] * n
        xhx = xhx_abs = zero
    else:
        Hi, EH = _ints(np.asarray(H, np.float64).reshape(n, n))
        hx = [_fr(v, EH + Ex) for v in Hi.dot(xi)]
        hx_abs = [_fr(v, EH + Ex) for v in np.abs(Hi).dot(axi)]
        xhx = _fr(xi.dot(Hi.dot(xi)), EH + 2 * Ex)
        xhx_abs = _fr(axi.dot(np.abs(Hi).dot(axi)), EH + 2 * Ex)
    # C x, C'lam, C'|lam| (the row's own sum of absolute terms next to each)
    cx = [_fr(xi[k], Ex) for k in range(ms)]
    cx_abs = [abs(v) for v in cx]
    ctl = [_fr(li[j], El) if j < ms else zero for j in range(n)]
    ctl_abs = [abs(v) for v in ctl]          # sum_k |c_kj| |lam_k|: the S of both column sums
    cta = list(ctl_abs)                      # sum_k c_kj |lam_k| (C with its signs: kkt_reference.py:116)
    if mA:
        Ai, EA = _ints(np.asarray(A, np.float64).reshape(mA, n))
        aAi = np.abs(Ai)
        cx += [_fr(v, EA + Ex) for v in Ai.dot(xi)]
        cx_abs += [_fr(v, EA + Ex) for v in aAi.dot(axi)]
        g = Ai.T.dot(li[ms:])
        ga = aAi.T.dot(ali[ms:])
        ctl = [ctl[j] + _fr(g[j], EA + El) for j in range(n)]
        ctl_abs = [ctl_abs[j] + _fr(ga[j], EA + El) for j in range(n)]
        gs = Ai.T.dot(ali[ms:])
        cta = [cta[j] + _fr(gs[j], EA + El) for j in range(n)]
    fj = [_fr(v, Ef) for v in fi]
    lamf = [_fr(v, El) for v in li]
    buf = [_fr(v, Ebu) for v in bui]
    blf = [_fr(v, Ebl) for v in bli]
    out = {}
    Kcol = mA + 1
    # stationarity
    Kst = n + 1 + mA + 1
    ent = [(abs(hx[j] + fj[j] + ctl[j]), contract_bound(hx[j] + fj[j] + ctl[j], Kst, hx_abs[j] + abs(fj[j]) + ctl_abs[j])) for j in range(n)]
    out["stationarity"] = _max_with_bound(ent)[:2]
    ent = [(abs(hx[j]), contract_bound(hx[j], n, hx_abs[j])) for j in range(n)] + [(abs(v), zero) for v in fj] \
        + [(abs(cta[j]), contract_bound(cta[j], Kcol, ctl_abs[j])) for j in range(n)]
    out["stationarity_scale"] = _max_with_bound(ent, floor=Fraction(1))[:2]
    ent = [(abs(ctl[j]), contract_bound(ctl[j], Kcol, ctl_abs[j])) for j in range(n)]
    out["ray_residual"] = _max_with_bound(ent)[:2]
    ent = [(abs(cta[j]), contract_bound(cta[j], Kcol, ctl_abs[j])) for j in range(n)]
    out["ray_scale"] = _max_with_bound(ent)[:2]
    # rows
    prim, prim_rows, comp = [], [], []
    wrong = 0
    support = support_abs = zero
    for k in range(m):
        Krow = (1 if k < ms else n) + 1
        over, under = cx[k] - buf[k], blf[k] - cx[k]
        b_over = contract_bound(over, Krow, cx_abs[k] + abs(buf[k]))
        b_under = contract_bound(under, Krow, cx_abs[k] + abs(blf[k]))
        soft, imm = bool(sense[k] & SOFT), bool(sense[k] & IMMUTABLE)
        equality = imm and bu[k] == bl[k]
        ignored = imm and not equality
        nz, upper = lamf[k] != 0, lamf[k] > 0
        if not ignored and not (soft and nz):
            prim.append((over, b_over) if over >= under else (under, b_under))
            prim_rows.append(k)
        if equality:
            comp.append((abs(over), b_over))
        elif nz and not soft:
            comp.append((abs(over), b_over) if upper else (abs(under), b_under))
        if nz and not equality and ((over >= under) != upper):
            wrong += 1
        if nz:
            t = lamf[k] * (buf[k] if upper else blf[k])
            support += t
            support_abs += abs(t)
    pv, pb, parg = _max_with_bound(prim, floor=zero)
    out["primal"] = (pv, pb)
    out["primal_row"] = prim_rows[parg] if (parg >= 0 and pv > 0) else -1
    out["complementarity"] = _max_with_bound(comp, floor=zero)[:2]
    out["wrong_sign"] = wrong
    fx = sum((fj[j] * _fr(xi[j], Ex) for j in range(n)), zero)
    fx_abs = sum((abs(fj[j] * _fr(xi[j], Ex)) for j in range(n)), zero)
    obj = xhx / 2 + fx
    out["objective"] = (obj, contract_bound(obj, n * n + n, xhx_abs / 2 + fx_abs))
    out["ray_support"] = (support, contract_bound(support, max(m, 1), support_abs))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# builders: dict(H, f, A, bupper, blower, sense, x, lam, ms, kind) of ONE problem, float64 / int32
def _dyadic(rng, shape, lo, hi, den):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64) / den


def kkt_point(n, m, ms, seed):
    """(a): an exact KKT point.  H = (B B' + (n + 1) I) / 16 with B in {-1, 0, 1}; A in {-4..4} / 4; x in {-8..8} / 8; lam in
    +-{1..8} / 8 on the active rows.  Every product and sum below stays far inside 53 bits, so the float64 arithmetic of the builder
    is exact (exact() confirms it: tests/test_cpu_certify.py)."""
    rng = np.random.default_rng([seed, n, m, ms])
    mA = m - ms
    B = rng.integers(-1, 2, size=(n, n)).astype(np.float64)
    H = (B @ B.T + (n + 1) * np.eye(n)) / 16.0
    A = _dyadic(rng, (mA, n), -4, 4, 4.0)
    x = _dyadic(rng, n, -8, 8, 8.0)
    C = np.vstack([np.eye(n)[:ms], A]) if m else np.zeros((0, n))
    cx = C @ x
    lam = np.zeros(m)
    sense = np.zeros(m, np.int32)
    bu = cx + _dyadic(rng, m, 1, 16, 8.0)
    bl = cx - _dyadic(rng, m, 1, 16, 8.0)
    order = rng.permutation(m)
    n_act = min(m, max(4, n // 3))      # all four kinds of active row wherever m >= 4
    for i, k in enumerate(order[:n_act]):
        mag = float(rng.integers(1, 9)) / 8.0
        kind = i % 4
        if kind == 0:        # on its upper bound
            lam[k], bu[k], sense[k] = mag, cx[k], ACTIVE
        elif kind == 1:      # on its lower bound
            lam[k], bl[k], sense[k] = -mag, cx[k], ACTIVE | LOWER
        elif kind == 2:      # an equality
            lam[k], bu[k], bl[k], sense[k] = (mag if rng.integers(2) else -mag), cx[k], cx[k], ACTIVE | IMMUTABLE
        else:                # a soft row beyond its upper bound: not held, no complementarity, the sign still has to name the nearer bound
            lam[k], bu[k], sense[k] = mag, cx[k] - 0.25, SOFT
    rest = order[n_act:]
    if len(rest) > 0:        # an IMMUTABLE row that is no equality is never held: violated here, and it must not count
        k = rest[0]
        sense[k], bu[k] = IMMUTABLE, cx[k] - 0.5
    if len(rest) > 1:        # a soft row without a multiplier is held like a hard one
        sense[rest[1]] = SOFT
    f = -(H @ x) - C.T @ lam
    return dict(H=H, f=f, A=A, bupper=bu, blower=bl, sense=sense, x=x, lam=lam, ms=ms, kind="kkt_point")


def _free_rows(p):
    """rows of a kkt_point without multiplier and without sense bits (hard, inactive)"""
    return [k for k in range(p["lam"].size) if p["lam"][k] == 0 and p["sense"][k] == 0]


def defect_x(p):
    """x_j moved by DELTA (j = n // 2): stationarity = DELTA max_i |H_ij| unless a row's c_kj is in the way -- exact() says what it is"""
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    q["x"][q["x"].size // 2] += DELTA
    q["kind"] = "defect_x"
    return q


def defect_sign(p):
    """the multiplier of the first active hard inequality flipped: wrong_sign = 1, stationarity = 2 |lam_k| max_j |c_kj|"""
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    rows = [k for k in range(q["lam"].size) if q["lam"][k] != 0 and not (q["sense"][k] & (IMMUTABLE | SOFT))]
    q["planted_row"] = rows[0] if rows else -1
    if rows:
        q["lam"][rows[0]] = -q["lam"][rows[0]]
    q["kind"] = "defect_sign"
    return q


def defect_bound(p):
    """the upper bound of an inactive hard row pulled DELTA inside: primal = DELTA at that row"""
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    rows = _free_rows(q)
    q["planted_row"] = rows[-1] if rows else -1
    if rows:
        k = rows[-1]
        cxk = q["x"][k] if k < q["ms"] else q["A"][k - q["ms"]] @ q["x"]
        q["bupper"][k] = cxk - DELTA
    q["kind"] = "defect_bound"
    return q


def defect_equality(p):
    """an equality row's bounds moved off c_k x by DELTA: complementarity = primal = DELTA"""
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    rows = [k for k in range(q["lam"].size) if (q["sense"][k] & IMMUTABLE) and q["bupper"][k] == q["blower"][k]]
    q["planted_row"] = rows[0] if rows else -1
    if rows:
        q["bupper"][rows[0]] += DELTA
        q["blower"][rows[0]] += DELTA
    q["kind"] = "defect_equality"
    return q


DEFECTS = (defect_x, defect_sign, defect_bound, defect_equality)


def _big(rng, shape):
    """odd 30-bit integers with random signs, times 2^-10: about 2^20, products of two of them about 2^40 with 60 significant bits"""
    v = (rng.integers(2 ** 29, 2 ** 30, size=shape) | 1).astype(np.float64)
    return v * rng.choice([-1.0, 1.0], size=shape) * 2.0 ** -10


def plain_float64_stationarity(p):
    """max_j |(Hx + f + C'lam)_j| in plain float64, two ways: numpy's products, and one accumulator per component fed term by term in
    the order of the device kernel (H row, f, simple bound, rows of A)"""
    H, f, A, x, lam, ms = p["H"], p["f"], p["A"], p["x"], p["lam"], p["ms"]
    n = f.size
    C = np.vstack([np.eye(n)[:ms], A.reshape(-1, n)])
    r1 = (H @ x + f) + C.T @ lam
    r2 = np.zeros(n)
    for j in range(n):
        s = 0.0
        for i in range(n):
            s += H[j, i] * x[i]
        s += f[j]
        if j < ms:
            s += lam[j]
        for k in range(A.shape[0]):
            s += A[k, j] * lam[ms + k]
        r2[j] = s
    return float(np.abs(r1).max()), float(np.abs(r2).max())


def cancellation(n, m, ms, seed):
    """(c): every term of Hx + C'lam is about 2^40 (60-bit products), T_j their exact sum; f_j = -fl(T_j) and one more small term --
    entry j of an absorbing row of A with multiplier 1, or lam_j itself where every variable has a simple bound and there is no
    general row -- carries fl(T_j) - T_j + 2^-20, which is exactly representable.  So every component of the residual is 2^-20
    exactly.  Bounds are wide open (+-2^60)."""
    rng = np.random.default_rng([seed, n, m, ms, 3])
    mA = m - ms
    H, x = _big(rng, (n, n)), _big(rng, n)
    A = _big(rng, (mA, n))
    lam = np.zeros(m)
    lam[ms:] = _big(rng, mA)
    absorb_row = mA >= 1
    if absorb_row:
        lam[:ms] = _big(rng, ms) * 2.0 ** 20
        A[-1], lam[-1] = 0.0, 1.0
    else:
        assert ms == n, "without a general row every variable needs a simple bound to absorb the rounding error of f"
    q = dict(H=H, f=np.zeros(n), A=A, bupper=np.full(m, 2.0 ** 60), blower=np.full(m, -2.0 ** 60), sense=np.zeros(m, np.int32), x=x, lam=lam, ms=ms)
    Hi, EH = _ints(H)
    xi, Ex = _ints(x)
    T = [_fr(v, EH + Ex) for v in Hi.dot(xi)]
    if mA:
        Ai, EA = _ints(A)
        li, El = _ints(lam)
        g = Ai.T.dot(li[ms:])
        T = [T[j] + _fr(g[j], EA + El) for j in range(n)]
        if absorb_row:
            T = [T[j] + (Fraction(float(lam[j])) if j < ms else 0) for j in range(n)]
    target = Fraction(1, 2 ** 20)
    f = np.array([-float(t) for t in T])
    rest = [target - T[j] - Fraction(float(f[j])) for j in range(n)]
    restf = np.array([float(r) for r in rest])
    assert all(Fraction(float(v)) == r for v, r in zip(restf, rest)), "the absorbed rounding errors must be representable"
    if absorb_row:
        A[-1] = restf
    else:
        lam[:ms] = restf
    q["f"] = f
    q["kind"] = "cancellation"
    ref = exact(**_args(q))
    assert ref["stationarity"][0] == target, ref["stationarity"][0]
    for plain in plain_float64_stationarity(q):      # what makes the GPU test able to fail for an uncompensated kernel
        assert abs(Fraction(plain) - target) > ref["stationarity"][1], (plain, float(ref["stationarity"][1]))
    return q


def ray_cases(n, m, ms, seed):
    """(d): [parallel rows with crossed bounds (m - ms >= 2), a three-row cycle (m - ms >= 3), the cycle's feasible twin], each with lam = the
    ray and the rows embedded among ordinary ones; shapes with fewer general rows give fewer cases"""
    rng = np.random.default_rng([seed, n, m, ms, 4])
    mA = m - ms
    base = kkt_point(n, m, ms, seed + 1)
    out = []

    def fresh(kind):
        q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        q["lam"][:] = 0.0
        q["sense"][:] = 0
        q["kind"] = kind
        return q
    if mA >= 2:
        q = fresh("ray_parallel")
        r = sorted(rng.choice(mA, size=2, replace=False))
        q["A"][r[1]] = q["A"][r[0]]
        k0, k1 = ms + r[0], ms + r[1]
        q["bupper"][k0], q["blower"][k0] = 0.5, -4.0          # a x <= 1/2
        q["bupper"][k1], q["blower"][k1] = 4.0, 0.75          # a x >= 3/4
        q["lam"][k0], q["lam"][k1] = 1.5, -1.5
        q["expect_support"] = Fraction(3, 2) * Fraction(1, 2) - Fraction(3, 2) * Fraction(3, 4)
        out.append(q)
    if mA >= 3:
        for kind, b3 in (("ray_cycle", -1.0), ("ray_cycle_feasible_twin", 0.25)):
            q = fresh(kind)
            r = sorted(rng.choice(mA, size=3, replace=False))
            q["A"][r[2]] = -(q["A"][r[0]] + q["A"][r[1]])
            for i, b in zip(r, (0.25, -0.5, b3)):
                q["bupper"][ms + i], q["blower"][ms + i] = b, -8.0
                q["lam"][ms + i] = 0.5
            q["expect_support"] = Fraction(1, 2) * (Fraction(1, 4) - Fraction(1, 2) + Fraction(b3))
            out.append(q)
    return out


def _args(q):
    return {k: q[k] for k in ("H", "f", "A", "bupper", "blower", "sense", "ms", "x", "lam")}


@functools.lru_cache(maxsize=None)
def pool(shape):
    """every constructed problem of a shape with its exact certificate: [(problem dict, exact dict)] (read-only, shared by the tests)"""
    n, m, ms = shape
    base = kkt_point(n, m, ms, 11)
    probs = [base] + [d(base) for d in DEFECTS] + [cancellation(n, m, ms, 12)] + ray_cases(n, m, ms, 13)
    for q in probs:
        for v in q.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return [(q, exact(**_args(q))) for q in probs]


def stack(problems, N):
    """N problems, the list repeated cyclically, stacked as certify_batch takes them"""
    sel = [problems[i % len(problems)] for i in range(N)]
    return {k: np.stack([q[k] for q in sel]) for k in ("H", "f", "A", "bupper", "blower", "sense", "x", "lam")}


def within(value, ref):
    """a device value against (exact, bound)"""
    return abs(Fraction(float(value)) - ref[0]) <= ref[1]
