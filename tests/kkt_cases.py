"""Case families of the KKT certificate tests (tests/kkt_reference.py), as data: which shape reaches which solve kernel under which
environment, how its problems are drawn, and the bars the certificate is held to.  tests/test_cpu_kkt_reference.py runs the oracle
over every family (bars, formulas, coverage conditions); tests/test_gpu_kkt.py runs the GPU over the same problems.

The shapes are the ones other GPU test files already tie to a kernel (test_gpu_fast_mode, test_gpu_image_kernel, test_gpu_hand_over,
test_gpu_wg_tier, test_gpu_branches).  With two soft rows (ns_max = 2) a working set may hold n + 3 rows: for n >= 62 the sense and
degenerate variants of a one-wave family are served by the kernel behind it (hand-over / workgroup) -- they stay in the list, the
certificate does not care which kernel produced the numbers.
"""
import functools

import numpy as np

from oracle import oracle as O

VARIANTS = ("plain", "sense", "degenerate")
NS_MAX = 2
RHO_SOFT = 1e-6          # the default settings' value (oracle.default_settings)
PRIMAL_TOL = 1e-6

# name, data set (families that differ only in their environment share one), shape (n, m, ms, n_active), N, environment, kernel meant
FAMILIES = [
    dict(name="tiny", shape=(12, 48, 12, 6), N=16, env={}, kernel="k_tiny_setup + k_ldp_reg"),
    dict(name="reg20", shape=(20, 40, 0, 8), N=16, env={}, kernel="k_ldp_reg", soft_push=4.0),
    dict(name="reg21", shape=(21, 33, 4, 7), N=16, env={}, kernel="k_ldp_reg<1,13>", soft_push=6.0),
    dict(name="reg26", shape=(26, 64, 26, 10), N=16, env={}, kernel="k_ldp_reg<1,13>, every variable bounded", soft_push=6.0),
    dict(name="rows193", shape=(16, 193, 4, 6), N=12, env={}, kernel="k_ldp_reg<4,8>", soft_push=0.3),
    dict(name="blk41", shape=(41, 90, 20, 12), N=12, env={}, kernel="k_setup_blk with bounds", soft_push=6.0),
    dict(name="blk63", shape=(63, 140, 63, 20), N=12, env={}, kernel="k_setup_blk with bounds", soft_push=16.0),
    dict(name="reg64", shape=(64, 128, 8, 30), N=12, env={"DAQP_AMD_REG_ROWS": "14"}, kernel="k_ldp_reg<2,32> + hand-over", soft_push=8.0),
    dict(name="img3", shape=(50, 150, 10, 20), N=12, env={"DAQP_AMD_IMG_MIN_BATCH": "1"}, kernel="image kernel, three row blocks", soft_push=6.0),
    dict(name="img3c", data="img3", shape=(50, 150, 10, 20), N=12, env={"DAQP_AMD_IMG_MIN_BATCH": "1", "DAQP_AMD_IMG_CACHE": "4"},
         kernel="image kernel, three row blocks, four cached rows"),
    dict(name="img2", shape=(60, 120, 8, 20), N=12, env={"DAQP_AMD_IMG_MIN_BATCH": "1"}, kernel="image kernel, two row blocks", soft_push=8.0),
    dict(name="img2c", data="img2", shape=(60, 120, 8, 20), N=12, env={"DAQP_AMD_IMG_MIN_BATCH": "1", "DAQP_AMD_IMG_CACHE": "4"},
         kernel="image kernel, two row blocks, four cached rows"),
    dict(name="generic", data="reg20", shape=(20, 40, 0, 8), N=16, env={"DAQP_AMD_STREAM_M": "1"}, kernel="k_ldp"),
    dict(name="spill", shape=(24, 60, 6, 8), N=12, env={"DAQP_AMD_STREAM_M": "1", "DAQP_AMD_FORCE_SPILL": "1"}, kernel="k_ldp, spilled", soft_push=4.0),
    dict(name="wg70", shape=(70, 160, 5, 25), N=8, env={}, kernel="k_ldp_wg, inverse factor", soft_push=8.0),
    dict(name="wg70L", data="wg70", shape=(70, 160, 5, 25), N=8, env={"DAQP_AMD_WG_INVERSE": "0"}, kernel="k_ldp_wg, substitution chains"),
    dict(name="wg130", shape=(130, 300, 0, 50), N=3, env={}, kernel="k_ldp_wg", soft_push=12.0),
    dict(name="rows520", shape=(258, 520, 6, 70), N=2, env={}, kernel="k_ldp, eight chunks, HBM scratch", soft_push=24.0),
]
# the proximal loop (singular Hessian; LP): no q_k, no soft rows -- the certificate in the problem's own units
PROX_FAMILIES = [
    dict(name="singular12", kind="singular", shape=(12, 30, 2), N=8),
    dict(name="singular24", kind="singular", shape=(24, 50, 0), N=8),
    dict(name="lp12", kind="lp", shape=(12, 30, 2), N=8),
    dict(name="lp24", kind="lp", shape=(24, 50, 0), N=8),
]
WARM_FAMILIES = ("reg21", "img3", "wg70", "generic")
SHARED_FAMILIES = ("reg21", "img3", "wg70")
SINGLE_CASES = (("reg26", "plain"), ("wg70", "plain"), ("blk41", "sense"))

# Seeds: data set k of FAMILIES (in order of first appearance) draws problem j of variant v from default_rng([SEED0 + k, v, j]) (plain:
# O.generate_batch(seed = SEED0 + k)).  SEEDS overrides SEED0 + k where the first draw missed a coverage condition of
# tests/test_cpu_kkt_reference.py.
#
# Soft rows: generate_nasty puts a soft row's upper bound up to 0.2 below the generator's optimum.  With the default rho_soft = 1e-6 such a
# row is active (lam != 0) in every problem, but its slack rho_soft q_k lam_k^2 is 3e-11 ... 4e-7 -- below primal_tol in every problem of every
# family but tiny and rows193, so the reference reports OPTIMAL, not SOFT_OPTIMAL.  soft_push multiplies that distance per family so that
# part of each sense and degenerate family ends SOFT_OPTIMAL (slack > primal_tol) with multipliers of order 1 ... 10.  Pushing further makes
# more problems SOFT_OPTIMAL, but at a vertex of hard rows with lam ~ 1e5 (see "Conditioning" below), where in addition the reference's
# refinement step (auxiliary.c:498-593) corrects lam and keeps the soft slack of the unrefined lam.  A search over soft_push in 1 ... 16
# (rows520: to 64, rows193: 0.3 ... 0.8) and 13 seeds per family (the family's first seed, then 7000 ... 7011), keeping only draws that meet
# every other condition of test_coverage and the 1e-10 formula check, took per family the pair with the largest share of SOFT_OPTIMAL
# problems; the shares it reached (sense, degenerate) out of the problems with an active soft row:
#   tiny 4/16 1/16, reg20 4/16 6/16, reg21 8/16 4/16, reg26 3/16 4/16, rows193 3/11 0/12, blk41 2/12 2/12, blk63 7/12 7/12, reg64 9/12 7/12,
#   img3 5/12 6/12, img2 3/12 3/12, spill 7/12 3/12, wg70 4/8 4/8, wg130 2/3 2/3, rows520 1/2 1/2.
# No family reaches "every problem"; test_coverage asserts at least one SOFT_OPTIMAL problem per family and variant, rows193/degenerate
# excepted (none found).
SEED0 = 5100
#
# Conditioning: where the soft rows cannot be met inside the hard rows, the optimum sits at a vertex with multipliers of 1e3 ... 1e5 on a
# pivot of ~ rho_soft, and the ORACLE's own lam moves by 1e-7 when f and the bounds change by 1e-13 relative (the size of the default
# mode's LDP difference): no arithmetic can be held to |dlam| < 1e-8 there.  test_coverage therefore requires, on the oracle alone, that
# such a perturbation leaves flag and iterations as they are and moves lam by less than 1e-9 (PROBE_*).  SEED0 + k missed that in 4 of
# 16 problems of tiny/sense and in 5 of rows193/sense and degenerate (and, for rows193, left every simple bound inactive): tiny takes
# the first seed from 6200 on that meets every condition; for rows193 (16 variables inside 189 general rows) none of 600 seeds did
# until the soft rows' bounds were moved to 0.3 of their distance from the generator's optimum (soft_push) -- then 6214.
SEEDS = {"tiny": 6205, "rows193": 6214, "reg20": 7005, "reg21": 7011, "reg26": 7000, "blk41": 7006, "blk63": 7004, "img3": 7003, "img2": 7007, "spill": 7007, "wg70": 7003, "wg130": 7001, "rows520": 7003}
PROBE_REL, PROBE_LAM = 1e-13, 1e-9


def perturbed(p, seed=1):
    """the family's problems with f and the bounds changed by PROBE_REL relative"""
    rng = np.random.default_rng(seed)
    out = dict(p)
    for key in ("f", "bupper", "blower"):
        out[key] = p[key] * (1.0 + PROBE_REL * rng.uniform(-1.0, 1.0, p[key].shape))
    return out


def _data_names():
    out = []
    for fam in FAMILIES:
        d = fam.get("data", fam["name"])
        if d not in out:
            out.append(d)
    return out


DATA_SETS = _data_names()


def family(name):
    return next(f for f in FAMILIES + PROX_FAMILIES if f["name"] == name)


def seed_of(data):
    return SEEDS.get(data, SEED0 + DATA_SETS.index(data))


@functools.lru_cache(maxsize=None)
def problems(name, variant):
    """dict(H (N,n,n), f, A, bupper, blower, sense (N,m) int32 or None, n, m, ms, N, ns_max, degenerate) of a family; read-only"""
    fam = family(name)
    data = fam.get("data", name)
    n, m, ms, na = fam["shape"]
    N, seed = fam["N"], seed_of(data)
    if variant == "plain":
        q = O.generate_batch(N, n, m, ms, na, seed)
        out = {k: q[k] for k in ("H", "f", "A", "bupper", "blower")}
        out.update(sense=None, ns_max=0)
    else:
        qs = []
        for j in range(N):
            rng = np.random.default_rng([seed, VARIANTS.index(variant), j])
            if variant == "sense":
                q = O.generate_nasty(n, m, ms, na, 1e-2, rng, n_dup=0, n_eq=2, n_soft=2)
            else:
                eps = 10.0 ** rng.uniform(-10, -3)
                q = O.generate_nasty(n, m, ms, na, eps, rng, n_dup=3, n_eq=0, n_soft=2)
            push = family(data).get("soft_push", 1.0)
            if push != 1.0:      # a soft row's upper bound lies (0.2 rand) below the generator's optimum: keep only this part of that distance
                soft = np.flatnonzero((q["sense"] & O.SOFT) != 0)
                at_x = q["A"][soft - ms] @ q["x"]
                q["bupper"][soft] = at_x - push * (at_x - q["bupper"][soft])
                q["blower"][soft] = q["bupper"][soft] - 1.0
            qs.append(q)
        out = {k: np.stack([q[k] for q in qs]) for k in ("H", "f", "A", "bupper", "blower", "sense")}
        out.update(ns_max=NS_MAX)
    out.update(n=n, m=m, ms=ms, N=N, degenerate=(variant == "degenerate"))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def prox_problems(name):
    fam = family(name)
    n, m, ms = fam["shape"]
    N = fam["N"]
    seed = SEED0 + 100 + PROX_FAMILIES.index(fam)
    if fam["kind"] == "lp":
        qs = [O.generate_lp(n, m, ms, [seed, j]) for j in range(N)]
        keys = ("f", "A", "bupper", "blower", "sense")
    else:
        qs = [O.generate_singular_qp(n, m, ms, rank=n // 2 + j % 3, rng=[seed, j], kind="dense") for j in range(N)]
        keys = ("H", "f", "A", "bupper", "blower", "sense")
    out = {k: np.stack([q[k] for q in qs]) for k in keys}
    out.setdefault("H", None)
    out.update(n=n, m=m, ms=ms, N=N, ns_max=0, degenerate=False)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


WARM_SALT = {("img3", "sense"): 80}     # (family, variant) -> stream of the warm steps where 77 left the oracle's own solution of a step ill determined


def warm_steps(name, variant):
    """the three warm steps of test_kkt_warm: [(what changed, dict(f, bupper, blower))]: f + 0.05 N(0, 1), both bounds + 0.02 N(0, 1), f again"""
    fam, p = family(name), problems(name, variant)
    rng = np.random.default_rng([seed_of(fam.get("data", name)), WARM_SALT.get((fam.get("data", name), variant), 77)])
    data = dict(f=p["f"].copy(), bupper=p["bupper"].copy(), blower=p["blower"].copy())
    out = []
    for step in range(3):
        if step == 1:
            shift = 0.02 * rng.standard_normal(data["bupper"].shape)
            data = dict(data, bupper=data["bupper"] + shift, blower=data["blower"] + shift)
        else:
            data = dict(data, f=data["f"] + 0.05 * rng.standard_normal(data["f"].shape))
        out.append(("d" if step == 1 else "v", data))
    return out


def problem(p, k):
    """(H, f, A, bupper, blower, sense) of problem k of a family's dict"""
    return (None if p["H"] is None else p["H"][k], p["f"][k], p["A"][k], p["bupper"][k], p["blower"][k],
            None if p["sense"] is None else p["sense"][k])


def oracle_models(oracle, p, init_mask=0):
    """one OracleModel per problem, set up (init_mask 0: setup_daqp as BatchModel.setup calls it; 64 + 128: daqp_quadprog's)"""
    models = []
    for k in range(p["N"]):
        om = oracle.model(p["n"], p["m"], p["ms"], ns=p["ns_max"])
        flag = om.setup(*problem(p, k), init_mask=init_mask)
        assert flag >= 0, (k, flag)
        models.append(om)
    return models


def oracle_solve(models):
    """dict(x, lam, fval, exitflag, iter, soft_slack) of one solve of every model, stacked like BatchModel.solve's"""
    rs = [om.solve(with_soft=True) for om in models]
    return dict(x=np.stack([r[0] for r in rs]), lam=np.stack([r[1] for r in rs]), fval=np.array([r[2] for r in rs]),
                exitflag=np.array([r[3] for r in rs], np.int32), iter=np.array([r[4] for r in rs], np.int32),
                soft_slack=np.array([r[5] for r in rs]))


def bar_from(worst, lo=1e-13, hi=None):
    """100 x the oracle's worst value, rounded up to a power of ten, not below lo, not above hi"""
    b = max(lo, 10.0 ** np.ceil(np.log10(100.0 * worst))) if worst > 0 else lo
    return float(b if hi is None else min(b, hi))


# Obtained by `python tests/test_cpu_kkt_reference.py`: the certificate of the oracle's own (x, lam), worst value over all families and
# variants -> bar = bar_from(worst): 100 x worst rounded up to a power of ten, within [1e-13, the solver's tolerance for that quantity].
# fval / soft_slack: |value - value_ref| / max(1, |value_ref|).  (worst, bar)
BARS = {
    "qp": {
        "stationarity": (2.2e-15, 1e-12),
        "primal": (3.3e-07, 1e-06),
        "complementarity": (2.0e-10, 1e-07),
        "soft_relation": (5.9e-14, 1e-11),
        "fval": (1.4e-14, 1e-11),
        "soft_slack": (2.8e-19, 1e-13),
    },
    "prox": {       # (stationarity: eta_prox stops the outer loop, it holds to that and no better)
        "stationarity": (2.0e-11, 1e-08),
        "primal": (5.7e-10, 1e-07),
        "complementarity": (5.7e-10, 1e-07),
        "fval": (3.5e-11, 1e-08),
    },
}
CAPS = {"qp": dict(stationarity=None, primal=PRIMAL_TOL, complementarity=PRIMAL_TOL, soft_relation=PRIMAL_TOL, fval=1e-8, soft_slack=1e-8),
        "prox": dict(stationarity=None, primal=PRIMAL_TOL, complementarity=PRIMAL_TOL, fval=1e-8)}
