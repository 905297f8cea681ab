"""Planted near-ties for the fp32 screening scans -- numpy and the oracle only, no GPU.

The three default-arithmetic solve paths that decide a feasibility scan from an fp32 image of M (rscan_rows_img in
csrc/wave_ldp_reg.hip.h with IMG = 1 and the split-block IMG = 2, the image-only shapes, wg_scan32 / wscan in csrc/wg_ldp.hip.h)
accept an fp32 verdict only outside an error band E and run the fp64 scan otherwise.  On random draws hardly a scan reaches the
band, so a wrong band picks the same rows as a right one.  The cases built here put a second row's slack within
delta * |u| of the decisive quantity of one scan, delta from far below fp32 roundoff to beyond 2E, and keep only the cases the
oracle resolves the same way in two fp64 arithmetics.

Reference quantities (np.longdouble, no solver code)
----------------------------------------------------
H = L L', Y = L^-1 C' (C = [I_ms ; A]), g = L^-1 f.  nu_r = |Y[:, r]| is the norm of row r in the least-distance coordinates, M_r =
Y[:, r]' / nu_r its unit row there.  For a working set W with sides (b_W: the upper or lower bound of each row) the equality-
constrained QP in the QP's own coordinates is the system tests/kkt_reference.py states,

    [[H, C_W'], [C_W, -S]] [x; lam] = [-f; b_W],        S = diag(rho_soft q_r) on active SOFT rows, 0 elsewhere, q_r = nu_r^2,

solved through its Schur complement (Y_W'Y_W + S) lam = -(b_W + Y_W'g), y = L'x = -(g + Y_W lam).  Then c_r x = Y[:, r]'y, the
normalised slacks of every row are (bupper_r - c_r x)/nu_r and (c_r x - blower_r)/nu_r, u = y + g and |u|^2 + rho_soft sum q_r lam_r^2
is the level the oracle records at that scan (enable_levels) -- compared to 1e-9 relative for every case.  The working set before
an event comes from replaying the oracle's event trace; the side of every added row is the violated one at the replayed iterate.

Kinds of case (DELTAS x SIGMAS each)
------------------------------------
pick       scan k >= 1 of a cold solve (u != 0; every second base problem prefers a scan that follows a remove event): r1 the
           oracle's pick, r2 the row with the smallest slack among rows that appear nowhere in the trace before k; r2's bound is moved
           so that its slack is s(r1) + sigma delta |u_k|.  sigma = -1: r2 becomes the pick.
threshold  the final scan: r2 never active, its bound moved so that its slack is -primal_tol scaling_r + sigma delta |u|
           (scaling from oracle.model(...).ldp(), the threshold reg_kernel.hip.h stores as ep * scr).  sigma = -1: one more
           iteration at least; sigma = +1: the solve stops where it stopped.
warm       the pick tie at the first scan of a second solve after update(f) (UPDATE_v), working set carried over.
scale-3, scale+3   the pick tie with (f, bounds) scaled by 1e-3 / 1e3: x and u scale, M does not, delta stays relative to |u_k|.

Validation: the trace before the scan is unchanged, the event at the scan is the intended row and side (the side read from the
oracle stopped right after the event), Oracle(fast=True) and the exact oracle agree on the whole trace, the exit flag and the
iteration count, no branch marker (pivot, singular, refine, repair) occurs.  Anything else is dropped, and build() raises unless
every (family, kind, delta, sigma) cell keeps CAP_SMALL = 24 problems (n <= 64) or CAP_WG = 8 (workgroup shapes).

Survival (valid / attempted variants, the worst cell of each family and kind; measured on the CPU with the seeds below)
-----------------------------------------------------------------------------------------------------------------------
  family              pick       threshold  warm       scale-3    scale+3    
  img2-50x150         24/68      24/24      24/61      24/66      24/64      
  img2-17x129         24/75      24/25      24/53      24/57      24/94      
  img1-50x161         24/40      24/27      24/41      24/43      24/37      
  img1-63x128         24/49      24/24      24/39      24/43      24/40      
  img1-60x120-bounds  24/92      24/27      24/56      24/101     24/98      
  imgonly-40x256      24/47      24/25      24/42      24/48      24/44      
  imgonly-63x320      24/45      24/24      24/64      24/34      24/39      
  wg-65x150           8/20       8/9        8/14       8/10       8/19       
  wg-130x300          8/58       8/9        8/51       8/58       8/56       
  soft-50x150         24/58      24/24      24/60      24/40      24/70      
  (cells of one kind share their base problems, so all 14 cells of a family and kind survive at nearly the same rate; the first
   number is the cap because build() stops drawing once every cell is full)

Share of cases with delta <= 2^-30 that a numpy float32 model of the scan (M and u rounded to float32, float32 dot product, fp64
bounds) mis-orders or mis-judges (tests/test_cpu_scan_ties.py asserts >= 0.25 per family)
  family              pick       threshold  warm       scale-3    scale+3    
  img2-50x150         47/96      46/96      47/96      47/96      48/96      
  img2-17x129         47/96      47/96      48/96      47/96      47/96      
  img1-50x161         48/96      46/96      48/96      47/96      48/96      
  img1-63x128         47/96      42/96      48/96      48/96      48/96      
  img1-60x120-bounds  47/96      41/96      47/96      48/96      46/96      
  imgonly-40x256      45/96      44/96      47/96      48/96      48/96      
  imgonly-63x320      46/96      46/96      45/96      46/96      47/96      
  wg-65x150           16/32      15/32      16/32      14/32      14/32      
  wg-130x300          16/32      16/32      14/32      16/32      16/32      
  soft-50x150         45/96      44/96      47/96      46/96      48/96      

Worst-case fp32 error of the three scans, derived from the code (eps = 2^-24, first order in eps; |M_r| = 1)
----------------------------------------------------------------------------------------------------------
Every scan forms fl(sum_j m~_j u~_j) with m~_j = fl32(M_rj), u~_j = fl32(u_j): two rounded operands per term, (1 + eps)^2 on each
product.  A chain of K fused multiply-adds into one accumulator rounds each term's contribution at most K times (the product itself
is not rounded); d further additions combine the accumulators.  Hence

    |fl32(M_r . u) - M_r . u| <= (K + d + 2) eps sum_j |M_rj u_j| <= (K + d + 2) eps |u|        (Cauchy-Schwarz, unit rows).

Both conversions to fp64 afterwards (mu, and du - mu in fp64) are exact or belong to the fp64 scan's own noise.  Underflow of a
u~_j or of a partial sum adds at most n 2^-126 in absolute terms, below the fp64 rounding of du - mu for any du the thresholds
(primal_tol * scaling) can tell from zero; the coded bands add 1e-37 / 1e-300 and are not claimed to cover it.

  rscan_rows_img, full blocks (IMG = 1, IMG = 2 rows < 128, the image-only shapes): two accumulators ax / ay, one fma per column pair
    and accumulator: K = NP; msum = ax + ay: d = 1.                              derived (NP + 3) eps |u|; coded 1.0002 (NP + 8) eps |u|
  rscan_rows_img, split block of IMG = 2 (two lanes per row): K = NPH = (NP + 1) / 2 per lane and accumulator; part = ax + ay, both = part +
    (DPP swap of the other lane's part): d = 2; the permute to the row's own lane moves bits.   derived (NPH + 4) eps |u| = 17 eps |u| for NP = 25
  wg_scan32, DAQP_WG_SCAN_U_REGS = 1: four accumulators a0..a3, each one fma per quad of columns.  Whole blocks: K = nquad =
    ceil(ceil(n / 2) / 2), (a0 + a1) + (a2 + a3): d = 2.  Left-over blocks (cut into batches of 16 quads over all waves, partial sums
    through LDS): K = min(16, nquad), d = 2 per batch, then nb - 1 <= 3 additions in batch order with nquad > 16 (nb - 1): K + d <=
    nquad + 2.  u is read from registers by lane; quads past the row meet u = 0 and add exact zeros.
  wg_scan32, DAQP_WG_SCAN_U_REGS = 0: the same four chains of nquad terms over whole blocks (u from an fp32 copy in LDS), the repeated
    last load multiplied by an exact 0: K = nquad, d = 2.                        derived (nquad + 4) eps |u|; coded 1.001 (nquad + 8) eps |u|
  The image kernels take |u| as sqrtf((float)(fval - soft) * 1.0000003f): fval - soft = |u|^2 up to the fp64 rounding of the two sums
  (relative 2^-52 (1 + soft / |u|^2)), the conversion and the square root round by 2 eps in all: inside the factor 1.0002 while
  soft / |u|^2 < 1e11.  wscan sums the squares of u itself.

No derived bound exceeds the coded band, so no E was changed.  (n/4 + 8 in the comment above wg_scan32 is nquad + 8 in the code;
nquad >= n / 4.)
"""
import collections
import functools

import numpy as np

from oracle import oracle as O
import kkt_reference as K

LD = np.longdouble
DELTAS = tuple(2.0 ** -e for e in (34, 30, 27, 24, 21, 18, 14))
SIGMAS = (1, -1)
KINDS = ("pick", "threshold", "warm", "scale-3", "scale+3")
CAP_SMALL, CAP_WG = 24, 8
RHO_SOFT, PRIMAL_TOL = 1e-6, 1e-6           # the default settings every case runs under
LEVEL_RTOL = 1e-9

# id -> n, m, ms, n_active of the generator, SOFT rows, intended path (a key of daqp_batch_describe that must read 1), IMG argument
FAMILIES = {
    "img2-50x150": dict(n=50, m=150, ms=0, na=20, ns=0, path="img32", img_kind=2),
    "img2-17x129": dict(n=17, m=129, ms=0, na=6, ns=0, path="img32", img_kind=2),
    "img1-50x161": dict(n=50, m=161, ms=0, na=20, ns=0, path="img32", img_kind=1),
    "img1-63x128": dict(n=63, m=128, ms=0, na=30, ns=0, path="img32", img_kind=1),
    "img1-60x120-bounds": dict(n=60, m=120, ms=8, na=20, ns=0, path="img32", img_kind=1),
    "imgonly-40x256": dict(n=40, m=256, ms=0, na=14, ns=0, path="img_only", img_kind=0),
    "imgonly-63x320": dict(n=63, m=320, ms=0, na=25, ns=0, path="img_only", img_kind=0),
    "wg-65x150": dict(n=65, m=150, ms=0, na=30, ns=0, path="has_m32", img_kind=0),
    "wg-130x300": dict(n=130, m=300, ms=5, na=40, ns=0, path="has_m32", img_kind=0),
    "soft-50x150": dict(n=50, m=150, ms=0, na=20, ns=2, path="img32", img_kind=2),
}
SEED = 77100
WHY = collections.Counter()    # why base problems and variants were dropped (diagnostics for the survival table)
MAX_BASES = 400          # base problems tried per (family, kind) before build() gives up


def cap_of(fam):
    return CAP_SMALL if FAMILIES[fam]["n"] <= 64 else CAP_WG


# ---- the longdouble reference ---------------------------------------------------------------------------------------------------
def _backward_solve(L, b):
    """x with L' x = b"""
    n = L.shape[0]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


class Reference:
    """the fixed part of one base problem: Y = L^-1 C', nu, q"""

    def __init__(self, H, A, ms):
        n = H.shape[0]
        self.L = K.cholesky(H)
        self.Y = K.forward_solve(self.L, K.constraint_matrix(A, ms, n).T.copy())
        self.q = (self.Y * self.Y).sum(axis=0)
        self.nu = np.sqrt(self.q)

    def g(self, f):
        return K.forward_solve(self.L, np.array(f, dtype=LD).reshape(-1, 1))[:, 0]

    def eqp(self, g, bu, bl, sense, W):
        """the equality-constrained QP on W = [(row, upper?)]: normalised slacks of every row, |u|, u, the level"""
        if W:
            rows = np.array([r for r, _ in W])
            b = np.array([bu[r] if up else bl[r] for r, up in W], dtype=LD)
            Yw = self.Y[:, rows]
            S = np.where((sense[rows] & O.SOFT) != 0, LD(RHO_SOFT) * self.q[rows], LD(0))
            G = Yw.T @ Yw + np.diag(S)
            Lg = K.cholesky(G)
            lam = _backward_solve(Lg, K.forward_solve(Lg, (-(b + Yw.T @ g)).reshape(-1, 1))[:, 0])
            u = -(Yw @ lam)
            soft = (S * lam * lam).sum()
        else:
            u, soft = np.zeros_like(g), LD(0)
        cx = self.Y.T @ (u - g)
        su = (np.array(bu, dtype=LD) - cx) / self.nu
        sl = (cx - np.array(bl, dtype=LD)) / self.nu
        return dict(su=su, sl=sl, s=np.minimum(su, sl), cx=cx, u=u, unorm=np.sqrt(u @ u), level=u @ u + soft)


def replay(ref, g, bu, bl, sense, trace, W0=()):
    """the scans behind the add events of `trace`, from working set W0; returns (scans, final working set).  A scan: dict(pos, W, out, row, up)"""
    W, scans = list(W0), []
    for pos, e in enumerate(trace):
        r = abs(int(e)) - 1
        if e > 0:
            out = ref.eqp(g, bu, bl, sense, W)
            up = bool(out["su"][r] < out["sl"][r])
            scans.append(dict(pos=pos, W=list(W), out=out, row=r, up=up))
            W.append((r, up))
        else:
            hit = [i for i, (rr, _) in enumerate(W) if rr == r]
            if len(hit) != 1:
                raise ValueError("trace removes a row that is not active")
            del W[hit[0]]
    return scans, W


# ---- the oracle runs ----------------------------------------------------------------------------------------------------------------
def run_oracle(ora, fam, q, f2=None, stop_after=None, levels=False):
    """cold solve of q (and, with f2, update(UPDATE_v) + a second solve): per solve (trace with markers, x, lam, flag, iterations); the
    levels of the last solve; with stop_after = p the last solve ends right after its event p and the sense words are returned too"""
    F = FAMILIES[fam]
    md = ora.model(F["n"], F["m"], F["ms"], F["ns"])
    if md.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"]) < 0:
        return None
    solves = []
    for stage, f in enumerate((q["f"],) if f2 is None else (q["f"], f2)):
        last = stage == (0 if f2 is None else 1)
        if stage == 1 and md.update(O.UPDATE_v, f=f) != 0:
            return None
        if last and stop_after is not None:
            md.settings(iter_limit=stop_after + 2)
        md.enable_trace(4096)
        if last and levels:
            md.enable_levels(4096)
        r = md.solve()
        solves.append(dict(trace=md.get_trace(marks=True), x=r[0], lam=r[1], flag=r[3], iter=r[4]))
    out = dict(solves=solves)
    if levels:
        out["levels"] = md.get_levels()
    if stop_after is not None:
        out["sense"] = md.state()[1]
    return out


def _clean(tr):
    return len(tr) > 0 and int(np.abs(tr).max()) < O.TRACE_MARK


def _same_run(a, b):
    return all(np.array_equal(x["trace"], y["trace"]) and x["flag"] == y["flag"] and x["iter"] == y["iter"] for x, y in zip(a["solves"], b["solves"]))


# ---- base problems ------------------------------------------------------------------------------------------------------------------
def base_problem(ora, fam, kind, idx):
    F = FAMILIES[fam]
    n, m, ms = F["n"], F["m"], F["ms"]
    q = O.generate_qp(n, m, ms, F["na"], rng=[SEED, sorted(FAMILIES).index(fam), KINDS.index(kind), idx])
    q = {k: q[k] for k in ("H", "f", "A", "bupper", "blower", "sense")}
    f2 = None
    if kind.startswith("scale"):
        s = 1e-3 if kind == "scale-3" else 1e3
        q["f"], q["bupper"], q["blower"] = q["f"] * s, q["bupper"] * s, q["blower"] * s
    if kind == "warm":
        f2 = q["f"] + 0.05 * np.random.default_rng([SEED + 1, idx]).standard_normal(n)
    if F["ns"]:
        # two rows of the optimal working set become SOFT: they stay active (a soft row sits rho_soft q lam beyond its bound)
        r = run_oracle(ora, fam, q)
        if r is None or r["solves"][0]["flag"] != 1:
            return None
        act = np.flatnonzero(r["solves"][0]["lam"] != 0)
        if act.size < F["ns"]:
            return None
        q["sense"] = q["sense"].copy()
        q["sense"][act[:: max(1, act.size // F["ns"])][: F["ns"]]] = O.SOFT
    return q, f2


def _region(fam, r):
    """the block class of a row: 'split' (two lanes per row, IMG = 2), 'bound' (a simple bound), 'full'"""
    F = FAMILIES[fam]
    if F["img_kind"] == 2 and r >= 128:
        return "split"
    return "bound" if r < F["ms"] else "full"


def _wanted(fam, idx):
    """(region wanted for r1 or None, region wanted for r2 or None) of base problem idx: the placements the issue names"""
    F = FAMILIES[fam]
    if F["img_kind"] == 2 and F["m"] - 128 > 1:
        return (("split", "split"), ("full", "full"), ("full", "split"), ("split", "full"))[idx % 4]
    if F["img_kind"] == 2:
        return (None, "split") if idx % 2 == 0 else (None, "full")       # one row in the split block: r2 sits there or not
    if F["ms"]:
        return (None, "bound") if idx % 2 == 0 else (None, None)
    return (None, None)


def _moved(q, r2, up2, value):
    q2 = dict(q)
    q2["bupper"], q2["blower"] = q["bupper"].copy(), q["blower"].copy()
    near, far = (q2["bupper"], q2["blower"]) if up2 else (q2["blower"], q2["bupper"])
    far[r2] += float(value) - near[r2]          # the row keeps its width: the far side only moves further off
    near[r2] = float(value)
    return q2


def variants_of_base(ora, ora_fast, fam, kind, idx):
    """every (delta, sigma) variant of base problem idx: list of (delta, sigma, case or None)"""
    F = FAMILIES[fam]
    none = [(d, s, None) for d in DELTAS for s in SIGMAS]
    bp = base_problem(ora, fam, kind, idx)
    if bp is None:
        return none
    q, f2 = bp
    base = run_oracle(ora, fam, q, f2, levels=True)
    if base is None or not all(_clean(s["trace"]) for s in base["solves"]) or base["solves"][-1]["flag"] not in (1, 2):
        return none
    if f2 is not None and base["solves"][0]["flag"] not in (1, 2):
        return none
    ref = Reference(q["H"], q["A"], F["ms"])
    sense = np.asarray(q["sense"], np.int64)
    bu, bl = q["bupper"], q["blower"]
    W0, seen = [], set()
    if f2 is not None:
        tr0 = base["solves"][0]["trace"]
        _, W0 = replay(ref, ref.g(q["f"]), bu, bl, sense, tr0)
        seen = {abs(int(e)) - 1 for e in tr0}
    g = ref.g(q["f"] if f2 is None else f2)
    tr = base["solves"][-1]["trace"]
    try:
        scans, Wend = replay(ref, g, bu, bl, sense, tr, W0)
    except ValueError:
        return none
    adds = [i for i, e in enumerate(tr) if e > 0]
    if len(base["levels"]) != len(adds) + 1:
        return none
    want1, want2 = _wanted(fam, idx)
    if kind == "threshold":
        out = ref.eqp(g, bu, bl, sense, Wend)
        pos, level = len(tr), base["levels"][-1]
        r1 = None
    else:
        if kind == "warm":
            cand = scans[:1] if scans and scans[0]["W"] else []
        else:
            cand = [s for s in scans if s["pos"] >= 1 and s["W"]]
        if F["ns"]:
            cand = [s for s in cand if any(sense[r] & O.SOFT for r, _ in s["W"])]
        if want1:
            cand = [s for s in cand if _region(fam, s["row"]) == want1] or cand
        after_remove = [s for s in cand if s["pos"] >= 1 and tr[s["pos"] - 1] < 0]
        if idx % 2 == 1 and after_remove:
            cand = after_remove
        if not cand:
            return none
        sc = cand[len(cand) // 2]
        out, pos, r1 = sc["out"], sc["pos"], sc["row"]
        level = base["levels"][adds.index(pos)]
        seen |= {abs(int(e)) - 1 for e in tr[:pos]}
    if abs(float(out["level"]) - level) > LEVEL_RTOL * max(abs(level), 1e-300) or not out["unorm"] > 0:
        return none
    open_ = np.ones(F["m"], bool)
    open_[[r for r, _ in (sc["W"] if r1 is not None else Wend)]] = False
    open_[(sense & O.IMMUTABLE) != 0] = False
    s = np.where(open_, out["s"], LD(np.inf))
    if r1 is not None:
        if int(np.argmin(s)) != r1:
            return none                      # the reference's own pick is not the oracle's: not a case to plant a tie on
        s1 = s[r1]
    else:
        seen |= {abs(int(e)) - 1 for sv in base["solves"] for e in sv["trace"]}
    ok2 = open_.copy()
    ok2[list(seen)] = False
    ok2[(sense & O.SOFT) != 0] = False
    if r1 is not None:
        ok2[r1] = False
    if want2 and any(ok2[r] and _region(fam, r) == want2 for r in range(F["m"])):
        ok2 &= np.array([_region(fam, r) == want2 for r in range(F["m"])])
    if not ok2.any():
        return none
    r2 = int(np.argmin(np.where(ok2, out["s"], LD(np.inf))))
    up2 = bool(out["su"][r2] <= out["sl"][r2])
    scaling = ora_model_scaling(ora, fam, q)
    res = []
    for d in DELTAS:
        for sg in SIGMAS:
            anchor = s1 if r1 is not None else -LD(PRIMAL_TOL) * LD(scaling[r2])
            target = anchor + LD(sg) * LD(d) * out["unorm"]
            value = out["cx"][r2] + ref.nu[r2] * target if up2 else out["cx"][r2] - ref.nu[r2] * target
            q2 = _moved(q, r2, up2, value)
            case = None
            if (q2["bupper"][r2] - q2["blower"][r2]) / float(ref.nu[r2]) > 8 * DELTAS[-1] * float(out["unorm"]):      # (its side unambiguous beyond every band and every delta)
                case = _validate(ora, ora_fast, fam, kind, q2, f2, base, pos, r1, sc["up"] if r1 is not None else None, r2, up2, sg)
            if case is not None:
                M1 = None if r1 is None else (ref.Y[:, r1] / ref.nu[r1])
                case.update(fam=fam, kind=kind, delta=d, sigma=sg, base=idx, pos=pos, r1=r1, r2=r2, up2=up2, unorm=float(out["unorm"]),
                            after_remove=bool(pos >= 1 and tr[pos - 1] < 0), regions=(None if r1 is None else _region(fam, r1), _region(fam, r2)),
                            soft_active=bool(any(sense[r] & O.SOFT for r, _ in (sc["W"] if r1 is not None else Wend))),
                            model=_fp32_model(out, M1, ref.Y[:, r2] / ref.nu[r2], r1, r2, up2, target, sg, anchor))
            res.append((d, sg, case))
    return res


def ora_model_scaling(ora, fam, q):
    F = FAMILIES[fam]
    md = ora.model(F["n"], F["m"], F["ms"], F["ns"])
    md.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    return md.ldp()[5]


def _validate(ora, ora_fast, fam, kind, q2, f2, base, pos, r1, up1, r2, up2, sg):
    """the planted case against the oracle: None unless everything the module's docstring lists holds"""
    run = run_oracle(ora, fam, q2, f2)
    if run is None or not all(_clean(s["trace"]) or len(s["trace"]) == 0 for s in run["solves"]):
        return None
    if f2 is not None and not np.array_equal(run["solves"][0]["trace"], base["solves"][0]["trace"]):
        return None
    tr, btr = run["solves"][-1]["trace"], base["solves"][-1]["trace"]
    if run["solves"][-1]["flag"] not in (1, 2) or not np.array_equal(tr[:pos], btr[:pos]):
        return None
    if r1 is None:                 # threshold tie
        if sg > 0:
            if not (np.array_equal(tr, btr) and run["solves"][-1]["iter"] == base["solves"][-1]["iter"] and run["solves"][-1]["flag"] == base["solves"][-1]["flag"]):
                return None
            want_row = None
        else:
            if not (len(tr) > pos and tr[pos] == r2 + 1 and run["solves"][-1]["iter"] > base["solves"][-1]["iter"]):
                return None
            want_row, want_up = r2, up2
    else:
        want_row, want_up = (r1, up1) if sg > 0 else (r2, up2)
        if not (len(tr) > pos and tr[pos] == want_row + 1):
            return None
    if want_row is not None:       # the side: the oracle stopped right after the event
        st = run_oracle(ora, fam, q2, f2, stop_after=pos)
        if st is None or not np.array_equal(st["solves"][-1]["trace"][: pos + 1], tr[: pos + 1]):
            return None
        if bool(st["sense"][want_row] & O.LOWER) == want_up or not st["sense"][want_row] & O.ACTIVE:
            return None
    fast = run_oracle(ora_fast, fam, q2, f2)
    if fast is None or not _same_run(run, fast):
        return None
    return dict(q=q2, f2=f2, expect=run["solves"])


def _fp32_model(out, M1, M2, r1, r2, up2, target, sg, anchor):
    """a numpy float32 model of the scan on the two rows that matter: does it order r1 and r2 (or judge r2 against its threshold) as the
    planted slacks say?  mu32 = float32 dot of the rounded row and the rounded u; the slack moves by the dot product's error."""
    u = out["u"]
    u32 = u.astype(np.float64).astype(np.float32)

    def err(Mr):
        mu32 = np.dot(Mr.astype(np.float64).astype(np.float32), u32)
        return LD(np.float64(mu32)) - Mr @ u            # fl32(M_r . u) - M_r . u

    e2 = err(M2)
    s2 = target - e2 if up2 else target + e2            # upper: du - mu; lower: mu - dl
    if r1 is None:
        return bool((s2 < anchor) == (sg < 0))          # anchor: the threshold
    e1 = err(M1)
    s1 = anchor - e1 if out["su"][r1] < out["sl"][r1] else anchor + e1
    return bool((s2 < s1) == (sg < 0))


# ---- the case sets ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracles():
    return O.Oracle(), O.Oracle(fast=True)


@functools.lru_cache(maxsize=None)
def build(fam, kind):
    """(cases, stats) of one family and kind: exactly cap_of(fam) cases per (delta, sigma) cell, stats[(delta, sigma)] = (valid, attempted).
    Raises when MAX_BASES base problems do not fill every cell."""
    ora, ora_fast = _oracles()
    cap = cap_of(fam)
    cells = {(d, s): [] for d in DELTAS for s in SIGMAS}
    tried = {c: 0 for c in cells}
    valid = {c: 0 for c in cells}
    for idx in range(MAX_BASES):
        if all(len(v) >= cap for v in cells.values()):
            break
        for d, s, case in variants_of_base(ora, ora_fast, fam, kind, idx):
            tried[(d, s)] += 1
            if case is not None:
                valid[(d, s)] += 1
                if len(cells[(d, s)]) < cap:
                    cells[(d, s)].append(case)
    short = {c: len(v) for c, v in cells.items() if len(v) < cap}
    if short:
        raise RuntimeError(f"scan tie cases {fam}/{kind}: cells below the cap of {cap} after {MAX_BASES} base problems: {short}")
    cases = [c for cell in cells.values() for c in cell]
    return cases, {c: (valid[c], tried[c]) for c in cells}


def batch_arrays(cases):
    """the cases of one family as the arrays BatchModel takes (sense: None when no row is flagged)"""
    a = {k: np.stack([c["q"][k] for c in cases]) for k in ("H", "f", "A", "bupper", "blower")}
    sense = np.stack([c["q"]["sense"] for c in cases]).astype(np.int32)
    a["sense"] = sense if sense.any() else None
    a["f2"] = None if cases[0]["f2"] is None else np.stack([c["f2"] for c in cases])
    return a
