"""Inputs, oracle side and dense reference of tests/test_gpu_backward_states.py (the adjoint behind every solve kernel family and
behind warm states); tests/test_cpu_backward_states.py holds the same inputs to their conditions on the oracle alone.  numpy and
the oracle only; no test in this file.

Reference, per problem, in numpy fp64:  [H C_W'; C_W -S] [dz; dnu] = [g; 0],  C = [I[:ms]; A],  S = 0 on hard rows and
rho_soft c_k H^-1 c_k' on the SOFT rows of W.  W and the side of each of its rows come from the ORACLE model that went through the
same setup / update / solve sequence (W = {i : lam_i != 0}; upper where lam_i > 0, lower where lam_i < 0), never from the GPU."""
import importlib.util
import os

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


S = _sibling("backward_soft_cases")          # dense_adjoint, SOFT, RHO

TOL = 1e-9               # relative to the max norm of [dz; dnu], as in test_gpu_backward.py
LAM_MIN = 1e-8           # every multiplier of a working set is at least this large: W and the sides are unambiguous
COND_MAX = 1e6           # cond_2 of every KKT matrix
PREFIX = "DAQP_AMD_"
GRAD_SEED = 11

# name -> (switches without their DAQP_AMD_ prefix, (n, m, ms, n_active), problems, seed, also in exact mode, forced cap or None)
COLD = {
    "register": ({}, (20, 40, 0, 8), 32, 5100, True, None),
    "register_bounds": ({}, (12, 48, 12, 6), 32, 5101, True, None),
    "image_3x25": ({"IMG_MIN_BATCH": "1"}, (50, 150, 0, 20), 32, 5102, True, None),
    "image_3x25_bounds": ({"IMG_MIN_BATCH": "1"}, (50, 150, 10, 20), 32, 5103, True, None),
    "image_scratch_tier": ({"IMG_MIN_BATCH": "1", "IMG_ROWS": "44", "IMG_CACHE": "6"}, (50, 150, 0, 20), 32, 5102, False, None),
    "image_hand_over": ({"IMG_MIN_BATCH": "1", "IMG_ROWS": "12", "IMG_CACHE": "3"}, (50, 150, 0, 20), 32, 5102, False, 12),
    "image_2x32": ({"IMG_MIN_BATCH": "1"}, (56, 120, 0, 20), 32, 5104, False, None),
    "image_only": ({}, (64, 256, 0, 30), 24, 5105, False, None),
    "generic": ({"STREAM_M": "1"}, (20, 40, 0, 8), 32, 5100, True, None),
    "generic_spill": ({"STREAM_M": "1", "FORCE_SPILL": "1"}, (24, 60, 6, 8), 32, 5106, False, None),
    # The (2,32) register shapes with a hand-over (a forced cap, or n = 64: 65 rows).  Under these switches alone a cold solve of a
    # batch in the default arithmetic goes to the image-only kernel, which holds every row (launch_ldp: reg_handover && img_only);
    # the exact mode runs the register kernel with k_ldp behind it, and so does the default arithmetic with the image-only kernel
    # switched off (DAQP_AMD_NO_IMG_ONLY=1, as in test_gpu_image_kernel.py): the *_registers rows.  All four run in both modes.
    "register_hand_over": ({"REG_ROWS": "12"}, (56, 120, 4, 20), 32, 5107, True, 12),
    "register_hand_over_registers": ({"REG_ROWS": "12", "NO_IMG_ONLY": "1"}, (56, 120, 4, 20), 32, 5107, True, 12),
    "register_64": ({}, (64, 100, 6, 60), 24, 5108, True, None),
    "register_64_registers": ({"NO_IMG_ONLY": "1"}, (64, 100, 6, 60), 24, 5108, True, None),
    "workgroup": ({}, (70, 160, 5, 25), 24, 5109, True, None),
    "workgroup_chains": ({"WG_INVERSE": "0"}, (70, 160, 5, 25), 24, 5109, False, None),
    # the shape of test_gpu_parity.py::test_workgroup_kernel_hands_over_large_working_sets: config C4
    "workgroup_hand_over": ({"WG_CAPL": "60"}, (200, 600, 0, 80), 16, 44, False, 60),
    "workgroup_tier": ({"WG_TIER_MIN_BATCH": "1", "WG_R0": "40"}, (129, 200, 10, 30), 16, 5110, False, None),
    "one_wave_n80": ({"NO_WG": "1"}, (80, 200, 0, 30), 24, 5111, False, None),
}

# soft variants: ns_max = 2, one equality and two SOFT rows per problem (oracle.add_sense_variety), rho_soft = S.RHO
SOFT = {
    "register": ({}, (20, 40, 0, 8), 32, 5200),
    "image_3x25": ({"IMG_MIN_BATCH": "1"}, (50, 150, 0, 20), 32, 5201),
    "workgroup": ({}, (70, 160, 5, 25), 24, 5202),
}
NS_MAX = 2

# warm sequences: solve, then update + solve per step.  name -> (switches, shape, problems, seed, {step: seed of its moves})
STEPS = ("f", "bounds", "A", "H", "sense")
MASK = {"f": O.UPDATE_v, "bounds": O.UPDATE_d, "A": O.UPDATE_M, "H": O.UPDATE_Rinv, "sense": O.UPDATE_sense}
WARM = {
    "register": ({}, (20, 40, 0, 8), 32, 5300, {"f": 0, "bounds": 0, "A": 0, "H": 0, "sense": 0}),
    "image_3x25": ({"IMG_MIN_BATCH": "1"}, (50, 150, 0, 20), 32, 5301, {"f": 0, "bounds": 0, "A": 0, "H": 0, "sense": 0}),
    "workgroup": ({}, (70, 160, 5, 25), 24, 5302, {"f": 0, "bounds": 0, "A": 0, "H": 0, "sense": 0}),
}
LAYER = ({"IMG_MIN_BATCH": "1"}, (50, 150, 0, 20), 32, 5400)

KEYS = ("H", "f", "A", "bupper", "blower", "sense")


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def perturbed(q, step, rng, n, m):
    """the new arrays of one problem for `step`: the sizes of tests/test_gpu_hand_over.py::perturbed (small moves: the optimum stays
    where working sets of the same size are)"""
    if step == "H":
        P = 0.005 * rng.standard_normal((n, n))
        return dict(H=q["H"] + P @ P.T)
    if step == "A":
        return dict(A=q["A"] * (1.0 + 1e-4 * rng.standard_normal(q["A"].shape)))
    if step == "f":
        return dict(f=q["f"] + 0.02 * rng.standard_normal(n))
    if step == "bounds":
        shift = 0.005 * rng.standard_normal(m)
        return dict(bupper=q["bupper"] + shift, blower=q["blower"] + shift)
    assert step == "sense"
    return dict(sense=np.zeros(m, np.int32))


def environment(switches):
    return {PREFIX + k: v for k, v in switches.items()}


def grad(N, n):
    return np.random.default_rng(GRAD_SEED).standard_normal((N, n))


def cold_batch(shape, N, seed):
    n, m, ms, na = shape
    q = O.generate_batch(N, n, m, ms, na, seed)
    q["sense"] = np.zeros((N, m), np.int32)
    return q


def soft_batch(shape, N, seed):
    n, m, ms, na = shape
    qs = []
    for k in range(N):
        q = O.generate_qp(n, m, ms, na, rng=[seed, k])
        qs.append(O.add_sense_variety({key: q[key] for key in KEYS}, ms, 1, NS_MAX, [seed + 1, k]))
    return {key: np.stack([q[key] for q in qs]) for key in KEYS}


def settings(soft):
    return dict(rho_soft=S.RHO) if soft else {}


def warm_moves(cur, step, shape, seed, index):
    """the new arrays of `step` for every problem; cur: the batch as it stands"""
    n, m, ms, _ = shape
    N = cur["f"].shape[0]
    kws = [perturbed({key: cur[key][k] for key in KEYS}, step, np.random.default_rng([seed, k, index]), n, m) for k in range(N)]
    return {key: np.stack([kw[key] for kw in kws]) for key in kws[0]}


class OracleBatch:
    """one kept oracle model per problem: setup / update / solve, and what the adjoint check needs from each solve"""

    def __init__(self, oracle, q, ms, ns=0, soft=False, init_mask=0):
        N, n = q["f"].shape
        m = q["bupper"].shape[1]
        self.N, self.n, self.m, self.ms = N, n, m, ms
        self.models = []
        for k in range(N):
            om = oracle.model(n, m, ms, ns, settings=O.default_settings(**settings(soft)))
            assert om.setup(q["H"][k], q["f"][k], q["A"][k], q["bupper"][k], q["blower"][k], q["sense"][k], init_mask=init_mask) == 1, k
            self.models.append(om)

    def update(self, mask, kw):
        for k, om in enumerate(self.models):
            assert om.update(mask, **{key: v[k] for key, v in kw.items()}) == 0, k

    def solve(self):
        """dict(x, lam, flag, iter, ws: the oracle's own working set per problem, in its order, lower: its LOWER bit per row)"""
        out = dict(x=np.zeros((self.N, self.n)), lam=np.zeros((self.N, self.m)), flag=np.zeros(self.N, np.int32),
                   iter=np.zeros(self.N, np.int32), ws=[], lower=np.zeros((self.N, self.m), bool))
        for k, om in enumerate(self.models):
            out["x"][k], out["lam"][k], _, out["flag"][k], out["iter"][k] = om.solve()
            ws, sense, _, _ = om.state()
            out["ws"].append(ws)
            out["lower"][k] = (sense & O.LOWER) != 0
        return out


def reference(q, ref, g, ms, rho=0.0):
    """per problem: dict(W sorted, upper, dz, dnu (on W), qk, U, scale, cond) from the oracle's multipliers and a dense solve"""
    out = []
    N, n = q["f"].shape
    for k in range(N):
        lam = ref["lam"][k]
        W = np.nonzero(lam)[0]
        Cm = np.vstack([np.eye(n)[:ms], q["A"][k]])
        is_soft = ((q["sense"][k][W] & S.SOFT) != 0).astype(float)
        dz, dnu, qk, U = S.dense_adjoint(q["H"][k], Cm, W, is_soft, rho, g[k])
        out.append(dict(W=W, upper=lam[W] > 0, is_soft=is_soft, dz=dz, dnu=dnu, qk=qk, U=U,
                        scale=max(np.abs(dz).max(), np.abs(dnu).max() if len(W) else 0.0)))
    return out


def kkt_cond(q, k, W, is_soft, ms, rho=0.0):
    n = q["f"].shape[1]
    Cm = np.vstack([np.eye(n)[:ms], q["A"][k]])
    U = np.linalg.solve(q["H"][k], Cm[W].T).T
    K = np.block([[q["H"][k], Cm[W].T], [Cm[W], -np.diag(rho * np.einsum("kj,kj->k", Cm[W], U) * is_soft)]])
    return np.linalg.cond(K)


def check_inputs(q, ref, ms, soft=False, cap=None, tag=""):
    """the input conditions of one solve, on the oracle alone; returns (largest working set, smallest |lam| on W, largest cond_2(K))"""
    N = q["f"].shape[0]
    rho = S.RHO if soft else 0.0
    lam_min, cond, na_max = np.inf, 0.0, 0
    for k in range(N):
        assert ref["flag"][k] in ((1, 2) if soft else (1,)), (tag, k, ref["flag"][k])
        lam = ref["lam"][k]
        W = np.nonzero(lam)[0]
        assert set(W.tolist()) == set(ref["ws"][k].tolist()), (tag, k, "lam != 0 is not the oracle's working set")
        if len(W):
            lam_min = min(lam_min, np.abs(lam[W]).min())
        is_soft = ((q["sense"][k][W] & S.SOFT) != 0).astype(float)
        cond = max(cond, kkt_cond(q, k, W, is_soft, ms, rho))
        na_max = max(na_max, len(W))
    assert lam_min >= LAM_MIN, (tag, lam_min)
    assert cond <= COND_MAX, (tag, cond)
    if cap is not None:
        assert na_max > cap, (tag, na_max, cap, "no working set beyond the forced cap: no hand-over")
    return na_max, lam_min, cond


def check_adjoint(q, ref, refsol, r, na, ws, o, ms, ns=0, rho=0.0, tag=""):
    """the reference section's three rules for one solve: r the GPU's solve results, (na, ws) its working_sets(), o its backward();
    returns the worst error relative to TOL's scale"""
    N, n = q["f"].shape
    m = q["bupper"].shape[1]
    worst = 0.0
    for k in range(N):
        R = refsol[k]
        W = R["W"]
        assert r["exitflag"][k] == ref["flag"][k] and o["status"][k] == 0, (tag, k, r["exitflag"][k], ref["flag"][k], o["status"][k])
        # 2. the iterate the solve left on the device
        assert na[k] == len(W), (tag, k, na[k], len(W))
        assert sorted(ws[k, :na[k]].tolist()) == W.tolist(), (tag, k, ws[k, :na[k]], W)
        # 3. the adjoint
        dnu = o["dbupper"][k] + o["dblower"][k]
        e1 = np.abs(o["dz"][k] - R["dz"]).max()
        e2 = np.abs(dnu[W] - R["dnu"]).max() if len(W) else 0.0
        worst = max(worst, e1 / R["scale"], e2 / R["scale"])
        assert e1 <= TOL * R["scale"] and e2 <= TOL * R["scale"], (tag, k, e1, e2, R["scale"])
        off = np.ones(m, bool)
        off[W] = False
        assert not o["dbupper"][k][off].any() and not o["dblower"][k][off].any(), (tag, k)
        # a row with bupper == blower has no side of its own: sign(lam) says nothing there, the oracle's LOWER bit does
        eq = q["bupper"][k][W] == q["blower"][k][W]
        upper = np.where(eq, ~ref["lower"][k][W], R["upper"])
        assert not o["dblower"][k][W[upper]].any(), (tag, k, "a row held at its upper bound has a value in dblower")
        assert not o["dbupper"][k][W[~upper]].any(), (tag, k, "a row held at its lower bound has a value in dbupper")
        if ns == 0:
            continue
        want_q = np.zeros(m)
        want_q[W] = R["qk"] * R["is_soft"]
        assert np.abs(o["qsoft"][k] - want_q).max() <= TOL * max(1.0, np.abs(want_q).max()), (tag, k)
        assert not o["qsoft"][k][want_q == 0].any(), (tag, k)
        # u_k in the order of the device's working set, unused slots zero / -1
        pos = {int(i): j for j, i in enumerate(W)}
        order = [int(i) for i in ws[k, :na[k]] if R["is_soft"][pos[int(i)]]]
        assert len(order) <= ns
        assert o["usoft_id"][k].tolist() == order + [-1] * (ns - len(order)), (tag, k, o["usoft_id"][k], order)
        for slot, i in enumerate(order):
            u = R["U"][pos[i]]
            assert np.abs(o["usoft"][k, slot] - u).max() <= TOL * np.abs(u).max(), (tag, k, slot)
        assert not o["usoft"][k, len(order):].any(), (tag, k)
    return worst
