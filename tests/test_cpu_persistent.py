"""The batches of tests/persistent_cases.py are what tests/test_gpu_persistent.py takes them for -- numpy and the oracle alone, no GPU:
the planted sizes of the working sets, the -20, infeasible, -6 and -8 problems among the first eight, and the tier arithmetic that
puts the chosen shapes into the scratch tiers with a grid of 512 < N."""
import numpy as np
import pytest

import backward_soft_cases as S
import persistent_cases as P
import refine_cases as RC
from oracle import oracle as O

SING_TOL = 3.7e-11      # of the solver's LDL' (tests/test_gpu_backward_soft.py::_near_dependent)


def test_tier_arithmetic_puts_the_shapes_into_the_scratch_tiers():
    n, m, ms = P.ADJOINT_SHAPE
    for ns in (0, P.NS_MAX):
        cap = n + ns + 1
        assert P.backward_lds_bytes(n, cap, False, True) > P.LDS_MAX      # 183 904 bytes at cap = 121: nl == false
        assert P.pick_tier(n, cap, P.backward_lds_bytes)[0] == 2
        assert P.persistent_grid(P.N, 8 * P.scratch_doubles(n, cap)) == P.GRID == 512 < P.N
    assert P.backward_lds_bytes(120, 121, False, True) == 183904
    n = P.REFINE_SHAPE[0]
    assert n == 106 and P.pick_tier(n, n + 1, P.refine_lds_bytes)[0] == 2 and P.pick_tier(n - 1, n, P.refine_lds_bytes)[0] == 1
    assert P.pick_tier(130, 131, P.refine_lds_bytes)[0] == 2             # the scratch shape of refine_cases
    assert P.persistent_grid(P.N, 8 * P.scratch_doubles(n, n + 1)) == P.GRID
    for n, neq, m, ms in P.ELIM_SHAPES:
        assert n > 64 and P.persistent_grid(P.N, 8 * n * n) == P.GRID < P.N
    # the rule's other two ends: 256 MiB of scratch, and never below 16 workgroups
    assert P.persistent_grid(10000, 8 * P.scratch_doubles(400, 401)) == (256 << 20) // (8 * P.scratch_doubles(400, 401)) < 512
    assert P.persistent_grid(10000, 256 << 20) == 16 and P.persistent_grid(3, 8) == 3
    assert len(P.TAIL) == 8 and (P.TAIL - P.GRID == P.HEAD).all() and P.SOLVE_GRID < P.SOLVE_N
    # the shapes the issue names for tiers that are not exercised here stay where they are
    assert P.pick_tier(64, 65, P.backward_lds_bytes)[0] == 0 and P.pick_tier(80, 81, P.backward_lds_bytes)[0] == 1


def oracle_states(oracle, q, shape, idx, ns=0, settings=None):
    """(flag, sorted working set) of the oracle's cold solve per problem of idx"""
    n, m, ms = shape
    out = {}
    for k in idx:
        om = oracle.model(n, m, ms, ns, settings=O.default_settings(**(settings or {})))
        flag = om.setup(*[q[key][k] for key in P.KEYS])
        if flag >= 0:
            flag = om.solve()[3]
        out[int(k)] = (flag, np.sort(om.state()[0]))
    return out


def check_head_and_tail(st, exact_sizes):
    others = [k for k in P.HEAD if k not in (P.K20, P.KINF)]
    assert st[P.KINF][0] == -1, st[P.KINF][0]
    assert all(st[k][0] in (1, 2) for k in others + list(P.TAIL) + [P.K20])
    big, small = [len(st[k][1]) for k in others], [len(st[int(k)][1]) for k in P.TAIL]
    assert min(big) > max(small) and min(small) > 0, (big, small)
    if exact_sizes:
        assert set(big) == {P.BIG} and set(small) == {P.SMALL}, (big, small)
    assert len(st[P.K20][1]) > max(small)


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_adjoint_batch_holds_its_adversaries(oracle, soft):
    n, m, ms = P.ADJOINT_SHAPE
    q = P.adjoint_batch(soft)
    settings = dict(zero_tol=P.ZERO_TOL, **(dict(rho_soft=S.RHO) if soft else {}))
    st = oracle_states(oracle, q, P.ADJOINT_SHAPE, list(P.HEAD) + list(P.TAIL), P.NS_MAX if soft else 0, settings)
    check_head_and_tail(st, exact_sizes=not soft)
    # the -20 problem: the solver holds both nearly parallel rows, and the unit-row Gram matrix has a pivot between the two tolerances
    assert {ms, ms + 1} <= set(st[P.K20][1].tolist())
    p = P.near_dependent(n, m, ms, P.BIG, [6200 if soft else 6100, P.K20, 1])
    assert all(np.array_equal(p[key], q[key][P.K20]) for key in P.KEYS)
    W, piv = P.dependent_pivot(p, ms)
    assert np.array_equal(W, st[P.K20][1]) and 10 * SING_TOL < piv < P.ZERO_TOL / 10, piv
    if soft:
        assert all(((q["sense"][k] & S.SOFT) != 0).sum() == P.NS_MAX for k in P.TAIL)


def test_refine_batch_holds_its_adversaries(oracle):
    n, m, ms = P.REFINE_SHAPE
    q = P.refine_batch()
    st = oracle_states(oracle, q, P.REFINE_SHAPE, list(P.HEAD) + list(P.TAIL), 0, dict(zero_tol=P.ZERO_TOL))
    check_head_and_tail(st, exact_sizes=True)
    assert {ms, ms + 1} <= set(st[P.K20][1].tolist())
    W, piv = P.dependent_pivot(P.near_dependent(n, m, ms, P.BIG, [6300, P.K20]), ms)
    assert np.array_equal(W, st[P.K20][1]) and 10 * SING_TOL < piv < P.ZERO_TOL / 10, piv
    for k, idx in ((P.BIG, 0), (None, 8), (P.SMALL, int(P.TAIL[0]))):
        p = P.refine_problem(k)
        assert RC.exact(p) and RC.COND_RANGE[0] <= np.linalg.cond(p["H"]) <= RC.COND_RANGE[1]
        assert all(np.array_equal(p[key], q[key][idx]) for key in P.KEYS[:5])
        if idx != 8:
            assert np.array_equal(st[idx][1], p["W"])
        # every pivot of the planted problems' unit-row Gram matrices is well above the batch's zero_tol
        R = np.linalg.cholesky(p["H"]).T
        Nw = np.linalg.solve(R.T, RC.rows(p, p["W"]).T).T
        Nw /= np.sqrt((Nw * Nw).sum(axis=1))[:, None]
        assert (np.diag(np.linalg.cholesky(Nw @ Nw.T)) ** 2).min() > 10 * P.ZERO_TOL


@pytest.mark.parametrize("i", range(len(P.ELIM_SHAPES)), ids=[str(s) for s in P.ELIM_SHAPES])
def test_elimination_batch_holds_its_adversaries(i):
    b = P.elim_batch(i)
    n, neq, m, ms = b["shape"]
    eq = b["eq_rows"]
    differ = (b["bupper"][:, eq] != b["blower"][:, eq]).any(axis=1)
    assert differ[P.K8] and differ.sum() == 1                                  # -8
    for k in list(P.HEAD) + list(P.TAIL):
        E = np.vstack([np.eye(n)[:ms], b["A"][k]])[eq]
        nrm = np.sqrt((E * E).sum(axis=1))
        if not (nrm > 0).all():
            assert k == P.K6 and neq == 1                                      # -6: a zero row
            continue
        r2 = np.diag(np.linalg.qr((E / nrm[:, None]).T, mode="r")) ** 2
        assert (r2.min() < 1e-20) == (k == P.K6), (k, r2.min())                # -6: R_jj^2 below zero_tol = 1e-11 by nine orders; 0.01 and more elsewhere
        assert k == P.K6 or r2.min() > 1e-3


@pytest.mark.parametrize("shape,seed", [(P.SOLVE_SHAPES[0], 6500), (P.SOLVE_SHAPES[1], 6501), (P.TIER_SHAPE, 6510)], ids=["n70", "n130", "n129"])
def test_solve_batch_holds_its_adversaries(oracle, shape, seed):
    n, m, ms, _ = shape
    q = P.solve_batch(shape, seed)
    peaks = []
    for k in range(P.SOLVE_N):
        om = oracle.model(n, m, ms)
        assert om.setup(q["H"][k], q["f"][k], q["A"][k], q["bupper"][k], q["blower"][k], None) == 1      # (K_INF too: the solve finds it)
        for step in ("cold", "warm"):
            if step == "warm":
                assert om.update(O.UPDATE_v, f=q["f2"][k]) == 0
            om.enable_trace()
            x, lam, _, flag_s, it = om.solve()
            if step == "cold":
                peaks.append(P.trace_peak(om.get_trace()))
            if k == P.K_INF:
                assert flag_s == -1 and it > 1, (step, flag_s, it)
            elif k == P.K_EMPTY:
                assert flag_s == 1 and not lam.any() and (step == "warm" or it == 1), (step, flag_s, it)
            else:
                assert flag_s == 1 and lam.any(), (k, step, flag_s)
    if (shape, seed) == (P.HAND_OVER_SHAPE, P.HAND_OVER_SEED):
        # working sets beyond DAQP_AMD_WG_CAPL on every trip of a grid of 8, and within it on every trip
        beyond = np.array(peaks) > P.HAND_OVER_CAPL
        for trip in range(P.SOLVE_N // P.SOLVE_GRID):
            part = beyond[trip * P.SOLVE_GRID:(trip + 1) * P.SOLVE_GRID]
            assert part.any() and not part.all(), (trip, peaks)
