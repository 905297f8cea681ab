"""The inputs of tests/test_gpu_backward_states.py held to their conditions on the oracle alone (tests/backward_state_cases.py is the
table both files read): every problem of every case ends OPTIMAL (SOFT_OPTIMAL allowed in the soft variants), every multiplier of a
working set is at least 1e-8 in size, cond_2 of every KKT matrix is at most 1e6, every hand-over case has a working set beyond its
forced cap, and every warm step changes the stored working set of at least one problem."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("backward_state_cases", os.path.join(HERE, "backward_state_cases.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)


@pytest.mark.parametrize("name", list(B.COLD))
def test_cold_cases_meet_their_conditions(oracle, name):
    switches, shape, N, seed, exact, cap = B.COLD[name]
    assert 16 <= N <= 48
    q = B.cold_batch(shape, N, seed)
    ref = B.OracleBatch(oracle, q, shape[2]).solve()
    na_max, lam_min, cond = B.check_inputs(q, ref, shape[2], cap=cap, tag=name)
    print(f"{name}: largest working set {na_max}, smallest |lam| {lam_min:.2e}, largest cond_2(K) {cond:.2e}")
    if shape[2]:
        assert any((ws < shape[2]).any() for ws in ref["ws"]), "no active simple bound in the batch"


@pytest.mark.parametrize("name", list(B.SOFT))
def test_soft_cases_meet_their_conditions(oracle, name):
    switches, shape, N, seed = B.SOFT[name]
    assert 16 <= N <= 48
    q = B.soft_batch(shape, N, seed)
    assert (((q["sense"] & B.S.SOFT) != 0).sum(1) == B.NS_MAX).all() and ((q["sense"] == 5).sum(1) == 1).all()
    ref = B.OracleBatch(oracle, q, shape[2], ns=B.NS_MAX, soft=True).solve()
    na_max, lam_min, cond = B.check_inputs(q, ref, shape[2], soft=True, tag=name)
    active_soft = ((ref["lam"] != 0) & ((q["sense"] & B.S.SOFT) != 0)).any(1)
    print(f"{name}: largest working set {na_max}, smallest |lam| {lam_min:.2e}, largest cond_2(K) {cond:.2e}, "
          f"problems with an active SOFT row {int(active_soft.sum())}, SOFT_OPTIMAL {int((ref['flag'] == 2).sum())}")
    # (not among the issue's conditions: without an active SOFT row S is zero and the variant repeats the hard case)
    assert 4 * active_soft.sum() >= N, (name, int(active_soft.sum()))
    assert all((q["sense"][k][ref["ws"][k]] == 5).any() for k in range(N)), "the equality is in every working set"


@pytest.mark.parametrize("name", list(B.WARM))
def test_warm_steps_meet_their_conditions(oracle, name):
    """every step changes the working set, as a set, of at least one problem.  (update(A) and update(H) on their own empty the
    working set but keep the ACTIVE bits of its rows, reference utils.c:470, so the solve after them ends OPTIMAL on the other rows
    only; update(sense = zeros) clears the bits and the solve after it finds the working set of the data as they stand.)"""
    switches, shape, N, seed, step_seeds = B.WARM[name]
    assert 16 <= N <= 48
    ms = shape[2]
    cur = B.cold_batch(shape, N, seed)
    ob = B.OracleBatch(oracle, cur, ms)
    ref = ob.solve()
    B.check_inputs(cur, ref, ms, tag=(name, "cold"))
    for index, step in enumerate(B.STEPS):
        kw = B.warm_moves(cur, step, shape, step_seeds[step], index)
        cur.update(kw)
        ob.update(B.MASK[step], kw)
        prev, ref = ref, ob.solve()
        na_max, lam_min, cond = B.check_inputs(cur, ref, ms, tag=(name, step))
        changed = sum(set(prev["ws"][k].tolist()) != set(ref["ws"][k].tolist()) for k in range(N))
        print(f"{name} after {step}: working set changed in {changed} of {N} problems, smallest |lam| {lam_min:.2e}, cond_2(K) {cond:.2e}")
        assert changed >= 1, (name, step, "the step leaves every working set as it was: it proves nothing about the state")


def test_layer_case_meets_its_conditions(oracle):
    switches, shape, N, seed = B.LAYER
    q = B.cold_batch(shape, N, seed)
    ref = B.OracleBatch(oracle, q, shape[2], init_mask=B.O.UPDATE_unconstrained).solve()
    B.check_inputs(q, ref, shape[2], tag="layer")


def test_the_check_rejects_a_wrong_iterate_or_adjoint(oracle):
    """check_adjoint on outputs made from the dense reference itself: accepted as they are, refused with a stale n_active, a wrong
    working-set slot, a value on the wrong side, a value off W, or dz off by 1e-8 of the scale"""
    switches, shape, N, seed, exact, cap = B.COLD["register_bounds"]
    n, m, ms, _ = shape
    q = B.cold_batch(shape, N, seed)
    ref = B.OracleBatch(oracle, q, ms).solve()
    g = B.grad(N, n)
    refsol = B.reference(q, ref, g, ms)

    def outputs():
        o = dict(dz=np.zeros((N, n)), dbupper=np.zeros((N, m)), dblower=np.zeros((N, m)), status=np.zeros(N, np.int32))
        na, ws = np.zeros(N, np.int32), np.full((N, n + 1), -1, np.int32)
        for k, R in enumerate(refsol):
            W = R["W"]
            na[k], ws[k, :len(W)] = len(W), W[::-1]
            o["dz"][k] = R["dz"]
            o["dbupper"][k][W[R["upper"]]] = R["dnu"][R["upper"]]
            o["dblower"][k][W[~R["upper"]]] = R["dnu"][~R["upper"]]
        return dict(x=ref["x"], lam=ref["lam"], exitflag=ref["flag"]), o, na, ws

    r, o, na, ws = outputs()
    assert B.check_adjoint(q, ref, refsol, r, na, ws, o, ms) == 0.0
    k = next(k for k, R in enumerate(refsol) if len(R["W"]) >= 2 and R["upper"].any() and abs(R["dnu"][R["upper"]]).max() > 0)
    W, up = refsol[k]["W"], refsol[k]["upper"]
    i = W[up][np.argmax(np.abs(refsol[k]["dnu"][up]))]
    free = next(j for j in range(m) if j not in W)

    def stale_count(r, o, na, ws): na[k] -= 1
    def wrong_slot(r, o, na, ws): ws[k, 0] = free
    def wrong_side(r, o, na, ws): o["dblower"][k][i], o["dbupper"][k][i] = o["dbupper"][k][i], 0.0
    def off_w(r, o, na, ws): o["dbupper"][k][free] = 1e-300
    def dz_off(r, o, na, ws): o["dz"][k][0] += 1e-8 * refsol[k]["scale"]
    def bad_status(r, o, na, ws): o["status"][k] = -20

    for spoil in (stale_count, wrong_slot, wrong_side, off_w, dz_off, bad_status):
        r, o, na, ws = outputs()
        spoil(r, o, na, ws)
        with pytest.raises(AssertionError):
            B.check_adjoint(q, ref, refsol, r, na, ws, o, ms)
