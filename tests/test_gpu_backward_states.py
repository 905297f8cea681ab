"""The adjoint (daqp_batch_backward, daqp_batch_backward_soft, qp_layer) behind every solve kernel family and behind warm states.

k_backward reads the iterate a solve leaves in device memory (WS, n_active, the LOWER / SOFT bits of sense, Rinv, scaling, A), and
each kernel family writes that iterate with its own bookkeeping.  Every case here forces one family with the switches the forward
tests use, and checks, per problem (tests/backward_state_cases.py):

  1. W and the side of each row come from the oracle model that went through the same setup / update / solve sequence;
  2. BatchModel.working_sets() equals that W as a set, n_active its size;
  3. dz and dbupper + dblower equal the dense fp64 solve of [H C_W'; C_W -S] [dz; dnu] = [g; 0] within TOL = 1e-9 of the max norm of
     [dz; dnu]; every entry off W is zero; every row of W has its value on the oracle's side only.

tests/test_cpu_backward_states.py holds the same inputs to their conditions (all OPTIMAL, |lam| >= 1e-8 on W, cond_2(K) <= 1e6, a
working set beyond the cap of every hand-over case, every warm step changes a working set).  Each test prints its worst error
relative to TOL's scale."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("backward_state_cases", os.path.join(HERE, "backward_state_cases.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

SWITCHES = sorted({k for t in (B.COLD, B.SOFT, B.WARM) for c in t.values() for k in c[0]} | {"EAGER_UPDATE"})
_oracle_side = {}      # the oracle's solves and the dense references: computed once per batch, shared, never modified


bits_equal = B.bits_equal


def _environment(monkeypatch, switches, exact):
    for k in SWITCHES:
        monkeypatch.delenv(B.PREFIX + k, raising=False)
    monkeypatch.setenv("DAQP_AMD_EXACT", "1" if exact else "0")
    for k, v in B.environment(switches).items():
        monkeypatch.setenv(k, v)


def _cold_reference(oracle, shape, N, seed, soft=False, init_mask=0):
    key = (shape, N, seed, soft, init_mask)
    if key not in _oracle_side:
        q = B.soft_batch(shape, N, seed) if soft else B.cold_batch(shape, N, seed)
        ref = B.OracleBatch(oracle, q, shape[2], ns=B.NS_MAX if soft else 0, soft=soft, init_mask=init_mask).solve()
        g = B.grad(N, shape[0])
        _oracle_side[key] = (q, ref, g, B.reference(q, ref, g, shape[2], B.S.RHO if soft else 0.0))
    return _oracle_side[key]


def _solve_and_differentiate(q, g, ms, soft=False):
    import daqp_amd
    N, n = q["f"].shape
    bm = daqp_amd.BatchModel(N, n, q["bupper"].shape[1], ms, B.NS_MAX if soft else 0, **B.settings(soft))
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"] if soft else None)
    r = bm.solve()
    o = bm.backward(g, out="numpy")
    na, ws = bm.working_sets()
    bm.close()
    return r, o, na, ws


# ---------------------------------------------------------------------------------------------------------------------------
# 1. cold solves, one case per family
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.COLD))
def test_cold_adjoint_behind_family(oracle, gpu_lib, monkeypatch, name):
    switches, shape, N, seed, _, cap = B.COLD[name]
    q, ref, g, refsol = _cold_reference(oracle, shape, N, seed)
    if cap is not None:
        assert max(len(R["W"]) for R in refsol) > cap, "no working set beyond the forced cap: no hand-over happened"
    _environment(monkeypatch, switches, exact=False)
    r, o, na, ws = _solve_and_differentiate(q, g, shape[2])
    worst = B.check_adjoint(q, ref, refsol, r, na, ws, o, shape[2], tag=name)
    print(f"{name}: max relative error against the dense KKT solve: {worst:.2e}")


@pytest.mark.parametrize("name", [k for k, c in B.COLD.items() if c[4]])
def test_cold_adjoint_behind_family_exact_mode(oracle, gpu_lib, monkeypatch, name):
    """DAQP_AMD_EXACT=1: the same check, and dz bit-identical to dz of the same problems under default dispatch (exact-mode iterates
    are bit-identical across families and k_backward is the same code).  The exact mode never runs an image kernel, and register
    and workgroup have no switch to drop: for register, register_bounds, image_3x25, image_3x25_bounds, workgroup and the two
    register_64 rows the second run repeats the first, and the comparison says only that the adjoint is reproducible.  It crosses
    paths for generic (k_ldp against the registers) and for the two register_hand_over rows (a cap of 12 rows with k_ldp behind the
    registers against the registers holding every row)."""
    switches, shape, N, seed, _, cap = B.COLD[name]
    q, ref, g, refsol = _cold_reference(oracle, shape, N, seed)
    _environment(monkeypatch, switches, exact=True)
    r, o, na, ws = _solve_and_differentiate(q, g, shape[2])
    worst = B.check_adjoint(q, ref, refsol, r, na, ws, o, shape[2], tag=name)
    print(f"{name}, exact mode: max relative error against the dense KKT solve: {worst:.2e}")
    _environment(monkeypatch, {}, exact=True)
    r0, o0, na0, ws0 = _solve_and_differentiate(q, g, shape[2])
    assert bits_equal(o["dz"], o0["dz"]), name
    assert bits_equal(o["dbupper"], o0["dbupper"]) and bits_equal(o["dblower"], o0["dblower"]), name


@pytest.mark.parametrize("name", list(B.SOFT))
def test_soft_adjoint_behind_family(oracle, gpu_lib, monkeypatch, name):
    switches, shape, N, seed = B.SOFT[name]
    q, ref, g, refsol = _cold_reference(oracle, shape, N, seed, soft=True)
    _environment(monkeypatch, switches, exact=False)
    r, o, na, ws = _solve_and_differentiate(q, g, shape[2], soft=True)
    worst = B.check_adjoint(q, ref, refsol, r, na, ws, o, shape[2], ns=B.NS_MAX, rho=B.S.RHO, tag=name)
    assert o["qsoft"].any() and (o["usoft_id"] >= 0).any()
    print(f"{name}, soft: max relative error against the dense KKT solve: {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. warm states
# ---------------------------------------------------------------------------------------------------------------------------
def _warm_reference(oracle, name):
    """[(q, ref, g, refsol, new arrays)] of the cold solve and of every step"""
    key = ("warm", name)
    if key not in _oracle_side:
        switches, shape, N, seed, step_seeds = B.WARM[name]
        ms = shape[2]
        g = B.grad(N, shape[0])
        cur = B.cold_batch(shape, N, seed)
        ob = B.OracleBatch(oracle, cur, ms)
        ref = ob.solve()
        out = [(dict(cur), ref, g, B.reference(cur, ref, g, ms), None)]
        for index, step in enumerate(B.STEPS):
            kw = B.warm_moves(cur, step, shape, step_seeds[step], index)
            cur.update(kw)
            ob.update(B.MASK[step], kw)
            ref = ob.solve()
            out.append((dict(cur), ref, g, B.reference(cur, ref, g, ms), kw))
        _oracle_side[key] = out
    return _oracle_side[key]


@pytest.mark.parametrize("eager", ["0", "1"], ids=["fused_update", "eager_update"])
@pytest.mark.parametrize("memory", ["device", "numpy"])
@pytest.mark.parametrize("name", list(B.WARM))
def test_warm_adjoint_after_every_update(oracle, gpu_lib, monkeypatch, name, memory, eager):
    """one kept BatchModel against one kept oracle model per problem: solve, then update(f), update(bupper, blower), update(A),
    update(H), update(sense = zeros), each followed by a solve and the full check.  memory: device tensors (used in place) or numpy
    arrays (staged).  eager: DAQP_AMD_EAGER_UPDATE set (the library asks whether it is set, so `0` is the variable unset); it
    decides only how update(f) and update(bupper, blower) of the register shapes are applied (NB > 0: fused into the next solve
    launch or by a kernel of their own) -- for workgroup, and for the A, H and sense steps, both ids run the same code.

    update(A) and update(H) on their own empty the working set but leave the ACTIVE bits of its rows set, as the reference does
    (utils.c:470: reset_daqp_workspace without daqp_deactivate_constraints), so the solve after them never takes those rows back:
    it ends OPTIMAL at a point that is NOT the optimum of the QP as it stands.  Oracle and GPU agree on that iterate, and the
    adjoint is checked there: it is the linear system at the stored W with the new A, Rinv and scaling, whatever W is.  After
    update(sense = zeros) the bits are gone and the solve is a cold one of the data as they stand."""
    import torch
    import daqp_amd
    switches, shape, N, seed, _ = B.WARM[name]
    n, m, ms, _ = shape
    seq = _warm_reference(oracle, name)
    _environment(monkeypatch, switches, exact=False)
    if eager == "1":
        monkeypatch.setenv("DAQP_AMD_EAGER_UPDATE", "1")
    give = (lambda a: torch.tensor(a, device="cuda")) if memory == "device" else (lambda a: a.copy())
    bm = daqp_amd.BatchModel(N, n, m, ms)
    q, ref, g, refsol, _ = seq[0]
    bm.setup(*(give(q[k]) for k in ("H", "f", "A", "bupper", "blower")))
    worst = 0.0
    for (q, ref, g, refsol, kw), step in zip(seq, ("cold",) + B.STEPS):
        if kw is not None:
            bm.update(**{k: give(v) for k, v in kw.items()})
        r = bm.solve()
        o = bm.backward(g, out="numpy")
        na, ws = bm.working_sets()
        worst = max(worst, B.check_adjoint(q, ref, refsol, r, na, ws, o, ms, tag=(name, memory, eager, step)))
        if step in ("cold", "sense"):
            # both are cold solves of the data as they stand (after `sense` the working sets were rebuilt from all-zero ACTIVE bits):
            # reset + solve is the same cold solve again
            bm.reset()
            r2 = bm.solve()
            o2 = bm.backward(g, out="numpy")
            na2, ws2 = bm.working_sets()
            B.check_adjoint(q, ref, refsol, r2, na2, ws2, o2, ms, tag=(name, memory, eager, step, "reset"))
            for key in ("dz", "dbupper", "dblower"):
                assert bits_equal(o[key], o2[key]), (name, memory, eager, step, key)
    bm.close()
    print(f"{name}, {memory}, eager {eager}: max relative error against the dense KKT solve over the sequence: {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. qp_layer behind the headline path
# ---------------------------------------------------------------------------------------------------------------------------
def test_layer_gradients_behind_image_kernel(oracle, gpu_lib, monkeypatch):
    """l = <g, x>: dl/df = -dz, dl/dH = -1/2 (dz x' + x dz'), dl/dA_i = -(lam_i dz + dnu_i x)', dl/dbupper, dl/dblower = dnu on the side
    the row is held at (BatchModel.backward's docstring), assembled in numpy from the dense solution and the oracle's x and lam.
    Tolerance: TOL of the max norm of [dz; dnu] for every gradient."""
    import torch
    import daqp_amd
    switches, shape, N, seed = B.LAYER
    n, m, ms, _ = shape
    q, ref, g, refsol = _cold_reference(oracle, shape, N, seed, init_mask=B.O.UPDATE_unconstrained)
    _environment(monkeypatch, switches, exact=False)
    t = {k: torch.tensor(q[k], device="cuda", requires_grad=True) for k in ("H", "f", "A", "bupper", "blower")}
    info = {}
    x = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=ms, info=info)
    x.backward(torch.tensor(g, device="cuda"))
    assert np.array_equal(info["exitflag"].cpu().numpy(), ref["flag"]) and not info["status"].any()
    assert np.array_equal(np.sign(info["lam"].cpu().numpy()), np.sign(ref["lam"]))
    got = {k: t[k].grad.cpu().numpy() for k in t}
    worst = 0.0
    for k in range(N):
        R = refsol[k]
        W, dz = R["W"], R["dz"]
        xk, lam = ref["x"][k], ref["lam"][k]
        dnu = np.zeros(m)
        dnu[W] = R["dnu"]
        want = dict(f=-dz, H=-0.5 * (np.outer(dz, xk) + np.outer(xk, dz)), A=-(np.outer(lam[ms:], dz) + np.outer(dnu[ms:], xk)),
                    bupper=np.where(lam > 0, dnu, 0.0), blower=np.where(lam < 0, dnu, 0.0))
        for key in want:
            err = np.abs(got[key][k] - want[key]).max() / R["scale"]
            worst = max(worst, err)
            assert err <= B.TOL, (key, k, err)
        assert not got["bupper"][k][lam <= 0].any() and not got["blower"][k][lam >= 0].any(), k
    print(f"qp_layer behind the image kernel: max relative error of the gradients: {worst:.2e}")
