"""daqp_batch_backward_nullspace (BatchModel.backward(nullspace=...), qp_layer(nullspace=True)): the adjoint of problems that went
through the proximal loop -- singular H, LPs -- by the null-space method on the caller's own H (daqp_amd/csrc/nullspace.hip.h).

Per case of tests/backward_nullspace_cases.py and per problem: BatchModel.working_sets() equals the oracle's W; dz and dbupper +
dblower equal np.linalg.solve on the full KKT matrix within TOL = 1e-9 of the max norm of [dz; dnu]; every entry off W is zero;
every dnu sits on the side of its row's LOWER bit.  tests/test_cpu_backward_nullspace.py holds the same inputs to their conditions
on the oracle alone and the dense reference to central differences.  Each test prints its worst error relative to TOL's scale."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("backward_nullspace_cases", os.path.join(HERE, "backward_nullspace_cases.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

_oracle_side = {}      # the oracle's solves and the dense references: computed once per case, shared, never modified
UNSUPPORTED, SINGULAR = -8, -20


def _reference(oracle, name):
    if name not in _oracle_side:
        q = B.batch(name)
        ref = B.oracle_solve(oracle, name)
        g = B.grad(q["f"].shape[0], B.CASES[name]["shape"][0])
        _oracle_side[name] = (q, ref, g, B.reference(name, ref, g))
    return _oracle_side[name]


def _model(name, settings=None, give=lambda a: a):
    """the case's batch, set up and solved; (model, solve results)"""
    import daqp_amd
    c = B.CASES[name]
    n, m, ms = c["shape"]
    q = B.batch(name)
    bm = daqp_amd.BatchModel(q["f"].shape[0], n, m, ms, **(c.get("settings", {}) if settings is None else settings))
    args = [None if q[k] is None else give(q[k]) for k in ("H", "f", "A", "bupper", "blower", "sense")]
    if c.get("shared", False):
        bm.setup_shared(*args)
    else:
        bm.setup(*args)
    return bm, bm.solve()


@pytest.mark.parametrize("exact", ["0", "1"], ids=["default_mode", "exact_mode"])
@pytest.mark.parametrize("name", list(B.CASES))
def test_nullspace_adjoint_against_the_dense_reference(oracle, gpu_lib, monkeypatch, name, exact):
    monkeypatch.setenv("DAQP_AMD_EXACT", exact)
    q, ref, g, refsol = _reference(oracle, name)
    bm, r = _model(name)
    assert (bm.prox_info()["n_prox"] > 0).all(), name
    plain = bm.backward(g, out="numpy")
    assert (plain["status"] == UNSUPPORTED).all() and not plain["dz"].any(), "daqp_batch_backward itself must keep refusing these"
    o = bm.backward(g, out="numpy", nullspace=True)
    na, ws = bm.working_sets()
    worst = B.check_adjoint(name, ref, refsol, r, na, ws, o, tag=exact)
    o1 = bm.backward(g, out="numpy", nullspace="all")      # every problem is proximal here: the same launch for the same problems
    for key in ("dz", "dbupper", "dblower", "status"):
        assert B.bits_equal(o[key].astype(np.float64), o1[key].astype(np.float64)), (name, key)
    bm.close()
    fam = B.CASES[name]["family"]
    print(f"family {fam} ({B.FAMILIES[fam]}), {name}, exact {exact}: max relative error against the dense KKT solve: {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------
# the two algorithms against each other
# ---------------------------------------------------------------------------------------------------------------------------
def _agree(a, b, tag):
    worst = 0.0
    for k in range(a["dz"].shape[0]):
        assert a["status"][k] == 0 and b["status"][k] == 0, (tag, k, a["status"][k], b["status"][k])
        da, db = a["dbupper"][k] + a["dblower"][k], b["dbupper"][k] + b["dblower"][k]
        scale = max(np.abs(b["dz"][k]).max(), np.abs(db).max())
        err = max(np.abs(a["dz"][k] - b["dz"][k]).max(), np.abs(da - db).max()) / scale
        worst = max(worst, err)
        assert err <= B.TOL, (tag, k, err)
        assert np.array_equal(a["dbupper"][k] != 0, b["dbupper"][k] != 0) and np.array_equal(a["dblower"][k] != 0, b["dblower"][k] != 0), (tag, k)
    return worst


@pytest.mark.parametrize("name", [k for k, c in B.CASES.items() if c["family"] in (4, 7)])
def test_nullspace_agrees_with_the_gram_adjoint(oracle, gpu_lib, monkeypatch, name):
    """positive definite H: (a) solved with the shift forced (n_prox > 0) and differentiated by the null-space kernel, against the
    same data solved without it and differentiated by daqp_batch_backward -- same H, A and W, so the same adjoint; (b) on that plain
    batch, nullspace="all" against daqp_batch_backward."""
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    q, ref, g, refsol = _reference(oracle, name)
    forced, r = _model(name)
    o_forced = forced.backward(g, out="numpy", nullspace="all")
    naf, wsf = forced.working_sets()
    plain, r0 = _model(name, settings={})
    assert not plain.prox_info()["n_prox"].any()
    o_gram = plain.backward(g, out="numpy")
    o_all = plain.backward(g, out="numpy", nullspace="all")
    o_true = plain.backward(g, out="numpy", nullspace=True)
    nap, wsp = plain.working_sets()
    for k in range(len(naf)):
        assert sorted(wsf[k, :naf[k]].tolist()) == sorted(wsp[k, :nap[k]].tolist()), (name, k)
    w1 = _agree(o_forced, o_gram, (name, "forced shift"))
    w2 = _agree(o_all, o_gram, (name, "plain"))
    for key in ("dz", "dbupper", "dblower"):      # no proximal problem: which = 0 is daqp_batch_backward
        assert B.bits_equal(o_true[key], o_gram[key]), (name, key)
    forced.close()
    plain.close()
    print(f"{name}: null-space kernel against the Gram adjoint: forced shift {w1:.2e}, plain batch {w2:.2e}")


def _mixed_batch():
    """n = 16: even problems positive definite (n_prox == 0 under the automatic shift), odd ones dense PSD of rank 10"""
    n, m, ms, N = 16, 40, 4, 12
    qs = []
    for k in range(N):
        if k % 2 == 0:
            p = O.generate_qp(n, m, ms, 6, rng=[770, k])
            qs.append({key: p[key] for key in B.KEYS + ("H",)})
        else:
            qs.append(O.generate_singular_qp(n, m, ms, 10, [771, k]))
    return (n, m, ms, N), {key: np.stack([p[key] for p in qs]) for key in B.KEYS + ("H",)}


def test_mixed_batch_keeps_the_other_problems_bit_for_bit(oracle, gpu_lib, monkeypatch):
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    (n, m, ms, N), q = _mixed_batch()
    g = B.grad(N, n)
    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    r = bm.solve()
    assert (r["exitflag"] == 1).all()
    prox = bm.prox_info()["n_prox"] > 0
    assert np.array_equal(prox, np.arange(N) % 2 == 1)
    o0 = bm.backward(g, out="numpy")
    o1 = bm.backward(g, out="numpy", nullspace=True)
    na, ws = bm.working_sets()
    bm.close()
    assert (o0["status"][prox] == UNSUPPORTED).all() and not o0["status"][~prox].any() and not o1["status"].any()
    for key in ("dz", "dbupper", "dblower"):
        assert B.bits_equal(o0[key][~prox], o1[key][~prox]), key
    worst = 0.0
    for k in np.nonzero(prox)[0]:      # and the proximal ones against the dense solve at the oracle's working set
        om = oracle.model(n, m, ms)
        assert om.setup(q["H"][k], q["f"][k], q["A"][k], q["bupper"][k], q["blower"][k], q["sense"][k]) == 1
        assert om.solve()[3] == 1
        W = np.sort(om.state()[0])
        assert sorted(ws[k, :na[k]].tolist()) == W.tolist(), k
        dz, dnu = B.dense_adjoint(q["H"][k], q["A"][k], ms, W, g[k])
        scale = max(np.abs(dz).max(), np.abs(dnu).max())
        err = max(np.abs(o1["dz"][k] - dz).max(), np.abs((o1["dbupper"][k] + o1["dblower"][k])[W] - dnu).max()) / scale
        worst = max(worst, err)
        assert err <= B.TOL, (k, err)
    print(f"mixed batch: proximal problems against the dense KKT solve: {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------
# statuses and refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _zero_outputs(o, k):
    return not o["dz"][k].any() and not o["dbupper"][k].any() and not o["dblower"][k].any()


@pytest.mark.parametrize("f1,rows", [(1.0, 0), (2.0, 1)])
def test_semidefinite_on_the_null_space_is_singular(gpu_lib, monkeypatch, f1, rows):
    """H = diag(1, 0), f = (f1, 0), -1 <= x <= 1: the optimum is not unique in x_2, Z'HZ has a zero pivot, status -20, zero outputs.
    f1 = 1: x_1 = -1 is the unconstrained minimiser as well, the bound is touched with a zero multiplier and the solver (the oracle
    too) ends with W empty: Z'HZ = H.  f1 = 2: lam_1 = -1, W = {x_1 lower}, Z = e_2 and Z'HZ = 0."""
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    N = 3
    H = np.tile(np.diag([1.0, 0.0]), (N, 1, 1))
    f = np.tile([f1, 0.0], (N, 1))
    bm = daqp_amd.BatchModel(N, 2, 2, 2)
    bm.setup(H, f, np.zeros((N, 0, 2)), np.ones((N, 2)), -np.ones((N, 2)))
    r = bm.solve()
    na, ws = bm.working_sets()
    assert (r["exitflag"] == 1).all() and (na == rows).all() and (ws[:, :rows] == 0).all() and np.allclose(r["x"][:, 0], -1.0)
    for mode in (True, "all"):
        o = bm.backward(np.ones((N, 2)), out="numpy", nullspace=mode)
        assert (o["status"] == SINGULAR).all() and all(_zero_outputs(o, k) for k in range(N)), (mode, o)
    bm.close()


def test_infeasible_and_unbounded_lps_carry_their_exit_flags(gpu_lib, monkeypatch):
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    n, m, ms, N = 5, 14, 2, 6
    qs = [O.generate_lp(n, m, ms, [780, k], unbounded=(k == 1)) for k in range(N)]
    b = {key: np.stack([p[key] for p in qs]) for key in B.KEYS}
    b["A"][4, 1] = b["A"][4, 0]      # problem 4: two copies of one row with disjoint bounds
    b["blower"][4, ms + 1] = b["bupper"][4, ms] + 1.0
    b["bupper"][4, ms + 1] = b["bupper"][4, ms] + 2.0
    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(None, b["f"], b["A"], b["bupper"], b["blower"], b["sense"])
    r = bm.solve()
    assert r["exitflag"][1] == -3 and r["exitflag"][4] == -1 and (np.delete(r["exitflag"], [1, 4]) == 1).all(), r["exitflag"]
    o = bm.backward(B.grad(N, n), out="numpy", nullspace=True)
    bm.close()
    assert o["status"][1] == -3 and o["status"][4] == -1 and _zero_outputs(o, 1) and _zero_outputs(o, 4)
    good = np.delete(np.arange(N), [1, 4])
    assert not o["status"][good].any() and all(o["dbupper"][k].any() or o["dblower"][k].any() for k in good)


def test_beyond_one_wavefront_stays_unsupported(gpu_lib, monkeypatch):
    """n = 80: proximal problems keep DAQP_EXIT_UNSUPPORTED with which = 0, which = 1 is refused"""
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    n, m, ms, N = 80, 160, 0, 4
    qs = [O.generate_singular_qp(n, m, ms, 40, [790, k]) for k in range(N)]
    b = {key: np.stack([p[key] for p in qs]) for key in B.KEYS + ("H",)}
    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(b["H"], b["f"], b["A"], b["bupper"], b["blower"], b["sense"])
    r = bm.solve()
    assert (r["exitflag"] == 1).all() and (bm.prox_info()["n_prox"] > 0).all()
    o = bm.backward(B.grad(N, n), out="numpy", nullspace=True)
    assert (o["status"] == UNSUPPORTED).all() and all(_zero_outputs(o, k) for k in range(N))
    with pytest.raises(RuntimeError, match="n <= 64"):
        bm.backward(B.grad(N, n), out="numpy", nullspace="all")
    bm.close()


def test_refusals(gpu_lib, monkeypatch):
    """a batch created with ns_max > 0; a batch whose last operation is an update or a reset"""
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    n, m, ms, N = 5, 14, 2, 4
    q = O.generate_batch(N, n, m, ms, 2, 795)
    g = B.grad(N, n)
    soft = daqp_amd.BatchModel(N, n, m, ms, 2)
    soft.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
    soft.solve()
    for mode in (True, "all"):
        with pytest.raises(RuntimeError, match="ns_max > 0"):
            soft.backward(g, out="numpy", nullspace=mode)
    soft.close()
    bm, r = _model("lp_n5")
    g = B.grad(B.batch("lp_n5")["f"].shape[0], 5)
    assert not bm.backward(g, out="numpy", nullspace=True)["status"].any()
    bm.update(f=B.batch("lp_n5")["f"] * 1.01)
    with pytest.raises(RuntimeError, match="successful daqp_batch_solve"):
        bm.backward(g, out="numpy", nullspace=True)
    bm.solve()
    assert not bm.backward(g, out="numpy", nullspace=True)["status"].any()
    bm.reset()
    with pytest.raises(RuntimeError, match="successful daqp_batch_solve"):
        bm.backward(g, out="numpy", nullspace="all")
    with pytest.raises(ValueError):
        bm.backward(g, out="numpy", nullspace="yes")
    bm.close()


# ---------------------------------------------------------------------------------------------------------------------------
# memory
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lp_n16", "psd_n33", "shared_n12"])
def test_host_and_device_memory_give_identical_bits(oracle, gpu_lib, monkeypatch, name):
    import torch
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    q, ref, g, refsol = _reference(oracle, name)
    host, _ = _model(name)
    oh = host.backward(g, out="numpy", nullspace=True)
    host.close()
    dev, _ = _model(name, give=lambda a: torch.tensor(a, device="cuda"))      # H and A adopted: read in place by the kernel
    od = dev.backward(torch.tensor(g, device="cuda"), out="torch", nullspace=True)
    od = {k: v.cpu().numpy() for k, v in od.items()}
    dev.close()
    assert not oh["status"].any() and np.array_equal(oh["status"], od["status"])
    for key in ("dz", "dbupper", "dblower"):
        assert B.bits_equal(oh[key], od[key]), (name, key)


# ---------------------------------------------------------------------------------------------------------------------------
# qp_layer
# ---------------------------------------------------------------------------------------------------------------------------
def _layer_check(name, ref, refsol, got, tag):
    """dl/df = -dz, dl/dH = -1/2 (dz x' + x dz'), dl/dA_i = -(lam_i dz + dnu_i x)', dl/dbupper, dl/dblower = dnu on the side of the
    row's LOWER bit, from the dense solution and the oracle's x and lam.  Tolerance: TOL of the max norm of [dz; dnu], times
    max(1, |x|_max, |lam|_max) -- the factors dz and dnu are multiplied with."""
    n, m, ms = B.CASES[name]["shape"]
    worst = 0.0
    for k, R in enumerate(refsol):
        W, dz = R["W"], R["dz"]
        xk, lam = ref["x"][k], ref["lam"][k]
        dnu = np.zeros(m)
        dnu[W] = R["dnu"]
        lower = ref["lower"][k]
        want = dict(f=-dz, A=-(np.outer(lam[ms:], dz) + np.outer(dnu[ms:], xk)), bupper=np.where(lower, 0.0, dnu), blower=np.where(lower, dnu, 0.0))
        if "H" in got:
            want["H"] = -0.5 * (np.outer(dz, xk) + np.outer(xk, dz))
        bound = B.TOL * R["scale"] * max(1.0, np.abs(xk).max(), np.abs(lam).max())
        for key in want:
            err = np.abs(got[key][k] - want[key]).max()
            worst = max(worst, err / bound * B.TOL)
            assert err <= bound, (tag, key, k, err, bound)
    return worst


def test_layer_differentiates_a_vertex_lp(oracle, gpu_lib, monkeypatch):
    import torch
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    name = "lp_n16"
    n, m, ms = B.CASES[name]["shape"]
    q, ref, g, refsol = _reference(oracle, name)
    t = {k: torch.tensor(q[k], device="cuda", requires_grad=True) for k in ("f", "A", "bupper", "blower")}
    info = {}
    x = daqp_amd.qp_layer(None, t["f"], t["A"], t["bupper"], t["blower"], ms=ms, info=info, nullspace=True)
    x.backward(torch.tensor(g, device="cuda"))
    assert (info["exitflag"].cpu().numpy() == 1).all() and not info["status"].any()
    got = {k: t[k].grad.cpu().numpy() for k in t}
    assert not got["f"].any(), "at a vertex dz = 0: dl/df = 0"
    worst = _layer_check(name, ref, refsol, got, name)
    assert np.abs(got["A"]).max() > 1e-3 and (np.abs(got["bupper"]) + np.abs(got["blower"])).max() > 1e-3
    # without nullspace=True an LP batch is not something the layer takes, and a shared-plant LP is refused by name
    with pytest.raises(Exception):
        daqp_amd.qp_layer(None, t["f"], t["A"], t["bupper"], t["blower"], ms=ms)
    with pytest.raises(ValueError, match="shared-plant LP"):
        daqp_amd.qp_layer(None, t["f"], t["A"][0], t["bupper"], t["blower"], ms=ms, nullspace=True)
    print(f"qp_layer, vertex LP: max relative error of the gradients: {worst:.2e}")


def test_layer_differentiates_a_semidefinite_hessian(oracle, gpu_lib, monkeypatch):
    import torch
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    name = "psd_n16"
    n, m, ms = B.CASES[name]["shape"]
    q, ref, g, refsol = _reference(oracle, name)
    t = {k: torch.tensor(q[k], device="cuda", requires_grad=True) for k in ("H", "f", "A", "bupper", "blower")}
    info = {}
    x = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=ms, info=info, nullspace=True)
    x.backward(torch.tensor(g, device="cuda"))
    assert (info["exitflag"].cpu().numpy() == 1).all() and not info["status"].any()
    got = {k: t[k].grad.cpu().numpy() for k in t}
    worst = _layer_check(name, ref, refsol, got, name)
    assert np.abs(got["H"]).max() > 1e-3
    # the default still raises, as it did before there was a null-space kernel
    t2 = {k: torch.tensor(q[k], device="cuda", requires_grad=True) for k in ("H", "f", "A", "bupper", "blower")}
    x2 = daqp_amd.qp_layer(t2["H"], t2["f"], t2["A"], t2["bupper"], t2["blower"], ms=ms)
    with pytest.raises(RuntimeError, match="have no derivative"):
        x2.backward(torch.tensor(g, device="cuda"))
    print(f"qp_layer, dense PSD H: max relative error of the gradients: {worst:.2e}")
