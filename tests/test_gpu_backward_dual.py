"""daqp_batch_backward_dual / BatchModel.backward(grad_lam=) / qp_layer(returns=): the adjoint with a dual right-hand side,

    [ H    C_W' ] [ dz  ]   [ g_x       ]
    [ C_W  0    ] [ dnu ] = [ g_lam[W]  ]

against np.linalg.solve on the dense matrix, and the layer's gradients through x, lam and fval against finite differences.

Tolerance of the adjoint: that of tests/test_gpu_backward.py, 1e-9 relative to the max norm of the solution [dz; dnu] -- the matrix
is the same, so the conditioning argument of that file's docstring holds for any right-hand side (cond_2(K) <= 5e4 on its draws, <= 1e6
on those of tests/backward_nullspace_cases.py).  The problems, their generators and the planted layer problems are those files' own."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_dual", os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("test_gpu_backward")             # CASES, _generate, _solve, _grad, _planted, _crossed, _shared_problem
B = _load("backward_nullspace_cases")      # the proximal batches, dense_adjoint's matrix, bits_equal
TR = _load("test_gpu_refine")              # near_dependent

N, TOL = T.N, T.TOL
UNSUPPORTED, SINGULAR = -8, -20
KEYS = ("dz", "dbupper", "dblower")


def _grad_lam(Nq, m, seed=13):
    return np.random.default_rng(seed).standard_normal((Nq, m))


def _dense(H, A, ms, W, gx, glW):
    n = gx.size
    K, Cm = B.kkt(H, A, ms, W, n)
    sol = np.linalg.solve(K, np.concatenate([gx, glW]))
    return sol[:n], sol[n:], Cm


def _check(bm, q, r, gx, gl, o, ms, only=None, expect_in_ws=None, tol=TOL, side_tol=1e-9):
    """every assertion of test_gpu_backward.py's _check, with g_lam on W in the right-hand side; returns (n_active, WS).  side_tol: how
    close to the bound of its side a row of W must sit -- 1e-9 as in that file; 1e-6 for problems that went through the proximal loop,
    whose x is as good as the outer fixed-point tolerance (the row's other bound is at least 1e-2 away in every batch used here)"""
    Nq, n = q["f"].shape
    m = q["bupper"].shape[1]
    na, ws = bm.working_sets()
    worst = 0.0
    for k in (range(Nq) if only is None else only):
        H = None if q["H"] is None else (q["H"] if q["H"].ndim == 2 else q["H"][k])
        A = q["A"] if q["A"].ndim == 2 else q["A"][k]
        assert r["exitflag"][k] == 1 and o["status"][k] == 0, (k, r["exitflag"][k], o["status"][k])
        W = ws[k, :na[k]]
        assert len(set(W.tolist())) == na[k] and (W >= 0).all() and (W < m).all()
        if expect_in_ws is not None:
            assert expect_in_ws in W, (k, W)
        dz, dnuW, Cm = _dense(H, A, ms, W, gx[k], gl[k][W])
        scale = max(np.abs(dz).max(), np.abs(dnuW).max() if na[k] else 0.0)
        dnu = o["dbupper"][k] + o["dblower"][k]
        e1, e2 = np.abs(o["dz"][k] - dz).max(), (np.abs(dnu[W] - dnuW).max() if na[k] else 0.0)
        worst = max(worst, e1 / scale, e2 / scale)
        assert e1 <= tol * scale and e2 <= tol * scale, (k, e1, e2, scale)
        # zeros off W, each dnu_i on exactly one side, and that side is where the row sits
        off = np.ones(m, bool)
        off[W] = False
        assert not o["dbupper"][k][off].any() and not o["dblower"][k][off].any(), k
        assert not ((o["dbupper"][k] != 0) & (o["dblower"][k] != 0)).any(), k
        cx = Cm @ r["x"][k]
        for i in W:
            if o["dbupper"][k][i] != 0:
                assert abs(cx[i] - q["bupper"][k][i]) < side_tol, (k, i)
            if o["dblower"][k][i] != 0:
                assert abs(cx[i] - q["blower"][k][i]) < side_tol, (k, i)
    print(f"max relative error against the dense KKT solve: {worst:.2e}")
    return na, ws


def _same_bits(a, b, tag=""):
    for key in KEYS:
        assert B.bits_equal(a[key], b[key]), (tag, key)
    assert np.array_equal(a["status"], b["status"]), tag


# ---------------------------------------------------------------------------------------------------------------------------
# the Gram route against the dense solve: every mapping of k_backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: "n%d_m%d_ms%d_na%d" % c)
def test_dual_adjoint_equals_dense_kkt(gpu_lib, case):
    import daqp_amd
    n, m, ms, nact = case
    q = T._generate(N, n, m, ms, nact)
    bm, r = T._solve(q, ms, init_mask=daqp_amd.UPDATE_unconstrained if nact == 0 else 0)
    gx, gl = T._grad(N, n), _grad_lam(N, m)
    o = bm.backward(gx, out="numpy", grad_lam=gl)
    na, ws = _check(bm, q, r, gx, gl, o, ms)
    if nact == 0:       # the shortcut: W is empty, dz = H^-1 g and grad_lam is ignored
        assert (na == 0).all() and (r["iter"] == 1).all()
        _same_bits(o, bm.backward(gx, out="numpy"), "empty W")
    if nact == n:       # a vertex: C_W dz = g_lamW, so |g_lamW|_max <= n |C_W|_max |dz|_max -- dz is NOT small any more
        assert (na == n).all()
        for k in range(N):
            W = ws[k, :n]
            assert np.abs(o["dz"][k]).max() >= 0.5 * np.abs(gl[k][W]).max() / (n * np.abs(q["A"][k][W - ms]).max()), k
        assert np.abs(bm.backward(gx, out="numpy")["dz"]).max() <= TOL * np.abs(gx).max()
    if ms:
        assert (ws[ws >= 0] < ms).any(), "no active simple bound in the batch: the normalised rows of R^-1 are not exercised"
    bm.close()


def _raw(L, bm, gx, gl, dz, dbu, dbl, st, which=-1, null=()):
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    args = [ptr(gx), ptr(gl), ptr(dz), ptr(dbu), ptr(dbl), ptr(st)]
    for i in null:
        args[i] = None
    return L.daqp_batch_backward_dual(bm._h, *args, which, 1)


@pytest.mark.parametrize("case", [(12, 48, 0, 5), (80, 200, 0, 30)], ids=["wave", "workgroup"])
def test_gradient_combinations(gpu_lib, case):
    import torch
    n, m, ms, nact = case
    q = T._generate(N, n, m, ms, nact)
    bm, r = T._solve(q, ms)
    gx, gl = T._grad(N, n), _grad_lam(N, m)
    plain = bm.backward(gx, out="numpy")
    # grad_x = None is grad_x of zeros
    a, b = bm.backward(None, out="numpy", grad_lam=gl), bm.backward(np.zeros((N, n)), out="numpy", grad_lam=gl)
    _same_bits(a, b, "grad_x None")
    assert np.abs(a["dz"]).max() > 0 and not a["status"].any()
    # grad_lam = NULL through the C entry: the bits of daqp_batch_backward
    dd = dict(dtype=torch.float64, device="cuda")
    dz, dbu, dbl = torch.empty((N, n), **dd), torch.empty((N, m), **dd), torch.empty((N, m), **dd)
    st = torch.empty(N, dtype=torch.int32, device="cuda")
    assert _raw(gpu_lib, bm, torch.tensor(gx, **dd), None, dz, dbu, dbl, st) == 0
    torch.cuda.synchronize()
    got = dict(dz=dz.cpu().numpy(), dbupper=dbu.cpu().numpy(), dblower=dbl.cpu().numpy(), status=st.cpu().numpy())
    _same_bits(got, plain, "grad_lam NULL")
    # grad_lam of zeros compares equal
    z = bm.backward(gx, out="numpy", grad_lam=np.zeros((N, m)))
    for key in KEYS + ("status",):
        assert np.array_equal(z[key], plain[key]), key
    # entries of grad_lam off W change no output bit
    na, ws = bm.working_sets()
    gl2 = gl.copy()
    for k in range(N):
        off = np.ones(m, bool)
        off[ws[k, :na[k]]] = False
        gl2[k][off] = 1e6 * (1.0 + np.arange(off.sum()))
    full = bm.backward(gx, out="numpy", grad_lam=gl)
    _same_bits(bm.backward(gx, out="numpy", grad_lam=gl2), full, "off W")
    assert not B.bits_equal(full["dz"], plain["dz"])
    bm.close()


@pytest.mark.parametrize("case", [(12, 48, 0, 5), (80, 200, 0, 30)], ids=lambda c: "n%d" % c[0])
def test_host_and_device_memory_identical_bits(gpu_lib, case):
    import torch
    n, m, ms, nact = case
    q = T._generate(N, n, m, ms, nact)
    bm, r = T._solve(q, ms)
    gx, gl = T._grad(N, n), _grad_lam(N, m)
    h1 = bm.backward(gx, out="numpy", grad_lam=gl)
    d1 = bm.backward(torch.from_numpy(gx).cuda(), out="torch", grad_lam=torch.from_numpy(gl).cuda())
    h2 = bm.backward(gx, out="numpy", grad_lam=gl)
    assert all(d1[k].is_cuda for k in d1)
    d1 = {k: v.cpu().numpy() for k, v in d1.items()}
    _same_bits(h1, d1, "device")
    _same_bits(h1, h2, "host again")
    assert np.abs(h1["dz"]).max() > 0
    bm.close()


def test_dual_equality_row(gpu_lib):
    """bupper == blower on row 0 of every problem: the row is in every working set, on either side"""
    n, m, ms, nact = 12, 48, 0, 5
    q = T._generate(N, n, m, ms, nact)
    v = np.einsum("qk,qk->q", q["A"][:, 0, :], q["xref"]) + 0.05
    q["bupper"][:, 0] = v
    q["blower"][:, 0] = v
    bm, r = T._solve(q, ms)
    gx, gl = T._grad(N, n), _grad_lam(N, m)
    _check(bm, q, r, gx, gl, bm.backward(gx, out="numpy", grad_lam=gl), ms, expect_in_ws=0)
    bm.close()


def test_dual_shared_setup(gpu_lib):
    q = T._shared_problem()
    bm, r = T._solve(q, 0, shared=True)
    gx, gl = T._grad(N, 12), _grad_lam(N, 48)
    na, ws = _check(bm, q, r, gx, gl, bm.backward(gx, out="numpy", grad_lam=gl), 0)
    assert na.max() > 0 and len(set(map(tuple, ws.tolist()))) > 1
    bm.close()


def test_dual_exact_mode(gpu_lib, monkeypatch):
    monkeypatch.setenv("DAQP_AMD_EXACT", "1")
    n, m, ms, nact = 50, 150, 0, 20
    q = T._generate(N, n, m, ms, nact)
    bm, r = T._solve(q, ms)
    gx, gl = T._grad(N, n), _grad_lam(N, m)
    _check(bm, q, r, gx, gl, bm.backward(gx, out="numpy", grad_lam=gl), ms)
    bm.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the null-space route
# ---------------------------------------------------------------------------------------------------------------------------
def _model(name, settings=None):
    import daqp_amd
    c = B.CASES[name]
    n, m, ms = c["shape"]
    q = B.batch(name)
    bm = daqp_amd.BatchModel(q["f"].shape[0], n, m, ms, **(c.get("settings", {}) if settings is None else settings))
    bm.setup(*[q[k] for k in ("H", "f", "A", "bupper", "blower", "sense")])
    return q, bm, bm.solve()


def test_nullspace_mixed_batch(gpu_lib, monkeypatch):
    """n = 5: even problems positive definite (n_prox == 0), odd ones dense PSD of rank 3 (the batch of psd_n5).  which = 0: the
    proximal problems against the dense solve on the caller's H, the others bit for bit as which = -1 gives them."""
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    n, m, ms = B.CASES["psd_n5"]["shape"]
    psd, pd = B.batch("psd_n5"), B._definite(n, m, ms, 2, 8, 733)
    Nq = 16
    q = {key: np.stack([(pd if k % 2 == 0 else psd)[key][k // 2] for k in range(Nq)]) for key in B.KEYS + ("H",)}
    bm = daqp_amd.BatchModel(Nq, n, m, ms)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    r = bm.solve()
    assert (r["exitflag"] == 1).all()
    prox = bm.prox_info()["n_prox"] > 0
    assert np.array_equal(prox, np.arange(Nq) % 2 == 1)
    gx, gl = B.grad(Nq, n), _grad_lam(Nq, m)
    gram = bm.backward(gx, out="numpy", grad_lam=gl)
    assert (gram["status"][prox] == UNSUPPORTED).all() and not gram["status"][~prox].any()      # which = -1 reports -8 for them
    assert not gram["dz"][prox].any() and not gram["dbupper"][prox].any() and not gram["dblower"][prox].any()
    o = bm.backward(gx, out="numpy", nullspace=True, grad_lam=gl)
    assert not o["status"].any()
    for key in KEYS:
        assert B.bits_equal(o[key][~prox], gram[key][~prox]), key
    _check(bm, q, r, gx, gl, o, ms, tol=B.TOL, side_tol=1e-6)
    # and without grad_lam the C entry is daqp_batch_backward_nullspace, bit for bit
    assert not B.bits_equal(o["dz"][prox], bm.backward(gx, out="numpy", nullspace=True)["dz"][prox])
    bm.close()


@pytest.mark.parametrize("name", ["forced_n2", "forced_n16"])
def test_nullspace_agrees_with_the_gram_route(gpu_lib, monkeypatch, name):
    """positive definite H, no shift: which = 1 (every problem through the null-space kernel) against which = -1, at the tolerance
    tests/test_gpu_backward_nullspace.py holds the two algorithms to"""
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    q, bm, r = _model(name, settings={})
    Nq, n = q["f"].shape
    m = q["bupper"].shape[1]
    assert not bm.prox_info()["n_prox"].any()
    gx, gl = B.grad(Nq, n), _grad_lam(Nq, m)
    a, b = bm.backward(gx, out="numpy", nullspace="all", grad_lam=gl), bm.backward(gx, out="numpy", grad_lam=gl)
    worst = 0.0
    for k in range(Nq):
        assert a["status"][k] == 0 and b["status"][k] == 0, k
        da, db = a["dbupper"][k] + a["dblower"][k], b["dbupper"][k] + b["dblower"][k]
        scale = max(np.abs(b["dz"][k]).max(), np.abs(db).max())
        err = max(np.abs(a["dz"][k] - b["dz"][k]).max(), np.abs(da - db).max()) / scale
        worst = max(worst, err)
        assert err <= B.TOL, (name, k, err)
        assert np.array_equal(a["dbupper"][k] != 0, b["dbupper"][k] != 0) and np.array_equal(a["dblower"][k] != 0, b["dblower"][k] != 0), k
    # zeros in grad_lam compare equal to the existing entry for the same which
    z, p = bm.backward(gx, out="numpy", nullspace="all", grad_lam=np.zeros((Nq, m))), bm.backward(gx, out="numpy", nullspace="all")
    for key in KEYS + ("status",):
        assert np.array_equal(z[key], p[key]), key
    _same_bits(bm.backward(gx, out="numpy", nullspace=True, grad_lam=gl), b, "which 0 without proximal problems")
    bm.close()
    print(f"{name}: null-space kernel against the Gram route, dual right-hand side: {worst:.2e}")


def test_nullspace_lp_vertex_moves_with_the_multipliers(gpu_lib, monkeypatch):
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    q, bm, r = _model("lp_n5")
    Nq, n = q["f"].shape
    m, ms = q["bupper"].shape[1], B.CASES["lp_n5"]["shape"][2]
    gx, gl = B.grad(Nq, n), _grad_lam(Nq, m)
    gram = bm.backward(gx, out="numpy", grad_lam=gl)
    assert (gram["status"] == UNSUPPORTED).all() and not gram["dz"].any() and not gram["dbupper"].any() and not gram["dblower"].any()
    o = bm.backward(gx, out="numpy", nullspace=True, grad_lam=gl)
    na, ws = _check(bm, q, r, gx, gl, o, ms, tol=B.TOL, side_tol=1e-6)
    assert (na == n).all()
    for k in range(Nq):      # C_W dz = g_lamW with rows of C_W = e_i or A_i
        Cm = np.vstack([np.eye(n)[:ms], q["A"][k]])
        W = ws[k, :n]
        assert np.abs(o["dz"][k]).max() >= 0.5 * np.abs(gl[k][W]).max() / (n * np.abs(Cm[W]).max()), k
    assert not bm.backward(gx, out="numpy", nullspace=True)["dz"].any(), "without g_lam a vertex does not move"
    _same_bits(bm.backward(None, out="numpy", nullspace=True, grad_lam=gl), bm.backward(np.zeros((Nq, n)), out="numpy", nullspace=True, grad_lam=gl), "grad_x None")
    bm.close()


def _zero_outputs(o, which):
    return not o["dz"][which].any() and not o["dbupper"][which].any() and not o["dblower"][which].any()


def test_nullspace_not_locally_unique_is_singular(gpu_lib, monkeypatch):
    """-1 <= x <= 1 in two variables, LP with f = (1, 0): x_1 = -1 and x_2 is free along an edge, k = 1 < n"""
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    Nq = 3
    bm = daqp_amd.BatchModel(Nq, 2, 2, 2)
    bm.setup(None, np.tile([1.0, 0.0], (Nq, 1)), np.zeros((Nq, 0, 2)), np.ones((Nq, 2)), -np.ones((Nq, 2)))
    r = bm.solve()
    na, ws = bm.working_sets()
    assert (r["exitflag"] == 1).all() and (na == 1).all() and (ws[:, 0] == 0).all()
    for mode in (True, "all"):
        o = bm.backward(np.ones((Nq, 2)), out="numpy", nullspace=mode, grad_lam=np.ones((Nq, 2)))
        assert (o["status"] == SINGULAR).all() and _zero_outputs(o, slice(None)), (mode, o)
    bm.close()


def test_dependent_active_rows_are_singular(gpu_lib, monkeypatch):
    """the nearly parallel equality rows of tests/test_gpu_refine.py: the pivot ~ eps^2 = 1e-9 is below zero_tol = 1e-7 on both routes"""
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    q = TR.near_dependent()
    Nq, n = q["f"].shape
    m = q["bupper"].shape[1]
    bm = daqp_amd.BatchModel(Nq, n, m, 0, zero_tol=1e-7)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    r = bm.solve()
    na, ws = bm.working_sets()
    both = np.array([0 in ws[k, :na[k]] and 1 in ws[k, :na[k]] for k in range(Nq)])
    assert (r["exitflag"] == 1).all() and both.any()
    gx, gl = T._grad(Nq, n), _grad_lam(Nq, m)
    for mode in (False, "all"):
        o = bm.backward(gx, out="numpy", nullspace=mode, grad_lam=gl)
        assert (o["status"][both] == SINGULAR).all() and not o["status"][~both].any(), (mode, o["status"])
        assert _zero_outputs(o, both), mode
    bm.close()


# ---------------------------------------------------------------------------------------------------------------------------
# per-problem status and refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_infeasible_problem_reports_its_flag(gpu_lib):
    n, m, ms, nact = 12, 48, 0, 5
    q = T._generate(N, n, m, ms, nact)
    k = T._crossed(q)
    bm, r = T._solve(q, ms)
    assert r["exitflag"][k] == -1 and (np.delete(r["exitflag"], k) == 1).all()
    gx, gl = T._grad(N, n), _grad_lam(N, m)
    o = bm.backward(gx, out="numpy", grad_lam=gl)
    assert o["status"][k] == -1 and _zero_outputs(o, k)
    _check(bm, q, r, gx, gl, o, ms, only=[i for i in range(N) if i != k])
    bm.close()


def test_refusals_launch_nothing(gpu_lib):
    import torch
    import daqp_amd
    n, m, ms, nact = 12, 48, 0, 5
    q = T._generate(N, n, m, ms, nact)
    dd = dict(dtype=torch.float64, device="cuda")
    gx, gl = torch.randn(N, n, **dd), torch.randn(N, m, **dd)
    dz, dbu, dbl = torch.full((N, n), 7.0, **dd), torch.full((N, m), 7.0, **dd), torch.full((N, m), 7.0, **dd)
    st = torch.full((N,), 7, dtype=torch.int32, device="cuda")

    def untouched(*arrays):
        torch.cuda.synchronize()
        return all(bool((a == 7).all()) for a in (arrays or (dz, dbu, dbl, st)))

    def refused(bm, words, **kw):
        args = dict(gx=gx, gl=gl, dz=dz, dbu=dbu, dbl=dbl, st=st)
        args.update(kw.pop("args", {}))
        rc = _raw(gpu_lib, bm, args["gx"], args["gl"], args["dz"], args["dbu"], args["dbl"], args["st"], **kw)
        err = daqp_amd.last_error()
        assert rc != 0 and "daqp_batch_backward" in err and words in err, (rc, err, words)
        assert untouched()

    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
    for which in (-1, 0, 1):
        refused(bm, "successful daqp_batch_solve", which=which)                 # before the solve
    with pytest.raises(RuntimeError, match="successful daqp_batch_solve"):
        bm.backward(gx, grad_lam=gl)
    bm.solve()
    refused(bm, "both null", null=(0, 1))                                       # nothing to differentiate
    for null in range(2, 6):
        refused(bm, "null", null=(null,))                                       # an output
    for which in (-2, 2):
        refused(bm, "which", which=which)
    bm.update(f=q["f"] * 1.01)
    refused(bm, "successful daqp_batch_solve")                                  # update, no solve
    bm.solve()
    bm.reset()
    refused(bm, "successful daqp_batch_solve", which=0)                         # reset, no solve
    bm.solve()
    for null in ((), (0,)):
        assert _raw(gpu_lib, bm, gx, gl, dz, dbu, dbl, st, null=null) == 0      # and now it runs, with and without grad_x
        torch.cuda.synchronize()
        assert (st == 0).all() and not (dz == 7).any()
        dz.fill_(7.0), dbu.fill_(7.0), dbl.fill_(7.0), st.fill_(7)
    bm.close()
    soft = daqp_amd.BatchModel(N, n, m, ms, ns_max=1)
    soft.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
    soft.solve()
    for which in (-1, 0, 1):
        refused(soft, "ns_max > 0", which=which)                                # soft rows are not built
    with pytest.raises(RuntimeError, match="ns_max > 0"):
        soft.backward(gx, grad_lam=gl)
    soft.close()
    # which == 1 beyond one wavefront
    n2, m2 = 80, 200
    q2 = T._generate(4, n2, m2, 0, 30)
    big, _ = T._solve(q2, 0)
    a = dict(gx=torch.randn(4, n2, **dd), gl=torch.randn(4, m2, **dd), dz=torch.full((4, n2), 7.0, **dd), dbu=torch.full((4, m2), 7.0, **dd),
             dbl=torch.full((4, m2), 7.0, **dd), st=torch.full((4,), 7, dtype=torch.int32, device="cuda"))
    assert _raw(gpu_lib, big, a["gx"], a["gl"], a["dz"], a["dbu"], a["dbl"], a["st"], which=1) != 0 and "n <= 64" in daqp_amd.last_error()
    assert untouched(a["dz"], a["dbu"], a["dbl"], a["st"])
    with pytest.raises(RuntimeError, match="n <= 64"):
        big.backward(a["gx"], nullspace="all", grad_lam=a["gl"])
    big.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------------------------------
def _weights(seed=17, Nq=2, n=4, m=8):
    import torch
    rng = np.random.default_rng(seed)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
    return t(rng.standard_normal((Nq, n))), t(rng.standard_normal((Nq, m))), t(rng.standard_normal(Nq))


def _planted_base_is_safe(L, f, A, bu, bl, xs, lam_planted):
    """the base problem: the planted optimum, >= 0.01 of slack on the inactive rows and |lam| >= 1e-3 on the active ones, so that the
    perturbed solves (eps = 1e-6) keep the active set; fval is the objective at x"""
    import torch
    import daqp_amd
    eye = torch.eye(4, dtype=torch.float64, device="cuda")
    info = {}
    with torch.no_grad():
        H = L @ L.transpose(-1, -2) + eye
        x, lam, fval = daqp_amd.qp_layer(H, f, A, bu, bl, ms=2, info=info, returns=("x", "lam", "fval"))
    assert (info["exitflag"] == 1).all()
    assert np.abs(x.cpu().numpy() - xs).max() < 1e-9 and np.abs(lam.cpu().numpy() - lam_planted).max() < 1e-8
    lam_np = lam.cpu().numpy()
    active = lam_np != 0
    assert np.array_equal(active, lam_planted != 0) and np.abs(lam_np[active]).min() >= 1e-3
    Cm = torch.cat([eye[:2].expand(2, 2, 4), A.expand(2, 6, 4)], dim=1)
    cx = torch.einsum("qik,qk->qi", Cm, x)
    assert torch.minimum(bu - cx, cx - bl).cpu().numpy()[~active].min() >= 0.01
    want = 0.5 * torch.einsum("qi,qij,qj->q", x, H.expand(2, 4, 4), x) + (f * x).sum(1)
    assert (fval - want).abs().max() <= 1e-9 * max(1.0, float(want.abs().max()))      # (the project's tolerance of a solution)


@pytest.mark.parametrize("returns", [("x", "lam", "fval"), ("fval", "x", "lam"), "fval", "lam", ("lam", "fval")], ids=lambda r: r if isinstance(r, str) else "_".join(r))
@pytest.mark.parametrize("shared", [False, True], ids=["per_problem", "shared"])
def test_layer_gradcheck(gpu_lib, shared, returns):
    import torch
    import daqp_amd
    L, f, A, bu, bl, xs, lam_planted = T._planted(shared)
    eye = torch.eye(4, dtype=torch.float64, device="cuda")
    w = dict(zip(("x", "lam", "fval"), _weights()))
    names = (returns,) if isinstance(returns, str) else returns

    def fn(L, f, A, bu, bl):
        out = daqp_amd.qp_layer(L @ L.transpose(-1, -2) + eye, f, A, bu, bl, ms=2, returns=returns)
        out = (out,) if isinstance(returns, str) else out
        assert len(out) == len(names) and all(o.shape == w[k].shape for o, k in zip(out, names))
        return sum((o * w[k]).sum() for o, k in zip(out, names))

    _planted_base_is_safe(L.detach(), f.detach(), A.detach(), bu.detach(), bl.detach(), xs, lam_planted)
    assert torch.autograd.gradcheck(fn, (L, f, A, bu, bl), eps=1e-6, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("shared", [False, True], ids=["per_problem", "shared"])
def test_layer_returns_x_is_the_default_call(gpu_lib, shared):
    import torch
    import daqp_amd
    eye = torch.eye(4, dtype=torch.float64, device="cuda")
    g = _weights()[0]
    grads = []
    for kw in ({}, dict(returns="x"), dict(returns=("x",))):
        L, f, A, bu, bl, _, _ = T._planted(shared)
        x = daqp_amd.qp_layer(L @ L.transpose(-1, -2) + eye, f, A, bu, bl, ms=2, **kw)
        x = x[0] if isinstance(x, tuple) else x
        x.backward(g)
        grads.append([t.grad.cpu().numpy() for t in (L, f, A, bu, bl)])
    for other in grads[1:]:
        for a, b in zip(grads[0], other):
            assert np.abs(a).max() > 0 and B.bits_equal(a, b)


def test_layer_refuses_soft_rows_and_unknown_names(gpu_lib):
    import torch
    import daqp_amd
    L, f, A, bu, bl, _, _ = T._planted(False)
    H = L @ L.transpose(-1, -2) + torch.eye(4, dtype=torch.float64, device="cuda")
    sense = torch.zeros(8, dtype=torch.int32)
    sense[3] = 8
    for returns in ("lam", ("x", "lam"), "fval"):
        with pytest.raises(ValueError, match="SOFT"):
            daqp_amd.qp_layer(H, f, A, bu, bl, ms=2, sense=sense, returns=returns)
    daqp_amd.qp_layer(H, f, A, bu, bl, ms=2, sense=sense, returns="x")      # the default route takes them as before
    with pytest.raises(ValueError, match="returns"):
        daqp_amd.qp_layer(H, f, A, bu, bl, ms=2, returns=("x", "slack"))


def test_layer_strict_and_lenient(gpu_lib):
    import torch
    import daqp_amd
    n, m, ms, nact = 12, 48, 0, 5
    q = T._generate(N, n, m, ms, nact)
    k = T._crossed(q)
    t = {key: torch.tensor(q[key], device="cuda", requires_grad=True) for key in ("H", "f", "A", "bupper", "blower")}
    keep = torch.ones(N, dtype=torch.float64, device="cuda")
    keep[k] = 0          # (the outputs of the infeasible problem are not a solution: they stay out of the loss)
    loss = lambda x, lam, fval: (x * keep[:, None]).sum() + (lam * keep[:, None]).sum() + (fval * keep).sum()
    with pytest.raises(RuntimeError, match="no derivative"):
        loss(*daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], returns=("x", "lam", "fval"))).backward()
    with pytest.raises(RuntimeError, match="no derivative"):      # no launch on this route: the exit flag of the solve speaks
        daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], returns="fval").sum().backward()
    info = {}
    loss(*daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], strict=False, info=info, returns=("x", "lam", "fval"))).backward()
    st = info["status"].cpu().numpy()
    assert st[k] == -1 and not np.delete(st, k).any()
    for key in t:
        gk = t[key].grad
        assert gk is not None and not gk[k].any() and torch.isfinite(gk).all(), key
    assert t["f"].grad.abs().max() > 0 and t["A"].grad.abs().max() > 0 and t["H"].grad.abs().max() > 0
