"""daqp_batch_backward / BatchModel.backward / qp_layer: the adjoint of a solved batch against a dense KKT solve in numpy, and the
autograd layer against finite differences.

Tolerance of the adjoint: 1e-9 relative in the max norm (the default-mode tolerance of test_golden_quadprog), relative to the max
norm of the KKT system's solution [dz; dnu] -- one linear system, one scale (at a vertex dz is zero and has no scale of its own).
cond_2(K) <= 5e4 on these draws, so both routes sit at 1e-11 or better."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SEED, TOL = 37, 7, 1e-9
# (n, m, ms, n_active): smallest | vertex: dz = 0 | unconstrained shortcut | active simple bounds, normalised rows of R^-1 | C3 |
# C2, the headline kernel family | cap 65 | the workgroup path (wg_inverse) | rows and Gram matrix beyond LDS: the HBM scratch
CASES = [(3, 8, 0, 2), (3, 8, 0, 3), (4, 8, 0, 0), (6, 40, 6, 4), (12, 48, 0, 5), (50, 150, 0, 20), (64, 256, 0, 30), (80, 200, 0, 30),
         (128, 192, 0, 40)]
UNSUPPORTED, SINGULAR = -8, -20


def _generate(Nq, n, m, ms, na, seed=SEED):
    from daqp_amd.synthetic import generate_batch_torch
    q = generate_batch_torch(Nq, n, m, ms, na, seed)
    return {k: v.cpu().numpy() for k, v in q.items()}


def _solve(q, ms, init_mask=0, shared=False, H=None):
    import daqp_amd
    Nq, n = q["f"].shape
    bm = daqp_amd.BatchModel(Nq, n, q["bupper"].shape[1], ms)
    if shared:
        bm.setup_shared(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
    else:
        bm.setup(H if H is not None else q["H"], q["f"], q["A"], q["bupper"], q["blower"], init_mask=init_mask)
    return bm, bm.solve()


def _grad(Nq, n, seed=11):
    return np.random.default_rng(seed).standard_normal((Nq, n))


def _check(bm, q, r, g, o, ms, only=None, expect_in_ws=None):
    """every assertion of the adjoint test for the problems in `only` (default: all)"""
    Nq, n = q["f"].shape
    m = q["bupper"].shape[1]
    na, ws = bm.working_sets()
    worst = 0.0
    for k in (range(Nq) if only is None else only):
        H = q["H"] if q["H"].ndim == 2 else q["H"][k]
        A = q["A"] if q["A"].ndim == 2 else q["A"][k]
        Cm = np.vstack([np.eye(n)[:ms], A])
        x, lam = r["x"][k], r["lam"][k]
        assert r["exitflag"][k] == 1 and o["status"][k] == 0, (k, r["exitflag"][k], o["status"][k])
        # the sign convention the formulas assume
        assert np.abs(H @ x + q["f"][k] + Cm.T @ lam).max() <= 1e-9 * np.abs(q["f"][k]).max(), k
        W = ws[k, :na[k]]
        assert len(set(W.tolist())) == na[k] and (W >= 0).all() and (W < m).all()
        if expect_in_ws is not None:
            assert expect_in_ws in W, (k, W)
        K = np.zeros((n + na[k], n + na[k]))
        K[:n, :n] = H
        K[:n, n:] = Cm[W].T
        K[n:, :n] = Cm[W]
        sol = np.linalg.solve(K, np.concatenate([g[k], np.zeros(na[k])]))
        scale = np.abs(sol).max()
        dnu = o["dbupper"][k] + o["dblower"][k]
        e1, e2 = np.abs(o["dz"][k] - sol[:n]).max(), (np.abs(dnu[W] - sol[n:]).max() if na[k] else 0.0)
        worst = max(worst, e1 / scale, e2 / scale)
        assert e1 <= TOL * scale and e2 <= TOL * scale, (k, e1, e2, scale)
        # zeros off W, each dnu_i on exactly one side, and that side is where the row sits
        off = np.ones(m, bool)
        off[W] = False
        assert not o["dbupper"][k][off].any() and not o["dblower"][k][off].any(), k
        assert not ((o["dbupper"][k] != 0) & (o["dblower"][k] != 0)).any(), k
        cx = Cm @ x
        for i in W:
            if o["dbupper"][k][i] != 0:
                assert abs(cx[i] - q["bupper"][k][i]) < 1e-9, (k, i)
            if o["dblower"][k][i] != 0:
                assert abs(cx[i] - q["blower"][k][i]) < 1e-9, (k, i)
    print(f"max relative error against the dense KKT solve: {worst:.2e}")
    return na, ws


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_m%d_ms%d_na%d" % c)
def test_adjoint_equals_dense_kkt(gpu_lib, case):
    import daqp_amd
    n, m, ms, nact = case
    q = _generate(N, n, m, ms, nact)
    bm, r = _solve(q, ms, init_mask=daqp_amd.UPDATE_unconstrained if nact == 0 else 0)
    g = _grad(N, n)
    o = bm.backward(g, out="numpy")
    na, ws = _check(bm, q, r, g, o, ms)
    if nact == 0:       # the shortcut: W is empty, dz = H^-1 g
        assert (na == 0).all() and (r["iter"] == 1).all()
    if nact == n:       # a vertex: x does not move with f
        assert (na == n).all()
        assert np.abs(o["dz"]).max() <= TOL * np.abs(g).max()
    if ms:
        assert (ws[ws >= 0] < ms).any(), "no active simple bound in the batch: the normalised rows of R^-1 are not exercised"
    bm.close()


def test_adjoint_exact_mode(gpu_lib, monkeypatch):
    monkeypatch.setenv("DAQP_AMD_EXACT", "1")
    n, m, ms, nact = 50, 150, 0, 20
    q = _generate(N, n, m, ms, nact)
    bm, r = _solve(q, ms)
    g = _grad(N, n)
    _check(bm, q, r, g, bm.backward(g, out="numpy"), ms)
    bm.close()


def test_adjoint_single_problem(gpu_lib):
    n, m, ms, nact = 12, 48, 0, 5
    q = _generate(1, n, m, ms, nact)
    bm, r = _solve(q, ms)
    g = _grad(1, n)
    _check(bm, q, r, g, bm.backward(g, out="numpy"), ms)
    bm.close()


def _diag_problem(Nq=N, n=6, mA=4, seed=3):
    """diagonal H with simple bounds that the unconstrained optimum -f / d violates in most coordinates; x = 0 is feasible"""
    rng = np.random.default_rng(seed)
    d = 1.0 + 9.0 * rng.random((Nq, n))
    H = np.zeros((Nq, n, n))
    H[:, np.arange(n), np.arange(n)] = d
    f = 4.0 * rng.standard_normal((Nq, n))
    A = rng.standard_normal((Nq, mA, n))
    bu = np.concatenate([0.2 + 0.3 * rng.random((Nq, n)), 1.0 + rng.random((Nq, mA))], axis=1)
    bl = -np.concatenate([0.2 + 0.3 * rng.random((Nq, n)), 1.0 + rng.random((Nq, mA))], axis=1)
    return dict(H=H, f=f, A=A, bupper=bu, blower=bl)


def test_adjoint_diagonal_hessian(gpu_lib):
    """the RinvD route of the setup: rows < ms of R^-1 are kept un-normalised"""
    q = _diag_problem()
    bm, r = _solve(q, 6)
    g = _grad(N, 6)
    na, ws = _check(bm, q, r, g, bm.backward(g, out="numpy"), 6)
    assert (ws[ws >= 0] < 6).any() and (ws >= 6).any()
    bm.close()


def test_adjoint_equality_row(gpu_lib):
    """bupper == blower on row 0 of every problem: the row is in every working set, on either side"""
    n, m, ms, nact = 12, 48, 0, 5
    q = _generate(N, n, m, ms, nact)
    v = np.einsum("qk,qk->q", q["A"][:, 0, :], q["xref"]) + 0.05
    q["bupper"][:, 0] = v
    q["blower"][:, 0] = v
    bm, r = _solve(q, ms)
    g = _grad(N, n)
    _check(bm, q, r, g, bm.backward(g, out="numpy"), ms, expect_in_ws=0)
    bm.close()


def _shared_problem(Nq=N, n=12, mA=48, seed=5):
    base = _generate(1, n, mA, 0, 5)
    rng = np.random.default_rng(seed)
    return dict(H=base["H"][0], A=base["A"][0], f=30.0 * rng.standard_normal((Nq, n)),
                bupper=1.0 + rng.random((Nq, mA)), blower=-1.0 - rng.random((Nq, mA)))


def test_adjoint_shared_setup(gpu_lib):
    q = _shared_problem()
    bm, r = _solve(q, 0, shared=True)
    g = _grad(N, 12)
    na, ws = _check(bm, q, r, g, bm.backward(g, out="numpy"), 0)
    assert na.max() > 0 and len(set(map(tuple, ws.tolist()))) > 1, "the problems of the shared batch should differ in their working sets"
    bm.close()


@pytest.mark.parametrize("case", [(12, 48, 0, 5), (80, 200, 0, 30)], ids=lambda c: "n%d" % c[0])
def test_host_and_device_memory_identical_bits(gpu_lib, case):
    import torch
    n, m, ms, nact = case
    q = _generate(N, n, m, ms, nact)
    bm, r = _solve(q, ms)
    g = _grad(N, n)
    h1 = bm.backward(g, out="numpy")
    d1 = bm.backward(torch.from_numpy(g).cuda(), out="torch")
    h2 = bm.backward(g, out="numpy")
    for k in ("dz", "dbupper", "dblower", "status"):
        assert d1[k].is_cuda
        assert np.array_equal(h1[k], d1[k].cpu().numpy()) and np.array_equal(h1[k], h2[k]), k
    assert np.abs(h1["dz"]).max() > 0
    bm.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------------------------------
def _planted(shared, seed=2, Nq=2, n=4, mA=6, ms=2):
    """N = 2, n = 4, m = 8: simple bound 0 held at its upper side, general row 3 (constraint 5) at its lower side, multipliers 0.5;
    every other row has 0.5 of slack on both sides.  Leaves: L (H = L L' + I), f, A, bupper, blower."""
    import torch
    rng = np.random.default_rng(seed)
    L = np.tril(rng.standard_normal((n, n))) if shared else np.tril(rng.standard_normal((Nq, n, n)))
    A = rng.standard_normal((mA, n)) if shared else rng.standard_normal((Nq, mA, n))
    H = L @ np.swapaxes(L, -1, -2) + np.eye(n)
    xs = rng.standard_normal((Nq, n))
    Cm = np.concatenate([np.broadcast_to(np.eye(n)[:ms], (Nq, ms, n)), np.broadcast_to(A, (Nq, mA, n))], axis=1)
    cx = np.einsum("qik,qk->qi", Cm, xs)
    lam = np.zeros((Nq, ms + mA))
    lam[:, 0], lam[:, 5] = 0.5, -0.5
    f = -((H @ xs[:, :, None])[:, :, 0] + np.einsum("qik,qi->qk", Cm, lam))
    bu, bl = cx + 0.5, cx - 0.5
    bu[:, 0], bl[:, 0] = cx[:, 0], cx[:, 0] - 1.0
    bl[:, 5], bu[:, 5] = cx[:, 5], cx[:, 5] + 1.0
    t = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True)
    return t(L), t(f), t(A), t(bu), t(bl), xs, lam


@pytest.mark.parametrize("shared", [False, True], ids=["per_problem", "shared"])
def test_layer_gradcheck(gpu_lib, shared):
    import torch
    import daqp_amd
    L, f, A, bu, bl, xs, lam_planted = _planted(shared)
    eye = torch.eye(4, dtype=torch.float64, device="cuda")

    def fn(L, f, A, bu, bl):
        return daqp_amd.qp_layer(L @ L.transpose(-1, -2) + eye, f, A, bu, bl, ms=2)

    # the base problem: the planted optimum, >= 0.01 of slack on the inactive rows and |lam| >= 1e-3 on the active ones, so that the
    # perturbed solves (eps = 1e-6) keep the active set
    info = {}
    with torch.no_grad():
        x = daqp_amd.qp_layer(L @ L.transpose(-1, -2) + eye, f, A, bu, bl, ms=2, info=info)
    assert (info["exitflag"] == 1).all()
    assert np.abs(x.cpu().numpy() - xs).max() < 1e-9
    lam = info["lam"].cpu().numpy()
    active = lam != 0
    assert np.array_equal(active, lam_planted != 0) and np.abs(lam[active]).min() >= 1e-3
    Cm = torch.cat([eye[:2].expand(2, 2, 4), A.expand(2, 6, 4)], dim=1)
    cx = torch.einsum("qik,qk->qi", Cm, x)
    slack = torch.minimum(bu - cx, cx - bl).detach().cpu().numpy()
    assert slack[~active].min() >= 0.01
    assert torch.autograd.gradcheck(fn, (L, f, A, bu, bl), eps=1e-6, atol=1e-5, rtol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals and per-problem status
# ---------------------------------------------------------------------------------------------------------------------------
def _raw_backward(L, bm, g, dz, dbu, dbl, st, null=None):
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = [ptr(g), ptr(dz), ptr(dbu), ptr(dbl), ptr(st)]
    if null is not None:
        args[null] = None
    return L.daqp_batch_backward(bm._h, *args, 1)


def test_refusals_launch_nothing(gpu_lib):
    import torch
    import daqp_amd
    n, m, ms, nact = 12, 48, 0, 5
    q = _generate(N, n, m, ms, nact)
    dd = dict(dtype=torch.float64, device="cuda")
    g = torch.randn(N, n, **dd)
    dz, dbu, dbl = torch.full((N, n), 7.0, **dd), torch.full((N, m), 7.0, **dd), torch.full((N, m), 7.0, **dd)
    st = torch.full((N,), 7, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((dz == 7).all() and (dbu == 7).all() and (dbl == 7).all() and (st == 7).all())

    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
    assert _raw_backward(gpu_lib, bm, g, dz, dbu, dbl, st) != 0 and "daqp_batch_solve" in daqp_amd.last_error()      # before the solve
    with pytest.raises(RuntimeError):
        bm.backward(g)
    bm.solve()
    for null in range(5):
        assert _raw_backward(gpu_lib, bm, g, dz, dbu, dbl, st, null=null) != 0                                          # a NULL pointer
    assert untouched()
    bm.update(f=q["f"] * 1.01)
    assert _raw_backward(gpu_lib, bm, g, dz, dbu, dbl, st) != 0 and "daqp_batch_solve" in daqp_amd.last_error()      # update, no solve
    bm.solve()
    bm.reset()
    assert _raw_backward(gpu_lib, bm, g, dz, dbu, dbl, st) != 0                                                       # reset, no solve
    assert untouched()
    bm.solve()
    assert _raw_backward(gpu_lib, bm, g, dz, dbu, dbl, st) == 0                                                       # and now it runs
    torch.cuda.synchronize()
    assert (st == 0).all() and not (dz == 7).any()
    bm.close()
    dz.fill_(7.0)
    soft = daqp_amd.BatchModel(N, n, m, ms, ns_max=1)
    soft.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
    soft.solve()
    assert _raw_backward(gpu_lib, soft, g, dz, dbu, dbl, st) != 0 and "soft" in daqp_amd.last_error()                # soft constraints
    torch.cuda.synchronize()
    assert (dz == 7).all()
    soft.close()


def _crossed(q, k=5):
    q["blower"][k, 0] = q["bupper"][k, 0] + 1.0
    q["blower"][k, 1] = q["bupper"][k, 1] + 1.0
    return k


def test_infeasible_problem_reports_its_flag(gpu_lib):
    n, m, ms, nact = 12, 48, 0, 5
    q = _generate(N, n, m, ms, nact)
    k = _crossed(q)
    bm, r = _solve(q, ms)
    assert r["exitflag"][k] == -1 and (np.delete(r["exitflag"], k) == 1).all()
    g = _grad(N, n)
    o = bm.backward(g, out="numpy")
    assert o["status"][k] == -1
    assert not o["dz"][k].any() and not o["dbupper"][k].any() and not o["dblower"][k].any()
    _check(bm, q, r, g, o, ms, only=[i for i in range(N) if i != k])
    bm.close()


@pytest.mark.parametrize("kind", ["lp", "singular"])
def test_proximal_problems_are_unsupported(gpu_lib, kind):
    import daqp_amd
    Nq, n = 5, 4
    rng = np.random.default_rng(4)
    f = rng.standard_normal((Nq, n))
    bu, bl = np.ones((Nq, n)), -np.ones((Nq, n))
    H = None
    if kind == "singular":
        V = rng.standard_normal((Nq, n, 2))
        H = V @ np.swapaxes(V, 1, 2)
    bm = daqp_amd.BatchModel(Nq, n, n, n)
    bm.setup(H, f, None, bu, bl)
    r = bm.solve()
    assert (r["exitflag"] == 1).all() and (bm.prox_info()["n_prox"] > 0).all()
    o = bm.backward(_grad(Nq, n), out="numpy")
    assert (o["status"] == UNSUPPORTED).all()
    assert not o["dz"].any() and not o["dbupper"].any() and not o["dblower"].any()
    bm.close()


def test_layer_strict_and_lenient(gpu_lib):
    import torch
    import daqp_amd
    n, m, ms, nact = 12, 48, 0, 5
    q = _generate(N, n, m, ms, nact)
    k = _crossed(q)
    t = {key: torch.tensor(q[key], device="cuda", requires_grad=True) for key in ("H", "f", "A", "bupper", "blower")}
    x = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"])
    with pytest.raises(RuntimeError, match="no derivative"):
        x.sum().backward()
    info = {}
    x = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], strict=False, info=info)
    keep = torch.ones(N, 1, dtype=torch.float64, device="cuda")
    keep[k] = 0          # (x of the infeasible problem is not a solution: it stays out of the loss)
    (x * keep).sum().backward()
    st = info["status"].cpu().numpy()
    assert st[k] == -1 and not np.delete(st, k).any()
    for key in t:
        gk = t[key].grad
        assert gk is not None and not gk[k].any() and torch.isfinite(gk).all(), key
    assert t["f"].grad.abs().max() > 0 and t["A"].grad.abs().max() > 0 and t["H"].grad.abs().max() > 0
