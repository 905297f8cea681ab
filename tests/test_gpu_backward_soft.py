"""daqp_batch_backward_soft / BatchModel.backward with ns_max > 0 / qp_layer(sense=..., rho_soft=...): the adjoint of a batch with
soft rows against a dense KKT solve in numpy with -S in the (2,2) block, S = diag(rho_soft q_k), and the layer against finite
differences.  Tolerance and oracle are those of tests/test_gpu_backward.py: 1e-9 relative in the max norm of [dz; dnu]; q_k and u_k
at 1e-9 of their own max norm.  The batches come from tests/backward_soft_cases.py; tests/test_cpu_backward_soft.py holds them to
the same conditions on the reference library."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-9
UNSUPPORTED, SINGULAR, ITERLIMIT = -8, -20, -4

_spec = importlib.util.spec_from_file_location("backward_soft_cases", os.path.join(HERE, "backward_soft_cases.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)


def _solve(q, ns_max=None, **more):
    import daqp_amd
    N, n = q["f"].shape
    bm = daqp_amd.BatchModel(N, n, q["bupper"].shape[1], q["ms"], q["ns_max"] if ns_max is None else ns_max, **{**q["settings"], **more})
    if q["shared"]:
        bm.setup_shared(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    else:
        bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    return bm, bm.solve()


def _grad(N, n, seed=11):
    return np.random.default_rng(seed).standard_normal((N, n))


def _check(bm, q, r, g, o, only=None, need_soft=True):
    """every assertion of the parity cases for the problems in `only` (default: all); returns (n_active, WS)"""
    N, n = q["f"].shape
    m, ns, rho = q["bupper"].shape[1], bm.ns, q["settings"]["rho_soft"]
    na, ws = bm.working_sets()
    worst, with_soft = 0.0, 0
    for k in (range(N) if only is None else only):
        H, Cm, f, bu, bl, sense = S.problem(q, k)
        x, lam = r["x"][k], r["lam"][k]
        assert r["exitflag"][k] in (1, 2) and o["status"][k] == 0, (k, r["exitflag"][k], o["status"][k])
        assert np.abs(H @ x + f + Cm.T @ lam).max() <= 1e-9 * np.abs(f).max(), k      # the sign convention the formulas assume
        W = ws[k, :na[k]]
        assert len(set(W.tolist())) == na[k] and (W >= 0).all() and (W < m).all()
        is_soft = ((sense[W] & S.SOFT) != 0).astype(float)
        with_soft += int(r["exitflag"][k] == 2 and is_soft.any())
        dz, dnuW, qW, U = S.dense_adjoint(H, Cm, W, is_soft, rho, g[k])
        scale = max(np.abs(dz).max(), np.abs(dnuW).max() if na[k] else 0.0)
        dnu = o["dbupper"][k] + o["dblower"][k]
        e1, e2 = np.abs(o["dz"][k] - dz).max(), (np.abs(dnu[W] - dnuW).max() if na[k] else 0.0)
        worst = max(worst, e1 / scale, e2 / scale)
        assert e1 <= TOL * scale and e2 <= TOL * scale, (k, e1, e2, scale)
        off = np.ones(m, bool)
        off[W] = False
        assert not o["dbupper"][k][off].any() and not o["dblower"][k][off].any(), k
        assert not ((o["dbupper"][k] != 0) & (o["dblower"][k] != 0)).any(), k
        # each row on the side it is held at: a hard row at its bound, a soft row rho q_k lam_k beyond it
        cx = Cm @ x
        for j, i in enumerate(W):
            shift = rho * qW[j] * lam[i] * is_soft[j]
            if o["dbupper"][k][i] != 0:
                assert abs(cx[i] - bu[i] - shift) < 1e-9, (k, i)
            if o["dblower"][k][i] != 0:
                assert abs(cx[i] - bl[i] - shift) < 1e-9, (k, i)
        if ns == 0:
            continue
        # q_k on the SOFT rows of W and nowhere else; u_k and the ids in working-set order, unused slots zero / -1
        want_q = np.zeros(m)
        want_q[W] = qW * is_soft
        assert np.abs(o["qsoft"][k] - want_q).max() <= TOL * max(1.0, np.abs(want_q).max()), k
        assert not o["qsoft"][k][want_q == 0].any(), k
        sk = [j for j in range(na[k]) if is_soft[j]]
        assert len(sk) <= ns
        assert o["usoft_id"][k].tolist() == [int(W[j]) for j in sk] + [-1] * (ns - len(sk)), (k, o["usoft_id"][k], W)
        for slot, j in enumerate(sk):
            assert np.abs(o["usoft"][k, slot] - U[j]).max() <= TOL * np.abs(U[j]).max(), (k, slot)
        assert not o["usoft"][k, len(sk):].any(), k
    print(f"max relative error against the dense KKT solve: {worst:.2e}; SOFT_OPTIMAL with an active soft row: {with_soft}")
    if need_soft and only is None:
        assert 2 * with_soft >= N, (with_soft, N)
    return na, ws


@pytest.mark.parametrize("name", list(S.PARITY))
def test_soft_adjoint_equals_dense_kkt(gpu_lib, name):
    q = S.PARITY[name]()
    N, n = q["f"].shape
    bm, r = _solve(q)
    g = _grad(N, n)
    o = bm.backward(g, out="numpy")
    na, ws = _check(bm, q, r, g, o)
    sense_w = np.take_along_axis(q["sense"], np.maximum(ws, 0), axis=1) * (ws >= 0) * (np.arange(ws.shape[1])[None] < na[:, None])
    if name == "cap_beyond_n1":
        assert na.max() > n + 1, "no working set beyond n + 1 rows"
    if name in ("one_wave", "diag_h", "shared"):
        assert (((sense_w & S.SOFT) != 0) & (ws < q["ms"])).any(), "no active soft simple bound in the batch"
    if name == "diag_h":
        assert (ws >= q["ms"]).any()
    if name == "soft_equality":
        assert (ws[:, 0] == 3).all() or all(3 in ws[k, :na[k]] for k in range(N)), "the soft equality is in every working set"
        assert (o["dbupper"][:, 3] != 0).any() or (o["dblower"][:, 3] != 0).any()
    if name == "shared":
        assert len(set(map(tuple, ws.tolist()))) > 1
    bm.close()


def test_no_soft_row_active_equals_the_hard_adjoint(gpu_lib):
    import daqp_amd
    q = S.NO_SOFT_ACTIVE()
    N, n = q["f"].shape
    bm, r = _solve(q)
    g = _grad(N, n)
    o = bm.backward(g, out="numpy")
    assert (r["exitflag"] == 1).all()
    na, ws = _check(bm, q, r, g, o, need_soft=False)
    assert na.max() > 0 and not o["qsoft"].any() and not o["usoft"].any() and (o["usoft_id"] == -1).all()
    hard = daqp_amd.BatchModel(N, n, q["bupper"].shape[1], q["ms"], 0, **q["settings"])
    hard.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
    rh = hard.solve()
    oh = hard.backward(g, out="numpy")
    assert np.array_equal(np.sign(rh["lam"]), np.sign(r["lam"]))
    scale = max(np.abs(oh["dz"]).max(), np.abs(oh["dbupper"] + oh["dblower"]).max())
    for key in ("dz", "dbupper", "dblower"):
        assert np.abs(o[key] - oh[key]).max() <= TOL * scale, key
    bm.close()
    hard.close()


def _raw(L, bm, entry, g, outs, st, mem=1, null=None):
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    args = [ptr(g)] + [ptr(t) for t in outs] + [ptr(st)]
    if null is not None:
        args[null] = None
    return getattr(L, entry)(bm._h, *args, mem)


def test_ns_max_zero_through_the_new_entry_is_bit_identical(gpu_lib):
    import torch
    import daqp_amd
    from daqp_amd.synthetic import generate_batch_torch
    for n, m, ms, nact in ((12, 48, 0, 5), (6, 40, 6, 4), (80, 200, 0, 30)):
        N = 37
        q = generate_batch_torch(N, n, m, ms, nact, 7)
        bm = daqp_amd.BatchModel(N, n, m, ms)
        bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
        bm.solve()
        dd = dict(dtype=torch.float64, device="cuda")
        g = torch.randn(N, n, **dd)
        a = [torch.full((N, n), 7.0, **dd), torch.full((N, m), 7.0, **dd), torch.full((N, m), 7.0, **dd)]
        b = [torch.full((N, n), 5.0, **dd), torch.full((N, m), 5.0, **dd), torch.full((N, m), 5.0, **dd)]
        qs = torch.full((N, m), 5.0, **dd)
        sa, sb = torch.full((N,), 7, dtype=torch.int32, device="cuda"), torch.full((N,), 5, dtype=torch.int32, device="cuda")
        assert _raw(gpu_lib, bm, "daqp_batch_backward", g, a, sa) == 0
        assert _raw(gpu_lib, bm, "daqp_batch_backward_soft", g, b + [qs, None, None], sb) == 0
        torch.cuda.synchronize()
        for x, y in zip(a + [sa], b + [sb]):
            assert torch.equal(x, y)
        assert (sa == 0).all() and a[0].abs().max() > 0 and not qs.any()
        bm.close()


@pytest.mark.parametrize("name", ["one_wave", "workgroup"])
def test_soft_host_and_device_memory_identical_bits(gpu_lib, name):
    import torch
    q = S.PARITY[name]()
    N, n = q["f"].shape
    bm, r = _solve(q)
    g = _grad(N, n)
    h1 = bm.backward(g, out="numpy")
    d1 = bm.backward(torch.from_numpy(g).cuda(), out="torch")
    h2 = bm.backward(g, out="numpy")
    for k in ("dz", "dbupper", "dblower", "qsoft", "usoft", "usoft_id", "status"):
        assert d1[k].is_cuda
        assert np.array_equal(h1[k], d1[k].cpu().numpy()) and np.array_equal(h1[k], h2[k]), k
    assert np.abs(h1["dz"]).max() > 0 and h1["qsoft"].any() and (h1["usoft_id"] >= 0).any()
    bm.close()


def test_soft_refusals_launch_nothing(gpu_lib):
    import torch
    import daqp_amd
    q = S.PARITY["one_wave"]()
    N, n = q["f"].shape
    m, ns = q["bupper"].shape[1], q["ns_max"]
    dd = dict(dtype=torch.float64, device="cuda")
    g = torch.randn(N, n, **dd)
    outs = [torch.full(s, 7.0, **dd) for s in ((N, n), (N, m), (N, m), (N, m), (N, ns, n))] + [torch.full((N, ns), 7, dtype=torch.int32, device="cuda")]
    st = torch.full((N,), 7, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 7).all()) for t in outs + [st])

    soft = "daqp_batch_backward_soft"
    bm = daqp_amd.BatchModel(N, n, m, q["ms"], ns, **q["settings"])
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    assert _raw(gpu_lib, bm, soft, g, outs, st) != 0 and "daqp_batch_solve" in daqp_amd.last_error()          # before the solve
    with pytest.raises(RuntimeError):
        bm.backward(g)
    bm.solve()
    for null in (0, 1, 2, 3, 7):                                                                                # grad_x, dz, dbupper, dblower, status
        assert _raw(gpu_lib, bm, soft, g, outs, st, null=null) != 0 and "null" in daqp_amd.last_error()
    assert untouched()
    bm.update(f=q["f"] * 1.01)
    assert _raw(gpu_lib, bm, soft, g, outs, st) != 0 and "daqp_batch_solve" in daqp_amd.last_error()          # update, no solve
    assert untouched()
    bm.solve()
    assert _raw(gpu_lib, bm, "daqp_batch_backward", g, outs[:3], st) != 0 and "soft" in daqp_amd.last_error()  # the old entry still refuses
    assert untouched()
    for null in (4, 5, 6):                                                                                      # qsoft, usoft, usoft_id may be NULL
        assert _raw(gpu_lib, bm, soft, g, outs, st, null=null) == 0
    torch.cuda.synchronize()
    full = [t.clone() for t in outs]
    assert (st == 0).all() and not (outs[0] == 7).any()
    assert _raw(gpu_lib, bm, soft, g, outs, st) == 0
    torch.cuda.synchronize()
    for a, b in zip(full[:3], outs[:3]):
        assert torch.equal(a, b)
    bm.close()


def test_iteration_limit_reports_its_flag(gpu_lib):
    q = S.PARITY["one_wave"]()
    N, n = q["f"].shape
    bm, r = _solve(q, iter_limit=5)
    hit = r["exitflag"] == ITERLIMIT
    assert hit.any() and (r["exitflag"][~hit] > 0).all()
    g = _grad(N, n)
    o = bm.backward(g, out="numpy")
    assert (o["status"][hit] == ITERLIMIT).all() and not o["status"][~hit].any()
    for key in ("dz", "dbupper", "dblower", "qsoft", "usoft"):
        assert not o[key][hit].any(), key
    assert (o["usoft_id"][hit] == -1).all()
    if (~hit).any():
        _check(bm, q, r, g, o, only=np.nonzero(~hit)[0])
    bm.close()


def _near_dependent(N=16, n=5, mA=6, eps=3e-5, seed=9):
    """general rows 0 and 1 nearly parallel (relative distance eps), both equalities through one point; general row 3 SOFT and violated
    there.  With zero_tol = 1e-7 the solver (sing_tol 3.7e-11) keeps both rows, the adjoint's Cholesky (pivot ~ eps^2 = 1e-9
    of the normalised Gram matrix, a factor of ten or more either way, below zero_tol) does not."""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.standard_normal((N, n, n))) / np.sqrt(n)
    H = L @ np.swapaxes(L, 1, 2) + np.eye(n)
    A = rng.standard_normal((N, mA, n))
    A[:, 1] = A[:, 0] + eps * rng.standard_normal((N, n))
    xs = rng.standard_normal((N, n))
    ax = np.einsum("qik,qk->qi", A, xs)
    lam = np.zeros((N, mA))
    lam[:, 0] = lam[:, 1] = 0.5
    f = -((H @ xs[:, :, None])[:, :, 0] + np.einsum("qik,qi->qk", A, lam))
    bu, bl = ax + 0.5, ax - 0.5
    bu[:, :2] = bl[:, :2] = ax[:, :2]
    sense = np.zeros((N, mA), np.int32)
    sense[:, :2] = S.ACTIVE | S.IMMUTABLE
    sense[:, 3] = S.SOFT
    bu[:, 3] = ax[:, 3] - 0.3
    bl[:, 3] = ax[:, 3] - 1.3
    return dict(H=H, A=A, f=f, bupper=bu, blower=bl, sense=sense, ms=0, shared=False, ns_max=1, settings=dict(rho_soft=S.RHO, zero_tol=1e-7))


def test_dependent_active_hard_rows_are_singular(gpu_lib):
    q = _near_dependent()
    N, n = q["f"].shape
    bm, r = _solve(q)
    na, ws = bm.working_sets()
    both = np.array([0 in ws[k, :na[k]] and 1 in ws[k, :na[k]] for k in range(N)])
    assert (r["exitflag"] > 0).all() and both.any(), "the solver should hold both nearly parallel rows somewhere"
    o = bm.backward(_grad(N, n), out="numpy")
    assert (o["status"][both] == SINGULAR).all() and not o["status"][~both].any()
    for key in ("dz", "dbupper", "dblower", "qsoft", "usoft"):
        assert not o[key][both].any(), key
    assert (o["usoft_id"][both] == -1).all()
    bm.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------------------------------
def _planted_soft(shared, seed=2, N=2, n=4, mA=6, ms=2, rho=0.3):
    """the planted problem of tests/test_gpu_backward.py (simple bound 0 at its upper side, general row 3 = constraint 5 at its lower side,
    multipliers +-0.5, every other row 0.5 of slack) plus two SOFT rows forced active by bounds no x can meet: general rows 0 and 1
    (constraints 2, 3) are asked to sit 0.4 beyond general rows 4 and 5's reach -- their upper bounds lie below their lower-bound
    twins: row 1 is row 0 negated, so  a x <= v - 0.4  and  -a x <= -v - 0.4  cannot both hold.  Multipliers 0.5 each, so each soft
    row sits rho q 0.5 beyond its bound, clear of it (>= 0.01), and the hard problem is infeasible."""
    import torch
    rng = np.random.default_rng(seed)
    L = np.tril(rng.standard_normal((n, n))) if shared else np.tril(rng.standard_normal((N, n, n)))
    A = rng.standard_normal((mA, n)) if shared else rng.standard_normal((N, mA, n))
    A[..., 1, :] = -A[..., 0, :]
    H = L @ np.swapaxes(L, -1, -2) + np.eye(n)
    Hb, Ab = np.broadcast_to(H, (N, n, n)), np.broadcast_to(A, (N, mA, n))
    xs = rng.standard_normal((N, n))
    Cm = np.concatenate([np.broadcast_to(np.eye(n)[:ms], (N, ms, n)), Ab], axis=1)
    cx = np.einsum("qik,qk->qi", Cm, xs)
    lam = np.zeros((N, ms + mA))
    lam[:, 0], lam[:, 5], lam[:, 2], lam[:, 3] = 0.5, -0.5, 0.5, 0.7
    f = -((Hb @ xs[:, :, None])[:, :, 0] + np.einsum("qik,qi->qk", Cm, lam))
    bu, bl = cx + 0.5, cx - 0.5
    bu[:, 0], bl[:, 0] = cx[:, 0], cx[:, 0] - 1.0
    bl[:, 5], bu[:, 5] = cx[:, 5], cx[:, 5] + 1.0
    qk = np.einsum("qj,qj->q", Cm[:, 2], np.linalg.solve(Hb, Cm[:, 2][:, :, None])[:, :, 0])
    for i in (2, 3):          # held at the upper side, rho q lam beyond it
        bu[:, i] = cx[:, i] - rho * qk * lam[:, i]
        bl[:, i] = bu[:, i] - 1.0
    sense = np.zeros(ms + mA, np.int32)
    sense[[2, 3]] = S.SOFT
    t = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True)
    return t(L), t(f), t(A), t(bu), t(bl), t(np.array(rho)), torch.tensor(sense, device="cuda"), xs, lam


@pytest.mark.parametrize("shared", [False, True], ids=["per_problem", "shared"])
def test_soft_layer_gradcheck(gpu_lib, shared):
    """step and tolerances of tests/test_gpu_backward.py::test_layer_gradcheck; margins: >= 0.01 of slack on every inactive row, |lam| >=
    1e-3 on every active one, every soft row >= 0.01 beyond its bound (SOFT_OPTIMAL is far from its primal_tol threshold)"""
    import torch
    import daqp_amd
    L, f, A, bu, bl, rho, sense, xs, lam_planted = _planted_soft(shared)
    eye = torch.eye(4, dtype=torch.float64, device="cuda")

    def fn(L, f, A, bu, bl, rho):
        return daqp_amd.qp_layer(L @ L.transpose(-1, -2) + eye, f, A, bu, bl, ms=2, sense=sense, rho_soft=rho)

    info = {}
    with torch.no_grad():
        x = daqp_amd.qp_layer(L @ L.transpose(-1, -2) + eye, f, A, bu, bl, ms=2, sense=sense, rho_soft=rho, info=info)
    assert (info["exitflag"] == 2).all()
    assert np.abs(x.cpu().numpy() - xs).max() < 1e-9
    lam = info["lam"].cpu().numpy()
    active = lam != 0
    assert np.array_equal(active, lam_planted != 0) and np.abs(lam[active]).min() >= 1e-3
    assert np.abs(lam - lam_planted).max() < 1e-9
    Cm = torch.cat([eye[:2].expand(2, 2, 4), A.expand(2, 6, 4)], dim=1)
    cx = torch.einsum("qik,qk->qi", Cm, x)
    slack = torch.minimum(bu - cx, cx - bl).detach().cpu().numpy()
    assert slack[~active].min() >= 0.01
    assert (-slack[:, [2, 3]]).min() >= 0.01, "every soft row clearly beyond its bound"
    # the hard problem is infeasible: rows 2 and 3 ask for a x <= v - d1 and -a x <= -v - d2 with d1 + d2 > 0
    a_sum = (bu[:, 2] + bu[:, 3]).detach().cpu().numpy()
    assert (a_sum < -0.01).all()
    assert torch.autograd.gradcheck(fn, (L, f, A, bu, bl, rho), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_soft_layer_shapes_and_rho_gradient(gpu_lib):
    """sense of shape (m,), rho_soft as a float; exit flag 2 in info; dl/drho_soft arrives as a 0-dim tensor summed over the batch"""
    import torch
    import daqp_amd
    q = S.PARITY["one_wave"]()
    t = {k: torch.tensor(q[k], device="cuda", requires_grad=True) for k in ("H", "f", "A", "bupper", "blower")}
    rho = torch.tensor(S.RHO, dtype=torch.float64, requires_grad=True)      # (a CPU scalar: the gradient comes back to it)
    info = {}
    x = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=q["ms"], sense=torch.tensor(q["sense"][0]), rho_soft=rho, info=info)
    assert (info["exitflag"] == 2).any() and (info["exitflag"] > 0).all()
    x.sum().backward()
    assert rho.grad is not None and rho.grad.shape == () and rho.grad.abs() > 0 and not info["status"].any()
    x2 = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=q["ms"], sense=q["sense"][0], rho_soft=S.RHO)
    assert torch.equal(x, x2)
