"""daqp_batch_backward_soft_dual / BatchModel.backward_soft / qp_layer(..., soft_returns=True): the adjoint of a batch with soft rows
for a loss l(x, lam, fval, soft_slack),

    [ H    C_W' ] [ dz  ]   [ g_x       ]        ghat_lam_k = g_lam_k + 2 g_s rho_soft q_k lam_k  on the SOFT rows of W
    [ C_W  -S   ] [ dnu ] = [ ghat_lamW ],

against np.linalg.solve on the dense matrix at the GPU's own working set (tests/backward_soft_dual_cases.py), and the layer against
that file's numpy gradients, which tests/test_cpu_backward_soft_dual.py holds to central differences in np.longdouble.

Bounds: those tests/test_gpu_backward_soft.py holds the same batches to, read from it and unchanged -- TOL = 1e-9 relative to the max
norm of [dz; dnu], q_k at TOL of max(1, its max norm).  The matrix is the same; only the right-hand side differs.

The LDS pick.  The issue that asked for these kernels expected SOFT && DUAL to need more LDS than SOFT alone and a shape that moves a
path down.  No such shape exists: ghat_lam is kept in y[], a buffer of cap doubles that every instantiation carries and leaves idle
until the triangular solves, and gp[] (which DUAL writes) is a buffer of every instantiation as well -- backward_lds_bytes(n, cap, rl,
nl) is one function for all twelve kernels, so every shape runs the SOFT && DUAL kernel on the path its SOFT kernel runs on.  The
parity batches below cover all three paths (one wavefront; `workgroup`: rows and Gram matrix in LDS; `hbm_scratch`: in HBM)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_soft_dual", os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


D = _load("backward_soft_dual_cases")      # the batches, the dense oracle, the numpy gradients
TS = _load("test_gpu_backward_soft")       # _solve, _grad, TOL, _near_dependent

TOL = TS.TOL
SINGULAR = -20
KEYS7 = ("dz", "dbupper", "dblower", "qsoft", "usoft", "usoft_id", "status")


def _duals(q, seed=13):
    """random g_lam (N, m) and g_s (N,)"""
    N = q["f"].shape[0]
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, q["bupper"].shape[1])), rng.standard_normal(N)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(bm, q, r, gx, gl, gs, o, only=None, need_soft=True):
    """dz, dnu and qsoft of the problems in `only` (default: all) against the dense oracle at the GPU's own working set; None for a
    gradient is zero.  Returns the per-problem scale max(|dz|, |dnu|)."""
    N, n = q["f"].shape
    m, rho = q["bupper"].shape[1], q["settings"]["rho_soft"]
    na, ws = bm.working_sets()
    worst, with_soft, scales = 0.0, 0, np.zeros(N)
    for k in (range(N) if only is None else only):
        H, Cm, f, bu, bl, sense = D.problem(q, k)
        assert r["exitflag"][k] in (1, 2) and o["status"][k] == 0, (k, r["exitflag"][k], o["status"][k])
        W = ws[k, :na[k]]
        is_soft = ((sense[W] & D.SOFT) != 0).astype(float)
        with_soft += int(r["exitflag"][k] == 2 and is_soft.any())
        dz, dnuW, qW, U = D.dense_adjoint_dual(H, Cm, W, is_soft, rho, r["lam"][k][W], np.zeros(n) if gx is None else gx[k],
                                               np.zeros(na[k]) if gl is None else gl[k][W], 0.0 if gs is None else gs[k])
        scale = max(np.abs(dz).max(), np.abs(dnuW).max() if na[k] else 0.0)
        scales[k] = scale
        dnu = o["dbupper"][k] + o["dblower"][k]
        e1, e2 = np.abs(o["dz"][k] - dz).max(), (np.abs(dnu[W] - dnuW).max() if na[k] else 0.0)
        assert e1 <= TOL * scale and e2 <= TOL * scale, (k, e1, e2, scale)
        if scale > 0:      # (g_s alone on a problem without an active soft row: the right-hand side is zero, and so is the answer)
            worst = max(worst, e1 / scale, e2 / scale)
        off = np.ones(m, bool)
        off[W] = False
        assert not o["dbupper"][k][off].any() and not o["dblower"][k][off].any(), k
        assert not ((o["dbupper"][k] != 0) & (o["dblower"][k] != 0)).any(), k
        want_q = np.zeros(m)
        want_q[W] = qW * is_soft
        assert np.abs(o["qsoft"][k] - want_q).max() <= TOL * max(1.0, np.abs(want_q).max()), k
        assert not o["qsoft"][k][want_q == 0].any(), k
    print(f"max relative error against the dense KKT solve: {worst:.2e}; SOFT_OPTIMAL with an active soft row: {with_soft}")
    if need_soft and only is None:
        assert 2 * with_soft >= N, (with_soft, N)
    return scales


@pytest.mark.parametrize("name", list(D.PARITY))
def test_soft_dual_adjoint_equals_dense_kkt(gpu_lib, name):
    q = D.PARITY[name]()
    N, n = q["f"].shape
    bm, r = TS._solve(q)
    gx, (gl, gs) = TS._grad(N, n), _duals(q)
    o = bm.backward_soft(gx, gl, gs, r["lam"], out="numpy")
    _check(bm, q, r, gx, gl, gs, o)
    plain = bm.backward(gx, out="numpy")
    assert not _bits(o["dz"], plain["dz"]), "the dual right-hand side changed nothing"
    for key in ("qsoft", "usoft", "usoft_id"):      # q_k and u_k belong to the matrix, not to the right-hand side
        assert _bits(o[key], plain[key]), key
    bm.close()


@pytest.mark.parametrize("name", ["one_wave", "workgroup"])
def test_each_gradient_alone_and_their_sum(gpu_lib, name):
    """g_x, g_lam and g_s each alone (the other two NULL) against the dense oracle, and the three results against the joint call.  The
    system is linear, so they differ by rounding only: each of the four solves carries an error of about 2^-52 cond(K) of its own
    scale, cond_2(K) <= 5e4 on these draws (tests/test_gpu_backward.py, whose generator `workgroup` uses) -- so 4 * 2^-52 * 5e4 =
    4.4e-11 of the largest of the four scales, a twentieth of what the dense-oracle bound TOL = 1e-9 allows a single solve."""
    q = D.PARITY[name]()
    N, n = q["f"].shape
    bm, r = TS._solve(q)
    gx, (gl, gs) = TS._grad(N, n), _duals(q)
    joint = bm.backward_soft(gx, gl, gs, r["lam"], out="numpy")
    parts, scale = [], _check(bm, q, r, gx, gl, gs, joint)
    for a, b, c in ((gx, None, None), (None, gl, None), (None, None, gs)):
        o = bm.backward_soft(a, b, c, None if c is None else r["lam"], out="numpy")
        scale = np.maximum(scale, _check(bm, q, r, a, b, c, o))
        assert np.abs(o["dz"]).max() > 0
        parts.append(o)
    worst = 0.0
    for key in ("dz", "dbupper", "dblower"):
        diff = np.abs(parts[0][key] + parts[1][key] + parts[2][key] - joint[key]).max(1) / scale      # (every problem has an active row: scale > 0)
        worst = max(worst, diff.max())
    print(f"{name}: sum of the three single-gradient calls against the joint call: {worst:.2e} of the scale")
    assert worst <= 4 * 2.0 ** -52 * 5e4
    bm.close()


def _raw(L, bm, gx, gl, gs, lam, outs, st, null=()):
    """daqp_batch_backward_soft_dual on device tensors; outs = [dz, dbupper, dblower, qsoft, usoft, usoft_id]"""
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    args = [ptr(gx), ptr(gl), ptr(gs), ptr(lam)] + [ptr(t) for t in outs] + [ptr(st)]
    for i in null:
        args[i] = None
    return L.daqp_batch_backward_soft_dual(bm._h, *args, 1)


def _outs(N, n, m, ns, fill=7.0):
    import torch
    dd = dict(dtype=torch.float64, device="cuda")
    outs = [torch.full(s, fill, **dd) for s in ((N, n), (N, m), (N, m), (N, m), (N, ns, n))] + [torch.full((N, ns), int(fill), dtype=torch.int32, device="cuda")]
    return outs, torch.full((N,), int(fill), dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("name", ["one_wave", "workgroup", "hbm_scratch"])
def test_null_duals_are_the_soft_entry_bit_for_bit(gpu_lib, name):
    import torch
    q = D.PARITY[name]()
    N, n = q["f"].shape
    m, ns = q["bupper"].shape[1], q["ns_max"]
    bm, r = TS._solve(q)
    g = torch.tensor(TS._grad(N, n), device="cuda")
    a, sa = _outs(N, n, m, ns, 7.0)
    b, sb = _outs(N, n, m, ns, 5.0)
    assert TS._raw(gpu_lib, bm, "daqp_batch_backward_soft", g, a, sa) == 0
    assert _raw(gpu_lib, bm, g, None, None, None, b, sb) == 0
    torch.cuda.synchronize()
    for x, y in zip(a + [sa], b + [sb]):
        assert _bits(x.cpu().numpy(), y.cpu().numpy())
    assert (sa == 0).all() and a[0].abs().max() > 0 and a[3].abs().max() > 0
    # zero-filled duals compare equal to NULL ones
    z = bm.backward_soft(g, torch.zeros(N, m, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.float64, device="cuda"),
                         torch.tensor(r["lam"], device="cuda"), out="torch")
    for key, x in zip(KEYS7, a + [sa]):
        assert np.array_equal(z[key].cpu().numpy(), x.cpu().numpy()), key
    bm.close()


def test_ns_max_zero_is_the_dual_entry_bit_for_bit(gpu_lib):
    import torch
    import daqp_amd
    from daqp_amd.synthetic import generate_batch_torch
    for n, m, ms, nact in ((12, 48, 0, 5), (6, 40, 6, 4), (80, 200, 0, 30)):
        N = 37
        q = generate_batch_torch(N, n, m, ms, nact, 7)
        bm = daqp_amd.BatchModel(N, n, m, ms)
        bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
        r = bm.solve(out="torch")
        dd = dict(dtype=torch.float64, device="cuda")
        gx, gl, gs = torch.randn(N, n, **dd), torch.randn(N, m, **dd), torch.randn(N, **dd)
        want = bm.backward(gx, out="torch", grad_lam=gl)
        outs, st = _outs(N, n, m, 0, 5.0)
        assert _raw(gpu_lib, bm, gx, gl, gs, r["lam"], outs[:4] + [None, None], st) == 0
        torch.cuda.synchronize()
        for key, t in zip(("dz", "dbupper", "dblower"), outs):
            assert _bits(want[key].cpu().numpy(), t.cpu().numpy()), (n, key)
        assert torch.equal(want["status"], st) and (st == 0).all() and outs[0].abs().max() > 0 and not outs[3].any()
        bm.close()


def test_no_soft_row_active_ignores_grad_slack(gpu_lib):
    q = D.NO_SOFT_ACTIVE()
    N, n = q["f"].shape
    bm, r = TS._solve(q)
    assert (r["exitflag"] == 1).all()
    gx, (gl, gs) = TS._grad(N, n), _duals(q)
    a, b = bm.backward_soft(gx, gl, out="numpy"), bm.backward_soft(gx, gl, 1e3 * gs, r["lam"], out="numpy")
    for key in KEYS7:
        assert _bits(a[key], b[key]), key
    assert not a["status"].any() and np.abs(a["dz"]).max() > 0 and not a["qsoft"].any()
    _check(bm, q, r, gx, gl, gs, b, need_soft=False)
    bm.close()


def test_the_call_leaves_the_batch_state_alone(gpu_lib):
    """a backward, a warm update(f) + solve and a re-solve return the same bits with the new call in between and without it"""
    q = D.PARITY["one_wave"]()
    N, n = q["f"].shape
    gx, (gl, gs) = TS._grad(N, n), _duals(q)
    runs = []
    for with_call in (False, True):
        bm, r = TS._solve(q)
        call = (lambda res: bm.backward_soft(gx, gl, gs, res["lam"], out="numpy")) if with_call else (lambda res: None)
        call(r)
        b1 = bm.backward(gx, out="numpy")
        call(r)
        bm.update(f=q["f"] * 1.01)
        r2 = bm.solve()
        call(r2)
        r3 = bm.solve()
        call(r3)
        b3 = bm.backward(gx, out="numpy")
        runs.append([r, b1, r2, r3, b3])
        bm.close()
    for a, b in zip(*runs):
        assert a.keys() == b.keys()
        for key in a:
            assert _bits(a[key], b[key]), key
    assert not _bits(runs[0][0]["x"], runs[0][2]["x"]), "the update changed nothing"


def test_infeasible_and_singular_problems_report_their_status(gpu_lib):
    q = D.PARITY["one_wave"]()
    N, n = q["f"].shape
    k = 5
    for row in (0, 2):      # two hard rows (the SOFT ones are 1, 4, 7) with crossed bounds
        q["blower"][k, row] = q["bupper"][k, row] + 1.0
    bm, r = TS._solve(q)
    assert r["exitflag"][k] == -1 and (np.delete(r["exitflag"], k) > 0).all(), r["exitflag"]
    gx, (gl, gs) = TS._grad(N, n), _duals(q)
    o = bm.backward_soft(gx, gl, gs, r["lam"], out="numpy")
    assert o["status"][k] == -1 and not np.delete(o["status"], k).any()
    for key in ("dz", "dbupper", "dblower", "qsoft", "usoft"):
        assert not o[key][k].any(), key
    assert (o["usoft_id"][k] == -1).all()
    _check(bm, q, r, gx, gl, gs, o, only=[i for i in range(N) if i != k])
    bm.close()
    # dependent active hard rows: DAQP_BACKWARD_SINGULAR
    q = TS._near_dependent()
    N, n = q["f"].shape
    bm, r = TS._solve(q)
    na, ws = bm.working_sets()
    both = np.array([0 in ws[i, :na[i]] and 1 in ws[i, :na[i]] for i in range(N)])
    assert (r["exitflag"] > 0).all() and both.any()
    gl, gs = _duals(q)
    o = bm.backward_soft(TS._grad(N, n), gl, gs, r["lam"], out="numpy")
    assert (o["status"][both] == SINGULAR).all() and not o["status"][~both].any()
    for key in ("dz", "dbupper", "dblower", "qsoft", "usoft"):
        assert not o[key][both].any(), key
    assert (o["usoft_id"][both] == -1).all()
    bm.close()


def test_refusals_launch_nothing(gpu_lib):
    import torch
    import daqp_amd
    q = D.PARITY["one_wave"]()
    N, n = q["f"].shape
    m, ns = q["bupper"].shape[1], q["ns_max"]
    dd = dict(dtype=torch.float64, device="cuda")
    gx, gl, gs = torch.randn(N, n, **dd), torch.randn(N, m, **dd), torch.randn(N, **dd)
    outs, st = _outs(N, n, m, ns)

    def refused(words, **kw):
        rc = _raw(gpu_lib, bm, gx, gl, gs, lam, outs, st, **kw)
        err = daqp_amd.last_error()
        assert rc != 0 and "daqp_batch_backward_soft_dual" in err and words in err, (rc, err, words)
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in outs + [st])

    bm = daqp_amd.BatchModel(N, n, m, q["ms"], ns, **q["settings"])
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    lam = torch.zeros(N, m, **dd)
    refused("successful daqp_batch_solve")                                      # before the solve
    with pytest.raises(RuntimeError, match="successful daqp_batch_solve"):
        bm.backward_soft(gx, gl, gs, lam)
    lam = bm.solve(out="torch")["lam"]
    refused("all null", null=(0, 1, 2))                                         # nothing to differentiate
    refused("needs lam", null=(3,))                                             # grad_slack without lam
    for null in (4, 5, 6, 10):                                                  # dz, dbupper, dblower, status
        refused("null", null=(null,))
    bm.update(f=q["f"] * 1.01)
    refused("successful daqp_batch_solve")                                      # update, no solve
    with pytest.raises(ValueError, match="grad_lam"):
        bm.backward_soft(gx, gl[:, :-1])
    lam = bm.solve(out="torch")["lam"]
    with pytest.raises(RuntimeError, match="ns_max > 0"):                       # the dual entry keeps refusing soft models
        bm.backward(gx, grad_lam=gl)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs + [st])
    for null in ((), (0,), (1,), (2, 3), (0, 1), (7, 8, 9)):                    # and now it runs: any gradient may be NULL, and the soft arrays
        assert _raw(gpu_lib, bm, gx, gl, gs, lam, outs, st, null=null) == 0, null
        torch.cuda.synchronize()
        assert (st == 0).all() and not (outs[0] == 7).any()
        st.fill_(7), outs[0].fill_(7.0)
    bm.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------------------------------
NAMES = ("x", "lam", "fval", "soft_slack")
_layer_cache = {}


def _layer_reference(name):
    """the numpy gradients of every single name's loss (a.x, b.lam, c.fval, d.soft_slack, one dict per name) on a batch, at the working
    sets and the (x, lam) of a GPU solve -- computed once per batch and shared; a loss over several names is their sum"""
    if name in _layer_cache:
        return _layer_cache[name]
    import torch
    import daqp_amd
    q = D.PARITY[name]()
    N, n = q["f"].shape
    m, ms, rho = q["bupper"].shape[1], q["ms"], q["settings"]["rho_soft"]
    w = dict(zip(NAMES, D.weights(q)))
    info = {}
    t = {k: torch.tensor(q[k], device="cuda") for k in ("H", "f", "A", "bupper", "blower")}
    with torch.no_grad():
        x, lam, fval, slack = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=ms, sense=torch.tensor(q["sense"]),
                                                rho_soft=rho, info=info, returns=NAMES, soft_returns=True)
    flag = info["exitflag"].cpu().numpy()
    assert ((flag == 1) | (flag == 2)).all() and 2 * int((flag == 2).sum()) >= N
    x, lam, fval, slack = (v.cpu().numpy() for v in (x, lam, fval, slack))
    ref = {k: [] for k in NAMES}
    for k in range(N):
        H, Cm, f, bu, bl, sense = D.problem(q, k)
        W = np.nonzero(lam[k])[0]
        upper, is_soft = lam[k][W] > 0, ((sense[W] & D.SOFT) != 0).astype(float)
        # what the layer returns is what the formulas are about (tests/kkt_reference.py's definitions)
        qW = np.einsum("kj,kj->k", Cm[W], np.linalg.solve(H, Cm[W].T).T)
        want_slack = float((rho * qW * lam[k][W] ** 2 * is_soft).sum())
        assert abs(slack[k] - want_slack) <= 1e-9 * max(1.0, want_slack), (k, slack[k], want_slack)
        want_fval = 0.5 * x[k] @ H @ x[k] + f @ x[k] + 0.5 * want_slack
        assert abs(fval[k] - want_fval) <= 1e-9 * max(1.0, abs(want_fval)), (k, fval[k], want_fval)
        z = dict(a=np.zeros(n), b=np.zeros(m), c=0.0, d=0.0)
        for key, arg in zip(NAMES, "abcd"):
            ref[key].append(D.gradients(H, Cm, ms, W, upper, is_soft, rho, x[k], lam[k][W], **{**z, arg: w[key][k]}))
    out = {key: {g: np.stack([np.asarray(p[g]) for p in ref[key]]) for g in ("f", "H", "A", "bupper", "blower", "rho")} for key in NAMES}
    _layer_cache[name] = (q, w, out, lam)
    return _layer_cache[name]


def _layer_gradients(q, w, returns):
    import torch
    import daqp_amd
    t = {k: torch.tensor(q[k], device="cuda", requires_grad=True) for k in ("H", "f", "A", "bupper", "blower")}
    rho = torch.tensor(q["settings"]["rho_soft"], dtype=torch.float64, device="cuda", requires_grad=True)
    info = {}
    out = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=q["ms"], sense=torch.tensor(q["sense"]), rho_soft=rho,
                            info=info, returns=returns, soft_returns=True)
    names = (returns,) if isinstance(returns, str) else returns
    out = (out,) if isinstance(returns, str) else out
    assert len(out) == len(names) and all(o.shape == w[k].shape for o, k in zip(out, names))
    sum((o * torch.tensor(w[k], device="cuda")).sum() for o, k in zip(out, names)).backward()
    assert not info["status"].any()
    got = {k: t[k].grad.cpu().numpy() for k in ("H", "f", "A", "bupper", "blower")}
    got["rho"] = rho.grad.cpu().numpy()
    return got


@pytest.mark.parametrize("returns", [NAMES, "x", "lam", "fval", "soft_slack", ("soft_slack", "fval", "x")], ids=lambda r: r if isinstance(r, str) else "_".join(r))
@pytest.mark.parametrize("name", ["one_wave", "soft_equality", "shared"])
def test_layer_gradients_equal_the_numpy_formulas(gpu_lib, name, returns):
    """every input gradient of a random linear loss over `returns`, dl/drho_soft included, against the numpy gradients at the GPU's own
    working set, x and lam: the two differ by the adjoint solve alone, which is held to TOL of the scale of its solution; a gradient
    is a sum of products of that solution with x, lam, q_k and u_k (all O(1) here), so: TOL of max(1, |gradient|_inf) per problem,
    and of the batch sums for the arrays one plant shares.  An equality row (bupper == blower: the soft equality of `soft_equality`)
    may be held on either side (include/daqp_amd.h), so only the sum of its two bound gradients is defined: it is compared as
    dl/dbupper, with zero for dl/dblower, on both sides."""
    q, w, ref, lam = _layer_reference(name)
    names = (returns,) if isinstance(returns, str) else returns
    got = _layer_gradients(q, w, returns)
    eq = q["bupper"] == q["blower"]
    fold = lambda bu, bl: (np.where(eq, bu + bl, bu), np.where(eq, 0.0, bl))
    got["bupper"], got["blower"] = fold(got["bupper"], got["blower"])
    worst = 0.0
    for key in ("f", "H", "A", "bupper", "blower", "rho"):
        want = sum(ref[k][key] for k in names)
        if key in ("bupper", "blower"):
            want = fold(sum(ref[k]["bupper"] for k in names), sum(ref[k]["blower"] for k in names))[key == "blower"]
        if key == "rho" or (q["shared"] and key in ("H", "A")):
            want = want.sum(0)
            err = np.abs(got[key] - want).max() / max(1.0, np.abs(want).max())
        else:
            err = (np.abs(got[key] - want).reshape(want.shape[0], -1).max(1) / np.maximum(1.0, np.abs(want).reshape(want.shape[0], -1).max(1))).max()
        worst = max(worst, err)
        print(f"{name} {names} dl/d{key}: {err:.2e}")
        assert np.abs(want).max() > 0, key
    assert worst <= TOL, worst


def test_layer_end_to_end_central_difference(gpu_lib):
    """one central difference through two GPU solves on one_wave (step 1e-6 along backward_soft_dual_cases.fd_direction, in f and
    bupper) against the layer's gradients along that direction, per problem.  Problems whose working set differs between the two
    solves are skipped, at most 10 % of the batch (tests/test_cpu_backward_soft_dual.py establishes that on the reference library).
    Tolerance 1e-5 relative: eps cond / step is about 1e-16 1e3 / 1e-6."""
    import torch
    import daqp_amd
    q, w, ref, lam0 = _layer_reference("one_wave")
    N = q["f"].shape[0]
    Ef, Eb = D.fd_direction(q)
    got = _layer_gradients(q, w, NAMES)
    want = (got["f"] * Ef).sum(1) + (got["bupper"] * Eb).sum(1)
    h = D.FD_STEP
    tw = {k: torch.tensor(w[k], device="cuda") for k in NAMES}
    vals, lams = [], []
    for sgn in (1.0, -1.0):
        t = {k: torch.tensor(q[k], device="cuda") for k in ("H", "A", "blower")}
        f, bu = torch.tensor(q["f"] + sgn * h * Ef, device="cuda"), torch.tensor(q["bupper"] + sgn * h * Eb, device="cuda")
        with torch.no_grad():
            out = daqp_amd.qp_layer(t["H"], f, t["A"], bu, t["blower"], ms=q["ms"], sense=torch.tensor(q["sense"]), rho_soft=D.RHO, returns=NAMES,
                                    soft_returns=True)
        vals.append(sum((o * tw[k]).reshape(N, -1).sum(1) for o, k in zip(out, NAMES)).cpu().numpy())
        lams.append(np.sign(out[1].cpu().numpy()))
    keep = (lams[0] == lams[1]).all(1) & (lams[0] == np.sign(lam0)).all(1)
    fd = (vals[0] - vals[1]) / (2 * h)
    err = np.abs(fd - want) / np.maximum(1.0, np.abs(want))
    print(f"kept {int(keep.sum())} of {N} problems; worst error against the central difference: {err[keep].max():.2e}")
    assert 10 * int(keep.sum()) >= 9 * N
    assert err[keep].max() <= 1e-5
