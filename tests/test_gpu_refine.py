"""daqp_batch_refine / BatchModel.refine on the GPU.

Planted ill-conditioned cases (tests/refine_cases.py: exact integer data, cond(H) 1e8, the exact optimum known): after solve + refine
    E_after <= max(8 E_model, 2^-46)
with E_model from the CPU model of refine_cases (never from the kernel).  The floor is 64 units in the last place over the limiting
accuracy 2^-53 of fixed-precision refinement with doubled-precision residuals when cond 2^-53 << 1: a margin, not a measurement.
Well-conditioned families of tests/kkt_cases.py through every solve kernel family: the refined x stays within 1e-9 of the solve's,
the merit is not worse, fval is the certificate's objective to the contract bound of certify.hip.h (fval_tol).  Status, refusals, no side effects, host and device memory."""
import ctypes as C

import numpy as np
import pytest

import kkt_cases as K
import refine_cases as RC

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -46
UNSUPPORTED, SINGULAR = -8, -20
ENV_KEYS = sorted({k for f in K.FAMILIES for k in f["env"]})
def fval_tol(H, f, x, a, b):
    """bound of |a - b| for two values of 1/2 x'Hx + f'x that each meet the contract of certify.hip.h, per problem:
    |computed - exact| <= 2^-52 |exact| + (K + 2)^2 2^-104 S with K = n^2 + n terms and S = 1/2 |x|'|H||x| + |f|'|x| (the S_obj of
    tests/test_gpu_certify.py).  Two such values differ by at most twice that; |exact| <= max(|a|, |b|) (1 + 2^-40), since either value is
    within the bound of it."""
    n = x.shape[1]
    ax = np.abs(x)
    S = 0.5 * np.einsum("qi,qij,qj->q", ax, np.abs(np.broadcast_to(H, (x.shape[0], n, n))), ax) + np.einsum("qi,qi->q", np.abs(f), ax)
    Kt = n * n + n
    return 2.0 * (2.0 ** -52 * np.maximum(np.abs(a), np.abs(b)) * (1.0 + 2.0 ** -40) + (Kt + 2) ** 2 * 2.0 ** -104 * S)


def set_env(monkeypatch, env, exact):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DAQP_AMD_EXACT", "1" if exact else "0")
    if exact:
        monkeypatch.delenv("DAQP_AMD_NO_RECHECK", raising=False)
    else:
        monkeypatch.setenv("DAQP_AMD_NO_RECHECK", "1")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def planted_batch(i, N):
    """N copies of planted case i as device tensors, and a model set up on them"""
    import torch
    import daqp_amd
    p = RC.case(i)
    t = {k: torch.from_numpy(np.array(np.broadcast_to(p[k], (N,) + p[k].shape))).cuda() for k in ("H", "f", "A", "bupper", "blower")}
    bm = daqp_amd.BatchModel(N, p["n"], p["m"], p["ms"])
    bm.setup(t["H"], t["f"], t["A"], t["bupper"], t["blower"])
    return p, t, bm


def errors(p, o):
    return np.array([RC.error(p, x, lam) for x, lam in zip(np.asarray(o["x"]), np.asarray(o["lam"]))])


def ratio(c):
    return c["stationarity"] / c["stationarity_scale"]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
def test_planted_cases_reach_the_last_bits(gpu_lib, monkeypatch, exact):
    set_env(monkeypatch, {}, exact)
    came_in_off = 0
    for i, N in zip(range(len(RC.CASES)), (67, 3, 1, 3, 3)):
        p, t, bm = planted_batch(i, N)
        r = bm.solve(out="numpy")
        assert (r["exitflag"] == 1).all()
        x_in, lam_in = r["x"].copy(), r["lam"].copy()
        o = bm.refine(r)
        bar = max(8.0 * RC.model_error(i), FLOOR)
        e0, e1 = errors(p, r), errors(p, o)
        print(p["n"], "N", N, "E before %.2e after %.2e bar %.2e" % (e0.max(), e1.max(), bar), "steps", o["steps"].max(),
              "mu %.2e -> %.2e" % (o["residual_before"].max(), o["residual_after"].max()))
        assert (o["status"] == 0).all()
        assert (e1 <= bar).all(), (p["n"], e1.max(), bar)
        assert (o["residual_after"] <= o["residual_before"]).all() and (o["steps"] >= 1).all() and (o["steps"] <= 3).all()
        came_in_off += e0.min() >= 2.0 ** 10 * bar
        # lam off W is zero, and the caller's result is not modified
        off = np.setdiff1d(np.arange(p["m"]), p["W"])
        assert not o["lam"][:, off].any()
        assert bits_equal(r["x"], x_in) and bits_equal(r["lam"], lam_in)
        # an independent kernel agrees: the certificate's stationarity is no larger after than before
        c0, c1 = bm.certify(r, out="numpy"), bm.certify(o, out="numpy")
        assert (ratio(c1) <= ratio(c0)).all(), (ratio(c0), ratio(c1))
        Hn, fn = np.broadcast_to(p["H"], (N,) + p["H"].shape), np.broadcast_to(p["f"], (N, p["n"]))
        assert (np.abs(o["fval"] - c1["objective"]) <= fval_tol(Hn, fn, o["x"], o["fval"], c1["objective"])).all()
        bm.close()
    if exact:
        assert 2 * came_in_off >= len(RC.CASES), came_in_off


@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=[str(c["shape"][0]) for c in RC.CASES])
def test_from_zeros_the_kernel_solves_the_system(gpu_lib, monkeypatch, i):
    set_env(monkeypatch, {}, False)
    p, t, bm = planted_batch(i, 3)
    r = bm.solve(out="numpy")
    z = dict(x=np.zeros_like(r["x"]), lam=np.zeros_like(r["lam"]))
    o = bm.refine(z, max_steps=8)
    e = errors(p, o)
    print(p["n"], "E %.2e" % e.max(), "steps", o["steps"], "mu %.2e -> %.2e" % (o["residual_before"].max(), o["residual_after"].max()))
    assert (o["status"] == 0).all() and (o["steps"] >= 2).all()
    assert (e <= max(8.0 * RC.model_error(i), FLOOR)).all(), e.max()
    assert (o["residual_after"] <= o["residual_before"]).all() and not z["x"].any()
    bm.close()


def hard(p):
    """the family's problems with their SOFT bits cleared (refinement takes no soft rows): dict for a batch with ns_max = 0"""
    sense = None if p["sense"] is None else (p["sense"] & ~np.int32(8)).astype(np.int32)
    return dict(p, sense=sense, ns_max=0)


def check_family(tag, bm, p, data, r):
    """every assertion of the well-conditioned families on one solved batch"""
    import daqp_amd
    o = bm.refine(r)
    bw = bm.backward(np.zeros((p["N"], p["n"])), out="numpy")
    assert np.array_equal(o["status"], bw["status"]), (tag, o["status"], bw["status"])      # the rules of daqp_batch_backward
    ok = o["status"] == 0
    assert np.array_equal(ok | (o["status"] == SINGULAR), r["exitflag"] == 1), (tag, o["status"], r["exitflag"])
    bad = ~ok
    assert bits_equal(o["x"][bad], r["x"][bad]) and bits_equal(o["lam"][bad], r["lam"][bad]) and bits_equal(o["fval"][bad], r["fval"][bad]), tag
    assert not o["steps"][bad].any() and np.isnan(o["residual_before"][bad]).all() and np.isnan(o["residual_after"][bad]).all(), tag
    if not ok.any():
        return o
    assert (np.abs(o["x"][ok] - r["x"][ok]) <= 1e-9 * np.maximum(1.0, np.abs(r["x"][ok]))).all(), (tag, np.abs(o["x"] - r["x"])[ok].max())
    assert (o["residual_after"][ok] <= o["residual_before"][ok]).all(), tag
    H, A = data["H"], data["A"]
    c = daqp_amd.certify_batch(H, data["f"], A, data["bupper"], data["blower"], o["x"], o["lam"], sense=data.get("sense"), ms=p["ms"])
    assert (np.abs(o["fval"] - c["objective"]) <= fval_tol(H, data["f"], o["x"], o["fval"], c["objective"]))[ok].all(), tag
    print(tag, "ok", int(ok.sum()), "of", p["N"], "mu %.1e -> %.1e" % (o["residual_before"][ok].max(), o["residual_after"][ok].max()),
          "steps", o["steps"][ok].max(), "|dx| %.1e" % np.abs(o["x"] - r["x"])[ok].max())
    return o


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("variant", K.VARIANTS)
@pytest.mark.parametrize("name", ["reg21", "img3", "blk41", "wg70", "wg130", "generic"])
def test_well_conditioned_families(gpu_lib, monkeypatch, name, variant, exact):
    import daqp_amd
    fam, p = K.family(name), hard(K.problems(name, variant))
    set_env(monkeypatch, fam["env"], exact)
    bm = daqp_amd.BatchModel(p["N"], p["n"], p["m"], p["ms"])
    bm.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"])
    r = bm.solve()
    o = check_family((name, variant, exact), bm, p, p, r)
    if variant == "plain":
        assert (o["status"] == 0).all()
    bm.close()


def test_shared_setup(gpu_lib, monkeypatch):
    import daqp_amd
    set_env(monkeypatch, {}, False)
    base = K.problems("reg21", "plain")
    n, m, ms, N = base["n"], base["m"], base["ms"], base["N"]
    rng = np.random.default_rng(5)
    data = dict(H=base["H"][0], A=base["A"][0], f=base["f"] + 0.3 * rng.standard_normal((N, n)), bupper=base["bupper"][:1] + rng.random((N, m)),
                blower=base["blower"][:1] - rng.random((N, m)))
    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup_shared(data["H"], data["f"], data["A"], data["bupper"], data["blower"])
    r = bm.solve()
    assert (r["exitflag"] == 1).all()
    o = check_family("shared", bm, dict(N=N, n=n, m=m, ms=ms), data, r)
    assert (o["status"] == 0).all() and len(set(map(tuple, (o["lam"] != 0).tolist()))) > 1
    bm.close()


def test_diagonal_hessian_with_bounds_and_the_unconstrained_shortcut(gpu_lib, monkeypatch):
    import daqp_amd
    set_env(monkeypatch, {}, False)
    N, n, mA = 37, 6, 4
    rng = np.random.default_rng(3)
    H = np.zeros((N, n, n))
    H[:, np.arange(n), np.arange(n)] = 1.0 + 9.0 * rng.random((N, n))
    A = rng.standard_normal((N, mA, n))
    bu = np.concatenate([0.2 + 0.3 * rng.random((N, n)), 1.0 + rng.random((N, mA))], axis=1)
    data = dict(H=H, f=4.0 * rng.standard_normal((N, n)), A=A, bupper=bu, blower=-bu[:, ::-1].copy())
    bm = daqp_amd.BatchModel(N, n, n + mA, n)
    bm.setup(data["H"], data["f"], data["A"], data["bupper"], data["blower"])
    r = bm.solve()
    o = check_family("diag", bm, dict(N=N, n=n, m=n + mA, ms=n), data, r)
    assert (o["status"] == 0).all() and (o["lam"][:, :n] != 0).any() and (o["lam"][:, n:] != 0).any()
    bm.close()
    # no row can be active: the setup's shortcut leaves an empty working set, and refinement is that of H x = -f
    wide = dict(data, bupper=np.full_like(bu, 1e3), blower=np.full_like(bu, -1e3), H=H + 0.1 * (A[:, :1].transpose(0, 2, 1) @ A[:, :1]))
    bm = daqp_amd.BatchModel(N, n, n + mA, n)
    bm.setup(wide["H"], wide["f"], wide["A"], wide["bupper"], wide["blower"], init_mask=64)
    r = bm.solve()
    o = check_family("shortcut", bm, dict(N=N, n=n, m=n + mA, ms=n), wide, r)
    assert (o["status"] == 0).all() and not o["lam"].any()
    assert np.abs(np.einsum("qij,qj->qi", wide["H"], o["x"]) + wide["f"]).max() < 1e-12
    bm.close()


def near_dependent(N=16, n=5, mA=6, eps=3e-5, seed=9):
    """The hard rows of tests/test_gpu_backward_soft.py::_near_dependent without its SOFT row: general rows 0 and 1 nearly parallel
    (relative distance eps), both ACTIVE | IMMUTABLE equalities through one point, every other row 0.5 away on both sides.  With
    zero_tol = 1e-7 the solver (sing_tol 3.7e-11) keeps both rows; the pivot of the unit-row Gram Cholesky is ~ eps^2 = 1e-9, below
    zero_tol."""
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
    sense[:, :2] = 1 | 4      # DAQP_ACTIVE | DAQP_IMMUTABLE
    return dict(H=H, A=A, f=f, bupper=bu, blower=bl, sense=sense)


@pytest.mark.parametrize("memory", ["host", "device"])
def test_dependent_active_rows_are_singular_and_come_back_unchanged(gpu_lib, monkeypatch, memory):
    """status -20 from the Gram pivot, found after N_W and G were built: x, lam and fval bit for bit as they came in, no step, NaN residuals"""
    import torch
    import daqp_amd
    set_env(monkeypatch, {}, False)
    q = near_dependent()
    N, n = q["f"].shape
    m = q["bupper"].shape[1]
    bm = daqp_amd.BatchModel(N, n, m, 0, zero_tol=1e-7)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    r = bm.solve()
    na, ws = bm.working_sets()
    both = np.array([0 in ws[k, :na[k]] and 1 in ws[k, :na[k]] for k in range(N)])
    assert (r["exitflag"] == 1).all() and both.any(), "the solver should hold both nearly parallel rows somewhere"
    marked = dict(x=r["x"] + 0.125, lam=r["lam"] - 0.25, fval=r["fval"] + 3.0)      # not the solve's own outputs: nothing may be restored from the batch
    given = {k: torch.from_numpy(v).cuda() for k, v in marked.items()} if memory == "device" else marked
    o = bm.refine(given, max_steps=8, out="numpy")
    assert (o["status"][both] == SINGULAR).all() and not o["status"][~both].any(), o["status"]
    assert np.array_equal(o["status"], bm.backward(np.zeros((N, n)), out="numpy")["status"])
    for key in ("x", "lam", "fval"):
        assert bits_equal(o[key][both], marked[key][both]), key
    assert not o["steps"][both].any() and np.isnan(o["residual_before"][both]).all() and np.isnan(o["residual_after"][both]).all()
    if (~both).any():
        assert (o["residual_after"][~both] <= o["residual_before"][~both]).all()
    bm.close()


def _raw(L, bm, x, lam, st, max_steps=3, null=None):
    args = [C.c_void_p(t.data_ptr()) for t in (x, lam)] + [None, None, None, C.c_void_p(st.data_ptr())]
    if null is not None:
        args[null] = None
    return L.daqp_batch_refine(bm._h, *args, max_steps, 1)


def test_refusals_launch_nothing(gpu_lib, monkeypatch):
    import torch
    import daqp_amd
    set_env(monkeypatch, {}, False)
    p = K.problems("reg21", "plain")
    N, n, m, ms = p["N"], p["n"], p["m"], p["ms"]
    dd = dict(dtype=torch.float64, device="cuda")
    x, lam = torch.full((N, n), 7.0, **dd), torch.full((N, m), 7.0, **dd)
    st = torch.full((N,), 7, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((x == 7).all() and (lam == 7).all() and (st == 7).all())

    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"])
    assert _raw(gpu_lib, bm, x, lam, st) != 0 and "daqp_batch_solve" in daqp_amd.last_error()          # before the solve
    r = bm.solve()
    for null in (0, 1, 5):
        assert _raw(gpu_lib, bm, x, lam, st, null=null) != 0                                            # a NULL x, lam or status
    for steps in (0, 9, -1):
        assert _raw(gpu_lib, bm, x, lam, st, max_steps=steps) != 0 and "max_steps" in daqp_amd.last_error()
        with pytest.raises(RuntimeError, match="max_steps"):
            bm.refine(r, max_steps=steps)
    bm.update(f=p["f"] * 1.01)
    assert _raw(gpu_lib, bm, x, lam, st) != 0 and "daqp_batch_solve" in daqp_amd.last_error()          # update, no solve
    with pytest.raises(RuntimeError):
        bm.refine(r)
    assert untouched()
    bm.solve()
    assert _raw(gpu_lib, bm, x, lam, st) == 0                                                           # and now it runs
    torch.cuda.synchronize()
    assert (st == 0).all() and not (x == 7).any()
    bm.close()
    x.fill_(7.0)
    soft = daqp_amd.BatchModel(N, n, m, ms, ns_max=2)
    soft.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"])
    soft.solve()
    assert _raw(gpu_lib, soft, x, lam, st) != 0 and "soft" in daqp_amd.last_error()                    # ns_max > 0
    torch.cuda.synchronize()
    assert (x == 7).all()
    soft.close()


def test_infeasible_and_iteration_limited_problems_report_their_flags(gpu_lib, monkeypatch):
    import daqp_amd
    set_env(monkeypatch, {}, False)
    p = K.problems("reg21", "plain")
    bu, bl = p["bupper"].copy(), p["blower"].copy()
    k = 5
    bl[k, p["ms"]:p["ms"] + 2] = bu[k, p["ms"]:p["ms"] + 2] + 1.0
    data = dict(p, bupper=bu, blower=bl)
    bm = daqp_amd.BatchModel(p["N"], p["n"], p["m"], p["ms"])
    bm.setup(p["H"], p["f"], p["A"], bu, bl)
    r = bm.solve()
    assert r["exitflag"][k] == -1 and (np.delete(r["exitflag"], k) == 1).all()
    o = check_family("infeasible", bm, p, data, r)
    assert o["status"][k] == -1 and (np.delete(o["status"], k) == 0).all()
    bm.close()
    bm = daqp_amd.BatchModel(p["N"], p["n"], p["m"], p["ms"], iter_limit=2)
    bm.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"])
    r = bm.solve()
    assert (r["exitflag"] == -4).any()
    o = check_family("iter_limit", bm, p, p, r)
    assert np.array_equal(o["status"] == -4, r["exitflag"] == -4)
    bm.close()


@pytest.mark.parametrize("kind", ["lp", "singular"])
def test_proximal_problems_are_unsupported(gpu_lib, monkeypatch, kind):
    import daqp_amd
    set_env(monkeypatch, {}, False)
    N, n = 5, 4
    rng = np.random.default_rng(4)
    f = rng.standard_normal((N, n))
    H = None
    if kind == "singular":
        V = rng.standard_normal((N, n, 2))
        H = V @ np.swapaxes(V, 1, 2)
    bm = daqp_amd.BatchModel(N, n, n, n)
    bm.setup(H, f, None, np.ones((N, n)), -np.ones((N, n)))
    r = bm.solve()
    assert (r["exitflag"] == 1).all() and (bm.prox_info()["n_prox"] > 0).all()
    o = bm.refine(r)
    assert (o["status"] == UNSUPPORTED).all() and not o["steps"].any() and np.isnan(o["residual_after"]).all()
    assert bits_equal(o["x"], r["x"]) and bits_equal(o["lam"], r["lam"]) and bits_equal(o["fval"], r["fval"])
    bm.close()


@pytest.mark.parametrize("name", ["reg21", "wg70", "wg130"])
def test_no_side_effects(gpu_lib, monkeypatch, name):
    """solve, backward, update(f) + warm solve: the same bits with a refine in between and without"""
    import daqp_amd
    fam, p = K.family(name), K.problems(name, "plain")
    set_env(monkeypatch, fam["env"], False)
    g = np.random.default_rng(11).standard_normal((p["N"], p["n"]))
    f2 = p["f"] + 0.05 * np.random.default_rng(12).standard_normal(p["f"].shape)
    runs = []
    for with_refine in (False, True):
        bm = daqp_amd.BatchModel(p["N"], p["n"], p["m"], p["ms"])
        bm.setup(p["H"], p["f"], p["A"], p["bupper"], p["blower"])
        r0 = bm.solve()
        if with_refine:
            assert (bm.refine(r0)["status"] == 0).all()
        bw = bm.backward(g, out="numpy")
        if with_refine:
            bm.refine(r0, max_steps=8)
        r1 = bm.solve()
        bm.update(f=f2)
        r2 = bm.solve()
        if with_refine:
            assert (bm.refine(r2)["status"] == 0).all()
        bw2 = bm.backward(g, out="numpy")
        runs.append([r0, bw, r1, r2, bw2])
        bm.close()
    for a, b in zip(*runs):
        assert a.keys() == b.keys()
        for key in a:
            assert bits_equal(a[key], b[key]), key


@pytest.mark.parametrize("i", [0, 3, 4], ids=["12", "80", "130"])
def test_host_and_device_memory_identical_bits(gpu_lib, monkeypatch, i):
    import torch
    set_env(monkeypatch, {}, False)
    p, t, bm = planted_batch(i, 3)
    rd = bm.solve(out="torch")
    rh = {k: v.cpu().numpy() for k, v in rd.items()}
    h1 = bm.refine(rh)
    d1 = bm.refine(rd)
    h2 = bm.refine(rh, out="numpy")
    for k in ("x", "lam", "fval", "status", "steps", "residual_before", "residual_after"):
        assert d1[k].is_cuda and isinstance(h1[k], np.ndarray)
        assert bits_equal(h1[k], d1[k].cpu().numpy()) and bits_equal(h1[k], h2[k]), k
    assert bits_equal(rd["x"].cpu().numpy(), rh["x"]) and not bits_equal(h1["x"], rh["x"])
    bm.close()
