"""daqp_batch_refine_nullspace / BatchModel.refine(nullspace=...) on the GPU: refinement of the problems that went through the proximal
loop -- singular H, LPs -- by the null-space method on the caller's own H (daqp_amd/csrc/refine_nullspace.hip.h).

Planted exact cases (tests/refine_nullspace_cases.py: integer data, the exact optimum known): after solve + refine(nullspace=True)
    E_after <= max(8 E_model, 2^-46)
with E_model from the numpy model of refine_nullspace_cases run from the same start (never from the kernel); the factor 8 and the floor
are those of tests/test_gpu_refine.py: the GPU sums in another order than the model.  From zeros the loop ends, by its own rule, after
the first step that reaches mu <= 2^-50, which leaves E ~ cond(K) 2^-52: E_model is then the model's own run from zeros.
Random families of tests/backward_nullspace_cases.py: the status is that of backward(nullspace=True), mu does not grow, x moves by the
proximal tolerance's order at the most.  Singular systems, refusals, no side effects, host and device memory."""
import ctypes as C

import numpy as np
import pytest

import backward_nullspace_cases as B
import refine_cases as RC
import refine_nullspace_cases as NC
import test_gpu_refine as TR
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FLOOR = TR.FLOOR
UNSUPPORTED, SINGULAR = -8, -20
KEYS = ("x", "lam", "fval", "status", "steps", "residual_before", "residual_after")
bits_equal = TR.bits_equal


def planted_batch(p, N):
    """N copies of a planted problem as device tensors, and a model set up on them"""
    import torch
    import daqp_amd
    t = {k: torch.from_numpy(np.array(np.broadcast_to(p[k], (N,) + p[k].shape))).cuda() for k in ("H", "f", "A", "bupper", "blower") if p[k] is not None}
    bm = daqp_amd.BatchModel(N, p["n"], p["m"], p["ms"])
    bm.setup(t.get("H"), t["f"], t["A"], t["bupper"], t["blower"])
    return t, bm


def errors(p, o, err=NC.error):
    return np.array([err(p, x, lam) for x, lam in zip(np.asarray(o["x"]), np.asarray(o["lam"]))])


def check_refined(p, bm, r, o, N, bar, err=NC.error):
    """status 0, E below the bar, mu not larger, lam off W zero, the certificate no worse, fval the certificate's objective"""
    e1 = errors(p, o, err)
    assert (o["status"] == 0).all(), o["status"]
    assert (e1 <= bar).all(), (e1.max(), bar)
    assert (o["residual_after"] <= o["residual_before"]).all() and (o["steps"] <= 8).all()
    off = np.setdiff1d(np.arange(p["m"]), p["W"])
    assert not o["lam"][:, off].any()
    c1 = bm.certify(o, out="numpy")
    Hn = np.broadcast_to(NC.dense(p)["H"], (N, p["n"], p["n"]))
    fn = np.broadcast_to(p["f"], (N, p["n"]))
    assert (np.abs(o["fval"] - c1["objective"]) <= TR.fval_tol(Hn, fn, o["x"], o["fval"], c1["objective"])).all()
    return e1, c1


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("i", NC.PROXIMAL, ids=[NC.label(i) for i in NC.PROXIMAL])
def test_planted_cases_reach_the_last_bits(gpu_lib, monkeypatch, i, exact):
    TR.set_env(monkeypatch, {}, exact)
    p, N = NC.case(i), (67, 3, 1)[i % 3]
    t, bm = planted_batch(p, N)
    r = bm.solve(out="numpy")
    assert (r["exitflag"] == 1).all() and (bm.prox_info()["n_prox"] > 0).all()
    x_in, lam_in = r["x"].copy(), r["lam"].copy()
    # daqp_batch_refine itself still hands these back
    plain = bm.refine(r)
    assert (plain["status"] == UNSUPPORTED).all() and not plain["steps"].any() and np.isnan(plain["residual_after"]).all()
    assert bits_equal(plain["x"], r["x"]) and bits_equal(plain["lam"], r["lam"]) and bits_equal(plain["fval"], r["fval"])
    o = bm.refine(r, nullspace=True)
    bar = max(8.0 * NC.model_error(i), FLOOR)
    e0 = errors(p, r)
    e1, c1 = check_refined(p, bm, r, o, N, bar)
    print(NC.label(i), "N", N, "E before %.2e after %.2e bar %.2e" % (e0.max(), e1.max(), bar), "steps", o["steps"].min(), "..", o["steps"].max(),
          "mu %.2e -> %.2e" % (o["residual_before"].max(), o["residual_after"].max()))
    assert (o["steps"] <= 3).all()
    assert bits_equal(r["x"], x_in) and bits_equal(r["lam"], lam_in)
    c0 = bm.certify(r, out="numpy")
    assert (TR.ratio(c1) <= TR.ratio(c0)).all(), (TR.ratio(c0), TR.ratio(c1))
    bm.close()


@pytest.mark.parametrize("i", range(len(NC.CASES)), ids=[NC.label(i) for i in range(len(NC.CASES))])
def test_from_zeros_the_kernel_solves_the_system(gpu_lib, monkeypatch, i):
    TR.set_env(monkeypatch, {}, False)
    p = NC.case(i)
    t, bm = planted_batch(p, 3)
    r = bm.solve(out="numpy")
    assert (r["exitflag"] == 1).all()
    z = dict(x=np.zeros_like(r["x"]), lam=np.zeros_like(r["lam"]))
    o = bm.refine(z, max_steps=8, nullspace=True if i in NC.PROXIMAL else "all")
    bar = max(8.0 * NC.model_error(i, zeros=True), FLOOR)
    e1, _ = check_refined(p, bm, r, o, 3, bar)
    print(NC.label(i), "E %.2e bar %.2e" % (e1.max(), bar), "steps", o["steps"], "mu %.2e -> %.2e" % (o["residual_before"].max(), o["residual_after"].max()))
    assert (o["steps"] >= 1).all() and not z["x"].any()
    bm.close()


@pytest.mark.parametrize("i", NC.DEFINITE, ids=[str(RC.CASES[i]["shape"][0]) for i in NC.DEFINITE])
def test_from_zeros_on_the_definite_cases(gpu_lib, monkeypatch, i):
    TR.set_env(monkeypatch, {}, False)
    p, t, bm = TR.planted_batch(i, 3)
    r = bm.solve(out="numpy")
    z = dict(x=np.zeros_like(r["x"]), lam=np.zeros_like(r["lam"]))
    o = bm.refine(z, max_steps=8, nullspace="all")
    bar = max(8.0 * NC.definite_model_error(i, zeros=True), FLOOR)
    e1, _ = check_refined(p, bm, r, o, 3, bar, RC.error)
    print(p["n"], "E %.2e bar %.2e" % (e1.max(), bar), "steps", o["steps"], "mu %.2e -> %.2e" % (o["residual_before"].max(), o["residual_after"].max()))
    bm.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
@pytest.mark.parametrize("i", NC.DEFINITE, ids=[str(RC.CASES[i]["shape"][0]) for i in NC.DEFINITE])
def test_all_is_a_second_algorithm_on_the_definite_planted_cases(gpu_lib, monkeypatch, i, exact):
    TR.set_env(monkeypatch, {}, exact)
    N = (67, 3, 1)[i % 3]
    p, t, bm = TR.planted_batch(i, N)
    r = bm.solve(out="numpy")
    assert (r["exitflag"] == 1).all() and not bm.prox_info()["n_prox"].any()
    o = bm.refine(r, nullspace="all")
    bar = max(8.0 * RC.model_error(i), FLOOR)      # the bar of bm.refine(r) in tests/test_gpu_refine.py
    e1, _ = check_refined(p, bm, r, o, N, bar, RC.error)
    gram = bm.refine(r)
    print(p["n"], "N", N, "E before %.2e null-space %.2e Gram %.2e bar %.2e" % (TR.errors(p, r).max(), e1.max(), TR.errors(p, gram).max(), bar), "steps", o["steps"].max())
    assert np.array_equal(o["status"], bm.backward(np.zeros((N, p["n"])), out="numpy", nullspace="all")["status"])
    # no proximal problem: which = 0 is daqp_batch_refine
    same = bm.refine(r, nullspace=True)
    for key in KEYS:
        assert bits_equal(same[key], gram[key]), key
    bm.close()


def _mixed_batch():
    """the mix of tests/test_gpu_backward_nullspace.py -- n = 16: even problems positive definite (n_prox == 0 under the automatic
    shift), odd ones dense PSD of rank 10"""
    n, m, ms, N = 16, 40, 4, 12
    qs = []
    for k in range(N):
        if k % 2 == 0:
            p = O.generate_qp(n, m, ms, 6, rng=[770, k])
            qs.append({key: p[key] for key in B.KEYS + ("H",)})
        else:
            qs.append(O.generate_singular_qp(n, m, ms, 10, [771, k]))
    return (n, m, ms, N), {key: np.stack([p[key] for p in qs]) for key in B.KEYS + ("H",)}


def test_mixed_batch_keeps_the_other_problems_bit_for_bit(gpu_lib, monkeypatch):
    import daqp_amd
    TR.set_env(monkeypatch, {}, False)
    (n, m, ms, N), q = _mixed_batch()
    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    r = bm.solve()
    assert (r["exitflag"] == 1).all()
    prox = bm.prox_info()["n_prox"] > 0
    assert np.array_equal(prox, np.arange(N) % 2 == 1)
    o0 = bm.refine(r)
    o1 = bm.refine(r, nullspace=True)
    bm.close()
    assert (o0["status"][prox] == UNSUPPORTED).all() and not o0["status"][~prox].any() and not o1["status"].any()
    for key in KEYS:
        assert bits_equal(o0[key][~prox], o1[key][~prox]), key
    print("mixed batch, proximal problems: mu %.2e -> %.2e" % (o1["residual_before"][prox].max(), o1["residual_after"][prox].max()), "steps", o1["steps"][prox])
    assert (o1["residual_after"][prox] < o1["residual_before"][prox]).all() and (o1["steps"][prox] >= 1).all()


def _model(name):
    """the case's batch of tests/backward_nullspace_cases.py, set up and solved; (model, solve results)"""
    import daqp_amd
    c = B.CASES[name]
    n, m, ms = c["shape"]
    q = B.batch(name)
    bm = daqp_amd.BatchModel(q["f"].shape[0], n, m, ms, **c.get("settings", {}))
    args = [q[k] for k in ("H", "f", "A", "bupper", "blower", "sense")]
    if c.get("shared", False):
        bm.setup_shared(*args)
    else:
        bm.setup(*args)
    return bm, bm.solve()


@pytest.mark.parametrize("name", list(B.CASES))
def test_random_families(gpu_lib, monkeypatch, name):
    TR.set_env(monkeypatch, {}, False)
    bm, r = _model(name)
    N, n = r["x"].shape
    assert (bm.prox_info()["n_prox"] > 0).all(), name
    o = bm.refine(r, nullspace=True)
    bw = bm.backward(np.zeros((N, n)), out="numpy", nullspace=True)
    bm.close()
    assert np.array_equal(o["status"], bw["status"]) and not o["status"].any(), (name, o["status"], bw["status"])
    assert (o["residual_after"] <= o["residual_before"]).all(), name
    moved = (np.abs(o["x"] - r["x"]) / np.maximum(1.0, np.abs(r["x"]))).max()
    print(f"family {B.CASES[name]['family']} ({B.FAMILIES[B.CASES[name]['family']]}), {name}: mu {o['residual_before'].max():.2e} -> "
          f"{o['residual_after'].max():.2e}, steps {o['steps'].min()}..{o['steps'].max()}, |dx| / max(1, |x|) {moved:.2e}")
    assert moved <= 1e-6, (name, moved)


def _marked(r):
    """not the solve's own outputs: nothing may be restored from the batch"""
    return dict(x=r["x"] + 0.125, lam=r["lam"] - 0.25, fval=r["fval"] + 3.0)


def _came_back_unchanged(o, marked, which):
    assert (o["status"][which] == SINGULAR).all(), o["status"]
    for key in ("x", "lam", "fval"):
        assert bits_equal(o[key][which], marked[key][which]), key
    assert not o["steps"][which].any() and np.isnan(o["residual_before"][which]).all() and np.isnan(o["residual_after"][which]).all()


def _give(marked, memory):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in marked.items()} if memory == "device" else marked


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("kind", ["lp_off_a_vertex", "semidefinite_on_the_null_space"])
def test_not_locally_unique_is_singular_and_comes_back_unchanged(gpu_lib, monkeypatch, kind, memory):
    """-1 <= x <= 1 in two variables.  LP with f = (1, 0): x_1 = -1 and x_2 is free along an edge, k = 1 < n.  H = diag(1, 0) with
    f = (2, 0): W = {x_1 lower}, Z = e_2 and Z'HZ = 0."""
    import daqp_amd
    TR.set_env(monkeypatch, {}, False)
    N = 3
    lp = kind == "lp_off_a_vertex"
    H = None if lp else np.tile(np.diag([1.0, 0.0]), (N, 1, 1))
    f = np.tile([1.0 if lp else 2.0, 0.0], (N, 1))
    bm = daqp_amd.BatchModel(N, 2, 2, 2)
    bm.setup(H, f, np.zeros((N, 0, 2)), np.ones((N, 2)), -np.ones((N, 2)))
    r = bm.solve()
    na, ws = bm.working_sets()
    assert (r["exitflag"] == 1).all() and (na == 1).all() and (ws[:, 0] == 0).all() and np.allclose(r["x"][:, 0], -1.0)
    marked = _marked(r)
    for mode in (True, "all"):
        o = bm.refine(_give(marked, memory), max_steps=8, out="numpy", nullspace=mode)
        _came_back_unchanged(o, marked, np.ones(N, bool))
        assert np.array_equal(o["status"], bm.backward(np.ones((N, 2)), out="numpy", nullspace=mode)["status"])
    bm.close()


@pytest.mark.parametrize("memory", ["host", "device"])
def test_dependent_active_rows_are_singular_and_come_back_unchanged(gpu_lib, monkeypatch, memory):
    """the nearly parallel equality rows of tests/test_gpu_refine.py: R_jj^2 ~ eps^2 = 1e-9 is below zero_tol = 1e-7"""
    import daqp_amd
    TR.set_env(monkeypatch, {}, False)
    q = TR.near_dependent()
    N, n = q["f"].shape
    m = q["bupper"].shape[1]
    bm = daqp_amd.BatchModel(N, n, m, 0, zero_tol=1e-7)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    r = bm.solve()
    na, ws = bm.working_sets()
    both = np.array([0 in ws[k, :na[k]] and 1 in ws[k, :na[k]] for k in range(N)])
    assert (r["exitflag"] == 1).all() and both.any()
    marked = _marked(r)
    o = bm.refine(_give(marked, memory), max_steps=8, out="numpy", nullspace="all")
    _came_back_unchanged(o, marked, both)
    assert not o["status"][~both].any()
    assert np.array_equal(o["status"], bm.backward(np.zeros((N, n)), out="numpy", nullspace="all")["status"])
    if (~both).any():
        assert (o["residual_after"][~both] <= o["residual_before"][~both]).all()
    bm.close()


def _raw(L, bm, x, lam, st, max_steps=3, which=0, null=None):
    args = [C.c_void_p(t.data_ptr()) for t in (x, lam)] + [None, None, None, C.c_void_p(st.data_ptr())]
    if null is not None:
        args[null] = None
    return L.daqp_batch_refine_nullspace(bm._h, *args, max_steps, which, 1)


def test_refusals_launch_nothing(gpu_lib, monkeypatch):
    import torch
    import daqp_amd
    TR.set_env(monkeypatch, {}, False)
    name = "psd_n16"
    n, m, ms = B.CASES[name]["shape"]
    q = B.batch(name)
    N = q["f"].shape[0]
    dd = dict(dtype=torch.float64, device="cuda")
    x, lam = torch.full((N, n), 7.0, **dd), torch.full((N, m), 7.0, **dd)
    st = torch.full((N,), 7, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((x == 7).all() and (lam == 7).all() and (st == 7).all())

    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    assert _raw(gpu_lib, bm, x, lam, st) != 0 and "daqp_batch_solve" in daqp_amd.last_error()          # before the solve
    r = bm.solve()
    for null in (0, 1, 5):
        assert _raw(gpu_lib, bm, x, lam, st, null=null) != 0                                            # a NULL x, lam or status
    for steps in (0, 9):
        assert _raw(gpu_lib, bm, x, lam, st, max_steps=steps) != 0 and "max_steps" in daqp_amd.last_error()
        with pytest.raises(RuntimeError, match="max_steps"):
            bm.refine(r, max_steps=steps, nullspace=True)
    assert _raw(gpu_lib, bm, x, lam, st, which=2) != 0 and "which" in daqp_amd.last_error()
    with pytest.raises(ValueError):
        bm.refine(r, nullspace="yes")
    bm.update(f=q["f"] * 1.01)
    assert _raw(gpu_lib, bm, x, lam, st) != 0 and "daqp_batch_solve" in daqp_amd.last_error()          # update, no solve
    with pytest.raises(RuntimeError, match="successful daqp_batch_solve"):
        bm.refine(r, nullspace=True)
    assert untouched()
    r = bm.solve()
    x.copy_(torch.from_numpy(r["x"])), lam.copy_(torch.from_numpy(r["lam"]))
    assert _raw(gpu_lib, bm, x, lam, st) == 0                                                           # and now it runs
    torch.cuda.synchronize()
    assert (st != 7).all()
    bm.close()
    x.fill_(7.0), lam.fill_(7.0), st.fill_(7)
    soft = daqp_amd.BatchModel(N, n, m, ms, ns_max=2)
    soft.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"], q["sense"])
    soft.solve()
    assert _raw(gpu_lib, soft, x, lam, st) != 0 and "soft" in daqp_amd.last_error()                    # ns_max > 0
    assert untouched()
    soft.close()


def test_beyond_one_wavefront(gpu_lib, monkeypatch):
    """n = 70, singular H: which = 1 is refused; which = 0 leaves the proximal problems at -8 and is daqp_batch_refine for the rest"""
    import torch
    import daqp_amd
    TR.set_env(monkeypatch, {}, False)
    n, m, ms, N = 70, 140, 0, 4
    qs = [O.generate_singular_qp(n, m, ms, 35, [790, k]) for k in range(N)]
    b = {key: np.stack([p[key] for p in qs]) for key in B.KEYS + ("H",)}
    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(b["H"], b["f"], b["A"], b["bupper"], b["blower"], b["sense"])
    r = bm.solve()
    assert (r["exitflag"] == 1).all() and (bm.prox_info()["n_prox"] > 0).all()
    o, plain = bm.refine(r, nullspace=True), bm.refine(r)
    assert (o["status"] == UNSUPPORTED).all()
    for key in KEYS:
        assert bits_equal(o[key], plain[key]), key
    assert bits_equal(o["x"], r["x"]) and bits_equal(o["lam"], r["lam"])
    x, lam = torch.full((N, n), 7.0, dtype=torch.float64, device="cuda"), torch.full((N, m), 7.0, dtype=torch.float64, device="cuda")
    st = torch.full((N,), 7, dtype=torch.int32, device="cuda")
    assert _raw(gpu_lib, bm, x, lam, st, which=1) != 0 and "n <= 64" in daqp_amd.last_error()
    with pytest.raises(RuntimeError, match="n <= 64"):
        bm.refine(r, nullspace="all")
    torch.cuda.synchronize()
    assert (x == 7).all() and (lam == 7).all() and (st == 7).all()
    bm.close()
    # a definite batch of that size: no proximal problem, which = 0 is daqp_batch_refine
    q = O.generate_batch(N, n, m, ms, 20, 791)
    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
    r = bm.solve()
    o, plain = bm.refine(r, nullspace=True), bm.refine(r)
    assert not plain["status"].any()
    for key in KEYS:
        assert bits_equal(o[key], plain[key]), key
    bm.close()


def test_no_side_effects(gpu_lib, monkeypatch):
    """solve, backward(nullspace=True), update(f) + warm solve: the same bits with a refine(nullspace=True) in between and without"""
    TR.set_env(monkeypatch, {}, False)
    name = "psd_n16"
    q = B.batch(name)
    N, n = q["f"].shape
    g = B.grad(N, n)
    f2 = q["f"] + 0.01 * np.random.default_rng(12).standard_normal(q["f"].shape)
    runs = []
    for with_refine in (False, True):
        bm, r0 = _model(name)
        if with_refine:
            assert not bm.refine(r0, nullspace=True)["status"].any()
        bw = bm.backward(g, out="numpy", nullspace=True)
        if with_refine:
            bm.refine(r0, max_steps=8, nullspace="all")
        bm.update(f=f2)
        r1 = bm.solve()
        if with_refine:
            bm.refine(r1, nullspace=True)
        bw1 = bm.backward(g, out="numpy", nullspace=True)
        runs.append([r0, bw, r1, bw1])
        bm.close()
    for a, b in zip(*runs):
        assert a.keys() == b.keys()
        for key in a:
            assert bits_equal(a[key], b[key]), key


@pytest.mark.parametrize("i", [4, 8, 13], ids=[NC.label(i) for i in (4, 8, 13)])
def test_host_and_device_memory_identical_bits(gpu_lib, monkeypatch, i):
    TR.set_env(monkeypatch, {}, False)
    t, bm = planted_batch(NC.case(i), 3)
    rd = bm.solve(out="torch")
    rh = {k: v.cpu().numpy() for k, v in rd.items()}
    h1 = bm.refine(rh, nullspace=True)
    d1 = bm.refine(rd, nullspace=True)
    h2 = bm.refine(rh, out="numpy", nullspace="all")
    for k in KEYS:
        assert d1[k].is_cuda and isinstance(h1[k], np.ndarray)
        assert bits_equal(h1[k], d1[k].cpu().numpy()) and bits_equal(h1[k], h2[k]), k
    assert bits_equal(rd["x"].cpu().numpy(), rh["x"]) and not bits_equal(h1["x"], rh["x"])
    bm.close()
