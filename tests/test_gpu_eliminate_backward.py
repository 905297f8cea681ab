"""The adjoint of an eliminated batch on the device (daqp_batch_eliminate_backward, EliminatedBatchModel.backward,
qp_layer(eq_rows=...)) against the dense solve of the full KKT system (tests/eliminate_adjoint_cases.py), against the adjoint of the
unreduced BatchModel on the same problems, and the layer against finite differences.

The bar is that of tests/test_gpu_backward.py: 1e-9 relative to the max norm of the solution [dz; dnu]."""
import ctypes as C
import functools

import numpy as np
import pytest

import eliminate_adjoint_cases as AC
import eliminate_cases as EC

pytestmark = pytest.mark.gpu

TOL = 1e-9
KEYS = ("H", "f", "A", "bupper", "blower", "sense")
# (shape, bound_row); the last has n > 256: eight entries per lane
CASES = [((6, 2, 10, 2), True), ((64, 63, 70, 4), False), ((65, 1, 70, 0), False), ((130, 70, 150, 0), False), ((257, 200, 270, 0), False)]
IDS = [str(c[0]) for c in CASES]
GRADS = ("g_x", "g_lam", "both")
N = 3


@functools.lru_cache(maxsize=None)
def batch(i, lp=False):
    shape, bound_row = (EC.LP_SHAPE, False) if lp else CASES[i]
    b = EC.make_batch(shape, N, 800 + i, lp=lp, bound_row=bound_row)
    rng = np.random.default_rng(810 + i)
    b["gx"], b["gl"] = rng.standard_normal(b["f"].shape), rng.standard_normal(b["bupper"].shape)
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


def eliminated(b, ns=0, solve=True):
    import daqp_amd
    n, neq, m, ms = b["shape"]
    em = daqp_amd.EliminatedBatchModel(b["f"].shape[0], n, m, ms, b["eq_rows"], ns_max=ns)
    em.setup(*[b[k] for k in KEYS])
    if solve:
        em.solve()
    return em


def planted_working_set(em, b):
    """the reduced working set is the planted one: the active kept rows of every problem"""
    na, ws = em.reduced.working_sets()
    for k in range(b["f"].shape[0]):
        _, act = AC.working_set(b["lam"][k], b["eq_rows"])
        assert np.array_equal(np.sort(em.kept_rows[ws[k, :na[k]]]), act), (k, ws[k, :na[k]], act)


@functools.lru_cache(maxsize=None)
def solved(i, lp=False):
    b = batch(i, lp)
    em = eliminated(b)
    assert (em.flags == 1).all()
    planted_working_set(em, b)
    return b, em


def pick(which, b):
    return (b["gx"] if which != "g_lam" else None), (b["gl"] if which != "g_x" else None)


@functools.lru_cache(maxsize=None)
def reference(i, which, lp=False):
    """[dz; dnu] of the dense solve, per problem: computed once"""
    b = batch(i, lp)
    n, neq, m, ms = b["shape"]
    gx, gl = pick(which, b)
    out = []
    for k in range(N):
        p = AC.problem(b, k)
        W, _ = AC.working_set(p["lam"], b["eq_rows"])
        dz, dnu = AC.dense(p["H"], EC.cmat(p["A"], ms, n), W, None if gx is None else gx[k], None if gl is None else gl[k])
        out.append((dz.astype(np.float64), dnu.astype(np.float64)))
    return out


def against_reference(b, o, ref, label):
    m = b["shape"][2]
    eq = b["eq_rows"]
    worst = 0.0
    for k in range(N):
        assert o["status"][k] == 0, (k, o["status"][k])
        dz, dnu = ref[k]
        scale = max(np.abs(dz).max(), np.abs(dnu).max())
        got = o["dbupper"][k] + o["dblower"][k]
        err = max(np.abs(o["dz"][k] - dz).max(), np.abs(got - dnu).max()) / scale
        worst = max(worst, err)
        lam = b["lam"][k]
        W, act = AC.working_set(lam, eq)
        off = np.setdiff1d(np.arange(m), W)
        assert not o["dbupper"][k][off].any() and not o["dblower"][k][off].any(), k
        # sides: a kept row of W carries its dnu where it sits; an equality row carries it in dbupper
        assert not o["dblower"][k][eq].any(), k
        assert not o["dbupper"][k][act[lam[act] < 0]].any() and not o["dblower"][k][act[lam[act] > 0]].any(), k
    print(label, "worst relative error %.2e" % worst)
    assert worst <= TOL, (label, worst)


# ---- 1: against the dense reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", GRADS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_the_dense_reference(gpu_lib, i, which):
    """Worst relative error of [dz; dnu] over {g_x, g_lam, both}, measured on an MI355X (the bar is 1e-9): (6, 2, 10, 2) 1.8e-14,
    (64, 63, 70, 4) 8.9e-15, (65, 1, 70, 0) 1.4e-14, (130, 70, 150, 0) 7.1e-15, (257, 200, 270, 0) 4.1e-15."""
    b, em = solved(i)
    gx, gl = pick(which, b)
    o = em.backward(gx, grad_lam=gl)
    assert all(isinstance(v, np.ndarray) for v in o.values())
    against_reference(b, o, reference(i, which), (b["shape"], which))


# ---- 2: against the unreduced model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_the_unreduced_model(gpu_lib, i):
    import daqp_amd
    b, em = solved(i)
    n, neq, m, ms = b["shape"]
    eq = b["eq_rows"]
    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(*[b[k] for k in KEYS])
    r = bm.solve()
    assert (r["exitflag"] == 1).all()
    want = bm.backward(b["gx"], out="numpy", grad_lam=b["gl"])
    bm.close()
    o = em.backward(b["gx"], grad_lam=b["gl"])
    assert not want["status"].any() and not o["status"].any()
    for k in range(N):
        wnu = want["dbupper"][k] + want["dblower"][k]
        scale = max(np.abs(want["dz"][k]).max(), np.abs(wnu).max())
        ez = np.abs(o["dz"][k] - want["dz"][k]).max() / scale
        ee = np.abs((o["dbupper"][k] + o["dblower"][k])[eq] - wnu[eq]).max() / scale
        print(b["shape"], k, "dz %.2e dnu_E %.2e" % (ez, ee))
        assert ez <= TOL and ee <= TOL, (k, ez, ee)


# ---- 3: an LP batch ------------------------------------------------------------------------------------------------------------------
def test_lp_vertex_needs_the_null_space_route(gpu_lib):
    b, em = solved(0, lp=True)
    for which in GRADS:
        gx, gl = pick(which, b)
        against_reference(b, em.backward(gx, grad_lam=gl, nullspace=True), reference(0, which, lp=True), (b["shape"], "lp", which))
    o = em.backward(b["gx"], grad_lam=b["gl"])
    assert (o["status"] == -8).all()
    assert not o["dz"].any() and not o["dbupper"].any() and not o["dblower"].any()


# ---- 4: bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_host_and_device_memory_give_identical_bits(gpu_lib, i):
    import torch
    b, em = solved(i)
    for which in GRADS:
        gx, gl = pick(which, b)
        host = em.backward(gx, grad_lam=gl)
        t = lambda a: None if a is None else torch.tensor(a, device="cuda")
        dev = em.backward(t(gx), grad_lam=t(gl))
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values())
        for key in host:
            assert np.array_equal(host[key].view(np.int64 if host[key].dtype == np.float64 else np.int32),
                                  dev[key].cpu().numpy().view(np.int64 if host[key].dtype == np.float64 else np.int32)), (which, key)
    none = em.backward(b["gx"])
    zeros = em.backward(b["gx"], grad_lam=np.zeros_like(b["gl"]))
    for key in none:
        assert np.array_equal(none[key], zeros[key]), key


def test_intermediates_are_counted_from_the_first_call(gpu_lib):
    b = batch(0)
    n, neq, m, ms = b["shape"]
    em = eliminated(b)
    before = gpu_lib.daqp_batch_elimination_bytes(em._el)
    em.backward(b["gx"], grad_lam=b["gl"])
    first = gpu_lib.daqp_batch_elimination_bytes(em._el)
    em.backward(b["gx"])
    assert gpu_lib.daqp_batch_elimination_bytes(em._el) == first
    # grad_y, dz_r (N nr), grad_lam_r, dbupper_r, dblower_r (N mr), dz0 (N n) doubles and status_r (N) ints
    assert first - before == 8 * N * (2 * (n - neq) + 3 * (m - neq) + n) + 4 * N
    em.close()


# ---- 5: flags and isolation -------------------------------------------------------------------------------------------------------------
def test_flagged_problems_return_their_flag_and_zeros(gpu_lib):
    shape = EC.SHAPES[4]
    n, neq, m, ms = shape
    b = EC.make_batch(shape, 4, 830)
    eq = b["eq_rows"]
    rng = np.random.default_rng(831)
    gx, gl = rng.standard_normal((4, n)), rng.standard_normal((4, m))
    bad = {k: b[k].copy() for k in KEYS}
    bad["A"][1, eq[3] - ms] = bad["A"][1, eq[1] - ms]      # a duplicated equality row
    bad["bupper"][1, eq[3]] = bad["blower"][1, eq[3]] = bad["bupper"][1, eq[1]]
    bad["bupper"][2, eq[5]] += 0.5                          # no equality
    em = eliminated(dict(b, **bad))
    assert np.array_equal(em.flags, [1, -6, -8, 1])
    o = em.backward(gx, grad_lam=gl)
    em.close()
    assert np.array_equal(o["status"], [0, -6, -8, 0])
    for q in (1, 2):
        assert not o["dz"][q].any() and not o["dbupper"][q].any() and not o["dblower"][q].any()
    good = eliminated(b)
    og = good.backward(gx, grad_lam=gl)
    good.close()
    for key in og:
        assert np.array_equal(o[key][[0, 3]], og[key][[0, 3]]), key
    assert np.abs(og["dz"]).max() > 0


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu_lib):
    import torch
    import daqp_amd
    from daqp_amd import _lib
    b = batch(0)
    n, neq, m, ms = b["shape"]
    nr, mr = n - neq, m - neq
    dd = dict(dtype=torch.float64, device="cuda")
    gx, gl = torch.randn(N, n, **dd), torch.randn(N, m, **dd)
    dz, dbu, dbl = torch.full((N, n), 7.0, **dd), torch.full((N, m), 7.0, **dd), torch.full((N, m), 7.0, **dd)
    st = torch.full((N,), 7, dtype=torch.int32, device="cuda")

    def raw(el, red, which=-1, null=()):
        args = [el, red] + [t.data_ptr() for t in (gx, gl, dz, dbu, dbl, st)]
        for j in null:
            args[j] = None
        return gpu_lib.daqp_batch_eliminate_backward(*args, which, _lib.MEM_DEVICE)

    def refused(words, el, red, **kw):
        rc = raw(el, red, **kw)
        err = daqp_amd.last_error()
        assert rc != 0 and "daqp_batch_eliminate_backward" in err and words in err, (rc, err, words)
        torch.cuda.synchronize()
        assert all(bool((a == 7).all()) for a in (dz, dbu, dbl, st)), words

    em = eliminated(b, solve=False)
    el, red = em._el, em.reduced._h
    refused("successful daqp_batch_solve", el, red)                         # set up, not solved
    with pytest.raises(RuntimeError, match="successful daqp_batch_solve"):
        em.backward(gx, grad_lam=gl)
    em.solve()
    refused("null", el, red, null=(0,))                                      # the handle
    refused("null", el, red, null=(1,))                                      # the batch
    for j in (4, 5, 6, 7):
        refused("null", el, red, null=(j,))                                  # an output
    refused("both null", el, red, null=(2, 3))
    for which in (-2, 2):
        refused("which", el, red, which=which)
    other = daqp_amd.BatchModel(N, nr + 1, mr, 0)
    refused("shape", el, other._h)
    other.close()
    other = daqp_amd.BatchModel(N, nr, mr, 1)
    refused("shape", el, other._h)                                           # ms != 0
    other.close()
    side = torch.cuda.Stream()
    other = daqp_amd.BatchModel(N, nr, mr, 0)
    gpu_lib.daqp_batch_set_stream(other._h, C.c_void_p(side.cuda_stream))
    refused("stream", el, other._h)
    other.close()
    if torch.cuda.device_count() > 1:
        other = daqp_amd.BatchModel(N, nr, mr, 0, device=1)
        refused("device", el, other._h)
        other.close()
    em.update(f=b["f"] * 1.01)
    refused("successful daqp_batch_solve", el, red)                         # update, no solve
    em.solve()
    em.reset()
    refused("successful daqp_batch_solve", el, red, which=0)                # reset, no solve
    em.solve()
    assert raw(el, red) == 0                                                 # and now it runs
    torch.cuda.synchronize()
    assert (st == 0).all() and not (dz == 7).any()
    dz.fill_(7.0), dbu.fill_(7.0), dbl.fill_(7.0), st.fill_(7)
    em.close()
    soft = eliminated(b, ns=1)
    refused("ns_max > 0", soft._el, soft.reduced._h)
    with pytest.raises(RuntimeError, match="ns_max > 0"):
        soft.backward(gx, grad_lam=gl)
    soft.close()
    # which == 1 beyond one wavefront in the reduced space
    wide = eliminated(EC.make_batch((130, 2, 150, 0), 2, 840), solve=False)
    with pytest.raises(RuntimeError, match="nr <= 64"):
        wide.backward(np.zeros((2, 130)), nullspace="all")
    wide.close()


# ---- 7: the layer --------------------------------------------------------------------------------------------------------------------------
def layer_inputs(Nq=2):
    import torch
    shape, bound_row = CASES[0]
    b = EC.make_batch(shape, Nq, 850, bound_row=bound_row)
    t = lambda a, grad=True: torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=grad)
    eq = [int(r) for r in b["eq_rows"]]
    return b, eq, dict(S=t(np.zeros_like(b["H"])), f=t(b["f"]), A=t(b["A"]), bu=t(b["bupper"]), bl=t(b["blower"]), e=t(b["bupper"][:, eq]))


def layer_call(b, eq, S, f, A, bu, bl, e, **kw):
    """H moves symmetrically, and the equality right-hand side is ONE tensor feeding both bounds"""
    import torch
    import daqp_amd
    H = torch.tensor(b["H"], dtype=torch.float64, device="cuda") + 0.5 * (S + S.transpose(-1, -2))
    bu, bl = bu.clone(), bl.clone()
    bu[:, eq] = e
    bl[:, eq] = e
    return daqp_amd.qp_layer(H, f, A, bu, bl, ms=b["shape"][3], eq_rows=eq, **kw)


def test_layer_gradcheck(gpu_lib):
    import torch
    b, eq, t = layer_inputs()
    n, neq, m, ms = b["shape"]
    rng = np.random.default_rng(851)
    w = [torch.tensor(rng.standard_normal(s), dtype=torch.float64, device="cuda") for s in ((2, n), (2, m), (2,))]
    info = {}
    with torch.no_grad():
        x, lam, fval = layer_call(b, eq, *t.values(), info=info, returns=("x", "lam", "fval"))
    assert (info["exitflag"] == 1).all()
    # the base problem is the planted one (multipliers and slacks of at least 0.1): a step of 1e-6 keeps the active set
    assert np.abs(x.cpu().numpy() - b["x"]).max() <= 1e-9 and np.abs(lam.cpu().numpy() - b["lam"]).max() <= 1e-7
    assert np.array_equal(lam.cpu().numpy() != 0, b["lam"] != 0)

    def fn(*args):
        out = layer_call(b, eq, *args, returns=("x", "lam", "fval"))
        return sum((o * wk).sum() for o, wk in zip(out, w))

    assert torch.autograd.gradcheck(fn, tuple(t.values()), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_layer_bound_gradients_of_equality_rows_go_to_bupper(gpu_lib):
    import torch
    import daqp_amd
    b, eq, _ = layer_inputs()
    t = {k: torch.tensor(b[k], dtype=torch.float64, device="cuda", requires_grad=True) for k in ("H", "f", "A", "bupper", "blower")}
    info = {}
    x, lam, fval = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=b["shape"][3], eq_rows=eq, info=info,
                                     returns=("x", "lam", "fval"))
    (x.sum() + lam.sum() + fval.sum()).backward()
    assert not info["status"].any()
    assert not t["blower"].grad[:, eq].any() and t["bupper"].grad[:, eq].abs().min() > 0
    # "x" alone, the default: the same layer with one output
    x1 = daqp_amd.qp_layer(t["H"].detach(), t["f"].detach(), t["A"].detach(), t["bupper"].detach(), t["blower"].detach(), ms=b["shape"][3], eq_rows=eq)
    assert isinstance(x1, torch.Tensor) and torch.equal(x1, x.detach())


def test_layer_without_eq_rows_is_what_it_was(gpu_lib):
    import torch
    import daqp_amd
    b, eq, _ = layer_inputs()
    n, neq, m, ms = b["shape"]
    g = torch.tensor(np.random.default_rng(852).standard_normal((2, n)), device="cuda")
    t = {k: torch.tensor(b[k], dtype=torch.float64, device="cuda", requires_grad=True) for k in ("H", "f", "A", "bupper", "blower")}
    x = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=ms, eq_rows=None)
    x.backward(g)
    bm = daqp_amd.BatchModel(2, n, m, ms)
    bm.setup(*[t[k].detach() for k in ("H", "f", "A", "bupper", "blower")], init_mask=daqp_amd.UPDATE_unconstrained)
    r = bm.solve(out="torch")
    o = bm.backward(g)
    torch.cuda.synchronize()
    assert torch.equal(x.detach(), r["x"])
    assert torch.equal(t["f"].grad, -o["dz"]) and torch.equal(t["bupper"].grad, o["dbupper"]) and torch.equal(t["blower"].grad, o["dblower"])
    xr, rr = r["x"], r["lam"]
    assert torch.equal(t["H"].grad, -0.5 * (o["dz"][:, :, None] * xr[:, None, :] + xr[:, :, None] * o["dz"][:, None, :]))
    assert torch.equal(t["A"].grad, -(rr[:, ms:, None] * o["dz"][:, None, :] + (o["dbupper"] + o["dblower"])[:, ms:, None] * xr[:, None, :]))
    bm.close()


def test_layer_refuses_a_shared_plant_and_soft_rows(gpu_lib):
    import torch
    import daqp_amd
    b, eq, _ = layer_inputs()
    n, neq, m, ms = b["shape"]
    t = {k: torch.tensor(b[k], dtype=torch.float64, device="cuda") for k in ("H", "f", "A", "bupper", "blower")}
    with pytest.raises(ValueError, match="shared"):
        daqp_amd.qp_layer(t["H"][0], t["f"], t["A"][0], t["bupper"], t["blower"], ms=ms, eq_rows=eq)
    with pytest.raises(ValueError, match="shared"):
        daqp_amd.qp_layer(t["H"], t["f"], t["A"][0], t["bupper"], t["blower"], ms=ms, eq_rows=eq)
    sense = torch.zeros(m, dtype=torch.int32)
    sense[m - 1] = 8
    with pytest.raises(ValueError, match="SOFT"):
        daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=ms, eq_rows=eq, sense=sense)
