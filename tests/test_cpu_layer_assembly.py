"""daqp_amd.layer.assemble_gradients -- the one place where qp_layer turns an adjoint solution into (dH, df, dA, dbupper, dblower, drho) --
on the CPU, against the numpy gradients of tests/backward_soft_dual_cases.py (which tests/test_cpu_backward_soft_dual.py holds to central
differences in np.longdouble).  No library, no GPU: the adjoint solution comes from that file's dense solve and is laid out as the
kernels lay it out -- dbupper / dblower by side, qsoft (N, m), usoft (N, ns, n) and usoft_id (N, ns) in working-set order with -1 in
the unused slot.

Problems: N = 6, n = 4, m = 6, ms = 2, a planted working set W = (1, 3, 5) held at (upper, lower, upper) -- x and lam_W are drawn (|lam|
in 0.5 .. 1.5 with the sign of the side), f and the bounds follow from the KKT conditions, and the file's forward() recovers x, lam.
`soft`: row 1 (a simple bound) and row 3 (a general row) are SOFT, ns_max = 3; `plain`: no SOFT row, the dict has no soft keys.

Tolerance.  Both sides evaluate the same formulas in float64 from the same adjoint solution and differ in association only.  Measured
here, as |got - want|_inf / max(1, |want|_inf) per array, worst over every test of this file: 4.4e-16.  The bound is 100 times that,
4.4e-14 -- far below the 1e-9 of the GPU layer tests, as it must be if rounding is all that differs."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from daqp_amd.layer import assemble_gradients

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("backward_soft_dual_cases_for_assembly", os.path.join(HERE, "backward_soft_dual_cases.py"))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

BOUND = 100 * 4.4e-16
N, n, m, ms, NS = 6, 4, 6, 2, 3
W, UPPER = np.array([1, 3, 5]), np.array([True, False, True])
RHO = D.RHO
BAD, BAD_STATUS = 2, -20      # the problem without a derivative of the status tests
KEYS = ("H", "f", "A", "bupper", "blower", "rho")
worst_seen = [0.0]


def _case(soft):
    """dict of the batch, its x and lam (from forward()) and the weights a (N, n), b (N, m), c (N,), d (N,) of the linear loss"""
    rng = np.random.default_rng(5 if soft else 6)
    L = np.tril(rng.standard_normal((N, n, n))) / np.sqrt(n)
    H = L @ np.swapaxes(L, 1, 2) + np.eye(n)
    A = rng.standard_normal((N, m - ms, n))
    Cm = np.concatenate([np.broadcast_to(np.eye(n)[:ms], (N, ms, n)), A], axis=1)
    is_soft = np.array([1.0, 1.0, 0.0]) if soft else np.zeros(3)
    x0 = rng.standard_normal((N, n))
    lam0 = (0.5 + rng.random((N, 3))) * np.where(UPPER, 1.0, -1.0)
    CW = Cm[:, W, :]
    _, qk, _ = D.kkt(H, CW, is_soft, RHO)
    f = -(np.einsum("qij,qj->qi", H, x0) + np.einsum("qki,qk->qi", CW, lam0))
    bW = np.einsum("qki,qi->qk", CW, x0) - RHO * qk * is_soft * lam0
    cx = np.einsum("qki,qi->qk", Cm, x0)
    bupper, blower = cx + 1.0, cx - 1.0
    bupper[:, W[UPPER]], blower[:, W[~UPPER]] = bW[:, UPPER], bW[:, ~UPPER]
    x, lamW, fval, slack = D.forward(H, Cm, W, UPPER, is_soft, RHO, f, bupper, blower)
    assert np.abs(x - x0).max() < 1e-12 and np.abs(lamW - lam0).max() < 1e-12      # the planted optimum, sides included
    lam = np.zeros((N, m))
    lam[:, W] = lamW
    a, b, c, d = rng.standard_normal((N, n)), rng.standard_normal((N, m)), rng.standard_normal(N), rng.standard_normal(N)
    return dict(H=H, C=Cm, is_soft=is_soft, soft=soft, x=x, lam=lam, lamW=lamW, a=a, b=b, c=c, d=d)


CASES = {}


def case(name):
    if name not in CASES:
        CASES[name] = _case(name == "soft")
    return CASES[name]


def _reference(q, a, b, c, d, upper=UPPER, bad=()):
    """the numpy gradients per problem, stacked (zero for the problems in `bad`), and the adjoint solution as the kernels lay it out"""
    ref = {k: [] for k in KEYS}
    o = dict(dz=np.zeros((N, n)), dbupper=np.zeros((N, m)), dblower=np.zeros((N, m)))
    if q["soft"]:
        o.update(qsoft=np.zeros((N, m)), usoft=np.zeros((N, NS, n)), usoft_id=np.full((N, NS), -1, np.int32))
    for k in range(N):
        g = D.gradients(q["H"][k], q["C"][k], ms, W, upper, q["is_soft"], RHO, q["x"][k], q["lamW"][k], a[k], b[k], c[k], d[k])
        for key in KEYS:
            ref[key].append(np.zeros_like(np.asarray(g[key])) if k in bad else np.asarray(g[key]))
        if k in bad:      # (the kernels leave zeros, and -1 in usoft_id)
            continue
        dz, dnuW, qk, U = D.dense_adjoint_dual(q["H"][k], q["C"][k], W, q["is_soft"], RHO, q["lamW"][k], a[k], b[k][W], d[k])
        o["dz"][k] = dz
        o["dbupper"][k, W[upper]], o["dblower"][k, W[~upper]] = dnuW[upper], dnuW[~upper]
        if q["soft"]:
            slots = np.nonzero(q["is_soft"])[0]
            o["qsoft"][k, W[slots]] = qk[slots]
            o["usoft"][k, :len(slots)], o["usoft_id"][k, :len(slots)] = U[slots], W[slots]
    return {key: np.stack(v) for key, v in ref.items()}, {key: torch.from_numpy(v) for key, v in o.items()}


def _compare(got, ref, shared, keys=KEYS, nonzero=KEYS):
    for key, g in zip(KEYS, got):
        if key not in keys:
            continue
        want = ref[key].sum(0) if key == "rho" or (shared and key in ("H", "A")) else ref[key]
        assert g.dtype == torch.float64 and tuple(g.shape) == want.shape, key
        err = np.abs(g.numpy() - want).max() / max(1.0, np.abs(want).max())
        worst_seen[0] = max(worst_seen[0], err)
        print(f"dl/d{key}: {err:.2e} (worst of this run so far: {worst_seen[0]:.2e})")
        if key in nonzero:
            assert np.abs(want).max() > 0, key
        assert err <= BOUND, (key, err)


LOSSES = ("g_x", "g_lam", "g_fval", "g_slack", "all")


def _weights(q, loss):
    a, b, c, d = q["a"], q["b"], q["c"], q["d"]
    z = lambda v: np.zeros_like(v)
    return dict(g_x=(a, z(b), z(c), z(d)), g_lam=(z(a), b, z(c), z(d)), g_fval=(z(a), z(b), c, z(d)), g_slack=(z(a), z(b), z(c), d),
                all=(a, b, c, d))[loss]


def _call(q, o, status, c, d, loss, shared, need=(True,) * 6, eq=None):
    t = torch.from_numpy
    g_fval = t(c) if loss in ("g_fval", "all") else None
    g_slack = t(d) if loss in ("g_slack", "all") and q["soft"] else None
    return assemble_gradients(t(q["x"]), t(q["lam"]), ms, o, status, need, shared=shared, g_fval=g_fval, g_slack=g_slack, rho=RHO, eq=eq)


@pytest.mark.parametrize("shared", [False, True], ids=["per_problem", "shared"])
@pytest.mark.parametrize("loss", LOSSES)
def test_soft_batch_equals_the_numpy_gradients(loss, shared):
    q = case("soft")
    a, b, c, d = _weights(q, loss)
    ref, o = _reference(q, a, b, c, d)
    assert (o["usoft_id"][:, -1] == -1).all() and (o["usoft_id"][:, :2] >= 0).all()      # one padded slot
    got = _call(q, o, torch.zeros(N, dtype=torch.int32), c, d, loss, shared)
    _compare(got, ref, shared)


@pytest.mark.parametrize("shared", [False, True], ids=["per_problem", "shared"])
@pytest.mark.parametrize("loss", ["g_x", "g_lam", "g_fval", "all"])
def test_plain_batch_equals_the_numpy_gradients(loss, shared):
    """no SOFT row: the dict has no soft keys, no q_k-dependence term exists and drho is None"""
    q = case("plain")
    a, b, c, d = _weights(q, loss)
    ref, o = _reference(q, a, b, c, d)
    got = _call(q, o, torch.zeros(N, dtype=torch.int32), c, d, loss, shared)
    assert got[5] is None and not ref["rho"].any()
    _compare(got[:5], ref, shared)


@pytest.mark.parametrize("shared", [False, True], ids=["per_problem", "shared"])
@pytest.mark.parametrize("name", ["soft", "plain"])
def test_a_problem_without_a_derivative_contributes_exact_zeros(name, shared):
    """status != 0: the launch left zeros for that problem; its g_fval and g_slack, which are not zero, must be masked in every term"""
    q = case(name)
    a, b, c, d = _weights(q, "all")
    ref, o = _reference(q, a, b, c, d, bad=(BAD,))
    status = torch.zeros(N, dtype=torch.int32)
    status[BAD] = BAD_STATUS
    assert c[BAD] != 0 and d[BAD] != 0 and q["lam"][BAD].any()
    got = _call(q, o, status, c, d, "all", shared)
    for key, g in zip(KEYS, got):
        if g is not None and g.dim() > 0 and g.shape[0] == N and not (shared and key in ("H", "A")):
            assert not g[BAD].any(), key      # exact zeros, not small numbers
    _compare(got if q["soft"] else got[:5], ref, shared)
    # exact also inside the batch sums: whatever x and lam that problem has, not a bit of any result moves
    loud = dict(q, x=q["x"].copy(), lam=q["lam"].copy())
    loud["x"][BAD] *= 1e6
    loud["lam"][BAD] *= -1e6
    for g, h in zip(got, _call(loud, o, status, c, d, "all", shared)):
        assert (g is None and h is None) or torch.equal(g, h)


@pytest.mark.parametrize("loss", ["g_x", "g_lam", "g_fval", "all"])
def test_an_equality_row_sends_every_bound_term_to_bupper(loss):
    """eq = (3,): row 3 is held at its lower side (lam < 0); as an equality row of an eliminated batch its multiplier gradient comes
    back in dbupper, and the -g_fval lam term must follow it there -- the reference is gradients() with that row counted as upper"""
    q = case("plain")
    assert (q["lam"][:, 3] < 0).all()
    a, b, c, d = _weights(q, loss)
    as_upper = np.array([True, True, True])
    ref, o = _reference(q, a, b, c, d, upper=as_upper)
    got = _call(q, o, torch.zeros(N, dtype=torch.int32), c, d, loss, False, eq=torch.tensor([3]))
    assert not got[4].any() and not ref["blower"].any()      # W has no other lower row: blower gets exact zeros
    _compare(got[:5], ref, False, nonzero=("H", "f", "A", "bupper"))
    if loss != "g_x" and loss != "g_lam":      # without eq the envelope term of that row goes to blower
        plain = _call(q, o, torch.zeros(N, dtype=torch.int32), c, d, loss, False)
        assert plain[4][:, 3].abs().min() > 0 and torch.equal(plain[3][:, 3] + plain[4][:, 3], got[3][:, 3])


@pytest.mark.parametrize("shared", [False, True], ids=["per_problem", "shared"])
def test_nothing_launched_leaves_the_envelope_terms(shared):
    """o = None with g_fval only: what qp_layer does when fval alone carries a gradient"""
    q = case("plain")
    a, b, c, d = _weights(q, "g_fval")
    ref, _ = _reference(q, a, b, c, d)
    got = _call(q, None, torch.zeros(N, dtype=torch.int32), c, d, "g_fval", shared)
    assert got[5] is None
    _compare(got[:5], ref, shared)
    status = torch.zeros(N, dtype=torch.int32)
    status[BAD] = -1      # (nothing launched: an exit flag other than 1 is the status)
    ref0, _ = _reference(q, a, b, c, d, bad=(BAD,))
    masked = _call(q, None, status, c, d, "g_fval", shared)
    _compare(masked[:5], ref0, shared)
    assert all(not g[BAD].any() for g in masked[1:5])


def test_only_what_is_needed_is_formed():
    q = case("soft")
    a, b, c, d = _weights(q, "all")
    ref, o = _reference(q, a, b, c, d)
    status = torch.zeros(N, dtype=torch.int32)
    full = _call(q, o, status, c, d, "all", False)
    assert _call(q, o, status, c, d, "all", False, need=(False,) * 6) == (None,) * 6
    for i in range(6):
        one = _call(q, o, status, c, d, "all", False, need=tuple(j == i for j in range(6)))
        assert all((g is None) == (j != i) for j, g in enumerate(one)) and torch.equal(one[i], full[i]), KEYS[i]
