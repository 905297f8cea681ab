"""daqp_certify_batch on the GPU (daqp_amd/csrc/certify.hip.h): the constructed cases of tests/certify_cases.py against their exact
certificate within the accuracy contract of include/daqp_amd.h, the solver's own outputs against tests/kkt_reference.py, the forms
of the call (shared, LP, host / device, NULL outputs, sense=None, NaN), and its refusals.

NaN: x enters neither ray_residual, ray_scale nor ray_support (they are functions of lam, A and the bounds), so a NaN in x makes
the five outputs that depend on x NaN -- stationarity, stationarity_scale, primal, complementarity, objective -- and leaves the three
ray outputs of that problem as they are; every output of the neighbours keeps its bits."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import certify_cases as CC
import kkt_cases as K
import kkt_reference as R

pytestmark = pytest.mark.gpu
KEYS = CC.REAL_KEYS + CC.INT_KEYS
ARGS = ("H", "f", "A", "bupper", "blower", "x", "lam", "sense")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(o1, o2, keys=KEYS):
    for k in keys:
        assert np.array_equal(bits(o1[k]), bits(o2[k])), k


def certify(q, ms, **kw):
    import daqp_amd
    return daqp_amd.certify_batch(*[q[k] for k in ARGS], ms=ms, **kw)


def check_pool(shape, problems, refs, out, tag):
    for i, e in enumerate(refs):
        kind = problems[i]["kind"]
        for key in CC.REAL_KEYS:
            got = float(out[key][i])
            print(tag, i, kind, key, got, float(e[key][0]), "bound %.3e" % float(e[key][1]))
            assert CC.within(got, e[key]), (tag, i, kind, key, got, float(e[key][0]), float(e[key][1]))
        for key in CC.INT_KEYS:
            assert int(out[key][i]) == e[key], (tag, i, kind, key, int(out[key][i]), e[key])


@pytest.mark.parametrize("N", CC.BATCHES)
@pytest.mark.parametrize("shape", CC.SHAPES, ids=str)
def test_constructed_cases(gpu_lib, shape, N):
    """(a)-(d) of certify_cases at every shape: real outputs within the contract bound of the exact value, wrong_sign and primal_row
    equal.  N = 67: the pool repeated cyclically in one launch; N = 1, 3: the pool in launches of N."""
    pool = CC.pool(shape)
    problems, refs = [q for q, _ in pool], [e for _, e in pool]
    if N >= len(pool):
        out = certify(CC.stack(problems, N), shape[2])
        check_pool(shape, [problems[i % len(pool)] for i in range(N)], [refs[i % len(pool)] for i in range(N)], out, (shape, N))
        return
    for start in range(0, len(pool), N):
        sel = list(range(start, start + N))
        ps = [problems[i % len(pool)] for i in sel]
        out = certify(CC.stack(ps, N), shape[2])
        check_pool(shape, ps, [refs[i % len(pool)] for i in sel], out, (shape, N, start))


# ------------------------------------------------------------------------------------------------------------------------------
# solver outputs
LD = Fraction(1, 2 ** 64)
SOLVED = [f["name"] for f in K.FAMILIES if f["shape"][0] <= 64] + ["wg70"]      # every family at n <= 64, and one workgroup shape
ENV_KEYS = sorted({k for f in K.FAMILIES for k in f["env"]})


def tolerance(value, K_, S):
    """the contract bound plus the longdouble reference's own rounding, (K + 2) 2^-64 S"""
    return float(CC.contract_bound(Fraction(value), K_, Fraction(S)) + (K_ + 2) * LD * Fraction(S))


def compare_with_kkt_reference(tag, p, k, x, lam, cert, data=None):
    H, f, A, bu, bl, sense = K.problem(p, k)
    n, m, ms = p["n"], p["m"], p["ms"]
    c = R.certificate(H, f, A, bu, bl, sense, ms, x, lam, K.RHO_SOFT, normalised=False)
    Cm = np.abs(R.constraint_matrix(A, ms, n).astype(np.float64))
    S_col = float((0.0 if H is None else (np.abs(H) @ np.abs(x)).max()) + np.abs(f).max() + (Cm.T @ np.abs(lam)).max())
    S_row = float((Cm @ np.abs(x) + np.minimum(np.abs(bu), np.abs(bl))).max())
    Kst = n + 1 + (m - ms) + 1
    scale = float(cert["stationarity_scale"][k])
    got = float(cert["stationarity"][k]) / scale
    # numerator and denominator each carry their bound; the quotient of two values >= 1-scaled: twice the numerator's bound over the scale
    tol = 2.0 * tolerance(c["stationarity"] * scale, Kst, S_col) / scale + 2.0 ** -51 * c["stationarity"]
    print(tag, k, "stationarity", got, c["stationarity"], tol)
    assert abs(got - c["stationarity"]) <= tol, (tag, k, got, c["stationarity"], tol)
    for key in ("primal", "complementarity"):
        tol = tolerance(c[key], n + 1, S_row)
        print(tag, k, key, float(cert[key][k]), c[key], tol)
        assert abs(float(cert[key][k]) - c[key]) <= tol, (tag, k, key, float(cert[key][k]), c[key], tol)
    assert int(cert["wrong_sign"][k]) == c["wrong_sign"], (tag, k)
    soft_active = sense is not None and bool((((sense & R.SOFT) != 0) & (lam != 0)).any())
    if not soft_active:
        S_obj = float(0.0 if H is None else np.abs(x) @ np.abs(H) @ np.abs(x) / 2) + float(np.abs(f) @ np.abs(x))
        tol = tolerance(c["fval_ref"], n * n + n, S_obj)
        assert abs(float(cert["objective"][k]) - c["fval_ref"]) <= tol, (tag, k, float(cert["objective"][k]), c["fval_ref"], tol)


@pytest.mark.parametrize("variant", K.VARIANTS)
@pytest.mark.parametrize("name", SOLVED)
def test_solver_outputs(gpu_lib, monkeypatch, name, variant):
    """bm.certify(res) on what BatchModel solves (each family under the environment that selects its kernel), against
    kkt_reference.certificate(normalised=False) on the same (x, lam)"""
    import torch
    import daqp_amd
    p = K.problems(name, variant)
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for key, v in K.family(name)["env"].items():
        monkeypatch.setenv(key, v)
    dev = {k: (None if p[k] is None else torch.as_tensor(p[k]).cuda()) for k in ("H", "f", "A", "bupper", "blower", "sense")}
    bm = daqp_amd.BatchModel(p["N"], p["n"], p["m"], p["ms"], p["ns_max"])
    bm.setup(dev["H"], dev["f"], dev["A"], dev["bupper"], dev["blower"], dev["sense"])
    res = bm.solve()
    cert = bm.certify(res)
    bm.close()
    assert all(isinstance(cert[k], np.ndarray) and cert[k].shape == (p["N"],) for k in KEYS)
    for k in range(p["N"]):
        if res["exitflag"][k] in (1, 2):
            compare_with_kkt_reference((name, variant), p, k, res["x"][k], res["lam"][k], cert)


def test_infeasible_batch_ray_outputs(gpu_lib):
    """a batch with INFEASIBLE problems: the three ray outputs are the exact evaluation of whatever lam came back (nothing is claimed
    about that lam being a good ray; what it is gets printed)"""
    import torch
    import daqp_amd
    p = K.problems("reg21", "plain")
    N, n, m, ms = p["N"], p["n"], p["m"], p["ms"]
    A, bu, bl = p["A"].copy(), p["bupper"].copy(), p["blower"].copy()
    for k in range(0, N, 2):      # every other problem: two parallel general rows, a x <= b and a x >= b + 1
        A[k, 1] = A[k, 0]
        bl[k, ms + 1] = bu[k, ms] + 1.0
        bu[k, ms + 1] = bu[k, ms] + 2.0
    t = lambda a: torch.as_tensor(a).cuda()
    bm = daqp_amd.BatchModel(N, n, m, ms)
    bm.setup(t(p["H"]), t(p["f"]), t(A), t(bu), t(bl))
    res = bm.solve()
    cert = bm.certify(res)
    bm.close()
    assert (res["exitflag"][::2] == -1).all() and (res["exitflag"][1::2] == 1).all(), res["exitflag"]
    for k in range(N):
        e = CC.exact(p["H"][k], p["f"][k], A[k], bu[k], bl[k], None, ms, res["x"][k], res["lam"][k])
        for key in ("ray_residual", "ray_scale", "ray_support"):
            assert CC.within(cert[key][k], e[key]), (k, key, cert[key][k], float(e[key][0]))
        if res["exitflag"][k] == -1:
            print("infeasible", k, "ray_residual / ray_scale", cert["ray_residual"][k] / max(cert["ray_scale"][k], 1e-300), "ray_support", cert["ray_support"][k])


# ------------------------------------------------------------------------------------------------------------------------------
# forms
@pytest.fixture(scope="module")
def mixed():
    """per shape (one wave, one workgroup): the pool stacked, and its host-memory certificate"""
    out = {}
    for shape in ((7, 20, 3), (65, 80, 5)):
        q = CC.stack([p for p, _ in CC.pool(shape)], 11)
        out[shape] = (q, certify(q, shape[2]))
    return out


@pytest.mark.parametrize("shape", [(7, 20, 3), (65, 80, 5)], ids=str)
def test_forms(gpu_lib, mixed, shape):
    import torch
    import daqp_amd
    from daqp_amd import _lib
    q, host = mixed[shape]
    n, m, ms = shape
    N = q["f"].shape[0]
    # device memory == host memory, bit for bit; out='torch' gives device tensors
    d = {k: torch.as_tensor(q[k]).cuda() for k in ARGS}
    o = certify(d, ms, out="torch")
    assert all(o[k].is_cuda for k in KEYS)
    same_bits({k: o[k].cpu().numpy() for k in KEYS}, host)
    # shared H / A == the same data replicated
    rep = dict(q, H=np.repeat(q["H"][:1], N, 0), A=np.repeat(q["A"][:1], N, 0))
    same_bits(certify(dict(q, H=q["H"][0], A=q["A"][0]), ms), certify(rep, ms))
    sh = certify({k: (d[k][0] if k in ("H", "A") else d[k]) for k in ARGS}, ms)
    same_bits(sh, certify(rep, ms))
    # H = None == H = 0
    same_bits(certify(dict(q, H=None), ms), certify(dict(q, H=np.zeros_like(q["H"])), ms))
    # sense = None == zeros
    same_bits(certify(dict(q, sense=None), ms), certify(dict(q, sense=np.zeros_like(q["sense"])), ms))
    # NULL output pointers are skipped, the others unchanged
    L = daqp_amd.lib()
    prim, row = np.full(N, 7.0), np.full(N, 7, np.int32)
    cert = _lib.DAQPBatchCertificate(primal=prim.ctypes.data, primal_row=row.ctypes.data)
    p = _lib.DAQPBatchProblem(N, n, m, ms, *[q[k].ctypes.data for k in ("H", "f", "A", "bupper", "blower", "sense")], _lib.MEM_HOST)
    assert L.daqp_certify_batch(C.byref(cert), C.byref(p), q["x"].ctypes.data, q["lam"].ctypes.data, 0, -1, None) == 0
    same_bits(dict(primal=prim, primal_row=row), host, ("primal", "primal_row"))
    # a NaN in one problem's x
    x = q["x"].copy()
    x[4, n // 2] = np.nan
    o = certify(dict(q, x=x), ms)
    for k in ("stationarity", "stationarity_scale", "primal", "complementarity", "objective"):
        assert np.isnan(o[k][4]), k
    others = np.arange(N) != 4
    same_bits({k: o[k][others] for k in KEYS}, {k: host[k][others] for k in KEYS})
    same_bits({k: o[k][4:5] for k in KEYS}, {k: host[k][4:5] for k in KEYS}, ("ray_residual", "ray_scale", "ray_support"))


def test_refusals(gpu_lib):
    import daqp_amd
    from daqp_amd import _lib
    L = daqp_amd.lib()
    q = CC.stack([p for p, _ in CC.pool((7, 20, 3))], 2)
    out = np.zeros(2)
    cert = _lib.DAQPBatchCertificate(stationarity=out.ctypes.data)
    ptrs = [q[k].ctypes.data for k in ("H", "f", "A", "bupper", "blower", "sense")]
    good = _lib.DAQPBatchProblem(2, 7, 20, 3, *ptrs, _lib.MEM_HOST)
    x, lam = q["x"].ctypes.data, q["lam"].ctypes.data
    assert L.daqp_certify_batch(C.byref(cert), C.byref(good), x, lam, 0, -1, None) == 0
    for p, xx, word in ((good, None, "null"), (_lib.DAQPBatchProblem(2, 7, 20, 8, *ptrs, _lib.MEM_HOST), x, "ms=8"),
                        (_lib.DAQPBatchProblem(0, 7, 20, 3, *ptrs, _lib.MEM_HOST), x, "N=0")):
        assert L.daqp_certify_batch(C.byref(cert), C.byref(p), xx, lam, 0, -1, None) != 0
        assert word in _lib.last_error(), _lib.last_error()
    assert L.daqp_certify_batch(None, C.byref(good), x, lam, 0, -1, None) != 0
