"""Redundancy removal on the GPU (daqp_minrep / daqp_minrep_batch) against the reference's verdicts in tests/golden/golden_minrep.npz
(tests/golden/make_golden_minrep.py: every polyhedron's margins are clear of the tolerance, so the comparison is exact), and the
workspace reset (daqp_deactivate_constraints / reset_daqp_workspace / daqp_batch_reset)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# (n, m, ms): smallest shape | one row block | one row past it | simple bounds | three row blocks | the image kernel's shape |
# image-only, cap 65 | the workgroup kernel
SHAPES = [(3, 12, 0), (8, 64, 0), (8, 65, 0), (6, 40, 6), (12, 130, 0), (50, 150, 0), (64, 256, 0), (80, 200, 0)]


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "golden_minrep.npz"))
    out = {}
    for n, m, ms in SHAPES:
        key = f"{n}_{m}_{ms}"
        out[(n, m, ms)] = (z["A_" + key].astype(np.float64), z["b_" + key].astype(np.float64), z["red_" + key].astype(np.int32))
    return out


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("shape", SHAPES)
def test_minrep_c_abi_equals_reference(gpu_lib, golden, shape):
    """daqp_minrep (the reference's signature) on every polyhedron of the fixture: exactly the reference's verdicts"""
    n, m, ms = shape
    A, b, red = golden[shape]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    for p in range(A.shape[0]):
        Ap, bp = np.ascontiguousarray(A[p]), np.ascontiguousarray(b[p])
        out = np.full(m, -7, np.int32)
        gpu_lib.daqp_minrep(out.ctypes.data_as(ip), Ap.ctypes.data_as(dp), bp.ctypes.data_as(dp), n, m, ms)
        assert np.array_equal(out, red[p]), (shape, p, np.flatnonzero(out != red[p]))


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_minrep_batch_equals_reference(gpu_lib, golden, shape, resident):
    """minrep_batch on the stacked fixture, host inputs and device-resident inputs; every test ends OPTIMAL or INFEASIBLE"""
    import daqp_amd
    import torch
    A, b, red = golden[shape]
    info = {}
    if resident:
        out = daqp_amd.minrep_batch(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), ms=shape[2], out="torch", info=info)
        assert out.is_cuda and out.dtype == torch.int32
        out = out.cpu().numpy()
    else:
        out = daqp_amd.minrep_batch(A, b, ms=shape[2], info=info)
    assert out.shape == red.shape and out.dtype == np.int32
    assert np.array_equal(out, red), (shape, np.argwhere(out != red))
    assert info["unresolved"] == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_minrep_modes_agree(gpu_lib, golden, shape, monkeypatch):
    """the reference's arithmetic (DAQP_AMD_EXACT=1) and the default arithmetic give the same verdicts; (50, 150) also through the
    fp32-image kernel at two waves per SIMD (forced: a batch of 600 tests would not get it)"""
    import daqp_amd
    A, b, red = golden[shape]
    monkeypatch.setenv("DAQP_AMD_EXACT", "1")
    exact = daqp_amd.minrep_batch(A, b, ms=shape[2])
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    fast = daqp_amd.minrep_batch(A, b, ms=shape[2])
    assert np.array_equal(exact, fast) and np.array_equal(exact, red)
    if shape == (50, 150, 0):
        monkeypatch.setenv("DAQP_AMD_IMG_MIN_BATCH", "1")
        img = daqp_amd.minrep_batch(A, b, ms=0)
        assert np.array_equal(img, red)


def test_minrep_python_call_shape(gpu_lib, golden):
    """minrep(A, b) as the reference's binding has it: ms = len(b) - A.shape[0]"""
    import daqp_amd
    A, b, red = golden[(6, 40, 6)]
    out = daqp_amd.minrep(A[0], b[0])
    assert out.dtype == np.int32 and np.array_equal(out, red[0])


def test_minrep_unbounded_direction(gpu_lib):
    """x <= 1, x <= 2, y <= 1: the reference answers [0, 1, 0]"""
    import daqp_amd
    A = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    b = np.array([1.0, 2.0, 1.0])
    assert daqp_amd.minrep(A, b).tolist() == [0, 1, 0]


def test_minrep_empty_polyhedron_all_ones(gpu_lib):
    """x <= -1, -x <= -1, y <= 1, -y <= 1 is empty: every face is empty, all ones (the documented convention)"""
    import daqp_amd
    A = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    b = np.array([-1.0, -1.0, 1.0, 1.0])
    assert daqp_amd.minrep(A, b).tolist() == [1, 1, 1, 1]


def test_minrep_zero_row(gpu_lib):
    """a vanishing row of A is not tested (-1); the other rows get the verdicts they have without it"""
    import daqp_amd
    A = np.array([[1.0, 0.0], [0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    b = np.array([1.0, 5.0, 2.0, 1.0, 1.0, 1.0])
    assert daqp_amd.minrep(A, b).tolist() == [0, -1, 1, 0, 0, 0]


def _qp(seed=3):
    n, m, ms, na = 10, 30, 0, 5
    q = O.generate_qp(n, m, ms, na, rng=[77, seed])
    rng = np.random.default_rng([78, seed])
    f2 = q["f"] + 0.02 * rng.standard_normal(n)
    return q, f2


@pytest.mark.parametrize("exact", [True, False])
def test_workspace_reset_reproduces_cold_solve(gpu_lib, monkeypatch, exact):
    """setup, cold solve, update f, warm solve (fewer iterations); then daqp_deactivate_constraints + reset_daqp_workspace +
    daqp_solve gives, bit for bit, what a workspace gives that goes setup -> update f -> solve without ever having solved: the cold
    solve of the updated problem"""
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "1" if exact else "0")
    q, f2 = _qp()
    cold = daqp_amd.Model()
    assert cold.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])[0] > 0
    assert cold.update(f=f2) == 0
    xc, fc, flagc, ic = cold.solve()
    assert flagc == 1 and ic["iterations"] > 2

    mdl = daqp_amd.Model()
    assert mdl.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])[0] > 0
    x0, _, flag0, i0 = mdl.solve()
    assert flag0 == 1
    assert mdl.update(f=f2) == 0
    xw, _, flagw, iw = mdl.solve()
    assert flagw == 1 and iw["iterations"] < ic["iterations"]          # the warm start matters ...
    L = gpu_lib
    L.daqp_deactivate_constraints(mdl._ws)
    L.reset_daqp_workspace(mdl._ws)
    n_active = C.c_int.from_buffer(mdl._ws, O._WS_NACTIVE_OFF).value
    assert n_active == 0                                               # (host mirror)
    xr, fr, flagr, ir = mdl.solve()
    assert flagr == 1 and ir["iterations"] == ic["iterations"]         # ... and the reset takes it away
    assert bits_equal(xr, xc) and bits_equal(ir["lam"], ic["lam"]) and fr == fc
    assert np.abs(xw - xc).max() < 1e-9


@pytest.mark.parametrize("exact", [True, False])
def test_batch_reset_reproduces_cold_solve(gpu_lib, monkeypatch, exact):
    """the same for BatchModel.reset(), with empty working sets right after it"""
    import daqp_amd
    monkeypatch.setenv("DAQP_AMD_EXACT", "1" if exact else "0")
    N = 6
    qs = [_qp(seed) for seed in range(N)]
    st = lambda k: np.stack([q[k] for q, _ in qs])      # noqa: E731
    f2 = np.stack([f for _, f in qs])
    n, m = f2.shape[1], qs[0][0]["bupper"].size
    cold = daqp_amd.BatchModel(N, n, m)
    cold.setup(st("H"), st("f"), st("A"), st("bupper"), st("blower"))
    cold.update(f=f2)
    rc = cold.solve()
    mdl = daqp_amd.BatchModel(N, n, m)
    mdl.setup(st("H"), st("f"), st("A"), st("bupper"), st("blower"))
    mdl.solve()
    mdl.update(f=f2)
    rw = mdl.solve()
    assert (rw["exitflag"] == 1).all() and (rw["iter"] < rc["iter"]).all()
    assert (mdl.working_sets()[0] > 0).all()
    mdl.reset()
    na, ws = mdl.working_sets()
    assert (na == 0).all() and (ws == -1).all()
    rr = mdl.solve()
    assert np.array_equal(rr["exitflag"], rc["exitflag"]) and np.array_equal(rr["iter"], rc["iter"])
    assert bits_equal(rr["x"], rc["x"]) and bits_equal(rr["lam"], rc["lam"])
    cold.close(), mdl.close()
