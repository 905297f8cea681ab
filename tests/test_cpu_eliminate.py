"""Equality elimination without a GPU: the numpy reference of tests/eliminate_cases.py against the oracle on the full problem, the
golden eliminated problems replayed through it, and the C interface declared, exported and refusing loudly."""
import ctypes as C
import os

import numpy as np
import pytest

import eliminate_cases as EC
import kkt_reference as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_eliminated.npz")
ENTRIES = ("daqp_batch_eliminate", "daqp_batch_eliminate_update", "daqp_batch_elimination_problem", "daqp_batch_elimination_flags",
           "daqp_batch_expand", "daqp_batch_elimination_basis", "daqp_batch_elimination_read", "daqp_batch_elimination_bytes", "daqp_batch_elimination_free")


@pytest.fixture(scope="module")
def ora():
    return O.Oracle()


def osolve(ora, H, f, A, bupper, blower, sense, ms):
    """setup_daqp + daqp_solve on the oracle (its daqp_quadprog refuses problems the reference would eliminate first)"""
    ns = int(((np.asarray(sense) & 8) != 0).sum())
    om = ora.model(np.size(f), np.size(bupper), ms, ns)
    assert om.setup(H, f, A, bupper, blower, sense) >= 0
    return om.solve()


def reduce_solve_expand(ora, p, ms, eq_rows):
    """(x, lam, fval, flag) of problem p through the numpy elimination and the oracle on the reduced problem"""
    el = EC.eliminate(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms, eq_rows)
    r64 = {k: np.ascontiguousarray(el[k], dtype=np.float64) for k in ("H", "f", "A", "bupper", "blower")}
    y, lam_r, fval_r, flag, _ = osolve(ora, r64["H"], r64["f"], r64["A"], r64["bupper"], r64["blower"], el["sense"], 0)
    x, lam, fval = EC.expand(el, y, lam_r, fval_r)
    return x, lam, fval, flag, el


def close(x, lam, x_ref, lam_ref, kept):
    assert np.abs(x - x_ref).max() <= 1e-9, np.abs(x - x_ref).max()
    assert np.abs(lam - lam_ref).max() <= 1e-7 * max(1.0, np.abs(lam_ref).max()), np.abs(lam - lam_ref).max()
    act = lambda l: np.sign(np.where(np.abs(l) >= 1e-8, l, 0.0))[kept]
    assert np.array_equal(act(lam), act(lam_ref))      # the inequality active sets, side by side


@pytest.mark.parametrize("i", range(len(EC.SHAPES)), ids=[str(s) for s in EC.SHAPES])
def test_reference_agrees_with_the_oracle_on_the_full_problem(ora, i):
    shape = EC.SHAPES[i]
    n, neq, m, ms = shape
    b = EC.make_batch(shape, 2, 100 + i, bound_row=(i == 0), soft=(2 if i == 4 else 0))
    for k in range(2):
        p = {key: b[key][k] for key in ("H", "f", "A", "bupper", "blower", "sense")}
        x, lam, fval, flag, el = reduce_solve_expand(ora, p, ms, b["eq_rows"])
        xo, lo, fo, flago, _ = osolve(ora, p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms)
        assert flag == flago == 1
        close(x, lam, xo, lo, el["kept"])
        assert abs(fval - fo) <= 1e-9 * max(1.0, abs(fo))
        assert np.abs(xo - b["x"][k]).max() <= 1e-8 and (np.abs(lo[el["kept"]][b["lam"][k][el["kept"]] != 0]) >= 1e-8).all()      # the plant
        assert np.array_equal(el["H"], el["H"].T)
        c = R.certificate(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms, x, lam, 1e-6)
        assert c["stationarity"] <= 1e-9 and c["primal"] <= 1e-9 and c["complementarity"] <= 1e-9 and c["wrong_sign"] == 0, c


def test_golden_eliminated_problems_replay(ora):
    ps = EC.golden_problems(GOLDEN)
    assert len(ps) == 16
    for p in ps:
        assert 1 <= p["eq_rows"].size < p["f"].size
        x, lam, fval, flag, el = reduce_solve_expand(ora, p, p["ms"], p["eq_rows"])
        assert flag == int(p["exitflag"]) == 1, p["name"]
        close(x, lam, p["x"], p["lam"], el["kept"])
        assert abs(fval - float(p["fval"])) <= 1e-9 * max(1.0, abs(float(p["fval"]))), p["name"]


def test_entries_are_declared_exported_and_documented():
    import daqp_amd
    from daqp_amd import _lib
    with open(os.path.join(ROOT, "include", "daqp_amd.h")) as fh:
        header = fh.read()
    assert "typedef struct DAQPBatchElimination DAQPBatchElimination;" in header
    L = daqp_amd.lib()
    for e in ENTRIES:
        assert e + "(" in header and e in _lib.EXPORTS and hasattr(L, e), e
    for word in ("H_r = Z'HZ", "f_r = Z'(H x0 + f)", "A_r = C_I Z", "c0 = 1/2 x0'Hx0 + f'x0", "lam_E = -R^-1 Q1'(H x + f + C_I'lam_I)",
                 "DAQP_EXIT_OVERDETERMINED_INITIAL (-6)", "accepted and ignored", "no HIP device", "q_k = c_k Z H_r^-1 Z'c_k'", "ONLY this call has the workgroup tier"):
        assert word in header, word
    assert "eliminate_kernel.hip" in _lib.UNITS and "eliminate.hip.h" in _lib.UNITS["post_solve.hip"]
    assert callable(daqp_amd.EliminatedBatchModel) and "EliminatedBatchModel" in daqp_amd.__all__
    res = {k: v for k, v in _lib.kernel_resources().items() if k.startswith(("k_eliminate", "k_expand", "k_elim_basis"))}
    assert len(res) == 16, sorted(res)
    with open(os.path.join(ROOT, "daqp_amd", "api.py")) as fh:
        assert "libamdhip" not in fh.read()      # the binding reaches the device through the library's own entries only
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)


def test_every_entry_refuses_without_a_device():
    import daqp_amd
    from daqp_amd import _lib
    L = daqp_amd.lib()
    if L.daqp_amd_device_count() >= 1:
        return      # a HIP device is present: tests/test_gpu_eliminate.py holds the argument errors
    b = EC.make_batch(EC.SHAPES[0], 2, 1, bound_row=True)
    n, neq, m, ms = EC.SHAPES[0]
    p = _lib.DAQPBatchProblem(2, n, m, ms, *[b[k].ctypes.data for k in ("H", "f", "A", "bupper", "blower", "sense")], _lib.MEM_HOST)
    h = C.c_void_p()
    fake = C.c_void_p(8)      # never dereferenced: the device check comes first
    rp, rr = _lib.DAQPBatchProblem(), _lib.DAQPBatchResult()
    fl = np.zeros(2, np.int32)
    calls = [lambda: L.daqp_batch_eliminate(C.byref(h), C.byref(p), b["eq_rows"].ctypes.data_as(_lib.c_int_p), neq, None, -1, None),
             lambda: L.daqp_batch_eliminate_update(fake, b["f"].ctypes.data, None, None, _lib.MEM_HOST),
             lambda: L.daqp_batch_elimination_problem(fake, C.byref(rp)),
             lambda: L.daqp_batch_elimination_flags(fake, fl.ctypes.data_as(_lib.c_int_p)),
             lambda: L.daqp_batch_expand(fake, C.byref(rr), C.byref(rr)),
             lambda: L.daqp_batch_elimination_basis(fake, None, None, None, _lib.MEM_HOST),
             lambda: L.daqp_batch_elimination_read(fake, None, None, None, None, None, None, _lib.MEM_HOST)]
    for call in calls:
        L.daqp_amd_device_count()
        assert call() == -8
        assert "no HIP device" in _lib.last_error()
    assert not h.value
    assert L.daqp_batch_elimination_bytes(None) == 0
    L.daqp_batch_elimination_free(None)
    with pytest.raises(RuntimeError, match="no HIP device"):
        daqp_amd.EliminatedBatchModel(2, n, m, ms, b["eq_rows"])
