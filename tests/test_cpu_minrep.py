"""daqp_minrep / workspace reset: what can be checked without a GPU -- the exported symbols, the behaviour without a device, and
(where the reference build exists) that the committed fixture is what its generator writes."""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_minrep_symbols_exported():
    import daqp_amd
    from daqp_amd import _lib
    L = daqp_amd.lib()
    for name in ("daqp_minrep", "daqp_minrep_batch", "daqp_batch_reset", "reset_daqp_workspace", "daqp_deactivate_constraints"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name), name
    assert callable(daqp_amd.minrep) and callable(daqp_amd.minrep_batch)
    assert hasattr(daqp_amd.Model, "reset") and hasattr(daqp_amd.BatchModel, "reset")
    with open(os.path.join(ROOT, "include", "daqp_amd.h")) as fh:
        header = fh.read()
    for name in ("daqp_minrep_batch", "daqp_batch_reset", "reset_daqp_workspace", "daqp_deactivate_constraints"):
        assert name + "(" in header, name


def test_minrep_without_device_fills_minus_one():
    """no HIP device: is_redundant is filled with -1 and daqp_amd_last_error() names the reason (there is no CPU path)"""
    import daqp_amd
    L = daqp_amd.lib()
    if L.daqp_amd_device_count() > 0:
        pytest.skip("a HIP device is visible: the no-device path cannot be reached here")
    A = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    b = np.array([1.0, 2.0, 1.0])
    out = np.full(3, 7, np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.daqp_minrep(out.ctypes.data_as(ip), A.ctypes.data_as(dp), b.ctypes.data_as(dp), 2, 3, 0)
    assert out.tolist() == [-1, -1, -1]
    assert "no HIP device" in daqp_amd.last_error()
    with pytest.raises(RuntimeError, match="no HIP device"):
        daqp_amd.minrep_batch(A[None], b[None])


def test_minrep_fixture_reproducible():
    """three entries of golden_minrep.npz regenerated against the reference build, where it exists"""
    from oracle import oracle as O
    if not O.reference_available(strict=True):
        pytest.skip("oracle/_ref is not built here (reference sources not present)")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_minrep", os.path.join(HERE, "golden", "make_golden_minrep.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    z = np.load(os.path.join(HERE, "golden", "golden_minrep.npz"))
    ref = G.RefMinrep()
    for (n, m, ms), k in (((3, 12, 0), 0), ((6, 40, 6), 3), ((50, 150, 0), 1)):
        A, b, red, _ = G.entry(ref, n, m, ms, k)
        key = f"{n}_{m}_{ms}"
        assert np.array_equal(A, z["A_" + key][k].astype(np.float64)) and np.array_equal(b, z["b_" + key][k].astype(np.float64))
        assert np.array_equal(red, z["red_" + key][k].astype(np.int32))
