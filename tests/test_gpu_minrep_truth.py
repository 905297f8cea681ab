"""daqp_minrep / daqp_minrep_batch against the TRUTH of constructed polyhedra (tests/minrep_cases.py: a witness on the face of every
row that must stay, a Farkas combination for every row that may go, both checked in np.longdouble by tests/test_cpu_minrep_truth.py)
instead of against recorded verdicts: margins from 1e-1 down to the tolerance, near-parallel core rows, row scales over four (and
eight) decades, negative right-hand sides, simple bounds on every kernel family.  A "redundant" verdict is the bare INFEASIBLE exit
of a solve kernel with no second pass behind it, so: at clear margins the verdicts ARE the truth; at near margins no row with a
witness may ever be dropped, and the reference's arithmetic (DAQP_AMD_EXACT=1) answers what the reference answered
(tests/golden/golden_minrep_truth.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

import minrep_cases as MC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# every shape once with the dispatch as it is, and the image-kernel shape once more with the fp32-image kernel forced (a batch of 300
# tests would not get it): simple bounds on that kernel
RUNS = [(shape, None) for shape in MC.SHAPES] + [((50, 150, 10), "1")]
RUN_IDS = [f"{s[0]}-{s[1]}-{s[2]}" + ("-img" if f else "") for s, f in RUNS]


def _env(monkeypatch, exact, img):
    monkeypatch.setenv("DAQP_AMD_EXACT", str(exact))
    if img is None:
        monkeypatch.delenv("DAQP_AMD_IMG_MIN_BATCH", raising=False)
    else:
        monkeypatch.setenv("DAQP_AMD_IMG_MIN_BATCH", img)


def _where(out, want):
    return [tuple(ix) + (int(out[tuple(ix)]), int(want[tuple(ix)])) for ix in np.argwhere(out != want)[:12]]


@pytest.fixture(scope="module")
def recorded():
    z = np.load(os.path.join(HERE, "golden", "golden_minrep_truth.npz"))
    return {k: z[k].astype(np.int32) for k in z.files}


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("delta", MC.CLEAR)
@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_clear_margins_give_the_truth(gpu_lib, monkeypatch, run, delta, exact):
    """(a) every redundant row clears its bound by delta >= 100 primal_tol of its norm, every core row has a witness: the verdicts
    equal the truth, and every row test ends OPTIMAL or INFEASIBLE"""
    import daqp_amd
    shape, img = run
    _env(monkeypatch, exact, img)
    A, b, truth = MC.stack(MC.cases(shape, delta))
    info = {}
    out = daqp_amd.minrep_batch(A, b, ms=shape[2], info=info)
    assert out.dtype == np.int32 and out.shape == truth.shape
    assert np.array_equal(out, truth), (shape, delta, exact, _where(out, truth))
    assert info["unresolved"] == 0


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("delta", MC.NEAR)
@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_near_margins_never_drop_a_core_row(gpu_lib, monkeypatch, recorded, run, delta, exact):
    """(b) margins of 1 to 30 primal_tol: a redundant row may be kept in the default arithmetic, a row with a witness is never
    dropped; in the reference's arithmetic the verdicts are the reference's, row for row"""
    import daqp_amd
    shape, img = run
    _env(monkeypatch, exact, img)
    A, b, truth = MC.stack(MC.cases(shape, delta))
    info = {}
    out = daqp_amd.minrep_batch(A, b, ms=shape[2], info=info)
    missed = int(((truth == 1) & (out != 1)).sum())
    print(f"{shape} delta {delta:g} exact {exact}: {missed} of {int((truth == 1).sum())} redundant rows kept, unresolved {info['unresolved']}")
    assert set(np.unique(out)) <= {0, 1}
    dropped = (truth == 0) & (out != 0)
    assert not dropped.any(), (shape, delta, exact, np.argwhere(dropped))
    if exact:
        want = recorded["red_" + MC.fixture_key(shape, delta)]
        assert np.array_equal(out, want), (shape, delta, _where(out, want))


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("shape", MC.MIXED_SHAPES)
def test_unlike_polyhedra_in_one_batch(gpu_lib, monkeypatch, shape, exact):
    """(c) six polyhedra with different margins, pairs and seeds in one call: each gets the verdicts of its own daqp_minrep call
    (the reference's signature, P = 1) and its own truth -- the shared image, the scaling and the structural bits are per polyhedron"""
    import daqp_amd
    _env(monkeypatch, exact, None)
    cs = MC.mixed(shape)
    A, b, truth = MC.stack(cs)
    n, m, ms = shape
    info = {}
    out = daqp_amd.minrep_batch(A, b, ms=ms, info=info)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    for p, case in enumerate(cs):
        Ap, bp = np.ascontiguousarray(case["A"]).copy(), np.ascontiguousarray(case["b"]).copy()
        one = np.full(m, -7, np.int32)
        gpu_lib.daqp_minrep(one.ctypes.data_as(ip), Ap.ctypes.data_as(dp), bp.ctypes.data_as(dp), n, m, ms)
        assert np.array_equal(out[p], one), (shape, p, np.flatnonzero(out[p] != one))
        assert np.array_equal(Ap, case["A"]) and np.array_equal(bp, case["b"])      # the inputs are left as they were
    assert np.array_equal(out, truth), (shape, _where(out, truth))
    assert info["unresolved"] == 0


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("shape", [(8, 65, 0), (80, 200, 5)])
def test_vanishing_rows_among_the_others(gpu_lib, monkeypatch, shape, exact):
    """(d) zero rows of A at the first, a middle and the last general-row position (second polyhedron: one row further inside, so
    the structural bits of one polyhedron cannot stand in for the other's): -1 there, and every other row keeps the truth it has
    without them"""
    import daqp_amd
    _env(monkeypatch, exact, None)
    built = [MC.with_zero_rows(case, shift) for shift, case in enumerate(MC.cases(shape, 1e-3))]
    A, b, want = (np.ascontiguousarray(np.stack([t[k] for t in built])) for k in range(3))
    info = {}
    out = daqp_amd.minrep_batch(A, b, ms=shape[2], info=info)
    assert (want == -1).sum() == 3 * len(built) and not np.array_equal(want[0] == -1, want[1] == -1)
    assert np.array_equal(out, want), (shape, _where(out, want))
    assert info["unresolved"] == 0


@pytest.mark.parametrize("run", [((8, 65, 0), None), ((50, 150, 10), "1"), ((80, 200, 5), None)], ids=["register", "image", "workgroup"])
def test_device_resident_inputs(gpu_lib, monkeypatch, run):
    """(e) torch device tensors in, a device tensor out: the same int32 bits as from host arrays, one clear case per kernel family"""
    import daqp_amd
    import torch
    shape, img = run
    _env(monkeypatch, 0, img)
    A, b, truth = MC.stack(MC.cases(shape, 1e-3))
    host = daqp_amd.minrep_batch(A, b, ms=shape[2])
    tA, tb = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
    info = {}
    dev = daqp_amd.minrep_batch(tA, tb, ms=shape[2], out="torch", info=info)
    assert dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == truth.shape
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), host.view(np.uint32))
    assert np.array_equal(host, truth) and info["unresolved"] == 0
    assert np.array_equal(tA.cpu().numpy(), A) and np.array_equal(tb.cpu().numpy(), b)      # used in place, not written


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("delta", MC.CLEAR)
def test_row_scale_does_not_change_a_verdict(gpu_lib, monkeypatch, delta, exact):
    """(f) the general rows of (12, 130, 12) rescaled to lengths 10**U(-4, 4), b with them: the polyhedron and so the truth are the
    same, and the GPU normalises its rows, so the verdicts are the same.  (The new scale replaces the generator's 10**U(-2, 2), it
    does not multiply it: |A_i|^2 stays >= 1e-8, clear of zero_tol = 1e-11, below which a row counts as vanishing and is reported
    as -1 by the documented convention.)"""
    import daqp_amd
    shape = (12, 130, 12)
    _env(monkeypatch, exact, None)
    A, b, truth = MC.stack(MC.cases(shape, delta))
    s = 10.0 ** np.random.default_rng([7, int(-np.log10(delta))]).uniform(-4.0, 4.0, (A.shape[0], A.shape[1]))
    s = s / np.linalg.norm(A, axis=2)
    A2, b2 = A * s[:, :, None], b.copy()
    b2[:, shape[2]:] *= s
    info = {}
    out = daqp_amd.minrep_batch(np.ascontiguousarray(A2), b2, ms=shape[2], info=info)
    assert np.array_equal(out, truth), (delta, exact, _where(out, truth))
    assert info["unresolved"] == 0
