"""The polyhedra of tests/minrep_cases.py without a GPU: their certificates (np.longdouble: a witness on the face of every row
called not redundant, a Farkas combination for every row called redundant), the coverage the GPU tests rely on, and -- where the
reference build exists -- the reference's daqp_minrep on the normalised rows against the truth and against the committed record
tests/golden/golden_minrep_truth.npz."""
import importlib.util
import os

import numpy as np
import pytest

import minrep_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
ALL_DELTAS = MC.CLEAR_ALL + MC.NEAR


@pytest.fixture(scope="module")
def ref():
    from oracle import oracle as O
    if not O.reference_available(strict=True):
        pytest.skip("oracle/_ref is not built here (reference sources not present)")
    spec = importlib.util.spec_from_file_location("make_golden_minrep_truth", os.path.join(HERE, "golden", "make_golden_minrep_truth.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    G.ref = G.ref_minrep()
    return G


@pytest.mark.parametrize("shape", MC.SHAPES)
def test_certificates_hold(shape):
    """verify() for every case the GPU file uses: the two polyhedra per delta, the six unlike ones of the mixed batch"""
    for delta in ALL_DELTAS:
        for case in MC.cases(shape, delta):
            MC.verify(case)
            assert case["A"].shape == (shape[1] - shape[2], shape[0]) and case["b"].shape == (shape[1],)
    if shape in MC.MIXED_SHAPES:
        for case in MC.mixed(shape):
            MC.verify(case)


def test_verify_rejects_a_wrong_margin():
    """a redundant row pulled inside its Farkas bound, a witness pushed off its face: verify() says so"""
    case = MC.make_case(8, 65, 0, 1e-3, 1e-3, 0)
    j = next(iter(case["farkas"]))
    bad = dict(case, b=case["b"].copy())
    bad["b"][j] -= 2 * case["delta"] * np.linalg.norm(case["A"][j])
    with pytest.raises(AssertionError, match="Farkas margin"):
        MC.verify(bad)
    j = next(iter(case["witness"]))
    bad = dict(case, witness=dict(case["witness"]))
    bad["witness"][j] = case["witness"][j] * (1 + 1e-9)
    with pytest.raises(AssertionError, match="witness off its face"):
        MC.verify(bad)


@pytest.mark.parametrize("shape", MC.SHAPES)
def test_coverage_of_a_shape(shape):
    """both verdicts, a planted near-parallel pair whose rows are both core rows, and with simple bounds a redundant and a
    non-redundant one -- in every polyhedron; every gamma is met within the shape"""
    ms = shape[2]
    gammas = set()
    for delta in ALL_DELTAS:
        for case in MC.cases(shape, delta):
            t = case["truth"]
            assert (t == 0).any() and (t == 1).any() and set(np.unique(t)) == {0, 1}
            assert len(case["pairs"]) >= 1
            R, _ = MC.full_rows(case)
            for a, b in case["pairs"]:
                assert t[a] == 0 and t[b] == 0
                dot = R[a] @ R[b] / (np.linalg.norm(R[a]) * np.linalg.norm(R[b]))
                assert abs(dot - (1 - case["gamma"])) < 1e-12
            if ms > 0:
                assert (t[:ms] == 1).any() and (t[:ms] == 0).any()
            gammas.add(case["gamma"])
    assert gammas == set(MC.GAMMAS)


def test_negative_right_hand_sides_and_scales():
    """at least 10 % of all b are negative (the origin lies outside); general rows span four decades of scale"""
    bs, norms = [], []
    for shape in MC.SHAPES:
        for delta in ALL_DELTAS:
            for case in MC.cases(shape, delta):
                bs.append(case["b"])
                norms.append(np.linalg.norm(case["A"], axis=1))
    bs, norms = np.concatenate(bs), np.concatenate(norms)
    assert (bs < 0).mean() >= 0.10
    assert norms.min() < 0.03 and norms.max() > 30


@pytest.mark.parametrize("shape", MC.SHAPES)
def test_reference_equals_truth_at_clear_margins(ref, shape):
    """the reference on the normalised rows, every clear delta: exactly the truth"""
    for delta in MC.CLEAR_ALL:
        for case in MC.cases(shape, delta):
            An, bn = MC.normalised(case)
            red = ref.ref(An, bn, shape[2])
            assert np.array_equal(red, case["truth"]), (shape, delta, case["seed"], np.flatnonzero(red != case["truth"]))


@pytest.mark.parametrize("shape", MC.SHAPES)
def test_reference_never_drops_a_core_row(ref, shape):
    """any delta, normalised rows and rows as given, and the mixed batch: no row with a witness is called redundant"""
    some = [c for delta in ALL_DELTAS for c in MC.cases(shape, delta)] + (list(MC.mixed(shape)) if shape in MC.MIXED_SHAPES else [])
    for case in some:
        An, bn = MC.normalised(case)
        for red in (ref.ref(An, bn, shape[2]), ref.ref(case["A"], case["b"], shape[2])):
            assert set(np.unique(red)) <= {0, 1}
            assert not ((case["truth"] == 0) & (red != 0)).any(), (shape, case["delta"], case["seed"])


@pytest.mark.parametrize("shape", MC.SHAPES)
def test_fixture_is_what_the_reference_answers(ref, shape):
    """golden_minrep_truth.npz regenerated: verdicts and stability bits"""
    z = np.load(os.path.join(HERE, "golden", "golden_minrep_truth.npz"))
    for delta in MC.NEAR:
        red, stable = ref.record(ref.ref, shape, delta)
        key = MC.fixture_key(shape, delta)
        assert np.array_equal(red, z["red_" + key]) and np.array_equal(stable, z["stable_" + key]), key


def test_fixture_consistent_with_the_truth():
    """(needs no reference build) the record has every case, never calls a core row redundant, and at most 2 % of a shape's rows
    are unstable under the 1e-9 push"""
    z = np.load(os.path.join(HERE, "golden", "golden_minrep_truth.npz"))
    assert len(z.files) == 2 * len(MC.SHAPES) * len(MC.NEAR)
    for shape in MC.SHAPES:
        unstable, rows = 0, 0
        for delta in MC.NEAR:
            key = MC.fixture_key(shape, delta)
            truth = MC.stack(MC.cases(shape, delta))[2]
            red, stable = z["red_" + key], z["stable_" + key]
            assert red.dtype == np.int8 and red.shape == truth.shape == stable.shape
            assert not ((truth == 0) & (red != 0)).any(), key
            unstable += int((stable == 0).sum())
            rows += stable.size
        assert unstable <= 0.02 * rows, (shape, unstable, rows)
