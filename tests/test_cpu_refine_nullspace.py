"""The inputs of tests/test_gpu_refine_nullspace.py held to their conditions on the oracle alone, and the numpy model of the kernel
(tests/refine_nullspace_cases.py) to its bar.  No GPU."""
import numpy as np
import pytest

import refine_cases as RC
import refine_nullspace_cases as NC

FLOOR = 2.0 ** -46      # the floor of tests/test_gpu_refine.py


@pytest.mark.parametrize("i", range(len(NC.CASES)), ids=[NC.label(i) for i in range(len(NC.CASES))])
def test_committed_cases_meet_their_conditions(i):
    c, p = NC.CASES[i], NC.case(i)
    n, m, ms = c["shape"]
    k = c["k"]
    assert NC.exact(p) and NC.kkt_nonsingular(p)
    assert len(p["W"]) == k and len(set(p["W"].tolist())) == k
    if c["kind"] == "singular":
        assert np.linalg.matrix_rank(p["H"]) == c["r"] < n and k >= n - c["r"]
    elif c["kind"] == "lp":
        assert p["H"] is None and k == n
    else:
        assert k == 0 and np.linalg.eigvalsh(p["H"]).min() > 0
    if k >= 2:
        assert p["lower"].any() and not p["lower"].all()      # both sides
    if k >= 4:
        assert (p["W"] >= ms).any() and (ms == 0 or (p["W"] < ms).any())      # general rows, and simple bounds where there are any
        assert (p["bupper"][p["W"]] == p["blower"][p["W"]]).sum() == 1      # one equality
    x, lam, flag, ids, low, n_prox = NC.oracle_side(i)
    assert flag == 1 and NC.planted_working_set(p, ids, low), (flag, ids, p["W"])
    assert n_prox > 0 if i in NC.PROXIMAL else n_prox == 0
    # the model reaches its bar from the oracle's solution, and its run from zeros does not depend on the order of a sum
    assert NC.model_error(i) <= NC.MODEL_BAR, NC.model_error(i)
    trials = []
    xz, lz, steps, mu0, mu1 = NC.refine_nullspace_model(p, np.zeros(n), np.zeros(m), max_steps=8, trials=trials)
    assert steps >= 1 and mu1 <= RC.MU_DONE and NC.decisive(trials), (steps, mu1, trials)
    assert NC.error(p, xz, lz) == NC.model_error(i, zeros=True) <= 1e-9


def test_the_kernel_is_built_exported_and_keeps_out_of_scratch():
    import daqp_amd
    from daqp_amd import _lib
    daqp_amd.build()
    assert "daqp_batch_refine_nullspace" in _lib.EXPORTS and hasattr(_lib.lib(), "daqp_batch_refine_nullspace")
    res = {k: v for k, v in _lib.kernel_resources().items() if k.startswith("k_refine_nullspace<")}
    assert len(res) == 1, sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
    # the existing refinement kernels are the three they were
    assert len([k for k in _lib.kernel_resources() if k.startswith("k_refine<")]) == 3


def test_shapes_cover_what_the_mapping_can_get_wrong():
    ns = {c["shape"][0] for c in NC.CASES}
    assert {1, 5, 16, 33, 64} <= ns
    sing = [NC.CASES[i] for i in NC.SINGULAR]
    assert any(c["k"] == c["shape"][0] - 1 for c in sing) and any(c["k"] == c["shape"][0] - c["r"] < c["shape"][0] - 1 for c in sing)
    assert any(c["k"] == c["shape"][0] for c in sing) and any(c["k"] == 0 for c in NC.CASES)
    for n in (33, 64):
        assert any(c["shape"][0] == n and c["k"] == n - 1 for c in sing) and any(c["shape"][0] == n and c["k"] == n - c["r"] for c in sing)
    assert any(c["shape"][2] > 0 for c in sing) and any(c["shape"][2] == 0 for c in sing)
    assert [RC.CASES[i]["shape"][0] for i in NC.DEFINITE] == [12, 50, 64]


def test_the_oracle_comes_in_far_above_the_model():
    """the singular-H solutions of the proximal loop carry E of 1e-10 .. 1e-4; the model leaves 2^10 below that -- past the bar the GPU
    test holds the kernel to -- on at least half of the cases (the cap of tests/test_gpu_refine.py)"""
    far = 0
    for i in NC.SINGULAR:
        p = NC.case(i)
        x, lam = NC.oracle_side(i)[:2]
        e0, bar = NC.error(p, x, lam), max(8.0 * NC.model_error(i), FLOOR)
        print(NC.label(i), "E oracle %.2e model %.2e from zeros %.2e" % (e0, NC.model_error(i), NC.model_error(i, zeros=True)))
        far += e0 >= 2.0 ** 10 * bar
    assert 2 * far >= len(NC.SINGULAR), far


@pytest.mark.parametrize("i", NC.DEFINITE, ids=[str(RC.CASES[i]["shape"][0]) for i in NC.DEFINITE])
def test_the_model_is_a_second_algorithm_for_definite_hessians(i):
    """on the planted ill-conditioned cases of refine_cases the null-space model reaches what the Gram model reaches"""
    print(RC.CASES[i]["shape"], "null-space model %.2e, Gram model %.2e" % (NC.definite_model_error(i), RC.model_error(i)))
    assert NC.definite_model_error(i) <= 2.0 ** -49
