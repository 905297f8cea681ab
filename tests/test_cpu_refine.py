"""daqp_batch_refine without a GPU: the symbol, its Python wrapper and translation unit are there, and the planted cases of
tests/refine_cases.py are what tests/test_gpu_refine.py needs them to be -- exactly representable, solved by the oracle at the planted
working set, refined by the CPU model to the last bits, and ill-conditioned enough that the unrefined solution is visibly off."""
import os
import re
import subprocess

import numpy as np
import pytest

import refine_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = [str(c["shape"][0]) for c in RC.CASES]


def test_symbol_declared_listed_and_exported():
    import daqp_amd
    from daqp_amd import _lib
    header = open(os.path.join(ROOT, "include", "daqp_amd.h")).read()
    assert re.search(r"\bint\s+daqp_batch_refine\s*\(\s*DAQPBatch\s*\*", header)
    assert "daqp_batch_refine" in _lib.EXPORTS
    daqp_amd.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIBPATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT daqp_batch_refine\b", syms)
    assert len(daqp_amd.lib().daqp_batch_refine.argtypes) == 9
    assert callable(getattr(daqp_amd.BatchModel, "refine"))


def test_unit_is_built_on_its_own():
    from daqp_amd import _lib
    assert "refine_kernel.hip" in _lib.UNITS and "refine.hip.h" in _lib.UNITS["refine_kernel.hip"]
    assert "refine.hip.h" in _lib.UNITS["post_solve.hip"]      # the host unit that launches it


def test_wave_tier_keeps_nothing_in_scratch():
    """the code generator's own report of the new unit: no scratch and no VGPR spill in any tier"""
    import daqp_amd
    from daqp_amd import _lib
    daqp_amd.build()
    res = {k: v for k, v in _lib.kernel_resources().items() if k.startswith("k_refine<")}
    assert len(res) == 3, sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)


def test_shapes_and_condition_numbers():
    assert [c["shape"] for c in RC.CASES] == [(12, 30, 4), (50, 100, 0), (64, 96, 8), (80, 120, 0), (130, 150, 2)]
    for i, c in enumerate(RC.CASES):
        cond = np.linalg.cond(RC.case(i)["H"])
        assert RC.COND_RANGE[0] <= cond <= RC.COND_RANGE[1], (c["shape"], cond)
        assert abs(cond - c["cond"]) <= 0.05 * c["cond"], (c["shape"], cond, c["cond"])


@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=CASE_IDS)
def test_every_datum_is_exact(i):
    p = RC.case(i)
    assert RC.exact(p)
    W, low, ms = p["W"], p["lower"], p["ms"]
    assert low.any() and (~low[:-1]).any()                                  # both sides
    assert (W >= ms).any() and (ms == 0 or (W < ms).any())                  # general rows, and simple bounds where there are any
    assert p["bupper"][W[-1]] == p["blower"][W[-1]] and W[-1] >= ms         # an equality row
    assert (p["bupper"][W[:-1]] > p["blower"][W[:-1]]).all()


@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=CASE_IDS)
def test_oracle_ends_at_the_planted_working_set(oracle, i):
    p = RC.case(i)
    x, lam, flag, ids, low = RC.oracle_solution(oracle, p)
    assert flag == 1
    assert np.array_equal(ids, p["W"])
    assert np.array_equal(low[:-1], p["lower"][:-1])      # (the equality row may be held on either side)
    assert np.array_equal(np.flatnonzero(lam), p["W"])


@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=CASE_IDS)
def test_model_reaches_the_last_bits(oracle, i):
    p = RC.case(i)
    x, lam, _, ids, low = RC.oracle_solution(oracle, p)
    xm, lm, steps, mu0, mu1 = RC.refine_model(p, x, lam, ids, low)
    print(p["n"], "E before %.2e after %.2e" % (RC.error(p, x, lam), RC.error(p, xm, lm)), "steps", steps, "mu %.2e -> %.2e" % (mu0, mu1))
    assert RC.error(p, xm, lm) <= 2.0 ** -49
    assert mu1 <= mu0 and steps >= 1
    assert RC.model_error(i) == RC.error(p, xm, lm)
    # from zeros the model solves the system, it does not echo its input
    xz, lz, _, _, _ = RC.refine_model(p, np.zeros(p["n"]), np.zeros(p["m"]), ids, low, max_steps=8)
    assert RC.error(p, xz, lz) <= 2.0 ** -49


def test_the_unrefined_solution_is_visibly_off(oracle):
    off = 0
    for i in range(len(RC.CASES)):
        p = RC.case(i)
        x, lam, _, _, _ = RC.oracle_solution(oracle, p)
        off += RC.error(p, x, lam) >= 2.0 ** -36
    assert 2 * off >= len(RC.CASES), off
