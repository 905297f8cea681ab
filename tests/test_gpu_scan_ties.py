"""The fp32 screening scans on planted near-ties (tests/scan_tie_cases.py), pick for pick: rscan_rows_img (IMG = 1, the split block of
IMG = 2, the image-only shapes) and wg_scan32 / wscan take a verdict from the fp32 image of M only outside the band E; a second row's
slack planted within delta |u| of the winner's (or of its own threshold), delta from 2^-34 to 2^-14, is told apart correctly only if
the band sends the scan to fp64 whenever fp32 cannot decide it.  Bar: the project's own -- against the oracle, per problem, the event
trace step for step, exit flag, iteration count, the signs of lam, |x - x_ref|_inf < 1e-9.  Every test first reads the plan of the
live batch (daqp_batch_describe): a batch on another kernel would check nothing.  The control solves the same batch with the fp32
scans switched off (DAQP_AMD_NO_IMG32 / DAQP_AMD_NO_SCAN32): a failure there means the default arithmetic cannot resolve the case,
not that the screen is wrong, and is reported as such."""
import ctypes as C

import numpy as np
import pytest

import scan_tie_cases as S

pytestmark = pytest.mark.gpu
XTOL = 1e-9
CELLS = [(fam, kind) for fam in S.FAMILIES for kind in S.KINDS]


@pytest.fixture(autouse=True)
def default_arithmetic(monkeypatch):
    monkeypatch.delenv("DAQP_AMD_EXACT", raising=False)
    monkeypatch.setenv("DAQP_AMD_NO_RECHECK", "1")      # the kernel's own verdicts
    monkeypatch.setenv("DAQP_AMD_IMG_MIN_BATCH", "1")
    for k in ("DAQP_AMD_IMG_ROWS", "DAQP_AMD_IMG_CACHE", "DAQP_AMD_IMG_WAVES", "DAQP_AMD_NO_IMG32", "DAQP_AMD_NO_IMG_ONLY", "DAQP_AMD_NO_SCAN32"):
        monkeypatch.delenv(k, raising=False)


def plan_of(bm):
    import daqp_amd
    buf = C.create_string_buffer(8192)
    daqp_amd.lib().daqp_batch_describe(bm._h, buf, 8192)
    return dict(t.split("=", 1) for t in buf.value.decode().split(" "))


def solve_cases(fam, cases):
    """the cases as ONE batch: (plan, per solve (result dict, traces with markers))"""
    import daqp_amd
    F = S.FAMILIES[fam]
    a = S.batch_arrays(cases)
    bm = daqp_amd.BatchModel(len(cases), F["n"], F["m"], F["ms"], ns_max=F["ns"])
    bm.enable_trace(2048)
    plan = plan_of(bm)
    bm.setup(a["H"], a["f"], a["A"], a["bupper"], a["blower"], a["sense"])
    runs = [(bm.solve(), bm.read_trace(marks=True))]
    if a["f2"] is not None:
        bm.update(f=a["f2"])
        runs.append((bm.solve(), bm.read_trace(marks=True)))
    bm.close()
    return plan, runs


def mismatches(cases, runs):
    """every problem that misses the bar: (case index, delta as a power of two, sigma, solve, what)"""
    bad = []
    for k, c in enumerate(cases):
        tag = (k, int(np.log2(c["delta"])), c["sigma"], c["regions"])
        for stage, (exp, (g, tr)) in enumerate(zip(c["expect"], runs)):
            if not np.array_equal(tr[k], exp["trace"]):
                first = next((i for i, (p, e) in enumerate(zip(tr[k], exp["trace"])) if p != e), min(len(tr[k]), len(exp["trace"])))
                bad.append(tag + (stage, f"trace differs at event {first} (the planted scan: {c['pos']})"))
            elif g["exitflag"][k] != exp["flag"] or g["iter"][k] != exp["iter"]:
                bad.append(tag + (stage, f"flag {g['exitflag'][k]} / {exp['flag']}, iterations {g['iter'][k]} / {exp['iter']}"))
            elif not np.array_equal(np.sign(g["lam"][k]), np.sign(exp["lam"])):
                bad.append(tag + (stage, "signs of lam"))
            elif not np.abs(g["x"][k] - exp["x"]).max() < XTOL:
                bad.append(tag + (stage, f"|x - x_ref| = {np.abs(g['x'][k] - exp['x']).max():.2e}"))
    return bad


@pytest.mark.parametrize("fam,kind", CELLS, ids=[f"{f}-{k}" for f, k in CELLS])
def test_screening_scan_on_planted_ties(gpu_lib, monkeypatch, fam, kind):
    F = S.FAMILIES[fam]
    cases, _ = S.build(fam, kind)
    plan, runs = solve_cases(fam, cases)
    assert plan[F["path"]] == "1", f"the batch is not on the intended path ({F['path']}): {plan}"
    if F["img_kind"]:
        assert int(plan["img_kind"]) == F["img_kind"], plan
    bad = mismatches(cases, runs)
    # the control: fp64 scans only
    monkeypatch.setenv("DAQP_AMD_NO_SCAN32" if F["path"] == "has_m32" else "DAQP_AMD_NO_IMG32", "1")
    cplan, cruns = solve_cases(fam, cases)
    assert cplan[F["path"]] == "0", f"the control still runs the fp32 scan: {cplan}"
    cbad = mismatches(cases, cruns)
    print(f"{fam} {kind}: {len(cases)} problems, {len(bad)} miss the bar with the fp32 screen, {len(cbad)} with fp64 scans only")
    assert not cbad, f"CONTROL (fp64 scans only): the default arithmetic does not resolve {len(cbad)} of {len(cases)} cases: {cbad[:8]}"
    assert not bad, f"SCREEN: {len(bad)} of {len(cases)} cases differ from the oracle with the fp32 screening scan and agree without it: {bad[:8]}"
