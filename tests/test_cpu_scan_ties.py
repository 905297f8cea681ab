"""The planted near-ties of tests/scan_tie_cases.py, checked without a GPU: every (family, kind, delta, sigma) cell meets its cap from the
oracle alone, every case does what it was planted to do in both fp64 arithmetics of the oracle, and a float32 model of the scan gets
at least a quarter of the cases with delta <= 2^-30 wrong in every family -- the cases would convict a kernel that trusted fp32."""
import collections

import numpy as np
import pytest

import scan_tie_cases as S

FAMS = list(S.FAMILIES)


@pytest.mark.parametrize("fam", FAMS)
def test_every_cell_meets_the_cap(fam):
    cap = S.cap_of(fam)
    assert cap == (24 if S.FAMILIES[fam]["n"] <= 64 else 8)
    for kind in S.KINDS:
        cases, stats = S.build(fam, kind)           # (raises when a cell stays below the cap)
        count = collections.Counter((c["delta"], c["sigma"]) for c in cases)
        assert set(count) == {(d, s) for d in S.DELTAS for s in S.SIGMAS}
        assert all(v == cap for v in count.values()), count
        assert all(valid >= cap and tried >= valid for valid, tried in stats.values())
        assert all(c["unorm"] > 0 for c in cases)
        if kind != "threshold":
            assert all(c["r1"] is not None and c["r1"] != c["r2"] for c in cases)
            if kind != "warm":
                assert all(c["pos"] >= 1 for c in cases)           # k >= 1: a scan with a working set behind it
                assert any(c["after_remove"] for c in cases), "no scan that follows a remove event"
        else:
            # (the final scan: the solve stops there on one side and goes on on the other)
            assert all(c["r1"] is None and (len(c["expect"][0]["trace"]) == c["pos"] if c["sigma"] > 0 else len(c["expect"][0]["trace"]) > c["pos"]) for c in cases)
        if S.FAMILIES[fam]["ns"]:
            assert all(c["soft_active"] for c in cases), "a scan without an active SOFT row in the soft family"
    regions = collections.Counter(c["regions"] for c in S.build(fam, "pick")[0])
    if fam == "img2-50x150":        # r1 / r2 both in the split block, both in full blocks, across the two
        assert all(regions[r] >= 14 for r in (("split", "split"), ("full", "full"), ("full", "split"), ("split", "full"))), regions
    if fam == "img2-17x129":        # (one row in the split block)
        assert regions[("full", "split")] >= 14, regions
    if fam == "img1-60x120-bounds":
        assert sum(v for r, v in regions.items() if r[1] == "bound") >= 14, regions


@pytest.mark.parametrize("fam", FAMS)
def test_cases_hold_in_both_oracle_arithmetics(fam):
    ora, fast = S._oracles()
    for kind in S.KINDS:
        for c in S.build(fam, kind)[0]:
            a, b = S.run_oracle(ora, fam, c["q"], c["f2"]), S.run_oracle(fast, fam, c["q"], c["f2"])
            assert S._same_run(a, b)
            assert all(np.array_equal(x["trace"], e["trace"]) and x["iter"] == e["iter"] for x, e in zip(a["solves"], c["expect"]))
            tr = a["solves"][-1]["trace"]
            if c["r1"] is not None:
                assert tr[c["pos"]] == (c["r1"] if c["sigma"] > 0 else c["r2"]) + 1
            elif c["sigma"] < 0:
                assert tr[c["pos"]] == c["r2"] + 1
            else:
                assert len(tr) == c["pos"] and c["r2"] + 1 not in np.abs(tr)


@pytest.mark.parametrize("fam", FAMS)
def test_float32_model_fails_a_quarter_of_the_small_gaps(fam):
    for kind in S.KINDS:
        small = [c for c in S.build(fam, kind)[0] if c["delta"] <= 2.0 ** -30]
        wrong = sum(not c["model"] for c in small)
        print(f"{fam} {kind}: float32 model wrong on {wrong} of {len(small)} cases with delta <= 2^-30")
        assert 4 * wrong >= len(small), (kind, wrong, len(small))
