"""The solve plan (csrc/plan.hip.h) without a device: daqp_amd_describe_plan against the table recorded from the parent commit's batch_create
(tests/golden/plan_table.json), the invariants of a plan over n = 1..511, pick_path against a truth table written from launch_ldp's branches as
they stood before the plan existed, and the pool key against the list of switches it had then."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import daqp_amd

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "plan_table.json")))
# the pool key of the parent commit: its env_signature() list, in its order
KEY_SWITCHES = ["LDS_LIMIT", "FORCE_SPILL", "STREAM_M", "NO_WG", "WG_WAVES", "WG_CAPL", "WG_GRID", "NO_WG_TIER", "WG_R0", "WG_TIER_GRID", "WG_TIER_MIN_BATCH",
                "SLOW_SETUP", "NO_SCAN32", "WG_INVERSE", "NO_TINY_SETUP", "NO_RECHECK", "NO_SETUP_M", "NO_BLK_SETUP", "REG_ROWS", "NO_REG_HANDOVER", "NO_FACT_WG",
                "NO_FACT_SMALL", "NO_IMG32", "IMG_ROWS", "IMG_MIN_BATCH", "IMG_WAVES", "IMG_CACHE", "IMG_WARM_ROWS", "IMG_WARM_WAVES", "NO_IMG_ONLY",
                "IMG_ONLY_MIN_BATCH", "NO_BLK_BOUNDS"]
NOT_IN_KEY = ["EXACT", "NO_POOL", "NO_MAPPED_RESULTS", "EAGER_UPDATE", "NO_EXIT_SYNC", "RECHECK_DEVICE"]
WG, WG_TIER, REG, REG_IMG, N64_IMG_ONLY, REG_HANDOVER, WAVE, WAVE_IMG_ONLY = range(8)      # enum SolvePath


def describe(jobs, env=None):
    """lines of daqp_amd_describe_plan for jobs [[N, n, m, ms, ns_max, cus, per_cu, tier_attr_ok, per_cu_tier], ...], in a child with exactly `env`'s switches"""
    daqp_amd.build()
    e = {k: v for k, v in os.environ.items() if not k.startswith("DAQP_AMD_")}
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(HERE, "plan_child.py")], input=json.dumps(jobs), capture_output=True, text=True, env=e, check=True)
    return r.stdout.split("\n")


def fields(line):
    return dict(t.split("=", 1) for t in line.split(" "))


def job(r):
    return [r[k] for k in ("N", "n", "m", "ms", "ns_max", "cus", "per_cu", "tier_attr_ok", "per_cu_tier")]


@pytest.fixture(scope="module")
def golden_lines():
    """one child per distinct environment of the table"""
    groups = {}
    for i, r in enumerate(GOLDEN["rows"]):
        groups.setdefault(json.dumps(r["env"], sort_keys=True), []).append(i)
    lines = [None] * len(GOLDEN["rows"])

    def run(item):
        env, idx = item
        for i, line in zip(idx, describe([job(GOLDEN["rows"][i]) for i in idx], json.loads(env))):
            lines[i] = line
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(run, groups.items()))
    return lines


def test_golden_table_covers_every_family():
    assert len(GOLDEN["parent"]) == 40 and len(GOLDEN["rows"]) >= 200
    k = GOLDEN["plan_keys"]
    plans = [dict(zip(k, r["plan"])) for r in GOLDEN["rows"] if "plan" in r]
    for what in ("tiny_setup", "img32", "img_only", "reg_handover", "use_wg", "wg_tier_grid", "fact_gs", "setup_spill", "spill", "img_rows_warm"):
        assert any(p[what] for p in plans) and any(not p[what] for p in plans), what
    assert {p["img_kind"] for p in plans} == {0, 1, 2} and any(p["C"] == 8 for p in plans)
    assert sum("refused" in r for r in GOLDEN["rows"]) >= 5
    assert len({s for r in GOLDEN["rows"] for s in r["env"]}) >= 25     # switches exercised


def test_plan_matches_parent_commit(golden_lines):
    """field by field, exactly: what the parent's batch_create chose for the row is what plan_shape + plan_device choose"""
    wrong = []
    for r, line in zip(GOLDEN["rows"], golden_lines):
        if "refused" in r:
            if line != "refused=" + r["refused"]:
                wrong.append((job(r), r["env"], line))
            continue
        got = fields(line)
        want = dict(zip(GOLDEN["plan_keys"], r["plan"]), N=r["N"], n=r["n"], m=r["m"], ms=r["ms"], ns_max=r["ns_max"])
        diff = {k: (v, got.get(k)) for k, v in want.items() if got.get(k) != str(v)}
        if diff:
            wrong.append((job(r), r["env"], diff))
    assert not wrong, wrong[:5]


@pytest.fixture(scope="module")
def walk():
    jobs = []
    for n in range(1, 512):
        for m in sorted({0, 1, n // 2, n, 2 * n, 3 * n, 64, 128, 129, 192, 256, 257, 320, 384, 512, 600}):
            for ms in sorted({0, min(m, n) // 2, min(m, n)}):
                for ns in (0, 3):
                    for N in (1, 2, 4096, 20000):
                        jobs.append([N, n, m, ms, ns, 256, 1, 1, 2])
    return jobs, describe(jobs)


def test_walk_invariants(walk):
    jobs, lines = walk
    assert len(jobs) == len(lines)
    KB160 = 160 * 1024
    seen = set()
    for j, line in zip(jobs, lines):
        N, n, m, ms, ns = j[:5]
        if line.startswith("refused="):
            assert n + ns + 1 > 512 or "too large for the LDS" in line, (j, line)
            continue
        assert n + ns + 1 <= 512
        p = {k: (v if k in ("paths", "env_key") else int(v)) for k, v in fields(line).items()}
        cap = p["cap"]
        assert cap == n + ns + 1 and p["nblk"] == (m + 63) // 64 and p["npair"] == (n + 1) // 2
        assert len(p["paths"]) == 24 and set(p["paths"]) <= set("01234567")      # exactly one path for each (mode, exact, fresh, image allowed)
        seen |= set(p["paths"])
        for k in ("lds_fb", "lds_img", "lds_img_warm", "lds_wg", "lds_wg_tier", "lds_setup", "lds_ldp", "lds_update"):
            assert 0 <= p[k] <= KB160, (j, k, p[k])
        if p["NB"]:
            assert p["nblk"] <= p["NB"] and p["npair"] <= p["NP"], j
        if p["img_only"]:
            assert p["nblk"] <= p["io_nb"] and p["npair"] <= p["io_np"], j
        if p["img32"] or p["img_only"]:
            assert 2 <= p["img_cache"] <= p["img_rows"] <= min(cap, 64), j
        if p["img32"]:
            assert p["img_rows_warm"] < p["img_rows"], j
        assert p["spill"] + p["img32"] + p["img_only"] <= 1, j      # one owner of rowc_g
        if p["use_wg"]:
            assert p["NB"] == 0 and not p["img_only"] and 64 < cap <= 256, j
            assert 1 <= p["wg_grid"] <= N and 4 <= p["wg_W"] <= 8 and p["wg_capL"] <= cap
        if p["wg_tier_grid"]:
            assert p["use_wg"] and 32 <= p["wg_r0"] < cap and 0 < p["lds_wg_tier"] <= (KB160 - 512) // 2 - 256, j
        assert p["tiny_setup"] <= p["fast_setup"] and not (p["fast_setup"] and (p["setup_spill"] or p["fact_gs"])), j
    assert seen == set("01234567")      # the walk meets every path


def plan_line(walk_or_lines, want):
    for line in walk_or_lines:
        if not line.startswith("refused=") and all(fields(line)[k] == str(v) for k, v in want.items()):
            return fields(line)
    raise AssertionError(f"no plan with {want}")


# one row per branch of launch_ldp as it stood at the parent commit: (what selects a plan of the branch's family, then
# path(mode, exact_kernels, fresh, img_allowed) written out by hand)
TRUTH = [
    # if (use_wg): tiered launch in front only for (wg_tier_grid > 0 && fresh && mode == 0 && !exact)
    (dict(use_wg=1, wg_tier_grid=0), lambda mode, ex, fresh, img: WG),
    (dict(use_wg=1, n=150, m=300, N=4096), lambda mode, ex, fresh, img: WG_TIER if (fresh and mode == 0 and not ex) else WG),
    # if (NB > 0): use_img = img32 && !exact && (what the launch knows) -> image kernel in front, any mode
    (dict(NB=3, NP=25, img32=1), lambda mode, ex, fresh, img: REG_IMG if (not ex and img) else REG),
    (dict(NB=3, NP=25, img32=0), lambda mode, ex, fresh, img: REG),
    (dict(NB=1, NP=6), lambda mode, ex, fresh, img: REG),
    # reg_handover && img_only && mode == 0 && !exact: the n = 64 image-only launch; otherwise the register kernel with k_ldp behind it
    (dict(NB=2, NP=32, reg_handover=1, img_only=1), lambda mode, ex, fresh, img: N64_IMG_ONLY if (mode == 0 and not ex) else REG_HANDOVER),
    (dict(NB=2, NP=32, reg_handover=1, img_only=0), lambda mode, ex, fresh, img: REG_HANDOVER),
    # the one-wave kernel: image-only in front for (img_only && mode == 0 && !exact)
    (dict(NB=0, use_wg=0, img_only=1), lambda mode, ex, fresh, img: WAVE_IMG_ONLY if (mode == 0 and not ex) else WAVE),
    (dict(NB=0, use_wg=0, img_only=0), lambda mode, ex, fresh, img: WAVE),
]


@pytest.mark.parametrize("case", range(len(TRUTH)))
def test_pick_path_truth_table(walk, case):
    want, rule = TRUTH[case]
    p = plan_line(walk[1], want)
    for i in range(24):
        mode, ex, fresh, img = i >> 3, bool(i >> 2 & 1), bool(i >> 1 & 1), bool(i & 1)
        assert int(p["paths"][i]) == rule(mode, ex, fresh, img), (want, mode, ex, fresh, img)


def test_pool_key_follows_exactly_the_listed_switches():
    j = [[1, 50, 150, 0, 0, 0, 0, 0, 0]]
    base = fields(describe(j)[0])["env_key"]
    assert base.count("|") == len(KEY_SWITCHES)

    def key(name):
        return fields(describe(j, {"DAQP_AMD_" + name: "3"})[0])["env_key"]
    with ThreadPoolExecutor(8) as ex:
        changed = dict(zip(KEY_SWITCHES + NOT_IN_KEY, ex.map(key, KEY_SWITCHES + NOT_IN_KEY)))
    for i, name in enumerate(KEY_SWITCHES):
        parts, want = changed[name].split("|"), base.split("|")
        want[i] = "3"
        assert parts == want, name          # its own slot, and only that
    for name in NOT_IN_KEY:
        assert changed[name] == base, name
