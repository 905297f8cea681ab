"""The plan of live batches: daqp_batch_describe against the table recorded from the parent commit (one row per solve path), and the pool of
one-problem workspaces keyed by the switches of the plan."""
import ctypes as C
import json
import os

import pytest

import daqp_amd

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_table.json")))
DEVICE_KEYS = ("cus", "per_cu", "tier_attr_ok", "per_cu_tier")
# (N, n, m, ms, ns_max, env): one golden row per path of launch_ldp, plus the setup families
ROWS = [
    (600, 100, 300, 0, 0, {}),                                  # workgroup
    (600, 150, 300, 0, 0, {}),                                  # workgroup, tiered launch in front
    (4096, 12, 64, 0, 0, {}),                                   # register (1,6)
    (20000, 50, 150, 0, 0, {}),                                 # register (3,25) with the image in front, img_kind 2
    (64, 50, 192, 0, 0, {"DAQP_AMD_IMG_MIN_BATCH": "1"}),       # ... img_kind 1
    (64, 64, 128, 0, 0, {}),                                    # n = 64: image-only in front of k_ldp
    (1, 64, 128, 0, 0, {}),                                     # register with hand-over
    (4096, 8, 256, 0, 0, {}),                                   # one-wave, M streamed
    (64, 60, 256, 0, 0, {}),                                    # one-wave with image-only in front
    (64, 12, 48, 0, 0, {}),                                     # tiny setup
    (100, 140, 280, 0, 0, {}),                                  # generic setup beyond the LDS-resident factors
    (100, 300, 400, 0, 0, {}),                                  # cap > 256
]


def fields(line):
    return dict(t.split("=", 1) for t in line.split(" "))


def golden_row(N, n, m, ms, ns, env):
    for r in GOLDEN["rows"]:
        if (r["N"], r["n"], r["m"], r["ms"], r["ns_max"], r["env"]) == (N, n, m, ms, ns, env):
            return r
    raise AssertionError("row not in the golden table")


@pytest.fixture
def switches():
    saved = {k: v for k, v in os.environ.items() if k.startswith("DAQP_AMD_")}
    for k in saved:
        del os.environ[k]
    yield os.environ
    for k in [k for k in os.environ if k.startswith("DAQP_AMD_")]:
        del os.environ[k]
    os.environ.update(saved)


def create(N, n, m, ms, ns):
    L = daqp_amd.lib()
    h = C.c_void_p()
    assert L.daqp_batch_create(C.byref(h), N, n, m, ms, ns, None, 0) == 0, daqp_amd.last_error()
    buf = C.create_string_buffer(8192)
    L.daqp_batch_describe(h, buf, 8192)
    return h, buf.value.decode()


@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"N{r[0]}-n{r[1]}-m{r[2]}" + ("-env" if r[5] else ""))
def test_live_batch_plan_matches_parent_commit(row, switches):
    N, n, m, ms, ns, env = row
    g = golden_row(*row)
    switches.update(env)
    L = daqp_amd.lib()
    h, line = create(N, n, m, ms, ns)
    L.daqp_batch_free(h)
    got = fields(line)
    want = dict(zip(GOLDEN["plan_keys"], g["plan"]))
    if all(int(got[k]) == g[k] for k in DEVICE_KEYS):
        print("compared with the golden row (device numbers as recorded on", GOLDEN["recorded_on"]["device"] + ")")
    else:   # another device than the table's: the pure planner, fed the numbers this batch was created with
        buf = C.create_string_buffer(8192)
        L.daqp_amd_describe_plan(N, n, m, ms, ns, *[int(got[k]) for k in DEVICE_KEYS], buf, 8192)
        ref = fields(buf.value.decode())
        want = {k: int(ref[k]) for k in want}
        print("device numbers differ from the golden row's: compared with daqp_amd_describe_plan fed the batch's own", {k: got[k] for k in DEVICE_KEYS})
    diff = {k: (v, got[k]) for k, v in want.items() if int(got[k]) != v}
    assert not diff, diff


def test_pool_hands_back_under_same_switches_only(switches):
    L = daqp_amd.lib()
    L.daqp_amd_release_pool()
    h1, line1 = create(1, 60, 128, 0, 0)
    L.daqp_batch_free(h1)                       # parked
    h2, line2 = create(1, 60, 128, 0, 0)
    assert h2.value == h1.value and line2 == line1
    L.daqp_batch_free(h2)
    switches["DAQP_AMD_REG_ROWS"] = "40"        # (2,32) with 40 rows held: the hand-over shape
    h3, line3 = create(1, 60, 128, 0, 0)
    assert h3.value != h1.value
    assert fields(line1)["reg_rows"] == "64" and fields(line1)["reg_handover"] == "0"
    assert fields(line3)["reg_rows"] == "40" and fields(line3)["reg_handover"] == "1"
    assert fields(line3)["env_key"] != fields(line1)["env_key"]
    L.daqp_batch_free(h3)
    del switches["DAQP_AMD_REG_ROWS"]
    h4, line4 = create(1, 60, 128, 0, 0)
    assert h4.value == h1.value and line4 == line1
    L.daqp_batch_free(h4)
    L.daqp_amd_release_pool()
