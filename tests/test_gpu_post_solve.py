"""What the post-solve entries (daqp_amd/csrc/post_solve.hip: adjoint, refinement, certificate) share, and what sharing could break.

One planted shape of tests/refine_cases.py per tier of the tier pick -- one wavefront, rows in LDS, rows in scratch --, N = 8 each:
  * adjoint and refinement keep their scratch and their staging slots apart: backward, refine, backward gives the first adjoint again bit
    for bit, and so does refine, backward, refine for the refinement; with host and with device arguments;
  * the certificate from host memory and from device memory has the same bits (the staging of a call of its own);
  * daqp_batch_refine without its optional outputs returns the x, lam and status of a call that asks for them, in both memory kinds.
"""
import ctypes as C

import numpy as np
import pytest

import kkt_cases as K
import refine_cases as RC

N = 8
LDS_MAX = 144 * 1024
TIERS = {"12": (0, "wave"), "80": (3, "lds"), "130": (4, "scratch")}      # id -> (index into RC.CASES, tier)
ENV_KEYS = sorted({k for f in K.FAMILIES for k in f["env"]})


def lds_bytes(kind, n, cap, rl, nl):
    """backward_lds_bytes (backward.hip.h) / refine_lds_bytes (refine.hip.h)"""
    dbl = {"backward": 3 * n + 4 * cap, "refine": 6 * n + 7 * cap + 16}[kind]
    if rl:
        dbl += n * (n + 1) // 2
    if nl:
        dbl += cap * (n | 1) + cap * (cap + 1) // 2
    return dbl * 8 + (2 * cap + 2) * 4


def tier_of(kind, n, cap):
    """the pick of post_solve.hip"""
    small = n <= 64 and lds_bytes(kind, n, cap, True, True) <= LDS_MAX
    nl = small or lds_bytes(kind, n, cap, small, True) <= LDS_MAX
    assert (lds_bytes(kind, n, cap, small, True) if nl else lds_bytes(kind, n, cap, False, False)) <= LDS_MAX
    return "wave" if small else ("lds" if nl else "scratch")


@pytest.mark.parametrize("case", TIERS)
def test_shapes_land_in_the_tiers_named(case):
    i, tier = TIERS[case]
    n = RC.CASES[i]["shape"][0]
    assert str(n) == case
    for kind in ("backward", "refine"):
        assert tier_of(kind, n, n + 1) == tier, (kind, n)      # cap = n + ns_max + 1 with ns_max = 0


def bits_equal(a, b):
    a, b = (np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for v in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same(o1, o2, keys=None):
    keys = o1.keys() if keys is None else keys
    return [k for k in keys if not bits_equal(o1[k], o2[k])]


@pytest.fixture
def solved(gpu_lib, monkeypatch, request):
    """(planted problem, its device tensors, a solved model, the solve's result on the device)"""
    import torch
    import daqp_amd
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DAQP_AMD_EXACT", "0")
    monkeypatch.setenv("DAQP_AMD_NO_RECHECK", "1")
    p = RC.case(TIERS[request.param][0])
    t = {k: torch.from_numpy(np.array(np.broadcast_to(p[k], (N,) + p[k].shape))).cuda() for k in ("H", "f", "A", "bupper", "blower")}
    bm = daqp_amd.BatchModel(N, p["n"], p["m"], p["ms"])
    bm.setup(t["H"], t["f"], t["A"], t["bupper"], t["blower"])
    r = bm.solve(out="torch")
    assert (r["exitflag"] == 1).all()
    yield p, t, bm, r
    bm.close()


def given(r, memory):
    return r if memory == "device" else {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("solved", TIERS, indirect=True)
def test_interleaved_calls_leave_each_other_alone(solved, memory):
    import torch
    p, t, bm, r = solved
    res = given(r, memory)
    g = np.random.default_rng(7).standard_normal((N, p["n"]))
    out = "torch" if memory == "device" else "numpy"
    g = torch.from_numpy(g).cuda() if memory == "device" else g
    b1 = bm.backward(g, out=out)
    r1 = bm.refine(res, max_steps=8)
    b2 = bm.backward(g, out=out)
    r2 = bm.refine(res, max_steps=8)
    b3 = bm.backward(g, out=out)
    torch.cuda.synchronize()
    assert not given(b1, "host")["status"].any() and not given(r1, "host")["status"].any()
    assert given(b1, "host")["dz"].any() and not bits_equal(r1["x"], res["x"])      # both did something
    assert same(b1, b2) == [] and same(b2, b3) == []      # backward, refine, backward
    assert same(r1, r2) == []                             # refine, backward, refine


@pytest.mark.gpu
@pytest.mark.parametrize("solved", TIERS, indirect=True)
def test_certificate_host_and_device_memory_identical_bits(solved):
    import daqp_amd
    p, t, bm, r = solved
    o = bm.refine(r)
    for res in (r, o):
        d = daqp_amd.certify_batch(t["H"], t["f"], t["A"], t["bupper"], t["blower"], res["x"], res["lam"], ms=p["ms"], out="torch")
        h = daqp_amd.certify_batch(*(given(t, "host")[k] for k in ("H", "f", "A", "bupper", "blower")), res["x"].cpu().numpy(),
                                   res["lam"].cpu().numpy(), ms=p["ms"])
        assert all(v.is_cuda for v in d.values()) and all(isinstance(v, np.ndarray) for v in h.values())
        assert same(h, d) == [] and set(h) == set(d) and len(h) == 10
        assert np.isfinite(h["stationarity"]).all() and (h["stationarity_scale"] > 0).all()


def raw_refine(L, bm, res, memory, optional):
    """daqp_batch_refine on copies of res, with or without fval / residual / steps: (x, lam, status) as numpy"""
    import torch
    if memory == "device":
        x, lam = res["x"].clone(), res["lam"].clone()
        fval, resid = res["fval"].clone(), torch.empty((N, 2), dtype=torch.float64, device="cuda")
        steps, status = (torch.full((N,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        ptr = lambda a: C.c_void_p(a.data_ptr())
    else:
        x, lam, fval = (res[k].cpu().numpy().copy() for k in ("x", "lam", "fval"))
        resid, steps, status = np.empty((N, 2)), np.full(N, -7, np.int32), np.full(N, -7, np.int32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)
    opt = [ptr(a) if optional else None for a in (fval, resid, steps)]
    assert L.daqp_batch_refine(bm._h, ptr(x), ptr(lam), *opt, ptr(status), 3, 1 if memory == "device" else 0) == 0
    if memory == "device":
        torch.cuda.synchronize()
    o = dict(x=x, lam=lam, status=status, steps=steps)
    return {k: (v.cpu().numpy() if memory == "device" else v) for k, v in o.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("solved", TIERS, indirect=True)
def test_refine_without_optional_outputs(gpu_lib, solved):
    p, t, bm, r = solved
    first = raw_refine(gpu_lib, bm, r, "host", False)      # (before any call that asks: the slots of the optional outputs do not exist yet)
    full = raw_refine(gpu_lib, bm, r, "host", True)
    assert not full["status"].any() and (full["steps"] >= 1).all() and not bits_equal(full["x"], r["x"])
    assert (first["steps"] == -7).all() and same(full, first, ("x", "lam", "status")) == []
    for memory in ("host", "device"):
        bare = raw_refine(gpu_lib, bm, r, memory, False)
        assert (bare["steps"] == -7).all() and same(full, bare, ("x", "lam", "status")) == [], memory
        assert same(full, raw_refine(gpu_lib, bm, r, memory, True)) == [], memory
