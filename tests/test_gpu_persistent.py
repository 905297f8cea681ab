"""Persistent workgroups past their first problem, bit for bit (batches: tests/persistent_cases.py).

Seven kernels walk a batch with `for (q = blockIdx.x; q < N; q += gridDim.x)`: a workgroup that finishes problem q goes on to q + grid
with the same LDS, the same flag words and -- in the scratch tiers -- the same slab of HBM.  Every kernel here is deterministic per
problem, so the criterion needs no tolerance: what a workgroup computes for a problem it takes SECOND (or third) equals, as bit
patterns, what a workgroup computes for the same problem taken FIRST.  The first-trip run is
  - the adjoint, the refinement, the elimination: the batch of the later-trip problems alone (eight problems, one per workgroup);
  - the solve kernels: the same batch with a workgroup per problem (DAQP_AMD_WG_GRID / DAQP_AMD_WG_TIER_GRID unset).
Every test establishes the grid of the launch from what the library reports -- the plan of a solve (daqp_batch_describe), the bytes of
per-workgroup scratch of a post-solve or elimination launch -- and asserts grid < N before it compares, and holds a handful of later-trip
problems to the bar its kernel family already has (imported from that family's test module), so that a kernel wrong in both runs
alike does not pass."""
import ctypes as C
import functools

import numpy as np
import pytest

import backward_soft_cases as S
import backward_state_cases as BS
import persistent_cases as P
import refine_cases as RC
import test_gpu_backward as TB
import test_gpu_backward_dual as TD
import test_gpu_eliminate as TE
import test_gpu_fast_mode as FM
import test_gpu_refine as TR
from oracle import oracle as O

pytestmark = pytest.mark.gpu
KEYS = P.KEYS
SWITCHES = ("EXACT", "NO_RECHECK", "WG_GRID", "WG_TIER_GRID", "WG_TIER_MIN_BATCH", "WG_R0", "WG_INVERSE", "WG_CAPL", "NO_WG_TIER", "NO_WG")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def fields(fn, handle):
    buf = C.create_string_buffer(4096)
    assert fn(handle, buf, 4096) > 0
    return {k: int(v) for k, v in (t.split("=", 1) for t in buf.value.decode().split(" ") if "=" in t) if v.lstrip("-").isdigit()}


@pytest.fixture
def switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv("DAQP_AMD_" + k, raising=False)

    def set_(**kw):
        for k, v in kw.items():
            monkeypatch.setenv("DAQP_AMD_" + k, str(v))
    return set_


# ---- 1, 2: the adjoint and the refinement in their scratch tiers ------------------------------------------------------------------
def solved(q, shape, ns=0):
    """(model, result) of a batch of persistent_cases; the tiered launch of the solve is off so that batches of 520 and of 8 problems take
    the same solve path (its threshold is a batch size)"""
    import daqp_amd
    n, m, ms = shape
    settings = dict(zero_tol=P.ZERO_TOL, **(dict(rho_soft=S.RHO) if ns else {}))
    bm = daqp_amd.BatchModel(q["f"].shape[0], n, m, ms, ns, **settings)
    bm.setup(*[q[k] for k in KEYS])
    return bm, bm.solve()


def same_solver_state(big, tail, rb, rt):
    """what the post-solve kernels read of the solve is the same in both batches: iterate, flags, working sets in their order, R^-1"""
    for key in ("x", "lam", "exitflag", "iter"):
        assert bits_equal(rb[key][P.TAIL], rt[key]), key
    (nab, wsb), (nat, wst) = big.working_sets(), tail.working_sets()
    assert np.array_equal(nab[P.TAIL], nat)
    for j, k in enumerate(P.TAIL):
        assert np.array_equal(wsb[k, :nab[k]], wst[j, :nat[j]]), k
        assert all(bits_equal(a, b) for a, b in zip(big.read_ldp(int(k)), tail.read_ldp(j))), k
    return nab


def reached_the_loop(big, tail, before, lds_bytes, cap):
    """The library does not export the grid of a post-solve launch; it does count the scratch it allocates with the family's first
    call (daqp_batch_device_bytes), one slab per workgroup of the persistent grid, and with device-resident arguments that call
    allocates nothing else.  before: (device bytes of big, of tail) in front of that call.  Tier 2 and grid = 512 < N for the big
    batch, a workgroup per problem for the tail batch -- by the restated rule of persistent_cases AND by the bytes."""
    n = big.n
    slab = 8 * P.scratch_doubles(n, cap)
    assert P.pick_tier(n, cap, lds_bytes)[0] == 2
    grid_big, grid_tail = (big.device_bytes() - before[0]) / slab, (tail.device_bytes() - before[1]) / slab
    assert grid_big == P.persistent_grid(P.N, slab) == P.GRID < P.N, grid_big
    assert grid_tail == P.persistent_grid(len(P.TAIL), slab) == len(P.TAIL), grid_tail


def to_numpy(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def adversaries_did_their_part(status, na):
    assert status[P.K20] == P.SINGULAR and status[P.KINF] == -1, status[P.HEAD]
    others = np.setdiff1d(P.HEAD, [P.K20, P.KINF])
    assert not status[others].any() and not status[P.TAIL].any()
    assert na[others].min() > na[P.TAIL].max(), (na[P.HEAD], na[P.TAIL])      # stale rows lie beyond the new working set


@pytest.mark.parametrize("kind", ["primal", "dual", "soft"])
def test_adjoint_scratch_tier_second_trip(gpu_lib, switches, kind):
    """k_backward<256, false, false, SOFT, DUAL>: problems 512 ... 519 behind problems 0 ... 7 of the same workgroups"""
    import torch
    switches(NO_WG_TIER=1)
    soft = kind == "soft"
    ns = P.NS_MAX if soft else 0
    n, m, ms = P.ADJOINT_SHAPE
    q = P.adjoint_batch(soft)
    qt = P.subset(q, P.TAIL)
    g = np.random.default_rng(61).standard_normal((P.N, n))
    gl = np.random.default_rng(62).standard_normal((P.N, m)) if kind == "dual" else None
    big, rb = solved(q, P.ADJOINT_SHAPE, ns)
    tail, rt = solved(qt, P.ADJOINT_SHAPE, ns)
    na = same_solver_state(big, tail, rb, rt)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    before = big.device_bytes(), tail.device_bytes()
    ob = to_numpy(big.backward(dev(g), out="torch", grad_lam=dev(gl)))
    ot = to_numpy(tail.backward(dev(g[P.TAIL]), out="torch", grad_lam=None if gl is None else dev(gl[P.TAIL])))
    reached_the_loop(big, tail, before, P.backward_lds_bytes, n + ns + 1)
    adversaries_did_their_part(ob["status"], na)
    for key in ("dz", "dbupper", "dblower", "status") + (("qsoft", "usoft", "usoft_id") if soft else ()):
        assert bits_equal(ob[key][P.TAIL], ot[key]), key
    assert np.abs(ob["dz"][P.TAIL]).max(axis=1).min() > 0
    # the bar of the family on the later-trip problems
    if kind == "primal":
        TB._check(big, q, rb, g, ob, ms, only=P.TAIL)
    elif kind == "dual":
        TD._check(big, q, rb, g, gl, ob, ms, only=P.TAIL)
    else:
        _, ws = big.working_sets()
        for k in P.TAIL:
            W = ws[k, :na[k]]
            Cm = np.vstack([np.eye(n)[:ms], q["A"][k]])
            is_soft = ((q["sense"][k][W] & S.SOFT) != 0).astype(float)
            dz, dnu, qk, _ = S.dense_adjoint(q["H"][k], Cm, W, is_soft, S.RHO, g[k])
            scale = max(np.abs(dz).max(), np.abs(dnu).max())
            assert rb["exitflag"][k] in (1, 2) and ob["status"][k] == 0
            assert np.abs(ob["dz"][k] - dz).max() <= BS.TOL * scale and np.abs((ob["dbupper"][k] + ob["dblower"][k])[W] - dnu).max() <= BS.TOL * scale, k
            assert np.abs(ob["qsoft"][k][W] - qk * is_soft).max() <= BS.TOL * max(1.0, np.abs(qk).max()), k
    big.close()
    tail.close()


def test_refine_scratch_tier_second_trip(gpu_lib, switches):
    """k_refine<256, false, false> at the smallest n whose rows and Gram matrix leave LDS"""
    import torch
    switches(NO_WG_TIER=1, EXACT=0, NO_RECHECK=1)
    n, m, ms = P.REFINE_SHAPE
    assert P.pick_tier(n - 1, n, P.refine_lds_bytes)[0] == 1
    q = P.refine_batch()
    big, rb = solved(q, P.REFINE_SHAPE)
    tail, rt = solved(P.subset(q, P.TAIL), P.REFINE_SHAPE)
    na = same_solver_state(big, tail, rb, rt)
    dev = lambda r: {key: torch.from_numpy(r[key]).cuda() for key in ("x", "lam", "fval")}
    before = big.device_bytes(), tail.device_bytes()
    ob = to_numpy(big.refine(dev(rb)))
    ot = to_numpy(tail.refine(dev(rt)))
    reached_the_loop(big, tail, before, P.refine_lds_bytes, n + 1)
    adversaries_did_their_part(ob["status"], na)
    for key in ("x", "lam", "fval", "status", "steps", "residual_before", "residual_after"):
        assert bits_equal(ob[key][P.TAIL], ot[key]), key
    # the bar of tests/test_gpu_refine.py::test_planted_cases_reach_the_last_bits on the later-trip problems
    p = P.refine_problem(P.SMALL)
    x, lam, _, _, _ = RC.oracle_solution(O.Oracle(), p)
    xm, lm, _, _, _ = RC.refine_model(p, x, lam)
    bar = max(8.0 * RC.error(p, xm, lm), TR.FLOOR)
    e = TR.errors(p, {key: ob[key][P.TAIL] for key in ("x", "lam")})
    print("E after %.2e bar %.2e" % (e.max(), bar), "steps", ob["steps"][P.TAIL], "mu %.2e -> %.2e" % (ob["residual_before"][P.TAIL].max(), ob["residual_after"][P.TAIL].max()))
    assert (e <= bar).all(), (e.max(), bar)
    assert (ob["residual_after"][P.TAIL] <= ob["residual_before"][P.TAIL]).all() and (ob["steps"][P.TAIL] <= 3).all()
    big.close()
    tail.close()


# ---- 3: the elimination's reduction kernel, workgroup tier --------------------------------------------------------------------------
def eliminated(b):
    """eliminate only (no reduced setup, no solve): flags, basis, reduced problem and the bytes the handle holds"""
    import daqp_amd
    n, neq, m, ms = b["shape"]
    em = daqp_amd.EliminatedBatchModel(b["f"].shape[0], n, m, ms, b["eq_rows"])
    em.eliminate(*[b[k] for k in KEYS])
    em._read_flags()
    out = dict(flags=em.flags, basis=em.basis(), red=em.reduced_problem(), bytes=int(daqp_amd.lib().daqp_batch_elimination_bytes(em._el)))
    em.close()
    return out


def elim_bytes_without_scratch(Nq, n, neq, m, ms):
    """what daqp_batch_eliminate allocates for host-resident QPs with a sense array, but for the workgroup tier's scratch: the row lists,
    the copies of H, A, sense, f and the bounds, V (row stride n | 1), beta, rd, rn, x0, c0, the flags and the reduced problem"""
    nr, mr, mA = n - neq, m - neq, m - ms
    doubles = Nq * (n * n + mA * n + n + 2 * m + neq * (n | 1) + 3 * neq + n + 1 + nr * nr + nr + mr * nr + 2 * mr)
    ints = neq + mr + Nq * m + Nq + Nq * mr
    return 8 * doubles + 4 * ints


@pytest.mark.parametrize("i", range(len(P.ELIM_SHAPES)), ids=[str(s) for s in P.ELIM_SHAPES])
def test_elimination_workgroup_tier_second_trip(gpu_lib, i):
    """k_eliminate<NV, 4>: the n x n scratch matrix, the reflectors in LDS and the -6 / -8 paths of a workgroup's first problem"""
    b = P.elim_batch(i)
    n, neq, m, ms = b["shape"]
    bt = dict(P.subset(b, P.TAIL), shape=b["shape"], eq_rows=b["eq_rows"])
    big, tail = eliminated(b), eliminated(bt)
    # the grid is not exported; the handle's bytes are, and what is not the per-workgroup n x n scratch is known
    assert n > 64
    assert (big["bytes"] - elim_bytes_without_scratch(P.N, *b["shape"])) / (8 * n * n) == P.persistent_grid(P.N, 8 * n * n) == P.GRID < P.N
    assert (tail["bytes"] - elim_bytes_without_scratch(len(P.TAIL), *b["shape"])) / (8 * n * n) == len(P.TAIL)
    want = np.ones(P.N, np.int32)
    want[P.K6], want[P.K8] = -6, -8
    assert np.array_equal(big["flags"], want) and np.array_equal(tail["flags"], want[P.TAIL])
    for key in ("x0", "Z", "c0"):
        assert bits_equal(big["basis"][key][P.TAIL], tail["basis"][key]), key
    for key in KEYS:
        assert bits_equal(big["red"][key][P.TAIL], tail["red"][key]), key
    # the bar of tests/test_gpu_eliminate.py::test_algebra_against_the_devices_own_basis on three later-trip problems
    floor = n * 2.0 ** -52
    for k in P.TAIL[[0, 3, 7]]:
        p = {key: b[key][k] for key in KEYS}
        dev = TE.defects(p, ms, b["eq_rows"], big["basis"]["x0"][k], big["basis"]["Z"][k], big["basis"]["c0"][k],
                         {key: big["red"][key][k] for key in ("H", "f", "A", "bupper", "blower")})
        ref = TE.EC.eliminate(p["H"], p["f"], p["A"], p["bupper"], p["blower"], p["sense"], ms, b["eq_rows"], dtype=np.float64)
        refd = TE.defects(p, ms, b["eq_rows"], ref["x0"], ref["Z"], ref["c0"], ref)
        for key in dev:
            assert dev[key] <= max(8.0 * refd[key], floor), (k, key, dev[key], refd[key])


# ---- 4 - 6: the workgroup solve kernel ----------------------------------------------------------------------------------------------
def run_solves(q, shape):
    """cold solve, then update(f) + warm solve, under the environment of the moment: everything the comparison reads"""
    import daqp_amd
    n, m, ms, _ = shape
    bm = daqp_amd.BatchModel(P.SOLVE_N, n, m, ms)
    plan = fields(daqp_amd.lib().daqp_batch_describe, bm._h)
    bm.enable_trace(4096)
    bm.setup(q["H"], q["f"], q["A"], q["bupper"], q["blower"])
    out = dict(plan=plan)
    for step in ("cold", "warm"):
        if step == "warm":
            bm.update(f=q["f2"])
        r = bm.solve()
        na, ws = bm.working_sets()
        out[step] = dict(r, na=na, ws=ws, trace=bm.read_trace(marks=True))
    bm.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle_solves(shape, seed):
    """the oracle on the later-trip problems 8 ... 23: (x, lam, fval, flag, iter, trace) per step and problem"""
    n, m, ms, _ = shape
    q = P.solve_batch(shape, seed)
    ora = O.Oracle()
    out = dict(cold=[], warm=[])
    for k in range(P.SOLVE_GRID, P.SOLVE_N):
        om = ora.model(n, m, ms)
        assert om.setup(q["H"][k], q["f"][k], q["A"][k], q["bupper"][k], q["blower"][k], None) == 1
        for step in ("cold", "warm"):
            if step == "warm":
                assert om.update(O.UPDATE_v, f=q["f2"][k]) == 0
            om.enable_trace()
            out[step].append(om.solve() + (om.get_trace(marks=True),))
    return out


def differences(ra, rb, key):
    """per problem whose `key` differs: (problem, exit flag, iterations of either run, rows of its working set, entries that differ,
    the largest difference)"""
    d = (ra[key] != rb[key]).reshape(P.SOLVE_N, -1)
    return [(int(k), int(ra["exitflag"][k]), int(ra["iter"][k]), int(rb["iter"][k]), int(ra["na"][k]), int(d[k].sum()),
             float(np.abs(ra[key][k] - rb[key][k]).max())) for k in np.flatnonzero(d.any(axis=1))]


def compare_solves(shape, seed, a, b, exact, grid_key="wg_grid"):
    """a: the persistent run (grid 8), b: a workgroup per problem; then the later-trip problems of a against the oracle"""
    assert a["plan"]["use_wg"] == b["plan"]["use_wg"] == 1
    assert a["plan"][grid_key] == P.SOLVE_GRID < P.SOLVE_N and b["plan"][grid_key] == P.SOLVE_N, (a["plan"], b["plan"])
    ref = oracle_solves(shape, seed)
    for step in ("cold", "warm"):
        ra, rb = a[step], b[step]
        for key in ("x", "lam", "fval", "exitflag", "iter", "soft_slack", "na"):
            assert bits_equal(ra[key], rb[key]), (step, key, differences(ra, rb, key))
        for k in range(P.SOLVE_N):
            assert np.array_equal(ra["trace"][k], rb["trace"][k]), (step, k)
            assert np.array_equal(ra["ws"][k, :ra["na"][k]], rb["ws"][k, :rb["na"][k]]), (step, k)
        assert ra["exitflag"][P.K_INF] == -1 and ra["iter"][P.K_INF] > 1, (step, ra["exitflag"][:8], ra["iter"][:8])      # the solve kernel's own verdict
        assert ra["exitflag"][P.K_EMPTY] == 1 and ra["na"][P.K_EMPTY] == 0, (step, ra["exitflag"][:8], ra["na"][:8])
        if step == "cold":
            assert ra["iter"][P.K_EMPTY] == 1
        for j, k in enumerate(range(P.SOLVE_GRID, P.SOLVE_N)):
            x, lam, fval, flag, it, trace = ref[step][j]
            assert ra["exitflag"][k] == flag == 1 and ra["iter"][k] == it, (step, k, ra["exitflag"][k], flag, ra["iter"][k], it)
            if exact:
                assert bits_equal(ra["x"][k], x) and bits_equal(ra["lam"][k], lam) and ra["fval"][k] == fval, (step, k)
                assert np.array_equal(ra["trace"][k], trace), (step, k)
            else:
                assert np.array_equal(np.sign(ra["lam"][k]), np.sign(lam)), (step, k)
                assert np.abs(ra["x"][k] - x).max() < FM.XTOL, (step, k)


@pytest.mark.parametrize("inverse", [None, "0"], ids=["inverse", "chains"])
@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("j", range(len(P.SOLVE_SHAPES)), ids=[str(s) for s in P.SOLVE_SHAPES])
def test_workgroup_solve_kernel_three_trips(gpu_lib, switches, j, exact, inverse):
    """k_ldp_wg with DAQP_AMD_WG_GRID=8 on 24 problems: every workgroup takes three, cold and warm"""
    shape, seed = P.SOLVE_SHAPES[j], 6500 + j
    q = P.solve_batch(shape, seed)
    switches(EXACT=int(exact), NO_RECHECK=1, **({} if inverse is None else dict(WG_INVERSE=inverse)))
    b = run_solves(q, shape)
    switches(WG_GRID=P.SOLVE_GRID)
    a = run_solves(q, shape)
    assert a["plan"]["wg_inverse"] == b["plan"]["wg_inverse"] and (inverse is None or a["plan"]["wg_inverse"] == 0)
    compare_solves(shape, seed, a, b, exact)


def test_tiered_launch_three_trips(gpu_lib, switches):
    """the tiered launch in front of a cold solve (most of every factor in the HBM tier) with DAQP_AMD_WG_TIER_GRID=8"""
    shape, seed = P.TIER_SHAPE, 6510
    q = P.solve_batch(shape, seed)
    switches(EXACT=0, NO_RECHECK=1, WG_TIER_MIN_BATCH=1, WG_R0=40)
    b = run_solves(q, shape)
    switches(WG_TIER_GRID=P.SOLVE_GRID)
    a = run_solves(q, shape)
    assert a["plan"]["wg_r0"] == b["plan"]["wg_r0"] == 40
    compare_solves(shape, seed, a, b, False, grid_key="wg_tier_grid")


def test_hand_over_behind_a_persistent_launch(gpu_lib, switches):
    """packed factor capped below the working sets of some problems of every trip: the problems the workgroup kernel flags are redone by
    k_ldp from their untouched state, whichever trip flagged them.  (The issue names the first shape of the solve cases; the planner
    leaves the workgroup kernel below a cap of 48 rows, which that shape's working sets never reach: persistent_cases.HAND_OVER_SHAPE.)"""
    shape, seed, capl = P.HAND_OVER_SHAPE, P.HAND_OVER_SEED, P.HAND_OVER_CAPL
    q = P.solve_batch(shape, seed)
    switches(EXACT=0, NO_RECHECK=1, WG_CAPL=capl)
    b = run_solves(q, shape)
    switches(WG_GRID=P.SOLVE_GRID)
    a = run_solves(q, shape)
    assert a["plan"]["wg_capL"] == b["plan"]["wg_capL"] == capl
    beyond = np.array([P.trace_peak(t) for t in a["cold"]["trace"]]) > capl
    for trip in range(P.SOLVE_N // P.SOLVE_GRID):
        part = beyond[trip * P.SOLVE_GRID:(trip + 1) * P.SOLVE_GRID]
        assert part.any() and not part.all(), (trip, beyond)
    compare_solves(shape, seed, a, b, False)
