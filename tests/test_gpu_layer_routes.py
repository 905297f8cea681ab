"""What a rho_soft tensor that requires grad receives on each route of qp_layer.  The routes differ here, and the difference is part of
the layer's behaviour: the default call gives it dl/drho_soft, a zero where the batch has no SOFT row; returns=(...) without
soft_returns leaves it without a gradient; soft_returns=True gives it dl/drho_soft again.  N = 4, n = 3, m = 4, ms = 2: the planted
batches of tests/backward_soft_cases.py at that size -- with seed 41 every problem ends SOFT_OPTIMAL with its one SOFT row (id 2, a
general row) active, which the test asserts on the GPU's own result."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("backward_soft_cases_for_routes", os.path.join(HERE, "backward_soft_cases.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)


def _inputs(soft):
    import torch
    q = S.planted_batch(4, 3, 2, 2, [2] if soft else [], seed=41)
    t = {k: torch.tensor(q[k], device="cuda", requires_grad=True) for k in ("H", "f", "A", "bupper", "blower")}
    rho = torch.tensor(S.RHO, dtype=torch.float64, device="cuda", requires_grad=True)
    return q, t, rho


def test_rho_soft_gradient_per_route(gpu_lib):
    import torch
    import daqp_amd
    from daqp_amd.layer import soft_gradient_terms
    # the default call on a batch without SOFT rows: a zero
    q, t, rho = _inputs(soft=False)
    x = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=q["ms"], rho_soft=rho)
    x.sum().backward()
    assert t["f"].grad.abs().max() > 0
    assert rho.grad is not None and rho.grad.shape == rho.shape and rho.grad.dtype == rho.dtype and float(rho.grad) == 0.0
    # returns=(...) without soft_returns: no gradient at all
    q, t, rho = _inputs(soft=False)
    x, lam = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=q["ms"], rho_soft=rho, returns=("x", "lam"))
    (x.sum() + lam.sum()).backward()
    assert t["f"].grad.abs().max() > 0 and rho.grad is None
    # soft_returns=True with an active SOFT row: drho of soft_gradient_terms on what backward_soft returns for the same gradients
    q, t, rho = _inputs(soft=True)
    sense, info = torch.tensor(q["sense"]), {}
    x, lam = daqp_amd.qp_layer(t["H"], t["f"], t["A"], t["bupper"], t["blower"], ms=q["ms"], sense=sense, rho_soft=rho, info=info,
                               returns=("x", "lam"), soft_returns=True)
    assert (info["exitflag"] == 2).all() and (lam[:, 2] != 0).all()
    gx, gl = torch.randn_like(x), torch.randn_like(lam)
    ((x * gx).sum() + (lam * gl).sum()).backward()
    assert not info["status"].any()
    bm = daqp_amd.BatchModel(4, 3, 4, q["ms"], 1, rho_soft=S.RHO)
    bm.setup(*(t[k].detach() for k in ("H", "f", "A", "bupper", "blower")), sense.cuda(), init_mask=daqp_amd.UPDATE_unconstrained)
    r = bm.solve(out="torch")
    assert torch.equal(r["lam"], lam.detach())
    o = bm.backward_soft(gx, gl, out="torch")
    want = soft_gradient_terms(r["lam"], o["dbupper"] + o["dblower"], o["qsoft"], o["usoft"], o["usoft_id"], S.RHO, q["ms"])["drho"].sum()
    assert float(want) != 0.0 and rho.grad is not None and rho.grad.shape == rho.shape
    assert float(rho.grad) == float(want), (float(rho.grad), float(want))
    bm.close()
