"""A batch of QPs as a differentiable torch operation (OptNet-style QP layer, learned condensed MPC).

    x = qp_layer(H, f, A, bupper, blower)          # (N, n), differentiable in H, f, A, bupper, blower

Forward is a BatchModel setup + solve on the inputs' device and current stream.  Backward is ONE daqp_batch_backward call -- the
adjoint system at the stored working set, on the factor the solve kept (include/daqp_amd.h) -- followed by a few torch
operations that form only the gradients somebody asked for:

    dl/df = -dz      dl/dH = -1/2 (dz x' + x dz')      dl/dA_i = -(lam_i dz + dnu_i x)'      dl/dbupper, dl/dblower = dbupper, dblower

Out of scope: soft constraints, problems that went through the proximal loop (singular H, LPs), gradients of lam or fval.
"""
import torch
from torch.autograd.function import once_differentiable

from .api import INF, UPDATE_unconstrained, BatchModel


class _QPLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, f, A, bupper, blower, ms, strict, info, settings):
        if not f.is_cuda:
            raise ValueError("qp_layer needs its inputs on the GPU")
        N, n = f.shape
        m = bupper.shape[1]
        shared = H.dim() == 2
        if A is not None and (A.dim() == 2) != shared:
            raise ValueError("H of shape (n, n) goes with A of shape (mA, n): one plant for the whole batch")
        mA = 0 if A is None else A.shape[-2]
        ms = m - mA if ms is None else int(ms)
        if ms + mA != m:
            raise ValueError(f"m = {m} bounds for ms = {ms} simple bounds and {mA} rows of A")
        c = lambda t: None if t is None else t.detach().to(torch.float64).contiguous()
        bl = torch.full_like(bupper, -INF).detach() if blower is None else blower
        with torch.cuda.device(f.device):      # the model takes that device's current stream
            bm = BatchModel(N, n, m, ms, 0, device=f.device.index, **settings)
            if shared:
                bm.setup_shared(c(H), c(f), c(A), c(bupper), c(bl))
            else:
                bm.setup(c(H), c(f), c(A), c(bupper), c(bl), init_mask=UPDATE_unconstrained)
            r = bm.solve(out="torch")
        ctx.bm, ctx.x, ctx.lam = bm, r["x"], r["lam"]
        ctx.ms, ctx.shared, ctx.strict, ctx.info = ms, shared, strict, info
        if info is not None:
            info["exitflag"] = r["exitflag"]
            info["lam"] = r["lam"]
        return r["x"].clone()      # (the kept copy is what backward multiplies with, whatever the caller does to its own)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_x):
        bm, x, lam, ms = ctx.bm, ctx.x, ctx.lam, ctx.ms
        with torch.cuda.device(x.device):
            o = bm.backward(grad_x.to(torch.float64).contiguous(), out="torch")
        status = o["status"]
        if ctx.info is not None:
            ctx.info["status"] = status
        if ctx.strict:
            badq = torch.nonzero(status).flatten()
            if badq.numel():
                q = int(badq[0])
                raise RuntimeError(f"qp_layer: {badq.numel()} of {bm.N} problems have no derivative (first: problem {q}, status "
                                   f"{int(status[q])}); strict=False gives them zero gradients")
        dz, dbu, dbl = o["dz"], o["dbupper"], o["dblower"]
        need = ctx.needs_input_grad
        gH = gf = gA = gbu = gbl = None
        if need[0]:
            gH = -0.5 * (dz[:, :, None] * x[:, None, :] + x[:, :, None] * dz[:, None, :])
            if ctx.shared:
                gH = gH.sum(0)
        if need[1]:
            gf = -dz
        if need[2]:
            lg, ng = lam[:, ms:], (dbu + dbl)[:, ms:]
            if ctx.shared:
                gA = -(lg.t() @ dz + ng.t() @ x)
            else:
                gA = -(lg[:, :, None] * dz[:, None, :] + ng[:, :, None] * x[:, None, :])
        if need[3]:
            gbu = dbu
        if need[4]:
            gbl = dbl
        return gH, gf, gA, gbu, gbl, None, None, None, None


def qp_layer(H, f, A, bupper, blower=None, ms=None, strict=True, info=None, **settings):
    """x* (N, n) of  min 1/2 x'Hx + f'x  s.t.  blower <= [x[:ms]; A x] <= bupper  for N problems, differentiable.

    H (N, n, n), f (N, n), A (N, mA, n) or None, bupper / blower (N, m) with m = ms + mA (ms defaults to m - mA; blower None =
    no lower bounds).  H of shape (n, n) together with A of shape (mA, n) is ONE plant for the whole batch (BatchModel.setup_shared);
    their gradients are then the sums over the batch.  **settings are DAQP settings (primal_tol=..., iter_limit=...).

    Backward raises if a problem has no derivative (it was not solved to optimality, it went through the proximal loop, or its
    active constraints are linearly dependent).  strict=False gives such problems zero gradients instead; pass info={} to read
    info["exitflag"] (after forward) and info["status"] (after backward), both (N,) int32 device tensors."""
    return _QPLayer.apply(H, f, A, bupper, blower, ms, strict, info, dict(settings))
