"""A batch of QPs as a differentiable torch operation (OptNet-style QP layer, learned condensed MPC).

    x = qp_layer(H, f, A, bupper, blower)                                  # (N, n), differentiable in H, f, A, bupper, blower
    x = qp_layer(H, f, A, bupper, blower, sense=sense, rho_soft=rho)       # rows with DAQP_SOFT in sense may be violated at a price

Forward is a BatchModel setup + solve on the inputs' device and current stream.  Backward is ONE daqp_batch_backward call
(daqp_batch_backward_soft when sense has SOFT rows) -- the adjoint system at the stored working set, on the factor the solve kept
(include/daqp_amd.h) -- followed by a few torch operations that form only the gradients somebody asked for:

    dl/df = -dz      dl/dH = -1/2 (dz x' + x dz')      dl/dA_i = -(lam_i dz + dnu_i x)'      dl/dbupper, dl/dblower = dbupper, dblower

Every route below ends in those torch operations, and they are written once: assemble_gradients (pure torch, any device, no
library) turns what a model's backward returned into (dH, df, dA, dbupper, dblower, drho).

An active SOFT row k sits at c_k x - b_k = rho_soft q_k lam_k, q_k = c_k H^-1 c_k': the system's (2,2) block is -S, S = diag(rho_soft
q_k), and since q_k depends on H and A their gradients gain a term each (soft_gradient_terms below; dsig_k = dnu_k lam_k, u_k = H^-1 c_k'):

    dl/drho_soft = sum_k dsig_k q_k      dl/dH -= rho_soft sum_k dsig_k u_k u_k'      dl/dA_i += 2 rho_soft dsig_i u_i'

Problems that went through the proximal loop (a positive semi-definite H, or H=None: an LP batch) have no factor of H to solve
that system on; qp_layer(..., nullspace=True) sends them through daqp_batch_backward_nullspace instead -- the null-space method on
the caller's own H: QR of the active rows, Cholesky of Z'HZ -- and the same formulas give the gradients (an LP has no dl/dH).  Such
a problem is differentiable where its optimum is locally unique: independent active rows (R_jj^2 >= zero_tol) and Z'HZ positive
definite (pivots > zero_tol max(1, max_i H_ii)); an LP must sit at a vertex.  n <= 64, no SOFT rows.

qp_layer(..., returns=("x", "lam", "fval")) also hands back the signed multipliers lam (N, m) and the optimal value fval (N,) as
differentiable tensors.  Backward is still ONE launch -- daqp_batch_backward_dual: the same system with g_lam on the working set in
the second block of its right-hand side -- and the formulas above, unchanged.  A gradient g_fval through fval = 1/2 x'Hx + f'x needs
no solve (envelope theorem) and is added in torch:

    dl/df += g_fval x      dl/dH += 1/2 g_fval x x'      dl/dbupper_i, dl/dblower_i += -g_fval lam_i (the row's side)      dl/dA_i += g_fval lam_i x'

qp_layer(..., eq_rows=[...]) names the equality rows of C = [first ms rows of I; A] (one ascending set for the batch, bupper == blower
there): forward is an EliminatedBatchModel -- the rows are eliminated on the device, the reduced batch solved, the result expanded --
and backward is ONE daqp_batch_eliminate_backward call: the KKT system of the full problem at its full working set, solved on the
factor of the equality rows and the factor of the reduced Hessian (include/daqp_amd.h).  The formulas above are unchanged.  Every
bound gradient of an equality row -- its multiplier gradient and the -g_fval lam term -- goes to bupper; blower gets zero there.

qp_layer(..., returns=(..., "soft_slack"), soft_returns=True) takes SOFT rows on that route and adds soft_slack (N,) = sum_k S_k lam_k^2
to the names; fval is then 1/2 x'Hx + f'x + 1/2 soft_slack.  Backward is ONE daqp_batch_backward_soft_dual launch: -S in the (2,2)
block and ghat_lam_k = g_lam_k + 2 g_slack rho_soft q_k lam_k (SOFT rows of W) in the second block of the right-hand side.  The
formulas are unchanged; the q_k-dependence terms take the wider

    dsig_k = dnu_k lam_k - 1/2 g_fval lam_k^2 + g_slack lam_k^2

(soft_slack depends on S_k directly; fval through the envelope theorem: dfval/dS_k = -1/2 lam_k^2).

Out of scope: per-row soft weights, proximal problems with n > 64 or
with SOFT rows, an LP with one shared A; with eq_rows: SOFT rows and one shared H / A.
"""
import torch
from torch.autograd.function import once_differentiable

from .api import INF, UPDATE_unconstrained, BatchModel, EliminatedBatchModel

SOFT = 8      # DAQP_SOFT (include/daqp_amd.h)


def soft_gradient_terms(lam, dnu, qsoft, usoft, usoft_id, rho_soft, ms, dsig_extra=None):
    """The terms that S = diag(rho_soft q_k), q_k = c_k H^-1 c_k', adds to the gradients of a batch with active SOFT rows, from what
    BatchModel.backward returns for it: lam (N, m) of the solve, dnu = dbupper + dblower (N, m), qsoft (N, m), usoft (N, ns, n),
    usoft_id (N, ns) (-1: unused slot).  Pure torch, any device.  Returns per problem

        dH   (N, n, n)       -rho_soft sum_k dsig_k u_k u_k'              add to -1/2 (dz x' + x dz')
        dA   (N, m - ms, n)  +2 rho_soft dsig_i u_i' on the SOFT general rows of W, zero elsewhere (a soft simple bound has c_k = e_k,
                             no row of A)                                  add to -(lam_i dz + dnu_i x)'
        drho (N,)            sum_k dsig_k q_k

    with dsig_k = dnu_k lam_k on the SOFT rows of W.  dsig_extra (N, m), optional: added to dnu lam there -- what a loss that depends on
    soft_slack or fval adds to dl/dS_k (g_slack lam_k^2 - 1/2 g_fval lam_k^2); read on the SOFT rows of W only."""
    N, ns, n = usoft.shape
    m = lam.shape[1]
    valid = usoft_id >= 0
    idx = usoft_id.clamp(min=0).long()
    dsig_all = dnu * lam if dsig_extra is None else dnu * lam + dsig_extra
    dsig = torch.gather(dsig_all, 1, idx) * valid                                    # (N, ns), working-set order
    su = (rho_soft * dsig)[:, :, None] * usoft                                        # rho dsig_k u_k
    dH = -torch.einsum("qsi,qsj->qij", su, usoft)
    general = (valid & (idx >= ms))[:, :, None]
    row = (idx - ms).clamp(min=0)[:, :, None].expand(N, ns, n)
    dA = torch.zeros((N, m - ms, n), dtype=usoft.dtype, device=usoft.device)
    if m > ms:
        dA.scatter_add_(1, row, 2.0 * su * general)
    drho = (dsig_all * qsoft).sum(1)                                                  # qsoft is zero off the SOFT rows of W
    return dict(dH=dH, dA=dA, drho=drho)


def assemble_gradients(x, lam, ms, o, status, need, shared=False, g_fval=None, g_slack=None, rho=0.0, eq=None):
    """(dH, df, dA, dbupper, dblower, drho) of a loss l(x, lam, fval, soft_slack) from the adjoint solution of ITS g_x, g_lam (and
    g_slack): the formulas of the module docstring, once for every route of qp_layer.  Pure torch, any device, no library.

        x (N, n), lam (N, m)   of the solve; ms: the number of simple bounds (rows ms.. of lam belong to A)
        o                      the dict a model's backward / backward_soft returned -- dz (N, n), dbupper, dblower (N, m) and, of a model
                               with SOFT rows, qsoft (N, m), usoft (N, ns, n), usoft_id (N, ns) -- or None: nothing was launched
        status (N,)            0, or why that problem has no derivative: g_fval and g_slack are zeroed there (o is zero there already)
        need                   six booleans, for H, f, A, bupper, blower, rho: what is not needed is not computed and comes back None
        shared                 one H (n, n) and one A (m - ms, n) for the batch: dH and dA are the sums over the batch
        g_fval, g_slack (N,)   dl/dfval, dl/dsoft_slack, or None
        rho                    rho_soft, the float
        eq                     index tensor of the equality rows of an eliminated batch: the -g_fval lam term of such a row goes to
                               dbupper whatever its sign, and dblower gets zero there

    In this order: the five formulas on o; the q_k-dependence terms of soft_gradient_terms with dsig_extra = g_slack lam^2 - 1/2 g_fval
    lam^2 (only where o has SOFT slots and H, A or rho is needed); the envelope terms of g_fval; the batch sum of a shared dH.  drho
    is the sum over the batch (rho_soft is one number), None when no q_k-dependence term was formed."""
    nH, nf, nA, nbu, nbl, nrho = need
    gH = gf = gA = gbu = gbl = grho = None
    add = lambda a, b: b if a is None else a + b
    ok = status == 0      # a problem without a derivative gets zero gradients from every term
    gv = None if g_fval is None else g_fval * ok
    if o is not None:
        dz, dbu, dbl = o["dz"], o["dbupper"], o["dblower"]
        soft = None
        if o.get("usoft") is not None and o["usoft"].shape[1] > 0 and (nH or nA or nrho):      # the q_k-dependence of S
            extra = None
            if g_slack is not None:
                extra = (g_slack * ok)[:, None] * lam * lam
            if gv is not None:
                extra = add(extra, -0.5 * gv[:, None] * lam * lam)
            soft = soft_gradient_terms(lam, dbu + dbl, o["qsoft"], o["usoft"], o["usoft_id"], rho, ms, dsig_extra=extra)
        if nH:
            gH = -0.5 * (dz[:, :, None] * x[:, None, :] + x[:, :, None] * dz[:, None, :])
            if soft is not None:
                gH = gH + soft["dH"]
        if nf:
            gf = -dz
        if nA:
            lg, ng = lam[:, ms:], (dbu + dbl)[:, ms:]
            gA = -(lg.t() @ dz + ng.t() @ x) if shared else -(lg[:, :, None] * dz[:, None, :] + ng[:, :, None] * x[:, None, :])
            if soft is not None:
                gA = gA + (soft["dA"].sum(0) if shared else soft["dA"])
        if nbu:
            gbu = dbu
        if nbl:
            gbl = dbl
        if nrho and soft is not None:
            grho = soft["drho"].sum()
    if gv is not None:
        if nH:
            gH = add(gH, 0.5 * gv[:, None, None] * x[:, :, None] * x[:, None, :])
        if nf:
            gf = add(gf, gv[:, None] * x)
        if nA:
            lg = gv[:, None] * lam[:, ms:]
            gA = add(gA, lg.t() @ x if shared else lg[:, :, None] * x[:, None, :])
        up, lo = lam.clamp(min=0.0), lam.clamp(max=0.0)      # lam_i > 0: the row sits at (or, SOFT, beyond) its upper bound;
        if eq is not None:
            up[:, eq], lo[:, eq] = lam[:, eq], 0.0            # an equality row: everything to bupper
        if nbu:
            gbu = add(gbu, -gv[:, None] * up)
        if nbl:
            gbl = add(gbl, -gv[:, None] * lo)
    if shared and gH is not None:
        gH = gH.sum(0)
    return gH, gf, gA, gbu, gbl, grho


def _backward_status(o, exitflag, info, strict):
    """status of a backward: the launch's, or -- nothing launched: the envelope terms exist wherever the solve ended optimal -- the exit
    flag with 1 turned into 0.  Written into info; strict raises on the first problem without a derivative."""
    status = o["status"] if o is not None else torch.where(exitflag == 1, torch.zeros_like(exitflag), exitflag)
    if info is not None:
        info["status"] = status
    if strict:
        badq = torch.nonzero(status).flatten()
        if badq.numel():
            q = int(badq[0])
            raise RuntimeError(f"qp_layer: {badq.numel()} of {status.numel()} problems have no derivative (first: problem {q}, status "
                               f"{int(status[q])}); strict=False gives them zero gradients")
    return status


def _prepare(H, f, A, bupper, blower, ms, sense, lp):
    """what forward checks and converts whatever model it builds: (N, n, m, ms, shared, ns_max, [H, f, A, bupper, blower] detached
    float64 contiguous, sense (N, m) int32 or None).  lp: H=None is an LP batch (it has no plant to share)."""
    if not f.is_cuda:
        raise ValueError("qp_layer needs its inputs on the GPU")
    N, n = f.shape
    m = bupper.shape[1]
    if H is None and lp:
        if A is not None and A.dim() == 2:
            raise ValueError("H=None (an LP batch) goes with A of shape (N, mA, n): a shared-plant LP is not supported")
        shared = False
    else:
        shared = H.dim() == 2
    if A is not None and H is not None and (A.dim() == 2) != shared:
        raise ValueError("H of shape (n, n) goes with A of shape (mA, n): one plant for the whole batch")
    mA = 0 if A is None else A.shape[-2]
    ms = m - mA if ms is None else int(ms)
    if ms + mA != m:
        raise ValueError(f"m = {m} bounds for ms = {ms} simple bounds and {mA} rows of A")
    c = lambda t: None if t is None else t.detach().to(torch.float64).contiguous()
    bl = torch.full_like(bupper, -INF).detach() if blower is None else blower
    ns_max = 0
    if sense is not None:
        sense = torch.as_tensor(sense).detach().to(device=f.device, dtype=torch.int32)
        if sense.dim() == 1:
            sense = sense.expand(N, m)
        if tuple(sense.shape) != (N, m):
            raise ValueError(f"sense must have shape {(N, m)} or {(m,)}")
        sense = sense.contiguous()
        ns_max = int(((sense & SOFT) != 0).sum(1).max())
    return N, n, m, ms, shared, ns_max, [c(H), c(f), c(A), c(bupper), c(bl)], sense


class _QPLayer(torch.autograd.Function):
    """every route of qp_layer.  route: "x" (the default call), "names" (returns=...), "soft" (soft_returns=True) or "eq" (eq_rows=...):
    it picks the model forward builds and the adjoint call backward makes; names: what forward returns, always as a tuple."""

    @staticmethod
    def forward(ctx, H, f, A, bupper, blower, rho_soft, ms, strict, info, settings, sense, nullspace, names, route, eq_rows):
        N, n, m, ms, shared, ns_max, arrays, sense = _prepare(H, f, A, bupper, blower, ms, sense, lp=nullspace or route == "eq")
        settings = dict(settings)
        if rho_soft is not None:
            settings["rho_soft"] = float(rho_soft)
        with torch.cuda.device(f.device):      # the model takes that device's current stream
            if route == "eq":
                model = EliminatedBatchModel(N, n, m, ms, eq_rows, 0, settings=settings, device=f.device.index)
                model.setup(*arrays, sense, init_mask=UPDATE_unconstrained)
            else:
                model = BatchModel(N, n, m, ms, ns_max, device=f.device.index, **settings)
                if shared:
                    model.setup_shared(*arrays, sense)
                else:
                    model.setup(*arrays, sense, init_mask=UPDATE_unconstrained)
            r = model.solve(out="torch")
        ctx.model, ctx.x, ctx.lam, ctx.exitflag = model, r["x"], r["lam"], r["exitflag"]
        ctx.rho = model._settings.rho_soft
        ctx.rho_like = rho_soft if isinstance(rho_soft, torch.Tensor) else None
        ctx.ms, ctx.shared, ctx.strict, ctx.info = ms, shared, strict, info
        ctx.nullspace, ctx.names, ctx.route = bool(nullspace), names, route
        ctx.eq = torch.as_tensor(model.eq_rows, dtype=torch.long, device=f.device) if route == "eq" else None
        if info is not None:
            info["exitflag"] = r["exitflag"]
            info["lam"] = r["lam"]
        ctx.set_materialize_grads(False)      # a gradient nobody sent stays None
        return tuple(r[k].clone() for k in names)      # (the kept copies are what backward multiplies with, whatever the caller does to its own)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        model, x, lam, route = ctx.model, ctx.x, ctx.lam, ctx.route
        g = dict(zip(ctx.names, grads))
        c = lambda t: None if t is None else t.to(torch.float64).contiguous()
        gx, gl, gv, gs = c(g.get("x")), c(g.get("lam")), c(g.get("fval")), c(g.get("soft_slack"))
        if model.ns == 0:      # soft_slack = 0: g_slack meets nothing
            gs = None
        none = (None,) * 15
        if gx is None and gl is None and gv is None and gs is None:
            return none
        o = None      # stays None when only fval carries a gradient: its terms need no solve
        with torch.cuda.device(x.device):
            if route == "soft":
                if gx is not None or gl is not None or gs is not None:
                    o = model.backward_soft(gx, gl, gs, lam if gs is not None else None, out="torch")
                elif model.ns > 0:      # g_fval alone: its dsig term still needs q_k and u_k
                    o = model.backward_soft(torch.zeros_like(x), out="torch")
            elif route == "eq":
                if gx is not None or gl is not None:
                    o = model.backward(gx, grad_lam=gl, out="torch", nullspace=ctx.nullspace)
            elif gl is not None:
                o = model.backward(gx, out="torch", nullspace=ctx.nullspace, grad_lam=gl)
            elif gx is not None:
                o = model.backward(gx, out="torch", nullspace=ctx.nullspace)
        status = _backward_status(o, ctx.exitflag, ctx.info, ctx.strict)
        need = ctx.needs_input_grad[:6]
        gH, gf, gA, gbu, gbl, grho = assemble_gradients(x, lam, ctx.ms, o, status, need, ctx.shared, gv, gs, ctx.rho, ctx.eq)
        if need[5] and route != "names":      # (returns=... without soft_returns leaves a rho_soft tensor without a gradient)
            like = ctx.rho_like
            grho = torch.zeros((), dtype=torch.float64, device=x.device) if grho is None else grho
            grho = grho.to(device=like.device, dtype=like.dtype).reshape(like.shape)
        else:
            grho = None
        return (gH, gf, gA, gbu, gbl, grho) + none[6:]


RETURNS = ("x", "lam", "fval")
SOFT_RETURNS = RETURNS + ("soft_slack",)


def qp_layer(H, f, A, bupper, blower=None, ms=None, strict=True, info=None, sense=None, rho_soft=None, nullspace=False, returns="x",
             eq_rows=None, soft_returns=False, **settings):
    """x* (N, n) of  min 1/2 x'Hx + f'x  s.t.  blower <= [x[:ms]; A x] <= bupper  for N problems, differentiable.

    H (N, n, n), f (N, n), A (N, mA, n) or None, bupper / blower (N, m) with m = ms + mA (ms defaults to m - mA; blower None =
    no lower bounds).  H of shape (n, n) together with A of shape (mA, n) is ONE plant for the whole batch (BatchModel.setup_shared);
    their gradients are then the sums over the batch.  **settings are DAQP settings (primal_tol=..., iter_limit=...).

    sense (N, m) or (m,) int32, not differentiable: the reference's sense bits per row; rows with DAQP_SOFT (8) may be violated, an
    active one sits rho_soft q_k lam_k beyond its bound (q_k = c_k H^-1 c_k').  The batch is created with ns_max = the largest number
    of SOFT rows of a problem.  rho_soft: a float or a 0-dim tensor (default: the DAQP setting, 1e-6); a tensor that requires grad
    receives dl/drho_soft summed over the batch.  info["exitflag"] holds 2 (DAQP_EXIT_SOFT_OPTIMAL) where a soft row is violated.

    Backward raises if a problem has no derivative (it was not solved to optimality, it went through the proximal loop, or its
    active constraints are linearly dependent).  strict=False gives such problems zero gradients instead; pass info={} to read
    info["exitflag"] (after forward) and info["status"] (after backward), both (N,) int32 device tensors.

    nullspace=True: backward is daqp_batch_backward_nullspace -- problems that went through the proximal loop are differentiated
    too (null-space method on H itself; n <= 64, no SOFT rows), every other problem as without it.  H may then be a positive
    semi-definite matrix, or None: an LP batch with per-problem A (N, mA, n) -- dl/dH is None, dl/df, dl/dA, dl/dbupper and
    dl/dblower come from the same formulas with the x and lam of the solve.  An LP is differentiable at a vertex only.

    returns: "x" (the default: x* alone), or one or several of "x", "lam", "fval" in any order -- ("x", "lam", "fval"), "fval", ... --
    for a tuple of differentiable tensors in that order (a single name other than "x" gives that one tensor): x (N, n), the signed
    multipliers lam (N, m) (> 0 at an upper bound, < 0 at a lower one, 0 off the working set) and fval (N,) = 1/2 x'Hx + f'x.
    Backward is one daqp_batch_backward_dual launch for the gradients through x and lam; the gradient through fval is added in
    torch without a solve.  With a gradient through fval alone nothing is launched and status is 0 wherever the solve ended
    optimal.  Not with SOFT rows, unless soft_returns=True.

    soft_returns=True: returns takes SOFT rows, and one more name: "soft_slack" (N,) = sum_k rho_soft q_k lam_k^2 over the active SOFT
    rows, from the solve's result; fval then is 1/2 x'Hx + f'x + 1/2 soft_slack, the optimal value of the penalised problem.  Backward
    is ONE daqp_batch_backward_soft_dual launch (g_lam and 2 g_slack rho_soft q_k lam_k in the second block of the right-hand side),
    the formulas above with dsig_k = dnu_k lam_k + g_slack lam_k^2 - 1/2 g_fval lam_k^2, and the envelope terms of g_fval; a rho_soft
    tensor receives dl/drho_soft as without it.  A single name, "x" included, gives that one tensor.  Not with nullspace or eq_rows.

    eq_rows: a list or array of equality rows of [first ms rows of I; A] -- ONE ascending set of 1 .. n-1 indices for the whole batch,
    bupper == blower there.  Forward goes through EliminatedBatchModel (the rows eliminated on the device, the reduced batch of n - neq
    variables solved, the result expanded), backward is one daqp_batch_eliminate_backward call; returns, strict, info and nullspace
    work as without it, nullspace being applied to the reduced problem (n - neq <= 64; H=None: an LP batch, differentiable at a vertex
    of the reduced problem).  info["status"] is the elimination flag (-6: dependent equality rows, -8: bupper != blower on one) where
    that is negative.  EVERY BOUND GRADIENT OF AN EQUALITY ROW GOES TO bupper -- the multiplier gradient dnu_E and the -g_fval lam_E
    term of a gradient through fval -- and blower gets zero there: an equality right-hand side that feeds both bounds receives their
    sum, which is its gradient.  Raises ValueError for H or A of one shared plant (2-D) and for SOFT rows.  Without eq_rows the layer
    is what it was."""
    has_soft = sense is not None and bool(((torch.as_tensor(sense) & SOFT) != 0).any())
    route = "soft" if soft_returns else "eq" if eq_rows is not None else "x" if isinstance(returns, str) and returns == "x" else "names"
    if route == "soft":
        if eq_rows is not None or nullspace:
            raise ValueError("qp_layer: soft_returns=True goes with neither eq_rows nor nullspace: SOFT rows are refused on both routes")
    elif route == "eq":
        if has_soft:
            raise ValueError("qp_layer: eq_rows does not take SOFT rows: a SOFT kept row is weighted by the reduced q_k")
        if (H is not None and H.dim() == 2) or (A is not None and A.dim() == 2):
            raise ValueError("qp_layer: eq_rows does not take one shared H / A: the elimination needs H (N, n, n) and A (N, mA, n)")
        if rho_soft is not None:
            raise ValueError("qp_layer: eq_rows does not take rho_soft: there are no SOFT rows to weigh")
    elif nullspace and has_soft:
        raise ValueError("qp_layer: nullspace=True does not take SOFT rows")
    names = (returns,) if isinstance(returns, str) else tuple(returns)
    allowed = SOFT_RETURNS if route == "soft" else RETURNS
    if not names or len(set(names)) != len(names) or any(k not in allowed for k in names):
        if route == "soft":
            raise ValueError(f'qp_layer: returns must be distinct names out of {SOFT_RETURNS} with soft_returns=True (got {returns!r})')
        raise ValueError(f'qp_layer: returns must be "x" or distinct names out of {RETURNS} (got {returns!r})')
    if route == "names" and has_soft:
        raise ValueError('qp_layer: returns other than "x" does not take SOFT rows: their multipliers and objective are not differentiated')
    out = _QPLayer.apply(H, f, A, bupper, blower, rho_soft, ms, strict, info, dict(settings), sense, nullspace, names, route, eq_rows)
    return out[0] if isinstance(returns, str) else out
