"""Host-side mirror of the reference's Python binding for the dense QP path, plus its batch twin.

  solve(H, f, A, bupper, blower, sense, **settings)      reference daqp.pyx:68-221  -> daqp_quadprog
  Model().setup/solve/update                              reference daqp.pyx:222-572 -> setup_daqp /
                                                          daqp_solve / daqp_update_ldp
  solve_batch(...), BatchModel                            N problems of one shape -> daqp_batch_*

Everything goes through the C ABI of libdaqp_amd.so; torch tensors on the GPU are passed by
device pointer (no copy), numpy arrays are staged by the library.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (DAQPBatchCertificate, DAQPBatchProblem, DAQPBatchResult, DAQPProblem, DAQPResult, MEM_DEVICE, MEM_HOST,
                   c_double_p, c_int_p, default_settings, lib)

UPDATE_Rinv, UPDATE_M, UPDATE_v, UPDATE_d, UPDATE_sense = 1, 2, 4, 8, 16
UPDATE_unconstrained, UPDATE_eliminate = 64, 128
INF = 1e30
TRACE_MARK = 0x40000000
TRACE_PIVOT, TRACE_SINGULAR, TRACE_REFINE, TRACE_REFACTOR, TRACE_CYCLE_RESET = (TRACE_MARK + k for k in range(1, 6))

try:  # torch is plumbing only (device memory, streams); the package works on numpy without it
    import torch
except Exception:  # pragma: no cover
    torch = None


def _np64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _np32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_double_p)


def _ip(a):
    return None if a is None else a.ctypes.data_as(c_int_p)


# ---------------------------------------------------------------------------
# single problem: same call shape as the reference binding
# ---------------------------------------------------------------------------
def solve(H, f, A, bupper, blower=None, sense=None, **settings):
    """x, fval, exitflag, info = solve(H, f, A, bupper, blower, sense, primal_tol=..., iter_limit=...)
    info carries the reference binding's keys and, beyond them, 'soft_slack' (DAQPResult.soft_slack, which daqp.pyx does not pass on)."""
    H, f, A, bupper = _np64(H), _np64(f), _np64(A), _np64(bupper)
    n, m = f.size, bupper.size
    mA = A.shape[0] if (A is not None and A.ndim == 2) else 0
    blower = np.full(m, -INF) if blower is None else _np64(blower)
    sense = np.zeros(m, np.int32) if sense is None else _np32(sense)
    x, lam = np.empty(n), np.empty(m)
    qp = DAQPProblem(n, m, m - mA, _dp(H), _dp(f), _dp(A) if mA else None, _dp(bupper), _dp(blower), _ip(sense),
                     None, 0, 0)
    st = default_settings(**settings)
    res = DAQPResult(_dp(x), _dp(lam), 0, 0, 0, 0, 0, 0, 0)
    lib().daqp_quadprog(C.byref(res), C.byref(qp), C.byref(st))
    if res.exitflag == -8 and _lib.last_error():
        info_err = _lib.last_error()
    else:
        info_err = ""
    return x, res.fval, res.exitflag, {"solve_time": res.solve_time, "setup_time": res.setup_time,
                                       "iterations": res.iter, "nodes": res.nodes, "lam": lam, "soft_slack": res.soft_slack,
                                       "error": info_err}


class Model:
    """Persistent workspace (reference daqp.pyx:222-572): setup once, then solve / update / solve ..."""

    def __init__(self):
        self._ws = None
        self._keep = {}
        self._qp = None
        self._settings = default_settings()
        self.n = self.m = self.ms = 0

    def _problem(self):
        k = self._keep
        self._qp = DAQPProblem(self.n, self.m, self.ms, _dp(k["H"]), _dp(k["f"]), _dp(k.get("A")), _dp(k["bupper"]),
                               _dp(k["blower"]), _ip(k.get("sense")), None, 0, 0)
        return self._qp

    def setup(self, H, f, A, bupper, blower=None, sense=None, **settings):
        self._free()
        H, f, A, bupper = _np64(H), _np64(f), _np64(A), _np64(bupper)
        self.n, self.m = f.size, bupper.size
        mA = A.shape[0] if (A is not None and A.ndim == 2) else 0
        self.ms = self.m - mA
        blower = np.full(self.m, -INF) if blower is None else _np64(blower)
        sense = np.zeros(self.m, np.int32) if sense is None else _np32(sense)
        self._keep = dict(H=H, f=f, A=A if mA else None, bupper=bupper, blower=blower, sense=sense)
        self._settings = default_settings(**settings)
        self._ws = C.create_string_buffer(_lib.WORKSPACE_BYTES)
        C.c_void_p.from_buffer(self._ws, 224).value = C.addressof(self._settings)  # work->settings (borrowed)
        t = C.c_double(0)
        flag = lib().setup_daqp(C.byref(self._problem()), self._ws, C.byref(t))
        if flag < 0:
            self._ws = None
        return flag, t.value

    def settings(self, **kw):
        for k, v in kw.items():
            setattr(self._settings, k, v)
        return {k: getattr(self._settings, k) for k, _ in self._settings._fields_}

    def update(self, H=None, f=None, A=None, bupper=None, blower=None, sense=None):
        """daqp.pyx:513-571: the mask is built field by field -- one bit per array given, arrays of the wrong shape are ignored as
        the reference ignores them -- and handed to daqp_update_ldp as it is (utils.c:58-221 runs each bit's step on its own: a
        new A keeps the factor, a new sense keeps everything else, ...)."""
        if self._ws is None:
            raise RuntimeError("Model.update called before setup")
        n, m, mA = self.n, self.m, self.m - self.ms
        mask = 0
        if H is not None and np.shape(H) == (n, n):
            self._keep["H"] = _np64(H); mask |= UPDATE_Rinv
        if A is not None and np.shape(A) == (mA, n):
            self._keep["A"] = _np64(A); mask |= UPDATE_M
        if f is not None and np.size(f) == n:
            self._keep["f"] = _np64(f); mask |= UPDATE_v
        if bupper is not None and np.size(bupper) == m:
            self._keep["bupper"] = _np64(bupper); mask |= UPDATE_d
        if blower is not None and np.size(blower) == m:
            self._keep["blower"] = _np64(blower); mask |= UPDATE_d
        if sense is not None and np.size(sense) == m:
            self._keep["sense"] = _np32(sense); mask |= UPDATE_sense
        return lib().daqp_update_ldp(mask, self._ws, C.byref(self._problem()))

    def update_mask(self, mask, **arrays):
        """daqp_update_ldp(mask, ...) with an explicit mask (C callers' usage): `arrays` (H, f, A, bupper, blower, sense) replace
        what the problem descriptor points to, whatever the mask says."""
        if self._ws is None:
            raise RuntimeError("Model.update_mask called before setup")
        for k, v in arrays.items():
            if v is not None:
                self._keep[k] = _np32(v) if k == "sense" else _np64(v)
        return lib().daqp_update_ldp(int(mask), self._ws, C.byref(self._problem()))

    def solve(self):
        """x, fval, exitflag, info as solve(); info['soft_slack'] is an extension over the reference binding"""
        if self._ws is None:
            raise RuntimeError("Model.solve called before setup")
        x, lam = np.empty(self.n), np.empty(self.m)
        res = DAQPResult(_dp(x), _dp(lam), 0, 0, 0, 0, 0, 0, 0)
        lib().daqp_solve(C.byref(res), self._ws)
        return x, res.fval, res.exitflag, {"solve_time": res.solve_time, "setup_time": 0.0, "iterations": res.iter,
                                           "nodes": res.nodes, "lam": lam, "soft_slack": res.soft_slack}

    def reset(self):
        """daqp_deactivate_constraints + reset_daqp_workspace: the next solve starts from an empty working set on the LDP as it is."""
        if self._ws is None:
            raise RuntimeError("Model.reset called before setup")
        lib().daqp_deactivate_constraints(self._ws)
        lib().reset_daqp_workspace(self._ws)
        return self

    def _free(self):
        if self._ws is not None:
            C.c_void_p.from_buffer(self._ws, 224).value = None  # borrowed settings are not ours to free
            lib().free_daqp_workspace(self._ws)
            lib().free_daqp_ldp(self._ws)
            self._ws = None

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass


# ---------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------
def _is_torch(a):
    return torch is not None and isinstance(a, torch.Tensor)


def _ptr(a, dtype, keep):
    """(pointer, memory) of a numpy array or torch tensor, made contiguous and of the right dtype."""
    if a is None:
        return None, None
    if _is_torch(a):
        tdt = torch.float64 if dtype == np.float64 else torch.int32
        t = a.to(tdt).contiguous()
        keep.append(t)
        return t.data_ptr(), (MEM_DEVICE if t.is_cuda else MEM_HOST)
    arr = np.ascontiguousarray(a, dtype=dtype)
    keep.append(arr)
    return arr.ctypes.data, MEM_HOST


def _pointers(arrays):
    """pointers and the one memory side of (name, array, dtype) triples; what must stay referenced comes back by name"""
    keep, ptrs, mems = {}, [], set()
    for name, a, dt in arrays:
        tmp = []
        p, mem = _ptr(a, dt, tmp)
        ptrs.append(p)
        if mem is not None:
            mems.add(mem)
            keep[name] = tmp[0]
    if len(mems) > 1:
        raise ValueError("mix of host and device arrays in one call")
    return ptrs, (mems.pop() if mems else MEM_HOST), keep


def _problem_pointers(H, f, A, bupper, blower, sense):
    return _pointers((("H", H, np.float64), ("f", f, np.float64), ("A", A, np.float64), ("bupper", bupper, np.float64),
                      ("blower", blower, np.float64), ("sense", sense, np.int32)))


_Kit = collections.namedtuple("_Kit", "conv new ptr f64 i32 mem")


def _kit(out, device):
    """What a call needs to take inputs and make outputs on one side -- out='torch': tensors on `device` (a torch.device, or the index
    of a GPU), out='numpy': host arrays: conv(a) = a as a contiguous float64 array of that side (None stays None), new(shape, dtype),
    ptr(a) = its address (None stays None), the two dtypes f64 and i32, and the library's memory tag."""
    if out == "torch":
        dev = device if isinstance(device, torch.device) else torch.device("cuda", device)
        return _Kit(lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float64, device=dev).contiguous(),
                    lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev),
                    lambda a: None if a is None else a.data_ptr(), torch.float64, torch.int32, MEM_DEVICE)
    return _Kit(lambda a: None if a is None else np.ascontiguousarray(a.detach().cpu().numpy() if _is_torch(a) else a, dtype=np.float64),
                lambda shape, dtype: np.empty(shape, dtype),
                lambda a: None if a is None else a.ctypes.data, np.float64, np.int32, MEM_HOST)


_RESULT_KEYS = ("x", "lam", "fval", "soft_slack", "exitflag", "iter")


def _result(N, n, m, out, device):
    """(the result dict of a solve of N problems, unfilled, and the DAQPBatchResult that points into it)"""
    k = _kit(out, device)
    o = dict(x=k.new((N, n), k.f64), lam=k.new((N, m), k.f64), fval=k.new((N,), k.f64), soft_slack=k.new((N,), k.f64),
             exitflag=k.new((N,), k.i32), iter=k.new((N,), k.i32))
    return o, DAQPBatchResult(*[k.ptr(o[key]) for key in _RESULT_KEYS], k.mem, 0, 0)


_BW_KEYS = ("dz", "dbupper", "dblower", "qsoft", "usoft", "usoft_id")


def _adjoint(model, out, entry, handles, ins, soft=False, which=None):
    """One adjoint call for BatchModel and EliminatedBatchModel: entry(*handles, inputs, outputs, status[, which], memory).  ins: (name,
    array or None, shape) per input, converted to the side of `out` and checked by name; outputs dz, dbupper, dblower and status are
    allocated, and qsoft, usoft, usoft_id with them where soft is set.  Returns the dict of outputs; the model keeps inputs and outputs
    alive, since the launch reads / writes them after this call has returned."""
    N, n, m, ns = model.N, model.n, model.m, model.ns
    k = _kit(out, model.device)
    arrays = [k.conv(a) for _, a, _ in ins]
    for (name, _, shape), a in zip(ins, arrays):
        if a is not None and tuple(a.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}")
    o = dict(dz=k.new((N, n), k.f64), dbupper=k.new((N, m), k.f64), dblower=k.new((N, m), k.f64), status=k.new((N,), k.i32))
    if soft:
        o.update(qsoft=k.new((N, m), k.f64), usoft=k.new((N, ns, n), k.f64), usoft_id=k.new((N, ns), k.i32))
    rc = getattr(lib(), entry)(*handles, *[k.ptr(a) for a in arrays], *[k.ptr(o[key]) for key in _BW_KEYS[:6 if soft else 3]], k.ptr(o["status"]),
                               *(() if which is None else (which,)), k.mem)
    if rc != 0:
        raise RuntimeError(f"{entry} failed ({rc}): {_lib.last_error()}")
    model._bw_keep = [arrays, o]
    return o


class BatchModel:
    """Device-resident workspaces of N QPs of one shape: setup -> solve -> {update(f, bounds) -> solve}*.

    Inputs may be numpy arrays (staged over PCIe by the library) or CUDA/HIP torch tensors (used in
    place; they must stay alive until the next setup/update replaces them).  Shapes: H (N,n,n),
    f (N,n), A (N,m-ms,n), bupper/blower (N,m), sense (N,m) int32 or None.
    """

    def __init__(self, N, n, m, ms=0, ns_max=0, device=None, **settings):
        self.N, self.n, self.m, self.ms, self.ns = N, n, m, ms, ns_max
        self._settings = default_settings(**settings)
        h = C.c_void_p()
        dev = -1 if device is None else int(device)
        rc = lib().daqp_batch_create(C.byref(h), N, n, m, ms, ns_max, C.byref(self._settings), dev)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_create failed ({rc}): {_lib.last_error()}")
        self._h = h
        self._keep = {}          # name -> array/tensor the device currently reads (one entry per input, replaced one by one)
        self._out_keep = []
        if torch is not None and torch.cuda.is_available():
            # the batch lives on ONE device: its launches go to that device's current stream and its outputs are allocated there
            self.device = torch.cuda.current_device() if device is None else int(device)
            lib().daqp_batch_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        else:
            self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().daqp_batch_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _problem(self, H=None, f=None, A=None, bupper=None, blower=None, sense=None):
        """DAQPBatchProblem of the given arrays.  Device arrays are used in place by the library (and bounds / f are read
        again by every later update and solve), so each one stays referenced under its own name until a later call
        replaces THAT array -- an update(f=...) must not drop the bounds adopted at setup."""
        ptrs, mem, keep = _problem_pointers(H, f, A, bupper, blower, sense)
        if mem == MEM_DEVICE:
            self._keep.update(keep)
        return DAQPBatchProblem(self.N, self.n, self.m, self.ms, *ptrs, mem), keep

    def setup(self, H, f, A, bupper, blower, sense=None, init_mask=0):
        p, keep = self._problem(H, f, A, bupper, blower, sense)
        rc = lib().daqp_batch_setup(self._h, C.byref(p), init_mask)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_setup failed ({rc}): {_lib.last_error()}")
        return self

    def setup_shared(self, H, f, A, bupper, blower, sense=None):
        """N problems with ONE H (n, n) and ONE A (m-ms, n) -- condensed MPC: same plant, per-problem f / bounds.
        Same result as Model.setup once (open bounds) followed by Model.update(f_k, bu_k, bl_k) per problem -- the reference's
        MPC usage; the factorisation runs once."""
        assert H.ndim == 2 and (A is None or A.ndim == 2), "setup_shared takes a single H and a single A"
        p, keep = self._problem(H, f, A, bupper, blower, sense)
        rc = lib().daqp_batch_setup_shared(self._h, C.byref(p), 0)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_setup_shared failed ({rc}): {_lib.last_error()}")
        return self

    def setup_flags(self):
        fl = np.zeros(self.N, np.int32)
        lib().daqp_batch_setup_flags(self._h, _ip(fl))
        return fl

    def update(self, f=None, bupper=None, blower=None, H=None, A=None, sense=None, mask=None):
        """daqp_update_ldp for every problem, the mask built field by field like Model.update (daqp.pyx:513-571): f -> v, bounds -> d
        (factors and working sets kept: the warm path), A -> M on the kept factor, H -> a new factor (v, M, d follow), sense ->
        the working sets are rebuilt from its ACTIVE bits.  mask: an explicit DAQP_UPDATE_* mask instead (sense=None with the
        sense bit means "all zeros", utils.c:85-86)."""
        if mask is None:
            mask = ((UPDATE_Rinv if H is not None else 0) | (UPDATE_M if A is not None else 0) | (UPDATE_v if f is not None else 0)
                    | (UPDATE_d if (bupper is not None or blower is not None) else 0) | (UPDATE_sense if sense is not None else 0))
        p, keep = self._problem(H, f, A, bupper, blower, sense)
        rc = lib().daqp_batch_update(self._h, int(mask), C.byref(p))
        if rc != 0:
            raise RuntimeError(f"daqp_batch_update failed ({rc}): {_lib.last_error()}")
        return self

    def solve(self, out="numpy"):
        """Returns dict(x, lam, fval, exitflag, iter, soft_slack); out='numpy' or 'torch' (device tensors)."""
        o, r = _result(self.N, self.n, self.m, out, self.device)
        rc = lib().daqp_batch_solve(self._h, C.byref(r))
        if rc != 0:
            raise RuntimeError(f"daqp_batch_solve failed ({rc}): {_lib.last_error()}")
        self._out_keep = [o]
        return o

    def backward(self, grad_x, out="torch", nullspace=False, grad_lam=None):
        """The adjoint of the last solve (daqp_batch_backward, include/daqp_amd.h): for grad_x = dl/dx of shape (N, n) returns
        dict(dz, dbupper, dblower, status) with dl/df = -dz, dl/dH = -1/2 (dz x' + x dz'), dl/dA_i = -(lam_i dz + dnu_i x)' on the
        general rows of the working set (dnu = dbupper + dblower), dl/dbupper = dbupper, dl/dblower = dblower.  status (N,) int32:
        0, or why that problem has no derivative (its outputs are zero then).  out='torch': device tensors, grad_x a device tensor,
        nothing waits for the device; out='numpy': host arrays.  Raises unless the last operation on the batch was a successful
        solve().  A model created with ns_max > 0 goes through daqp_batch_backward_soft: soft rows of the working set enter the
        system with rho_soft q_k in its (2,2) block, and the dict also holds qsoft (N, m): q_k = c_k H^-1 c_k' on those rows, usoft
        (N, ns_max, n): u_k = H^-1 c_k' per soft row of the working set, and usoft_id (N, ns_max) int32: their row ids, -1 for unused
        slots -- what the q_k-dependence terms of dl/dH, dl/dA and dl/drho_soft are made of (daqp_amd.layer.soft_gradient_terms).

        nullspace=True: daqp_batch_backward_nullspace with which = 0 -- problems that went through the proximal loop (singular H,
        LPs; status -8 otherwise) get their adjoint from the null-space kernel on the caller's own H, every other problem comes
        out bit for bit as without it.  nullspace="all": which = 1, every problem through that kernel.  n <= 64 ("all" is refused
        beyond, True leaves the -8), ns_max == 0, and H / A given as device tensors must still be alive and unchanged.

        grad_lam (N, m) = dl/dlam with respect to the signed multipliers of the solve: daqp_batch_backward_dual -- the same system
        with grad_lam on the working set in the second block of its right-hand side, the same outputs and the same formulas.
        grad_x may then be None (= 0).  nullspace selects its `which` (False: -1, True: 0, "all": 1); ns_max == 0 only (a model with soft
        rows: backward_soft below).  Without grad_lam the calls above are made, unchanged."""
        N, n, m, ns = self.N, self.n, self.m, self.ns
        if nullspace not in (False, True, "all"):
            raise ValueError('nullspace must be False, True or "all"')
        gx = ("grad_x", grad_x, (N, n))
        if grad_lam is not None:
            return _adjoint(self, out, "daqp_batch_backward_dual", (self._h,), (gx, ("grad_lam", grad_lam, (N, m))),
                            which=-1 if nullspace is False else (1 if nullspace == "all" else 0))
        if nullspace:      # (the entry refuses ns_max > 0 itself)
            return _adjoint(self, out, "daqp_batch_backward_nullspace", (self._h,), (gx,), which=1 if nullspace == "all" else 0)
        return _adjoint(self, out, "daqp_batch_backward" if ns == 0 else "daqp_batch_backward_soft", (self._h,), (gx,), soft=ns > 0)

    def backward_soft(self, grad_x=None, grad_lam=None, grad_slack=None, lam=None, out="torch"):
        """The adjoint of the last solve of a model with soft rows for a loss l(x, lam, fval, soft_slack)
        (daqp_batch_backward_soft_dual, include/daqp_amd.h): grad_x (N, n) = dl/dx, grad_lam (N, m) = dl/dlam, grad_slack (N,) =
        dl/dsoft_slack, each None for zero, not all three; lam (N, m): the multipliers solve() returned, needed with grad_slack.
        ONE system, K [dz; dnu] = [grad_x; ghat_lam on W] with -S in the (2,2) block of K and ghat_lam_k = grad_lam_k + 2 grad_slack
        rho_soft q_k lam_k on the SOFT rows of the working set.  Returns the dict of backward() on a soft model -- dz, dbupper,
        dblower, status, qsoft, usoft, usoft_id -- for the same formulas; the q_k-dependence terms take dsig_k = dnu_k lam_k +
        grad_slack lam_k^2 - 1/2 grad_fval lam_k^2 (daqp_amd.layer.soft_gradient_terms, dsig_extra).  Without grad_lam and grad_slack
        the result is that of backward(grad_x), bit for bit.  out='torch': device tensors in and out, nothing waits; out='numpy': host
        arrays."""
        N, n, m = self.N, self.n, self.m
        return _adjoint(self, out, "daqp_batch_backward_soft_dual", (self._h,), (("grad_x", grad_x, (N, n)), ("grad_lam", grad_lam, (N, m)),
                                                                               ("grad_slack", grad_slack, (N,)), ("lam", lam, (N, m))), soft=True)

    def certify(self, res, out=None):
        """certify_batch on the inputs this model reads (the device tensors given to setup / setup_shared / update, kept in place)
        and on res["x"], res["lam"] of a solve(): dict of the ten certificate arrays (daqp_certify_batch in include/daqp_amd.h).
        out: 'torch' or 'numpy' (default: what res holds).  One kernel on the current stream; nothing of the batch's state is read, so
        the call may come at any time after the solve.  A model set up from numpy arrays keeps no inputs: call certify_batch with them."""
        k = self._keep
        if "f" not in k or "bupper" not in k or "blower" not in k:
            raise ValueError("BatchModel.certify needs the device tensors of setup(); this model was set up from host arrays: use certify_batch")
        if out is None:
            out = "torch" if _is_torch(res["x"]) else "numpy"
        dev = k["f"].device
        x = torch.as_tensor(res["x"], dtype=torch.float64, device=dev)
        lam = torch.as_tensor(res["lam"], dtype=torch.float64, device=dev)
        o, keep = _certify(k.get("H"), k["f"], k.get("A") if self.m > self.ms else None, k["bupper"], k["blower"], x, lam, k.get("sense"), self.ms, out)
        self._cert_keep = keep      # the launch reads / writes them after this call has returned
        return o

    def refine(self, res, max_steps=3, out=None, nullspace=False):
        """Iterative refinement of res["x"], res["lam"] at the working set of the last solve() (daqp_batch_refine in
        include/daqp_amd.h: the algebra, the merit and the acceptance rule): dict(x, lam, fval, status, steps, residual_before,
        residual_after).  Works on copies: res itself is not modified.  status (N,) int32: 0, or why that problem was left as it came
        in (its residuals are NaN, its fval is res["fval"] where res has one, NaN otherwise).  residual_after <= residual_before
        for every problem with status 0.  out: 'torch' or 'numpy' (default: what res holds); device tensors stay on the device and
        nothing waits for it.  Raises unless the last operation on the batch was a successful solve(), for a model created with
        ns_max > 0 and for max_steps outside 1..8.  H, f, A and bounds given as device tensors must still be alive and unchanged.

        nullspace=True: daqp_batch_refine_nullspace with which = 0 -- problems that went through the proximal loop (singular H,
        LPs; status -8 otherwise) are refined by the null-space kernel on the caller's own H, every other problem comes out bit
        for bit as without it.  nullspace="all": which = 1, every problem through that kernel.  n <= 64 ("all" is refused beyond,
        True leaves the -8).  A problem whose optimum is not locally unique (an LP off a vertex) has status -20."""
        N, n, m = self.N, self.n, self.m
        if nullspace not in (False, True, "all"):
            raise ValueError('nullspace must be False, True or "all"')
        if out is None:
            out = "torch" if _is_torch(res["x"]) else "numpy"
        on_device = _is_torch(res["x"]) and res["x"].is_cuda
        fv = res.get("fval") if hasattr(res, "get") else None
        if on_device:
            dev = res["x"].device
            x = res["x"].to(torch.float64).contiguous().clone()
            lam = torch.as_tensor(res["lam"], dtype=torch.float64, device=dev).contiguous().clone()
            fval = torch.full((N,), float("nan"), dtype=torch.float64, device=dev) if fv is None else torch.as_tensor(fv, dtype=torch.float64, device=dev).contiguous().clone()
            resid = torch.empty((N, 2), dtype=torch.float64, device=dev)
            steps = torch.empty(N, dtype=torch.int32, device=dev)
            status = torch.empty(N, dtype=torch.int32, device=dev)
            ptrs = [t.data_ptr() for t in (x, lam, fval, resid, steps, status)]
            mem = MEM_DEVICE
        else:
            host = lambda a: a.detach().cpu().numpy() if _is_torch(a) else a
            x = np.array(host(res["x"]), dtype=np.float64, order="C")
            lam = np.array(host(res["lam"]), dtype=np.float64, order="C")
            fval = np.full(N, np.nan) if fv is None else np.array(host(fv), dtype=np.float64, order="C")
            resid = np.empty((N, 2))
            steps = np.empty(N, np.int32)
            status = np.empty(N, np.int32)
            ptrs = [a.ctypes.data for a in (x, lam, fval, resid, steps, status)]
            mem = MEM_HOST
        if tuple(x.shape) != (N, n) or tuple(lam.shape) != (N, m) or tuple(fval.shape) != (N,):
            raise ValueError(f"res must hold x of shape {(N, n)} and lam of shape {(N, m)}")
        if nullspace:
            entry = "daqp_batch_refine_nullspace"
            rc = lib().daqp_batch_refine_nullspace(self._h, *ptrs, int(max_steps), 1 if nullspace == "all" else 0, mem)
        else:
            entry = "daqp_batch_refine"
            rc = lib().daqp_batch_refine(self._h, *ptrs, int(max_steps), mem)
        if rc != 0:
            raise RuntimeError(f"{entry} failed ({rc}): {_lib.last_error()}")
        o = dict(x=x, lam=lam, fval=fval, status=status, steps=steps, residual_before=resid[:, 0], residual_after=resid[:, 1])
        self._rf_keep = o      # the launch reads / writes them after this call has returned
        if out == "torch":
            o = {k: (v if _is_torch(v) else torch.from_numpy(np.ascontiguousarray(v))) for k, v in o.items()}
        else:
            o = {k: (v.cpu().numpy() if _is_torch(v) else v) for k, v in o.items()}
        return o

    def reset(self):
        """Every problem back to an empty working set (daqp_deactivate_constraints + reset_daqp_workspace per problem): the next
        solve is a cold one on the LDPs as they are; an update(f, bounds) not yet applied stays pending."""
        rc = lib().daqp_batch_reset(self._h)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_reset failed ({rc}): {_lib.last_error()}")
        return self

    def set_primal_start(self, x):
        """api.c:636-641 for every problem: where the proximal iterations (singular H) start from; x: (N, n)."""
        keep = []
        ptr, mem = _ptr(x, np.float64, keep)
        rc = lib().daqp_batch_set_primal_start(self._h, ptr, mem)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_set_primal_start failed ({rc}): {_lib.last_error()}")
        return self

    def prox_info(self):
        """dict(n_prox, outer, eps): which problems go through the proximal outer loop (singular H), the outer
        iterations of the last solve and the shift of each factor."""
        npx, outer, eps = np.zeros(self.N, np.int32), np.zeros(self.N, np.int32), np.zeros(self.N)
        lib().daqp_batch_prox_info(self._h, _ip(npx), _ip(outer), eps.ctypes.data)
        return dict(n_prox=npx, outer=outer, eps=eps)

    def kernel_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        lib().daqp_batch_kernel_ms(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def working_sets(self):
        cap = self.n + self.ns + 1
        na, ws = np.zeros(self.N, np.int32), np.zeros((self.N, cap), np.int32)
        lib().daqp_batch_working_sets(self._h, _ip(na), _ip(ws))
        return na, ws

    def device_bytes(self):
        return int(lib().daqp_batch_device_bytes(self._h))

    def rechecked(self):
        """problems of the last solve whose INFEASIBLE verdict was re-derived in the reference's arithmetic (default mode, first
        solve after a setup: include/daqp_amd.h, daqp_batch_rechecked)"""
        return int(lib().daqp_batch_rechecked(self._h))

    def set_recheck(self, on):
        """switch the second pass of INFEASIBLE verdicts on / off for this batch (daqp_batch_set_recheck: off for a caller that
        recycles device-resident input buffers between setup and solve)"""
        lib().daqp_batch_set_recheck(self._h, 1 if on else 0)

    def recheck_ms(self):
        t = C.c_float(0)
        lib().daqp_batch_recheck_ms(self._h, C.byref(t))
        return t.value

    # test hooks
    def enable_trace(self, cap=4096):
        lib().daqp_batch_enable_trace(self._h, cap)
        self._trace_cap = cap

    def read_trace(self, marks=False):
        """Per problem: +(id+1) for an added constraint, -(id+1) for a removed one, in order.  marks=True keeps the branch
        markers as well (TRACE_PIVOT, TRACE_SINGULAR, TRACE_REFINE, TRACE_REFACTOR, TRACE_CYCLE_RESET)."""
        t = np.zeros((self.N, self._trace_cap), np.int32)
        lib().daqp_batch_read_trace(self._h, _ip(t))
        out = [t[q, : min(t[q, -1], self._trace_cap - 1)].copy() for q in range(self.N)]
        return out if marks else [e[e < TRACE_MARK] for e in out]

    def enable_profile(self, on=True):
        lib().daqp_batch_enable_profile(self._h, 1 if on else 0)

    def read_profile(self):
        """(N, 32) int64 per QP.  Solve kernel (register variant): cycles per state machine state [0:16] and
        visits [16:32]; setup kernel: cycles per phase [0:6]."""
        p = np.zeros((self.N, 32), np.int64)
        lib().daqp_batch_read_profile(self._h, p.ctypes.data_as(C.POINTER(C.c_longlong)))
        return p

    def read_ldp(self, q):
        n, m, ms = self.n, self.m, self.ms
        M, R, v = np.zeros((m - ms, n)), np.zeros(n * (n + 1) // 2), np.zeros(n)
        du, dl, sc = np.zeros(m), np.zeros(m), np.zeros(m)
        lib().daqp_batch_read_ldp(self._h, q, _dp(M), _dp(R), _dp(v), _dp(du), _dp(dl), _dp(sc))
        return M, R, v, du, dl, sc


class EliminatedBatchModel:
    """N QPs of one shape whose equality rows are eliminated on the device before they are solved (daqp_batch_eliminate in
    include/daqp_amd.h: the algebra): setup -> solve -> {update(f, bounds) -> solve}*, BatchModel's sequence and BatchModel's
    result dict, in the caller's full space.  eq_rows: the equality rows of C = [first ms rows of I; A], ONE ascending set of
    1 <= neq < n indices for the whole batch; bupper == blower is expected there.  The model owns the elimination handle and an
    inner BatchModel of the reduced shape (n - neq, m - neq, 0), exposed as .reduced (its working sets, prox_info, kernel_ms).
    .flags (N,) int32 after setup / update: 1, -6 (dependent equality rows) or -8 (bupper != blower on an equality row); such a
    problem comes back with that exit flag and zero x, lam -- the rest of the batch is untouched.  Inputs are numpy arrays (copied) or
    device tensors (used in place: they must stay alive and unchanged while the model is in use -- expansion reads H, f and A).
    settings: a dict of DAQP settings.  backward() is the adjoint of the full problem at its full working set (the equality rows and
    the active kept rows), solved on the two kept factors: qp_layer(..., eq_rows=...) is built on it.  Not built: refine through an
    eliminated model, the adjoint with SOFT rows (ns_max > 0), shared H / A, per-problem equality sets; basis() gives x0, Z, c0."""

    def __init__(self, N, n, m, ms, eq_rows, ns_max=0, settings=None, device=None):
        self.N, self.n, self.m, self.ms, self.ns = N, n, m, ms, ns_max
        self.eq_rows = np.ascontiguousarray(eq_rows, dtype=np.int32).ravel()
        neq = self.neq = int(self.eq_rows.size)
        if not 1 <= neq < n:
            raise ValueError(f"eq_rows must name 1 .. n-1 rows (got {neq}, n = {n})")
        if (self.eq_rows < 0).any() or (self.eq_rows >= m).any() or (np.diff(self.eq_rows) <= 0).any():
            raise ValueError("eq_rows must be distinct, ascending indices into 0..m-1")
        self.nr, self.mr = n - neq, m - neq
        self.kept_rows = np.setdiff1d(np.arange(m, dtype=np.int32), self.eq_rows)
        self._settings = default_settings(**(settings or {}))
        self.reduced = BatchModel(N, self.nr, self.mr, 0, ns_max, device=device, **(settings or {}))
        self.device = self.reduced.device
        # ONE stream for the handle and the reduced batch, taken here: eliminate / update / expand only enqueue with device-resident arrays,
        # and the reduced setup, update and solve are ordered against them by sitting on the same stream
        self._stream = None
        if torch is not None and torch.cuda.is_available():
            self._stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            lib().daqp_batch_set_stream(self.reduced._h, self._stream)
        self._el = None
        self._full = {}
        self._rp = None
        self.flags = None

    def close(self):
        if getattr(self, "_el", None):
            lib().daqp_batch_elimination_free(self._el)
            self._el = None
        if getattr(self, "reduced", None) is not None:
            self.reduced.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _read_flags(self):
        fl = np.zeros(self.N, np.int32)
        rc = lib().daqp_batch_elimination_flags(self._el, _ip(fl))
        if rc != 0:
            raise RuntimeError(f"daqp_batch_elimination_flags failed ({rc}): {_lib.last_error()}")
        self.flags = fl

    def setup(self, H, f, A, bupper, blower, sense=None, init_mask=0):
        self.eliminate(H, f, A, bupper, blower, sense)
        self.setup_reduced(init_mask)
        self._read_flags()
        return self

    def eliminate(self, H, f, A, bupper, blower, sense=None):
        """the first half of setup(): daqp_batch_eliminate alone (a new handle; follow with setup_reduced)"""
        ptrs, mem, keep = _problem_pointers(H, f, A if self.m > self.ms else None, bupper, blower, sense)
        p = DAQPBatchProblem(self.N, self.n, self.m, self.ms, *ptrs, mem)
        if self._el:
            lib().daqp_batch_elimination_free(self._el)
            self._el = None
        stream, dev = self._stream, -1 if self.device is None else int(self.device)
        h = C.c_void_p()
        rc = lib().daqp_batch_eliminate(C.byref(h), C.byref(p), _ip(self.eq_rows), self.neq, C.byref(self._settings), dev, stream)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_eliminate failed ({rc}): {_lib.last_error()}")
        self._el = h
        self._full = keep
        self._rp = DAQPBatchProblem()
        rc = lib().daqp_batch_elimination_problem(self._el, C.byref(self._rp))
        if rc != 0:
            raise RuntimeError(f"daqp_batch_elimination_problem failed ({rc}): {_lib.last_error()}")

    def setup_reduced(self, init_mask=0):
        """the second half of setup(): daqp_batch_setup of the inner model on the handle's reduced arrays"""
        rc = lib().daqp_batch_setup(self.reduced._h, C.byref(self._rp), init_mask)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_setup of the reduced batch failed ({rc}): {_lib.last_error()}")

    def update(self, f=None, bupper=None, blower=None, **other):
        """new f and / or bounds on the kept factor of the equality rows and the kept factors and working sets of the reduced batch:
        the warm path.  Anything else (H, A, sense) changes the factor: call setup."""
        if any(v is not None for v in other.values()):
            raise ValueError(f"EliminatedBatchModel.update takes f, bupper and blower only; for {sorted(other)} call setup again")
        if not self._el:
            raise RuntimeError("EliminatedBatchModel.update called before setup")
        ptrs, mem, keep = _pointers((("f", f, np.float64), ("bupper", bupper, np.float64), ("blower", blower, np.float64)))
        rc = lib().daqp_batch_eliminate_update(self._el, *ptrs, mem)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_eliminate_update failed ({rc}): {_lib.last_error()}")
        self._full.update(keep)
        mask = UPDATE_v | (UPDATE_d if (bupper is not None or blower is not None) else 0)      # (new bounds move x0, and with it f_r)
        rc = lib().daqp_batch_update(self.reduced._h, mask, C.byref(self._rp))
        if rc != 0:
            raise RuntimeError(f"daqp_batch_update of the reduced batch failed ({rc}): {_lib.last_error()}")
        self._read_flags()
        return self

    def solve(self, out="numpy"):
        """dict(x, lam, fval, exitflag, iter, soft_slack) in the full space: the keys and shapes of BatchModel.solve"""
        if not self._el:
            raise RuntimeError("EliminatedBatchModel.solve called before setup")
        return self.expand(self.reduced.solve(out=out), out)

    def expand(self, r, out="numpy"):
        """the second half of solve(): daqp_batch_expand of a result dict of .reduced.solve(out=out)"""
        k = _kit(out, self.device)
        o, fr = _result(self.N, self.n, self.m, out, self.device)
        rr = DAQPBatchResult(*[k.ptr(r[key]) for key in _RESULT_KEYS], k.mem, 0, 0)
        rc = lib().daqp_batch_expand(self._el, C.byref(rr), C.byref(fr))
        if rc != 0:
            raise RuntimeError(f"daqp_batch_expand failed ({rc}): {_lib.last_error()}")
        self._out_keep = [r, o]
        return o

    def reset(self):
        """the reduced batch back to empty working sets: the next solve is a cold one"""
        self.reduced.reset()
        return self

    def backward(self, grad_x, grad_lam=None, out=None, nullspace=False):
        """The adjoint of the last solve in the full space (daqp_batch_eliminate_backward, include/daqp_amd.h): for grad_x = dl/dx
        (N, n) and grad_lam = dl/dlam (N, m) -- either may be None (= 0), not both -- returns dict(dz, dbupper, dblower, status)
        with BatchModel.backward's meaning and formulas, x and lam being those of solve().  The multiplier gradient of an
        equality row comes back in dbupper (dblower is 0 there).  status (N,) int32: 0, the elimination flag (-6, -8) or why the
        reduced problem has no derivative; the outputs of such a problem are zero.  Gradients are numpy arrays or device tensors;
        out: 'torch' (device tensors, nothing waits for the device) or 'numpy' (default: what the gradients are).  nullspace
        (False, True, "all") selects `which` = -1, 0, 1 of the reduced adjoint: an LP batch or a singular H_r needs True, nr <= 64.
        Raises unless the last operation on the model was a successful solve(); models with ns_max > 0 are refused."""
        if not self._el:
            raise RuntimeError("EliminatedBatchModel.backward called before setup")
        if nullspace not in (False, True, "all"):
            raise ValueError('nullspace must be False, True or "all"')
        if grad_x is None and grad_lam is None:
            raise ValueError("grad_x and grad_lam are both None: there is nothing to differentiate")
        if out is None:
            out = "torch" if any(_is_torch(a) and a.is_cuda for a in (grad_x, grad_lam)) else "numpy"
        return _adjoint(self, out, "daqp_batch_eliminate_backward", (self._el, self.reduced._h),
                        (("grad_x", grad_x, (self.N, self.n)), ("grad_lam", grad_lam, (self.N, self.m))),
                        which=-1 if nullspace is False else (1 if nullspace == "all" else 0))

    def certify(self, res, out=None):
        """certify_batch on the caller's FULL problem and res["x"], res["lam"] of a solve()"""
        k = self._full
        if out is None:
            out = "torch" if _is_torch(res["x"]) else "numpy"
        x, lam = res["x"], res["lam"]
        if _is_torch(k["f"]) and k["f"].is_cuda:
            x = torch.as_tensor(x, dtype=torch.float64, device=k["f"].device)
            lam = torch.as_tensor(lam, dtype=torch.float64, device=k["f"].device)
        else:
            x = x.detach().cpu().numpy() if _is_torch(x) else x
            lam = lam.detach().cpu().numpy() if _is_torch(lam) else lam
        o, keep = _certify(k.get("H"), k["f"], k.get("A"), k["bupper"], k["blower"], x, lam, k.get("sense"), self.ms, out)
        self._cert_keep = keep
        return o

    def basis(self):
        """dict(x0 (N, n), Z (N, n, n - neq), c0 (N,)) as numpy arrays: x = x0 + Z y, fval = fval_r + c0"""
        if not self._el:
            raise RuntimeError("EliminatedBatchModel.basis called before setup")
        o = dict(x0=np.empty((self.N, self.n)), Z=np.empty((self.N, self.n, self.nr)), c0=np.empty(self.N))
        rc = lib().daqp_batch_elimination_basis(self._el, o["x0"].ctypes.data, o["Z"].ctypes.data, o["c0"].ctypes.data, MEM_HOST)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_elimination_basis failed ({rc}): {_lib.last_error()}")
        return o

    def reduced_problem(self):
        """the reduced arrays as numpy copies (daqp_batch_elimination_read): dict(H (None for an LP), f, A, bupper, blower, sense)"""
        if not self._el:
            raise RuntimeError("EliminatedBatchModel.reduced_problem called before setup")
        N, nr, mr = self.N, self.nr, self.mr
        o = dict(H=None if not self._rp.H else np.empty((N, nr, nr)), f=np.empty((N, nr)), A=np.empty((N, mr, nr)), bupper=np.empty((N, mr)),
                 blower=np.empty((N, mr)), sense=np.empty((N, mr), np.int32))
        rc = lib().daqp_batch_elimination_read(self._el, *[None if o[k] is None else o[k].ctypes.data for k in ("H", "f", "A", "bupper", "blower", "sense")], MEM_HOST)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_elimination_read failed ({rc}): {_lib.last_error()}")
        return o

    def device_bytes(self):
        return int(lib().daqp_batch_elimination_bytes(self._el)) + self.reduced.device_bytes()


def solve_batch(H, f, A, bupper, blower=None, sense=None, ms=None, out="numpy", eq_rows=None, **settings):
    """N x daqp_quadprog in one call (daqp_quadprog_batch semantics: unconstrained shortcut on).
    eq_rows: a list or array of equality rows (one set for the batch) sends the call through EliminatedBatchModel.

    Returns dict(x, lam, fval, exitflag, iter, soft_slack)."""
    N, n = f.shape[0], f.shape[1]
    m = bupper.shape[1]
    mA = A.shape[1] if A is not None and A.ndim == 3 else 0
    ms = m - mA if ms is None else ms
    if blower is None:
        blower = (torch.full_like(bupper, -INF) if _is_torch(bupper) else np.full(bupper.shape, -INF))
    if eq_rows is not None and N > 0:
        ns = 0
        if sense is not None:
            s = sense.cpu().numpy() if _is_torch(sense) else np.asarray(sense)
            ns = int(((s & 8) != 0).sum(axis=1).max()) if s.size else 0
        em = EliminatedBatchModel(N, n, m, ms, eq_rows, ns, settings=settings)
        try:
            em.setup(H, f, A, bupper, blower, sense, init_mask=UPDATE_unconstrained | UPDATE_eliminate)
            res = em.solve(out=out)
            if out == "torch":
                torch.cuda.synchronize()
        finally:
            em.close()
        return res
    if N == 0:   # an empty batch is a valid (empty) answer, as it is for daqp_quadprog_batch
        return _result(0, n, m, "torch", f.device)[0] if out == "torch" and _is_torch(f) else _result(0, n, m, "numpy", None)[0]
    ns = 0
    if sense is not None:
        s = sense.cpu().numpy() if _is_torch(sense) else np.asarray(sense)
        ns = int(((s & 8) != 0).sum(axis=1).max()) if s.size else 0
    bm = BatchModel(N, n, m, ms, ns, **settings)
    try:
        bm.setup(H, f, A, bupper, blower, sense, init_mask=UPDATE_unconstrained | UPDATE_eliminate)
        res = bm.solve(out=out)
        if out == "torch":
            torch.cuda.synchronize()
    finally:
        bm.close()
    return res


_CERT_REAL = ("stationarity", "stationarity_scale", "primal", "complementarity", "objective", "ray_residual", "ray_scale", "ray_support")
_CERT_INT = ("wrong_sign", "primal_row")


def _certify(H, f, A, bupper, blower, x, lam, sense, ms, out):
    """(dict of outputs, what the launch still reads or writes)"""
    if f.ndim != 2 or bupper.ndim != 2:
        raise ValueError("f must be (N, n) and bupper (N, m)")
    N, n, m = int(f.shape[0]), int(f.shape[1]), int(bupper.shape[1])
    mA = 0 if A is None else int(A.shape[-2])
    ms = m - mA if ms is None else int(ms)
    if mA != m - ms or (A is not None and int(A.shape[-1]) != n):
        raise ValueError("A must be (N, m - ms, n) or (m - ms, n)")
    shared = (H is None or H.ndim == 2) and (A is None or A.ndim == 2) and not (H is None and A is None)
    if not shared and ((H is not None and H.ndim != 3) or (A is not None and A.ndim != 3)):
        raise ValueError("H and A are either both per problem (3-d) or both shared (2-d)")
    for name, a, shape in (("H", H, (n, n) if shared else (N, n, n)), ("blower", blower, (N, m)), ("x", x, (N, n)), ("lam", lam, (N, m)),
                           ("sense", sense, (N, m))):
        if a is not None and tuple(a.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}")
    keep, mems, ptrs = [], set(), []
    for a, dt in ((H, np.float64), (f, np.float64), (A if mA else None, np.float64), (bupper, np.float64), (blower, np.float64),
                  (sense, np.int32), (x, np.float64), (lam, np.float64)):
        ptr, mem = _ptr(a, dt, keep)
        ptrs.append(ptr)
        if mem is not None:
            mems.add(mem)
    if len(mems) > 1:
        raise ValueError("mix of host and device arrays in one call")
    mem = mems.pop()
    stream, device = None, -1
    if mem == MEM_DEVICE:
        dev = keep[0].device
        device = dev.index
        o = {k: torch.empty(N, dtype=torch.float64, device=dev) for k in _CERT_REAL}
        o.update({k: torch.empty(N, dtype=torch.int32, device=dev) for k in _CERT_INT})
        cert = DAQPBatchCertificate(*[o[k].data_ptr() for k in _CERT_REAL + _CERT_INT])
        stream = torch.cuda.current_stream(dev).cuda_stream
    else:
        o = {k: np.empty(N) for k in _CERT_REAL}
        o.update({k: np.empty(N, np.int32) for k in _CERT_INT})
        cert = DAQPBatchCertificate(*[o[k].ctypes.data for k in _CERT_REAL + _CERT_INT])
    p = DAQPBatchProblem(N, n, m, ms, *ptrs[:6], mem)
    rc = lib().daqp_certify_batch(C.byref(cert), C.byref(p), ptrs[6], ptrs[7], 1 if shared else 0, device, stream)
    if rc != 0:
        raise RuntimeError(f"daqp_certify_batch failed ({rc}): {_lib.last_error()}")
    if out == "torch":
        o = {k: (v if _is_torch(v) else torch.from_numpy(v)) for k, v in o.items()}
    else:
        o = {k: (v.cpu().numpy() if _is_torch(v) else v) for k, v in o.items()}
    return o, keep


def certify_batch(H, f, A, bupper, blower, x, lam, sense=None, ms=None, out="numpy"):
    """The certificate of N (x, lam) pairs, computed on the GPU in twice the working precision (daqp_certify_batch in
    include/daqp_amd.h: definitions and the accuracy contract): dict of stationarity, stationarity_scale, primal, complementarity,
    objective, ray_residual, ray_scale, ray_support (float64, N each) and wrong_sign, primal_row (int32, N each).  Stateless: it
    certifies the answer of any solver.  numpy arrays (staged; the call waits) or device tensors (used in place; one kernel on the
    current stream, nothing waits unless out='numpy').  f (N, n), bupper / blower / lam / sense (N, m), x (N, n); H (N, n, n) with
    A (N, m - ms, n), or ONE H (n, n) with ONE A (m - ms, n) for all problems (shared structure); H=None: an LP.  A ray (ray_residual
    == 0, ray_support < 0) with weight on a SOFT row proves nothing."""
    o, _ = _certify(H, f, A, bupper, blower, x, lam, sense, ms, out)      # (out='numpy' has waited; a 'torch' result is ordered on the stream, and torch's allocator keeps freed inputs off other streams)
    return o


def minrep_batch(A, b, ms=None, out="numpy", info=None, device=None, **settings):
    """Redundant rows of P polyhedra {x : A[p] x <= b[p]} of one shape: A (P, m - ms, n), b (P, m) with the ms simple bounds
    x_i <= b_i first; numpy arrays or torch device tensors (used in place).  Returns int32 (P, m): 1 redundant, 0 not, -1 a vanishing
    row of A (not tested); out='torch' gives a device tensor.  All P * m row tests run as one batch on the GPU (daqp_minrep_batch in
    include/daqp_amd.h: rows are normalised first, an empty polyhedron gives all ones).  info: a dict that receives 'unresolved',
    the number of tests that ended with neither OPTIMAL nor INFEASIBLE (0 when every verdict is clean)."""
    if b.ndim != 2:
        raise ValueError("b must be (P, m)")
    P, m = int(b.shape[0]), int(b.shape[1])
    mA = 0 if A is None else int(A.shape[1])
    if ms is None:
        ms = m - mA
    if A is not None and (A.ndim != 3 or int(A.shape[0]) != P or mA != m - ms):
        raise ValueError("A must be (P, m - ms, n)")
    n = int(A.shape[2]) if A is not None else ms      # (simple bounds only: the rows are the first ms coordinates)
    keep = []
    pa, mem_a = _ptr(A, np.float64, keep)
    pb, mem_b = _ptr(b, np.float64, keep)
    if mem_a is not None and mem_a != mem_b:
        raise ValueError("mix of host and device arrays in one call")
    st = default_settings(**settings)
    if mem_b == MEM_DEVICE:
        dev = keep[-1].device
        red = torch.empty((P, m), dtype=torch.int32, device=dev)
        pr = red.data_ptr()
        device = dev.index if device is None else device
        torch.cuda.current_stream(dev).synchronize()      # the library works on its own stream: the inputs must be there
    else:
        red = np.empty((P, m), np.int32)
        pr = red.ctypes.data
    rc = lib().daqp_minrep_batch(pr, pa, pb, P, n, m, ms, mem_b, C.byref(st), -1 if device is None else int(device))
    if rc < 0:
        raise RuntimeError(f"daqp_minrep_batch failed ({rc}): {_lib.last_error()}")
    if info is not None:
        info["unresolved"] = int(rc)
    if out == "torch":
        return red if _is_torch(red) else torch.from_numpy(red)
    return red.cpu().numpy() if _is_torch(red) else red


def minrep(A, b):
    """daqp.pyx:636-652: redundant rows of {x : A x <= b}; ms = len(b) - A.shape[0] simple bounds come first in b.  int32 array of m."""
    A, b = _np64(A), _np64(b)
    A = A.reshape(-1, A.shape[-1]) if A.ndim >= 2 else A.reshape(0, b.size)
    m, mA, n = b.size, A.shape[0], A.shape[1]
    return minrep_batch(A[None] if mA else None, b[None], ms=m - mA)[0]


def solve_batch_multi(H, f, A, bupper, blower=None, sense=None, ms=None, devices=None, **settings):
    """solve_batch over several GPUs of this host: problem k on devices[k mod len(devices)] (daqp_quadprog_batch_multi: one host
    thread, stream and set of workspaces per shard, no exchange step).  numpy arrays in, numpy arrays out; devices=None: every
    visible device.  Returns dict(x, lam, fval, exitflag, iter, soft_slack)."""
    N, n = f.shape[0], f.shape[1]
    m = bupper.shape[1]
    mA = A.shape[1] if A is not None and A.ndim == 3 else 0
    ms = m - mA if ms is None else ms
    if blower is None:
        blower = np.full(bupper.shape, -INF)
    keep = []
    ptrs = [_ptr(a, dt, keep)[0] for a, dt in ((H, np.float64), (f, np.float64), (A if mA else None, np.float64), (bupper, np.float64),
                                                (blower, np.float64), (sense, np.int32))]
    p = DAQPBatchProblem(N, n, m, ms, *ptrs, MEM_HOST)
    o = dict(x=np.empty((N, n)), lam=np.empty((N, m)), fval=np.empty(N), soft_slack=np.empty(N),
             exitflag=np.empty(N, np.int32), iter=np.empty(N, np.int32))
    r = DAQPBatchResult(o["x"].ctypes.data, o["lam"].ctypes.data, o["fval"].ctypes.data, o["soft_slack"].ctypes.data,
                        o["exitflag"].ctypes.data, o["iter"].ctypes.data, MEM_HOST, 0, 0)
    st = default_settings(**settings)
    dev = None if devices is None else np.ascontiguousarray(devices, np.int32)
    rc = lib().daqp_quadprog_batch_multi(C.byref(r), C.byref(p), C.byref(st), _ip(dev), 0 if dev is None else dev.size)
    if rc != 0:
        raise RuntimeError(f"daqp_quadprog_batch_multi failed ({rc}): {_lib.last_error()}")
    return o


class MultiBatchModel:
    """N QPs of one shape held on several GPUs of this host between calls (include/daqp_amd.h, DAQPMultiBatch): problem k lives on
    devices[k mod G].  setup -> solve -> {update(f, bounds) -> solve}* with ONE host-resident batch in the caller's order, numpy in,
    numpy out -- BatchModel's sequence, sharded.  devices=None: every visible device; a device may be listed more than once."""

    def __init__(self, N, n, m, ms=0, ns_max=0, devices=None, **settings):
        self.N, self.n, self.m, self.ms = N, n, m, ms
        self._settings = default_settings(**settings)
        dev = None if devices is None else np.ascontiguousarray(devices, np.int32)
        h = C.c_void_p()
        rc = lib().daqp_batch_create_multi(C.byref(h), N, n, m, ms, ns_max, C.byref(self._settings), _ip(dev), 0 if dev is None else dev.size)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_create_multi failed ({rc}): {_lib.last_error()}")
        self._h = h
        self.shards = int(lib().daqp_batch_multi_shards(h))

    def close(self):
        if getattr(self, "_h", None):
            lib().daqp_batch_free_multi(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _problem(self, keep, H=None, f=None, A=None, bupper=None, blower=None, sense=None):
        mA = self.m - self.ms
        ptrs = [_ptr(a, dt, keep)[0] for a, dt in ((H, np.float64), (f, np.float64), (A if mA else None, np.float64), (bupper, np.float64),
                                                    (blower, np.float64), (sense, np.int32))]
        return DAQPBatchProblem(self.N, self.n, self.m, self.ms, *ptrs, MEM_HOST)

    def setup(self, H, f, A, bupper, blower=None, sense=None, init_mask=0):
        if blower is None:
            blower = np.full(np.shape(bupper), -INF)
        keep = []
        p = self._problem(keep, H, f, A, bupper, blower, sense)
        rc = lib().daqp_batch_setup_multi(self._h, C.byref(p), init_mask)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_setup_multi failed ({rc}): {_lib.last_error()}")

    def update(self, f=None, bupper=None, blower=None, H=None, A=None, sense=None, mask=None):
        """BatchModel.update, sharded: any mask of daqp_update_ldp (built field by field unless given)"""
        if mask is None:
            mask = ((UPDATE_Rinv if H is not None else 0) | (UPDATE_M if A is not None else 0) | (UPDATE_v if f is not None else 0)
                    | (UPDATE_d if (bupper is not None or blower is not None) else 0) | (UPDATE_sense if sense is not None else 0))
        keep = []
        p = self._problem(keep, H, f, A, bupper, blower, sense)
        rc = lib().daqp_batch_update_multi(self._h, int(mask), C.byref(p))
        if rc != 0:
            raise RuntimeError(f"daqp_batch_update_multi failed ({rc}): {_lib.last_error()}")

    def solve(self):
        N, n, m = self.N, self.n, self.m
        o = dict(x=np.empty((N, n)), lam=np.empty((N, m)), fval=np.empty(N), soft_slack=np.empty(N),
                 exitflag=np.empty(N, np.int32), iter=np.empty(N, np.int32))
        r = DAQPBatchResult(o["x"].ctypes.data, o["lam"].ctypes.data, o["fval"].ctypes.data, o["soft_slack"].ctypes.data,
                            o["exitflag"].ctypes.data, o["iter"].ctypes.data, MEM_HOST, 0, 0)
        rc = lib().daqp_batch_solve_multi(self._h, C.byref(r))
        if rc != 0:
            raise RuntimeError(f"daqp_batch_solve_multi failed ({rc}): {_lib.last_error()}")
        o["solve_time"] = r.solve_time
        return o

    # ---- per-shard descriptors (daqp_batch_*_multi_shards): shard g's problems back to back, host arrays or tensors ON shard g's device
    def _shard_problems(self, shards, names):
        P = (DAQPBatchProblem * self.shards)()
        keep = []
        for g, sh in enumerate(shards):
            _, sn, dev = self.shard(g)
            ptrs, mems = [], set()
            for name in ("H", "f", "A", "bupper", "blower", "sense"):
                a = sh.get(name) if name in names else None
                if name == "A" and self.m == self.ms:
                    a = None
                ptr, mem = _ptr(a, np.int32 if name == "sense" else np.float64, keep)
                ptrs.append(ptr)
                if mem is not None:
                    mems.add(mem)
            if len(mems) > 1:
                raise ValueError("mix of host and device arrays in one shard")
            P[g] = DAQPBatchProblem(sn, self.n, self.m, self.ms, *ptrs, mems.pop() if mems else MEM_HOST)
        return P, keep

    def setup_shards(self, shards, init_mask=0):
        """shards[g]: dict(H, f, A, bupper, blower[, sense]) of shard g's problems (problem k of the batch is problem k // G of shard
        k mod G), numpy or torch tensors resident on that shard's device (used in place)"""
        P, keep = self._shard_problems(shards, ("H", "f", "A", "bupper", "blower", "sense"))
        self._shard_keep = keep
        rc = lib().daqp_batch_setup_multi_shards(self._h, P, init_mask)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_setup_multi_shards failed ({rc}): {_lib.last_error()}")

    def update_shards(self, shards, mask):
        P, keep = self._shard_problems(shards, ("H", "f", "A", "bupper", "blower", "sense"))
        self._shard_keep_upd = keep
        rc = lib().daqp_batch_update_multi_shards(self._h, int(mask), P)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_update_multi_shards failed ({rc}): {_lib.last_error()}")

    def solve_shards(self, out="torch"):
        """one result dict per shard; out='torch': tensors on the shard's device, 'numpy': host arrays"""
        R = (DAQPBatchResult * self.shards)()
        outs = []
        for g in range(self.shards):
            _, sn, dev = self.shard(g)
            if out == "torch":
                d = torch.device("cuda", dev)
                o = dict(x=torch.empty((sn, self.n), dtype=torch.float64, device=d), lam=torch.empty((sn, self.m), dtype=torch.float64, device=d),
                         fval=torch.empty(sn, dtype=torch.float64, device=d), soft_slack=torch.empty(sn, dtype=torch.float64, device=d),
                         exitflag=torch.empty(sn, dtype=torch.int32, device=d), iter=torch.empty(sn, dtype=torch.int32, device=d))
                R[g] = DAQPBatchResult(o["x"].data_ptr(), o["lam"].data_ptr(), o["fval"].data_ptr(), o["soft_slack"].data_ptr(),
                                       o["exitflag"].data_ptr(), o["iter"].data_ptr(), MEM_DEVICE, 0, 0)
            else:
                o = dict(x=np.empty((sn, self.n)), lam=np.empty((sn, self.m)), fval=np.empty(sn), soft_slack=np.empty(sn),
                         exitflag=np.empty(sn, np.int32), iter=np.empty(sn, np.int32))
                R[g] = DAQPBatchResult(o["x"].ctypes.data, o["lam"].ctypes.data, o["fval"].ctypes.data, o["soft_slack"].ctypes.data,
                                       o["exitflag"].ctypes.data, o["iter"].ctypes.data, MEM_HOST, 0, 0)
            outs.append(o)
        rc = lib().daqp_batch_solve_multi_shards(self._h, R)
        if rc != 0:
            raise RuntimeError(f"daqp_batch_solve_multi_shards failed ({rc}): {_lib.last_error()}")
        return outs

    def shard_kernel_ms(self, g=0):
        a, b = C.c_float(0), C.c_float(0)
        lib().daqp_batch_kernel_ms(self.shard(g)[0], C.byref(a), C.byref(b))
        return a.value, b.value

    def shard(self, g):
        """(DAQPBatch handle, problems on it, device) of shard g -- for the single-device inspection calls"""
        sn, dev = C.c_int(0), C.c_int(0)
        h = lib().daqp_batch_multi_shard(self._h, g, C.byref(sn), C.byref(dev))
        return h, sn.value, dev.value
