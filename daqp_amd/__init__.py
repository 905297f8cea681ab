"""daqp_amd -- MI355X-native batched dual active-set QP path behind the DAQP C API.

The numerical work is done by hand-written HIP kernels in daqp_amd/csrc (one wavefront per QP),
reached only through the C ABI in include/daqp_amd.h.  This package is the host-side mirror of
the reference's Python binding for that path.
"""
from ._lib import build, default_settings, last_error, lib, LIBPATH  # noqa: F401
from .api import (BatchModel, EliminatedBatchModel, MultiBatchModel, Model, certify_batch, minrep, minrep_batch, solve, solve_batch, solve_batch_multi, UPDATE_Rinv, UPDATE_M, UPDATE_v, UPDATE_d,  # noqa: F401
                  UPDATE_sense, UPDATE_unconstrained, UPDATE_eliminate)



def __getattr__(name):
    # the autograd layer needs torch: imported on first use, so that the package works on numpy without it
    if name in ("layer", "qp_layer"):
        import importlib
        mod = importlib.import_module(".layer", __name__)
        return mod if name == "layer" else mod.qp_layer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["qp_layer", "build", "lib", "solve", "Model", "solve_batch", "solve_batch_multi", "minrep", "minrep_batch", "certify_batch", "BatchModel", "EliminatedBatchModel", "MultiBatchModel", "default_settings", "last_error"]
