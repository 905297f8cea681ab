"""daqp_batch_backward / qp_layer: what can be checked without a GPU -- the exported symbol, its declaration and documented limits,
the Python surface, and that the package imports without its torch-only layer."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_backward_symbol_declared_and_exported():
    import daqp_amd
    from daqp_amd import _lib
    L = daqp_amd.lib()
    assert "daqp_batch_backward" in _lib.EXPORTS
    assert hasattr(L, "daqp_batch_backward")
    assert L.daqp_batch_backward(None, None, None, None, None, None, 0) != 0      # a NULL batch is refused, not dereferenced
    assert "null" in daqp_amd.last_error()
    assert callable(getattr(daqp_amd.BatchModel, "backward"))
    with open(os.path.join(ROOT, "include", "daqp_amd.h")) as fh:
        header = fh.read()
    assert "int daqp_batch_backward(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper," in header
    assert "#define DAQP_BACKWARD_SINGULAR" in header
    assert "SOFT CONSTRAINTS ARE OUT OF SCOPE" in header      # the header says what the call refuses
    assert "backward_kernel.hip" in _lib.units()


def test_import_does_not_touch_the_layer():
    """`import daqp_amd` leaves daqp_amd.layer alone (it needs torch), also when torch cannot be imported at all; the layer comes
    with the first use of daqp_amd.qp_layer"""
    code = ("import sys\n"
            "sys.path.insert(0, %r)\n"
            "sys.modules['torch'] = None\n"            # 'import torch' raises ImportError from here on
            "import daqp_amd\n"
            "assert 'daqp_amd.layer' not in sys.modules\n"
            "assert hasattr(daqp_amd.BatchModel, 'backward') and 'qp_layer' in daqp_amd.__all__\n"
            "try:\n"
            "    daqp_amd.qp_layer\n"
            "except ImportError:\n"
            "    print('lazy ok')\n") % ROOT
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable, *flags, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "lazy ok" in out.stdout, out.stderr[-2000:]
