"""ctypes binding of the C-ABI hot-path library (include/dr_hotpath.h).

There is NO fallback: if libdr_hotpath.so is missing or a tensor is not on a HIP device the call
raises.  PyTorch is used only for device memory and streams; every computation on the product path
happens inside the hand-written gfx950 kernels behind this boundary.
"""
import os

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "lib", "libdr_hotpath.so")

HEADER = os.path.join(_HERE, "..", "include", "dr_hotpath.h")   # the signatures are read from it (_cabi.py)

DR_OK, DR_EINVAL, DR_ELAUNCH, DR_ESHAPE = 0, -1, -2, -3
_ERR = {DR_EINVAL: "DR_EINVAL (bad argument)", DR_ELAUNCH: "DR_ELAUNCH (HIP launch error)",
        DR_ESHAPE: "DR_ESHAPE (shape contract violated)"}

_LIB = None


class HotPathLibraryMissing(RuntimeError):
    pass


def lib():
    """Returns the loaded library; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise HotPathLibraryMissing(
                "HIP hot-path library not built: %s is missing. Build it with "
                "`python -m deep_recommenders_amd.build` (or __graft_entry__.build()). "
                "There is no CPU/PyTorch fallback." % SO_PATH)
        _LIB = _cabi.load(SO_PATH, HEADER)   # AttributeError if the .so does not export a declared symbol
    return _LIB


def __getattr__(name):
    if name == "SIGNATURES":        # {name: (restype, [argtypes])} of every declared function, parsed on first use
        return _cabi.prototypes(HEADER)
    raise AttributeError(name)


def check(status, what):
    if status != DR_OK:
        raise RuntimeError("%s failed: %s" % (what, _ERR.get(status, status)))


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("hot-path kernels need tensors in HBM (got a %s tensor); there is no CPU fallback"
                           % t.device)
    return t.data_ptr()


_raw_stream = None


def stream_ptr():
    """The current torch stream of the current device as a raw hipStream_t.  Through torch's C entry points, not through
    torch.cuda.current_stream() (a Python object per call, ~2.5 us): every op of a training step asks once, ~22 times per step, and the
    host's launch work per step is what a busy shared host can turn into the step's bound (0.33 ms against 1.14 ms of GPU work)."""
    global _raw_stream
    if _raw_stream is None:
        import torch
        if hasattr(torch._C, "_cuda_getCurrentRawStream") and hasattr(torch._C, "_cuda_getDevice"):
            _raw_stream = (torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice)
        else:
            _raw_stream = (lambda dev: torch.cuda.current_stream(dev).cuda_stream, torch.cuda.current_device)
    return _raw_stream[0](_raw_stream[1]())
