"""ctypes binding of the C-ABI exchange library (include/dr_collectives.h -> lib/libdr_collectives.so, RCCL underneath); signatures
read from the header.

The Python engines in this package exchange through torch.distributed (backend "nccl" == RCCL); this library is the same plan
for a host that is not PyTorch.  Bound here for the tests (a single-rank communicator on one GPU)."""
import os

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(_HERE, "..", "include", "dr_collectives.h")
ID_BYTES = 128
_LIB = None


def path():
    return os.path.join(_HERE, "lib", "libdr_collectives.so")


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(path()):
            raise RuntimeError("%s not found: run `python -m deep_recommenders_amd.build`" % path())
        _LIB = _cabi.load(path(), HEADER)
    return _LIB


def __getattr__(name):
    if name == "SIGNATURES":        # {name: (restype, [argtypes])} of every declared function, parsed on first use
        return _cabi.prototypes(HEADER)
    raise AttributeError(name)


def check(status, what):
    if status != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, status, (lib().dr_coll_last_error() or b"").decode()))
