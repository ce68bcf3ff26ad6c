"""ctypes binding of the host-side input library (include/dr_input.h -> lib/libdr_input.so); signatures read from the header."""
import os

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(_HERE, "..", "include", "dr_input.h")
DRI_OK, DRI_EINVAL, DRI_EIO, DRI_ECORRUPT, DRI_EPARSE, DRI_ECAPACITY = 0, -1, -10, -11, -12, -13
_ERR = {DRI_EINVAL: "DRI_EINVAL (bad argument)", DRI_EIO: "DRI_EIO (cannot open / short read)",
        DRI_ECORRUPT: "DRI_ECORRUPT (TFRecord framing or CRC mismatch)",
        DRI_EPARSE: "DRI_EPARSE (malformed Example, or a fixed-length key missing / wrong kind / not one value)",
        DRI_ECAPACITY: "DRI_ECAPACITY (output too small)"}
_LIB = None


class InputLibraryMissing(RuntimeError):
    pass


def path():
    return os.path.join(_HERE, "lib", "libdr_input.so")


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(path()):
            raise InputLibraryMissing("%s not found: run `python -m deep_recommenders_amd.build`" % path())
        _LIB = _cabi.load(path(), HEADER)
    return _LIB


def __getattr__(name):
    if name == "SIGNATURES":        # {name: (restype, [argtypes])} of every declared function, parsed on first use
        return _cabi.prototypes(HEADER)
    raise AttributeError(name)


def check(status, what):
    if status != DRI_OK:
        raise ValueError("%s failed: %s" % (what, _ERR.get(status, status)))
