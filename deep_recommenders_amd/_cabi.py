"""ctypes signatures read from the C headers under include/: the header is the one place a prototype is written down (the compiler
checks the definitions in csrc*/ against it), so the bindings cannot drift from it.  Understands exactly what those headers use --
scalar stdint / float types, pointers, `typedef void* X;` handles -- and raises on anything else instead of guessing."""
import ctypes
import functools
import re

_SCALARS = {"void": None, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}


def _ctype(decl, handles, fn):
    """ctypes type of one return type or argument declaration (`const float* x`, `int32_t F`, `dr_stream_t stream`)."""
    words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
    if words and re.fullmatch(r"[\w\s*]+", decl):
        if "*" in words:
            return ctypes.c_char_p if words[:2] == ["char", "*"] else ctypes.c_void_p
        if words[0] in handles:
            return ctypes.c_void_p
        if words[0] in _SCALARS and len(words) <= 2:
            return _SCALARS[words[0]]
    raise ValueError("%s: no ctypes mapping for %r" % (fn, decl.strip()))


def parse(text):
    """{name: (restype, [argtypes])} of every `ret name(args);` in the text of a header."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text).replace("}", " ")
    handles = set(re.findall(r"\btypedef\s+void\s*\*\s*(\w+)\s*;", text))
    text = re.sub(r"\btypedef\s+void\s*\*\s*\w+\s*;", " ", text)
    protos = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(\w+)\s*\(([^()]*)\)", stmt, flags=re.S)
        if m is None:
            raise ValueError("not a prototype: %r" % stmt)
        ret, name, args = m.groups()
        args = [] if args.strip() in ("", "void") else args.split(",")
        protos[name] = (_ctype(ret, handles, name), [_ctype(a, handles, name) for a in args])
    return protos


@functools.lru_cache(maxsize=None)
def prototypes(header_path):
    with open(header_path) as f:
        return parse(f.read())


def load(so_path, header_path):
    """CDLL of so_path with argtypes / restype of every function the header declares (AttributeError if one is not exported)."""
    L = ctypes.CDLL(so_path)
    for name, (restype, argtypes) in prototypes(header_path).items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L
