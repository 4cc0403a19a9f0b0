"""ctypes prototypes of the C ABI, read from the headers under include/ (chaindp.h, chaindp_gaps.h, chaindp_debug.h, chaindp_fpga.h, and the stage headers chaindp.h includes).

The headers are the one place a prototype is written down: parse() turns a header's text into {name: (restype, [argtypes])} and
bind() sets them on the loaded library.  It reads these headers, it is not a C parser: a declaration or a type it does not
know raises, nothing defaults to int."""
import ctypes as C
import functools
import os
import re

from .params import AlignOpt, ChainParams, PostOpt

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "unsigned int": C.c_uint, "uint32_t": C.c_uint, "int64_t": C.c_int64,
            "unsigned long": C.c_ulong, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_STRUCTS = {"const chaindp_params_t *": C.POINTER(ChainParams), "const chaindp_post_opt_t *": C.POINTER(PostOpt),
            "const chaindp_align_opt_t *": C.POINTER(AlignOpt)}
_DECL = re.compile(r"(.+?[\s*])(\w+)\s*\(([^()]*)\)", re.S)      # ret name(args)


def _ctype(decl, where, ret=False):
    """The ctypes type of one parameter (`const int32_t *qlen`, `size_t bytes[4]`) or, with ret, of a return type -- by type alone.
    Every pointer but the parameter structs' is an address (c_void_p): callers pass array addresses, also for `const char *seq`."""
    t = " ".join(decl.replace("*", " * ").split())
    if not ret:
        t, is_array = re.subn(r" ?\[ ?\w* ?\]$", "", t)
        t = re.sub(r" ?\b\w+$", "", t) + (" *" if is_array else "")         # without the parameter's name
    if t in _STRUCTS:
        return _STRUCTS[t]
    if "*" in t:
        return C.c_char_p if ret and t == "const char *" else C.c_void_p
    if ret and t == "void":
        return None
    if t.replace("const ", "") not in _SCALARS:
        raise ValueError(f"{where}: no ctypes type for the C type {t!r}")
    return _SCALARS[t.replace("const ", "")]


def parse(text):
    """The functions a header declares: {name: (restype, [argtypes])}, in the header's order."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)             # comments
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)                    # preprocessor lines
    text = re.sub(r"\btypedef\b[^;{]*(\{[^}]*\})?[^;]*;", " ", text)        # typedefs, struct bodies included
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", text)
    out = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = _DECL.fullmatch(stmt)
        if not m:
            raise ValueError(f"not a function declaration: {stmt!r}")
        ret, name, args = m.groups()
        args = [] if args.strip() == "void" else [a.strip() for a in args.split(",")]
        out[name] = (_ctype(ret, f"{name}: return type", ret=True), [_ctype(a, f"{name}: parameter {a!r}") for a in args])
    return out


@functools.lru_cache(maxsize=None)
def prototypes(header):
    """parse() of include/<header>."""
    with open(os.path.join(INCLUDE, header)) as f:
        return parse(f.read())


def bind(lib, *headers):
    """Sets restype and argtypes of every function the headers declare on the loaded library `lib`."""
    for header in headers:
        for name, (restype, argtypes) in prototypes(header).items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib
