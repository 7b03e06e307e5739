"""Loader for libphastft_hip.so (the C ABI of include/phastft_hip.h).

The HIP library IS the product: there is no CPU path behind this module.  If the shared object is
missing or a call fails, the caller gets an exception -- never a silent fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PHASTFT_HIP_LIB") or os.path.join(_HERE, "lib", "libphastft_hip.so")

HEADER = os.path.join(os.path.dirname(_HERE), "include", "phastft_hip.h")  # where build.py finds it, too

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "unsigned long long": C.c_ulonglong,
            "double": C.c_double}
_POINTEE = re.compile(r"float|void|char|phast_\w+|" + "|".join(_SCALARS))


def _ctype(decl: str, proto: str):
    """the ctypes type of a C return type or parameter type: the scalars by value, `const char *` as c_char_p, every other
    pointer (handles, buffers, out-parameters, arrays of pointers) as c_void_p.  Anything else is an error, never a guess."""
    words = decl.replace("*", " * ").split()
    base = " ".join(w for w in words if w not in ("*", "const"))
    if "*" not in words:
        if base in _SCALARS:
            return _SCALARS[base]
    elif words == ["const", "char", "*"]:
        return C.c_char_p
    elif _POINTEE.fullmatch(base):
        return C.c_void_p
    raise ValueError(f"include/phastft_hip.h: no ctypes mapping for the type {decl!r} in `{proto}`")


def parse_prototypes(text: str) -> dict:
    """{name: (restype, argtypes)} of every function the text of a C header declares.  The header is plain on purpose: after
    the comments, the preprocessor lines and the typedefs are gone, one `type phast_name(type name, ...);` per function."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"\btypedef\b[^;{]*(\{[^}]*\})?[^;]*;", "", text)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    out = {}
    for proto in (" ".join(p.split()) for p in text.split(";")):
        if not proto:
            continue
        m = re.fullmatch(r"(.+?)\b(phast_\w+) ?\((.*)\)", proto)
        if not m:
            raise ValueError(f"include/phastft_hip.h: not a function prototype: `{proto}`")
        ret, name, params = m.groups()
        args = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            pm = re.fullmatch(r"(.*[\s*])\w+", param.strip())  # the type, then the parameter's name
            args.append(_ctype(pm.group(1) if pm else param, proto))
        out[name] = (None if ret.strip() == "void" else _ctype(ret, proto), args)
    return out


with open(HEADER) as _f:
    PROTOTYPES = parse_prototypes(_f.read())
SYMBOLS = list(PROTOTYPES)  # every symbol include/phastft_hip.h declares


class PhastOptions(C.Structure):
    """`phast_options` (options.rs:10-24)."""

    _fields_ = [("multithreaded_bit_reversal", C.c_int), ("smallest_parallel_chunk_size", C.c_size_t)]


class PhastTuneReport(C.Structure):
    """`phast_tune_report` (include/phastft_hip.h: PlannerMode::Tune)."""

    _fields_ = [("adopted", C.c_int), ("candidates", C.c_uint), ("us_heuristic", C.c_float), ("us_best", C.c_float),
                ("seconds", C.c_double), ("plan", C.c_char * 96)]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m phastft_amd.build` (hipcc, gfx950). "
            "phastft_amd has no CPU fallback.")
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  Whichever
    # copy is loaded first serves both, and mixing the two leaves the second user without a device.  The package
    # works on torch device tensors and torch streams, so torch's runtime must be the one: import it first.
    try:
        import torch  # noqa: F401
    except ImportError:  # a torch-less process (e.g. a C or Rust host) simply uses /opt/rocm's runtime
        pass
    l = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(l, name)  # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = restype, argtypes
    _lib = l
    return l
