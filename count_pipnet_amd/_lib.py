"""ctypes binding of the C-ABI in ``include/pipnet_amd.h`` (``libpipnet_amd.so``).

This is exactly the binding a maintainer would add to the reference:
the library takes raw device pointers, sizes and a hipStream_t, and returns a status
code that is raised here as ``RuntimeError`` (the reference raises Python exceptions,
SURVEY.md 8b).  There is no fallback: if the library is missing the import fails loudly.
"""
from __future__ import annotations

import ctypes
import os
import re

from .build import REPO, source_digest

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PIPNET_AMD_LIB") or os.path.join(_HERE, "libpipnet_amd.so")    # env: A/B builds (tools)

P = ctypes.c_void_p
I32 = ctypes.c_int
I64 = ctypes.c_int64
U64 = ctypes.c_uint64
F32 = ctypes.c_float
F64 = ctypes.c_double


class PipnetLibraryError(RuntimeError):
    pass


HEADER = os.path.join(REPO, "include", "pipnet_amd.h")
_SCALARS = {"int": I32, "int64_t": I64, "uint64_t": U64, "float": F32, "double": F64}
_RETURNS = {"int": I32, "int64_t": I64, "const char *": ctypes.c_char_p}


def _argtype(param: str, decl: str):
    toks = param.replace("*", " * ").split()
    if "*" in toks:                      # every pointer is opaque, but a writable char* is a label buffer
        return ctypes.c_char_p if toks[:2] == ["char", "*"] else P
    ctype = _SCALARS.get(" ".join(toks[:-1]))
    if ctype is None:
        raise PipnetLibraryError(f"{HEADER}: no ctypes type for parameter '{param.strip()}' of {decl}")
    return ctype


def parse_header(text: str):
    """(name -> argtypes, name -> restype, PIPNET_<NAME> -> int) of the C header ``text``: only the shapes
    include/pipnet_amd.h uses (one-line integer #defines, ``type pipnet_name(params);`` over any lines)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#define[ \t]+PIPNET_(\w+)[ \t]+(-?\d+)[ \t]*$", text,
                                                   flags=re.M)}
    argtypes, restypes = {}, {}
    for m in re.finditer(r"^[ \t]*([\w \t*]+?)(pipnet_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        ret, name, params = " ".join(m[1].replace("*", " * ").split()), m[2], m[3].strip()
        if ret not in _RETURNS:
            raise PipnetLibraryError(f"{HEADER}: no ctypes type for the return type '{ret}' of {name}")
        restypes[name] = _RETURNS[ret]
        argtypes[name] = [] if params == "void" else [_argtype(p, name) for p in params.split(",")]
    return argtypes, restypes, consts


def _read_header() -> str:
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:
        raise PipnetLibraryError(f"{HEADER} is missing: the binding of {LIB_PATH} is read from it") from e


# name -> argtypes / restype of every entry point, and the header's integer constants without the PIPNET_ prefix
SIGNATURES, RESTYPES, CONSTANTS = parse_header(_read_header())
globals().update({k: v for k, v in CONSTANTS.items() if k.startswith("EPI_")})       # _lib.EPI_NONE, ...
ABI_VERSION = CONSTANTS["AMD_ABI_VERSION"]

_lib = None


def load() -> ctypes.CDLL:
    """Load (once) and return the HIP library; raise if it is absent or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PipnetLibraryError(
            f"{LIB_PATH} is missing: the MI355X inference path has no fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `python count_pipnet_amd/build.py`.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError = missing export = loud failure
        fn.argtypes = args
        fn.restype = RESTYPES[name]
    _check_provenance(lib)
    if lib.pipnet_amd_abi_version() != ABI_VERSION:
        raise PipnetLibraryError(f"{LIB_PATH} exports ABI version {lib.pipnet_amd_abi_version()}, "
                                 f"this binding expects {ABI_VERSION} (include/pipnet_amd.h)")
    _lib = lib
    return lib


def _check_provenance(lib) -> None:
    """The library must have been compiled from the sources of this tree (sha256 compiled
    in by build.py).  ``PIPNET_AMD_ALLOW_STALE=1`` is the explicit A/B escape hatch (e.g. an
    experimental build loaded through ``PIPNET_AMD_LIB``)."""
    built = lib.pipnet_amd_source_digest().decode()
    here = source_digest()
    if built != here and os.environ.get("PIPNET_AMD_ALLOW_STALE") != "1":
        raise PipnetLibraryError(
            f"{LIB_PATH} was built from other sources (digest {built[:16]}..., tree {here[:16]}...): "
            "rebuild with `python count_pipnet_amd/build.py` (or set PIPNET_AMD_ALLOW_STALE=1 for an A/B run)")


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().pipnet_amd_status_string(status).decode()
        raise RuntimeError(f"{what} failed: PIPNET status {status} ({msg})")


def call(name: str, *args) -> None:
    check(getattr(load(), name)(*args), name)


def label(name: str, *args) -> str:
    """A profiling-label query (pipnet_*_label): the kernel name the launch with these arguments runs."""
    buf = ctypes.create_string_buffer(256)
    if getattr(load(), name)(*args, buf, len(buf)) < 0:
        raise RuntimeError(f"{name}{args}: the library launches no kernel for these arguments")
    return buf.value.decode()
