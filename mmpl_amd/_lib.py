"""ctypes binding of libmmpl_hip.so, made from include/mmpl_hip.h.  Fails loudly: there is no CPU / PyTorch fallback.

The header (the one csrc/ compiles against) is read at import, its /* */ comments stripped, and gives
  - the structs: every `typedef struct X { ... } X;` body (int / float members, several names per declaration) becomes the
    ctypes.Structure `X` of this module;
  - SYMBOLS: the sorted names of the `mmpl_*` functions it declares;
  - each function's restype / argtypes, by ONE rule: int, float, double, size_t, long long -> the matching ctypes scalar; a void
    return -> None; a `const char*` return -> c_char_p; a pointer to a struct the header defines -> POINTER(that struct), unless
    the parameter's name ends in `_dev` (the header's mark of a device pointer: `const MmplUniPCStep* table_dev` is device memory,
    passed as c_void_p(data_ptr())); every other pointer (mmpl_stream_t, opaque handles, Handle**, const void* const*, const int*,
    float*, ...) -> c_void_p, because the header's TYPE cannot say whether e.g. a `const float*` is a host array or a device
    pointer, and c_void_p takes every form callers pass (ctypes arrays, byref(), None, c_void_p, plain ints).
A type outside that rule, or a missing header, raises at import; a declared function the .so does not export raises in load().
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmmpl_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mmpl_hip.h")

_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "long long": C.c_longlong}


def _parse_header(path):
    """-> ({struct name: Structure class}, {function name: (restype, argtypes)}) by the rule in the module docstring."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    opaque = set(re.findall(r"typedef void\s*\*\s*(\w+);", src))          # mmpl_stream_t
    structs = {}

    def ctype(ty, decl, ret=False, name=""):
        ty = " ".join(ty.replace("const", " ").replace("*", " * ").split())
        if ty in _SCALARS:
            return _SCALARS[ty]
        if ret and ty in ("void", "char *"):
            return None if ty == "void" else C.c_char_p
        if not ret and (ty.endswith(" *") or ty in opaque):
            return C.POINTER(structs[ty[:-2]]) if ty[:-2] in structs and not name.endswith("_dev") else C.c_void_p
        raise ValueError(f"{path}: no ctypes mapping for {ty!r} in: {decl.strip()}")

    for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", src, flags=re.S):
        members = [d.split(None, 1) for d in body.split(";") if d.strip()]           # "int a, b" -> ["int", "a, b"]
        structs[name] = type(name, (C.Structure,), {"_fields_": [(n.strip(), ctype(ty, f"struct {name} {{{body}}}"))
                                                                  for ty, names in members for n in names.split(",")]})
    protos = {}
    for decl in re.findall(r"^[\w ]+?\**\s*\bmmpl_\w+\s*\([^)]*\)\s*;", src, flags=re.M):
        ret, name, params = re.match(r"(.*?)\b(mmpl_\w+)\s*\((.*)\)", decl, flags=re.S).groups()
        params = [] if params.strip() == "void" else [re.match(r"(.*?)(\w+)$", p.strip(), flags=re.S).groups() for p in params.split(",")]
        protos[name] = (ctype(ret, decl, ret=True), [ctype(ty, decl, name=pname) for ty, pname in params])
    return structs, protos


_STRUCTS, _PROTOS = _parse_header(HEADER_PATH)
globals().update(_STRUCTS)                # MmplDitConfig, MmplUniPCStep, MmplT5Config
SYMBOLS = sorted(_PROTOS)

_lib = None


def load() -> C.CDLL:
    """Load the HIP library; raise (never fall back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the MI355X HIP extension is not built. Run `python -m mmpl_amd.build` "
            "(or __graft_entry__.build()). mmpl_amd has no CPU/PyTorch fallback by design.")
    # torch first: it ships its own libamdhip64, and device memory / streams are shared with it.  If this library were
    # dlopen'ed before torch, the system HIP runtime would be bound instead and every hipMalloc here would fail once torch
    # initialises the device through the other copy (seen as "hipMalloc ... failed" in build() -> smoke() in one process).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _PROTOS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise RuntimeError(f"{LIB_PATH} does not export {name}, which include/mmpl_hip.h declares: it is stale, rebuild it "
                               "(`python -m mmpl_amd.build`)") from None
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise RuntimeError(f"libmmpl_hip {what}: {load().mmpl_last_error().decode()}")


def ptr(t) -> C.c_void_p:
    """Borrowed device pointer of a torch tensor (None -> NULL)."""
    return C.c_void_p(0 if t is None else t.data_ptr())


def bind_weights(fn, handle, tensors, what: str) -> None:
    """Hand the device pointers of `tensors`, in order, to the mmpl_*_bind_weights entry `fn`.  The library borrows them: the
    caller keeps the tensors alive."""
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    check(fn(handle, arr, len(tensors)), what)


def stream_ptr() -> C.c_void_p:
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
