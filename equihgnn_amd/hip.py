"""ctypes binding of libequihgnn_hip.so — the C ABI declared in include/equihgnn_hip.h.

The argument structs, the function signatures and the stage / error constants are derived from the header at import:
there is no second copy of the ABI to keep in step.  A type or a declaration the reader below does not know raises here.

There is NO fallback: if the shared library is missing or a call returns an error code this
module raises.  The product path never routes through a CPU implementation.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_size_t, c_void_p

_PKG = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_PKG), "include", "equihgnn_hip.h")
# (EQH_LIB_PATH: another build of the same sources -- how two variants of a kernel are timed on ONE box, whose clocks differ
# from the next box's by more than most optimisations gain)
LIB_PATH = os.environ.get("EQH_LIB_PATH") or os.path.join(_PKG, "libequihgnn_hip.so")

_SCALARS = {"int": c_int32, "int32_t": c_int32, "int64_t": c_int64, "size_t": c_size_t, "float": c_float}
_POINTEES = {*_SCALARS, "void", "char", "uint8_t"}          # base types a pointer may have (any such pointer is c_void_p)
# what the reader drops (keeping line breaks): comments, the `extern "C"` guard, other preprocessor lines
_NOISE = [re.compile(r"/\*[^*]*\*+(?:[^/*][^*]*\*+)*/"), re.compile(r"//[^\n]*"),
          re.compile(r"#[ \t]*ifdef[ \t]+__cplusplus\b.*?#[ \t]*endif\b[^\n]*", re.S), re.compile(r"#[^\n]*")]
_DEFINE = re.compile(r"#[ \t]*define[ \t]+(EQH_\w+)[ \t]+\(?(-?\d+)\)?")
_ITEM = re.compile(r"\s*(?:typedef\s+struct\s*\w*\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>\w+)\s*;"
                   r"|enum\s*\{(?P<enum>[^{}]*)\}\s*;"
                   r"|(?P<head>[^;{}()]+)\((?P<args>[^;{}()]*)\)\s*;)")
# one declarator: [const] base, stars (each may be followed by const), [__restrict__], name, [array length]
_DECL = re.compile(r"\s*(?:const\s+)?(?:(\w+(?:\s+\w+)*?)\b\s*)?((?:\*\s*(?:const\b\s*)?)*)(?:__restrict__\b\s*)?(\w+)\s*"
                   r"(?:\[\s*(\d+)\s*\]\s*)?")


def parse_header(text: str, path: str = "<header>"):
    """(structs, signatures, constants) of a C header in the form of include/equihgnn_hip.h: its `typedef struct [Tag] {
    ... } Name;` blocks as ctypes.Structure classes, every function declaration as name -> (restype, argtypes), and the
    values of its `enum { ... }` and `#define EQH_*` lines.  Raises ValueError, naming the line, on anything else."""
    lines = text.splitlines()
    blank = lambda m: " " + "\n" * m[0].count("\n")
    text = _NOISE[1].sub(blank, _NOISE[0].sub(blank, text))
    constants = {m[1]: int(m[2]) for m in _DEFINE.finditer(text)}
    text = _NOISE[3].sub(blank, _NOISE[2].sub(blank, text)).rstrip()
    structs, signatures, arg_types = {}, {}, {}      # arg_types: parameter text -> ctype (376 distinct of 1231 in the header)

    def fail(piece, at):                     # piece: the text at text[at:]
        line = text.count("\n", 0, at + len(piece) - len(piece.lstrip())) + 1
        raise ValueError(f"{path}:{line}: cannot bind `{lines[line - 1].strip()}`")

    def declarators(decl, at, kind="field"):
        """[(name, ctype)] of `base *name[length], *name2, ...`: one struct line; or one parameter or a function's head
        (kind "arg" / "ret": a single declarator, no array)"""
        out, base = [], None
        for piece in decl.split(",") if kind == "field" else (decl,):
            d = _DECL.fullmatch(piece)
            if d is None or bool(d[1]) == bool(base) or (d[4] and kind != "field"):
                fail(decl, at)
            base, stars = base or d[1], d[2].count("*")
            if base in structs and stars == 1:
                t = POINTER(structs[base])
            elif stars == 0 and base in _SCALARS:
                t = _SCALARS[base]
            elif kind == "ret" and (base, stars) in (("void", 0), ("char", 1)):
                t = None if stars == 0 else c_char_p
            elif stars and base in _POINTEES:
                t = POINTER(c_void_p) if (base, stars) == ("void", 2) else c_void_p
            else:
                fail(decl, at)
            out.append((d[3], t if d[4] is None else t * int(d[4])))
        return out

    pos = 0
    while pos < len(text):
        m = _ITEM.match(text, pos)
        if m is None:
            fail(text[pos:].split(";")[0], pos)
        if m["struct"]:
            fields, at = [], m.start("fields")
            for d in m["fields"].split(";"):
                if d.strip():
                    fields += declarators(d, at)
                at += len(d) + 1
            structs[m["struct"]] = type(m["struct"], (ctypes.Structure,),
                                        {"_fields_": fields, "__doc__": f"{m['struct']} of include/equihgnn_hip.h"})
        elif m["enum"] is not None:
            for item in m["enum"].split(","):
                k, eq, v = (w.strip() for w in item.partition("="))
                if not (eq and k.isidentifier() and v.lstrip("-").isdigit()):
                    fail(m[0], pos)
                constants[k] = int(v)
        else:
            ((name, res),) = declarators(m["head"], m.start("head"), "ret")
            args, at = [], m.start("args")
            if m["args"].strip() != "void":
                for a in m["args"].split(","):
                    if a.strip() not in arg_types:
                        arg_types[a.strip()] = declarators(a, at, "arg")[0][1]
                    args.append(arg_types[a.strip()])
                    at += len(a) + 1
            signatures[name] = (res, args)
        pos = m.end()
    return structs, signatures, constants


with open(HEADER) as _f:
    _structs, SIGNATURES, _constants = parse_header(_f.read(), HEADER)
globals().update(_structs)         # HgSmallMM, HgGemmProblem, HgPanelPack, HgConvPanel, HgPanelMulti, HgPanelSum, HbCollate, GbCollate
globals().update(_constants)       # EQH_OK, EQH_ERR_*, HG_CONV_F1 .. HG_EGNN_NODE_B

_lib = None


class HipLibraryError(RuntimeError):
    pass


def load(path: str, partial: bool = False) -> ctypes.CDLL:
    """Open a build of the library and type every function of the header that it exports.  partial=False (a product
    build): each of them must be there.  partial=True: a diagnostic build of some of the sources binds what it has."""
    if not os.path.exists(path):
        raise HipLibraryError(
            f"{path} is missing: build it with `python -m equihgnn_amd.build` "
            "(hipcc --offload-arch=gfx950).  equihgnn_amd has no CPU fallback.")
    try:
        handle = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise HipLibraryError(f"cannot load {path}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            if partial:
                continue
            raise HipLibraryError(f"{path} does not export {name}; rebuild it") from e
        fn.restype = res
        fn.argtypes = args
    return handle


def lib() -> ctypes.CDLL:
    """Load (once) and return the shared library; raise if it is not built."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH)
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().eqh_error_string(rc)
        raise HipLibraryError(f"{what} failed with code {rc}: {msg.decode() if msg else '?'}")
