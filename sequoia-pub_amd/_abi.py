"""The C ABI as ctypes, read from include/sequoia_hip.h -- the only place it is written down.

``parse`` understands exactly the forms the header uses: ``#define SQ_NAME <integer>``, ``typedef void* name;``,
``typedef struct tag { int32_t a, b; int64_t c; sq_other d[SQ_MACRO]; } name;`` and ``ret name(type arg, ...);``.
Anything else raises ``AbiError`` at import: a declaration is never skipped.  FUNCTIONS maps each function to
``(restype, argtypes)``, STRUCTS each struct's C name to its ``ctypes.Structure``, CONSTANTS each integer macro to its value.
"""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sequoia_hip.h")


class AbiError(Exception):
    pass


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = {"void", "char", "uint8_t", "uint32_t", "int64_t", *_SCALARS}        # T* of these is a c_void_p (char*: c_char_p)
_FIELDS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
_WORDS = {"resnet50": "ResNet50"}                                                 # sq_resnet50_layout -> ResNet50Layout

_STATEMENT = re.compile(r"""\s*(?:
      typedef\s+struct\s+\w+\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)
    | typedef\s+void\s*\*\s*(?P<handle>\w+)
    | (?P<ret>[\w\s*]+?)\b(?P<function>\w+)\s*\((?P<args>[^(){};]*)\)
    )\s*;""", re.X)


def _structure(cname, body, structs, constants):
    fields = []
    for line in filter(None, (s.strip() for s in body.split(";"))):
        kind, _, names = line.partition(" ")
        ctype = _FIELDS.get(kind) or structs.get(kind)
        if ctype is None:
            raise AbiError(f"{cname}: field {line!r} is not understood")
        for name in names.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", name)
            if not m:
                raise AbiError(f"{cname}: field {name!r} is not understood")
            if m.group(2) is None:
                fields.append((m.group(1), ctype))
            elif m.group(2).isdigit() or m.group(2) in constants:
                fields.append((m.group(1), ctype * int(constants.get(m.group(2), m.group(2)))))
            else:
                raise AbiError(f"{cname}.{m.group(1)}: extent {m.group(2)!r} is no integer macro of the header")
    pyname = "".join(_WORDS.get(w, w.capitalize()) for w in cname.split("_")[1:])
    return type(pyname, (ctypes.Structure,), {"_fields_": fields})


def _ctype(decl, named, structs, handles):
    """ctypes type of one parameter (``named``: the last word is its name) or of a return type."""
    tokens = [t for t in decl.replace("*", " * ").split() if t != "const"]
    if named and tokens and tokens[-1] != "*":
        tokens.pop()
    base, stars = " ".join(t for t in tokens if t != "*"), tokens.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if base in handles and stars <= 1:
        return ctypes.c_void_p
    if stars == 1 and base in structs:
        return ctypes.POINTER(structs[base])
    if stars == 1 and base == "char":
        return ctypes.c_char_p
    if stars >= 1 and base in _POINTEES:
        return ctypes.c_void_p
    raise AbiError(f"type {decl.strip()!r} is not understood")


def parse(text):
    """Header text -> (functions, structs, constants)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus\n.*?#endif", "", text, flags=re.S)          # extern "C" { ... }
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SQ_\w+)(.*)$", text, flags=re.M):
        if not re.fullmatch(r"\s*-?\d+\s*", value):
            raise AbiError(f"#define {name}{value}: not an integer")
        constants[name] = int(value)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    functions, structs, handles, pos = {}, {}, set(), 0
    while text[pos:].strip():
        m = _STATEMENT.match(text, pos)
        if not m:
            raise AbiError(f"declaration not understood: {' '.join(text[pos:].split())[:100]!r}")
        pos = m.end()
        if m.group("struct"):
            structs[m.group("struct")] = _structure(m.group("struct"), m.group("body"), structs, constants)
        elif m.group("handle"):
            handles.add(m.group("handle"))
        else:
            args = m.group("args").strip()
            try:
                restype = _ctype(m.group("ret"), False, structs, handles)
                argtypes = [] if args == "void" else [_ctype(a, True, structs, handles) for a in args.split(",")]
            except AbiError as e:
                raise AbiError(f"{m.group('function')}: {e}") from None
            functions[m.group("function")] = (restype, argtypes)
    return functions, structs, constants


with open(HEADER) as _f:
    FUNCTIONS, STRUCTS, CONSTANTS = parse(_f.read())
