"""Reader of the C-ABI headers (include/resr.h, include/resr_debug.h) for the ctypes binding of _lib.py.

It understands what those two files contain and nothing more: /* */ comments, preprocessor lines (`#define NAME integer` is a constant),
the extern "C" braces, enums with members `NAME = integer` or `NAME = 1 << k`, `typedef struct` with scalar, array and pointer fields,
and function declarations.  A statement it cannot classify, or a scalar type it does not know, raises ValueError quoting the statement.
"""
import ctypes as C
import re
import types

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}
_DECL = re.compile(r"(.+?)\b(\w+)(?:\[(\d+)\])?")   # type, name, array length: `const void* const* out`, `int32_t fq[9]`


def _ctype(abi, text, stmt, returned=False):
    """The ctypes type of a C type: a scalar of SCALARS; `const char*` returned -> c_char_p; ONE pointer to a structure named *Desc ->
    POINTER of it; every other pointer -> c_void_p."""
    base, *stars = [t for t in text.replace("*", " * ").split() if t != "const"] or [""]
    if stars == ["*"] * len(stars):
        if not stars:
            if base in SCALARS:
                return SCALARS[base]
            if returned and base == "void":
                return None
        elif len(stars) == 1 and base.endswith("Desc"):
            if base in abi.structs:
                return C.POINTER(abi.structs[base])
        else:
            return C.c_char_p if returned and (base, len(stars)) == ("char", 1) else C.c_void_p
    raise ValueError(f"unknown type {text.strip()!r} in: {stmt}")


def _struct(abi, name, body, stmt):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split("|"))):     # `int32_t n, h, w`: the names after the first share its type
        first, *more = (d.strip() for d in decl.split(","))
        m = _DECL.fullmatch(first)
        for d in [first] + [m.group(1) + d for d in more if m]:
            m = _DECL.fullmatch(d)
            if not m:
                raise ValueError(f"cannot read the field {d!r} of: {stmt}")
            t = _ctype(abi, m.group(1), stmt)
            fields.append((m.group(2), t * int(m.group(3)) if m.group(3) else t))
    abi.structs[name] = type(name[4:] if name.startswith("Resr") else name, (C.Structure,), {"_fields_": fields})


def _enum(abi, body, stmt):
    for member in body.split(","):
        m = re.fullmatch(r"\s*(\w+) = (?:(-?\d+)|1 << (\d+))\s*", member)
        if not m:
            raise ValueError(f"enum member {member.strip()!r} is neither `NAME = integer` nor `NAME = 1 << k` in: {stmt}")
        abi.consts[m.group(1)] = int(m.group(2)) if m.group(2) else 1 << int(m.group(3))


def _function(abi, returns, name, params, stmt):
    if "(" in params or ")" in params:
        raise ValueError(f"cannot read the parameters (a function pointer?) of: {stmt}")
    args = []
    for p in ([] if params == "void" else params.split(",")):
        m = _DECL.fullmatch(p.strip())
        if not m or m.group(3):
            raise ValueError(f"cannot read the parameter {p.strip()!r} of: {stmt}")
        args.append(_ctype(abi, m.group(1), stmt))
    abi.protos[name] = (_ctype(abi, returns, stmt, returned=True), args)


def parse(text, abi=None):
    """Adds the declarations of one header's text to `abi` (a new one if None): .consts name -> int, .structs C name -> ctypes.Structure
    class (fields in header order), .protos name -> (restype, [argtypes]).  A later header may use the structures of an earlier one."""
    abi = abi or types.SimpleNamespace(consts={}, structs={}, protos={})
    lines = []
    for line in re.sub(r"/\*.*?\*/", " ", text, flags=re.S).splitlines():
        m = re.fullmatch(r"\s*#\s*define\s+(\w+)(?:\s+(-?\d+))?\s*", line)
        if m and m.group(2):
            abi.consts[m.group(1)] = int(m.group(2))
        elif not m and re.match(r"\s*#\s*define\b", line):
            raise ValueError(f"cannot read: {line.strip()}")
        elif not line.lstrip().startswith("#"):
            lines.append(line)
    # the `;` inside a struct body become `|`, so that every `;` left ends one statement of the extern "C" block
    text = re.sub(r"\{([^{}]*)\}", lambda m: m.group(0).replace(";", "|"), " ".join(" ".join(lines).split()))
    block = re.fullmatch(r'extern "C" \{(.*)\}', text)
    if not block:
        raise ValueError('expected one extern "C" { ... } block around the declarations')
    for stmt in filter(None, (s.strip() for s in block.group(1).split(";"))):
        m = re.fullmatch(r"(typedef )?(enum|struct) \{(.*)\} ?(\w*)", stmt)
        stmt = stmt.replace("|", ";")   # as the header spells it, for the messages
        f = re.fullmatch(r"(.+?)\b(\w+) ?\((.*)\)", stmt)
        if m and m.group(2) == "enum" and bool(m.group(1)) == bool(m.group(4)):
            _enum(abi, m.group(3), stmt)
        elif m and m.group(2) == "struct" and m.group(1) and m.group(4):
            _struct(abi, m.group(4), m.group(3), stmt)
        elif f and not m:
            _function(abi, f.group(1), f.group(2), f.group(3).strip(), stmt)
        else:
            raise ValueError(f"cannot classify the statement: {stmt}")
    return abi


def read(*paths):
    """parse() over the header files at `paths`, in order."""
    abi = None
    for path in paths:
        try:
            with open(path) as f:
                abi = parse(f.read(), abi)
        except FileNotFoundError:
            raise RuntimeError(f"{path} not found: the binding is read from the headers of include/, which must lie beside the package") from None
    return abi
