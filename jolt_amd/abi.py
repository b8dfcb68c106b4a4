"""The C ABI of libjolt_hip.so as include/jolt_hip.h states it, read once: entry points, constants, callback types.

The header is the one place that knows the ABI.  `declare(lib)` gives every entry point its ctypes prototype, so a call site passes
plain Python ints and ctypes converts (or refuses) them by the header's types; tools/gen_rust_ffi.py renders the same declarations
for Rust.  A C type is a pair (base, consts): `base` the type name and `consts` one bool per pointer level, constness of what that
level points to -- ('jolt_fr_t', (True, True)) is `const jolt_fr_t *const *`, ('size_t', ()) a scalar.
"""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "jolt_hip.h")

SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}


def strip_comments(src):
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def opaque_handles(path=None):
    """every `typedef struct X X;` of the header, in declaration order: the handle types ffi.rs must define (a hand-kept list went stale in round 3)"""
    return re.findall(r"typedef\s+struct\s+(jolt_\w+)\s+\1\s*;", open(path or HEADER).read())


def c_type(text):
    """'const jolt_fr_t *const *' -> ('jolt_fr_t', (True, True))"""
    toks = re.findall(r"\*|\w+", text)
    base, const, consts = None, False, []
    for t in toks:
        if t == "*":
            consts.append(const)
            const = False
        elif t == "const":
            const = True
        elif t != "struct":
            assert base is None and not consts, text
            base = t
    return base, tuple(consts)


def _params(text):
    """'void *user, const jolt_fr_t u[3]' -> [(name, c_type)] (arrays decay to pointers; every parameter of the header is named)"""
    text = " ".join(text.split())
    if not text or text == "void":
        return []
    out = []
    for p in text.split(","):
        m = re.match(r"(.*?)(\w+)\s*(\[\s*\d*\s*\])?$", p.strip())
        out.append((m.group(2), c_type(m.group(1) + (" *" if m.group(3) else ""))))
    return out


def _code(path):
    src = re.sub(r"#.*", "", strip_comments(open(path).read()))
    return re.sub(r'extern\s+"C"\s*\{', "", src)


def parse_header(path=HEADER):
    """-> list of (name, ret_type, [(param_name, type)]) in declaration order"""
    src = _code(path)
    decls = []
    for m in re.finditer(r"(?:^|;|\})\s*((?:const\s+)?\w+\s*\**)\s*(jolt_\w+)\s*\(([^;{}]*?)\)\s*(?=;)", src, flags=re.S):
        stmt_start = max(src.rfind(";", 0, m.start(2)), src.rfind("}", 0, m.start(2))) + 1
        if "typedef" not in src[stmt_start:m.start(2)]:
            decls.append((m.group(2), c_type(m.group(1)), _params(m.group(3))))
    return decls


def parse_callbacks(path=HEADER):
    """every `typedef R (*jolt_x_fn)(...);` -> {name: (ret_type, [(param_name, type)])}"""
    return {m.group(2): (c_type(m.group(1)), _params(m.group(3)))
            for m in re.finditer(r"typedef\s+(\w+)\s*\(\s*\*\s*(jolt_\w+)\s*\)\s*\(([^;{}]*?)\)\s*;", _code(path), flags=re.S)}


def parse_constants(path=HEADER):
    """every member `JOLT_X = n` of the header's enums and every numeric `#define JOLT_X n[u]` -> {name: n}"""
    src = strip_comments(open(path).read())
    out = {}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", src):
        for member in filter(None, (x.strip() for x in body.split(","))):
            name, value = (x.strip() for x in member.split("="))
            out[name] = int(value, 0)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(JOLT_\w+)[ \t]+(\d+)[uU]?[ \t]*$", src, flags=re.M):
        out[name] = int(value)
    return out


def to_ctypes(ctype, callback=False):
    """The ctypes type of a parameter or return.  Pointers to anything and function pointers are c_void_p (it accepts arrays, byref(), handles, CFUNCTYPE instances
    and None alike), a returned `const char *` is c_char_p, scalars keep their exact width.  callback=True types what Python RECEIVES in a callback, where a
    pointer to scalars or to pointers is indexed: POINTER(scalar) / POINTER(c_void_p)."""
    base, consts = ctype
    if not consts:  # (no entry point returns void or takes a struct by value: either would be a KeyError here)
        return C.c_void_p if base in CALLBACKS else SCALARS[base]
    if callback and len(consts) == 2:
        return C.POINTER(C.c_void_p)
    if callback and base in SCALARS and len(consts) == 1:
        return C.POINTER(SCALARS[base])
    return C.c_void_p


def declare(lib):
    """set argtypes and restype on every entry point the header declares; a symbol the library lacks raises AttributeError"""
    for name, ret, params in parse_header():
        fn = getattr(lib, name)
        fn.argtypes = [to_ctypes(t) for _, t in params]
        fn.restype = C.c_char_p if ret == ("char", (True,)) else to_ctypes(ret)


CONSTANTS = parse_constants()
CALLBACKS = parse_callbacks()
CALLBACK_TYPES = {name: C.CFUNCTYPE(to_ctypes(ret), *[to_ctypes(t, callback=True) for _, t in params]) for name, (ret, params) in CALLBACKS.items()}
