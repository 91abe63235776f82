"""The C ABI read off include/air_hip.h and compared with its ctypes mirror air/_hip.py (tests/test_abi.py), and the two
helpers every test file that talks to the library shares: hip() builds and binds it, host_ptr() is an address to pass.

The header is regular enough to read with regular expressions: names come from them (struct types and their fields in
order, AIR_* constants, prototypes); every NUMBER -- sizeof, offsetof, the value of a constant -- comes from one gcc
compile of a generated C program."""
import collections
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "air_hip.h")

Header = collections.namedtuple("Header", "structs constants prototypes")   # {type: [field]}, [name], {fn: (ret, [param type])}
Numbers = collections.namedtuple("Numbers", "sizeof fields values")           # {type: n}, {(type, field): (offset, size)}, {name: v}


def hip(build=True):
    """air._hip with the library bound; build: made first (a no-op when it is newer than its sources)"""
    if build:
        import importlib.util
        spec = importlib.util.spec_from_file_location("air_build", os.path.join(ROOT, "tf-attend-infer-repeat_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    from air import _hip
    _hip.lib()
    return _hip


def gpu_hip():
    """hip() of the GPU tests: the library as it was built, or a skip where there is no device"""
    import pytest
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return hip(build=False)


_HOST = (C.c_char * 272)()


def host_ptr():
    """a 16-byte aligned non-null address (never dereferenced: the calls that take it return before a launch)"""
    base = C.addressof(_HOST)
    return C.c_void_p(base + (-base) % 16)


# ---- reading the header -------------------------------------------------------------------------------------------------
def _declarators(decls):
    """'const float* A; int32_t M, N' -> [('const float*', 'A'), ('int32_t', 'M'), ('int32_t', 'N')]"""
    out = []
    for decl in filter(None, (d.strip() for d in decls.split(";"))):
        first, *more = [p.strip() for p in decl.split(",")]
        ctype, name = re.fullmatch(r"(.*?)(\w+)", first, re.S).groups()
        out += [(" ".join(ctype.split()), n) for n in [name] + more]
    return out


def read_header(path=HEADER):
    src = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    constants = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(AIR_\w+)[ \t]+\S", src, flags=re.M)
    src = re.sub(r"^[ \t]*#.*$", "", src, flags=re.M)
    for body in re.findall(r"\benum\s*\{(.*?)\}", src, flags=re.S):
        constants += re.findall(r"\b(AIR_\w+)\s*=", body)
    structs = {name: [f for _, f in _declarators(body)]
               for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(air_\w+_t)\s*;", src, flags=re.S)}
    src = re.sub(r"(typedef\s+struct|enum)\s*\{.*?\}[^;]*;", "", src, flags=re.S)
    prototypes = {}
    for ret, name, params in re.findall(r"([\w \t\*]+?)\b(air_\w+)\s*\(([^)]*)\)\s*;", src):
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        prototypes[name] = (" ".join(ret.split()), [p if p.endswith("*") else re.sub(r"\s*\w+$", "", p) for p in params])
    return Header(structs, constants, prototypes)


@functools.lru_cache(maxsize=None)
def compile_numbers(path=HEADER):
    """sizeof of every struct, offsetof and sizeof of every field, the value of every constant: one gcc compile"""
    h = read_header(path)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.abspath(path), 'int main(void) {']
    for s, fields in h.structs.items():
        lines.append('printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f) for f in fields]
    lines += ['printf("V %s %%lld\\n", (long long)(%s));' % (c, c) for c in h.constants]
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as tmp:
        prog, exe = os.path.join(tmp, "abi.c"), os.path.join(tmp, "abi")
        open(prog, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", prog, "-o", exe])
        out = subprocess.check_output([exe]).decode().splitlines()
    n = Numbers({}, {}, {})
    for kind, *rest in (ln.split() for ln in out):
        if kind == "S":
            n.sizeof[rest[0]] = int(rest[1])
        elif kind == "F":
            n.fields[rest[0], rest[1]] = (int(rest[2]), int(rest[3]))
        else:
            n.values[rest[0]] = int(rest[1])
    return n


# ---- the comparison -----------------------------------------------------------------------------------------------------
def camel(ctype):
    """air_attend_fwd_t -> AttendFwd"""
    return "".join(w.capitalize() for w in ctype[len("air_"):-len("_t")].split("_"))


def mirrors(binding):
    return {k: v for k, v in vars(binding).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}


def constants(binding):
    return {k: v for k, v in vars(binding).items() if k.isupper() and isinstance(v, int) and not isinstance(v, bool)}


def check_structs(h, num, binding):
    """the same set of types, the same field names in order, the same sizeof; per field the same offset and size"""
    bad, mir = [], mirrors(binding)
    want = {camel(s): s for s in h.structs}
    bad += ["%s: in the header, no Structure %s in the binding" % (want[k], k) for k in sorted(set(want) - set(mir))]
    bad += ["%s: a Structure of the binding, no such air_*_t in the header" % k for k in sorted(set(mir) - set(want))]
    for k in sorted(set(want) & set(mir)):
        s, cls = want[k], mir[k]
        names = [f[0] for f in cls._fields_]
        if names != h.structs[s]:
            i = next((i for i, (a, b) in enumerate(zip(h.structs[s], names)) if a != b), min(len(names), len(h.structs[s])))
            bad.append("%s: field %d is %s in the header, %s in %s" % (s, i, (h.structs[s] + ["nothing"])[i], (names + ["nothing"])[i], k))
        if num.sizeof[s] != C.sizeof(cls):
            bad.append("%s: sizeof %d in C, %d in %s" % (s, num.sizeof[s], C.sizeof(cls), k))
        for name, ftype, *_ in cls._fields_:
            if (s, name) in num.fields and num.fields[s, name] != (getattr(cls, name).offset, C.sizeof(ftype)):
                bad.append("%s.%s: (offset, size) %s in C, %s in %s" % ((s, name, num.fields[s, name],
                                                                         (getattr(cls, name).offset, C.sizeof(ftype)), k)))
    return bad


def check_constants(h, num, binding):
    """every upper-case integer X of the binding is AIR_X of the header, with the value C gives it -- no exceptions"""
    return ["%s = %d: %s" % (k, v, "the header has no AIR_" + k if "AIR_" + k not in num.values else
                             "AIR_%s is %d in the header" % (k, num.values["AIR_" + k]))
            for k, v in sorted(constants(binding).items()) if num.values.get("AIR_" + k) != v]


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
            "double": C.c_double, "const char*": C.c_char_p, "char*": C.c_char_p}


def ctypes_of(ctype, h, binding, returned=False):
    """what a C type may be bound as.  A pointer to a bound struct: POINTER(its mirror), or c_void_p where the argument is a
    DEVICE array of descriptors (ctypes would take a host Structure for it); a double*: POINTER(c_double) or c_void_p;
    every other pointer, the trailing void* stream among them: c_void_p"""
    if ctype in _SCALARS and (returned or ctype != "const char*"):
        return (_SCALARS[ctype],)
    if not ctype.endswith("*"):
        return ()
    base = ctype[:-1].replace("const", "").strip()
    if base in h.structs and camel(base) in mirrors(binding):
        return (C.POINTER(mirrors(binding)[camel(base)]), C.c_void_p)
    return (C.POINTER(C.c_double), C.c_void_p) if base == "double" else (C.c_void_p,)


def check_signatures(h, binding):
    """the same set of functions; per function the restype and, element by element, the argtypes the prototype gives"""
    bad, rows = [], binding._SIGNATURES
    bad += ["%s: declared in the header, no _SIGNATURES row" % k for k in sorted(set(h.prototypes) - set(rows))]
    bad += ["%s: a _SIGNATURES row, not declared in the header" % k for k in sorted(set(rows) - set(h.prototypes))]
    for k in sorted(set(rows) & set(h.prototypes)):
        (ret, params), (res, args) = h.prototypes[k], rows[k]
        if res not in ctypes_of(ret, h, binding, returned=True):
            bad.append("%s: returns %s, bound as %s" % (k, ret, getattr(res, "__name__", res)))
        if len(params) != len(args):
            bad.append("%s: %d parameters in the header, %d argtypes" % (k, len(params), len(args)))
        bad += ["%s: argument %d is %s, bound as %s" % (k, i, p, a.__name__)
                for i, (p, a) in enumerate(zip(params, args)) if a not in ctypes_of(p, h, binding)]
    return bad


def check_abi(binding, path=HEADER):
    """every mismatch between the header at `path` and `binding` (air._hip, or a patched copy of it), each naming its item"""
    h, num = read_header(path), compile_numbers(path)
    return check_structs(h, num, binding) + check_constants(h, num, binding) + check_signatures(h, binding)
