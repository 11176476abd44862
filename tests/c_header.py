"""The one reader of the C headers under include/ for the tests that compare them with rware_amd._capi (test_capi_boundary.py,
test_capi_parts.py, test_capi_symbols.py): comment stripping, the prototypes, structures and enums of a header's text, the two sides'
types brought to one vocabulary ("pointer" or a ctypes scalar), and the strict C11 compile of a caller."""
import collections
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "char": C.c_char,
           "float": C.c_float}
GCC = ["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INCLUDE]
Prototype = collections.namedtuple("Prototype", "name ret args arg_texts")


def strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def read(name):
    """The text of include/<name> without its comments."""
    return strip(open(os.path.join(INCLUDE, name)).read())


def c_class(decl):
    """A C declarator without its name ("const int32_t *", "uint64_t", "char [16]") -> "pointer" or the ctypes scalar type."""
    if "*" in decl or "[" in decl:
        return "pointer"
    return SCALARS[" ".join(w for w in decl.split() if w != "const")]


def ctypes_class(t):
    return "pointer" if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer) else t


def prototypes(text):
    """[Prototype] of every rw_* function a header text declares, in order: the return and argument classes (c_class) and the arguments as
    written."""
    out = []
    for ret, name, args in re.findall(r"([A-Za-z_0-9 \*]+?)\b(rw_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        texts = [] if args.strip() == "void" else [a.strip() for a in args.split(",")]
        out.append(Prototype(name, c_class(ret), [c_class(re.sub(r"\b[A-Za-z_0-9]+\s*(\[\d*\])?\s*$", r"\1", a)) for a in texts], texts))
    return out


def struct(text, name):
    """(number of declarations, [(field, element ctypes type or "pointer", array length or None)]) of `typedef struct name { ... } name;`,
    comma lists expanded."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    fields = []
    for d in decls:
        first, *more = [p.strip() for p in d.split(",")]
        base = re.match(r"((?:const\s+)?[A-Za-z_0-9]+)\s", first).group(1)
        for declarator in [first[len(base):]] + more:
            m = re.fullmatch(r"\s*(\*?)\s*([A-Za-z_0-9]+)\s*(?:\[(\d+)\])?", declarator)
            fields.append((m.group(2), "pointer" if m.group(1) else c_class(base), int(m.group(3)) if m.group(3) else None))
    return len(decls), fields


def enum(text, name):
    body = re.search(r"enum %s \{(.*?)\};" % name, text, flags=re.S).group(1)
    return {n: int(v) for n, v in re.findall(r"\b(RW_[A-Z_0-9]+)\s*=\s*(-?\d+)", body)}


def gcc(*args):
    """`gcc -std=c11 -Wall -Wextra -pedantic -Werror -fsyntax-only -I include` on these arguments -> the CompletedProcess."""
    return subprocess.run(GCC + [str(a) for a in args], capture_output=True, text=True)
