"""The Python binding (pve_mcc_amd/_capi.py) against the four public headers, in both directions.

Binding -> header: `checks(binding)` writes one C++ translation unit that includes the headers and holds a static_assert for
every Structure (sizeof; each field's offsetof, size and, for a scalar, class), every row of _capi.PROTOTYPES (arity, the
result's class, each argument's class), every integer constant and every position of a name tuple; `compile_checks` hands it to
the compiler of tests/native.mk with -fsyntax-only.  A class is what ctypes can express: a pointer, a signed or unsigned integer
of a size, float, double, void.  Constness and pointee types are not checked, and cannot be from here.
Header -> binding: the compiler cannot enumerate, so `declared(header)` reads the comment-stripped text: the pve_*( prototypes,
the `typedef struct pve_x {` bodies, the object-like PVE_* macros with a value and the enumerators.  Function-like macros
(PVE_LEARNER_WIDE_FLOATS, which tests/test_learner_wide.py holds learner.wide_floats to) are out of scope.

Naming: Structure PveArrivalGen is pve_arrival_gen; an upper-case integer of _capi is the header's name with or without PVE_;
position k of ENV_OUT_NAMES / METRIC_NAMES / LAUNCH_NAMES / stats.STAT_NAMES is PVE_EO_ / PVE_M_ / PVE_LAUNCH_ / PVE_STAT_<NAME> = k."""
import ctypes as C
import os
import re
import subprocess
import types

from pve_mcc_amd import _capi, stats

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INCLUDE = os.path.join(ROOT, "include")
NAME_TUPLES = {"PVE_EO_": "ENV_OUT_NAMES", "PVE_M_": "METRIC_NAMES", "PVE_LAUNCH_": "LAUNCH_NAMES", "PVE_STAT_": "STAT_NAMES"}

PRELUDE = """#include <cstddef>
#include <tuple>
#include <type_traits>
%s
template <class T, bool = std::is_integral<T>::value> struct kind {
    static constexpr int v = std::is_void<T>::value ? 0 : std::is_pointer<T>::value ? 1 : std::is_same<T, float>::value ? 2
                             : std::is_same<T, double>::value ? 3 : -1; };
template <class T> struct kind<T, true> { static constexpr int v = (std::is_signed<T>::value ? 10 : 20) + (int) sizeof(T); };
template <class F> struct sig;
template <class R, class... A> struct sig<R(A...)> {
    static constexpr int arity = sizeof...(A), result = kind<R>::v;
    template <int K> using arg = typename std::tuple_element<K, std::tuple<A...>>::type; };
"""


def binding(**doctored):
    """The binding as the generator reads it: _capi's names (and stats.STAT_NAMES), with `doctored` ones replaced"""
    return types.SimpleNamespace(**dict(vars(_capi), STAT_NAMES=stats.STAT_NAMES, **doctored))


def c_name(structure):
    return re.sub(r"(?<!^)([A-Z])", r"_\1", structure).lower()


def structures(b):
    return {n: t for n, t in vars(b).items() if isinstance(t, type) and issubclass(t, C.Structure) and t is not C.Structure}


def constants(b):
    """header name -> (binding name, value)"""
    return {(n if n.startswith("PVE_") else "PVE_" + n): (n, v) for n, v in vars(b).items() if n.isupper() and type(v) is int}


def tuple_positions(b):
    """header name -> (tuple name, k)"""
    return {prefix + name.upper(): (tup, k) for prefix, tup in NAME_TUPLES.items() for k, name in enumerate(getattr(b, tup))}


def kind(t):
    """(class code of the C++ `kind`, words for it) of a ctypes type; (None, ...) for arrays and nested structures"""
    if t is None:
        return 0, "void"
    if issubclass(t, (C._Pointer, C.c_void_p, C.c_char_p)):
        return 1, "a pointer"
    if not issubclass(t, C._SimpleCData):
        return None, t.__name__
    if t._type_ in "fd":
        return (2, "float") if t._type_ == "f" else (3, "double")
    signed = t._type_ in "bhilq"
    assert signed or t._type_ in "BHILQ", t
    return (10 if signed else 20) + C.sizeof(t), "%s %d-byte integer" % ("a signed" if signed else "an unsigned", C.sizeof(t))


def checks(b):
    """The translation unit: what `b` states, as static_asserts against the headers"""
    out = [PRELUDE % "\n".join('#include "%s"' % h for h in b.PROTOTYPES)]

    def add(cond, text):
        out.append('static_assert(%s, "%s in the binding");' % (cond, text))

    for name, t in structures(b).items():
        c = c_name(name)
        add("sizeof(%s) == %d" % (c, C.sizeof(t)), "%s: sizeof %d" % (name, C.sizeof(t)))
        for field, ft in t._fields_:
            d = getattr(t, field)
            add("offsetof(%s, %s) == %d" % (c, field, d.offset), "%s.%s: offset %d" % (name, field, d.offset))
            add("sizeof(%s::%s) == %d" % (c, field, d.size), "%s.%s: %d bytes" % (name, field, d.size))
            code, words = kind(ft)
            if code is not None:
                add("kind<decltype(%s::%s)>::v == %d" % (c, field, code), "%s.%s: %s" % (name, field, words))
    for group in b.PROTOTYPES.values():
        for name, (restype, argtypes) in group.items():
            s = "sig<decltype(%s)>" % name
            add("%s::arity == %d" % (s, len(argtypes)), "%s: %d arguments" % (name, len(argtypes)))
            add("%s::result == %d" % (s, kind(restype)[0]), "%s: the result is %s" % (name, kind(restype)[1]))
            for k, t in enumerate(argtypes):
                add("kind<%s::arg<%d>>::v == %d" % (s, k, kind(t)[0]), "%s: argument %d is %s" % (name, k, kind(t)[1]))
    for header_name, (name, v) in constants(b).items():
        add("%s == %d" % (header_name, v), "%s = %d" % (name, v))
    for header_name, (tup, k) in tuple_positions(b).items():
        add("%s == %d" % (header_name, k), "%s[%d] = '%s'" % (tup, k, getattr(b, tup)[k]))
    return "\n".join(out) + "\n"


def compile_checks(source, include=INCLUDE):
    """-> (exit status, the compiler's messages)"""
    p = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-fsyntax-only", "-I", include, "-x", "c++", "-"],
                       input=source, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


def declared(header, include=INCLUDE):
    """What a header declares, by kind: prototypes, structs, macros (name -> value text), enumerators"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(include, header)).read(), flags=re.S)
    enums = [e.split("=")[0].strip() for body in re.findall(r"\benum\s*\{(.*?)\}", src, flags=re.S) for e in body.split(",")]
    return types.SimpleNamespace(prototypes=sorted(set(re.findall(r"\b(pve_[a-z0-9_]+)\s*\(", src))),
                                 structs=re.findall(r"typedef\s+struct\s+(pve_\w+)\s*\{", src),
                                 macros=dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PVE_\w+)[ \t]+(\S+)", src, flags=re.M)),
                                 enumerators=[e for e in enums if e])
