"""The ctypes binding is derived from include/mobocmf_hip.h (mobocmf_amd/_header.py); here the host C++ compiler checks the
derivation: every struct's size and every field's offset and size, every constant's value, every entry point's arity and
parameter kinds, as the compiler sees the header, against what _lib binds.  CPU-only, nothing links against the library."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from mobocmf_amd import _header, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

_PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include "mobocmf_hip.h"
template <class T> struct Code;                      // a parameter type without a code does not compile
template <class T> struct Code<T*> { static const char* s() { return "P"; } };
#define CODE(T, S) template <> struct Code<T> { static const char* s() { return S; } };
CODE(int32_t, "I4") CODE(int64_t, "I8") CODE(uint32_t, "U4") CODE(uint64_t, "U8") CODE(double, "F8")
template <class F> struct Sig;
template <class... A> struct Sig<int(A...)> {        // decltype of a declaration: unevaluated, nothing is linked
    static void print(const char* name) {
        const char* codes[] = {Code<A>::s()..., 0};
        std::printf("F %s %zu", name, sizeof...(A));
        for (const char** c = codes; *c; ++c) std::printf(" %s", *c);
        std::printf("\n");
    }
};
#define STRUCT(T) std::printf("S %s %zu\n", #T, sizeof(T));
#define FIELD(T, f) std::printf("M %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f));
#define CONSTANT(X) std::printf("C %s %lld\n", #X, (long long)(MOBOCMF_##X));
#define FUNCTION(f) Sig<decltype(f)>::print(#f);
int main() {
@BODY@
    return 0;
}
"""
_CODES = {ctypes.c_int32: "I4", ctypes.c_int64: "I8", ctypes.c_uint32: "U4", ctypes.c_uint64: "U8", ctypes.c_size_t: "U8",
          ctypes.c_double: "F8", ctypes.c_void_p: "P", ctypes.POINTER(ctypes.c_size_t): "P"}


def binding_lines():
    """What _lib binds, one line per fact, in the format of the program below."""
    out = []
    for c_name, cls in _lib.STRUCTS.items():
        out.append(f"S {c_name} {ctypes.sizeof(cls)}")
        out += [f"M {c_name} {f} {getattr(cls, f).offset} {getattr(cls, f).size}" for f, _ in cls._fields_]
    out += [f"C {name} {value}" for name, value in _lib.CONSTANTS.items()]
    out += [" ".join([f"F {name} {len(argtypes)}"] + [_CODES[t] for t in argtypes]) for name, argtypes in _lib.SYMBOLS.items()]
    return out


def compiler_lines(include_dir, tmp_path):
    """The same facts from the host compiler, for the names _lib publishes."""
    body = []
    for c_name, cls in _lib.STRUCTS.items():
        body.append(f"STRUCT({c_name})")
        body += [f"FIELD({c_name}, {f})" for f, _ in cls._fields_]
    body += [f"CONSTANT({name})" for name in _lib.CONSTANTS] + [f"FUNCTION({name})" for name in _lib.SYMBOLS]
    src, exe = tmp_path / "abi.cpp", tmp_path / "abi"
    src.write_text(_PROGRAM.replace("@BODY@", "\n".join("    " + line for line in body)))
    cxx = next((c for c in ("c++", "g++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, ROCm's clang++)"
    subprocess.run([cxx, "-std=c++11", "-I", str(include_dir), str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_the_binding_is_the_compilers_view_of_the_header(tmp_path):
    want, got = compiler_lines(INCLUDE, tmp_path), binding_lines()
    assert got == want, [pair for pair in zip(got, want) if pair[0] != pair[1]][:10]
    assert all(getattr(_lib.load(), n).restype is ctypes.c_int for n in _lib.SYMBOLS)
    # the constants are published under their own names, the error names come from the enum
    assert all(getattr(_lib, name) == value for name, value in _lib.CONSTANTS.items())
    assert _lib._ERR[_lib.BAD_ARCH] == "MOBOCMF_BAD_ARCH" and sorted(_lib._ERR) == list(range(6))
    assert _lib.Tuning.KNOBS[0] == "small_gemm_max" and _lib.RffRefineOptions.KNOBS[0] == "outer" and _lib.NsgaOptions.KNOBS[0] == "eta_c"
    assert isinstance(_lib.Tuning().copy(), _lib.Tuning)


def test_the_reader_drops_no_declaration():
    """The names above are the reader's; the counts here are an independent regex's over the raw header."""
    hdr = open(os.path.join(INCLUDE, "mobocmf_hip.h")).read()
    assert len(re.findall(r"^typedef struct\b", hdr, flags=re.M)) == len(_lib.STRUCTS) == 13
    defines = re.findall(r"^#define (MOBOCMF_\w+)[ \t]+[^\s/]", hdr, flags=re.M)
    members = [m for body in re.findall(r"^enum \{(.*?)\};", hdr, flags=re.M | re.S) for m in re.findall(r"(MOBOCMF_\w+)\s*=", body)]
    assert len(defines) + len(members) == len(_lib.CONSTANTS) and len(members) == 6
    assert {n[len("MOBOCMF_"):] for n in defines + members} == set(_lib.CONSTANTS)
    assert len(re.findall(r"^int mobocmf_", hdr, flags=re.M)) == len(_lib.SYMBOLS)


_GOOD = """
#ifndef MOBOCMF_HIP_H
#define MOBOCMF_HIP_H
typedef void* mobocmf_stream_t;
#define MOBOCMF_N 3      /* a bound */
#define MOBOCMF_BIG (2147483648LL + (1 << 4) * MOBOCMF_N)
enum { MOBOCMF_OK = 0, MOBOCMF_BAD = 1 };
typedef struct mobocmf_a { uint32_t size; int32_t p, q[MOBOCMF_N]; } mobocmf_a;
typedef struct {
    const struct mobocmf_later* later;   /* not complete here */
    const mobocmf_a* a; mobocmf_a as[2];
    double* raw[MOBOCMF_N][7];
    void* const* events;
} mobocmf_b;
int mobocmf_version(void);
int mobocmf_f(const mobocmf_b* b, const double* const* x, int64_t n, uint64_t seed, double s,
              size_t* bytes, size_t given, mobocmf_stream_t stream);
#endif
"""


def test_the_reader_reads_the_forms_the_header_uses():
    h = _header.Header(_GOOD)
    assert h.constants == {"N": 3, "BIG": 2147483648 + 48, "OK": 0, "BAD": 1} and h.enum == ["OK", "BAD"]
    classes = {}
    for c_name in h.structs:
        classes[c_name] = type(c_name, (ctypes.Structure,), {"_fields_": h.fields(c_name, classes)})
    A, P = classes["mobocmf_a"], ctypes.c_void_p
    assert A._fields_ == [("size", ctypes.c_uint32), ("p", ctypes.c_int32), ("q", ctypes.c_int32 * 3)]
    assert classes["mobocmf_b"]._fields_ == [("later", P), ("a", ctypes.POINTER(A)), ("as", A * 2), ("raw", (P * 7) * 3), ("events", P)]
    assert h.functions == {"mobocmf_version": [], "mobocmf_f": [P, P, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double,
                                                                ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t, P]}


@pytest.mark.parametrize("old, new, message", [
    ("uint32_t size;", "float size;", "unknown field type"),
    ("uint32_t size;", "unsigned int size;", "unknown field type"),
    ("uint32_t size;", "uint32_t size : 8;", "declarator"),
    ("q[MOBOCMF_N]", "q[n]", "not an integer constant"),
    ("q[MOBOCMF_N]", "q[MOBOCMF_LATER]", "not an integer constant"),
    ("mobocmf_a as[2];", "mobocmf_c as[2];", "unknown field type"),
    ("const mobocmf_a* a;", "const mobocmf_a* a, b;", "several declarators"),
    ("mobocmf_a as[2];", "union { int32_t i; double d; } u;", "typedef struct"),
    ("#define MOBOCMF_N 3 ", "#define MOBOCMF_N 3.5 ", "not an integer constant"),
    ("#define MOBOCMF_N 3 ", '#define MOBOCMF_N "three" ', "not an integer constant"),
    ("#define MOBOCMF_N 3 ", "#define MOBOCMF_N 3\n#define MOBOCMF_TWICE(x) (2 * (x))", "cannot read"),
    ("MOBOCMF_BAD = 1", "MOBOCMF_BAD", "enum member"),
    ("enum {", "enum mobocmf_code {", "cannot read"),
    ("double s,", "float s,", "cannot read the parameter 'float s'"),
    ("int64_t n,", "long n,", "cannot read the parameter 'long n'"),
    ("int64_t n,", "int64_t,", "cannot read the parameter"),
    ("size_t given,", "void (*done)(int32_t),", "cannot read: 'int mobocmf_f"),
    ("mobocmf_stream_t stream);", "mobocmf_stream_t stream)", "cannot read: 'int mobocmf_f"),
])
def test_the_reader_refuses_what_it_cannot_read(old, new, message):
    assert old in _GOOD
    with pytest.raises(_header.HeaderError, match=re.escape(message)):
        _header.Header(_GOOD.replace(old, new))


def test_a_missing_header_is_named(tmp_path):
    path = str(tmp_path / "include" / "mobocmf_hip.h")
    with pytest.raises(_lib.MobocmfError, match=re.escape(path)):
        _lib.read_header(path)
    assert _lib.HEADER_PATH == os.path.join(INCLUDE, "mobocmf_hip.h")
