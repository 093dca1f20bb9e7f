"""Reader of include/mobocmf_hip.h: the header is the one statement of the C-ABI, _lib derives its ctypes binding from it.

Not a C parser.  It reads the three declaration forms the header uses -- integer constants (#define MOBOCMF_X <expression>
and the anonymous enum), `typedef struct [tag] { ... } name;` and `int mobocmf_name(args);` -- and raises HeaderError on a
declaration of these kinds that it could not consume, so nothing is ever bound from a guess.
"""
import ctypes
import re


class HeaderError(ValueError):
    pass


SCALARS = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_PREFIX = "MOBOCMF_"
_COMMENT = re.compile(r"/\*[^*]*\*+(?:[^/*][^*]*\*+)*/|//[^\n]*")      # unrolled: four times faster than /\*.*?\*/ here
_DEFINE = re.compile(r"^#define MOBOCMF_(\w+)[ \t]+(\S.*)$", re.M)
_ENUM = re.compile(r"^enum\s*\{([^{}]*)\}\s*;", re.M)
_STRUCT = re.compile(r"^typedef struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", re.M)
_PROTO = re.compile(r"^int (mobocmf_\w+)\s*\(([^()]*)\)\s*;", re.M)
_UNREAD = re.compile(r"^#define MOBOCMF_\w+[^\w\n][^\n]*\S|\benum\b.*|\btypedef struct\b.*|^int mobocmf_.*", re.M)
_TYPE = r"(?:const\s+)?(?:struct\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)"      # base type, its stars
_FIELD = re.compile(_TYPE + r"(.+)", re.S)
_DECLARATOR = re.compile(r"(\w+)\s*((?:\[[^\[\]]+\]\s*)*)")
_PARAM = re.compile(_TYPE + r"\w+")
_INTEGER = re.compile(r"(?:\d+|<<|[()+*\s])+")


class Header:
    """constants: name (without MOBOCMF_) -> int, the enum's members included (`enum` names those); structs: C name ->
    [(field, base type, is a pointer, array bounds)]; functions: name -> argtypes.  All in the header's order."""

    def __init__(self, text):
        self.constants, self.enum, self.structs, self.functions = {}, [], {}, {}
        text = _COMMENT.sub(" ", text)
        for pattern, read in ((_DEFINE, self._define), (_ENUM, self._enum), (_STRUCT, self._struct), (_PROTO, self._proto)):
            text = pattern.sub(read, text)
        left = _UNREAD.search(text)
        if left:
            raise HeaderError(f"a declaration the binding cannot read: {left.group().strip()!r}")

    def value(self, expr):
        """An integer expression of literals, ( ) + * << and constants already read."""
        if expr.strip().isdigit():
            return int(expr)
        known = lambda m: str(self.constants.get(m.group(1), m.group()))
        s = re.sub(r"\b(\d+)(?:U?LL?|U)\b", r"\1", re.sub(r"\bMOBOCMF_(\w+)", known, expr))
        if not _INTEGER.fullmatch(s) or "**" in s:
            raise HeaderError(f"not an integer constant expression: {expr.strip()!r}")
        try:
            return int(eval(s, {"__builtins__": {}}))
        except Exception as e:
            raise HeaderError(f"not an integer constant expression: {expr.strip()!r}") from e

    def _define(self, m):
        self.constants[m.group(1)] = self.value(m.group(2))
        return ""

    def _enum(self, m):
        for member in filter(None, (s.strip() for s in m.group(1).split(","))):
            name, eq, expr = member.partition("=")
            if not (eq and name.strip().startswith(_PREFIX)):
                raise HeaderError(f"an enum member without MOBOCMF_ or without a value: {member!r}")
            self.enum.append(name.strip()[len(_PREFIX):])
            self.constants[self.enum[-1]] = self.value(expr)
        return ""

    def _struct(self, m):
        fields = []
        for decl in filter(None, (s.strip() for s in m.group(1).split(";"))):
            f = _FIELD.fullmatch(decl)
            if not f:
                raise HeaderError(f"{m.group(2)}: cannot read the field {decl!r}")
            base, stars, declarators = f.groups()
            if stars and base not in self.structs:
                base = "void"           # the pointee's layout is not this struct's business (or not declared yet)
            elif not stars and base not in SCALARS and base not in self.structs:
                raise HeaderError(f"{m.group(2)}: unknown field type in {decl!r}")
            if stars and "," in declarators:
                raise HeaderError(f"{m.group(2)}: several declarators after a pointer type in {decl!r}")
            for item in declarators.split(","):
                d = _DECLARATOR.fullmatch(item.strip())
                if not d:
                    raise HeaderError(f"{m.group(2)}: cannot read the declarator {item.strip()!r} of {decl!r}")
                fields.append((d.group(1), base, bool(stars), [self.value(b) for b in re.findall(r"\[([^\[\]]+)\]", d.group(2))]))
        self.structs[m.group(2)] = fields
        return ""

    def _proto(self, m):
        argtypes = []
        for param in [] if m.group(2).strip() == "void" else (p.strip() for p in m.group(2).split(",")):
            p = _PARAM.fullmatch(param)
            base, stars = p.groups() if p else (None, None)
            if stars:       # host or device, the header cannot say: an address.  Every size_t* is a host out-parameter.
                argtypes.append(ctypes.POINTER(ctypes.c_size_t) if (base, stars.strip()) == ("size_t", "*") else ctypes.c_void_p)
            elif base == "mobocmf_stream_t":
                argtypes.append(ctypes.c_void_p)
            elif base in SCALARS:
                argtypes.append(SCALARS[base])
            else:
                raise HeaderError(f"{m.group(1)}: cannot read the parameter {param!r}")
        self.functions[m.group(1)] = argtypes
        return ""

    def fields(self, c_name, classes):
        """The ctypes _fields_ of struct c_name; `classes` holds the Structure classes of the header structs before it.  A
        pointer to a struct that was complete at that point is POINTER(its class), every other pointer c_void_p."""
        out = []
        for name, base, pointer, bounds in self.structs[c_name]:
            t = classes[base] if base in self.structs else ctypes.c_void_p if base == "void" else SCALARS[base]
            if pointer and base != "void":
                t = ctypes.POINTER(t)
            for n in reversed(bounds):
                t = t * n
            out.append((name, t))
        return out
