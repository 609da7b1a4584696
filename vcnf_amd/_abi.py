"""Reader of ``include/vcnf_hip.h``: the header is the one statement of the C ABI, and ``_lib`` binds what this module
reads from it.  ``read(path, pointer)`` gives

* ``functions``: name -> (argtypes, restype) of every function declaration;
* ``structs``: name -> ``ctypes.Structure`` of every ``typedef struct`` (named by its typedef);
* ``constants``: name -> int of every ``enum { ... }`` entry and every object-like ``#define`` with an integer value;
* ``decls``: name -> (return type, argument types) and ``members``: struct -> [(type, name, array length or None)] as
  the header spells them, from which tests/test_abi.py writes the declarations back for a compiler.

It knows the subset of C the header is written in and nothing more: a declaration it cannot match in full (an unknown
type word, a function pointer, an enumerator without a value, a missing ``;``) raises ``HeaderError`` naming the
declaration.  Nothing is skipped and nothing is guessed.
"""
import ctypes
import re
from collections import namedtuple


class HeaderError(ValueError):
    pass


Abi = namedtuple("Abi", "functions structs constants decls members")


def type_map(pointer):
    """C spelling -> ctypes type of an argument or a return value; ``pointer`` is the class of data pointers.  A pointer
    to a header struct is added by ``read`` as POINTER(that Structure)."""
    return {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double, "const char*": ctypes.c_char_p,
            "float*": pointer, "double*": pointer, "int32_t*": pointer, "int64_t*": pointer, "uint8_t*": pointer,
            "void*": pointer}


_NAME = r"[A-Za-z_]\w*"
_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_DECLARATOR = re.compile(r"(?P<type>(?:const )?%s\*?) ?(?P<name>%s)(?:\[(?P<len>\d+)\])?" % (_NAME, _NAME))
_MORE = re.compile(r"(?P<name>%s)(?:\[(?P<len>\d+)\])?" % _NAME)
_FUNCTION = re.compile(r"(?P<ret>(?:const )?%s\*?) ?(?P<name>%s) ?\((?P<args>[^()]*)\)" % (_NAME, _NAME))
_STRUCT = re.compile(r"typedef struct(?: %s)? ?\{(?P<body>[^{}]*)\} ?(?P<name>%s)" % (_NAME, _NAME))
_ENUM = re.compile(r"enum ?\{(?P<body>[^{}]*)\}")
_DEFINE = re.compile(r"#\s*define\s+(?P<name>%s)(?P<rest>.*)" % _NAME)
_IGNORED = re.compile(r"#\s*(?:include|ifdef|ifndef|endif)\b.*")      # include guards and the extern "C" bracket


def _statements(text):
    """The header's declarations (text up to a ';' outside braces) and its #define lines, comments removed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines, body = [], []
    for line in text.split("\n"):
        if line.lstrip().startswith("#"):
            if line.rstrip().endswith("\\"):
                raise HeaderError("continued preprocessor line: %r" % line.strip())
            if not _IGNORED.fullmatch(line.strip()):
                defines.append(line.strip())
        else:
            body.append(line)
    text = " ".join(body)
    text, n = re.subn(r'extern "C" \{', " ", text)          # its '}' is the header's last brace
    if n:
        text, brace, tail = text.rpartition("}")
        if n != 1 or not brace or tail.strip():
            raise HeaderError('extern "C" bracket not understood')
    text = re.sub(r"\s*\*\s*", "* ", re.sub(r"\s+", " ", text)).strip()
    out, depth, start = [], 0, 0
    for i, c in enumerate(text):
        depth += (c == "{") - (c == "}")
        if c == ";" and depth == 0:
            out.append(text[start:i].strip())
            start = i + 1
    if depth or text[start:].strip():
        raise HeaderError("unterminated declaration: %r" % text[start:].strip()[:120])
    return defines, out


def _declarators(text, what):
    """[(type, name, array length or None)] of 'type a' or 'type a, b[4]' (one type, plain further names)."""
    first, *more = [p.strip() for p in text.split(",")]
    m = _DECLARATOR.fullmatch(first)
    if not m:
        raise HeaderError("%s: cannot read %r" % (what, first))
    ctype = m.group("type")
    found = [m] + [_MORE.fullmatch(p) for p in more]
    if None in found or (more and ctype.endswith("*")):
        raise HeaderError("%s: cannot read %r" % (what, text))
    return [(ctype, f.group("name"), int(f.group("len")) if f.group("len") else None) for f in found]


def _lookup(types, ctype, what):
    """The ctypes type of a C spelling; ``const`` only matters where the map spells it (const char*)."""
    key = ctype if ctype in types else re.sub(r"^const ", "", ctype)
    if key not in types:
        raise HeaderError("%s: unknown type %r" % (what, ctype))
    return types[key]


def read(path, pointer=ctypes.c_void_p):
    with open(path) as f:
        defines, statements = _statements(f.read())
    types = type_map(pointer)
    abi = Abi({}, {}, {}, {}, {})

    def constant(name, value, what):
        if name in abi.constants or not re.fullmatch(_INT, value):
            raise HeaderError("%s: %s is repeated or has no integer value (%r)" % (what, name, value))
        abi.constants[name] = int(value, 0)

    for line in defines:
        m = _DEFINE.fullmatch(line)
        if not m or m.group("rest").startswith("("):
            raise HeaderError("preprocessor line not understood: %r" % line)
        if m.group("rest").strip():                          # an empty one is the include guard
            constant(m.group("name"), m.group("rest").strip(), line)
    for s in statements:
        what = "%r" % s[:120]
        if _ENUM.fullmatch(s):
            for entry in _ENUM.fullmatch(s).group("body").split(","):
                name, eq, value = [p.strip() for p in entry.partition("=")]
                constant(name, value, what)
        elif _STRUCT.fullmatch(s):
            m = _STRUCT.fullmatch(s)
            body = m.group("body").strip()
            if not body.endswith(";"):
                raise HeaderError("%s: a member is not terminated" % what)
            members = [d for part in body[:-1].split(";") for d in _declarators(part.strip(), what)]
            fields = []
            for ctype, name, length in members:
                # a data pointer inside a struct is a plain address: the caller fills it with data_ptr()
                t = _lookup(types, ctype, what)
                t = ctypes.c_void_p if t is pointer else t
                fields.append((name, t * length if length else t))
            name = m.group("name")
            abi.structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": "struct " + name})
            abi.members[name] = members
            types[name + "*"] = ctypes.POINTER(abi.structs[name])
        elif _FUNCTION.fullmatch(s):
            m = _FUNCTION.fullmatch(s)
            args = m.group("args").strip()
            params = [] if args == "void" else [_declarators(a.strip(), what) for a in args.split(",")]
            if any(len(p) != 1 or p[0][2] is not None for p in params) or m.group("name") in abi.functions:
                raise HeaderError("%s: cannot read the parameters, or the function is declared twice" % what)
            ret = m.group("ret")
            spelled = [p[0][0] for p in params]
            abi.decls[m.group("name")] = (ret, spelled)
            abi.functions[m.group("name")] = ([_lookup(types, c, what) for c in spelled], _lookup(types, ret, what))
        else:
            raise HeaderError("declaration not understood: %s" % what)
    return abi
