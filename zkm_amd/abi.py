"""include/zkm_hip.h, read once: its prototypes, structs and integer constants, for the ctypes binding (zkm_amd.load) and the ABI lock
(tests/test_abi.py).  The header is the only statement of the C ABI; what is read here is judged by the C compiler (the layout probe
below), the linker (`nm -D` of libzkmhip.so) and the hand-written Rust block.  The reader knows the few statement forms the header
uses; anything else raises ZkmError naming the line, so a new construct is an error at load and never a silently different binding."""
import functools
import os
import re

from . import ZkmError

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zkm_hip.h")

_NAME = r"[A-Za-z_]\w*"
_SPACE = re.compile(r"\s*")
_STATEMENT = re.compile(r"""\s*(?:
      \#[ \t]*define[ \t]+(?P<define>ZKM_\w+)[ \t]*(?P<value>[^\n]*)           # a constant (or the include guard: no value)
    | \#[^\n]*                                                                   # #include, #if.., #endif
    | extern\s+"C"\s*\{ | \}                                                      # the C++ guard's braces
    | typedef\s+struct\s+(?P<opaque>\w+)\s+(?P=opaque)\s*;                        # an opaque handle
    | typedef\s+struct\s*(?P<tag>\w*)\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;
    | struct\s+(?P<tagged>zkm_\w+)\s*\{(?P<tbody>[^{}]*)\}\s*;                  # a tagged struct (no typedef): `struct zkm_x` in prototypes
    | struct\s+(?P<handle>zkm_\w+)\s*;                                          # a tagged handle that is only declared
    | (?P<ret>[\w\s*]+?)\b(?P<fn>zkm_\w+)\s*\((?P<params>[^()]*)\)\s*;            # a prototype
    )""", re.X)


def _type(text):
    """C type text in the header's own spelling: one space between words, every `*` attached to the left."""
    return re.sub(r"\s*\*", "*", " ".join(text.split()))


def _declarator(text, where):
    """`const uint64_t* const* cols` -> (type, name, None); `uint64_t state_out[12]` -> (type, name, "12").  A struct's second
    declarator (`, n_out`) has an empty type."""
    m = re.fullmatch(r"\s*(.*?)\b(%s)\s*(?:\[(\w+)\])?\s*" % _NAME, text, flags=re.S)
    if not m or (m.group(1).strip() and not re.fullmatch(r"[\w\s*]+", m.group(1))):
        raise ZkmError("%s: cannot read the declaration %r" % (where, " ".join(text.split())))
    return _type(m.group(1)), m.group(2), m.group(3)


def _fields(body, where):
    """The field names of a struct's body, in order."""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *rest = decl.split(",")
        fields += [_declarator(first, where)[1]] + [_declarator(r, where)[1] for r in rest]
    return fields


@functools.lru_cache(maxsize=None)
def _parse():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), raw, flags=re.S)   # comments -> blanks: lines keep their numbers
    protos, structs, opaque, consts, tagged, handles = [], {}, [], {}, {}, []
    pos, end = 0, len(text.rstrip())
    while pos < end:
        m = _STATEMENT.match(text, pos)
        where = "zkm_hip.h:%d" % (text.count("\n", 0, _SPACE.match(text, pos).end()) + 1)
        if not m:
            raise ZkmError("%s: a statement this reader does not know: %r" % (where, " ".join(text[pos:].split())[:80]))
        pos = m.end()
        if m.group("define") and m.group("value").strip():
            v = re.fullmatch(r"(0[xX][0-9a-fA-F]+|\d+)(?:u|ULL)?", m.group("value").strip())
            if not v or consts.get(m.group("define"), int(v.group(1), 0)) != int(v.group(1), 0):
                raise ZkmError("%s: %s is not one integer" % (where, m.group("define")))
            consts[m.group("define")] = int(v.group(1), 0)
        elif m.group("opaque"):
            opaque.append(m.group("opaque"))
        elif m.group("struct"):
            if m.group("tag") not in ("", m.group("struct")):
                raise ZkmError("%s: struct tag %s differs from its typedef %s" % (where, m.group("tag"), m.group("struct")))
            structs[m.group("struct")] = _fields(m.group("body"), where)
        elif m.group("tagged"):
            tagged[m.group("tagged")] = _fields(m.group("tbody"), where)
        elif m.group("handle"):
            handles.append(m.group("handle"))
        elif m.group("fn"):
            # a pointer to a tagged struct or handle is a plain address to the bindings: `struct zkm_x` reads as `void`
            def address(t):
                if t.group(1) not in tagged and t.group(1) not in handles:
                    raise ZkmError("%s: %s names struct %s before its declaration" % (where, m.group("fn"), t.group(1)))
                return "void"
            plain = re.sub(r"\bstruct\s+(\w+)", address, m.group("params"))
            params = [] if plain.strip() == "void" else [_declarator(p, where) for p in plain.split(",")]
            if any(not ty for ty, _, _ in params):
                raise ZkmError("%s: %s has a parameter without a type or a name" % (where, m.group("fn")))
            protos.append((m.group("fn"), _type(m.group("ret")), [(ty + "*" if arr else ty, name) for ty, name, arr in params]))
    return protos, structs, opaque, consts, tagged, handles


def prototypes():
    """[(name, return type, [(parameter type, parameter name)])] in the header's order; an array parameter is a pointer."""
    return _parse()[0]


def structs():
    """{struct: [field names in order]} of every `typedef struct {` / `typedef struct tag {`."""
    return _parse()[1]


def opaque():
    """The handles that are only ever declared (`typedef struct zkm_ctx zkm_ctx;`)."""
    return _parse()[2]


def tagged():
    """{struct: [field names in order]} of every `struct zkm_x { ... };` (tagged, no typedef: prototypes spell it `struct zkm_x`, which
    prototypes() reports as `void` -- to the bindings a pointer to one is a plain address; tests/test_calls_entry_abi.py locks them)."""
    return _parse()[4]


def tagged_handles():
    """The tagged handles that are only ever declared (`struct zkm_x;`); `void` in prototypes() like the tagged structs."""
    return _parse()[5]


def constants(prefix=""):
    """{name: value} of every `#define ZKM_* <integer>`; with a prefix, the names that begin with it, without it."""
    return {k[len(prefix):]: v for k, v in _parse()[3].items() if k.startswith(prefix)}


def layout_probe_source(of_tagged=False):
    """A C99 program that prints {"struct": {"size", "align", "fields": [[name, offset, size]]}} for every struct of the header (of_tagged:
    for every tagged struct, under its tag), as JSON."""
    out = ["#include <stddef.h>", "#include <stdio.h>", '#include "%s"' % HEADER, "int main(void) {", '    printf("{");']
    for i, (name, fields) in enumerate((tagged() if of_tagged else structs()).items()):
        name = "struct " + name if of_tagged else name
        out.append('    printf("%s\\n  \\"%s\\": {\\"size\\": %%zu, \\"align\\": %%zu, \\"fields\\": [", sizeof(%s), offsetof(struct { char c; %s t; }, t));'
                   % ("," if i else "", name, name, name))
        out += ['    printf("%s[\\"%s\\", %%zu, %%zu]", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (", " if k else "", f, name, f, name, f)
                for k, f in enumerate(fields)]
        out.append('    printf("]}");')
    return "\n".join(out + ['    printf("\\n}\\n");', "    return 0;", "}", ""])
