"""The binding's signature table (hypersonic_rans_amd/_abi.py: SIGNATURES) against the prototypes of include/hsrans_hip.h: every function
of the header has an entry, every entry a prototype, and the width class of the return value and of every argument agree — a forgotten
or narrower argtype would make ctypes pass a 64-bit length or pointer as a C int, silently.  The header is parsed as text (no library, no
compiler); only test_applied_to_the_library loads the built library."""
import ctypes
import os
import re

from hypersonic_rans_amd import _abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hsrans_hip.h")
PROTOTYPES_IN_HEADER = 123  # counted by hand at the commit that added this test: a parser that starts to miss some must not pass

INT8, INT4 = ("size_t", "uint64_t", "int64_t"), ("int", "uint32_t", "int32_t")
PROTOTYPE = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+[\s*]+)(hsrans_\w+)\s*\(([^()]*)\)\s*;", re.M)


def c_class(decl: str) -> str:
    """'ptr', 'int8', 'int4', 'double' or 'void' for a return type or a parameter declaration (its name included)"""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    if words == ["void"]:
        return "void"
    kind = "int8" if words[0] in INT8 else "int4" if words[0] in INT4 else "double" if words[0] == "double" else None
    assert kind is not None and len(words) <= 2, f"cannot place {decl!r}"
    return kind


def ctypes_class(t) -> str:
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    if t is ctypes.c_double:
        return "double"
    assert issubclass(t, ctypes._SimpleCData) and t._type_ in "iIlLqQ", f"cannot place {t!r}"
    return f"int{ctypes.sizeof(t)}"


def header_prototypes() -> dict:
    """name -> (class of the return value, [class of every parameter]), in the header's order"""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    out = {}
    for ret, name, params in PROTOTYPE.findall(text):
        assert name not in out, f"{name} is declared twice"
        params = [p.strip() for p in params.split(",")]
        out[name] = (c_class(ret), [] if params == ["void"] else [c_class(p) for p in params])
    return out


def test_the_parser_finds_every_prototype():
    protos = header_prototypes()
    assert len(protos) >= PROTOTYPES_IN_HEADER, len(protos)
    # every `hsrans_<name>(` of the header that is not a prototype is prose in a comment: none is left once comments are gone
    assert protos["hsrans_capacity"] == ("int8", ["int4", "int4", "int8"])
    assert protos["hsrans_plan_stream_ranges"] == ("int4", ["ptr", "int8", "int4", "int4", "ptr"])  # (uint64_t ranges[4])
    assert protos["hsrans_batch_deal"][0] == "double" and protos["hsrans_version"] == ("ptr", []) and protos["hsrans_ctx_destroy"] == ("void", ["ptr"])


def test_table_and_header_agree():
    protos = header_prototypes()
    assert sorted(set(protos) - set(_abi.SIGNATURES)) == [], "prototypes without a table entry"
    assert sorted(set(_abi.SIGNATURES) - set(protos)) == [], "table entries without a prototype"
    wrong = {}
    for name, (ret, params) in protos.items():
        restype, argtypes = _abi.SIGNATURES[name]
        have = (ctypes_class(restype), [ctypes_class(t) for t in argtypes])
        if have != (ret, params):
            wrong[name] = {"header": (ret, params), "table": have}
    assert wrong == {}


def test_applied_to_the_library():
    L = _abi.load_library()
    for name, (restype, argtypes) in _abi.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
