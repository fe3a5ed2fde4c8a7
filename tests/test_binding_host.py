"""CPU-only tests of how host.py binds the C ABI: host.SIGNATURES, the one table every entry point is bound from, against the
prototypes of include/rt_mi355.h (arity, return type and the class of every parameter), the loaded library against the table, and
the lenient path of RT_LIB, where a library that lacks an entry point answers a call of it with an RtError.  No compute call is
made here."""
import collections
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt_mi355.h")

Prototype = collections.namedtuple("Prototype", "restype name params")      # params: the text of each parameter

_PROTOTYPE = re.compile(r"^(int|size_t|const char \*)\s*(rt_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)


def prototypes(path=HEADER):
    """Every function the header declares, in its order.  There are no function-pointer parameters, so a prototype has one pair of
    parentheses; it may run over several lines."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return [Prototype(r, n, [" ".join(p.split()) for p in a.split(",")] if a.strip() not in ("", "void") else [])
            for r, n, a in _PROTOTYPE.findall(text)]


RESTYPES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}
SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64}
# what a typed POINTER(...) of the table may point at, beyond SCALARS: the header's spelling -> the ctypes element
ELEMENTS = dict(SCALARS, unsigned=ctypes.c_uint32, int32_t=ctypes.c_int32, uint8_t=ctypes.c_uint8)


def c_parameter(text):
    """'const rt_yuv_desc *planes' -> ('rt_yuv_desc', 1); 'size_t offset[3]' -> ('size_t', 1); 'int n' -> ('int', 0): the type
    without qualifiers, and how many levels of pointer or array stand on it."""
    depth = text.count("*") + text.count("[")
    words = [w for w in re.sub(r"\[[^\]]*\]", "", text).replace("*", " ").split() if w != "const"]
    return " ".join(words[:-1]), depth


def snake(name):
    """RtYuvDesc -> rt_yuv_desc."""
    return re.sub(r"(?<!^)([A-Z])", r"_\1", name).lower()


def mismatch(param, ctype):
    """None when the table's `ctype` is of the class the header's parameter `param` asks for, else what is wrong."""
    base, depth = c_parameter(param)
    if depth == 0:
        return None if SCALARS.get(base) is ctype else f"'{param}' is bound as {ctype.__name__}"
    if ctype in (ctypes.c_void_p, ctypes.c_char_p):
        return None
    if not (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer)):
        return f"'{param}' is a pointer, bound as {ctype.__name__}"
    to = ctype._type_
    if issubclass(to, ctypes.Structure):                       # a named struct: CamelCase here, snake_case there
        return None if depth == 1 and snake(to.__name__) == base else f"'{param}' is bound as POINTER({to.__name__})"
    if to is ctypes.c_void_p:                                  # void **, rt_context **: a pointer to a pointer
        return None if depth == 2 else f"'{param}' is bound as POINTER(c_void_p)"
    return None if depth == 1 and ELEMENTS.get(base) is to else f"'{param}' is bound as POINTER({to.__name__})"


def table_errors(table, protos):
    """Every disagreement between a signature table and the header's prototypes, as text."""
    errors = [f"{name}: in the table, not in the header" for name in table if name not in {p.name for p in protos}]
    for p in protos:
        if p.name not in table:
            errors.append(f"{p.name}: in the header, not in the table")
            continue
        restype, argtypes = table[p.name]
        if RESTYPES[p.restype] is not restype:
            errors.append(f"{p.name}: returns '{p.restype}', bound as {getattr(restype, '__name__', restype)}")
        if len(argtypes) != len(p.params):
            errors.append(f"{p.name}: {len(p.params)} parameters in the header, {len(argtypes)} in the table")
            continue
        errors += [f"{p.name}: parameter {k}: {bad}" for k, (param, t) in enumerate(zip(p.params, argtypes)) if (bad := mismatch(param, t))]
    return errors


def test_the_parser_reads_the_header():
    protos = prototypes()
    names = [p.name for p in protos]
    assert len(names) == len(set(names)) >= 101
    by_name = {p.name: p for p in protos}
    assert by_name["rt_wire_bytes"] == Prototype("size_t", "rt_wire_bytes", ["size_t nPixels"])
    assert by_name["rt_last_error"].restype == "const char *"
    assert len(by_name["rt_wire_unpack"].params) == 16                       # three lines long
    assert by_name["rt_scene_write"].params[4] == "const char *const *objNames"
    assert c_parameter("const rt_yuv_desc *planes") == ("rt_yuv_desc", 1) and c_parameter("size_t offset[3]") == ("size_t", 1)
    assert c_parameter("const void **hostPixels") == ("void", 2) and c_parameter("uint32_t maxSamples") == ("uint32_t", 0)
    assert snake("RtYuvDesc") == "rt_yuv_desc" and snake("RtParams") == "rt_params"


def test_signature_table_matches_the_header(host):
    """Name for name: the same arity, the same return type, the same class of every parameter, and no name the header lacks."""
    assert table_errors(host.SIGNATURES, prototypes()) == []
    assert list(host.SIGNATURES) == [p.name for p in prototypes()], "the table follows the header's order"
    assert host.EXPORTS == list(host.SIGNATURES)


def test_loaded_library_is_bound_from_the_table(host):
    lib = host.load_library()
    for name, (restype, argtypes) in host.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_a_library_without_an_entry_point_raises_when_it_is_called(host, tmp_path, monkeypatch):
    """RT_LIB names an experiment build, which may predate newer entry points: what it has is bound, a call of the rest raises."""
    src, so = tmp_path / "wire.c", tmp_path / "libwire_only.so"
    src.write_text("#include <stddef.h>\nsize_t rt_wire_bytes(size_t nPixels) { return nPixels * 30; }\n")
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(host, "_LIB", None)                                # the session's library comes back after the test
    monkeypatch.setenv("RT_LIB", str(so))
    lib = host.load_library()
    assert host._LIB is lib and lib.rt_wire_bytes(7) == 210
    assert lib.rt_wire_bytes.restype is ctypes.c_size_t and lib.rt_wire_bytes.argtypes == [ctypes.c_size_t]
    for name in host.EXPORTS:
        if name == "rt_wire_bytes":
            continue
        with pytest.raises(host.RtError) as e:
            getattr(lib, name)(None)
        assert e.value.code == -2 and str(e.value) == f"RT_ERR_NO_DEVICE: {name} is not exported by {so}"
    with pytest.raises(host.RtError, match="rt_accum_layout is not exported by") as e:     # and through the helpers
        host.accum_layout(4, 4)
    assert e.value.code == -2
