"""CPU (no GPU): the ctypes signature table of sdslam_amd/capi.py against the prototypes of include/sdslam_hip.h.

The header is the ABI and the compiler checks only the C++ facade against it; a wrong c_float / c_double or a missing `int cap`
in the binding is no error in ctypes, only a garbage argument to a call that launches kernels.  So the table is parsed against
the header here, the parser is guarded against skipping declarations, and the source is checked to have no other declaration."""
import ast
import ctypes as C
import io
import os
import re
import subprocess
import sys
import tokenize

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sdslam_hip.h")
PTR = "pointer"         # c_void_p, c_char_p and every POINTER(...) are one class for a parameter
SCALARS = {"int": C.c_int, "int32_t": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "unsigned long long": C.c_ulonglong}
RETURNS = {"int": C.c_int, "int32_t": C.c_int, "void": None, "char*": C.c_char_p}
EXTRA_EXPORTS = set()   # sd_* symbols the library exports beyond the header's: none


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()          # hipcc cross-compiles gfx950 without a GPU
    return sdslam_amd


def stripped_header():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)        # preprocessor lines


def c_type(decl, named):
    """A parameter or return declaration -> PTR or the C scalar type's name; `named`: a trailing parameter name may be there."""
    words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
    if "*" in words:
        return PTR if named else "".join(w for w in words if w != "*") + "*" * words.count("*")
    for n in ((len(words) - 1, len(words)) if named else (len(words),)):        # with a name first: `unsigned long long x`
        if " ".join(words[:n]) in SCALARS or (not named and " ".join(words[:n]) == "void"):
            return " ".join(words[:n])
    raise ValueError(f"unknown C type in {decl!r}")


def prototypes():
    """name -> (return type, [parameter types]) of every function the header declares."""
    out = {}
    for m in re.finditer(r"(?<=[;{}\s])([A-Za-z_][\w\s\*]*?)\b(sd_\w+)\s*\(([^()]*)\)\s*;", stripped_header()):
        ret, name, params = m.groups()
        assert name not in out, name
        params = [] if params.strip() in ("void", "") else [c_type(p, True) for p in params.split(",")]
        out[name] = (c_type(ret, False), params)
    return out


def ctypes_class(t):
    return PTR if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer)) else t


def disagreements(table, unbound, protos):
    """Every (name, what) in which `table` / `unbound` differ from the header's prototypes."""
    bad = []
    for name, (restype, argtypes) in table.items():
        if name not in protos:
            bad.append((name, "not in the header"))
            continue
        ret, params = protos[name]
        if restype is not RETURNS.get(ret, "unknown"):
            bad.append((name, "restype"))
        if len(argtypes) != len(params):
            bad.append((name, "argument count"))
            continue
        bad += [(name, f"argument {i}") for i, (a, p) in enumerate(zip(argtypes, params))
                if ctypes_class(a) is not (PTR if p == PTR else SCALARS[p])]
    bad += [(name, "in the table and in _UNBOUND") for name in unbound if name in table]
    bad += [(name, "not in the header") for name in unbound if name not in protos]
    bad += [(name, "neither in the table nor in _UNBOUND") for name in protos if name not in table and name not in unbound]
    return bad


def test_parser_sees_every_declaration(sd):
    protos = prototypes()
    crude = re.findall(r"\b(sd_\w+)\s*\(", stripped_header())          # every sd_name( left once comments are gone
    assert len(protos) == len(crude) == len(set(crude)) >= 119, (len(protos), len(crude))
    L = sd.lib()
    for name in protos:
        assert hasattr(L, name), name
    assert {ret for ret, _ in protos.values()} == {"int", "void", "char*"}
    assert protos["sd_last_error"] == ("char*", []) and protos["sd_orb_destroy"] == ("void", [PTR])
    assert protos["sd_debug_pnp_prof"] == ("int", [PTR, "int"])             # `unsigned long long* out32`
    assert protos["sd_track_pnp"] == ("int", [PTR, "int", "double", "int", "int", "int", "float", "float", "int"])
    assert protos["sd_orb_extract_batch_device"][1][-1] == "size_t" and protos["sd_track_stage_ms"] == ("int", [PTR, PTR, "int"])


def test_exported_symbols_are_the_header(sd):
    nm = subprocess.run(["nm", "-D", "--defined-only", sd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if re.search(r"\ssd_\w+$", line)}
    assert exported - EXTRA_EXPORTS == set(prototypes()), exported ^ set(prototypes())


def test_table_agrees_with_the_header(sd):
    from sdslam_amd import capi
    assert disagreements(capi._SIGNATURES, capi._UNBOUND, prototypes()) == []
    assert not set(capi._UNBOUND) & set(capi._SIGNATURES)
    assert {n for n, (r, _) in capi._SIGNATURES.items() if r is None} == {"sd_orb_destroy", "sd_track_destroy"}
    assert {n for n, (r, _) in capi._SIGNATURES.items() if r is C.c_char_p} == {"sd_last_error", "sd_version", "sd_option_name",
                                                                              "sd_orb_stage_name"}


def test_checker_bites(sd):
    from sdslam_amd import capi
    table = {k: (r, list(a)) for k, (r, a) in capi._SIGNATURES.items()}
    assert table["sd_track_pnp"][1][2] is C.c_double
    table["sd_track_pnp"][1][2] = C.c_float                                # a double taken for a float
    table["sd_track_set_rand"][1].pop()                                    # the `int per_frame` forgotten
    table["sd_track_no_such_call"] = (C.c_int, [C.c_void_p])               # a name the header lacks
    assert sorted(disagreements(table, capi._UNBOUND, prototypes())) == [
        ("sd_track_no_such_call", "not in the header"), ("sd_track_pnp", "argument 2"), ("sd_track_set_rand", "argument count")]
    table = dict(capi._SIGNATURES)
    dropped = table.pop("sd_hamming")
    assert disagreements(table, capi._UNBOUND, prototypes()) == [("sd_hamming", "neither in the table nor in _UNBOUND")]
    assert disagreements(capi._SIGNATURES, capi._UNBOUND + ("sd_hamming",), prototypes()) == [("sd_hamming", "in the table and in _UNBOUND")]
    table["sd_hamming"] = (None, dropped[1])
    assert disagreements(table, capi._UNBOUND, prototypes()) == [("sd_hamming", "restype")]


def test_table_is_the_only_declaration_site():
    """No `.argtypes` / `.restype` in capi.py but the two assignments of the one loop in lib()."""
    path = os.path.join(ROOT, "sdslam_amd", "capi.py")
    src = open(path).read()
    toks = [t for t in tokenize.generate_tokens(io.StringIO(src).readline) if t.type in (tokenize.NAME, tokenize.OP)]
    sites = [(toks[i - 1].string, t.string, toks[i + 1].string, t.start[0]) for i, t in enumerate(toks)
             if t.string in ("argtypes", "restype") and toks[i - 1].string == "."]          # as an attribute, read or written
    assert sorted(s[:3] for s in sites) == [(".", "argtypes", "="), (".", "restype", "=")], sites
    assert not re.search(r"""["'](argtypes|restype)["']""", src)          # nor through setattr
    lib_fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "lib")
    loops = [n for n in ast.walk(lib_fn) if isinstance(n, ast.For)]
    assert len(loops) == 1 and "_SIGNATURES" in ast.unparse(loops[0].iter)
    assert all(loops[0].lineno < s[3] <= loops[0].end_lineno for s in sites), sites


CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
from sdslam_amd import capi
L = capi.lib()                  # nothing else: no ORBextractor, no Tracker
for name, (restype, argtypes) in capi._SIGNATURES.items():
    fn = getattr(L, name)
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
assert list(L.sd_track_get_stereo.argtypes) == [capi.C.c_void_p, capi.C.c_int, capi.C.c_int, capi.C.c_void_p, capi.C.c_void_p, capi.C.c_int]
assert L.sd_track_destroy.restype is None and L.sd_orb_destroy.restype is None
assert L.sd_track_get_stereo(None, 0, 1, None, None, 0) == 1 and b"NULL" in L.sd_last_error()
print("LOAD_OK")
"""


def test_table_is_applied_at_load(sd):
    """In a fresh process, lib() alone declares every row."""
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", CHILD, ROOT], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "LOAD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_a_missing_export_fails_the_load(sd, monkeypatch):
    from sdslam_amd import capi
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setitem(capi._SIGNATURES, "sd_track_no_such_call", (C.c_int, [C.c_void_p]))
    with pytest.raises(AttributeError, match="sd_track_no_such_call"):
        capi.lib()
    assert capi._lib is None
