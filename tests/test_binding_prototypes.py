"""CPU: the `argtypes` and `restype` the ctypes binding sets are the prototypes of include/rroi_align_hip.h -- the same
number of parameters and, position by position, the same kind.  A mismatch does not raise at the call: it passes a
truncated pointer or a shifted argument list into a launch, so it is held here, against the header, for every export."""
import ctypes
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rroi_align_hip.h")

# the exports the binding never calls with arguments and sets neither `restype` nor `argtypes` for: the two deprecated
# trig-recipe shims and the launchers' recipe query (int f(void) or int f(int): ctypes' defaults serve them)
UNBOUND = {"rroi_align_set_trig_recipe_hip", "rroi_align_get_trig_recipe_hip", "rroi_align_launcher_trig_recipe"}
# ... and the one it gives a `restype` only: checked below for its return type and for taking no parameter
RESTYPE_ONLY = {"rroi_align_hip_version"}

SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           "long long": ctypes.c_longlong}
RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}


def prototypes():
    """{name: (return type, [parameter type, ...])} of every function the header declares, types as written with the
    parameter's name and a top-level `const` removed, pointers as "... *" collapsed to a trailing `*`."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^[ \t]*((?:const\s+)?(?:int|size_t|char|void)\s*\*?)\s*(\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.M | re.S):
        ret, name, params = re.sub(r"\s+", " ", m.group(1)).replace(" *", "*").strip(), m.group(2), m.group(3)
        params = [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
        if params == ["void"]:
            params = []
        kinds = []
        for p in params:
            if "*" in p:
                kinds.append("*")
            else:
                words = [w for w in p.split(" ") if w != "const"]
                assert len(words) >= 2, (name, p)          # a type and the parameter's name
                kinds.append(" ".join(words[:-1]))
        assert name not in out, name
        out[name] = (ret, kinds)
    return out


def is_pointer(t) -> bool:
    return t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as ext
    for sub in ("remainder", "preprocess", "ctc_loss", "detection_loss"):      # loaded on first use by fots_e2e
        importlib.import_module(f"{ext.__name__}.{sub}")
    return ext


def test_the_parser_reads_every_declared_function(ext):
    protos = prototypes()
    assert set(protos) == set(ext.EXPORTS)
    # three prototypes read by hand, one of each shape: no parameters, a pointer return, scalars of every kind
    assert protos["rroi_align_hip_version"] == ("const char*", [])
    assert protos["rroi_align_write_probe_hip"] == ("int", ["*", "size_t", "*"])
    assert protos["rroi_ctc_loss_plan"] == ("int", ["int"] * 5 + ["long long", "long long", "int", "*"])
    assert protos["rroi_instancenorm_forward_hip"][1][9:11] == ["double", "float"]
    assert {k for _, kinds in protos.values() for k in kinds} <= set(SCALARS) | {"*"}
    assert {ret for ret, _ in protos.values()} <= set(RETURNS)


def test_the_unbound_exports_are_exactly_the_listed_ones(ext):
    without = {n for n in ext.EXPORTS if getattr(ext._lib, n).argtypes is None}
    assert without == UNBOUND | RESTYPE_ONLY
    assert all(getattr(ext._lib, n).restype is ctypes.c_int for n in UNBOUND)          # ctypes' default: never set


def test_argtypes_and_restype_are_the_headers(ext):
    protos = prototypes()
    wrong = []
    for name in ext.EXPORTS:
        if name in UNBOUND:
            continue
        fn, (ret, kinds) = getattr(ext._lib, name), protos[name]
        if fn.restype is not RETURNS[ret]:
            wrong.append(f"{name}: restype {fn.restype} for `{ret}`")
        argtypes = fn.argtypes
        if argtypes is None:                               # restype only: the header must declare no parameter
            assert name in RESTYPE_ONLY, name
            argtypes = ()
        if len(argtypes) != len(kinds):
            wrong.append(f"{name}: {len(argtypes)} argtypes for {len(kinds)} parameters")
            continue
        for at, (got, kind) in enumerate(zip(argtypes, kinds)):
            ok = is_pointer(got) if kind == "*" else got is SCALARS[kind]
            if not ok:
                wrong.append(f"{name}: argtypes[{at}] is {got} for `{kind}`")
    assert not wrong, "\n".join(wrong)
