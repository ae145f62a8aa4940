"""CPU tests of pt_scene_update_instances' C ABI: the symbol exists with the argument types
include/pt.h declares, and rejects bad arguments before any device call."""
import ctypes as C
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1
NAME = "pt_scene_update_instances"
ARGS = [("pt_scene*", C.c_void_p), ("const pt_instance*", C.c_void_p), ("int64_t", C.c_int64), ("int64_t", C.c_int64)]


def declared_types(name):
    """Argument types of `name`'s declaration in include/pt.h, without the parameter names."""
    header = open(os.path.join(REPO, "include", "pt.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/pt.h"
    out = []
    for arg in m.group(1).split(","):
        arg = re.sub(r"/\*.*?\*/", "", arg, flags=re.S).strip()
        typ = re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*$", "", arg)   # drop the parameter's name
        out.append(re.sub(r"\s*\*", "*", re.sub(r"\s+", " ", typ)))
    return out


def test_symbol_and_argument_types(pt):
    raw = C.CDLL(pt.LIB_PATH)
    assert hasattr(raw, NAME), f"libpt.so does not export {NAME}"
    assert NAME in pt.EXPORTS
    assert declared_types(NAME) == [a for a, _ in ARGS]
    f = getattr(pt.lib, NAME)
    assert f.restype is C.c_int
    assert list(f.argtypes) == [c for _, c in ARGS]
    assert pt.lib.pt_abi_version() == 1   # a symbol was added, nothing changed
    assert hasattr(pt.Scene, "update_instances")


def test_wide_info_sources_are_documented():
    header = open(os.path.join(REPO, "include", "pt.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+pt_scene_wide_info\s*\(", header, flags=re.S)
    assert m
    assert re.search(r"\b3\b", m.group(1)) and re.search(r"\b4\b", m.group(1))


def test_bad_arguments_are_invalid_and_named(pt):
    inst = np.zeros(4, pt.INSTANCE_DTYPE)
    f = pt.lib.pt_scene_update_instances
    assert f(None, inst.ctypes.data, 0, 4) == PT_ERR_INVALID   # NULL scene
    assert NAME.encode() in pt.lib.pt_last_error()
    # checked before the scene is looked at: any non-NULL handle will do
    fake = C.create_string_buffer(4096)
    for first, n, arr in ((-1, 1, inst.ctypes.data), (0, -1, inst.ctypes.data), (0, 4, None)):
        assert f(C.addressof(fake), arr, first, n) == PT_ERR_INVALID, (first, n)
        assert NAME.encode() in pt.lib.pt_last_error()
