"""CPU tests of pt_scene_download_wide's surface: the symbol exists with the argument types
include/pt.h declares, the header and the binding agree on the array constants, and bad arguments
are rejected before any device call.  What the call returns is tested on the GPU
(tests/test_gpu_wide_structure.py)."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1
NAME = "pt_scene_download_wide"
ARGS = [("pt_scene*", C.c_void_p), ("int", C.c_int), ("void*", C.c_void_p), ("int64_t", C.c_int64),
        ("int64_t*", C.POINTER(C.c_int64))]
ARRAYS = ["PT_WIDE_NODES", "PT_WIDE_PRIMS", "PT_WIDE_SHADE", "PT_WIDE_BOXES", "PT_WIDE_RANKS", "PT_WIDE_EDGE_PRIMS",
          "PT_WIDE_INSTANCES"]


def header():
    return open(os.path.join(REPO, "include", "pt.h")).read()


def declared_types(name):
    """Argument types of `name`'s declaration in include/pt.h, without the parameter names."""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header())
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
    assert re.search(r"#define\s+PT_ABI_VERSION\s+1\b", header())


def test_array_constants(pt):
    h = header()
    for value, name in enumerate(ARRAYS):
        m = re.search(r"\b" + name + r"\s*=\s*(\d+)", h)
        assert m and int(m.group(1)) == value, name
        assert getattr(pt, name[3:]) == value    # ptamd.WIDE_NODES ...
    assert pt.WIDE_NODE_DWORDS == 20             # pt::kW8NodeDwords: the 80-byte node record
    # the header names where the layouts are defined, next to pt_scene_download_bvh
    assert h.index("pt_scene_download_bvh(") < h.index(NAME + "(")
    doc = h[h.index("pt_scene_download_bvh("):h.index(NAME + "(")]
    assert "pt_wide8.cpp" in doc and "pt_wide8.hpp" in doc
    assert hasattr(pt.Scene, "download_wide")
    assert NAME in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_bad_arguments_are_invalid_and_named(pt):
    size = C.c_int64(123)
    buf = C.create_string_buffer(64)
    rc = pt.lib.pt_scene_download_wide(None, pt.WIDE_NODES, buf, 64, C.byref(size))   # NULL scene
    assert rc == PT_ERR_INVALID and size.value == 0
    assert NAME.encode() in pt.lib.pt_last_error()
    # an unknown array, a negative capacity (checked before the scene is looked at: any non-NULL handle will do)
    fake = C.create_string_buffer(4096)
    for array in (-1, len(ARRAYS), 1 << 20):
        size.value = 123
        rc = pt.lib.pt_scene_download_wide(C.addressof(fake), array, buf, 64, C.byref(size))
        assert rc == PT_ERR_INVALID and size.value == 0, array
        assert b"unknown array" in pt.lib.pt_last_error()
    rc = pt.lib.pt_scene_download_wide(C.addressof(fake), pt.WIDE_PRIMS, buf, -1, None)
    assert rc == PT_ERR_INVALID and b"capacity" in pt.lib.pt_last_error()
    assert buf.raw == bytes(64)
