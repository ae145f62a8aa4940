"""CPU tests of the occlusion queries' C ABI: pt_trace_occluded / pt_trace_occluded_device exist with
the argument types include/pt.h declares, and reject bad arguments before any device call."""
import ctypes as C
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1

HOST_ARGS = [("pt_scene*", C.c_void_p), ("const pt_ray*", C.c_void_p), ("int64_t", C.c_int64), ("float", C.c_float),
             ("float", C.c_float), ("const float*", C.c_void_p), ("int", C.c_int), ("uint8_t*", C.c_void_p),
             ("pt_stats*", None)]
DEVICE_ARGS = HOST_ARGS[:-1] + [("void*", C.c_void_p), ("pt_stats*", None)]


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


def test_symbols_and_argument_types(pt):
    raw = C.CDLL(pt.LIB_PATH)
    for name, args in (("pt_trace_occluded", HOST_ARGS), ("pt_trace_occluded_device", DEVICE_ARGS)):
        assert hasattr(raw, name), f"libpt.so does not export {name}"
        assert name in pt.EXPORTS
        assert declared_types(name) == [a for a, _ in args]
        f = getattr(pt.lib, name)
        assert f.restype is C.c_int
        want = [c if c is not None else C.POINTER(pt.Stats) for _, c in args]
        assert list(f.argtypes) == want
    assert pt.lib.pt_abi_version() == 1   # symbols were added, nothing changed


def test_bad_arguments_are_invalid_and_named(pt):
    rays = np.zeros(4, pt.RAY_DTYPE)
    occ = np.zeros(4, np.uint8)
    st = pt.Stats()
    # NULL scene
    rc = pt.lib.pt_trace_occluded(None, rays.ctypes.data, 4, 0.001, 1.0, None, pt.KERNEL_DEFAULT, occ.ctypes.data,
                                  C.byref(st))
    assert rc == PT_ERR_INVALID
    assert b"pt_trace_occluded" in pt.lib.pt_last_error()
    rc = pt.lib.pt_trace_occluded_device(None, rays.ctypes.data, 4, 0.001, 1.0, None, pt.KERNEL_DEFAULT,
                                         occ.ctypes.data, None, C.byref(st))
    assert rc == PT_ERR_INVALID
    assert b"pt_trace_occluded_device" in pt.lib.pt_last_error()
    # negative n (checked before the scene is looked at: any non-NULL handle will do)
    fake = C.create_string_buffer(64)
    for name in ("pt_trace_occluded", "pt_trace_occluded_device"):
        f = getattr(pt.lib, name)
        extra = (None,) if name.endswith("_device") else ()
        rc = f(C.addressof(fake), rays.ctypes.data, -1, 0.001, 1.0, None, pt.KERNEL_DEFAULT, occ.ctypes.data, *extra,
               C.byref(st))
        assert rc == PT_ERR_INVALID
        assert name.encode() in pt.lib.pt_last_error()
        # NULL arrays with n > 0
        rc = f(C.addressof(fake), None, 4, 0.001, 1.0, None, pt.KERNEL_DEFAULT, occ.ctypes.data, *extra, C.byref(st))
        assert rc == PT_ERR_INVALID
        rc = f(C.addressof(fake), rays.ctypes.data, 4, 0.001, 1.0, None, pt.KERNEL_DEFAULT, None, *extra, C.byref(st))
        assert rc == PT_ERR_INVALID
    assert occ.sum() == 0
