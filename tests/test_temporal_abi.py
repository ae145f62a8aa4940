"""CPU tests of the surface of pt_film_temporal and pt_film_temporal_reset: the option struct's size and
layout as a C compiler sees include/pt.h, the symbols and their argument types, and the arguments rejected
before any device call.  What the call computes is tested on the GPU (tests/test_gpu_temporal.py)
against tests/temporal_ref.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "pt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(pt_temporal_opts), offsetof(pt_temporal_opts, max_history),
           offsetof(pt_temporal_opts, sigma_plane), offsetof(pt_temporal_opts, normal_cos),
           offsetof(pt_temporal_opts, flags), offsetof(pt_temporal_opts, reserved), PT_TEMPORAL_LINEAR);
    return 0;
}
"""


def header():
    return open(os.path.join(REPO, "include", "pt.h")).read()


def test_struct_size_and_layout(pt, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([os.environ.get("CC") or shutil.which("cc") or "gcc", "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32, 0, 4, 8, 12, 16, 1]
    assert C.sizeof(pt.TemporalOpts) == 32
    assert [getattr(pt.TemporalOpts, f).offset for f in ("max_history", "sigma_plane", "normal_cos", "flags", "reserved")] == [0, 4, 8, 12, 16]
    assert pt.TEMPORAL_LINEAR == 1


def test_symbols_and_abi_version(pt):
    raw = C.CDLL(pt.LIB_PATH)
    h = header()
    for name in ("pt_film_temporal", "pt_film_temporal_reset"):
        assert hasattr(raw, name), f"libpt.so does not export {name}"
        assert name in pt.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", h)
        assert getattr(pt.lib, name).restype is C.c_int
    assert list(pt.lib.pt_film_temporal.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pt.Camera), C.c_void_p,
                                                       C.c_void_p, C.c_int, C.c_void_p, C.POINTER(pt.TemporalOpts)]
    assert list(pt.lib.pt_film_temporal_reset.argtypes) == [C.c_void_p]
    assert pt.lib.pt_abi_version() == 1   # symbols and a struct were added, nothing changed
    assert re.search(r"#define\s+PT_ABI_VERSION\s+1\b", h)
    assert hasattr(pt, "temporal") and hasattr(pt.Film, "temporal_reset")
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(REPO, doc)).read()
        assert "pt_film_temporal" in text, doc


def test_null_arguments(pt):
    fake = C.create_string_buffer(4096)
    a = C.addressof(fake)
    cam = pt.Camera()
    buf, length = C.create_string_buffer(12), C.create_string_buffer(4)
    for film, rgb, aov, camera, out in ((None, a, a, C.byref(cam), buf), (a, None, a, C.byref(cam), buf), (a, a, None, C.byref(cam), buf),
                                        (a, a, a, None, buf), (a, a, a, C.byref(cam), None)):
        rc = pt.lib.pt_film_temporal(film, rgb, aov, camera, out, length, 0, None, None)
        assert rc == PT_ERR_INVALID and b"pt_film_temporal: null" in pt.lib.pt_last_error()
    assert buf.raw == bytes(12) and length.raw == bytes(4)
    assert pt.lib.pt_film_temporal_reset(None) == PT_ERR_INVALID
    assert b"pt_film_temporal_reset" in pt.lib.pt_last_error()


BAD = [("max_history", v) for v in (0.0, 0.5, -1.0, float("nan"), float("inf"))] + \
      [("sigma_plane", v) for v in (0.0, -1.0, float("nan"), float("inf"))] + \
      [("normal_cos", v) for v in (-1.5, 1.5, float("nan"), float("inf"), float("-inf"))]


@pytest.mark.parametrize("field,value", BAD)
def test_opts_validation(pt, field, value):
    """Checked first, before the film is looked at: nothing is enqueued and `out` stays as it was."""
    opts = pt.TemporalOpts(32.0, 0.02, 0.9, 0)
    setattr(opts, field, value)
    buf = C.create_string_buffer(12)
    rc = pt.lib.pt_film_temporal(None, None, None, None, buf, None, 0, None, C.byref(opts))
    assert rc == PT_ERR_INVALID and field.encode() in pt.lib.pt_last_error()
    assert buf.raw == bytes(12)


@pytest.mark.parametrize("opts", [(1.0, 0.02, 0.9, 0), (32.0, 1e-30, -1.0, 0), (1e30, 5.0, 1.0, 1), (32.0, 0.02, 0.9, 0x7ffffffe)])
def test_valid_opts_reach_the_null_check(pt, opts):
    """The bounds themselves are valid, and unknown flag bits are ignored: the NULL film is what is refused."""
    o = pt.TemporalOpts(*opts)
    assert pt.lib.pt_film_temporal(None, None, None, None, None, None, 0, None, C.byref(o)) == PT_ERR_INVALID
    assert b"null" in pt.lib.pt_last_error()
