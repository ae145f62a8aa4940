"""CPU tests of the surface of pt_render_aov and pt_film_denoise: the structs' sizes and layout as a C
compiler sees include/pt.h, the symbols and their argument types, and the arguments rejected before
any device call.  What the calls compute is tested on the GPU (tests/test_gpu_aov.py,
tests/test_gpu_denoise.py) against tests/atrous_ref.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import atrous_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "pt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(pt_aov), offsetof(pt_aov, albedo), offsetof(pt_aov, depth),
           offsetof(pt_aov, n), offsetof(pt_aov, obj), offsetof(pt_aov, p), offsetof(pt_aov, mat),
           sizeof(pt_denoise_opts), offsetof(pt_denoise_opts, reserved));
    return 0;
}
"""


def header():
    return open(os.path.join(REPO, "include", "pt.h")).read()


def test_struct_sizes(pt, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([os.environ.get("CC") or shutil.which("cc") or "gcc", "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [48, 0, 12, 16, 28, 32, 44, 32, 16]
    for dt in (pt.AOV_DTYPE, atrous_ref.AOV_DTYPE):
        assert dt.itemsize == 48
        assert [dt.fields[f][1] for f in ("albedo", "depth", "n", "obj", "p", "mat")] == [0, 12, 16, 28, 32, 44]
    assert pt.AOV_DTYPE == atrous_ref.AOV_DTYPE
    assert C.sizeof(pt.DenoiseOpts) == 32


def test_symbols_and_abi_version(pt):
    raw = C.CDLL(pt.LIB_PATH)
    h = header()
    for name in ("pt_render_aov", "pt_film_denoise"):
        assert hasattr(raw, name), f"libpt.so does not export {name}"
        assert name in pt.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", h)
        assert getattr(pt.lib, name).restype is C.c_int
    assert list(pt.lib.pt_render_aov.argtypes) == [C.c_void_p, C.c_void_p, C.POINTER(pt.Camera), C.c_void_p, C.c_int,
                                                    C.c_void_p, C.POINTER(pt.Stats)]
    assert list(pt.lib.pt_film_denoise.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                      C.POINTER(pt.DenoiseOpts)]
    assert pt.lib.pt_abi_version() == 1   # symbols and structs were added, nothing changed
    assert re.search(r"#define\s+PT_ABI_VERSION\s+1\b", h)
    for name in ("render_aov", "denoise", "AOV_DTYPE"):
        assert hasattr(pt, name)
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(REPO, doc)).read()
        assert "pt_render_aov" in text and "pt_film_denoise" in text and "--denoise" in text, doc


def test_render_aov_null_arguments(pt):
    fake = C.create_string_buffer(4096)
    cam = pt.Camera()
    buf = C.create_string_buffer(48)
    a = C.addressof(fake)
    for scene, film, camera, out in ((None, a, C.byref(cam), buf), (a, None, C.byref(cam), buf), (a, a, None, buf),
                                     (a, a, C.byref(cam), None)):
        rc = pt.lib.pt_render_aov(scene, film, camera, out, 0, None, None)
        assert rc == PT_ERR_INVALID and b"pt_render_aov" in pt.lib.pt_last_error()
    assert buf.raw == bytes(48)


def test_denoise_null_arguments(pt):
    fake = C.create_string_buffer(4096)
    a = C.addressof(fake)
    buf = C.create_string_buffer(12)
    for film, rgb, aov, out in ((None, a, a, buf), (a, None, a, buf), (a, a, None, buf), (a, a, a, None)):
        rc = pt.lib.pt_film_denoise(film, rgb, aov, out, 0, None, None)
        assert rc == PT_ERR_INVALID and b"pt_film_denoise: null" in pt.lib.pt_last_error()
    assert buf.raw == bytes(12)


@pytest.mark.parametrize("field,value", [("iterations", -1), ("iterations", 9)] + [
    (s, v) for s in ("sigma_color", "sigma_albedo", "sigma_plane") for v in (0.0, -1.0, float("nan"), float("inf"))])
def test_denoise_opts_validation(pt, field, value):
    """Checked first, before the film is looked at: nothing is enqueued and `out` stays as it was."""
    opts = pt.DenoiseOpts(5, 0.6, 0.1, 0.02)
    setattr(opts, field, value)
    buf = C.create_string_buffer(12)
    rc = pt.lib.pt_film_denoise(None, None, None, buf, 0, None, C.byref(opts))
    assert rc == PT_ERR_INVALID
    assert (b"iterations" if field == "iterations" else b"sigma") in pt.lib.pt_last_error()
    assert buf.raw == bytes(12)
    # the same opts, valid: the NULL film is what is refused
    ok = pt.DenoiseOpts(8 if field == "iterations" else 5, 0.6, 0.1, 0.02)
    assert pt.lib.pt_film_denoise(None, None, None, buf, 0, None, C.byref(ok)) == PT_ERR_INVALID
    assert b"null" in pt.lib.pt_last_error()


def test_denoise_sigma_helper(pt):
    """sigma_color=None: 1.2 / sqrt(max(1, spp)), and spp is required then (checked before the library is called)."""
    with pytest.raises(ValueError):
        pt.denoise(None, np.zeros((1, 3), np.float32), np.zeros(1, pt.AOV_DTYPE))
    assert atrous_ref.sigma_for(4) == 0.6 and atrous_ref.sigma_for(0) == 1.2
