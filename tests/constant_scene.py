"""A scene of constant radiance (a helper module, not a test file).

One triangle (-100, -100, -1), (100, -100, -1), (0, 100, -1) with a PT_EMISSIVE material E, a black
sky, and a pinhole camera at the origin looking down -z with a 40 degree field of view: every camera
ray of every frame shape used here hits the triangle's interior, so every sample contributes
exactly E, whichever random numbers it drew.  With E's components powers of two every partial sum
k * E is exact in fp32 for k <= 2^24, and in the 32.32 fixed-point accumulator while k * E < 2^31, so
the frame of N samples per pixel is known without tracing a path:

    sqrt(float32(N * E) * (float32(1) / float32(N)))      per channel, in float32 arithmetic

(pt.h's resolve formula), with rays == paths == pixels * N.  A dropped, duplicated or mis-converted
block changes a sum by at least E / N of it -- more than an ulp of the result at every N the tests
use -- and a miss contributes 0, so a bit-exact comparison sees either.
tests/test_constant_scene_host.py proves the formula against tests/pathloop.py on the CPU; the GPU
tests (tests/test_gpu_sample_scale.py) then use it at sample counts no CPU reference can follow.
"""
import numpy as np

import oracle as orc

F = np.float32
PT_TRIANGLE, PT_EMISSIVE = 3, 8
E_DEFAULT = (1024.0, 4.0, 0.25)
BLACK_SKY = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
TRIANGLE = (-100.0, -100.0, -1.0, 100.0, -100.0, -1.0, 0.0, 100.0, -1.0)


def scene(E=E_DEFAULT):
    """(objects, materials) of the constant scene with radiance E (per-channel powers of two)."""
    for e in E:
        m, _ = np.frexp(float(e))
        assert m == 0.5 and 0 < e <= 1024.0, "E's components must be powers of two (every k * E exact)"
    objs = np.zeros(1, orc.OBJECT_DTYPE)
    objs["type"], objs["mat"] = PT_TRIANGLE, 0
    objs["v"][0] = TRIANGLE
    mats = np.zeros(1, orc.MATERIAL_DTYPE)
    mats["type"] = PT_EMISSIVE
    mats["albedo"][0] = E
    return objs, mats


def camera(width, height):
    """The oracle's 25 camera floats (= the bytes of pt_camera): camera_make((0,0,0), (0,0,-1), 40, w/h)."""
    return orc.camera_make((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 40.0, width / height)


def expected(N, E=E_DEFAULT):
    """One pixel's fp32 RGB after N samples of E: float32[3]."""
    N = int(N)
    assert 0 < N < 2 ** 24
    s = np.array([float(e) * N for e in E], np.float64)
    assert (s.astype(F).astype(np.float64) == s).all(), "N * E must be exact in fp32"
    return np.sqrt((s.astype(F) * (F(1.0) / F(N))).astype(F)).astype(F)


def expected_frame(n_pixels, N, E=E_DEFAULT):
    return np.tile(expected(N, E), (n_pixels, 1))
