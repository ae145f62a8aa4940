"""The constant-radiance scene's closed-form frame (tests/constant_scene.py) against the render loop
restated on the CPU (tests/pathloop.py, itself proved against the oracle by test_emission_host.py):
bit for bit, every path ending on the emitter at bounce 0, rays == paths.  The GPU tests of sample
mode at long sample counts (test_gpu_sample_scale.py) rest on the formula; here it is proved without
a GPU, at small settings, including a sample base just below 2^23 and a ragged last block."""
import numpy as np
import pytest

import constant_scene as cs
import oracle as orc
import pathloop

SEED = 77


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("w,h,spp,chunk,base,E", [
    (8, 8, 37, 5, 0, cs.E_DEFAULT),
    (8, 8, 64, 64, 0, cs.E_DEFAULT),
    (13, 5, 37, 64, 0, cs.E_DEFAULT),
    (13, 5, 64, 5, 2 ** 23 - 3, cs.E_DEFAULT),
    (8, 8, 37, 5, 2 ** 23 - 3, (512.0, 128.0, 0.0625)),
])
def test_constant_scene_frame_is_the_closed_form(w, h, spp, chunk, base, E):
    objs, mats = cs.scene(E)
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    r = pathloop.render_sample(objs, mats, nodes, cs.camera(w, h), w, h, range(h), spp, 50, SEED, chunk,
                               sample_base=base, sky=cs.BLACK_SKY)
    np.testing.assert_array_equal(bits(r["image"]), bits(cs.expected_frame(w * h, spp, E)))
    assert r["rays"] == r["paths"] == w * h * spp
    assert set(r["kinds"]) == {(pathloop.EMITTER, 0)}
    # the sums themselves: N * E, exactly
    np.testing.assert_array_equal(r["sums"], np.tile(np.array(E, np.float32) * np.float32(spp), (w * h, 1)))


def test_expected_values():
    """Powers of four under the root come out exactly; the formula refuses an inexact N * E."""
    assert cs.expected(64).tolist() == [32.0, 2.0, 0.5]
    assert cs.expected(2 ** 21 - 1, (1024.0, 4.0, 0.25)).shape == (3,)
    with pytest.raises(AssertionError):
        cs.expected(2 ** 24 - 1, (1024.0 + 1.0 / 1024, 4.0, 0.25))   # N * E needs more than 24 bits
    with pytest.raises(AssertionError):
        cs.scene((3.0, 4.0, 0.25))
