"""Sample mode (PT_RNG_SAMPLE) at the sample counts where pt.h's numeric promises bind.

  * the 32.32 fixed-point accumulator is exact while samples x radiance < 2^31;
  * an accumulating film holds up to 2^24 - 1 samples per pixel;
  * a frame of fewer than 2^32 - 2^26 (pixel, block) tasks renders correctly, a larger one is refused.

No CPU reference can follow to 2^21 samples per pixel, so the frames are of the constant-radiance
scene (tests/constant_scene.py): every sample contributes exactly E, every partial sum is exact, and
the frame is sqrt(float32(N * E) * (float32(1) / float32(N))) whatever the scheduling -- proved on the
CPU by tests/test_constant_scene_host.py.  Every comparison is bit for bit, and the counters must be
rays == paths == pixels x N: a dropped, repeated or mis-converted block breaks both.  Films are tiny
(8 x 8 mostly), so the long sample counts cost fractions of a second.
"""
import numpy as np
import pytest

import constant_scene as cs

pytestmark = pytest.mark.gpu

SEED = 77
TASK_LIMIT = 2 ** 32 - 2 ** 26   # pt.h, PT_RNG_SAMPLE: tiles x blocks x 64 must stay below it


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def kernel_id(pt, name):
    return {"wide": pt.KERNEL_WIDE, "wavefront": pt.KERNEL_WAVEFRONT, "simple": pt.KERNEL_SIMPLE}[name]


def device_scene(pt, gpu, E=cs.E_DEFAULT):
    objs, mats = cs.scene(E)
    s = pt.Scene(objs, mats, device=gpu)
    s.set_sky(*cs.BLACK_SKY)
    return s


def camera_of(pt, w, h):
    return pt.Camera.from_buffer_copy(cs.camera(w, h).tobytes())


def check_frame(rgb, st, n_pixels, N, E=cs.E_DEFAULT, frame_spp=None):
    """The frame is the closed form for N samples; the counters are those of the frame's own spp."""
    np.testing.assert_array_equal(bits(rgb), bits(cs.expected_frame(n_pixels, N, E)))
    spp = N if frame_spp is None else frame_spp
    assert st.rays == st.paths == n_pixels * spp, (st.rays, st.paths, n_pixels * spp)


# ---------------------------------------------------------------- sanity: every kernel, small counts
@pytest.mark.parametrize("kernel", ["wide", "wavefront", "simple"])
@pytest.mark.parametrize("w,h", [(37, 19), (8, 8)])
def test_constant_scene_in_every_kernel(pt, gpu, kernel, w, h):
    """Ragged tiles and one tile; a ragged last block, the default block size, and a stripe
    partition (three films that share the frame's rows)."""
    s, cam, k = device_scene(pt, gpu), camera_of(pt, w, h), kernel_id(pt, kernel)
    f = pt.Film(w, h, SEED, device=gpu)
    for spp, chunk in ((37, 5), (64, 0)):
        rgb, st = pt.render(s, f, cam, spp, 50, rng=pt.RNG_SAMPLE, chunk=chunk, kernel=k)
        check_frame(rgb, st, w * h, spp)
    rows = 0
    for part in range(3):
        fp = pt.Film(w, h, SEED, device=gpu, stripe_height=2, n_parts=3, part=part)
        assert fp.n_rows > 0
        rgb, st = pt.render(s, fp, cam, 37, 50, rng=pt.RNG_SAMPLE, chunk=5, kernel=k)
        check_frame(rgb, st, fp.n_pixels, 37)
        rows += fp.n_rows
    assert rows == h


# ---------------------------------------------------------------- the accumulator's range
@pytest.mark.parametrize("kernel", ["wide", "wavefront"])
@pytest.mark.parametrize("chunk", [0, 1000])
def test_accumulator_exact_up_to_2_31(pt, gpu, kernel, chunk):
    """N = 2^21 - 1 samples of radiance 1024: N * 1024 = 2^31 - 1024, the last sum below the bound
    pt.h states.  Default blocks, and blocks of 1000 with a ragged last one."""
    N = 2 ** 21 - 1
    s, cam = device_scene(pt, gpu), camera_of(pt, 8, 8)
    f = pt.Film(8, 8, SEED, device=gpu)
    rgb, st = pt.render(s, f, cam, N, 50, rng=pt.RNG_SAMPLE, chunk=chunk, kernel=kernel_id(pt, kernel))
    check_frame(rgb, st, 64, N)


@pytest.mark.parametrize("kernel", ["wide", "wavefront"])
def test_large_blocks_take_the_general_conversion(pt, gpu, kernel):
    """Blocks of 32768 samples: the first channel's block sums are 2^25 >= 2^24, so the whole wave
    converts with blockFixed (addBlock's general branch) while the other channels' sums stay small;
    the last block is ragged (5 samples)."""
    N = 2 ** 20 + 5
    s, cam = device_scene(pt, gpu), camera_of(pt, 8, 8)
    f = pt.Film(8, 8, SEED, device=gpu)
    rgb, st = pt.render(s, f, cam, N, 50, rng=pt.RNG_SAMPLE, chunk=32768, kernel=kernel_id(pt, kernel))
    check_frame(rgb, st, 64, N)


# ---------------------------------------------------------------- accumulation up to its cap
def test_accumulation_to_the_cap(pt, gpu):
    """Fifteen frames of 2^20 spp and one of 2^20 - 1 reach 2^24 - 1 accumulated samples (radiance
    128: 2^24 x 128 = 2^31, pt.h's bound for the cap); every frame's output is the closed form of the
    samples so far.  One more sample is refused and changes nothing; clear() starts again."""
    E = (128.0, 4.0, 0.25)
    s, cam = device_scene(pt, gpu, E), camera_of(pt, 8, 8)
    f = pt.Film(8, 8, SEED, device=gpu)
    total = 0
    for spp in [2 ** 20] * 15 + [2 ** 20 - 1]:
        rgb, st = pt.render(s, f, cam, spp, 50, rng=pt.RNG_SAMPLE, chunk=2048, accumulate=True)
        total += spp
        check_frame(rgb, st, 64, total, E, frame_spp=spp)
        assert f.accumulated == total
    assert total == 2 ** 24 - 1
    with pytest.raises(pt.PtError) as e:
        pt.render(s, f, cam, 1, 50, rng=pt.RNG_SAMPLE, accumulate=True)
    assert e.value.code == 1
    assert f.accumulated == total
    f.clear()
    assert f.accumulated == 0
    rgb, st = pt.render(s, f, cam, 37, 50, rng=pt.RNG_SAMPLE, chunk=5, accumulate=True)
    check_frame(rgb, st, 64, 37, E)
    assert f.accumulated == 37


# ---------------------------------------------------------------- sample indices at a high base
def test_high_sample_base_equals_the_oracle(pt, orc, gpu):
    """sampleBase + sample is the Philox counter of a sample's stream.  A first accumulating frame of
    2^23 - 3 samples of nothing (no objects, black sky: A = 0 exactly) moves the film's base there;
    the second, 5 samples of the rtiow preset in blocks of 2, crosses 2^23 and must be the oracle's
    samples 2^23 - 3 ... 2^23 + 1: sqrt(S2 * (1 / (2^23 + 2))) bit for bit, and its ray count."""
    w = h = 8
    base = 2 ** 23 - 3
    p = pt.Preset("rtiow", w, h)
    f = pt.Film(w, h, SEED, device=gpu)
    void = pt.Scene(p.objects[:0], p.materials, device=gpu)
    void.set_sky(*cs.BLACK_SKY)
    rgb, st = pt.render(void, f, p.camera, base, 50, rng=pt.RNG_SAMPLE, chunk=4096, accumulate=True)
    assert not rgb.any() and st.rays == st.paths == w * h * base
    assert f.accumulated == base
    s = pt.Scene(p.objects, p.materials, device=gpu)
    rgb, st = pt.render(s, f, p.camera, 5, 50, rng=pt.RNG_SAMPLE, chunk=2, accumulate=True)
    nodes = orc.build_lbvh(p.objects, orc.morton_keys(p.objects), tight=True)
    _, s2, rst = orc.render_sample_sums(p.objects, p.materials, nodes, pt.camera_to_array(p.camera), w, h, f.rows, 5,
                                        50, SEED, 2, sample_base=base, nthreads=4)
    want = np.sqrt((s2 * (np.float32(1.0) / np.float32(base + 5))).astype(np.float32))
    np.testing.assert_array_equal(bits(rgb), bits(want))
    assert st.rays == rst.rays and st.paths == w * h * 5
    assert f.accumulated == base + 5
    # (the samples are the base's own: from base 0 the same five give other sums)
    _, s0, _ = orc.render_sample_sums(p.objects, p.materials, nodes, pt.camera_to_array(p.camera), w, h, f.rows, 5,
                                      50, SEED, 2, sample_base=0, nthreads=4)
    assert (bits(s0) != bits(s2)).any()


# ---------------------------------------------------------------- 8-bit outputs above 1
@pytest.mark.parametrize("rng", ["compat", "sample"])
def test_rgba8_outputs_above_one(pt, orc, gpu, rng):
    """The frame is (32, 2, 0.5): saveColor's quantiser clamps to 0.999 * 256, renderBySurface's
    (unsigned)(c * 255) wraps 8160 and 510 into its 8-bit field."""
    mode = pt.RNG_COMPAT if rng == "compat" else pt.RNG_SAMPLE
    s, cam = device_scene(pt, gpu), camera_of(pt, 8, 8)
    f = pt.Film(8, 8, SEED, device=gpu)
    rgb, st = pt.render(s, f, cam, 16, 50, rng=mode)
    check_frame(rgb, st, 64, 16)
    assert rgb[0].tolist() == [32.0, 2.0, 0.5]
    f.reset()
    q, _ = pt.render(s, f, cam, 16, 50, rng=mode, out_format=pt.OUT_RGBA8)
    np.testing.assert_array_equal(q, np.tile(np.array([255, 255, 128, 255], np.uint8), (64, 1)))
    np.testing.assert_array_equal(q, orc.quantize_png(rgb))
    f.reset()
    sfc, _ = pt.render(s, f, cam, 16, 50, rng=mode, out_format=pt.OUT_RGBA8_SURFACE)
    np.testing.assert_array_equal(sfc, np.tile(np.array([224, 254, 127, 255], np.uint8), (64, 1)))
    np.testing.assert_array_equal(sfc, orc.quantize_surface(rgb))


# ---------------------------------------------------------------- sample mode's limits
def test_frame_width_limit(pt, gpu):
    """A 65536 x 1 film renders in compat mode; sample mode packs pixel coordinates into 16 bits and
    refuses it.  (The camera keeps aspect 1, so that the whole row still looks at the triangle.)"""
    w = 65536
    s, cam = device_scene(pt, gpu), camera_of(pt, 1, 1)
    f = pt.Film(w, 1, SEED, device=gpu)
    rgb, st = pt.render(s, f, cam, 1, 50)
    check_frame(rgb, st, w, 1)
    with pytest.raises(pt.PtError) as e:
        pt.render(s, f, cam, 1, 50, rng=pt.RNG_SAMPLE)
    assert e.value.code == 1 and "65536" in str(e.value)


def test_task_limit_refused(pt, gpu):
    """64 x 32 pixels = 32 tiles, blocks of one sample: 2048 tasks per sample, so spp = 2^21 - 2^15
    is exactly the limit.  At it and above it the render is refused before anything is launched
    (a film that never rendered has no stats); the film then renders a small frame as usual."""
    w, h = 64, 32
    E = (512.0, 4.0, 0.25)
    s, cam = device_scene(pt, gpu, E), camera_of(pt, w, h)
    f = pt.Film(w, h, SEED, device=gpu)
    at = TASK_LIMIT // (32 * 64)
    assert 32 * at * 64 == TASK_LIMIT
    for spp in (at, at + 1, 2 ** 21 - 1):
        with pytest.raises(pt.PtError) as e:
            pt.render(s, f, cam, spp, 50, rng=pt.RNG_SAMPLE, chunk=1)
        assert e.value.code == 1 and "tasks" in str(e.value)
        with pytest.raises(pt.PtError):
            f.stats()
    # (larger blocks bring the same sample count under the limit -- not rendered here)
    rgb, st = pt.render(s, f, cam, 37, 50, rng=pt.RNG_SAMPLE, chunk=1)
    check_frame(rgb, st, w * h, 37, E)


def test_frame_at_the_task_limit(pt, gpu):
    """The largest accepted task count on this film: spp = 2^21 - 2^15 - 1 in blocks of one, 2048
    tasks (one sample of every pixel) under the limit, 4.2 x 10^9 one-ray samples.
    Every persistent wave pushes the 32-bit task counter 64 past the end; the limit leaves room for
    2^20 of them, so no grab wraps and no task runs twice: the frame is exact and so are the
    counters.  (With the earlier limit of 2^32 - 4096 a frame like this one, on a device of more
    than 64 persistent waves, re-rendered itself.)  Radiance 512: N * 512 < 2^31."""
    w, h = 64, 32
    E = (512.0, 4.0, 0.25)
    N = TASK_LIMIT // (32 * 64) - 1
    assert 32 * N * 64 == TASK_LIMIT - 2048 and N * 512 < 2 ** 31
    s, cam = device_scene(pt, gpu, E), camera_of(pt, w, h)
    f = pt.Film(w, h, SEED, device=gpu)
    rgb, st = pt.render(s, f, cam, N, 50, rng=pt.RNG_SAMPLE, chunk=1)
    print(f"at-limit frame: {st.kernel_ms:.1f} ms kernel, {st.rays} rays")
    check_frame(rgb, st, w * h, N, E)
