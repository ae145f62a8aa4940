"""The wide render kernels' deferred leaf-box rule on the GPU (triangle-only scenes).

The non-instanced wide render kernels keep the plain minimum of (t, rank) in their loop and decide
the reference's leaf-box rule once per ray, in SHADE, from the final hit's exact box
(DevScene::wbox); an order-dependent query is repeated in the reference's order.  Frames, RNG
streams, ray and path counts must equal the reference-order kernels' and the oracle's, bit for bit.
tests/test_wide_deferred_rule.py checks the rule itself on the CPU.
"""
import numpy as np
import pytest
import torch  # before libpt.so loads (the two must share torch's HIP runtime)

from wall_box import wall_box

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, SEED, CHUNK = 48, 40, 4, 50, 7, 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame(pt, gpu, s, cam, w, h, spp, depth, kernel, rng, launches=1, seed=SEED):
    """`launches` renders on one film; returns the last frame, its stats and the film's RNG states."""
    f = pt.Film(w, h, seed, device=gpu)
    for _ in range(launches):
        rgb, st = pt.render(s, f, cam, spp, depth, kernel=kernel, rng=rng, chunk=CHUNK if rng == pt.RNG_SAMPLE else 0)
    return rgb, st, f.get_rng(), f.rows


_oracle = {}


def oracle_frames(pt, orc, name):
    """The oracle's frames of preset `name`, computed once: sample mode, and two successive compat
    launches (the second starts from the first's RNG states)."""
    if name not in _oracle:
        p = pt.Preset(name, W, H)
        nodes = orc.build_lbvh(p.objects, orc.morton_keys(p.objects), tight=True)
        cam = pt.camera_to_array(p.camera)
        rows = np.arange(H, dtype=np.int32)
        sample = orc.render_sample(p.objects, p.materials, nodes, cam, W, H, rows, SPP, DEPTH, SEED, CHUNK, nthreads=8)
        states = orc.film_states(SEED, W, rows)
        first = orc.render(p.objects, p.materials, nodes, cam, W, H, rows, SPP, DEPTH, states, nthreads=8)
        second = orc.render(p.objects, p.materials, nodes, cam, W, H, rows, SPP, DEPTH, states, nthreads=8)
        _oracle[name] = {"sample": sample, "compat": (first, second), "states": states.copy()}
    return _oracle[name]


@pytest.mark.parametrize("name", ["bunny_cornell", "cornell"])
def test_sample_frame_equals_simple_kernel_and_oracle(pt, orc, gpu, name):
    p = pt.Preset(name, W, H)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    wide, wst, _, rows = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_WIDE, pt.RNG_SAMPLE)
    simple, sst, _, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_SIMPLE, pt.RNG_SAMPLE)
    np.testing.assert_array_equal(rows, np.arange(H))
    ref, rst = oracle_frames(pt, orc, name)["sample"]
    np.testing.assert_array_equal(bits(wide), bits(simple))
    np.testing.assert_array_equal(bits(wide), bits(ref))
    assert (wst.rays, wst.paths) == (sst.rays, sst.paths) == (rst.rays, W * H * SPP)
    assert s.wide_info()["source"] == 1


@pytest.mark.parametrize("name", ["bunny_cornell", "cornell"])
def test_compat_two_launches_equal_simple_kernel_and_oracle(pt, orc, gpu, name):
    """Two launches on one film: the second has critical pixels, whose waves run the per-lane loop
    (PT_CRIT_TRACE) with the same deferred rule."""
    p = pt.Preset(name, W, H)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    o = oracle_frames(pt, orc, name)
    for launches in (1, 2):
        wide, wst, wrng, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_WIDE, pt.RNG_COMPAT, launches)
        simple, sst, srng, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_SIMPLE, pt.RNG_COMPAT, launches)
        ref, rst = o["compat"][launches - 1]
        np.testing.assert_array_equal(bits(wide), bits(simple))
        np.testing.assert_array_equal(bits(wide), bits(ref))
        np.testing.assert_array_equal(wrng, srng)
        assert (wst.rays, wst.paths) == (sst.rays, sst.paths) == (rst.rays, W * H * SPP)
    np.testing.assert_array_equal(wrng, o["states"])


def test_lit_frame_equals_simple_kernel(pt, gpu):
    p = pt.Preset("cornell_lit", W, H)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    s.set_sky(*p.sky)
    for rng in (pt.RNG_SAMPLE, pt.RNG_COMPAT):
        wide, wst, wrng, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_WIDE, rng)
        simple, sst, srng, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_SIMPLE, rng)
        np.testing.assert_array_equal(bits(wide), bits(simple))
        np.testing.assert_array_equal(wrng, srng)
        assert (wst.rays, wst.paths) == (sst.rays, sst.paths)
        assert wide.max() > 1.0   # the lamp is seen


def test_device_built_tree_equals_host_built(pt, gpu):
    """PT_BVH_WIDE_DEVICE: the device build writes the exact boxes too; same frames, and the array
    is counted in bvh_info()["device_bytes"]."""
    p = pt.Preset("bunny_cornell", W, H)
    host = pt.Scene(p.objects, p.materials, device=gpu)
    before = host.bvh_info()["device_bytes"]
    dev = pt.Scene(p.objects, p.materials, device=gpu, flags=pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_WIDE_DEVICE)
    for rng in (pt.RNG_SAMPLE, pt.RNG_COMPAT):
        a, ast, arng, _ = frame(pt, gpu, host, p.camera, W, H, SPP, DEPTH, pt.KERNEL_WIDE, rng)
        b, bst, brng, _ = frame(pt, gpu, dev, p.camera, W, H, SPP, DEPTH, pt.KERNEL_WIDE, rng)
        np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(arng, brng)
        assert (ast.rays, ast.paths) == (bst.rays, bst.paths)
    assert (host.wide_info()["source"], dev.wide_info()["source"]) == (1, 2)
    assert host.bvh_info()["device_bytes"] == before + 32 * len(p.objects) == dev.bvh_info()["device_bytes"]


def test_doubled_walls_take_the_redo_branch(pt, gpu):
    """Every bounce starts on a wall and about half of the hits graze their flat box, each with its
    twin inside the window: those queries are repeated in the reference's order
    (test_wide_deferred_rule.py shows the rule firing on this scene; a PT_DIAG build counts 7,057 of
    this sample-mode frame's 24,357 rays redone, none with the walls single)."""
    objs, mats = wall_box(doubled=True)
    s = pt.Scene(objs, mats, device=gpu)
    cam = pt.camera_make((270.0, 280.0, 40.0), (200.0, 250.0, 500.0), 70.0, 1.0)
    for rng in (pt.RNG_SAMPLE, pt.RNG_COMPAT):
        wide, wst, wrng, _ = frame(pt, gpu, s, cam, 32, 32, 2, 12, pt.KERNEL_WIDE, rng)
        simple, sst, srng, _ = frame(pt, gpu, s, cam, 32, 32, 2, 12, pt.KERNEL_SIMPLE, rng)
        np.testing.assert_array_equal(bits(wide), bits(simple))
        np.testing.assert_array_equal(wrng, srng)
        assert (wst.rays, wst.paths) == (sst.rays, sst.paths)
        assert wst.rays > 32 * 32 * 2 * 6   # a closed box: paths run to their depth


def test_sphere_scene_keeps_the_per_candidate_rule(pt, gpu):
    p = pt.Preset("rtiow", W, H)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    for rng in (pt.RNG_SAMPLE, pt.RNG_COMPAT):
        wide, wst, wrng, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_WIDE, rng)
        simple, sst, srng, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_SIMPLE, rng)
        np.testing.assert_array_equal(bits(wide), bits(simple))
        np.testing.assert_array_equal(wrng, srng)
        assert (wst.rays, wst.paths) == (sst.rays, sst.paths)
