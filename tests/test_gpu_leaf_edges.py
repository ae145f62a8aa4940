"""The wide LEAF step on edge-form triangle records, on the GPU.

Triangle-only, non-instanced scenes are rendered by the wide kernels from records {v0, rank}{v1 -
v0}{v2 - v0} with a straight-line triangle test (pt_device.hip wideTestTri).  Nothing may change:
pixels, ray and path counts, primitive tests and the films' RNG states are compared bit for bit
between the wide kernel, the binary wavefront kernel, the one-lane-per-pixel kernel and the oracle,
at 32 x 32, 3 spp, depth 50, in both RNG modes (compat mode twice on one film, so that the
critical-pixel waves run), on a host-built tree, a device-built one (PT_BVH_WIDE_DEVICE) and after
further builds of the same scene.  The scenes (tests/leaf_edge_scenes.py) put camera rays on every
decision of the test; each case first checks in numpy that they do.
"""
import numpy as np
import pytest
import torch  # before libpt.so loads (the two must share torch's HIP runtime)

from leaf_edge_scenes import CHUNK, DEPTH, H, SEED, SPP, W, conditions, scenes

pytestmark = pytest.mark.gpu

SCENES = scenes()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame(pt, gpu, s, cam, kernel, rng, launches=1):
    f = pt.Film(W, H, SEED, device=gpu)
    for _ in range(launches):
        rgb, st = pt.render(s, f, cam, SPP, DEPTH, kernel=kernel, rng=rng, chunk=CHUNK if rng == pt.RNG_SAMPLE else 0)
    return rgb, st, f.get_rng()


def oracle_frames(pt, orc, objs, mats, cam):
    """Sample mode, and two successive compat launches (the second starts from the first's states)."""
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    c = pt.camera_to_array(cam)
    rows = np.arange(H, dtype=np.int32)
    sample = orc.render_sample(objs, mats, nodes, c, W, H, rows, SPP, DEPTH, SEED, CHUNK, nthreads=8)
    states = orc.film_states(SEED, W, rows)
    first = orc.render(objs, mats, nodes, c, W, H, rows, SPP, DEPTH, states, nthreads=8)
    after_first = states.copy()
    second = orc.render(objs, mats, nodes, c, W, H, rows, SPP, DEPTH, states, nthreads=8)
    return {"sample": sample, "compat": (first, second), "states": (after_first, states.copy())}


def assert_scene_equals_oracle(pt, gpu, s, cam, ref, kernels, what):
    """Every kernel's frames against the oracle's; returns the wide kernel's primitive-test counts.
    (A single primitive is the root: the binary kernels test it without a traversal and count no test.)"""
    counted = len(s.objects) > 1
    wide_tests = []
    for kernel in kernels:
        msg = f"{what}, kernel {kernel}"
        rgb, st, _ = frame(pt, gpu, s, cam, kernel, pt.RNG_SAMPLE)
        oref, ost = ref["sample"]
        np.testing.assert_array_equal(bits(rgb), bits(oref), err_msg=msg + ", sample mode")
        assert (st.rays, st.paths) == (ost.rays, W * H * SPP), msg
        tests = [st.tri_tests]
        if kernel == pt.KERNEL_WAVEFRONT and counted:   # the reference's primitive tests (the wide tree visits its own)
            assert st.tri_tests == ost.tri_tests, msg
        for launches in (1, 2):
            rgb, st, rng = frame(pt, gpu, s, cam, kernel, pt.RNG_COMPAT, launches)
            oref, ost = ref["compat"][launches - 1]
            np.testing.assert_array_equal(bits(rgb), bits(oref), err_msg=f"{msg}, compat launch {launches}")
            np.testing.assert_array_equal(rng, ref["states"][launches - 1], err_msg=f"{msg}, compat launch {launches}")
            assert (st.rays, st.paths) == (ost.rays, W * H * SPP), msg
            if kernel == pt.KERNEL_WAVEFRONT and counted:
                assert st.tri_tests == ost.tri_tests, msg
            tests.append(st.tri_tests)
        if kernel == pt.KERNEL_WIDE:
            wide_tests = tests
    return wide_tests


def check_scene(pt, orc, gpu, objs, mats, cam, device_tree=True):
    ref = oracle_frames(pt, orc, objs, mats, cam)
    every = (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT, pt.KERNEL_SIMPLE)
    host_flags, dev_flags = pt.PT_BVH_ORIGIN_BOUNDS, pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_WIDE_DEVICE
    s = pt.Scene(objs, mats, device=gpu)
    first = assert_scene_equals_oracle(pt, gpu, s, cam, ref, every, "host tree")
    assert s.wide_info()["source"] == 1 and min(first) > 0   # (the wide kernels count every test)
    if device_tree:
        d = pt.Scene(objs, mats, device=gpu, flags=dev_flags)
        assert d.wide_info()["source"] == 2
        assert_scene_equals_oracle(pt, gpu, d, cam, ref, (pt.KERNEL_WIDE,), "device tree")
        d.build_bvh(dev_flags)   # a second build on the same scene: the buffers are reused
        again = assert_scene_equals_oracle(pt, gpu, d, cam, ref, (pt.KERNEL_WIDE,), "device tree, second build")
        assert d.wide_info()["source"] == 2 and min(again) > 0
        s.build_bvh(dev_flags)   # the host-built scene rebuilt on the device, then on the host again
        assert_scene_equals_oracle(pt, gpu, s, cam, ref, (pt.KERNEL_WIDE,), "host tree rebuilt on the device")
    s.build_bvh(host_flags)
    again = assert_scene_equals_oracle(pt, gpu, s, cam, ref, (pt.KERNEL_WIDE,), "host tree, second build")
    assert s.wide_info()["source"] == 1
    # the same tree: the same primitive tests (the first compat launch: fixed tiles, a lane per pixel;
    # in sample mode the lanes' tasks, and with them what a speculating lane visits, vary from run to run)
    assert again[1] == first[1]


def test_bunny_cornell(pt, orc, gpu):
    p = pt.Preset("bunny_cornell", W, H)
    check_scene(pt, orc, gpu, p.objects, p.materials, p.camera)


# (huge: host tree only -- the device builder's fp32 surface areas are not made for 2^61 coordinates)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_hand_made_scene(pt, orc, gpu, name):
    objs, mats, campar = SCENES[name]
    cam = pt.camera_make(*campar)
    if name in ("degenerate", "huge", "ties"):
        met = conditions(orc, name, objs, pt.camera_to_array(cam))
        assert met, name
        for what, rays in met.items():
            assert rays > 0, f"{name}: no camera ray with {what}"
    check_scene(pt, orc, gpu, objs, mats, cam, device_tree=name != "huge")


@pytest.mark.parametrize("rng", ["sample", "compat"])
def test_sphere_scene_is_unchanged(pt, gpu, rng):
    """A scene with spheres has no edge records: its LEAF step reads the vertices (wideTest)."""
    p = pt.Preset("rtiow", W, H)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    r = pt.RNG_SAMPLE if rng == "sample" else pt.RNG_COMPAT
    launches = 1 if rng == "sample" else 2
    wide, wst, wrng = frame(pt, gpu, s, p.camera, pt.KERNEL_WIDE, r, launches)
    simple, sst, srng = frame(pt, gpu, s, p.camera, pt.KERNEL_SIMPLE, r, launches)
    np.testing.assert_array_equal(bits(wide), bits(simple))
    np.testing.assert_array_equal(wrng, srng)
    assert (wst.rays, wst.paths) == (sst.rays, sst.paths) and wst.sphere_tests > 0


@pytest.mark.parametrize("rng", ["sample", "compat"])
def test_instanced_scene_is_unchanged(pt, gpu, rng):
    """An instanced scene has none either: cornell's one identity instance gives the flattened
    scene's frame bit for bit (tests/test_gpu_instancing.py), from the vertex records."""
    r = pt.RNG_SAMPLE if rng == "sample" else pt.RNG_COMPAT
    ip, fp = pt.InstancedPreset("cornell", W, H), pt.Preset("cornell", W, H)
    si = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, ip.instances, ip.materials, device=gpu)
    sf = pt.Scene(fp.objects, fp.materials, device=gpu)
    a, ast, arng = frame(pt, gpu, si, ip.camera, pt.KERNEL_WIDE, r)
    b, bst, brng = frame(pt, gpu, sf, fp.camera, pt.KERNEL_WIDE, r)
    np.testing.assert_array_equal(bits(a), bits(b))
    np.testing.assert_array_equal(arng, brng)
    assert (ast.rays, ast.paths) == (bst.rays, bst.paths) == (bst.rays, W * H * SPP)
