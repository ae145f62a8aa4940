"""The wide NODE step (pt_device.hip wideHits) on the inputs where its parts can go wrong, on the GPU.

wideHits takes the near / far planes by the signs of 1 / d, scales the plane bytes by the node's
exponent bytes and assembles the children's hit bits by slot and ray octant.  Nothing of that may
show: pixels, ray and path counts, primitive tests and the films' RNG states are compared bit for
bit between the wide kernel, the binary wavefront kernel, the one-lane-per-pixel kernel and the
oracle, at 48 x 40, 4 spp, depth 50, in both RNG modes (compat mode twice on one film, so that the
critical-pixel waves run wideHits in their per-lane loop), on a host-built tree, a device-built one
and after further builds of the same scene; the wide kernel's node visits and primitive tests are
the same on the same tree.  tests/node_step_scenes.py describes the scenes.

Instanced scenes have no oracle: an identity instance gives the flat scene's frame bit for bit
(also on rays parallel to an axis plane, which only the instanced NODE step tests itself,
wideHitsInst), and the frames of cornell under a mirrored and a sheared instance are pinned by
tests/golden/node_step_instanced.npz, recorded before the NODE step was slimmed (DESIGN.md section
11 item 15).
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401  before libpt.so loads (the two must share torch's HIP runtime)

import node_step_scenes as ns
from node_step_scenes import CHUNK, DEPTH, H, SEED, SPP, W
from wall_box import wall_box

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_step_instanced.npz")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame(pt, gpu, s, cam, kernel, rng, launches=1):
    f = pt.Film(W, H, SEED, device=gpu)
    for _ in range(launches):
        rgb, st = pt.render(s, f, cam, SPP, DEPTH, kernel=kernel, rng=rng, chunk=CHUNK if rng == pt.RNG_SAMPLE else 0)
    return rgb, st, f.get_rng()


def oracle_frames(pt, orc, objs, mats, cam):
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    c = pt.camera_to_array(cam)
    rows = np.arange(H, dtype=np.int32)
    sample = orc.render_sample(objs, mats, nodes, c, W, H, rows, SPP, DEPTH, SEED, CHUNK, nthreads=8)
    states = orc.film_states(SEED, W, rows)
    first = orc.render(objs, mats, nodes, c, W, H, rows, SPP, DEPTH, states, nthreads=8)
    after_first = states.copy()
    second = orc.render(objs, mats, nodes, c, W, H, rows, SPP, DEPTH, states, nthreads=8)
    return {"sample": sample, "compat": (first, second), "states": (after_first, states.copy())}


def assert_equals_oracle(pt, gpu, s, cam, ref, kernels, what):
    """Every kernel's frames against the oracle's; returns the wide kernel's (node visits, primitive
    tests) of the first compat launch (fixed tiles, a lane per pixel: the same on the same tree)."""
    counted = len(s.objects) > 1   # (a single primitive is the root: the binary kernels count no test)
    wide = None
    for kernel in kernels:
        msg = f"{what}, kernel {kernel}"
        rgb, st, _ = frame(pt, gpu, s, cam, kernel, pt.RNG_SAMPLE)
        oref, ost = ref["sample"]
        np.testing.assert_array_equal(bits(rgb), bits(oref), err_msg=msg + ", sample mode")
        assert (st.rays, st.paths) == (ost.rays, W * H * SPP), msg
        if kernel == pt.KERNEL_WAVEFRONT and counted:
            assert (st.tri_tests, st.sphere_tests) == (ost.tri_tests, ost.sphere_tests), msg
        for launches in (1, 2):
            rgb, st, rng = frame(pt, gpu, s, cam, kernel, pt.RNG_COMPAT, launches)
            oref, ost = ref["compat"][launches - 1]
            np.testing.assert_array_equal(bits(rgb), bits(oref), err_msg=f"{msg}, compat launch {launches}")
            np.testing.assert_array_equal(rng, ref["states"][launches - 1], err_msg=f"{msg}, compat launch {launches}")
            assert (st.rays, st.paths) == (ost.rays, W * H * SPP), msg
            if kernel == pt.KERNEL_WAVEFRONT and counted:
                assert (st.tri_tests, st.sphere_tests) == (ost.tri_tests, ost.sphere_tests), msg
            if kernel == pt.KERNEL_WIDE and launches == 1:
                wide = (st.node_visits, st.tri_tests + st.sphere_tests)
    return wide


def check_scene(pt, orc, gpu, objs, mats, cam, device_tree=True):
    ref = oracle_frames(pt, orc, objs, mats, cam)
    every = (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT, pt.KERNEL_SIMPLE)
    host_flags, dev_flags = pt.PT_BVH_ORIGIN_BOUNDS, pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_WIDE_DEVICE
    s = pt.Scene(objs, mats, device=gpu)
    first = assert_equals_oracle(pt, gpu, s, cam, ref, every, "host tree")
    assert s.wide_info()["source"] == 1 and first[1] > 0
    if device_tree:
        d = pt.Scene(objs, mats, device=gpu, flags=dev_flags)
        assert d.wide_info()["source"] == 2
        dev = assert_equals_oracle(pt, gpu, d, cam, ref, (pt.KERNEL_WIDE,), "device tree")
        d.build_bvh(dev_flags)   # a second build on the same scene: the buffers are reused
        assert assert_equals_oracle(pt, gpu, d, cam, ref, (pt.KERNEL_WIDE,), "device tree, second build") == dev
        s.build_bvh(dev_flags)   # the host-built scene rebuilt on the device, then on the host again
        assert assert_equals_oracle(pt, gpu, s, cam, ref, (pt.KERNEL_WIDE,), "host tree rebuilt on the device") == dev
    s.build_bvh(host_flags)
    again = assert_equals_oracle(pt, gpu, s, cam, ref, (pt.KERNEL_WIDE,), "host tree, second build")
    assert s.wide_info()["source"] == 1 and again == first


def test_all_octants(pt, orc, gpu):
    """Twelve triangles around the camera: the two cameras' first rays have every sign combination."""
    objs, mats = wall_box(1)
    assert len(objs) == 12
    cams = ns.octant_cameras(pt)
    seen = set()
    for cam in cams:
        seen |= ns.first_ray_octants(orc, pt, cam)
    assert seen == set(range(8)), seen
    for cam in cams:
        check_scene(pt, orc, gpu, objs, mats, cam)


@pytest.mark.parametrize("zero_axes", [(1,), (0,), (0, 1), (1, 2)])
def test_axis_parallel_rays(pt, orc, gpu, zero_axes):
    """Camera rays with one direction component of exactly 0 from a point in the plane that splits the
    box's walls, and with two: the flat scene (such rays take the reference-order query), and the same
    box as an identity instance, whose NODE step culls by the exact slab test on those axes and must
    then select the same planes on the others -- the flat scene's frame bit for bit."""
    objs, mats = wall_box(2)
    axis = next(a for a in (2, 0, 1) if a not in zero_axes)
    origin = ns.CENTRE.copy()
    if len(zero_axes) == 2:   # (one ray: off the splitting planes, where it would only meet the walls' shared edges)
        origin[list(zero_axes)] += np.array([7.25, 3.5], np.float32)
    cam = ns.slit_camera(pt, origin, axis, zero_axes)
    c = pt.camera_to_array(cam)
    for a in zero_axes:
        assert c[3 + a] == c[a] and c[6 + a] == 0.0 and c[9 + a] == 0.0   # lower_left = origin, no extent
    mid = objs["v"].reshape(-1, 3)
    if len(zero_axes) == 1:
        assert (mid[:, zero_axes[0]] == origin[zero_axes[0]]).any(), "the origin lies in no wall-splitting plane"
    check_scene(pt, orc, gpu, objs, mats, cam)
    inst = np.zeros(1, pt.INSTANCE_DTYPE)
    inst["m"] = np.eye(3, 4, dtype=np.float32).reshape(12)
    si = pt.Scene.instanced(objs, [0], [len(objs)], inst, mats, device=gpu)
    sf = pt.Scene(objs, mats, device=gpu)
    for rng in (pt.RNG_SAMPLE, pt.RNG_COMPAT):
        a, ast, arng = frame(pt, gpu, si, cam, pt.KERNEL_WIDE, rng)
        b, bst, brng = frame(pt, gpu, sf, cam, pt.KERNEL_WIDE, rng)
        np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(arng, brng)
        assert (ast.rays, ast.paths) == (bst.rays, bst.paths) == (bst.rays, W * H * SPP)


@pytest.mark.parametrize("exp", [-20, 20])
def test_scaled_cornell(pt, orc, gpu, exp):
    """cornell times 2^exp about the origin: small and large exponent bytes on every axis."""
    p = pt.Preset("cornell", W, H)
    s = np.float32(2.0 ** exp)
    check_scene(pt, orc, gpu, ns.scale_objects(p.objects, s), p.materials, ns.scaled_camera(pt, p.camera, s))


def test_anisotropic_box(pt, orc, gpu):
    """Extents that differ by 2^16 between axes: a different exponent byte per axis."""
    objs, mats, centre = ns.anisotropic_box()
    ext = objs["v"].reshape(-1, 3).max(0) - objs["v"].reshape(-1, 3).min(0)
    assert ext[0] / ext[1] > 2.0 ** 15.9
    cam = pt.camera_make(centre, centre + np.array([256.0, 1.0 / 256.0, 1.0], np.float32), 100.0, W / H)
    check_scene(pt, orc, gpu, objs, mats, cam)


def test_far_camera(pt, orc, gpu):
    """cornell from 20 extents away: the camera rays take the reference-order query (wideFar), the
    bounces the wide tree."""
    p = pt.Preset("cornell", W, H)
    v = p.objects["v"].reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    mid, ext = (lo + hi) / 2, float((hi - lo).max())
    frm = mid + np.array([0.1, 0.05, -20.0], np.float32) * ext
    check_scene(pt, orc, gpu, p.objects, p.materials, pt.camera_make(frm, mid, 4.0, W / H))


@pytest.mark.parametrize("n", [1, 2, 3, 9, 65])
def test_sparse_nodes(pt, orc, gpu, n):
    objs, mats, campar = ns.sparse_scene(n)
    check_scene(pt, orc, gpu, objs, mats, pt.camera_make(*campar))


def test_doubled_wall_box(pt, orc, gpu):
    """Order-dependent queries (every grazing hit has an exact twin): repeated in the reference's order
    by the SHADE step, whatever step ran before it."""
    objs, mats = wall_box(3, doubled=True)
    cam = pt.camera_make((270.0, 280.0, 40.0), (200.0, 250.0, 500.0), 70.0, W / H)
    check_scene(pt, orc, gpu, objs, mats, cam)


def test_sphere_scene(pt, orc, gpu):
    """rtiow: spheres (and a root with nine-plus children) through the same node test."""
    p = pt.Preset("rtiow", W, H)
    check_scene(pt, orc, gpu, p.objects, p.materials, p.camera, device_tree=False)


def test_mirrored_and_sheared_instances(pt, gpu):
    """cornell's meshes under a mirrored and a sheared instance (the direction, 1 / d and the octant
    are recomputed on instance entry): the recorded frames, counts and film states, and the same
    after the transforms are set by an update and the top level is rebuilt."""
    want = np.load(GOLDEN)
    objs, first, count, inst, mats, cam, _ = ns.instanced_case(pt)
    fresh = pt.Scene.instanced(objs, first, count, inst, mats, device=gpu)
    start = inst.copy()
    start["m"] = np.eye(3, 4, dtype=np.float32).reshape(12)
    upd = pt.Scene.instanced(objs, first, count, start, mats, device=gpu)
    upd.update_instances(inst)
    upd.build_bvh()
    for what, s in (("fresh", fresh), ("updated", upd)):
        for name, rng in (("sample", pt.RNG_SAMPLE), ("compat", pt.RNG_COMPAT)):
            rgb, st, states = ns.render_instanced(pt, gpu, s, cam, rng)
            np.testing.assert_array_equal(bits(rgb), want[name + "_rgb"], err_msg=f"{what}, {name}")
            np.testing.assert_array_equal(states, want[name + "_states"], err_msg=f"{what}, {name}")
            assert [st.rays, st.paths] == want[name + "_counts"].tolist(), (what, name)
            assert st.paths == W * H * SPP and st.node_visits > st.rays
