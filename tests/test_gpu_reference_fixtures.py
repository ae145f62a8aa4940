"""The HIP path (through the C ABI) against tests/golden/reference_fixtures.npz: outputs of the
reference's OWN code (compiled for the CPU, tools/make_reference_fixtures.py), so these tests tie
the kernels to the reference directly, with no oracle and no reference tree at run time.
Tolerance 0 everywhere; a NaN equals any NaN; pixel 0 of a frame is left out (main.cu:286)."""
import os

import numpy as np
import pytest

from helpers import INSTANCE_DTYPE, rays_to_struct

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(REPO, "tests", "golden", "reference_fixtures.npz")
LBVH = [(k, n) for k in ("soup", "dup") for n in (1, 2, 3, 7, 64, 65, 1000)]
DEG = ("soup_negr", "one_sphere", "one_sphere_negr", "one_triangle")
FRAMES = ("rtiow", "triangle_world", "cornell", "l2")


@pytest.fixture(scope="module")
def fx():
    with np.load(FIX) as d:
        return {k: d[k] for k in d.files}


def canon(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def assert_bits(got, want, what=""):
    np.testing.assert_array_equal(canon(got), canon(want), err_msg=what)


def camera(pt, arr):
    return pt.Camera.from_buffer_copy(np.ascontiguousarray(arr, np.float32).tobytes())


@pytest.mark.parametrize("host_keys", [False, True], ids=["device_keys", "host_keys"])
@pytest.mark.parametrize("kind,n", LBVH)
def test_device_lbvh(pt, gpu, fx, kind, n, host_keys):
    """Device LBVH == the reference's topology, and device box U {origin} == the reference's box."""
    objs, ref = fx[f"lbvh_{kind}_{n}_objects"], fx[f"lbvh_{kind}_{n}_nodes"]
    flags = pt.PT_BVH_ORIGIN_BOUNDS | (pt.PT_BVH_HOST_KEYS if host_keys else 0)
    s = pt.Scene(objs, fx["lbvh_materials"], device=gpu, flags=flags)
    g = s.download_bvh()
    for f in ("left", "right", "parent", "objid"):
        np.testing.assert_array_equal(g[f], ref[f], err_msg=f)
    k = n - 1
    assert_bits(np.minimum(g["bmin"][:k], np.float32(0)), ref["bmin"][:k], "internal bmin")
    assert_bits(np.maximum(g["bmax"][:k], np.float32(0)), ref["bmax"][:k], "internal bmax")
    assert_bits(g["bmin"][k:], ref["bmin"][k:], "leaf bmin")
    assert_bits(g["bmax"][k:], ref["bmax"][k:], "leaf bmax")


def expected_hits(fx, scene):
    """The reference's records under pt.h's one stated change: a record whose t is NaN is the miss
    record.  (A ray the reference carried through a NaN candidate to a finite one -- `via_nan`, none
    in the file as recorded -- takes the file's lib_hits record.)"""
    hits, via = fx[f"deg_{scene}_hits"].copy(), fx[f"deg_{scene}_via_nan"]
    hits["obj"] = fx[f"deg_{scene}_lib_hits"]["obj"]   # hit_record has no object id
    nan_t = (hits["hit"] == 1) & np.isnan(hits["t"])
    miss = np.zeros(1, hits.dtype)
    miss["obj"] = miss["mat"] = -1
    hits[nan_t] = miss[0]
    hits[via] = fx[f"deg_{scene}_lib_hits"][via]
    return hits


@pytest.mark.parametrize("tree", ["binary", "wide_host", "wide_device"])
@pytest.mark.parametrize("scene", DEG)
def test_closest_hits_and_occlusion(pt, gpu, fx, scene, tree):
    """pt_trace_closest_ex on the recorded degenerate and ordinary rays -- the binary kernel, the wide
    kernel on a host-built tree and on a device-built one -- and pt_trace_occluded == the hit flag."""
    flags = pt.PT_BVH_ORIGIN_BOUNDS | (pt.PT_BVH_WIDE_DEVICE if tree == "wide_device" else 0)
    s = pt.Scene(fx[f"deg_{scene}_objects"], fx["deg_materials"], device=gpu, flags=flags)
    kernel = pt.KERNEL_SIMPLE if tree == "binary" else pt.KERNEL_WIDE
    rays = rays_to_struct(fx[f"deg_{scene}_rays"], pt.RAY_DTYPE)
    want = expected_hits(fx, scene)
    got, _ = s.trace(rays, kernel=kernel)
    if tree != "binary" and len(s.objects) > 1:
        assert s.wide_info()["source"] == (2 if tree == "wide_device" else 1)
    for f in ("hit", "obj", "mat", "front_face"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    for f in ("t", "p", "n"):   # a miss record's are zero on both sides
        assert_bits(got[f], want[f], f)
    occ, _ = s.occluded(rays, kernel=kernel)
    np.testing.assert_array_equal(occ, want["hit"].astype(np.uint8))


def render_launches(pt, gpu, scene, fx, name, kernel):
    w, h, spp, depth, seed, launches = (int(v) for v in fx[f"fr_{name}_params"])
    film = pt.Film(w, h, seed, device=gpu)
    cam = camera(pt, fx[f"fr_{name}_camera"])
    for launch in range(launches):   # a later launch continues the film's streams
        rgb, st = pt.render(scene, film, cam, spp, depth, kernel=kernel)
        assert st.paths == w * h * spp
        assert_bits(rgb[1:], fx[f"fr_{name}_rgb"][launch][1:], f"{name} launch {launch} image")
        np.testing.assert_array_equal(film.get_rng()[1:], fx[f"fr_{name}_states"][launch][1:],
                                      err_msg=f"{name} launch {launch} streams")


@pytest.mark.parametrize("kernel", ["simple", "wavefront", "wide"])
@pytest.mark.parametrize("name", FRAMES)
def test_compat_frames(pt, gpu, fx, name, kernel):
    """Frames of the three kernels and pt_film_get_rng afterwards == the reference's frames and states."""
    assert bytes(fx["draw_order"]) == b"xyz"
    s = pt.Scene(fx[f"fr_{name}_objects"], fx[f"fr_{name}_materials"], device=gpu)
    k = {"wide": pt.KERNEL_WIDE, "wavefront": pt.KERNEL_WAVEFRONT, "simple": pt.KERNEL_SIMPLE}[kernel]
    render_launches(pt, gpu, s, fx, name, k)


@pytest.mark.parametrize("name", FRAMES)
def test_identity_instance_frames(pt, gpu, fx, name):
    """The same frames through a scene of one identity instance: bit-equal, as pt.h promises."""
    objs = fx[f"fr_{name}_objects"]
    inst = np.zeros(1, INSTANCE_DTYPE)
    inst["m"][0] = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(-1)
    s = pt.Scene.instanced(objs, [0], [len(objs)], inst, fx[f"fr_{name}_materials"], device=gpu)
    render_launches(pt, gpu, s, fx, name, pt.KERNEL_WIDE)
