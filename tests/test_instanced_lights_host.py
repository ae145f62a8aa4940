"""Sampled lights of instanced scenes (PT_BVH_LIGHTS), the part that needs no GPU: the ABI additions
and the float64 restatement of the light-record rule (tests/instanced_lights_ref.py), which the GPU
tests compare the device's list against bit for bit."""
import ctypes as C

import numpy as np

import instanced_lights_ref as ilr
import pathloop_nee as pn
from helpers import INSTANCE_DTYPE


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_abi_additions(pt):
    assert hasattr(pt.lib, "pt_scene_download_lights")
    assert pt.PT_BVH_LIGHTS == 8
    others = (pt.PT_BVH_ORIGIN_BOUNDS, pt.PT_BVH_HOST_KEYS, pt.PT_BVH_WIDE_DEVICE)
    assert all(pt.PT_BVH_LIGHTS & o == 0 for o in others) and len(set(others + (pt.PT_BVH_LIGHTS,))) == 4
    assert pt.lib.pt_abi_version() == 1


def test_download_lights_null_scene(pt):
    """A NULL scene is PT_ERR_INVALID before any device is looked for."""
    buf = np.full(12, -7.0, np.float32)
    assert pt.lib.pt_scene_download_lights(None, buf.ctypes.data_as(C.c_void_p)) == 1
    assert "pt_scene_download_lights" in pt.lib.pt_last_error().decode()
    assert (buf == -7.0).all()
    assert pt.lib.pt_scene_download_lights(None, None) == 1


def _identity_instance(n):
    inst = np.zeros(1, INSTANCE_DTYPE)
    inst["m"][0] = ilr.IDENT
    return [0], [n], inst


def test_identity_matrix_gives_the_flat_list():
    """N1 and N2 as one mesh under the identity: the flat scene's records bit for bit (x * 1 and + 0 are
    exact in float64, and the one rounding to float32 returns the float32 vertex)."""
    for name in ("N1", "N2"):
        sc = pn.nee_scene(name)
        want = pn.light_list(sc.objects, sc.materials)
        first, count, inst = _identity_instance(len(sc.objects))
        got = ilr.light_list(sc.objects, first, count, inst, sc.materials)
        assert len(got[0]) == len(want[0]) > 0
        for g, w in zip(got, want):
            np.testing.assert_array_equal(bits(g), bits(w))


def test_list_order_and_count():
    """Instances in order, each its mesh's emissive triangles in object order; nL from the meshes alone."""
    objs, first, count, inst, mats = ilr.lamp_scene()
    v0, e1, e2, E = ilr.light_list(objs, first, count, inst, mats)
    assert len(v0) == 10 and ilr.records((v0, e1, e2, E)).shape == (10, 4, 3)
    np.testing.assert_array_equal(E, np.tile(np.array(ilr.LAMP_E, np.float32), (10, 1)))
    flat = pn.light_list(objs, mats)
    for k in range(2):   # the identity lamp
        np.testing.assert_array_equal(bits(v0[k]), bits(flat[0][k]))
        np.testing.assert_array_equal(bits(e1[k]), bits(flat[1][k]))
    moved = ilr.light_list(objs, first, count, ilr.moved_instances(inst), mats)
    assert len(moved[0]) == 10
    changed = [k for k in range(10) if (bits(moved[0][k]) != bits(v0[k])).any()]
    assert changed == [2, 3, 6, 7]   # lamps 1 and 3


def test_mirror_keeps_the_area():
    """|cross(e1, e2)| -- the light's area and 1 / pdf -- under a mirrored matrix equals the unmirrored
    one's: the cross product only flips sign.  The two lists round their vertices independently (the
    mirrored coordinates are other float32 values), so the bar is the rounding of the operands, derived,
    not measured: a world coordinate below 16 is rounded by at most half an ulp, 4.8e-7, an edge component
    by two of those, an edge vector by sqrt(3) times that, 1.65e-6; the edges are at most 11.4 long (the
    quad's diagonal at scale 2), so each list's |cross| is off by at most 2 * 1.65e-6 * 11.4 = 3.8e-5 and
    the two lists differ by at most 7.5e-5 (the areas themselves are taken in float64): the bar is 1e-4
    on areas of 4 to 64."""
    objs, first, count, inst, mats = ilr.lamp_scene()
    rng = np.random.default_rng(5)
    for _ in range(20):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a = q * rng.uniform(0.5, 2.0)
        t = rng.uniform(-4, 4, (3, 1))   # (|coordinate| <= 4 + 2 * |(2, 5, 2)| < 16)
        pair = inst[:2].copy()
        pair["mesh"] = 0
        pair["m"][0] = np.concatenate([a, t], 1).reshape(-1)
        pair["m"][1] = np.concatenate([a @ np.diag([-1.0, 1.0, 1.0]), t], 1).reshape(-1)
        v0, e1, e2, _ = ilr.light_list(objs, first, count, pair, mats)
        area = np.linalg.norm(np.cross(e1.astype(np.float64), e2.astype(np.float64)), axis=1)
        assert (area > 1.0).all()
        np.testing.assert_allclose(area[2:], area[:2], rtol=0, atol=1e-4)
