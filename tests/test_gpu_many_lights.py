"""NEE and MIS (PT_RENDER_NEE, PT_RENDER_MIS, PT_BVH_LIGHTS) with hundreds of sampled lights, flat and
instanced: light lists longer than a block (256) and a scan tile (2048 objects), light-less and empty
instances first, between and last, mesh, range and instance orders that all differ, and the list
growing and shrinking by orders of magnitude across rebuilds.

The scenes are tests/many_lights.py's; tests/test_many_lights_host.py holds the conditions on the
reference frames (every event of the rule at least 20 times, picks in every scan tile, scatter rays
that land on the lights of every mesh) and proves that a wrong slot, rank or first-record table moves
the reference frame's bits.  So the bar is bit-exact throughout: lists against the restatements
(pathloop_nee.light_list, instanced_lights_ref.light_list), frames against pathloop_mis's loop or a
fresh scene.
"""
import numpy as np
import pytest

import instanced_lights_ref as ilr
import many_lights as ml
import pathloop_nee as pn
from pathloop import SEED

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def counters(st):
    return (st.rays, st.paths, st.node_visits, st.tri_tests, st.sphere_tests)


def camera_of(pt, sc):
    return pt.Camera.from_buffer_copy(sc.camera.tobytes())


def soup_camera(pt, w, h):
    return pt.camera_make(np.array((0.0, 1.0, 2.5 * ml.SOUP_SPREAD), np.float32), np.zeros(3, np.float32), 60.0, w / h)


def flat_device_scene(pt, gpu, objects, materials, flags=None):
    s = pt.Scene(objects, materials, device=gpu, flags=pt.PT_BVH_ORIGIN_BOUNDS if flags is None else flags)
    s.set_sky(*ml.SOUP_SKY)
    return s


def flat_records(objects, materials):
    return ilr.records(pn.light_list(objects, materials))


# ---------------------------------------------------------------- a. the list at the tile and block edges
EDGE_NS = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 6145)


def test_light_list_at_tile_and_block_edges(pt, gpu):
    """Builds and downloads only.  n objects for n around the list kernel's block (256), the scan's tile
    (2048), two tiles and three, with every pattern of many_lights.edge_list_scene that makes sense at n
    -- all, none, the first object only, the last only, every other one, and lights exactly at objects
    2047, 2048, 4095 and 4096: the count and the records against pathloop_nee.light_list bit for bit.
    The largest n again with host-made keys and with the device-built wide tree: the list does not depend
    on how the tree is built."""
    builds = 0
    for n in EDGE_NS:
        variants = [None]
        if n == EDGE_NS[-1]:
            variants += [pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_HOST_KEYS, pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_WIDE_DEVICE]
        for pattern in ml.edge_patterns(n):
            objs, mats = ml.edge_list_scene(n, pattern)
            want = flat_records(objs, mats)
            assert len(want) == len(ml.edge_light_indices(n, pattern))
            for flags in variants:
                s = flat_device_scene(pt, gpu, objs, mats, flags)
                builds += 1
                assert s.n_lights == len(want), (n, pattern, flags)
                got = s.lights()
                assert got.shape == (len(want), 4, 3) and got.dtype == np.float32
                np.testing.assert_array_equal(bits(got), bits(want), err_msg=str((n, pattern, flags)))
                s.close()
    print("scenes built:", builds)


# ---------------------------------------------------------------- b. flat many-light frames
@pytest.fixture(scope="module")
def flat_scenes(pt, gpu):
    """many_lights.flat_scene() on the device: the host-built tree and the device-built wide tree."""
    sc = ml.flat_scene()
    return {"host": flat_device_scene(pt, gpu, sc.objects, sc.materials),
            "device": flat_device_scene(pt, gpu, sc.objects, sc.materials, pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_WIDE_DEVICE)}


@pytest.fixture(scope="module")
def flat_refs():
    """The four numpy frames of flat_scene() (NEE and MIS, compat and sample mode), computed once,
    before the tests that compare with them (so their run times are the device's)."""
    return {(mis, sample): ml.flat_reference(mis, sample) for mis in (False, True) for sample in (False, True)}


FLAT_CONFIGS = {"simple": ("host", "KERNEL_SIMPLE"), "wide": ("host", "KERNEL_WIDE"),
                "wide_device": ("device", "KERNEL_WIDE")}


def _frames(pt, gpu, scene, cam, sc, mis, **kw):
    """(compat frame, its streams, its Stats, sample frame, its Stats) of one scene."""
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    rgb, st = pt.render(scene, f, cam, sc.spp, sc.max_depth, nee=not mis, mis=mis, **kw)
    states = f.get_rng()
    srgb, sst = pt.render(scene, f, cam, 5, sc.max_depth, rng=pt.RNG_SAMPLE, chunk=2, nee=not mis, mis=mis, **kw)
    np.testing.assert_array_equal(f.get_rng(), states)   # sample mode leaves the film's streams alone
    return rgb, states, st, srgb, sst


def _check_against_reference(frames, refs, mis):
    rgb, states, st, srgb, sst = frames
    ref, sref = refs[mis, False], refs[mis, True]
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(states, ref["states"])
    assert st.rays == ref["rays"] and st.paths == ref["paths"]
    np.testing.assert_array_equal(bits(srgb), bits(sref["image"]))
    assert sst.rays == sref["rays"] and sst.paths == sref["paths"]


@pytest.mark.parametrize("config", list(FLAT_CONFIGS))
def test_flat_many_light_frames_bit_exact(pt, gpu, flat_scenes, flat_refs, config):
    """The 4,500-object soup with 905 sampled lights in three scan tiles, 32 x 24: the list against the
    restatement, then the NEE and the MIS frame in compat mode (3 spp) and sample mode (5 spp, chunk 2)
    against the numpy loop -- image bits, streams, rays and paths -- and the MIS frames' counters
    against the NEE frames'."""
    tree, kernel = FLAT_CONFIGS[config]
    sc = ml.flat_scene()
    s, cam = flat_scenes[tree], camera_of(pt, sc)
    assert s.n_lights == 905
    np.testing.assert_array_equal(bits(s.lights()), bits(flat_records(sc.objects, sc.materials)))
    nee = _frames(pt, gpu, s, cam, sc, False, kernel=getattr(pt, kernel))
    _check_against_reference(nee, flat_refs, False)
    mis = _frames(pt, gpu, s, cam, sc, True, kernel=getattr(pt, kernel))
    _check_against_reference(mis, flat_refs, True)
    assert counters(mis[2]) == counters(nee[2]) and counters(mis[4]) == counters(nee[4])
    np.testing.assert_array_equal(mis[1], nee[1])
    assert (bits(mis[0]) != bits(nee[0])).any() and (bits(mis[3]) != bits(nee[3])).any()


# ---------------------------------------------------------------- c. identity instances
@pytest.fixture(scope="module")
def identity_scenes(pt, gpu):
    objs, first, count, inst, mats = ml.instanced_identity_scene()
    out = {}
    for name, flags in (("host", pt.PT_BVH_LIGHTS), ("device", pt.PT_BVH_LIGHTS | pt.PT_BVH_WIDE_DEVICE)):
        out[name] = pt.Scene.instanced(objs, first, count, inst, mats, device=gpu, flags=flags)
        out[name].set_sky(*ml.SOUP_SKY)
    return out


@pytest.mark.parametrize("mis", [False, True], ids=["nee", "mis"])
@pytest.mark.parametrize("layout", ["host", "device"])
def test_identity_instanced_many_light_frames_bit_exact(pt, gpu, identity_scenes, flat_scenes, flat_refs, layout, mis):
    """The same objects as six meshes (one empty, one without lights) under identity matrices, the mesh
    numbers, the ranges in the object array and the instance order all different: the records are the
    flat list of the flattened objects, and the frames are the numpy loop's of the flattened scene and
    the flat device scene's, bit for bit -- what a wrong rank or first-record lookup would break
    (test_many_lights_host.py: test_a_wrong_slot_table_moves_the_frames_bits)."""
    sc = ml.flat_scene()
    s, cam = identity_scenes[layout], camera_of(pt, sc)
    assert s.n_lights == 905
    np.testing.assert_array_equal(bits(s.lights()), bits(flat_records(sc.objects, sc.materials)))
    got = _frames(pt, gpu, s, cam, sc, mis, kernel=pt.KERNEL_WIDE)
    _check_against_reference(got, flat_refs, mis)
    flat = _frames(pt, gpu, flat_scenes["host"], cam, sc, mis, kernel=pt.KERNEL_WIDE)
    for k in (0, 3):
        np.testing.assert_array_equal(bits(got[k]), bits(flat[k]))
    np.testing.assert_array_equal(got[1], flat[1])
    for k in (2, 4):
        assert (got[k].rays, got[k].paths) == (flat[k].rays, flat[k].paths)


# ---------------------------------------------------------------- d. transformed instances
def transformed(pt, gpu, flags, inst=None, single=False):
    objs, first, count, inst0, mats = ml.instanced_transformed_scene(single=single)
    s = pt.Scene.instanced(objs, first, count, inst0 if inst is None else inst, mats, device=gpu, flags=flags)
    s.set_sky(*ml.SOUP_SKY)
    return s


def xf_camera(pt):
    return pt.camera_make(np.array(ml.XF_CAMERA_FROM, np.float32), np.array(ml.XF_CAMERA_AT, np.float32),
                          ml.XF_CAMERA_VFOV, 1.0)


def test_transformed_many_light_records(pt, gpu):
    """536 records in three blocks of the record kernel, thirteen instances of four meshes (light-less and
    empty ones first, between and last; a mirror, a stretch and a shear among the matrices): the list
    against instanced_lights_ref.light_list bit for bit, the same from the scene laid out for updates,
    and a single instance of the 106-light mesh (the search over one instance)."""
    objs, first, count, inst, mats = ml.instanced_transformed_scene()
    want = ilr.records(ilr.light_list(objs, first, count, inst, mats))
    assert len(want) == 536
    for flags in (pt.PT_BVH_LIGHTS, pt.PT_BVH_LIGHTS | pt.PT_BVH_WIDE_DEVICE):
        s = transformed(pt, gpu, flags)
        assert s.n_lights == 536
        np.testing.assert_array_equal(bits(s.lights()), bits(want), err_msg=str(flags))
    one = ml.instanced_transformed_scene(single=True)
    assert len(one[3]) == 1 and tuple(one[3]["m"][0]) != tuple(np.array(ilr.IDENT, np.float32))
    want1 = ilr.records(ilr.light_list(*one))
    for flags in (pt.PT_BVH_LIGHTS, pt.PT_BVH_LIGHTS | pt.PT_BVH_WIDE_DEVICE):
        s1 = transformed(pt, gpu, flags, single=True)
        assert s1.n_lights == len(want1) == 106
        np.testing.assert_array_equal(bits(s1.lights()), bits(want1), err_msg=str(flags))


def test_many_lights_follow_update_instances(pt, gpu):
    """update_instances on the sub-range [5, 9) -- a 106-light instance, a light-less one, another
    106-light one and the 3-light one -- and a top-level rebuild: the list is a fresh scene's and the
    restatement's and differs from the one before; an NEE sample-mode frame and a MIS compat frame of the
    rebuilt scene are the fresh scene's, bit for bit (image, rays, streams)."""
    objs, first, count, inst, mats = ml.instanced_transformed_scene()
    flags = pt.PT_BVH_WIDE_DEVICE | pt.PT_BVH_LIGHTS
    s = transformed(pt, gpu, flags)
    before = s.lights()
    moved = ml.moved(inst)
    a, b = ml.XF_MOVED
    s.update_instances(moved[a:b], first=a)
    s.build_bvh(flags)
    assert s.wide_info()["source"] == 4
    fresh = transformed(pt, gpu, flags, inst=moved)
    assert fresh.wide_info()["source"] == 3 and s.n_lights == fresh.n_lights == 536
    got = s.lights()
    np.testing.assert_array_equal(bits(got), bits(fresh.lights()))
    np.testing.assert_array_equal(bits(got), bits(ilr.records(ilr.light_list(objs, first, count, moved, mats))))
    changed = np.flatnonzero((bits(got) != bits(before)).any(axis=(1, 2)))
    assert changed.min() == 109 and changed.max() == 323   # the moved instances' records and no other
    cam = xf_camera(pt)
    for kw in (dict(rng=pt.RNG_SAMPLE, nee=True), dict(mis=True)):
        frames = []
        for scene in (s, fresh):
            f = pt.Film(16, 16, 3, device=gpu)
            rgb, st = pt.render(scene, f, cam, 4, 8, **kw)
            frames.append((rgb, st.rays, f.get_rng()))
        np.testing.assert_array_equal(bits(frames[0][0]), bits(frames[1][0]), err_msg=str(kw))
        assert frames[0][1] == frames[1][1]
        np.testing.assert_array_equal(frames[0][2], frames[1][2])
        blind, _ = pt.render(s, pt.Film(16, 16, 3, device=gpu), cam, 4, 8, rng=kw.get("rng", pt.RNG_COMPAT))
        assert (bits(frames[0][0]) != bits(blind)).any()   # (the lights are in the frame)


# ---------------------------------------------------------------- e. growing and shrinking the list
@pytest.mark.parametrize("kernel", ["simple", "wide"])
def test_light_list_grows_and_shrinks_across_rebuilds(pt, gpu, kernel):
    """One scene of the soup's 4,500 objects walked by update_objects through 2, 905, 0, 838 and 5
    lights (many_lights.growth_steps): after each rebuild the count and the records are the
    restatement's, and a MIS compat frame (12 x 8, 2 spp) is a fresh scene's bit for bit -- records left
    over from a longer list are out of reach.  With no light left the MIS frame is the frame without
    the flag, bits and streams."""
    k = {"simple": pt.KERNEL_SIMPLE, "wide": pt.KERNEL_WIDE}[kernel]
    sc = ml.flat_scene()
    w, h, spp = 12, 8, 2
    cam = soup_camera(pt, w, h)
    steps = ml.growth_steps()

    def frame(scene, **kw):
        f = pt.Film(w, h, SEED, device=gpu)
        rgb, st = pt.render(scene, f, cam, spp, sc.max_depth, kernel=k, **kw)
        return rgb, f.get_rng(), counters(st)

    s = flat_device_scene(pt, gpu, steps[0], sc.materials)
    seen = []
    for i, objs in enumerate(steps):
        if i:
            s.update_objects(objs)
            s.build_bvh()
        want = flat_records(objs, sc.materials)
        assert s.n_lights == len(want), i
        np.testing.assert_array_equal(bits(s.lights()), bits(want), err_msg=f"step {i}")
        seen.append(len(want))
        fresh = flat_device_scene(pt, gpu, objs, sc.materials)
        got, ref = frame(s, mis=True), frame(fresh, mis=True)
        np.testing.assert_array_equal(bits(got[0]), bits(ref[0]), err_msg=f"step {i}")
        np.testing.assert_array_equal(got[1], ref[1])
        assert got[2][:2] == ref[2][:2], i
        if len(want) == 0:
            blind = frame(s)
            np.testing.assert_array_equal(bits(got[0]), bits(blind[0]))
            np.testing.assert_array_equal(got[1], blind[1])
            assert got[2] == blind[2]
        fresh.close()
    assert seen == [2, 905, 0, 838, 5]


# ---------------------------------------------------------------- f. scheduling independence
def test_identity_instanced_mis_frame_independent_of_scheduling(pt, gpu, identity_scenes, flat_refs):
    """The identity-instanced MIS sample-mode frame of test c, with other LEAF / SHADE thresholds, in the
    identity launch order and as a 2-way partition of 8-row stripes: the same bits and rays
    (test_instanced_mis_frame_independent_of_scheduling's form)."""
    sc = ml.flat_scene()
    s, cam = identity_scenes["host"], camera_of(pt, sc)
    w, h = sc.width, sc.height
    sref = flat_refs[True, True]

    def frame(film_kw=None, **kw):
        f = pt.Film(w, h, SEED, device=gpu, **(film_kw or {}))
        img, st = pt.render(s, f, cam, 5, sc.max_depth, kernel=pt.KERNEL_WIDE, rng=pt.RNG_SAMPLE, chunk=2, mis=True, **kw)
        return img, st, f

    a, sa, _ = frame()
    np.testing.assert_array_equal(bits(a), bits(sref["image"]))
    assert sa.rays == sref["rays"]
    for kw in ({"leaf_batch": 5, "shade_batch": 40}, {"leaf_batch": 40, "shade_batch": 6}, {"flags": pt.IDENTITY_ORDER}):
        b, sb, _ = frame(**kw)
        np.testing.assert_array_equal(bits(b), bits(a), err_msg=str(kw))
        assert sb.rays == sa.rays, kw
    full = a.reshape(h, w, 3)
    rays = 0
    for part in (0, 1):
        img, st, f = frame({"stripe_height": 8, "n_parts": 2, "part": part})
        assert 0 < f.n_rows < h
        np.testing.assert_array_equal(bits(img.reshape(-1, w, 3)), bits(full[f.rows]))
        rays += st.rays
    assert rays == sa.rays
