"""pt_render_aov on the GPU: the first-hit guide records, bit for bit, against the restatement from the
oracle's closest hits (tests/atrous_ref.py) and against the records built from the library's own
pt_trace_closest_ex(PT_KERNEL_WIDE) of the same pixel-centre rays (include/pt.h defines them so).
"""
import numpy as np
import pytest
import torch  # before libpt.so loads (the two must share torch's HIP runtime)

import atrous_ref
from atrous_ref import lit_soup
from helpers import (OBJECT_DTYPE, random_soup, rays_to_struct, tree_shape_instances,
                     tree_shape_meshes)

pytestmark = pytest.mark.gpu
PT_ERR_STATE = 6


def same_records(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for f in ("obj", "mat"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    for f in ("albedo", "depth", "n", "p"):
        np.testing.assert_array_equal(got[f].view(np.uint32), want[f].view(np.uint32), err_msg=f)


def from_trace(pt, scene, camera, W, H, rows, materials):
    """The records include/pt.h defines: from the scene's own wide closest hits of the pixel-centre rays."""
    rays = atrous_ref.pixel_rays(pt.camera_to_array(camera), W, H, rows)
    hits, _ = scene.trace(rays_to_struct(rays, pt.RAY_DTYPE), tmin=0.001, tmax=float("inf"), kernel=pt.KERNEL_WIDE)
    return atrous_ref.aov_from_hits(hits, rays, materials)


@pytest.fixture(scope="module")
def soup(pt, gpu):
    objs, mats = lit_soup()
    cam = pt.camera_make((0, 0, 28), (0, 0, 0), 50, 37 / 23)
    return objs, mats, cam, pt.Scene(objs, mats, device=gpu)


@pytest.fixture(scope="module")
def soup_ref(pt, orc, soup):
    objs, mats, cam, _ = soup
    return atrous_ref.aov_ref(orc, objs, mats, pt.camera_to_array(cam), 37, 23)


def test_soup_equals_oracle_and_trace(pt, gpu, soup, soup_ref):
    objs, mats, cam, scene = soup
    film = pt.Film(37, 23, 1, device=gpu)
    got, st = pt.render_aov(scene, film, cam)
    same_records(got, soup_ref)
    same_records(got, from_trace(pt, scene, cam, 37, 23, film.rows, mats))
    hit = got["obj"] >= 0
    types = mats["type"][got["mat"][hit]]
    assert hit.sum() >= 50 and (~hit).sum() > 100 and set(types) == {1, 2, 4, 8}
    emis = got[hit][types == 8]
    np.testing.assert_array_equal(emis["albedo"], np.tile(np.float32([1.0, 0.4, 1.0]), (len(emis), 1)))
    np.testing.assert_array_equal(got[hit][types == 4]["albedo"], 1.0)
    assert st.rays == film.n_pixels and st.paths == 0
    assert st.node_visits > 0 and st.tri_tests > 0 and st.sphere_tests > 0 and st.kernel_ms > 0
    assert st.box_tests == 8 * st.node_visits


@pytest.mark.parametrize("name,W,H,typ", [("cornell_lit", 24, 24, 8), ("rtiow", 30, 20, 4)])
def test_preset_albedo_rule(pt, orc, gpu, name, W, H, typ):
    p = pt.Preset(name, W, H)
    scene = pt.Scene(p.objects, p.materials, device=gpu)
    got, _ = pt.render_aov(scene, pt.Film(W, H, 1, device=gpu), p.camera)
    same_records(got, atrous_ref.aov_ref(orc, p.objects, p.materials, pt.camera_to_array(p.camera), W, H))
    hit = got["obj"] >= 0
    seen = p.materials["type"][got["mat"][hit]] == typ
    assert seen.any()   # the lamp / a glass ball is in view
    if typ == 4:
        np.testing.assert_array_equal(got[hit][seen]["albedo"], 1.0)
    else:
        e = p.materials["albedo"][got["mat"][hit][seen]]
        np.testing.assert_array_equal(got[hit][seen]["albedo"], np.minimum(e, np.float32(1)))


def test_device_built_wide_tree(pt, gpu, soup, soup_ref):
    objs, mats, cam, _ = soup
    scene = pt.Scene(objs, mats, device=gpu, flags=pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_WIDE_DEVICE)
    got, _ = pt.render_aov(scene, pt.Film(37, 23, 1, device=gpu), cam)
    assert scene.wide_info()["source"] == 2
    same_records(got, soup_ref)


def test_partitioned_film(pt, orc, gpu, soup):
    objs, mats, _, scene = soup
    W, H = 37, 40
    cam = pt.camera_make((0, 0, 28), (0, 0, 0), 50, W / H)
    full = atrous_ref.aov_ref(orc, objs, mats, pt.camera_to_array(cam), W, H).reshape(H, W)
    film = pt.Film(W, H, 1, device=gpu, stripe_height=8, n_parts=3, part=1)
    assert list(film.rows) == list(range(8, 16)) + list(range(32, 40))
    got, st = pt.render_aov(scene, film, cam)
    same_records(got, full[film.rows].reshape(-1))
    assert st.rays == film.n_pixels == 16 * W


def instanced_world(pt, gpu, count=12, seed=3):
    meshes, mats = tree_shape_meshes()
    m, mesh, reach = tree_shape_instances(count, seed)
    m = m.copy()
    m.reshape(-1, 3, 4)[2, :, 0] *= -1.0   # one mirror (det < 0) among the rotations and scales
    objs = np.concatenate(meshes)
    cnt = np.array([len(x) for x in meshes], np.int64)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    inst = np.zeros(len(m), pt.INSTANCE_DTYPE)
    inst["m"] = m
    inst["mesh"] = mesh
    return pt.Scene.instanced(objs, first, cnt, inst, mats, device=gpu), mats, reach


@pytest.mark.parametrize("far", [False, True], ids=["near", "far-origin"])
def test_instanced_scene_equals_its_trace(pt, gpu, far):
    """Rotated, scaled and mirrored instances: the records of the same scene's wide trace of the same
    rays -- from a camera 40 world extents away too, where the query moves the ray's origin to its
    entry into the world and shifts t back."""
    scene, mats, reach = instanced_world(pt, gpu)
    W, H = 33, 21
    extent = 2.0 * (reach + 8.0)
    cam = (pt.camera_make((0.3 * extent, 0.2 * extent, 40.0 * extent), (0, 0, 0), 1.6, W / H) if far
           else pt.camera_make((0, 0, 2.2 * reach), (0, 0, 0), 60, W / H))
    film = pt.Film(W, H, 1, device=gpu)
    got, st = pt.render_aov(scene, film, cam)
    same_records(got, from_trace(pt, scene, cam, W, H, film.rows, mats))
    hit = got["obj"] >= 0
    assert hit.sum() >= 20 and (~hit).sum() >= 20, hit.sum()
    assert st.rays == W * H


def test_identity_instances_equal_the_flat_scene(pt, gpu):
    a, mats = random_soup(300, 40, seed=11)
    b, _ = random_soup(200, 30, seed=12)
    b["v"][:, :3] += 3.0
    objs = np.concatenate([a, b])
    inst = np.zeros(2, pt.INSTANCE_DTYPE)
    inst["m"] = np.eye(3, 4, dtype=np.float32).reshape(-1)
    inst["mesh"] = [0, 1]
    si = pt.Scene.instanced(objs, [0, len(a)], [len(a), len(b)], inst, mats, device=gpu)
    sf = pt.Scene(objs, mats, device=gpu)
    W, H = 33, 21
    cam = pt.camera_make((0, 0, 30), (0, 0, 0), 50, W / H)
    gi, _ = pt.render_aov(si, pt.Film(W, H, 1, device=gpu), cam)
    gf, _ = pt.render_aov(sf, pt.Film(W, H, 1, device=gpu), cam)
    same_records(gi, gf)
    assert (gf["obj"] >= 0).sum() > 100


def test_small_frames(pt, orc, gpu, soup):
    objs, mats, cam, scene = soup
    at = objs[objs["type"] == 1][0]["v"][:3]   # one pixel, looking at a sphere
    cam1 = pt.camera_make((0, 0, 28), tuple(float(x) for x in at), 5, 1.0)
    one, st = pt.render_aov(scene, pt.Film(1, 1, 1, device=gpu), cam1)
    same_records(one, atrous_ref.aov_ref(orc, objs, mats, pt.camera_to_array(cam1), 1, 1))
    assert st.rays == 1 and one["obj"][0] >= 0
    empty = pt.Scene(np.zeros(0, OBJECT_DTYPE), mats, device=gpu)
    got, st = pt.render_aov(empty, pt.Film(5, 3, 1, device=gpu), cam)
    miss = np.zeros(15, pt.AOV_DTYPE)
    miss["albedo"] = 1
    miss["obj"] = miss["mat"] = -1
    same_records(got, miss)
    assert st.rays == 15 and st.node_visits == 0
    sphere = np.zeros(1, OBJECT_DTYPE)
    sphere["type"] = 1
    sphere["mat"] = 1
    sphere["v"][0, :4] = (0, 0, 0, 6)
    single = pt.Scene(sphere, mats, device=gpu)
    got, _ = pt.render_aov(single, pt.Film(9, 7, 1, device=gpu), cam)
    want = atrous_ref.aov_ref(orc, sphere, mats, pt.camera_to_array(cam), 9, 7)
    same_records(got, want)
    assert (want["obj"] == 0).any() and (want["obj"] < 0).any()


def test_thin_lens_camera_gives_the_pinhole_records(pt, gpu, soup, soup_ref):
    _, _, _, scene = soup
    lens = pt.camera_make((0, 0, 28), (0, 0, 0), 50, 37 / 23, aperture=0.8, focus=10.0)
    assert lens.lens_radius > 0
    pin = pt.Camera.from_buffer_copy(bytes(lens))
    pin.lens_radius = 0.0
    a, _ = pt.render_aov(scene, pt.Film(37, 23, 1, device=gpu), lens)
    b, _ = pt.render_aov(scene, pt.Film(37, 23, 1, device=gpu), pin)
    same_records(a, b)
    assert (a["obj"] >= 0).sum() >= 50


def test_film_state_untouched(pt, gpu, soup):
    _, _, cam, scene = soup
    film = pt.Film(37, 23, 9, device=gpu)
    pt.render(scene, film, cam, 2, 4, accumulate=True)
    rng, acc = film.get_rng(), film.accumulated
    frame_stats = film.stats().as_dict()
    pt.render_aov(scene, film, cam)
    np.testing.assert_array_equal(film.get_rng(), rng)
    assert film.accumulated == acc == 2
    assert film.stats().as_dict() == frame_stats
    a, _ = pt.render(scene, film, cam, 2, 4, accumulate=True)
    other = pt.Film(37, 23, 9, device=gpu)
    pt.render(scene, other, cam, 2, 4, accumulate=True)
    b, _ = pt.render(scene, other, cam, 2, 4, accumulate=True)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_asynchronous_call_on_a_stream(pt, gpu, soup, soup_ref):
    _, _, cam, scene = soup
    film = pt.Film(37, 23, 1, device=gpu)
    dev = torch.device("cuda", gpu)
    stream = torch.cuda.Stream(dev)
    out = torch.zeros(film.n_pixels * 48, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    rec, st = pt.render_aov(scene, film, cam, out=out.data_ptr(), stream=stream.cuda_stream, wait=False)
    assert rec is None and st is None
    stream.synchronize()
    same_records(np.frombuffer(out.cpu().numpy().tobytes(), pt.AOV_DTYPE), soup_ref)
    out.zero_()
    torch.cuda.synchronize(dev)
    _, st = pt.render_aov(scene, film, cam, out=out.data_ptr(), stream=stream.cuda_stream)   # with stats: waits
    assert st.rays == film.n_pixels
    same_records(np.frombuffer(out.cpu().numpy().tobytes(), pt.AOV_DTYPE), soup_ref)


def test_stale_scene_is_refused(pt, gpu):
    objs, mats = lit_soup(7)
    scene = pt.Scene(objs, mats, device=gpu)
    film = pt.Film(5, 3, 1, device=gpu)
    cam = pt.camera_make((0, 0, 28), (0, 0, 0), 50, 5 / 3)
    unbuilt = pt.Scene(objs, mats, device=gpu, build=False)
    with pytest.raises(pt.PtError) as e:
        pt.render_aov(unbuilt, film, cam)
    assert e.value.code == PT_ERR_STATE
    pt.render_aov(scene, film, cam)
    scene.update_objects(objs[:1])
    out = np.full(film.n_pixels, 7, np.uint8).repeat(48).view(pt.AOV_DTYPE)
    with pytest.raises(pt.PtError) as e:
        pt.render_aov(scene, film, cam, out=out)
    assert e.value.code == PT_ERR_STATE
    assert (out.view(np.uint8) == 7).all()
    scene.build_bvh()
    pt.render_aov(scene, film, cam)
