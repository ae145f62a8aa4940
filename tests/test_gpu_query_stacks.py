"""The ray queries' traversal-stack sizes: one small scene per size that a small scene can reach.

The query kernels are instantiated per stack size (binary tree: 16, 24, 32, 48, 64, 80 entries for
depth + 1; wide tree: 8, 16, 24 entries for the depth) and the host picks the instantiation from the
tree's depth (pt_device.hip: stackFor, wideStackFor; bin_stack and wide_stack below mirror them,
as no API reports the chosen size).  Only a scene of the right depth runs a given size, so each
case here first checks that its scene's depth does select the size it names, then that the queued
closest-hit kernel gives the grid-stride kernel's records and work counters (PT_TRACE_STRIDE=1, as
test_gpu_trace_queue.py) and that the occlusion query gives the closest-hit `hit` flags.  The first-hit
AOV kernel (aovKernelWideQ, the wide family's newest member) is held at each wide size, flat and
instanced, to the records include/pt.h defines it by: those of the scene's own wide closest hits of the
pixel-centre rays (test_gpu_aov.py's construction), and on flat scenes to the oracle's as well.

Scenes (depths found on the CPU: the oracle's bvh_depth, and the host wide builder as
test_wide_builder.py drives it):
  binary 16  random soup, 360 primitives                      depth 13
  binary 24  random soup of 1800 + 256 copies of one of them  depth 21
  binary 32  helpers.deep_stack_scene(2)                      depth 26
  binary 48  helpers.deep_stack_scene(256)                    depth 34
  wide 8     the random soup                                  depth 4
  wide 16    200 triangles in geometric progression (1.15)    depth 12
  wide 24    300 triangles in geometric progression (1.1)     depth 18
  instanced  two instances of those three meshes: the mesh's depth + 3 (top level, marker, root)
  AOV        the wide scenes above, and stack_scenes' S16 and S24 (spheres of every material: depth 11
             and 19), seen from their small ends

Not covered: binary 64 and 80.  The LBVH's keys are 30 Morton bits and the object index, so a tree
of n primitives is at most 30 + ceil(log2(n)) levels deep: 64 entries (depth 48..62) need at least
2^18 primitives, and no scene reaches the depth 64 that would select 80.
"""
import numpy as np
import pytest

import atrous_ref
import stack_scenes
from helpers import OBJECT_DTYPE, MATERIAL_DTYPE, deep_stack_scene, random_rays, random_soup, rays_to_struct
from test_gpu_aov import from_trace, same_records
from test_gpu_parity import assert_hits_equal
from test_gpu_trace_queue import both, same_work

pytestmark = pytest.mark.gpu

N_RAYS = 4096


def bin_stack(depth):   # (stackFor)
    return next(s for s in (16, 24, 32, 48, 64, 80) if depth + 1 <= s)


def wide_stack(depth):   # (wideStackFor)
    return next(s for s in (8, 16, 24) if depth <= s)


def soup():
    return random_soup(300, 60, seed=1)


def soup_with_copies():
    objs, mats = random_soup(1500, 300, seed=3)
    return np.concatenate([objs, np.repeat(objs[:1], 256)]), mats


def geometric(n, ratio):
    """Triangle k at x = ratio^k with edges ratio^k / 4: the SAH builder peels the largest ones off at
    every split, so the wide tree of such a chain is a chain too (12 levels for 200, 18 for 300)."""
    objs = np.zeros(n, OBJECT_DTYPE)
    objs["type"] = 3
    x = (ratio ** np.arange(n, dtype=np.float64)).astype(np.float32)
    objs["v"][:, 0] = objs["v"][:, 3] = objs["v"][:, 6] = x
    objs["v"][:, 3] += 0.25 * x
    objs["v"][:, 7] = 0.25 * x
    mats = np.zeros(1, MATERIAL_DTYPE)
    mats["type"] = 1
    mats["albedo"] = 0.5
    return objs, mats


def deep(n_group):
    return lambda: deep_stack_scene(n_group) + ((1024.0, 1024.0, 1024.0),)


def rays_for(objs, inner=None):
    """Half from the scene's bounding sphere, half from around `inner` (default: the scene's low
    corner, where a chain's smallest triangles are; deep_stack_scene: the point inside every sphere),
    so that those cross every level of the tree; half of each aimed at primitives."""
    lo, hi = objs["v"][:, :3].min(0), objs["v"][:, :3].max(0)
    far = random_rays(N_RAYS // 2, seed=31, center=(lo + hi) / 2, radius=float(np.linalg.norm(hi - lo)), objects=objs)
    near = random_rays(N_RAYS // 2, seed=32, center=lo if inner is None else inner, radius=0.5, objects=objs)
    return np.concatenate([far, near])


def check(pt, s, kernel, stack_of, depth_of, stack, rays, monkeypatch):
    r = rays_to_struct(rays, pt.RAY_DTYPE)
    q, qst, ref, rst = both(s, r, kernel, monkeypatch)
    assert stack_of(depth_of()) == stack   # (the wide tree is built by the first wide query)
    assert_hits_equal(q, ref)
    same_work(qst, rst)
    assert qst.rays == len(r) and q["hit"].sum() > 0
    occ, _ = s.occluded(r, kernel=kernel)
    np.testing.assert_array_equal(occ, q["hit"].astype(np.uint8))


@pytest.mark.parametrize("stack,make", [(16, soup), (24, soup_with_copies), (32, deep(2)), (48, deep(256))],
                         ids=["16", "24", "32", "48"])
def test_binary_stack(pt, gpu, monkeypatch, stack, make):
    objs, mats, *inner = make()
    s = pt.Scene(objs, mats, device=gpu)
    check(pt, s, pt.KERNEL_WAVEFRONT, bin_stack, lambda: s.bvh_info()["depth"], stack, rays_for(objs, *inner),
          monkeypatch)


WIDE = [(8, soup), (16, lambda: geometric(200, 1.15)), (24, lambda: geometric(300, 1.1))]


@pytest.mark.parametrize("stack,make", WIDE, ids=["8", "16", "24"])
def test_wide_stack(pt, gpu, monkeypatch, stack, make):
    objs, mats = make()
    s = pt.Scene(objs, mats, device=gpu)
    check(pt, s, pt.KERNEL_WIDE, wide_stack, lambda: s.wide_info()["depth"], stack, rays_for(objs), monkeypatch)


@pytest.mark.parametrize("stack,make", WIDE, ids=["8", "16", "24"])
def test_instanced_stack(pt, gpu, monkeypatch, stack, make):
    objs, mats = make()
    inst = np.zeros(2, pt.INSTANCE_DTYPE)
    inst["m"][:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    inst["m"][1, 7] = 2.0 * float(objs["v"][:, 7].max()) + 1.0   # the second copy: moved up, clear of the first
    s = pt.Scene.instanced(objs, [0], [len(objs)], inst, mats, device=gpu)
    check(pt, s, pt.KERNEL_WIDE, wide_stack, lambda: s.wide_info()["depth"], stack, rays_for(objs), monkeypatch)


# ---------------------------------------------------------------- the AOV kernel at each wide size
AOV_W, AOV_H = 32, 24
SOUP_CAMERA = ((0.0, 0.0, 30.0), (0.0, 0.0, 0.0), 50.0)
CHAIN_CAMERA = ((2.0, 0.3, -2.0), (2.0, 0.3, 0.0), 90.0)   # in front of a chain's small end: 70 of 768 pixels hit


def facing_chains(name):
    sc = stack_scenes.scene(name)
    return lambda: (sc.objects, sc.materials)


# (stack, scene, camera, whether its instanced records are the flat scene's: a copy placed by the identity
# gives them bit for bit unless two primitives tie at exactly the same t, which a flat scene decides in the
# reference's order and an instanced one by (instance, primitive) -- pt.h; the coplanar chains' overlapping
# triangles tie, and the soup's second copy is in view)
WIDE_AOV = [(8, soup, SOUP_CAMERA, False), (16, WIDE[1][1], CHAIN_CAMERA, False), (24, WIDE[2][1], CHAIN_CAMERA, False),
            (16, facing_chains("S16"), stack_scenes.CHAIN_CAMERA, True),
            (24, facing_chains("S24"), stack_scenes.CHAIN_CAMERA, True)]
WIDE_AOV_IDS = ["8", "16", "24", "16-spheres", "24-spheres"]


def check_aov(pt, s, mats, campar, stack, orc_objects=None, orc=None):
    cam = pt.camera_make(*campar, AOV_W / AOV_H)
    film = pt.Film(AOV_W, AOV_H, 1, device=s.device)
    got, st = pt.render_aov(s, film, cam)
    assert wide_stack(s.wide_info()["depth"]) == stack
    same_records(got, from_trace(pt, s, cam, AOV_W, AOV_H, film.rows, mats))
    if orc_objects is not None:
        same_records(got, atrous_ref.aov_ref(orc, orc_objects, mats, pt.camera_to_array(cam), AOV_W, AOV_H))
    hit = got["obj"] >= 0
    assert hit.sum() >= 40 and (~hit).sum() >= 40, hit.sum()
    assert st.rays == AOV_W * AOV_H and st.node_visits > 0
    return got


@pytest.mark.parametrize("stack,make,campar,flat_too", WIDE_AOV, ids=WIDE_AOV_IDS)
def test_wide_stack_aov(pt, orc, gpu, stack, make, campar, flat_too):
    objs, mats = make()
    s = pt.Scene(objs, mats, device=gpu)
    got = check_aov(pt, s, mats, campar, stack, orc_objects=objs, orc=orc)
    if (objs["type"] == 1).any():
        assert (objs["type"][got["obj"][got["obj"] >= 0]] == 1).any()   # a sphere in view


@pytest.mark.parametrize("stack,make,campar,flat_too", WIDE_AOV, ids=WIDE_AOV_IDS)
def test_instanced_stack_aov(pt, gpu, stack, make, campar, flat_too):
    objs, mats = make()
    inst = np.zeros(2, pt.INSTANCE_DTYPE)
    inst["m"][:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    inst["m"][1, 7] = 2.0 * float(objs["v"][:, 7].max()) + 1.0   # the second copy: moved up, clear of the first
    s = pt.Scene.instanced(objs, [0], [len(objs)], inst, mats, device=gpu)
    got = check_aov(pt, s, mats, campar, stack)
    if flat_too:   # (the second copy is far out of view)
        flat, _ = pt.render_aov(pt.Scene(objs, mats, device=gpu), pt.Film(AOV_W, AOV_H, 1, device=gpu),
                                pt.camera_make(*campar, AOV_W / AOV_H))
        same_records(got, flat)
