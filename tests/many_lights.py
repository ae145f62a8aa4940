"""Scenes with hundreds of sampled lights, flat and instanced (a helper module, not a test file).

The NEE / MIS scenes of pathloop_nee.py, pathloop_mis.py and instanced_lights_ref.py have 2 to 10
lights.  The scenes here put the light machinery where its indexing is hardest: a light list longer than
one block (256) and one scan tile (2048 objects), instances without lights first, between and last, an
empty mesh among them, mesh ranges, mesh numbers and instance order that all differ, and light counts
that are no power of two.  tests/test_many_lights_host.py holds the conditions the GPU tests
(tests/test_gpu_many_lights.py) rely on.

  flat_scene()                   the soup below, flattened: 4,500 objects, 905 sampled lights in three scan tiles
  instanced_identity_scene()     the same objects as five meshes and an empty one under identity matrices
  instanced_transformed_scene()  a 106-light mesh five times and a 3-light mesh twice: 536 records, three blocks
  edge_list_scene(n, pattern)    n objects with lights at chosen indices (list building only, never rendered)
"""
import contextlib
import functools

import numpy as np

import instanced_lights_ref as ilr
import oracle as orc
import pathloop
import pathloop_mis as pm
from helpers import INSTANCE_DTYPE, random_soup, random_transforms
from pathloop import SEED

F = np.float32
PT_SPHERE, PT_LAMBERTIAN, PT_TRIANGLE, PT_EMISSIVE = 1, 1, 3, 8
SCAN_TILE, BLOCK = 2048, 256   # the flat list's scan tile (256 x 8 items); lightListKernel's / instLightKernel's block


def is_light(objects, materials):
    return (objects["type"] == PT_TRIANGLE) & (materials["type"][objects["mat"]] == PT_EMISSIVE)


# ---------------------------------------------------------------- the soup, flat and as identity instances
# random_soup(4400, 100, seed 3001, spread 14, n_mat 5) with material 4 emissive, E = (4, 3, 0.5), seen as
# pathloop_nee's N2 is: from (0, 1, 2.5 * spread) towards the origin, vfov 60, under N2's sky, depth 12.
# The soup's objects are dealt into five meshes (the identity split), and the flat scene is that split
# flattened, so one numpy reference holds the flat and the instanced frames:
#
#   flattened order   L  the first 300 objects of the soup that are no sampled light (Lambertian, metal and
#                        glass triangles and spheres, emissive spheres among them)      objects    0 ..  299
#                     A  the next 1,500 of the remaining 4,200, in soup order                       300 .. 1799
#                     B  the next 500   (scan tile 0 ends inside it, at object 2047)               1800 .. 2299
#                     C  the next 1,300                                                            2300 .. 3599
#                     D  the last 900   (scan tile 1 ends inside it, at object 4095)               3600 .. 4499
#   instances         L, A, empty, B, C, empty, D, empty          (lightless first; empty between and last)
#   mesh numbers      0 = C, 1 = empty, 2 = A, 3 = L, 4 = D, 5 = B  (instance order != mesh order)
#   object array      D, A, L, C, B                                 (mesh 0 is the fourth range)
#
# flat_scene()'s docstring says how the seed, the spread and the frame were chosen.
SOUP_TRIANGLES, SOUP_SPHERES, SOUP_SEED, SOUP_SPREAD = 4400, 100, 3001, 14.0
SOUP_E = (4.0, 3.0, 0.5)
SOUP_SKY = ((0.2, 0.1, 0.3), (0.9, 0.8, 0.1))
FLAT_W, FLAT_H, FLAT_SPP, FLAT_DEPTH = 32, 24, 3, 12
SPLIT_SIZES = {"L": 300, "A": 1500, "B": 500, "C": 1300, "D": 900}
SPLIT_INSTANCES = ("L", "A", "", "B", "C", "", "D", "")           # "" = the empty mesh
SPLIT_MESHES = ("C", "", "A", "L", "D", "B")                      # mesh number -> part
SPLIT_STORAGE = ("D", "A", "L", "C", "B")                         # the parts' order in the object array
LIGHT_PARTS = ("A", "B", "C", "D")


@functools.lru_cache(maxsize=None)
def _soup_parts():
    objs, mats = random_soup(SOUP_TRIANGLES, SOUP_SPHERES, SOUP_SEED, spread=SOUP_SPREAD, n_mat=5)
    mats[4]["type"] = PT_EMISSIVE
    mats[4]["albedo"] = SOUP_E
    mats[4]["fuzz"] = mats[4]["ir"] = 0.0
    dark = np.flatnonzero(~is_light(objs, mats))[:SPLIT_SIZES["L"]]
    rest = np.setdiff1d(np.arange(len(objs)), dark)   # (sorted: soup order)
    parts, at = {"L": objs[dark], "": objs[:0]}, 0
    for name in LIGHT_PARTS:
        parts[name] = objs[rest[at:at + SPLIT_SIZES[name]]]
        at += SPLIT_SIZES[name]
    assert at == len(rest)
    return parts, mats


def instanced_identity_scene():
    """(objects, mesh_first, mesh_count, instances, materials) of the identity split above."""
    parts, mats = _soup_parts()
    objs = np.concatenate([parts[p] for p in SPLIT_STORAGE])
    start, at = {}, 0
    for p in SPLIT_STORAGE:
        start[p] = at
        at += len(parts[p])
    start[""] = start["L"] + 7   # the empty mesh: a range of length 0 somewhere inside the array
    first = np.array([start[p] for p in SPLIT_MESHES], np.int64)
    count = np.array([len(parts[p]) for p in SPLIT_MESHES], np.int64)
    inst = np.zeros(len(SPLIT_INSTANCES), INSTANCE_DTYPE)
    inst["m"][:] = ilr.IDENT
    inst["mesh"] = [SPLIT_MESHES.index(p) for p in SPLIT_INSTANCES]
    return objs, first, count, inst, mats.copy()


def flattened(objects, mesh_first, mesh_count, instances):
    """The flattened object array of an instanced scene under identity matrices: instances in order,
    each contributing its mesh's objects."""
    return np.concatenate([objects[int(mesh_first[i["mesh"]]):int(mesh_first[i["mesh"]]) + int(mesh_count[i["mesh"]])]
                           for i in instances])


def flat_part_ranges():
    """Part name -> (first, end) in the flattened object array, for the non-empty parts."""
    out, at = {}, 0
    for p in SPLIT_INSTANCES:
        if p:
            out[p] = (at, at + SPLIT_SIZES[p])
            at += SPLIT_SIZES[p]
    return out


@functools.lru_cache(maxsize=None)
def flat_scene():
    """The soup as a flat scene: the identity split flattened (a pathloop.LitScene, 32 x 24, 3 spp, depth 12).
    Chosen on the CPU with pathloop_mis's loop (compat mode, MIS, 3 spp) for the conditions of
    tests/test_many_lights_host.py: every event but `clamped` and the weighted emitter hits at least 20
    times, picks in every scan tile, at least 3 scatter-ray hits on the lights of each of A, B, C, D.
      seed 3001, spread 14, 24 x 16   unoccluded 50, occluded 114, back-facing 177, weighted emitter hits 32,
                                      after specular 28; 341 picks of 279 lights; hits A 14, B 3, C 9, D 6 --
                                      B at the floor itself, so the frame grew
      seed 3001, spread 14, 32 x 24   107 / 293 / 425 / 58 / 64; 825 picks of 540 lights, light 0 among them;
                                      hits 21 / 5 / 19 / 13; 0.3 s of Python a frame            <- chosen
      seed 3002, spread 14, 32 x 24   89 / 219 / 387 / 59 / 68; hits 20 / 7 / 21 / 11   (857 lights)
      seed 3003, spread 14, 32 x 24   92 / 227 / 357 / 52 / 70; hits 15 / 9 / 15 / 13   (904 lights)
      seed 3004, spread 14, 32 x 24   120 / 266 / 413 / 55 / 59; hits 18 / 6 / 21 / 10  (889 lights)
      seed 3001, spread 10, 32 x 24   85 / 621 / 757 / 159 / 159; hits 65 / 13 / 46 / 35: denser, mostly occluded
      seed 3001, spread 18, 32 x 24   117 / 131 / 260 / 28 / 34; hits 7 / 0 / 15 / 6: no hit on B's lights
    Every spread-14 candidate at 32 x 24 would do; 3001 is the soup the many-light gap was first measured
    on.  None shows `clamped`.  The sample-mode frame (5 spp, chunk 2) of the chosen one: 182 / 456 / 719 /
    110 / 106, 1,357 picks of 698 lights, hits 39 / 9 / 30 / 32."""
    objs, first, count, inst, mats = instanced_identity_scene()
    cam = orc.camera_make((0.0, 1.0, 2.5 * SOUP_SPREAD), (0.0, 0.0, 0.0), 60.0, FLAT_W / FLAT_H)
    return pathloop.LitScene("many", flattened(objs, first, count, inst), mats, cam, FLAT_W, FLAT_H, FLAT_SPP, FLAT_DEPTH,
                             SOUP_SKY)


@contextlib.contextmanager
def recorded(slots=None):
    """While active, pathloop_mis records (picks, hits): the light index k of every light sample, and
    the slot of every sampled light a weighted scatter ray landed on (MIS runs); `slots` (optional)
    replaces the object-to-slot table -- the teeth experiments' wrong tables.  The loops' arithmetic is
    untouched: the recorders call the originals."""
    picks, hits = [], []
    pick0, weight0, slots0 = pm.pick_light, pm.emitter_weight, pm.light_slots

    def pick(uL, nL):
        picks.append(pick0(uL, nL))
        return picks[-1]

    def weight(lights, slot, t, d, pbs):
        hits.append(slot)
        return weight0(lights, slot, t, d, pbs)

    pm.pick_light, pm.emitter_weight = pick, weight
    if slots is not None:
        pm.light_slots = lambda objects, materials: slots
    try:
        yield picks, hits
    finally:
        pm.pick_light, pm.emitter_weight, pm.light_slots = pick0, weight0, slots0


def render_flat(sc, mis, sample=False, spp=None, width=None, height=None, slots=None, objects=None, nee=True):
    """A frame of the numpy loop over the LitScene `sc` (compat mode from film seed SEED, or sample mode
    5 spp chunk 2 as the existing tests); the result has two more entries, picks and hits (see recorded).
    `objects` replaces the scene's (another material assignment of the same geometry)."""
    w, h = width or sc.width, height or sc.height
    objs = sc.objects if objects is None else objects
    nodes = sc.nodes if objects is None else orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    cam = sc.camera
    if (w, h) != (sc.width, sc.height):
        cam = orc.camera_make((0.0, 1.0, 2.5 * SOUP_SPREAD), (0.0, 0.0, 0.0), 60.0, w / h)
    with recorded(slots) as (picks, hits):
        if sample:
            r = pm.render_sample(objs, sc.materials, nodes, cam, w, h, range(h), 5 if spp is None else spp,
                                 sc.max_depth, SEED, 2, sky=sc.sky, nee=nee, mis=mis)
        else:
            r = pm.render(objs, sc.materials, nodes, cam, w, h, range(h), sc.spp if spp is None else spp, sc.max_depth,
                          orc.film_states(SEED, w, range(h)), sky=sc.sky, nee=nee, mis=mis)
    r["picks"], r["hits"] = picks, hits
    return r


@functools.lru_cache(maxsize=None)
def flat_reference(mis, sample=False):
    """The shared reference frames of flat_scene(); computed once, read-only."""
    return render_flat(flat_scene(), mis, sample)


# ---------------------------------------------------------------- transformed instances
# Mesh 0 "big": random_soup(300, 16, seed 3107, spread 4, n_mat 6), materials 4 and 5 emissive with
#   E = (4, 3, 0.5) and (0.5, 2, 6): 106 emissive triangles interleaved with 210 other objects.
# Mesh 1 "empty".  Mesh 2 "dark": random_soup(40, 6, seed 3102, spread 3, n_mat 4) -- no emissive material.
# Mesh 3 "small": five triangles, the first, third and fifth emissive (materials 5, 4, 5).
# The object array stores them as dark, small, big, so mesh 0 is the last range.
# Thirteen instances: dark, empty, big, small, empty, big, dark, big, small, big, big, empty, dark --
# lightless and empty ones first, between and last.  Their first records: 0, 0, 0, 106, 109, 109, 215, 215,
# 321, 324, 430, 536, 536; nL = 536 = 2 * 256 + 24 (three blocks of instLightKernel; blocks 0 and 1 each end
# inside an instance), and no light-bearing instance but the first starts on a multiple of 256.
XF_BIG = dict(n_tri=300, n_sph=16, seed=3107, spread=4.0, n_mat=6)
XF_DARK = dict(n_tri=40, n_sph=6, seed=3102, spread=3.0, n_mat=4)
XF_E = ((4.0, 3.0, 0.5), (0.5, 2.0, 6.0))
XF_INSTANCES = ("dark", "empty", "big", "small", "empty", "big", "dark", "big", "small", "big", "big", "empty", "dark")
XF_MESHES = ("big", "empty", "dark", "small")
XF_STORAGE = ("dark", "small", "big")
XF_MOVED = (5, 9)   # moved() changes instances [5, 9): big, dark, big, small
XF_CAMERA_FROM, XF_CAMERA_AT, XF_CAMERA_VFOV = (0.0, 25.0, 95.0), (0.0, 0.0, 0.0), 50.0


@functools.lru_cache(maxsize=None)
def _xf_meshes():
    big, mats = random_soup(XF_BIG["n_tri"], XF_BIG["n_sph"], XF_BIG["seed"], spread=XF_BIG["spread"],
                            n_mat=XF_BIG["n_mat"])
    for m, E in zip((4, 5), XF_E):
        mats[m]["type"], mats[m]["albedo"] = PT_EMISSIVE, E
        mats[m]["fuzz"] = mats[m]["ir"] = 0.0
    dark, _ = random_soup(XF_DARK["n_tri"], XF_DARK["n_sph"], XF_DARK["seed"], spread=XF_DARK["spread"],
                          n_mat=XF_DARK["n_mat"])
    small = np.zeros(5, orc.OBJECT_DTYPE)
    small["type"] = PT_TRIANGLE
    small["mat"] = (5, 0, 4, 3, 5)
    for k in range(5):
        small["v"][k] = (k - 2.0, 0.0, 0.1 * k, k - 1.2, 0.3, 0.0, k - 1.6, 1.0 + 0.1 * k, 0.4)
    return {"big": big, "dark": dark, "small": small, "empty": big[:0]}, mats


def _xf_matrices(seed):
    m = random_transforms(len(XF_INSTANCES), seed, reach=30.0)
    big = [i for i, p in enumerate(XF_INSTANCES) if p == "big"]
    for i, lamp in zip(big[1:4], ilr.lamp_transforms()[2:5]):   # the mirror, the stretch and the shear
        m[i].reshape(3, 4)[:, :3] = lamp.reshape(3, 4)[:, :3]
    return m


def instanced_transformed_scene(single=False):
    """(objects, mesh_first, mesh_count, instances, materials); single=True: one instance, the big mesh
    under the shear (instLightKernel's search with nInst == 1)."""
    parts, mats = _xf_meshes()
    objs = np.concatenate([parts[p] for p in XF_STORAGE])
    start, at = {"empty": 3}, 0
    for p in XF_STORAGE:
        start[p] = at
        at += len(parts[p])
    first = np.array([start[p] for p in XF_MESHES], np.int64)
    count = np.array([len(parts[p]) for p in XF_MESHES], np.int64)
    inst = np.zeros(len(XF_INSTANCES), INSTANCE_DTYPE)
    inst["m"] = _xf_matrices(3103)
    inst["mesh"] = [XF_MESHES.index(p) for p in XF_INSTANCES]
    if single:
        inst = inst[9:10].copy()
        assert XF_INSTANCES[9] == "big"
    return objs, first, count, inst, mats.copy()


def moved(instances):
    """The transformed scene's instances with the sub-range XF_MOVED moved: each turned further (by
    another angle about another axis) and drawn a fifth of the way towards the origin, so that no mesh
    reaches further than it did (the rebuild stays a top-level one)."""
    out = instances.copy()
    a, b = XF_MOVED
    for i in range(a, b):
        m = out["m"][i].reshape(3, 4).astype(np.float64)
        m[:, :3] = ilr._rot(i % 3, 20.0 + 15.0 * (i - a)) @ m[:, :3]
        m[:, 3] = 0.8 * m[:, 3] + (1.0, -0.5, 2.0)
        out["m"][i] = m.reshape(-1)
    return out


# ---------------------------------------------------------------- light lists at the tile and block edges
EDGE_PATTERNS = ("all", "none", "first_only", "last_only", "alternate", "tile_ends")
EDGE_E = ((17.0, 12.0, 4.0), (0.25, 8.0, 1.5))
TILE_ENDS = (SCAN_TILE - 1, SCAN_TILE, 2 * SCAN_TILE - 1, 2 * SCAN_TILE)


def edge_sphere_indices(n):
    """The objects of edge_list_scene(n, .) that are spheres (emissive material, never listed)."""
    return (2, n // 2 + 1, n - 3) if n >= 16 else ()


def edge_patterns(n):
    """The patterns that make sense at n."""
    return [p for p in EDGE_PATTERNS if (p != "alternate" or n >= 2) and (p != "tile_ends" or n >= SCAN_TILE)]


def edge_light_indices(n, pattern):
    """The object indices of the sampled lights, ascending."""
    sph = set(edge_sphere_indices(n))
    idx = {"all": range(n), "none": (), "first_only": (0,), "last_only": (n - 1,), "alternate": range(0, n, 2),
           "tile_ends": [i for i in TILE_ENDS if i < n]}[pattern]
    return [i for i in idx if i not in sph]


def edge_list_scene(n, pattern):
    """(objects, materials): n objects, small distinct triangles on a 64 x 64 x . lattice but for the
    spheres of edge_sphere_indices(n).  Material 0 is Lambertian, 1 and 2 are emissive with different
    E; the lights of `pattern` carry 1 and 2 in turn, the spheres 1, everything else 0."""
    assert pattern in EDGE_PATTERNS and n >= 1
    i = np.arange(n)
    c = np.stack([i % 64, (i // 64) % 64, i // 4096], 1).astype(F) * F(1.5)
    objs = np.zeros(n, orc.OBJECT_DTYPE)
    objs["type"] = PT_TRIANGLE
    objs["v"][:, 0:3] = c
    objs["v"][:, 3:6] = c + np.array([0.5, 0.0, 0.125], F) + (i % 7).astype(F)[:, None] * F(0.03125)
    objs["v"][:, 6:9] = c + np.array([0.0, 0.75, 0.25], F)
    lit = np.array(edge_light_indices(n, pattern), np.int64)
    objs["mat"][lit] = 1 + np.arange(len(lit)) % 2
    for s in edge_sphere_indices(n):
        objs["type"][s], objs["mat"][s] = PT_SPHERE, 1
        objs["v"][s, 3:] = 0.0
        objs["v"][s, 3] = 0.25
    mats = np.zeros(3, orc.MATERIAL_DTYPE)
    mats[0]["type"], mats[0]["albedo"] = PT_LAMBERTIAN, (0.6, 0.6, 0.6)
    for m, E in zip((1, 2), EDGE_E):
        mats[m]["type"], mats[m]["albedo"] = PT_EMISSIVE, E
    return objs, mats


# ---------------------------------------------------------------- growing and shrinking the list
def growth_steps():
    """flat_scene()'s objects under five material assignments, a walk of the light count through
    2, 905, 0, 838 and 5 (the geometry never changes): two of the soup's lights (slots 3 and 700) and the
    rest Lambertian; the soup; no emissive triangle; the emissive triangles Lambertian and the triangles
    of material 3 emissive (another 838 triangles); five lights -- the first, the last, and the ones on
    either side of the first scan tile's end and before the second's."""
    sc = flat_scene()
    base = sc.objects
    lit = np.flatnonzero(is_light(base, sc.materials))

    def only(keep):
        o = base.copy()
        o["mat"][np.setdiff1d(lit, keep)] = 0
        return o

    other = base.copy()
    other["mat"][(base["type"] == PT_TRIANGLE) & (base["mat"] == 3)] = 4
    other["mat"][lit] = 3
    per_tile = [int((lit < t).sum()) for t in (SCAN_TILE, 2 * SCAN_TILE)]
    ends = [0, per_tile[0] - 1, per_tile[0], per_tile[1] - 1, len(lit) - 1]
    return [only(lit[[3, 700]]), base.copy(), only(lit[:0]), other, only(lit[ends])]
