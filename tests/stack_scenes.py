"""Small lit scenes with deep trees, and their pinned references (a helper module, not a test file):
the inputs of tests/test_gpu_render_stacks.py, whose conditions tests/test_stack_scenes_host.py checks.

Every traversal kernel is compiled once per traversal-stack size and the host picks the copy from the
tree's depth (pt_device.hip: wideStackFor -- 8, 16, 24 entries for the wide depth; stackFor -- 16, 24,
32, 48, 64, 80 for the binary depth + 1).  The lit test scenes of tests/pathloop*.py all have wide
trees of depth <= 8 and binary trees of depth <= 15 (test_stack_scenes_host.py prints them: cornell_lit
2 / 8, N2 3 / 8, clamp, rim and open 1 / 2, the many-lights soup 5 / 15); these select the deeper copies,
and the lighting rules have teeth on them.

Scenes (depths found on the CPU: the host wide builder through tools/micro/wide_tree_check, and the
oracle's bvh_depth; on the GPU the device wide builder reports the host builder's depths on all four):

  name  what                                            objects  wide depth / stack  instanced (+3)  kernels
  T16   two facing chains of 100 triangles (1.15)         200       12 / 16           15 / 16      wide TRI; instanced
  S16   the same and 14 spheres                           214       11 / 16           14 / 16      wide generic; instanced
  T24   two facing chains of 200 triangles (1.15)         400       19 / 24           22 / 24      wide TRI; instanced
  S24   the same and 28 spheres                           428       19 / 24           22 / 24      wide generic; instanced
                                                                 binary depth / stack
  B24   test_gpu_query_stacks.soup_with_copies + stage   2062       21 / 24                        simple, wavefront
  B32   helpers.deep_stack_scene(2) + stage                58       26 / 32                        simple, wavefront
  B48   helpers.deep_stack_scene(256) + stage             312       34 / 48                        simple, wavefront
        (sample mode at 48: 32 entries in LDS, the rest in the global spill buffer)

The chains: triangle k of chain A at x = 1.15^k (tri_kernel_scenes.geometric, lowered to z = -0.03 x with
its third vertex at z = 0), chain B lifted to z = 0.3 x with its third vertex at z = 0.4 x, so the two
face each other at every scale and no two triangles share a plane (chains(): exact ties); the spheres
sit between them (glass, metal, Lambertian in turn).  Five triangles of the small end emit
(A 4, 9; B 2, 6, 11: all at x < 5 -- a light 10^12 away adds 0 by overflow, legal but toothless); the
rest are Lambertian; the sky is the soups' own.  The camera sits just before the small end, above chain
A, and looks along the chains (within the wide kernels' near-origin rule: the scene's extent is 10^6 and
more).  From the apex itself both chains are edge-on, and tri_kernel_scenes' camera sees chain A from
behind, where no surface sees a light: cameras at x in {0.8, 1.5, 2.5}, y in {0.1, 0.3}, z in {0.3, 0.5,
0.8} looking along (1, dy, dz), dy in {0, 0.1}, dz in {-0.1, 0.05, 0.15}, at 20, 30 and 45 degrees were
tried with the restatement (NEE, compat); the one chosen is the best of those that see the chains from
before their small end, where the trees are deepest.
stage(): around the camera point of a binary scene, a Lambertian floor and wall, two emissive triangles
and a Lambertian blocker between the upper lamp and the floor.  In B32 and B48 the camera point lies
inside every sphere, so every ray crosses every level of the tree.

The frames: 16 x 12; compat 3 spp, sample mode 5 spp in blocks of 2; max depth 8; film seed 21.  What
the rules do on them (the restatement's events; light terms and weighted emitter hits all > 0; none
clamps) -- compat / sample:

  scene      rays lit -> NEE   unoccluded  occluded  back-facing  scatter rays on a light  after specular
  T16, T24   879 -> 1137          119        129         65              17                     0
             1452 -> 1837         169        210        119              28                     0
  S16, S24   989 -> 1281          118        146         65              19                     3
             1612 -> 2008         157        229        110              29                     9     (glass 71 / 96 scatters, metal 41 / 70)
  B24        2873 -> 3735         325        574        263              21                    32
             4623 -> 6023         539        893        439              51                    50     (glass 654 / 1050, metal 517 / 838)
  B32, B48   4105 -> 7487        2300       1053        205              94                     0
             6899 -> 12535       3818       1782        375             152                     0

(T24 is T16 with larger triangles behind everything the camera's paths reach, so their paths agree; the
trees, and with them the kernels, differ.  Likewise S24 / S16 and B48 / B32.)
"""
import contextlib
import functools

import numpy as np

import oracle as orc
import pathloop
import pathloop_mis as pm
from helpers import MATERIAL_DTYPE, OBJECT_DTYPE, deep_stack_scene, random_soup
from pathloop import DEFAULT_SKY, PT_EMISSIVE, SEED

W, H = 16, 12
SPP, DEPTH = 3, 8                 # compat launches
SAMPLE_SPP, SAMPLE_CHUNK = 5, 2   # sample mode: a short last block
LONG_DEPTH, LONG_SPP = 20, 2      # the two-launch compat case (the wide kernels' critical pixels need depth > 16)
SKY = ((0.2, 0.1, 0.3), (0.9, 0.8, 0.1))
RADIANCE = (6.0, 5.0, 2.0)
RATIO = 1.15

WIDE = {"T16": (16, 100, False), "S16": (16, 100, True), "T24": (24, 200, False), "S24": (24, 200, True)}
BINARY = {"B24": 24, "B32": 32, "B48": 48}
MODES = {"blind": (False, False), "lit": (False, False), "nee": (True, False), "mis": (False, True)}


def bin_stack(depth):   # (stackFor)
    return next(s for s in (16, 24, 32, 48, 64, 80) if depth + 1 <= s)


def wide_stack(depth):   # (wideStackFor)
    return next(s for s in (8, 16, 24) if depth <= s)


def wide_interval(stack):
    """The wide depths that select `stack` entries."""
    return {8: (0, 8), 16: (9, 16), 24: (17, 24)}[stack]


def bin_interval(stack):
    """The binary depths that select `stack` entries."""
    return {16: (0, 15), 24: (16, 23), 32: (24, 31), 48: (32, 47)}[stack]


# ---------------------------------------------------------------- materials
LAMBERT = ((0.8, 0.3, 0.2), (0.2, 0.7, 0.3), (0.3, 0.4, 0.9))
M_LIGHT, M_GLASS, M_METAL = 3, 4, 5


def materials():
    mats = np.zeros(6, MATERIAL_DTYPE)
    mats["type"] = (1, 1, 1, PT_EMISSIVE, 4, 2)
    mats["albedo"][:3] = LAMBERT
    mats["albedo"][M_LIGHT] = RADIANCE
    mats["albedo"][M_GLASS] = 1.0
    mats["ir"][M_GLASS] = 1.5
    mats["albedo"][M_METAL] = (0.8, 0.8, 0.7)
    mats["fuzz"][M_METAL] = 0.2
    return mats


def blind_materials(mats):
    """The same materials with every emitter turned into a grey Lambertian: nothing emits, and under
    the default sky the blind (non-LIT) kernels render the scene -- and the oracle knows all of it."""
    out = mats.copy()
    em = out["type"] == PT_EMISSIVE
    out["type"][em] = 1
    out["albedo"][em] = 0.5
    return out


# ---------------------------------------------------------------- the wide scenes: two facing chains
LIGHTS_A, LIGHTS_B = (4, 9), (2, 6, 11)   # the emissive triangles of either chain: the small end
CHAIN_CAMERA = ((0.8, 0.1, 0.5), (1.8, 0.1, 0.4), 20.0)


def chains(n, spheres, ratio=RATIO):
    """Two chains of n triangles in geometric progression, x = ratio^k: chain A as
    tri_kernel_scenes.geometric but lowered to z = -0.03 x with its third vertex at z = 0, chain B lifted
    to z = 0.3 x with its third vertex at z = 0.4 x, so the two face each other at every scale (a coplanar
    chain sees no light: cs <= 0).  Within a chain the triangles overlap in x but lie in parallel planes
    of their own -- never in one plane, where a ray through two of them would find both at exactly the
    same t, a tie that flat scenes decide in the reference's order and instanced ones by (instance,
    primitive) (include/pt.h): the identity-instanced frames would not be the flat ones.
    with `spheres`, one small sphere per seven triangles between them, at x = 1.1 ratio^(3 + 7i),
    y = 0.1 x, z = 0.15 x, r = 0.05 x -- glass, metal and Lambertian in turn."""
    x = (ratio ** np.arange(n, dtype=np.float64)).astype(np.float32)
    a = np.zeros(n, OBJECT_DTYPE)
    a["type"] = 3
    a["v"][:, 0] = a["v"][:, 3] = a["v"][:, 6] = x
    a["v"][:, 3] += 0.25 * x
    a["v"][:, 7] = 0.25 * x
    a["mat"] = np.arange(n) % 3
    b = a.copy()
    a["v"][:, 2] = a["v"][:, 5] = -0.03 * x
    b["v"][:, 2] = b["v"][:, 5] = 0.3 * x
    b["v"][:, 8] = 0.4 * x
    b["mat"] = (np.arange(n) + 1) % 3
    a["mat"][list(LIGHTS_A)] = M_LIGHT
    b["mat"][list(LIGHTS_B)] = M_LIGHT
    parts = [a, b]
    if spheres:
        m = n // 7
        xs = (1.1 * ratio ** (3.0 + 7.0 * np.arange(m, dtype=np.float64)))
        s = np.zeros(m, OBJECT_DTYPE)
        s["type"] = 1
        s["v"][:, 0], s["v"][:, 1], s["v"][:, 2], s["v"][:, 3] = xs, 0.1 * xs, 0.15 * xs, 0.05 * xs
        s["mat"] = np.array([M_GLASS, M_METAL, 0])[np.arange(m) % 3]
        parts.append(s)
    return np.concatenate(parts)


# ---------------------------------------------------------------- the binary scenes
def _tri(v, mat):
    t = np.zeros(1, OBJECT_DTYPE)
    t["type"] = 3
    t["mat"] = mat
    t["v"][0] = np.asarray(v, np.float32).reshape(9)
    return t


def stage(c, s, first_mat):
    """A handful of triangles around the point c, of size s: a Lambertian floor (two triangles) below
    it, a Lambertian wall in front (-z), an emissive triangle above and one beside, and a Lambertian
    blocker between the upper lamp and the floor.  Materials first_mat + {0, 1: Lambertian, 2: emissive}."""
    cx, cy, cz = c
    lam0, lam1, light = first_mat, first_mat + 1, first_mat + 2
    return np.concatenate([
        _tri([(cx - 2 * s, cy - s, cz - 3 * s), (cx - 2 * s, cy - s, cz + s), (cx + 2 * s, cy - s, cz + s)], lam0),
        _tri([(cx - 2 * s, cy - s, cz - 3 * s), (cx + 2 * s, cy - s, cz + s), (cx + 2 * s, cy - s, cz - 3 * s)], lam0),
        _tri([(cx - 2 * s, cy - s, cz - 3 * s), (cx + 2 * s, cy - s, cz - 3 * s), (cx, cy + 2 * s, cz - 3 * s)], lam1),
        _tri([(cx - s, cy + 1.5 * s, cz - 2.5 * s), (cx + s, cy + 1.5 * s, cz - 2.5 * s), (cx, cy + 1.5 * s, cz - 0.5 * s)], light),
        _tri([(cx + 1.8 * s, cy - 0.8 * s, cz - 2.5 * s), (cx + 1.8 * s, cy - 0.8 * s, cz - 1.0 * s),
              (cx + 1.8 * s, cy + 0.6 * s, cz - 1.8 * s)], light),
        _tri([(cx - 0.6 * s, cy + 0.5 * s, cz - 2.2 * s), (cx + 0.6 * s, cy + 0.5 * s, cz - 2.2 * s),
              (cx, cy + 0.5 * s, cz - 1.0 * s)], lam1),
    ])


def stage_materials(mats):
    extra = np.zeros(3, MATERIAL_DTYPE)
    extra["type"] = (1, 1, PT_EMISSIVE)
    extra["albedo"] = ((0.7, 0.7, 0.6), (0.3, 0.5, 0.8), RADIANCE)
    return np.concatenate([mats, extra])


def stage_camera(c, s):
    cx, cy, cz = c
    return ((cx, cy, cz), (cx, cy - 0.5 * s, cz - 3 * s), 70.0)


BINARY_STAGE = {"B24": ((0.0, 0.0, 7.0), 1.5), "B32": ((1024.0, 1024.0, 1024.0), 150.0),
                "B48": ((1024.0, 1024.0, 1024.0), 150.0)}


def binary_objects(name):
    """test_gpu_query_stacks.py's scenes of the binary sizes, with stage() around the camera point."""
    if name == "B24":   # (soup_with_copies)
        objs, mats = random_soup(1500, 300, seed=3)
        objs = np.concatenate([objs, np.repeat(objs[:1], 256)])
    else:
        objs, mats = deep_stack_scene({"B32": 2, "B48": 256}[name])
    c, s = BINARY_STAGE[name]
    return np.concatenate([objs, stage(c, s, len(mats))]), stage_materials(mats)


# ---------------------------------------------------------------- scenes and references
class StackScene(pathloop.LitScene):
    def __init__(self, name, objects, mats, campar, stack):
        cam = orc.camera_make(campar[0], campar[1], campar[2], W / H)
        super().__init__(name, objects, mats, cam, W, H, SPP, DEPTH, SKY)
        self.stack = stack                              # the traversal-stack size the scene is meant to select
        self.blind_materials = blind_materials(mats)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in WIDE:
        stack, n, spheres = WIDE[name]
        return StackScene(name, chains(n, spheres), materials(), CHAIN_CAMERA, stack)
    objs, mats = binary_objects(name)
    c, s = BINARY_STAGE[name]
    return StackScene(name, objs, mats, stage_camera(c, s), BINARY[name])


@contextlib.contextmanager
def _counting_scatter(counts):
    """pathloop_mis._path's scatter call, counted per material type (which materials the frame's paths
    went through: the restatement's results do not say)."""
    inner = pm._scatter

    def counted(ctx, mat, ray, hit, state):
        counts[int(mat["type"])] = counts.get(int(mat["type"]), 0) + 1
        return inner(ctx, mat, ray, hit, state)

    pm._scatter = counted
    try:
        yield
    finally:
        pm._scatter = inner


@functools.lru_cache(maxsize=None)
def reference(name, mode, rng, max_depth=DEPTH, frames=1, rows=None, spp=None):
    """The restatement's frames of a scene: a list of `frames` results (compat: each continues the
    streams of the one before; sample: one result, the film's streams untouched).  mode: 'lit' (no
    flag), 'nee', 'mis', or 'blind' (the emitters Lambertian, the default sky: no LIT kernel).  Each
    result also has "scattered": {material type: scatter calls}.  Computed once per set of arguments,
    shared, read-only."""
    sc = scene(name)
    nee, mis = MODES[mode]
    mats, sky = (sc.blind_materials, DEFAULT_SKY) if mode == "blind" else (sc.materials, sc.sky)
    rows = tuple(range(H)) if rows is None else rows
    counts = {}
    with _counting_scatter(counts):
        if rng == "sample":
            assert frames == 1
            out = [pm.render_sample(sc.objects, mats, sc.nodes, sc.camera, W, H, rows, SAMPLE_SPP if spp is None else spp,
                                    max_depth, SEED, SAMPLE_CHUNK, sky=sky, nee=nee, mis=mis)]
        else:
            assert rng == "compat"
            states = orc.film_states(SEED, W, rows)
            out = []
            for _ in range(frames):
                r = pm.render(sc.objects, mats, sc.nodes, sc.camera, W, H, rows, SPP if spp is None else spp, max_depth,
                              states, sky=sky, nee=nee, mis=mis)
                states = r["states"]
                out.append(r)
    out[-1]["scattered"] = counts
    return out
