"""A closed axis-aligned box of flat walls (shared by test_wide_deferred_rule.py and
test_gpu_deferred_leafbox.py).

Every wall is a g x g grid of quads (two triangles each) in a plane x, y or z = const, so every
triangle's exact box is flat on one axis.  A ray started on one wall that hits another has a hit
distance t and a box entry lo that are the same quantity computed two ways: they differ by a
rounding, and t < lo (a grazing hit) for about half of the hits.  With every wall doubled, each
grazing hit has an exact twin inside its window [t, lo): the query is order-dependent.
"""
import numpy as np

from helpers import MATERIAL_DTYPE, OBJECT_DTYPE

LO = np.array([-3.3, 0.7, 1.9], np.float32)
HI = np.array([551.7, 548.3, 559.1], np.float32)


def wall_box(g: int = 3, doubled: bool = False):
    tris = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        us = np.linspace(LO[u], HI[u], g + 1).astype(np.float32)
        vs = np.linspace(LO[v], HI[v], g + 1).astype(np.float32)
        for plane in (LO[axis], HI[axis]):
            for i in range(g):
                for j in range(g):
                    c = np.zeros((4, 3), np.float32)
                    c[:, axis] = plane
                    c[:, u] = (us[i], us[i + 1], us[i + 1], us[i])
                    c[:, v] = (vs[j], vs[j], vs[j + 1], vs[j + 1])
                    tris += [c[[0, 1, 2]].ravel(), c[[0, 2, 3]].ravel()]
    objs = np.zeros(len(tris), OBJECT_DTYPE)
    objs["type"] = 3
    objs["v"] = np.array(tris, np.float32)
    objs["mat"] = np.arange(len(objs)) % 3
    if doubled:
        twin = objs.copy()
        twin["mat"] = (objs["mat"] + 1) % 3   # (the copies differ: the kept one shows in a frame)
        objs = np.concatenate([objs, twin])
        objs = objs[np.random.default_rng(7).permutation(len(objs))]
    mats = np.zeros(3, MATERIAL_DTYPE)
    mats["type"] = 1   # Lambertian: every path bounces from wall to wall until its depth ends
    mats["albedo"] = [(0.8, 0.3, 0.2), (0.2, 0.7, 0.3), (0.3, 0.4, 0.9)]
    return objs, mats


def wall_rays(n: int, seed: int):
    """Rays from points on the walls (exactly in the wall's plane) toward points on other walls."""
    rng = np.random.default_rng(seed)

    def on_wall(m):
        p = (LO + (HI - LO) * rng.uniform(0.02, 0.98, (m, 3))).astype(np.float32)
        axis = rng.integers(0, 3, m)
        p[np.arange(m), axis] = np.where(rng.integers(0, 2, m) == 0, LO[axis], HI[axis])
        return p

    o, tgt = on_wall(n), on_wall(n)
    rays = np.zeros((n, 6), np.float32)
    rays[:, :3] = o
    rays[:, 3:] = (tgt - o) * rng.uniform(0.3, 3.0, (n, 1)).astype(np.float32)   # unnormalised
    return rays
