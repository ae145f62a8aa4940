"""The light records of an instanced scene built with PT_BVH_LIGHTS, restated in float64 (a helper
module, not a test file), and the lamp scene the instanced NEE / MIS tests share.

include/pt.h states the rule next to PT_RENDER_NEE:

  lights   the (instance, object) pairs whose object is a triangle (type 3) with an emissive material
           (type 8), in flattened object order: instances in order, each contributing its mesh's
           emissive triangles in object order.  nL does not depend on the matrices.
  vertex   w_r = ((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3] with m, x, y, z converted to
           double, one rounded float64 operation each in that order; rounded to float32 once.
  record   v0', e1 = v1' - v0', e2 = v2' - v0' in float32, E = the material's albedo.

tests/test_instanced_lights_host.py holds this to pathloop_nee.light_list on identity matrices.
"""
import functools

import numpy as np

import oracle as orc
from helpers import INSTANCE_DTYPE

F = np.float32
PT_LAMBERTIAN, PT_TRIANGLE, PT_EMISSIVE = 1, 3, 8


def world_vertex(m, v):
    """m: float32 (12,) row-major 3 x 4; v: float32 (n, 3).  float32 (n, 3) by the rule above."""
    m = np.asarray(m, F).reshape(3, 4).astype(np.float64)
    x, y, z = (np.asarray(v, F)[:, a].astype(np.float64) for a in range(3))
    out = np.empty((len(x), 3), F)
    for r in range(3):
        out[:, r] = (((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]).astype(F)
    return out


def light_list(objects, mesh_first, mesh_count, instances, materials):
    """(v0, e1, e2, E), float32 (nL, 3) each, in list order."""
    objects = np.ascontiguousarray(objects, orc.OBJECT_DTYPE)
    materials = np.ascontiguousarray(materials, orc.MATERIAL_DTYPE)
    v0s, e1s, e2s, Es = [], [], [], []
    for inst in instances:
        first, count = int(mesh_first[inst["mesh"]]), int(mesh_count[inst["mesh"]])
        o = objects[first:first + count]
        o = o[(o["type"] == PT_TRIANGLE) & (materials["type"][o["mat"]] == PT_EMISSIVE)]
        v = o["v"].astype(F).reshape(-1, 9)
        w0, w1, w2 = (world_vertex(inst["m"], v[:, 3 * k:3 * k + 3]) for k in range(3))
        v0s.append(w0)
        e1s.append((w1 - w0).astype(F))
        e2s.append((w2 - w0).astype(F))
        Es.append(materials["albedo"][o["mat"]].astype(F).reshape(-1, 3))
    if not v0s:
        return tuple(np.zeros((0, 3), F) for _ in range(4))
    return tuple(np.concatenate(x) for x in (v0s, e1s, e2s, Es))


def records(lights):
    """The (nL, 4, 3) layout of Scene.lights() / pt_scene_download_lights."""
    return np.stack([np.asarray(x, F) for x in lights], axis=1)


# ---------------------------------------------------------------- the lamp scene
# One emissive quad (two triangles, E = (17, 12, 4), the lit presets' lamp) centred at (0, 5, 0) in its
# object space, placed five times: by the identity, a rotation times a uniform scale, a mirror
# (det < 0), a non-uniform stretch and a shear, with translations of order 10; a Lambertian floor of
# 80 x 80 (identity) and one Lambertian occluder quad under the first lamp (a translation).  Seen from
# above one corner so that every lamp and its pool of light on the floor is in the frame.
LAMP_E = (17.0, 12.0, 4.0)
LAMP_CAMERA_FROM, LAMP_CAMERA_AT, LAMP_CAMERA_VFOV = (4.0, 22.0, 34.0), (0.0, 1.0, 0.0), 50.0
IDENT = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def _quad(y, h, mat):
    o = np.zeros(2, orc.OBJECT_DTYPE)
    o["type"], o["mat"] = PT_TRIANGLE, mat
    o["v"][0] = (-h, y, -h, -h, y, h, h, y, h)
    o["v"][1] = (-h, y, -h, h, y, h, h, y, -h)
    return o


def _rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def lamp_transforms():
    """float32 (5, 12): the five lamp placements."""
    lin = [np.eye(3),
           1.5 * (_rot(1, 20.0) @ _rot(2, 30.0)),               # rotation x uniform scale
           _rot(0, -25.0) @ np.diag([-1.0, 1.0, 1.0]),          # a mirror: det < 0
           np.diag([2.0, 1.0, 0.5]),                            # a non-uniform stretch
           np.array([[1.0, 0.4, 0.0], [0.0, 1.0, 0.0], [0.3, 0.0, 1.0]])]   # a shear
    tr = [(0.0, 0.0, 0.0), (12.0, 1.0, -9.0), (-11.0, 0.5, 8.0), (-10.0, 1.0, -12.0), (9.0, -0.5, 10.0)]
    return np.array([np.concatenate([a, np.array(t).reshape(3, 1)], 1).reshape(-1) for a, t in zip(lin, tr)], F)


@functools.lru_cache(maxsize=None)
def lamp_scene():
    """(objects, mesh_first, mesh_count, instances, materials):
    meshes 0 = lamp, 1 = floor, 2 = occluder; instances 0-4 the lamps, 5 the floor, 6 the occluder."""
    mats = np.zeros(2, orc.MATERIAL_DTYPE)
    mats[0]["type"], mats[0]["albedo"] = PT_LAMBERTIAN, (0.7, 0.7, 0.7)
    mats[1]["type"], mats[1]["albedo"] = PT_EMISSIVE, LAMP_E
    objs = np.concatenate([_quad(5.0, 2.0, 1), _quad(0.0, 40.0, 0), _quad(0.0, 1.5, 0)])
    inst = np.zeros(7, INSTANCE_DTYPE)
    inst["mesh"] = (0, 0, 0, 0, 0, 1, 2)
    inst["m"][:5] = lamp_transforms()
    inst["m"][5:] = IDENT
    inst["m"][6, 7] = 2.5   # the occluder, halfway between the floor and the first lamp
    return objs, np.array([0, 2, 4], np.int64), np.array([2, 2, 2], np.int64), inst, mats


def moved_instances(inst):
    """The lamp scene's instances with two lamps moved: lamp 1 turned further about its own
    translation, lamp 3 translated."""
    inst = inst.copy()
    a = inst["m"][1].reshape(3, 4).astype(np.float64)
    a[:, :3] = _rot(1, 35.0) @ a[:, :3]
    inst["m"][1] = a.reshape(-1)
    inst["m"][3, 3] += 3.0
    inst["m"][3, 11] += 5.0
    return inst
