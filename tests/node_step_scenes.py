"""Small scenes for the wide NODE step (shared by test_gpu_node_step.py and, run as a script, the
recorder of tests/golden/node_step_instanced.npz).

wideHits (pt_device.hip) decides per node which planes are near and which are far (the signs of
1 / d), scales the plane bytes by 2^(exponent byte) per axis and assembles the children's hit bits by
slot and ray octant.  Each scene puts rays on one of those:

  octants      wall_box(g=1): a closed box of 12 triangles seen from its centre by two opposite
               cameras whose first rays cover all eight sign combinations (checked in numpy)
  slits        wall_box(g=2) seen from its centre through cameras whose viewport is collapsed onto a
               line or a point: every camera ray has one or two direction components of exactly 0,
               and the origin lies exactly in the plane that splits the walls (a node plane)
  scaled       cornell times 2^-20 and 2^20 about the origin (small and large exponent bytes, the
               reference-order fallback of rays whose |1 / d| is beyond the MIX planes' limit), a box
               whose extents differ by 2^16 between axes, and cornell seen from 20 extents away
               (the far-origin fallback)
  sparse       1, 2, 3, 9 and 65 triangles: a root that is a leaf, nodes with empty slots, leaves of
               1-3 primitives
  doubled      wall_box(doubled=True): order-dependent queries, repeated in the reference's order
  instanced    cornell's meshes under a mirrored and a sheared instance
"""
import numpy as np

from helpers import MATERIAL_DTYPE, OBJECT_DTYPE
from wall_box import HI, LO, wall_box

W, H = 48, 40
SPP, DEPTH, SEED, CHUNK = 4, 50, 11, 2
# (the coordinate at which wall_box(2) splits its walls, per axis)
CENTRE = np.array([np.linspace(LO[a], HI[a], 3).astype(np.float32)[1] for a in range(3)], np.float32)


def scaled_camera(pt, cam, s):
    """The camera of a scene scaled by s (a power of two: every product is exact)."""
    c = pt.Camera.from_buffer_copy(bytes(cam))
    for f in ("origin", "lower_left", "horizontal", "vertical"):
        v = getattr(c, f)
        for i in range(3):
            v[i] = float(np.float32(v[i]) * np.float32(s))
    c.focus_dist = float(np.float32(c.focus_dist) * np.float32(s))
    c.lens_radius = float(np.float32(c.lens_radius) * np.float32(s))
    return c


def slit_camera(pt, origin, axis, zero_axes):
    """A camera at `origin` looking along `axis` whose viewport has no extent along `zero_axes`:
    every camera ray's direction is exactly 0 there."""
    c = pt.camera_make(origin, np.asarray(origin, np.float32) + np.eye(3, dtype=np.float32)[axis], 90.0, 1.0)
    for a in zero_axes:
        c.horizontal[a] = 0.0
        c.vertical[a] = 0.0
        c.lower_left[a] = c.origin[a]
    return c


def octant_cameras(pt):
    d = np.array([1.0, 0.7, 0.4], np.float32)
    return [pt.camera_make(CENTRE, CENTRE + sgn * d, 140.0, W / H) for sgn in (1.0, -1.0)]


def first_ray_octants(orc, pt, cam):
    """The set of sign combinations (1/d < 0 per axis, as PT_BEGIN_RAY's oct) of the first camera rays."""
    from leaf_edge_scenes import first_camera_rays
    _, d = first_camera_rays(orc, pt.camera_to_array(cam), seed=SEED, w=W, h=H)
    with np.errstate(divide="ignore"):
        inv = np.float32(1.0) / d
    return set(((inv[:, 0] < 0) * 1 + (inv[:, 1] < 0) * 2 + (inv[:, 2] < 0) * 4).tolist())


def scale_objects(objs, s):
    out = objs.copy()
    out["v"] = (objs["v"] * np.asarray(s, np.float32)).astype(np.float32)
    return out


def anisotropic_box():
    """wall_box(g=2) with x times 2^8 and y times 2^-8: extents that differ by 2^16."""
    objs, mats = wall_box(2)
    s = np.tile(np.array([256.0, 1.0 / 256.0, 1.0], np.float32), 3)
    return scale_objects(objs, s), mats, (CENTRE * s[:3]).astype(np.float32)


def sparse_scene(n):
    """n triangles: a wall behind, and small ones scattered in front of it."""
    rng = np.random.default_rng(100 + n)
    tris = [((-6.0, -6.0, 6.0), (6.0, -6.0, 6.0), (0.0, 7.0, 6.0))]
    for _ in range(n - 1):
        c = rng.uniform((-3.0, -3.0, 0.5), (3.0, 3.0, 5.0))
        tris.append(tuple(tuple(c + rng.uniform(-0.8, 0.8, 3)) for _ in range(3)))
    objs = np.zeros(n, OBJECT_DTYPE)
    objs["type"] = 3
    objs["v"] = np.array(tris, np.float32).reshape(n, 9)
    objs["mat"] = np.arange(n) % 3
    mats = np.zeros(3, MATERIAL_DTYPE)
    mats["type"] = 1
    mats["albedo"] = [(0.8, 0.3, 0.2), (0.2, 0.7, 0.3), (0.3, 0.4, 0.9)]
    return objs, mats, ((0.3, 0.2, -4.0), (0.0, 0.0, 6.0), 60.0, W / H)


def instanced_case(pt):
    """The instanced cornell preset with its first instance mirrored in x about the box's middle and
    its last one sheared: (objects, mesh_first, mesh_count, instances, materials, camera, depth)."""
    ip = pt.InstancedPreset("cornell", W, H)
    inst = ip.instances.copy()
    m = inst["m"].reshape(-1, 3, 4).astype(np.float64)
    lo = np.array([np.inf] * 3)
    hi = -lo
    for k, i in enumerate(inst):
        f, c = int(ip.mesh_first[i["mesh"]]), int(ip.mesh_count[i["mesh"]])
        v = ip.objects["v"][f:f + c].astype(np.float64).reshape(-1, 3) @ m[k, :, :3].T + m[k, :, 3]
        lo, hi = np.minimum(lo, v.min(0)), np.maximum(hi, v.max(0))
    mid = (lo[0] + hi[0]) / 2
    mirror = np.diag([-1.0, 1.0, 1.0])
    m[0, :, :3] = mirror @ m[0, :, :3]
    m[0, :, 3] = mirror @ m[0, :, 3] + np.array([2 * mid, 0.0, 0.0])
    shear = np.eye(3)
    shear[0, 1] = 0.25
    shear[2, 1] = -0.125
    m[-1, :, :3] = shear @ m[-1, :, :3]
    inst["m"] = m.reshape(-1, 12).astype(np.float32)
    assert np.linalg.det(m[0, :, :3]) < 0
    return ip.objects, ip.mesh_first, ip.mesh_count, inst, ip.materials, ip.camera, DEPTH


def render_instanced(pt, gpu, scene, cam, rng):
    f = pt.Film(W, H, SEED, device=gpu)
    rgb, st = pt.render(scene, f, cam, SPP, DEPTH, kernel=pt.KERNEL_WIDE, rng=rng, chunk=CHUNK if rng == pt.RNG_SAMPLE else 0)
    return rgb, st, f.get_rng()


def record_instanced(pt, gpu=0):
    """What tests/golden/node_step_instanced.npz holds: the instanced case's frames, ray and path
    counts and film states in both RNG modes."""
    objs, first, count, inst, mats, cam, _ = instanced_case(pt)
    s = pt.Scene.instanced(objs, first, count, inst, mats, device=gpu)
    out = {}
    for name, rng in (("sample", pt.RNG_SAMPLE), ("compat", pt.RNG_COMPAT)):
        rgb, st, states = render_instanced(pt, gpu, s, cam, rng)
        out[name + "_rgb"] = np.ascontiguousarray(rgb).view(np.uint32)
        out[name + "_counts"] = np.array([st.rays, st.paths], np.uint64)
        out[name + "_states"] = states
    return out


if __name__ == "__main__":   # python tests/node_step_scenes.py out.npz  (on a GPU, with the library to record)
    import sys

    import torch  # noqa: F401  before libpt.so loads

    import ptamd
    np.savez_compressed(sys.argv[1], **record_instanced(ptamd))
