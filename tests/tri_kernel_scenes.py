"""Scenes and the recorder of tests/test_gpu_tri_kernels.py.

A triangle-only, non-instanced scene is rendered by the wide kernels' TRI instantiations
(pt_device.hip renderKernelWF<.., TRI>), in which the scene's hasSpheres flag is a compile-time 0;
PT_WIDE_TRI=0 launches the generic kernels on the same scene.  The knob is read when a launch is
enqueued, so each setting is recorded by a process of its own:

    PT_WIDE_TRI=<0|1> python tests/tri_kernel_scenes.py out.npz

renders every case below at 48 x 40, 4 spp, depth 50 and stores, per case and variant, the frame's
bits, the film's RNG states and the counters {rays, paths, node visits, triangle tests, sphere tests}.
Variants: sample mode, and two successive compat launches on one film (the second launch has
critical pixels, whose waves run the per-lane loop PT_CRIT_TRACE).

  tri1, tri2, tri3, tri65   node_step_scenes.sparse_scene: a root that is a leaf, leaves of 1-3 primitives
  box, doubled              wall_box(1), closed; wall_box(1, doubled): order-dependent queries, redone
                            through SHADE's deferred rule
  stack16, stack24          chains of 200 / 300 triangles in geometric progression: wide trees of depth
                            12 and 18 (tests/test_gpu_query_stacks.py), the 16- and 24-entry kernels
  *@device, *@rebuilt       the same scene's tree built on the device, and built again on the host after that
  lit                       cornell_lit with its sky: the LIT kernels, and with nee / mis the NEE / MIS ones
  shadow                    a wall and eight small triangles in front of it
  hidden_sphere             `shadow` plus a sphere behind the wall that no ray reaches: hasSpheres, the generic kernel
  was_sphere                that scene with the sphere overwritten by a triangle: hasSpheres is sticky
  instanced                 cornell's meshes as instances: the instanced kernels know no TRI
"""
import os
import sys

import numpy as np

from helpers import MATERIAL_DTYPE, OBJECT_DTYPE
from node_step_scenes import CHUNK, DEPTH, H, SEED, SPP, W, sparse_scene
from wall_box import wall_box

COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "sphere_tests")
BOX_CAMERA = ((270.0, 280.0, 40.0), (200.0, 250.0, 500.0), 70.0, W / H)
TREES = ("tri3", "tri65", "box", "doubled")   # the cases also rendered from device-built and rebuilt trees


def geometric(n, ratio):
    """Triangle k at x = ratio^k with edges ratio^k / 4 (test_gpu_query_stacks.py: the SAH builder
    peels the largest off at every split, so the wide tree is a chain)."""
    objs = np.zeros(n, OBJECT_DTYPE)
    objs["type"] = 3
    x = (ratio ** np.arange(n, dtype=np.float64)).astype(np.float32)
    objs["v"][:, 0] = objs["v"][:, 3] = objs["v"][:, 6] = x
    objs["v"][:, 3] += 0.25 * x
    objs["v"][:, 7] = 0.25 * x
    objs["mat"] = np.arange(n) % 3
    mats = np.zeros(3, MATERIAL_DTYPE)
    mats["type"] = 1
    mats["albedo"] = [(0.8, 0.3, 0.2), (0.2, 0.7, 0.3), (0.3, 0.4, 0.9)]
    # the camera looks at the chain's small end, where the tree is deepest
    return objs, mats, ((8.0, 1.0, -10.0), (8.0, 1.0, 0.0), 90.0, W / H)


def shadow_scene():
    """A wall (one triangle in the plane z = 6) seen from z = -4, and eight small triangles in front of
    it whose projections along z lie well inside the wall's, like the camera's: a segment from any of
    them to a point behind the wall's middle crosses the wall (its projection is convex), so nothing
    that lies there is ever reached -- camera rays and bounces alike hit the wall first."""
    rng = np.random.default_rng(5)
    tris = [((-6.0, -6.0, 6.0), (6.0, -6.0, 6.0), (0.0, 7.0, 6.0))]
    for _ in range(8):
        c = rng.uniform((-1.5, -4.0, 1.0), (1.5, -1.0, 5.0))
        tris.append(tuple(tuple(c + rng.uniform(-0.8, 0.8, 3)) for _ in range(3)))
    objs = np.zeros(len(tris), OBJECT_DTYPE)
    objs["type"] = 3
    objs["v"] = np.array(tris, np.float32).reshape(len(tris), 9)
    objs["mat"] = np.arange(len(tris)) % 3
    mats = np.zeros(3, MATERIAL_DTYPE)
    mats["type"] = 1
    mats["albedo"] = [(0.8, 0.3, 0.2), (0.2, 0.7, 0.3), (0.3, 0.4, 0.9)]
    return objs, mats, ((0.3, -1.8, -4.0), (0.0, -2.0, 6.0), 60.0, W / H)


def hidden_sphere_scene():
    """`shadow` and, appended, a sphere behind the wall's middle, where no ray gets."""
    objs, mats, _ = shadow_scene()
    sph = np.zeros(1, OBJECT_DTYPE)
    sph["type"] = 1
    sph["v"][0, :4] = (0.0, -2.0, 9.0, 1.0)
    return np.concatenate([objs, sph]), mats


def replacement_triangle():
    """What overwrites the sphere in `was_sphere`: a triangle in its place, as unreachable."""
    t = np.zeros(1, OBJECT_DTYPE)
    t["type"] = 3
    t["v"][0] = (-1.0, -2.5, 9.0, 1.0, -2.5, 9.0, 0.0, -1.0, 9.5)
    return t


def flat_cases():
    """name -> (objects, materials, camera parameters): the triangle-only scenes."""
    out = {f"tri{n}": sparse_scene(n) for n in (1, 2, 3, 65)}
    out["box"] = wall_box(1) + (BOX_CAMERA,)
    out["doubled"] = wall_box(1, doubled=True) + (BOX_CAMERA,)
    out["stack16"] = geometric(200, 1.15)
    out["stack24"] = geometric(300, 1.1)
    out["shadow"] = shadow_scene()
    return out


def was_sphere_objects():
    objs, mats = hidden_sphere_scene()
    objs = objs.copy()
    objs[-1:] = replacement_triangle()
    return objs, mats


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _counters(st):
    return np.array([getattr(st, k) for k in COUNTERS], np.uint64)


def record_scene(pt, out, name, s, cam, kernel, gpu=0, **flags):
    """Sample mode, then two compat launches on one film; stored under name|sample, name|compat1, name|compat2."""
    f = pt.Film(W, H, SEED, device=gpu)
    rgb, st = pt.render(s, f, cam, SPP, DEPTH, kernel=kernel, rng=pt.RNG_SAMPLE, chunk=CHUNK, **flags)
    out[f"{name}|sample|rgb"], out[f"{name}|sample|n"], out[f"{name}|sample|rng"] = _bits(rgb), _counters(st), f.get_rng()
    f = pt.Film(W, H, SEED, device=gpu)
    for launch in (1, 2):
        rgb, st = pt.render(s, f, cam, SPP, DEPTH, kernel=kernel, rng=pt.RNG_COMPAT, **flags)
        k = f"{name}|compat{launch}"
        out[k + "|rgb"], out[k + "|n"], out[k + "|rng"] = _bits(rgb), _counters(st), f.get_rng()


def record(pt, gpu=0):
    out = {}
    host, dev = pt.PT_BVH_ORIGIN_BOUNDS, pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_WIDE_DEVICE
    for name, (objs, mats, campar) in flat_cases().items():
        cam = pt.camera_make(*campar)
        s = pt.Scene(objs, mats, device=gpu)
        record_scene(pt, out, name, s, cam, pt.KERNEL_WIDE)
        out[f"{name}|tree"] = np.array([s.wide_info()["source"], s.wide_info()["depth"]])
        record_scene(pt, out, name + "/wavefront", s, cam, pt.KERNEL_WAVEFRONT)
        if name in TREES:
            d = pt.Scene(objs, mats, device=gpu, flags=dev)
            record_scene(pt, out, name + "@device", d, cam, pt.KERNEL_WIDE)
            out[f"{name}@device|tree"] = np.array([d.wide_info()["source"], d.wide_info()["depth"]])
            d.build_bvh(host)
            record_scene(pt, out, name + "@rebuilt", d, cam, pt.KERNEL_WIDE)
            out[f"{name}@rebuilt|tree"] = np.array([d.wide_info()["source"], d.wide_info()["depth"]])
    # the LIT kernels, and with the flags the NEE / MIS ones
    p = pt.Preset("cornell_lit", W, H)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    s.set_sky(*p.sky)
    out["lit|lights"] = np.array([s.n_lights])
    for name, flags in (("lit", {}), ("lit/nee", {"nee": True}), ("lit/mis", {"mis": True})):
        record_scene(pt, out, name, s, p.camera, pt.KERNEL_WIDE, **flags)
    # dispatch: a sphere anywhere in the scene, now or before an update, keeps the generic kernels
    cam = pt.camera_make(*shadow_scene()[2])
    objs, mats = hidden_sphere_scene()
    s = pt.Scene(objs, mats, device=gpu)
    record_scene(pt, out, "hidden_sphere", s, cam, pt.KERNEL_WIDE)
    s.update_objects(replacement_triangle(), first=len(objs) - 1)
    s.build_bvh(host)
    record_scene(pt, out, "was_sphere", s, cam, pt.KERNEL_WIDE)
    ip = pt.InstancedPreset("cornell", W, H)
    s = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, ip.instances, ip.materials, device=gpu)
    record_scene(pt, out, "instanced", s, ip.camera, pt.KERNEL_WIDE)
    return out


if __name__ == "__main__":
    import torch  # noqa: F401  before libpt.so loads

    HERE = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(HERE), "path-tracer-cuda-opengl_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ptamd

    np.savez(sys.argv[1], **record(ptamd))
