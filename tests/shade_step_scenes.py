"""Scenes of tests/test_gpu_shade_step.py and the recorder of tests/golden/shade_step.npz.

The wide kernels' SHADE step (pt_device.hip renderKernelWF) keeps its wave counters in scalar
registers, reads the shading record and the hit's exact box through 32-bit offsets, checks the range of
a ray's three reciprocals once per wave, seeds a path's stream with Philox's first two rounds written
out, and finishes a task with a 24-bit pixel index.  Each case puts
frames on one of those:

  edges        sparse_scene(65) at 43 x 37, 5 spp: tasks off both frame edges, a last block of one sample
  depth0/1     the same scene with max_depth 0 (no step loop) and 1 (every path ends at its first hit)
  bunny        the bunny in the Cornell box: 5,000 shading records and exact boxes
  wide_film    wall_box(1) on a 4,104 x 2 film at 1 spp, and
  tall_film    on a 2 x 4,104 one: column and row indices beyond 4,095
  slit*        wall_box(2) through cameras whose rays have one or two direction components of exactly
               0 (node_step_scenes.slit_camera): those lanes take the IEEE divisions, their wave mates
               on a bounce do not
  materials    wall_box(1) with a metal and a dielectric quad: waves hold mixed materials
  lamp0        that box with an emissive quad of radiance 0 under the ceiling (the LIT kernels; the
               oracle absorbs at an emitter, so a black one has a whole-frame oracle)
  lamp         the same with radiance (4, 3, 0.5): compared between the kernels
  cornell      the Cornell box: every material Lambertian

A case is (objects, materials, camera, width, height, spp, max_depth).  Run as a script on a GPU,

    python tests/shade_step_scenes.py tests/golden/shade_step.npz

it records, per case, the wide kernel's {node visits, primitive tests} of two successive compat
launches on one film (fixed waves: the same on the same tree), from a host-built and a device-built
tree, with whatever library ptamd loads (PT_LIB).  The committed file was recorded with the build
before item 17.
"""
import os
import sys

import numpy as np

from helpers import OBJECT_DTYPE
from node_step_scenes import CENTRE, DEPTH, SEED, SPP, H, W, slit_camera, sparse_scene
from wall_box import HI, LO, wall_box

BOX_FROM, BOX_AT, BOX_VFOV = (270.0, 280.0, 40.0), (200.0, 250.0, 500.0), 70.0
SLITS = {"slit_y": (1,), "slit_x": (0,), "slit_xy": (0, 1), "slit_yz": (1, 2)}
LAMP_RADIANCE = (4.0, 3.0, 0.5)


def material_box(pt, lamp=None):
    """wall_box(1) -- walls 0..5 of two triangles each, Lambertian -- with the wall x = HI metal and the
    wall y = LO a dielectric; lamp: the radiance of an emissive quad under the ceiling (None: no quad)."""
    objs, mats3 = wall_box(1)
    mats = np.zeros(6, mats3.dtype)
    mats[:3] = mats3
    mats[3] = (2, (0.8, 0.8, 0.6), 0.3, 0.0)    # metal, fuzzy
    mats[4] = (4, (1.0, 1.0, 1.0), 0.0, 1.5)    # dielectric
    mats[5] = (pt.PT_EMISSIVE, lamp if lamp is not None else (0.0, 0.0, 0.0), 0.0, 0.0)
    # (wall_box lists axis 0's planes LO, HI, then axis 1's, axis 2's: two triangles per plane)
    objs["mat"][2:4] = 3    # x = HI
    objs["mat"][4:6] = 4    # y = LO
    if lamp is not None:
        y = HI[1] - np.float32(20.0)
        x0, x1 = np.float32(180.0), np.float32(380.0)
        z0, z1 = np.float32(200.0), np.float32(360.0)
        quad = np.zeros(2, OBJECT_DTYPE)
        quad["type"] = 3
        quad["mat"] = 5
        quad["v"][0] = (x0, y, z0, x1, y, z0, x1, y, z1)
        quad["v"][1] = (x0, y, z0, x1, y, z1, x0, y, z1)
        objs = np.concatenate([objs, quad])
    assert (objs["v"].reshape(-1, 3, 3)[2:4, :, 0] == HI[0]).all() and (objs["v"].reshape(-1, 3, 3)[4:6, :, 1] == LO[1]).all()
    return objs, mats


def cases(pt):
    """name -> (objects, materials, camera, width, height, spp, max_depth)."""
    out = {}
    objs, mats, campar = sparse_scene(65)
    out["edges"] = (objs, mats, pt.camera_make(campar[0], campar[1], campar[2], 43 / 37), 43, 37, 5, DEPTH)
    for depth in (0, 1):
        out[f"depth{depth}"] = (objs, mats, pt.camera_make(*campar), W, H, SPP, depth)
    p = pt.Preset("bunny_cornell", W, H)
    out["bunny"] = (p.objects, p.materials, p.camera, W, H, SPP, DEPTH)
    objs, mats = wall_box(1)
    out["wide_film"] = (objs, mats, pt.camera_make(BOX_FROM, BOX_AT, 4.0, 4104 / 2), 4104, 2, 1, DEPTH)
    out["tall_film"] = (objs, mats, pt.camera_make(BOX_FROM, BOX_AT, 120.0, 2 / 4104), 2, 4104, 1, DEPTH)
    objs, mats = wall_box(2)
    for name, zero_axes in SLITS.items():
        axis = next(a for a in (2, 0, 1) if a not in zero_axes)
        origin = CENTRE.copy()
        if len(zero_axes) == 2:   # (one ray: off the splitting planes, where it would only meet the walls' shared edges)
            origin[list(zero_axes)] += np.array([7.25, 3.5], np.float32)
        out[name] = (objs, mats, slit_camera(pt, origin, axis, zero_axes), W, H, SPP, DEPTH)
    cam = pt.camera_make(BOX_FROM, BOX_AT, BOX_VFOV, W / H)
    out["materials"] = material_box(pt) + (cam, W, H, SPP, DEPTH)
    out["lamp0"] = material_box(pt, (0.0, 0.0, 0.0)) + (cam, W, H, SPP, DEPTH)
    out["lamp"] = material_box(pt, LAMP_RADIANCE) + (cam, W, H, SPP, DEPTH)
    p = pt.Preset("cornell", W, H)
    out["cornell"] = (p.objects, p.materials, p.camera, W, H, SPP, DEPTH)
    return out


def compat_launches(pt, gpu, scene, case, kernel):
    """Two compat launches on one film: [(rgb, stats, film states)] per launch."""
    _, _, cam, w, h, spp, depth = case
    f = pt.Film(w, h, SEED, device=gpu)
    out = []
    for _ in range(2):
        rgb, st = pt.render(scene, f, cam, spp, depth, kernel=kernel, rng=pt.RNG_COMPAT)
        out.append((rgb, st, f.get_rng()))
    return out


def scenes_of(pt, gpu, case):
    """The case's scene from a host-built and from a device-built wide tree."""
    objs, mats = case[0], case[1]
    host = pt.Scene(objs, mats, device=gpu)
    dev = pt.Scene(objs, mats, device=gpu, flags=pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_WIDE_DEVICE)
    return {"host": host, "device": dev}


def tree_sources(scenes):
    """(1, 2) once both scenes have rendered with the wide kernel: host-built, device-built."""
    return scenes["host"].wide_info()["source"], scenes["device"].wide_info()["source"]


def wide_work(launches):
    """[[node visits, primitive tests] per launch] of compat_launches(.., KERNEL_WIDE)."""
    return np.array([[st.node_visits, st.tri_tests + st.sphere_tests] for _, st, _ in launches], np.uint64)


def record(pt, gpu=0):
    out = {}
    for name, case in cases(pt).items():
        scenes = scenes_of(pt, gpu, case)
        for tree, s in scenes.items():
            out[f"{name}|{tree}"] = wide_work(compat_launches(pt, gpu, s, case, pt.KERNEL_WIDE))
        assert tree_sources(scenes) == (1, 2), name
    return out


if __name__ == "__main__":
    import torch  # noqa: F401  before libpt.so loads

    HERE = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(HERE), "path-tracer-cuda-opengl_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ptamd

    np.savez_compressed(sys.argv[1], **record(ptamd))
