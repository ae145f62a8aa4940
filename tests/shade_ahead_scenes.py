"""Cases and the recorder of tests/test_gpu_shade_ahead.py.

On a triangle-only flat scene without a metal or dielectric material, seen through a pinhole camera and
rendered in sample mode without light sampling, the wide kernel's AHEAD instantiations (pt_device.hip
renderKernelWF<.., AHEAD>) draw a path's scatter vectors one bounce ahead: the SHADE step's one trial
loop runs as long as the lanes that scatter now and hold no vector, and every other lane on a path draws
along into a one-entry LDS slot.  PT_SHADE_AHEAD=0 launches the kernels without the slot on the same
scene.  The knob is read when a launch is enqueued, so each setting is recorded by a process of its own:

    PT_SHADE_AHEAD=<0|1> PT_KERNEL_LOG=1 python tests/shade_ahead_scenes.py out.npz

renders every case below in sample mode and stores, per case and launch, the frame's bits and {rays,
paths}; on stderr a line `[case] <name>` precedes each case's launches, so the library's PT_KERNEL_LOG
lines (one per launch, naming the instantiation) can be told apart by case.

Eligible (the log must name an AHEAD kernel under knob 1 and its twin under knob 0):
  d<depth>s<spp>      the all-Lambertian Cornell box on a 43 x 37 film at 5 and 37 spp (37: blocks of 16, 16
                      and 5), max_depth 1, 2, 8 and 50 -- at depths 1 and 2 every path that scatters ends
                      as the pseudo-miss of a scatter out of bounces
  tiny                a 5 x 3 film: fewer tasks than lanes
  wide_film           a 4,104 x 2 film at 1 spp
  part0, part1        a 43 x 37 film in two stripe partitions
  seed1, seedF        seeds 1 and 0xFFFFFFFF, a 3-spp launch and an accumulating 5-spp launch after it
  bunny               the bunny in the Cornell box: 5,000 records, 64 x 40 at 8 spp, depth 50
  lit                 cornell_lit under its black sky (pathloop.lit_scene("L1"): 24 x 24, depth 8): the LIT
                      instantiation and the emissive exit, against the Python restatement of the render loop
                      (tests/pathloop.py; oracle/ absorbs at an emitter)
  lamp0               cornell_lit with radiance 0 under the reference's sky: LIT, and the oracle's frame
  chain16             a chain of 200 triangles whose wide tree takes the 16-entry stack
                      (tri_kernel_scenes.geometric; every scene of tests/stack_scenes.py holds a metal
                      and a dielectric material, so none of them qualifies)
  cornell@device, bunny@device   trees built on the device
Fallbacks (the log must name the same kernel, without AHEAD, under both knob values):
  metal, glass        a box with one metal / one dielectric wall
  lens                the Cornell box through a lens of radius 20
  nee                 the same cornell_lit scene with PT_RENDER_NEE, against tests/pathloop_nee.py
  instanced           cornell as its instanced preset, one identity instance: the flat scene's frame bit for
                      bit (tests/test_gpu_step_masks.py), so it is held to d50s5's oracle frame
"""
import os
import sys

import numpy as np

from tri_kernel_scenes import geometric
from wall_box import wall_box

DEPTH, CHUNK = 50, 2
W, H = 43, 37
COUNTERS = ("rays", "paths")
BOX_CAMERA = ((270.0, 280.0, 40.0), (200.0, 250.0, 500.0), 70.0)


def one_wall(mat_row):
    """wall_box(1) with the wall x = HI given the material `mat_row` (the others stay Lambertian)."""
    objs, mats3 = wall_box(1)
    mats = np.zeros(4, mats3.dtype)
    mats[:3] = mats3
    mats[3] = mat_row
    objs["mat"][2:4] = 3
    return objs, mats


def cases(pt):
    """name -> dict(objs, mats, cam, w, h, depth, seed, launches [(spp, chunk, accumulate)], and optionally
    sky, parts (n_parts, part), device (tree built on the device), nee, instanced)."""
    import pathloop   # (needs oracle/ on the path: the tests' conftest, or this file run as a script)

    out = {}
    box = pt.Preset("cornell", W, H)

    def case(objs, mats, cam, w=W, h=H, spp=5, chunk=CHUNK, depth=DEPTH, seed=11, launches=None, **kw):
        return dict(objs=objs, mats=mats, cam=cam, w=w, h=h, depth=depth, seed=seed,
                    launches=launches or [(spp, chunk, False)], **kw)

    for depth in (1, 2, 8, 50):
        for spp, chunk in ((5, CHUNK), (37, 16)):
            out[f"d{depth}s{spp}"] = case(box.objects, box.materials, box.camera, spp=spp, chunk=chunk, depth=depth)
    out["tiny"] = case(box.objects, box.materials, pt.Preset("cornell", 5, 3).camera, w=5, h=3)
    c = pt.camera_to_array(box.camera)
    frm, front = c[0:3], c[18:21]
    out["wide_film"] = case(box.objects, box.materials, pt.camera_make(frm, frm - front, 4.0, 4104 / 2), w=4104, h=2, spp=1)
    for part in (0, 1):
        out[f"part{part}"] = case(box.objects, box.materials, box.camera, parts=(2, part))
    for name, seed in (("seed1", 1), ("seedF", 0xFFFFFFFF)):
        out[name] = case(box.objects, box.materials, box.camera, seed=seed, launches=[(3, CHUNK, True), (5, CHUNK, True)])
    bunny = pt.Preset("bunny_cornell", 64, 40)
    out["bunny"] = case(bunny.objects, bunny.materials, bunny.camera, w=64, h=40, spp=8)
    lit = pt.Preset("cornell_lit", W, H)
    l1 = pathloop.lit_scene("L1")   # (its sample-mode references: 5 spp in blocks of 2, pathloop.SEED)
    l1cam = pt.Camera.from_buffer_copy(l1.camera.tobytes())
    l1case = dict(w=l1.width, h=l1.height, spp=5, chunk=2, depth=l1.max_depth, seed=pathloop.SEED, sky=l1.sky)
    out["lit"] = case(l1.objects, l1.materials, l1cam, **l1case)
    dark = lit.materials.copy()
    dark["albedo"][dark["type"] == pt.PT_EMISSIVE] = 0.0
    out["lamp0"] = case(lit.objects, dark, lit.camera)
    objs, mats, campar = geometric(200, 1.15)
    out["chain16"] = case(objs, mats, pt.camera_make(campar[0], campar[1], campar[2], W / H))
    out["cornell@device"] = case(box.objects, box.materials, box.camera, device=True)
    out["bunny@device"] = case(bunny.objects, bunny.materials, bunny.camera, w=64, h=40, spp=8, device=True)
    # fallbacks
    cam = pt.camera_make(*BOX_CAMERA, W / H)
    out["metal"] = case(*one_wall((2, (0.8, 0.8, 0.6), 0.3, 0.0)), cam)
    out["glass"] = case(*one_wall((4, (1.0, 1.0, 1.0), 0.0, 1.5)), cam)
    out["lens"] = case(box.objects, box.materials, pt.camera_make(frm, frm - front, 40.0, W / H, 40.0, 800.0), depth=12)
    out["nee"] = case(l1.objects, l1.materials, l1cam, nee=True, **l1case)
    out["instanced"] = case(None, None, None, instanced=True)   # (the camera, film and sampling of d50s5)
    return out


ELIGIBLE = ([f"d{d}s{s}" for d in (1, 2, 8, 50) for s in (5, 37)] +
            ["tiny", "wide_film", "part0", "part1", "seed1", "seedF", "bunny", "lit", "lamp0", "chain16", "cornell@device",
             "bunny@device"])
FALLBACKS = ["metal", "glass", "lens", "nee", "instanced"]
# the instantiation's <stack, .., LIT, NEE, ..> the eligible cases must launch (LIT: an emitter or a sky of the scene's own)
STACK_LIT = {name: (8, name in ("lit", "lamp0")) for name in ELIGIBLE}
STACK_LIT["chain16"] = (16, False)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _launches(pt, out, key, scene, case, kernel, gpu):
    parts = case.get("parts", (1, 0))
    f = pt.Film(case["w"], case["h"], case["seed"], device=gpu, n_parts=parts[0], part=parts[1])
    for k, (spp, chunk, accumulate) in enumerate(case["launches"]):
        rgb, st = pt.render(scene, f, case["cam"], spp, case["depth"], kernel=kernel, rng=pt.RNG_SAMPLE, chunk=chunk,
                            accumulate=accumulate, nee=case.get("nee", False))
        out[f"{key}|{k}|rgb"] = _bits(rgb)
        out[f"{key}|{k}|n"] = np.array([getattr(st, c) for c in COUNTERS], np.uint64)


def _mark(name):
    sys.stderr.flush()
    sys.stderr.write(f"[case] {name}\n")
    sys.stderr.flush()


def record(pt, gpu=0):
    out = {}
    for name, case in cases(pt).items():
        if case.get("instanced"):
            ip = pt.InstancedPreset("cornell", W, H)
            s = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, ip.instances, ip.materials, device=gpu)
            case = dict(case, cam=ip.camera)
        else:
            flags = pt.PT_BVH_ORIGIN_BOUNDS | (pt.PT_BVH_WIDE_DEVICE if case.get("device") else 0)
            s = pt.Scene(case["objs"], case["mats"], device=gpu, flags=flags)
            if "sky" in case:
                s.set_sky(*case["sky"])
        _mark(name)
        _launches(pt, out, name, s, case, pt.KERNEL_WIDE, gpu)
        if not case.get("instanced"):
            out[f"{name}|tree"] = np.array([s.wide_info()["source"], s.wide_info()["depth"]])
    _mark("end")
    return out


if __name__ == "__main__":
    import torch  # noqa: F401  before libpt.so loads

    HERE = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(HERE), "path-tracer-cuda-opengl_amd", "python"),
              os.path.join(os.path.dirname(HERE), "oracle"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ptamd

    np.savez(sys.argv[1], **record(ptamd))
