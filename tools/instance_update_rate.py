"""Moving the instances of the C5 bunny field (pt_preset_instanced "bunny_field": the Cornell box and
210 bunnies): what a frame's rebuild costs after pt_scene_update_instances, what the rebuilt tree
costs to trace, and what laying a scene out for updates costs a scene that never moves (GPU only).

    python tools/instance_update_rate.py [share_of_bunnies_moved] [n_rays_millions] [frames]

Each frame moves the chosen share of the bunnies (default: all) by a small translation and a small
rotation about its own centre.
  rebuild   per frame, interleaved: Scene.update_instances + build_bvh (wall time, and the build's
            device time from pt_scene_build_time) beside the only way there was before -- a new
            Scene.instanced of the moved instances, created and built (wall time; build_ms alone
            is its build without the scene's creation).  Median and min..max over the frames after
            a warm-up frame.
  quality   the last frame's instances: camera rays and incoherent rays (random origins inside the
            world box, random directions) traced through the rebuilt scene and through a fresh
            host-built one, interleaved, best of 3 after a warm-up and the spread of the repeats:
            kernel ms and node visits per ray.
  reach     an unmoved scene built plain and built with PT_BVH_WIDE_DEVICE (mesh trees quantised
            for twice the reach, top level in its reserved region): frame time at the preset's
            frame, 4 spp, sample RNG, interleaved, median and min..max of 7 frames.
"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "path-tracer-cuda-opengl_amd", "python"))
import ptamd as pt  # noqa: E402

share = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
n = int(float(sys.argv[2]) * 1e6) if len(sys.argv) > 2 else 16_000_000
frames = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ip = pt.InstancedPreset("bunny_field")
rng = np.random.default_rng(1)
bunny = ip.objects[int(ip.mesh_first[1]):int(ip.mesh_first[1]) + int(ip.mesh_count[1])]
centre = bunny["v"][:, :9].reshape(-1, 3).astype(np.float64).mean(0)   # object space


def fresh(inst, flags=None):
    s = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, inst, ip.materials, build=False)
    s.build_bvh(*(() if flags is None else (flags,)))
    return s


def move(inst):
    """The chosen share of the bunnies: a rotation of up to 0.05 rad about the vertical through the
    bunny's own centre and a translation of up to 2 units, composed with its matrix."""
    out = inst.copy()
    ids = 1 + np.nonzero(rng.random(len(inst) - 1) < share)[0]
    for i in ids:
        m = np.vstack([inst["m"][i].astype(np.float64).reshape(3, 4), [0, 0, 0, 1]])
        a = rng.uniform(-0.05, 0.05)
        r = np.eye(4)
        r[0, 0], r[0, 2], r[2, 0], r[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
        r[:3, 3] = centre - r[:3, :3] @ centre
        t = np.eye(4)
        t[:3, 3] = rng.uniform(-2.0, 2.0, 3) * [1, 0, 1]
        out["m"][i] = (t @ m @ r)[:3].reshape(-1).astype(np.float32)
    return out, len(ids)


def stat(x):
    return f"median {np.median(x):8.3f}  min {min(x):8.3f}  max {max(x):8.3f}"


# ---------------------------------------------------------------- rebuild
scene = fresh(ip.instances)
inst = ip.instances
upd_wall, upd_dev, new_wall, new_build, sources = [], [], [], [], []
for f in range(frames + 1):
    inst, moved = move(inst)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scene.update_instances(inst)
    scene.build_bvh()
    t1 = time.perf_counter()
    other = fresh(inst)
    t2 = time.perf_counter()
    if f == 0:
        continue   # warm-up: the dynamic scene's first build is the full one, in the layout for updates
    upd_wall.append((t1 - t0) * 1e3)
    upd_dev.append(scene.build_ms)
    new_wall.append((t2 - t1) * 1e3)
    new_build.append(other.wide_info()["build_ms"])
    sources.append(scene.wide_info()["source"])
print(f"rebuild: {frames} frames, {moved} of {len(inst) - 1} bunnies moved per frame; ms")
print(f"  update_instances + build_bvh, wall     {stat(upd_wall)}   sources {sorted(set(sources))}")
print(f"  update_instances + build_bvh, device   {stat(upd_dev)}")
print(f"  new Scene.instanced + build_bvh, wall  {stat(new_wall)}")
print(f"  (of which its build_bvh)               {stat(new_build)}", flush=True)

# ---------------------------------------------------------------- quality
other = fresh(inst)
cam = pt.camera_to_array(ip.camera)
pos, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
u, v = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
camera = np.zeros(n, pt.RAY_DTYPE)
camera["o"] = pos
camera["d"] = ll + u[:, None] * hor + v[:, None] * ver - pos
t = inst["m"][:, [3, 7, 11]]
lo, hi = t.min(0) - 50.0, t.max(0) + 50.0
lo[1], hi[1] = 0.0, 300.0
inco = np.zeros(n, pt.RAY_DTYPE)
inco["o"] = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
d = rng.normal(size=(n, 3)).astype(np.float32)
inco["d"] = d / np.linalg.norm(d, axis=1, keepdims=True)
dev = torch.device("cuda", 0)
hits = torch.empty(n * pt.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
print(f"quality: {n} rays per set, best of 3 after a warm-up (spread of the repeats)")
for set_name, rays in (("camera", camera), ("incoherent", inco)):
    rd = torch.from_numpy(rays.view(np.uint8)).to(dev)
    runs = {"rebuilt": [], "fresh": []}
    keep = {}
    for rep in range(4):
        for name, s in (("rebuilt", scene), ("fresh", other)):
            st = s.trace_device(rd.data_ptr(), n, hits.data_ptr(), kernel=pt.KERNEL_WIDE)
            if rep:
                runs[name].append(st)
            elif name == "rebuilt":
                keep[name] = hits.clone()
            else:
                assert torch.equal(keep["rebuilt"], hits), "the rebuilt scene's hits differ from the fresh scene's"
    for name in ("rebuilt", "fresh"):
        ms = [s.kernel_ms for s in runs[name]]
        print(f"  {set_name:10s} {name:8s} {min(ms):8.3f} ms  spread {max(ms) - min(ms):6.3f}  "
              f"visits/ray {runs[name][0].node_visits / n:6.3f}", flush=True)
del hits

# ---------------------------------------------------------------- reach
w, h = ip.width, ip.height
plain, laid = fresh(ip.instances), fresh(ip.instances, pt.PT_BVH_WIDE_DEVICE)
films = {"plain": pt.Film(w, h, 1), "laid out": pt.Film(w, h, 1)}
ms = {"plain": [], "laid out": []}
img = {}
for rep in range(8):
    for name, s in (("plain", plain), ("laid out", laid)):
        rgb, st = pt.render(s, films[name], ip.camera, 4, ip.max_depth, kernel=pt.KERNEL_WIDE, rng=pt.RNG_SAMPLE)
        img[name] = rgb
        if rep:
            ms[name].append(st.kernel_ms)
assert np.array_equal(img["plain"], img["laid out"]), "the two layouts' frames differ"
print(f"reach: unmoved scene, {w}x{h}, 4 spp, kernel ms over 7 frames (the same frame bit for bit)")
for name in ("plain", "laid out"):
    print(f"  {name:9s} {stat(ms[name])}")
