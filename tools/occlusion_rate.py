"""Occlusion-query throughput of pt_trace_occluded_device beside the closest-hit query of the same
batch (pt_trace_closest_device, same process; GPU only): C3 scene, trace_rate.py's two ray sets --
camera rays, and incoherent rays (random origins inside the Cornell box, random directions) -- plus
shadow rays: from the incoherent set's closest-hit points toward random points of the light quad
(models/cornellbox/light.obj), each with its own tmax just short of the light.

    python tools/occlusion_rate.py [n_rays_millions]

Per set and tree: kernel_ms (best of REPEATS after a warm-up; the closest-hit line also gives the
spread of its repeats, the margin for comparing the two), Mray/s, node visits and primitive tests per
ray, and the fraction of rays that hit / are occluded.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "path-tracer-cuda-opengl_amd", "python"))
import ptamd as pt  # noqa: E402

REPEATS = 3
n = int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 16_000_000
p = pt.Preset("bunny_cornell")
scene = pt.Scene(p.objects, p.materials)
rng = np.random.default_rng(1)
cam = pt.camera_to_array(p.camera)   # origin (pos), lower-left, horizontal, vertical
pos, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
u, v = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
camera = np.zeros(n, pt.RAY_DTYPE)
camera["o"] = pos
camera["d"] = ll + u[:, None] * hor + v[:, None] * ver - pos
inco = np.zeros(n, pt.RAY_DTYPE)
lo, hi = p.objects["v"][:, :3].min(0), p.objects["v"][:, :3].max(0)
inco["o"] = rng.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), (n, 3)).astype(np.float32)
d = rng.normal(size=(n, 3)).astype(np.float32)
inco["d"] = d / np.linalg.norm(d, axis=1, keepdims=True)

dev = torch.device("cuda", 0)
hits = torch.empty(n * pt.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
occ = torch.empty(n, dtype=torch.uint8, device=dev)


def shadow_rays():
    """Origins: the incoherent set's closest-hit points (rays that miss keep their origin);
    directions: to a random point of the light quad, unnormalised, so the light is at t = 1;
    ray_tmax = 1 - 1e-3.  tmin = 0.001 of that segment keeps the ray off its own surface."""
    rd = torch.from_numpy(inco.view(np.uint8)).to(dev)
    scene.trace_device(rd.data_ptr(), n, hits.data_ptr(), kernel=pt.KERNEL_WIDE)
    h = hits.cpu().numpy().view(pt.HIT_DTYPE)
    light = pt.load_obj(os.path.join(pt.MODELS_DIR, "cornellbox", "light.obj"))["v"].reshape(-1, 3, 3)
    tri = light[rng.integers(0, len(light), n)]
    b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(np.float32)
    target = (b[:, :, None] * tri).sum(1)
    rays = np.zeros(n, pt.RAY_DTYPE)
    rays["o"] = np.where((h["hit"] == 1)[:, None], h["p"], inco["o"])
    rays["d"] = target - rays["o"]
    return rays, np.full(n, 1.0 - 1e-3, np.float32)


def best_of(call):
    call()   # warm-up (and, at first use, the wide tree's build)
    runs = [call() for _ in range(REPEATS)]
    ms = [s.kernel_ms for s in runs]
    return min(runs, key=lambda s: s.kernel_ms), max(ms) - min(ms)


def line(set_name, what, st, spread, frac):
    prims = (st.tri_tests + st.sphere_tests) / n
    extra = f"  spread {spread:6.3f} ms" if spread is not None else ""
    print(f"{set_name:10s} {what:17s} {st.kernel_ms:8.3f} ms  {n / st.kernel_ms / 1e3:9.0f} Mray/s  "
          f"visits/ray {st.node_visits / n:5.2f}  prims/ray {prims:5.2f}  {frac:.3f}{extra}", flush=True)


print(f"{n} rays per set, best of {REPEATS} after a warm-up; last column: fraction hit / occluded")
for set_name, make in (("camera", lambda: (camera, None)), ("incoherent", lambda: (inco, None)), ("shadow", shadow_rays)):
    rays, rt = make()
    rd = torch.from_numpy(rays.view(np.uint8)).to(dev)
    td = torch.from_numpy(rt).to(dev) if rt is not None else None
    # the closest-hit query takes one tmax per batch: the shadow set's common 1 - 1e-3
    tmax = float(rt[0]) if rt is not None else float("inf")
    for kname, k in (("wide", pt.KERNEL_WIDE), ("binary", pt.KERNEL_WAVEFRONT)):
        c, spread = best_of(lambda: scene.trace_device(rd.data_ptr(), n, hits.data_ptr(), 0.001, tmax, kernel=k))
        nhit = int(hits.view(torch.int32).view(n, -1)[:, 0].sum().item())
        a, aspread = best_of(lambda: scene.occluded_device(rd.data_ptr(), n, occ.data_ptr(), 0.001, tmax,
                                                           ray_tmax_ptr=td.data_ptr() if td is not None else None,
                                                           kernel=k))
        nocc = int(occ.sum(dtype=torch.int64).item())
        line(set_name, kname + " closest", c, spread, nhit / n)
        line(set_name, kname + " occluded", a, aspread, nocc / n)
        assert nocc == nhit, (nocc, nhit)   # the contract, on the whole batch
