#!/usr/bin/env python3
"""What next-event estimation (PT_RENDER_NEE) buys on the lit presets: noise against time (GPU; a
measurement, not a test).

For each scene, at a reduced frame, in sample mode with the default (wide) kernel:
  * the reference image: one long BLIND run (the integrator without the flag, not the code under
    test), film seed 1;
  * blind and NEE frames at a ladder of samples per pixel, film seed 2: RMSE of the linear image (the
    output squared) against the reference, over all pixels and channels, and the frame's kernel time
    (median of --repeat frames after a warm-up frame);
  * RMSE at equal time: the blind RMSE interpolated (log-log between the ladder's rungs, slope -1/2
    beyond its ends) at the NEE frame's time, and its ratio to the NEE RMSE.
The reference's own noise (RMSE of a blind frame scales as spp^-1/2, so it is sqrt(spp / ref_spp) of a
rung's blind RMSE) is in every figure, and so is the clamp's bias in the NEE rows; neither is removed.

usage: nee_noise.py [--scenes cornell_lit,bunny_cornell_lit] [--size 512] [--ref-spp 65536]
                    [--ladder 16,64,256,1024] [--repeat 3] [--json FILE]
(Smaller frames or rungs are not throughput-bound: a 256 x 256 frame at 4 spp is one launch's overhead.)
Prints a Markdown table per scene and, with --json, writes every figure.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "path-tracer-cuda-opengl_amd", "python"))
import ptamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", default="cornell_lit,bunny_cornell_lit")
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--ref-spp", type=int, default=65536)
ap.add_argument("--ladder", default="16,64,256,1024")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--json")
a = ap.parse_args()
ladder = [int(x) for x in a.ladder.split(",")]


def frame(scene, p, seed, spp, nee, repeat):
    """(linear image float64, median kernel ms, rays) of `repeat` identical frames after a warm-up."""
    film = ptamd.Film(a.size, a.size, seed=seed)
    ms, rgb, st = [], None, None
    for _ in range(repeat + 1):   # (the first frame builds the wide tree and measures tile costs)
        rgb, st = ptamd.render(scene, film, p.camera, spp, p.max_depth, rng=ptamd.RNG_SAMPLE, nee=nee)
        ms.append(st.kernel_ms)
    return rgb.astype(np.float64) ** 2, statistics.median(ms[1:] or ms), int(st.rays)


def blind_rmse_at(t, rungs):
    """The blind ladder's RMSE at time t: log-log interpolation, slope -1/2 beyond the ends."""
    ts = [r["ms"] for r in rungs]
    es = [r["rmse"] for r in rungs]
    if t <= ts[0]:
        return es[0] * math.sqrt(ts[0] / t)
    if t >= ts[-1]:
        return es[-1] * math.sqrt(ts[-1] / t)
    for i in range(len(ts) - 1):
        if ts[i] <= t <= ts[i + 1]:
            w = (math.log(t) - math.log(ts[i])) / (math.log(ts[i + 1]) - math.log(ts[i]))
            return math.exp((1 - w) * math.log(es[i]) + w * math.log(es[i + 1]))
    raise AssertionError


out = {"size": a.size, "ref_spp": a.ref_spp, "ladder": ladder, "scenes": {}}
for name in a.scenes.split(","):
    p = ptamd.Preset(name, a.size, a.size)
    scene = ptamd.Scene(p.objects, p.materials)
    scene.set_sky(*p.sky)
    ref, ref_ms, _ = frame(scene, p, 1, a.ref_spp, False, 0)
    rows = {"blind": [], "nee": []}
    for nee in (False, True):
        for spp in ladder:
            img, ms, rays = frame(scene, p, 2, spp, nee, a.repeat)
            rows["nee" if nee else "blind"].append(
                {"spp": spp, "rmse": float(np.sqrt(((img - ref) ** 2).mean())), "ms": ms, "rays": rays,
                 "mean": float(img.mean())})
    for r in rows["nee"]:
        r["blind_rmse_at_equal_time"] = blind_rmse_at(r["ms"], rows["blind"])
        r["ratio"] = r["blind_rmse_at_equal_time"] / r["rmse"]
    out["scenes"][name] = {"lights": scene.n_lights, "max_depth": p.max_depth, "reference_ms": ref_ms,
                           "reference_mean": float(ref.mean()), **rows}
    print(f"\n{name}, {a.size} x {a.size}, depth {p.max_depth}, {scene.n_lights} sampled lights; reference: blind, "
          f"{a.ref_spp} spp ({ref_ms:.0f} ms), mean {ref.mean():.4f}\n")
    print("| spp | blind RMSE | blind ms | NEE RMSE | NEE ms | blind RMSE at the NEE frame's time | ratio |")
    print("|---|---|---|---|---|---|---|")
    for b, n in zip(rows["blind"], rows["nee"]):
        print(f"| {b['spp']} | {b['rmse']:.4f} | {b['ms']:.3f} | {n['rmse']:.4f} | {n['ms']:.3f} | "
              f"{n['blind_rmse_at_equal_time']:.4f} | {n['ratio']:.2f} |")
if a.json:
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
