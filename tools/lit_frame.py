#!/usr/bin/env python3
"""One frame of a lit preset (an emissive lamp under the preset's own sky), timed: a record, no target.

usage: lit_frame.py [--scene bunny_cornell_lit] [--width 1920] [--height 1080] [--spp 256]
                    [--rng sample|compat] [--repeat 3] [--png FILE]
Prints one JSON line: scene, resolution, spp, depth, rng, the kernel ms of each repeat and their median.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "path-tracer-cuda-opengl_amd", "python"))
import ptamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="bunny_cornell_lit")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--spp", type=int, default=256)
ap.add_argument("--rng", choices=["sample", "compat"], default="sample")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--png")
a = ap.parse_args()

p = ptamd.Preset(a.scene, a.width, a.height)
scene = ptamd.Scene(p.objects, p.materials)
scene.set_sky(*p.sky)
film = ptamd.Film(a.width, a.height, seed=1)
rng = ptamd.RNG_SAMPLE if a.rng == "sample" else ptamd.RNG_COMPAT
ms, rgb, st = [], None, None
for _ in range(max(1, a.repeat) + 1):   # (the first frame builds the wide tree and measures tile costs)
    film.reset()
    rgb, st = ptamd.render(scene, film, p.camera, a.spp, p.max_depth, rng=rng)
    ms.append(st.kernel_ms)
ms = ms[1:]
if a.png:
    ptamd.write_png(a.png, rgb, a.width, a.height)
print(json.dumps({"scene": a.scene, "width": a.width, "height": a.height, "spp": a.spp, "max_depth": p.max_depth,
                  "rng": a.rng, "sky": [x.tolist() for x in p.sky], "kernel_ms": [round(x, 3) for x in ms],
                  "median_ms": round(statistics.median(ms), 3), "rays": int(st.rays),
                  "mean_rgb": [round(float(x), 4) for x in rgb.mean(0)]}))
