#!/usr/bin/env python3
"""What next-event estimation (PT_RENDER_NEE) and its MIS form (PT_RENDER_MIS) buy on the lit presets:
noise against time (GPU; a measurement, not a test).

For each scene, at a reduced frame, in sample mode with the default (wide) kernel:
  * the reference image: one long BLIND run (the integrator without the flag, not the code under
    test), film seed 1;
  * blind, NEE and MIS frames at a ladder of samples per pixel, film seed 2: RMSE of the linear image (the
    output squared) against the reference, over all pixels and channels, and the frame's kernel time
    (median of --repeat frames after a warm-up frame);
  * RMSE at equal time: the blind RMSE interpolated (log-log between the ladder's rungs, slope -1/2
    beyond its ends) at the NEE frame's time, and its ratio to the NEE RMSE; the same for MIS.
  * with --split SPP: one more frame each at SPP samples, and the split of its squared error into the
    0.2 % of the pixels with the largest error and the rest (where a bias sits: the clamp's, next to
    the lamp), with the means of the reference and of the frame over those pixels.
The reference's own noise (RMSE of a blind frame scales as spp^-1/2, so it is sqrt(spp / ref_spp) of a
rung's blind RMSE) is in every figure, and so is the clamp's bias in the NEE rows; neither is removed.

With --instanced the same ladder runs on the instanced form of each preset (pt_preset_instanced), built
with PT_BVH_LIGHTS: the instanced NEE / MIS kernels, reference and blind rungs instanced too.

usage: nee_noise.py [--scenes cornell_lit,bunny_cornell_lit] [--size 512] [--ref-spp 65536]
                    [--ladder 16,64,256,1024] [--repeat 3] [--split SPP] [--instanced] [--json FILE]
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
ap.add_argument("--split", type=int, default=0)
ap.add_argument("--instanced", action="store_true")
ap.add_argument("--json")
a = ap.parse_args()
ladder = [int(x) for x in a.ladder.split(",")]


MODES = {"blind": {}, "nee": {"nee": True}, "mis": {"mis": True}}


def frame(scene, p, seed, spp, mode, repeat):
    """(linear image float64, median kernel ms, rays) of `repeat` identical frames after a warm-up."""
    film = ptamd.Film(a.size, a.size, seed=seed)
    ms, rgb, st = [], None, None
    for _ in range(repeat + 1):   # (the first frame builds the wide tree and measures tile costs)
        rgb, st = ptamd.render(scene, film, p.camera, spp, p.max_depth, rng=ptamd.RNG_SAMPLE, **MODES[mode])
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


out = {"size": a.size, "ref_spp": a.ref_spp, "ladder": ladder, "instanced": a.instanced, "scenes": {}}
for name in a.scenes.split(","):
    if a.instanced:
        p = ptamd.InstancedPreset(name, a.size, a.size)
        scene = ptamd.Scene.instanced(p.objects, p.mesh_first, p.mesh_count, p.instances, p.materials,
                                      flags=ptamd.PT_BVH_LIGHTS)
    else:
        p = ptamd.Preset(name, a.size, a.size)
        scene = ptamd.Scene(p.objects, p.materials)
    scene.set_sky(*p.sky)
    ref, ref_ms, _ = frame(scene, p, 1, a.ref_spp, "blind", 0)
    rows = {m: [] for m in MODES}
    for mode in MODES:
        for spp in ladder:
            img, ms, rays = frame(scene, p, 2, spp, mode, a.repeat)
            rows[mode].append(
                {"spp": spp, "rmse": float(np.sqrt(((img - ref) ** 2).mean())), "ms": ms, "rays": rays,
                 "mean": float(img.mean())})
    for r in rows["nee"] + rows["mis"]:
        r["blind_rmse_at_equal_time"] = blind_rmse_at(r["ms"], rows["blind"])
        r["ratio"] = r["blind_rmse_at_equal_time"] / r["rmse"]
    out["scenes"][name] = {"lights": scene.n_lights, "max_depth": p.max_depth, "reference_ms": ref_ms,
                           "reference_mean": float(ref.mean()), **rows}
    print(f"\n{name}{' (instanced)' if a.instanced else ''}, {a.size} x {a.size}, depth {p.max_depth}, {scene.n_lights} sampled lights; reference: blind, "
          f"{a.ref_spp} spp ({ref_ms:.0f} ms), mean {ref.mean():.4f}\n")
    print("| spp | blind RMSE | blind ms | NEE RMSE | NEE ms | blind RMSE at the NEE frame's time | ratio "
          "| MIS RMSE | MIS ms | blind RMSE at the MIS frame's time | ratio |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for b, n, m in zip(rows["blind"], rows["nee"], rows["mis"]):
        print(f"| {b['spp']} | {b['rmse']:.4f} | {b['ms']:.3f} | {n['rmse']:.4f} | {n['ms']:.3f} | "
              f"{n['blind_rmse_at_equal_time']:.4f} | {n['ratio']:.2f} | {m['rmse']:.4f} | {m['ms']:.3f} | "
              f"{m['blind_rmse_at_equal_time']:.4f} | {m['ratio']:.2f} |")
    if a.split > 0:
        split = {}
        print(f"\nsquared error at {a.split} spp: the 0.2 % of the pixels with the largest error, and the rest\n")
        print("| | RMSE | share of the squared error in those pixels | reference mean there (R / G / B) | "
              "frame mean there | frame / reference | RMSE without them |")
        print("|---|---|---|---|---|---|---|")
        for mode in MODES:
            img, _, _ = frame(scene, p, 2, a.split, mode, 0)
            e2 = ((img - ref) ** 2).sum(axis=1)   # per pixel, over the channels
            top = np.argsort(e2)[-max(1, round(0.002 * len(e2))):]
            rest = np.setdiff1d(np.arange(len(e2)), top)
            rm, fm = ref[top].mean(0), img[top].mean(0)
            split[mode] = {"rmse": float(np.sqrt(e2.sum() / img.size)), "pixels": int(len(top)),
                           "share": float(e2[top].sum() / e2.sum()), "reference_mean": rm.tolist(),
                           "frame_mean": fm.tolist(), "rmse_rest": float(np.sqrt(e2[rest].sum() / (3 * len(rest))))}
            print(f"| {mode} | {split[mode]['rmse']:.4f} | {100 * split[mode]['share']:.0f} % of it in {len(top)} pixels | "
                  f"{rm[0]:.3f} / {rm[1]:.3f} / {rm[2]:.3f} | {fm[0]:.3f} / {fm[1]:.3f} / {fm[2]:.3f} | "
                  f"{fm.sum() / rm.sum():.3f} | {split[mode]['rmse_rest']:.4f} |")
        out["scenes"][name]["split"] = {"spp": a.split, **split}
if a.json:
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
