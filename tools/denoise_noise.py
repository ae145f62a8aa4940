#!/usr/bin/env python3
"""What the first-hit AOVs and the guided a-trous filter (pt_render_aov, pt_film_denoise) buy on
low-spp frames of the lit presets, and what they cost (GPU; a measurement, not a test).

For each scene and frame size, in sample mode with the default (wide) kernel and PT_RENDER_MIS:
  * the reference image: one long MIS run, film seed 1;
  * at each rung of the ladder (film seed 2): the frame's kernel time (median of --repeat frames after a
    warm-up frame), the AOV pass's kernel_ms, the device time of the denoise passes (events around the
    enqueued call, median of --repeat), and the RMSE of the noisy and of the denoised frame against the
    reference, in the sqrt(mean) domain pt_render writes, over all pixels and channels;
    sigma_color = 1.2 / sqrt(spp), 5 passes, the binding's defaults otherwise;
  * RMSE at equal time: the noisy RMSE interpolated (log-log between the ladder's rungs, slope -1/2
    beyond its ends) at the rung's total time frame + AOV + denoise, and its ratio to the denoised RMSE
    (> 1: denoising N spp beats spending the same time on more samples).
The reference's own noise is in every figure and is not removed.

usage: denoise_noise.py [--scenes cornell_lit,bunny_cornell_lit] [--sizes 512x512,1920x1080]
                        [--ref-spp 4096] [--ladder 1,4,16,64] [--repeat 3] [--json FILE]
Prints a Markdown table per scene and size and, with --json, writes every figure.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch  # before libpt.so loads: one HIP runtime per process

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "path-tracer-cuda-opengl_amd", "python"))
import ptamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", default="cornell_lit,bunny_cornell_lit")
ap.add_argument("--sizes", default="512x512,1920x1080")
ap.add_argument("--ref-spp", type=int, default=4096)
ap.add_argument("--ladder", default="1,4,16,64")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--json")
a = ap.parse_args()
ladder = [int(x) for x in a.ladder.split(",")]
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev)


def rmse(x, ref):
    return float(np.sqrt(np.mean((x.astype(np.float64) - ref) ** 2)))


def host(t, dtype, cols):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype).reshape(-1, cols)


def interp(times, errs, t):
    """errs at time t: log-log between rungs, slope -1/2 beyond the ends."""
    lt, le, x = [math.log(v) for v in times], [math.log(v) for v in errs], math.log(t)
    if x <= lt[0]:
        return math.exp(le[0] - 0.5 * (x - lt[0]))
    if x >= lt[-1]:
        return math.exp(le[-1] - 0.5 * (x - lt[-1]))
    for i in range(len(lt) - 1):
        if lt[i] <= x <= lt[i + 1]:
            f = (x - lt[i]) / (lt[i + 1] - lt[i])
            return math.exp(le[i] + f * (le[i + 1] - le[i]))
    raise AssertionError


def run(name, W, H):
    p = ptamd.Preset(name, W, H)
    scene = ptamd.Scene(p.objects, p.materials)
    scene.set_sky(*p.sky)
    n = W * H
    ref, _ = ptamd.render(scene, ptamd.Film(W, H, seed=1), p.camera, a.ref_spp, p.max_depth, rng=ptamd.RNG_SAMPLE, mis=True)
    ref = ref.astype(np.float64)
    rgb = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    out = torch.zeros_like(rgb)
    aov = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    rows = []
    for spp in ladder:
        film = ptamd.Film(W, H, seed=2)
        ms = []
        for _ in range(a.repeat + 1):   # (the first frame builds the wide tree and measures tile costs)
            _, st = ptamd.render(scene, film, p.camera, spp, p.max_depth, out=rgb.data_ptr(), stream=stream.cuda_stream,
                                 rng=ptamd.RNG_SAMPLE, mis=True)
            ms.append(st.kernel_ms)
        aov_ms, dn_ms = [], []
        for _ in range(a.repeat + 1):
            _, st = ptamd.render_aov(scene, film, p.camera, out=aov.data_ptr(), stream=stream.cuda_stream)
            aov_ms.append(st.kernel_ms)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ptamd.denoise(film, rgb.data_ptr(), aov.data_ptr(), out=out.data_ptr(), stream=stream.cuda_stream, spp=spp)
            e1.record(stream)
            e1.synchronize()
            dn_ms.append(e0.elapsed_time(e1))
        noisy, den = host(rgb, np.float32, 3), host(out, np.float32, 3)
        rows.append({"spp": spp, "frame_ms": statistics.median(ms[1:]), "aov_ms": statistics.median(aov_ms[1:]),
                     "denoise_ms": statistics.median(dn_ms[1:]), "rmse_noisy": rmse(noisy, ref), "rmse_denoised": rmse(den, ref)})
    times, errs = [r["frame_ms"] for r in rows], [r["rmse_noisy"] for r in rows]
    print(f"\n### {name} {W}x{H}, MIS, sample mode, reference {a.ref_spp} spp\n")
    print("| spp | frame ms | AOV ms | denoise ms (5 passes) | RMSE noisy | RMSE denoised | ratio | noisy RMSE at the same total time | its ratio to denoised |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        r["total_ms"] = r["frame_ms"] + r["aov_ms"] + r["denoise_ms"]
        r["rmse_noisy_equal_time"] = interp(times, errs, r["total_ms"])
        print(f"| {r['spp']} | {r['frame_ms']:.3f} | {r['aov_ms']:.3f} | {r['denoise_ms']:.3f} | {r['rmse_noisy']:.4f} | "
              f"{r['rmse_denoised']:.4f} | {r['rmse_denoised'] / r['rmse_noisy']:.3f} | {r['rmse_noisy_equal_time']:.4f} | "
              f"{r['rmse_noisy_equal_time'] / r['rmse_denoised']:.2f} |")
    sys.stdout.flush()
    return rows


result = {}
for name in a.scenes.split(","):
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        result[f"{name} {size}"] = run(name, W, H)
if a.json:
    with open(a.json, "w") as f:
        json.dump({"ref_spp": a.ref_spp, "ladder": ladder, "repeat": a.repeat, "results": result}, f, indent=1)
