#!/usr/bin/env python3
"""What temporal reprojection of the frame history (pt_film_temporal) buys on low-spp frames of the lit
presets along a camera dolly, alone and in front of the a-trous filter, and what it costs (GPU; a
measurement, not a test).

For each scene and frame size, in sample mode with the default (wide) kernel and PT_RENDER_MIS: the camera
makes --frames - 1 pt_camera_move steps (FORWARD by --forward seconds, RIGHT by --right seconds each); every
frame is rendered at the rung's spp (film seed 2, the streams running on from frame to frame), its AOVs are
taken and pt_film_temporal is called with the binding's defaults.  For the last frame:
  * the reference image: one long MIS run at the last camera, film seed 1;
  * RMSE against it, in the sqrt(mean) domain pt_render writes, over all pixels and channels, of the noisy
    frame, the temporal output, a-trous alone (5 passes, sigma_color = 1.2 / sqrt(spp)) and temporal followed
    by a-trous (sigma_color = 1.2 / sqrt(spp x the mean history length of the hit pixels));
  * the share of hit pixels that found history (length > 1) and the hit pixels' mean history length;
  * device times: the frame's kernel_ms, the AOV pass's kernel_ms, the temporal pass and the a-trous call
    (events around the enqueued call), each the median of --repeat runs after a warm-up.  The timed temporal
    calls repeat the last frame's on a second film that holds the history of the frames before it; between
    runs the frame before is replayed on it, so each timed call gathers from a history at the previous
    camera, as the real one did;
  * the temporal pass's effective bytes per second over the traffic it must move: per pixel 60 B read at
    the pixel, the kept projections' 4 x 48 B gathered (counted in full for every hit pixel), 64 B written.
The reference's own noise is in every figure and is not removed.

usage: temporal_noise.py [--scenes cornell_lit,bunny_cornell_lit] [--sizes 512x512,1920x1080] [--ref-spp 4096]
                         [--ladder 1,4] [--frames 16] [--forward 4.0] [--right 2.0] [--repeat 3] [--json FILE]
Prints a Markdown table per scene and size and, with --json, writes every figure.
"""
import argparse
import json
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
ap.add_argument("--ladder", default="1,4")
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--forward", type=float, default=4.0)
ap.add_argument("--right", type=float, default=2.0)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--json")
a = ap.parse_args()
ladder = [int(x) for x in a.ladder.split(",")]
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev)
S = stream.cuda_stream


def rmse(x, ref):
    return float(np.sqrt(np.mean((x.astype(np.float64) - ref) ** 2)))


def host(t, dtype, cols):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype).reshape(-1, cols)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def cameras(p):
    cam = ptamd.Camera.from_buffer_copy(bytes(p.camera))
    cams = [ptamd.Camera.from_buffer_copy(bytes(cam))]
    for _ in range(a.frames - 1):
        ptamd.camera_move(cam, 0, a.forward)
        ptamd.camera_move(cam, 3, a.right)
        cams.append(ptamd.Camera.from_buffer_copy(bytes(cam)))
    return cams


def run(name, W, H):
    p = ptamd.Preset(name, W, H)
    scene = ptamd.Scene(p.objects, p.materials)
    scene.set_sky(*p.sky)
    n = W * H
    cams = cameras(p)
    step = float(np.linalg.norm(ptamd.camera_to_array(cams[-1])[:3] - ptamd.camera_to_array(cams[0])[:3])) / max(1, a.frames - 1)
    ref, _ = ptamd.render(scene, ptamd.Film(W, H, seed=1), cams[-1], a.ref_spp, p.max_depth, rng=ptamd.RNG_SAMPLE, mis=True)
    ref = ref.astype(np.float64)
    rgb = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    prev_rgb, tmp = torch.zeros_like(rgb), torch.zeros_like(rgb)
    out, den, both = torch.zeros_like(rgb), torch.zeros_like(rgb), torch.zeros_like(rgb)
    length = torch.zeros(n, dtype=torch.float32, device=dev)
    aov = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    prev_aov = torch.zeros_like(aov)
    torch.cuda.synchronize(dev)
    rows = []
    for spp in ladder:
        film, timing = ptamd.Film(W, H, seed=2), ptamd.Film(W, H, seed=3)
        for f, cam in enumerate(cams):
            if f == len(cams) - 1:
                prev_rgb.copy_(rgb)
                prev_aov.copy_(aov)
            ptamd.render(scene, film, cam, spp, p.max_depth, out=rgb.data_ptr(), stream=S, rng=ptamd.RNG_SAMPLE, mis=True)
            ptamd.render_aov(scene, film, cam, out=aov.data_ptr(), stream=S)
            ptamd.temporal(film, rgb.data_ptr(), aov.data_ptr(), cam, out=out.data_ptr(), out_len=length.data_ptr(), stream=S)
            if f < len(cams) - 1:   # the second film follows, one call behind the frame it will be timed on
                ptamd.temporal(timing, rgb.data_ptr(), aov.data_ptr(), cam, out=tmp.data_ptr(), stream=S)
        stream.synchronize()
        hit = host(aov, ptamd.AOV_DTYPE, 1).reshape(-1)["obj"] >= 0
        ln = host(length, np.float32, 1).reshape(-1)
        mean_len = float(ln[hit].mean())
        ptamd.denoise(film, rgb.data_ptr(), aov.data_ptr(), out=den.data_ptr(), stream=S, spp=spp)
        ptamd.denoise(film, out.data_ptr(), aov.data_ptr(), out=both.data_ptr(), stream=S, spp=spp * mean_len)
        stream.synchronize()
        # times: the last frame again (the film's streams run on: another frame of the same cost)
        frame_ms, aov_ms, tp_ms, dn_ms = [], [], [], []
        for _ in range(a.repeat + 1):
            _, st = ptamd.render(scene, film, cams[-1], spp, p.max_depth, out=tmp.data_ptr(), stream=S, rng=ptamd.RNG_SAMPLE, mis=True)
            frame_ms.append(st.kernel_ms)
            _, st = ptamd.render_aov(scene, film, cams[-1], out=aov.data_ptr(), stream=S)
            aov_ms.append(st.kernel_ms)
            tp_ms.append(timed(lambda: ptamd.temporal(timing, rgb.data_ptr(), aov.data_ptr(), cams[-1], out=tmp.data_ptr(), stream=S)))
            # put the second film's history back: that of the frame before, whose own history is now two calls old
            ptamd.temporal(timing, prev_rgb.data_ptr(), prev_aov.data_ptr(), cams[-2], out=tmp.data_ptr(), stream=S)
            dn_ms.append(timed(lambda: ptamd.denoise(film, rgb.data_ptr(), aov.data_ptr(), out=tmp.data_ptr(), stream=S, spp=spp)))
        noisy = host(rgb, np.float32, 3)
        tp = statistics.median(tp_ms[1:])
        moved = n * (60 + 64) + int(hit.sum()) * 4 * 48
        rows.append({"spp": spp, "frame_ms": statistics.median(frame_ms[1:]), "aov_ms": statistics.median(aov_ms[1:]),
                     "temporal_ms": tp, "atrous_ms": statistics.median(dn_ms[1:]), "atrous_pass_ms": statistics.median(dn_ms[1:]) / 5,
                     "rmse_noisy": rmse(noisy, ref), "rmse_temporal": rmse(host(out, np.float32, 3), ref),
                     "rmse_atrous": rmse(host(den, np.float32, 3), ref), "rmse_temporal_atrous": rmse(host(both, np.float32, 3), ref),
                     "history_share": float((ln[hit] > 1).mean()), "mean_length": mean_len, "bytes": moved,
                     "tb_per_s": moved / (tp * 1e-3) / 1e12})
    print(f"\n### {name} {W}x{H}, MIS, sample mode, {a.frames} frames, {step:.2f} units per frame, reference {a.ref_spp} spp\n")
    print("| spp | RMSE noisy | temporal | ratio | a-trous | temporal + a-trous | ratio to a-trous | hits with history | mean length | "
          "frame ms | AOV ms | temporal ms | a-trous ms (per pass) | temporal TB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['spp']} | {r['rmse_noisy']:.4f} | {r['rmse_temporal']:.4f} | {r['rmse_temporal'] / r['rmse_noisy']:.3f} | "
              f"{r['rmse_atrous']:.4f} | {r['rmse_temporal_atrous']:.4f} | {r['rmse_temporal_atrous'] / r['rmse_atrous']:.3f} | "
              f"{100 * r['history_share']:.1f} % | {r['mean_length']:.2f} | {r['frame_ms']:.3f} | {r['aov_ms']:.3f} | "
              f"{r['temporal_ms']:.3f} | {r['atrous_ms']:.3f} ({r['atrous_pass_ms']:.3f}) | {r['tb_per_s']:.2f} |")
    sys.stdout.flush()
    return rows


result = {}
for name in a.scenes.split(","):
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        result[f"{name} {size}"] = run(name, W, H)
if a.json:
    with open(a.json, "w") as f:
        json.dump({"ref_spp": a.ref_spp, "ladder": ladder, "frames": a.frames, "repeat": a.repeat, "results": result}, f, indent=1)
