"""pt_render_ex's launch plan (host/pt_render_plan.hpp) on the CPU, through tools/micro/render_plan_check
(tests/cpp/render_plan_check.cpp, built by the package Makefile with the host compiler alone).

The plan is host arithmetic that no image test sees: thresholds, grids, split tiles, tile priorities and
cost measurement change speed only.  The expected values below were read off pt_render_ex as it stood
before the plan was split out of it (the options, the knobs' defaults and their clamping included), so a
changed value here is a changed launch.

Base case: a 64 x 64 film in one part (8 x 8 tiles, 4096 pixels); a flat triangle-only Lambertian scene of
1000 objects with its wide tree and edge records ready, the default sky, no emitter, centre 0, extent 1,
wide depth 5, binary depth 8; the camera at the centre with lens 0; 4 spp, depth 8; opts NULL; no PT_*
variable in the environment.
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(REPO, "tools", "micro", "render_plan_check")

SIMPLE, WAVEFRONT, WIDE = 1, 2, 3             # pt.h: PT_KERNEL_*
SAMPLE = 1                                    # PT_RNG_SAMPLE
RGBA8 = 1                                     # PT_OUT_RGBA8
IDENTITY, ACCUMULATE, NEE, MIS = 1, 2, 4, 8   # PT_RENDER_* flag bits
ERR_INVALID = 1

BASE = dict(width=64, height=64, nrows=64, npix=4096, wideReady=1, haveWtris=1, lambertOnly=1, nobj=1000, extent=1,
            wideDepth=5, depth=8, spp=4, max_depth=8)
LONG = dict(max_depth=50, haveOrder=1, critK=256)   # compat, long paths, a film that has rendered before
DEEP = dict(LONG, wideDepth=12)


def run(args, env=None):
    """The checker's key=value lines as a dict (numbers as int); env: the PT_* knobs of the call, no others."""
    assert os.path.exists(CHECK), "tools/micro/render_plan_check not built (make -C path-tracer-cuda-opengl_amd)"
    e = {k: v for k, v in os.environ.items() if not k.startswith("PT_")}
    e.update(env or {})
    r = subprocess.run([CHECK] + args, capture_output=True, text=True, timeout=60, env=e)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    out = {}
    for line in r.stdout.splitlines():
        k, v = line.split("=", 1)
        out[k] = v if k == "message" else int(v)
    return out


def plan(*facts, env=None, **more):
    """The plan for BASE updated by `facts` (dicts) and `more`."""
    f = dict(BASE)
    for d in facts:
        f.update(d)
    f.update(more)
    return run([f"{k}={v}" for k, v in f.items()], env)


def expect(got, **want):
    assert "error" not in got, got
    assert {k: got[k] for k in want} == want


def test_compat_default_kernel():
    expect(plan(), kernel=WIDE, stack=8, tri=1, ahead=0, lit=0, camFar=0, leafBatch=28, shadeBatch=28, nodeMin=8, critOn=0,
           splitTiles=0, compatGrid=64, resolve=0, prioTiles=0, tiles_x=8, ntiles=64)
    expect(plan(LONG), critOn=1, nCrit=256, critLanes=4, critWaves=64, splitTiles=0, compatGrid=128, prioTiles=1024,
           prioLevel=2, nodeMin=8)
    expect(plan(LONG, critK=0), critOn=1, nCrit=0, compatGrid=64)
    expect(plan(DEEP), stack=16, leafBatch=24, shadeBatch=24, critOn=0, splitWays=2, splitTiles=64, compatGrid=128, nodeMin=8)
    expect(plan(DEEP, haveOrder=0), splitTiles=0, compatGrid=64)
    expect(plan(DEEP, max_depth=16), splitTiles=0)
    expect(plan(LONG, flags=IDENTITY), critOn=0, splitTiles=0, compatGrid=64, prioTiles=0)


def test_compat_environment_knobs():
    expect(plan(DEEP, env={"PT_SPLIT_WAYS": "1"}), splitTiles=0)
    expect(plan(LONG, env={"PT_CRIT_LANES": "100"}), critLanes=64)
    expect(plan(LONG, env={"PT_COMPAT_GRID_LIMIT": "10"}), compatGrid=10)


def test_sample_blocks_and_tasks():
    expect(plan(rng=SAMPLE, spp=256), block=16, nblocks=16, ngroups=16, nblocksShift=4, ntasks=65536, ahead=1, leafBatch=28,
           shadeBatch=28, nodeMin=8, resolve=1, rawOut=0)
    expect(plan(rng=SAMPLE, spp=100), nblocks=7, nblocksShift=-1, ntasks=28672)
    expect(plan(rng=SAMPLE, spp=4096), block=64, nblocks=64)
    expect(plan(rng=SAMPLE, spp=100, chunk=10), block=10, nblocks=10)


def test_sample_measures_tile_costs():
    s = dict(rng=SAMPLE, spp=256)
    expect(plan(s), measureCost=1)
    expect(plan(s, haveOrder=1, framesSinceCost=3), measureCost=0)
    expect(plan(s, haveOrder=1, framesSinceCost=7), measureCost=1)
    expect(plan(s, flags=IDENTITY), measureCost=0)


def test_persistent_waves():
    assert run(["waves", "256", "20", "65536"]) == {"nwaves": 1024}
    assert run(["waves", "256", "0", "65536"]) == {"nwaves": 256}


def test_ahead_kernels_only_where_they_exist():
    s = dict(rng=SAMPLE, spp=256)
    expect(plan(s), ahead=1, tri=1)
    expect(plan(s, lens=0.1), ahead=0)
    expect(plan(s, lambertOnly=0), ahead=0)
    expect(plan(s, flags=NEE, nLights=3), ahead=0, nee=1)
    expect(plan(s, wideDepth=20), ahead=0, stack=24, leafBatch=24, shadeBatch=24)
    expect(plan(s, env={"PT_SHADE_AHEAD": "0"}), ahead=0, tri=1)
    expect(plan(s, env={"PT_WIDE_TRI": "0"}), ahead=0, tri=0)
    expect(plan(s, hasSpheres=1), ahead=0, tri=0)
    expect(plan(s, flags=NEE, nLights=0), nee=0, ahead=1)
    expect(plan(s, flags=MIS, nLights=3), nee=1, mis=1)


def test_lit_and_far_camera():
    expect(plan(hasEmissive=1), lit=1)
    expect(plan(skyZ_x=0.25), lit=1)
    for rng in (0, SAMPLE):
        expect(plan(instanced=1, rng=rng), leafBatch=16, shadeBatch=20, tri=0, nodeMin=8)
    expect(plan(instanced=1, cam_x=2.5), camFar=1)
    expect(plan(cam_x=2.5), camFar=0)
    expect(plan(cam_x=8.5), camFar=1)
    expect(plan(cam_x=7.9, lens=0.2, right_x=1, up_y=1), camFar=1)
    # A NaN coordinate drops out of the host's maximum (std::max(m, NaN) = m), so the camera counts as near:
    # what pt_render_ex has always computed.
    expect(plan(cam_x="nan"), camFar=0)


def test_binary_kernels():
    expect(plan(kernel=WAVEFRONT), leafBatch=20, shadeBatch=12, nodeMin=8)
    expect(plan(kernel=WAVEFRONT, rng=SAMPLE), leafBatch=24, shadeBatch=32, nodeMin=8)
    expect(plan(kernel=SIMPLE), leafBatch=0, shadeBatch=12)
    expect(plan(kernel=SIMPLE, rng=SAMPLE), leafBatch=0, shadeBatch=32)
    expect(plan(kernel=WAVEFRONT, nobj=1), stack=16)
    expect(plan(kernel=WAVEFRONT, depth=15), stack=16)
    expect(plan(kernel=WAVEFRONT, depth=16), stack=24)
    deep = plan(kernel=WAVEFRONT, depth=40)
    expect(deep, stack=48, compatGrid=64, spill_bytes=deep["compatGrid"] * 64 * 16 * 4)


def test_kernel_from_the_environment_only_by_default():
    expect(plan(env={"PT_RENDER_KERNEL": "simple"}), kernel=SIMPLE)
    expect(plan(env={"PT_RENDER_KERNEL": "wavefront"}), kernel=WAVEFRONT)
    expect(plan(env={"PT_RENDER_KERNEL": "other"}), kernel=WIDE)
    expect(plan(kernel=0, env={"PT_RENDER_KERNEL": "simple"}), kernel=SIMPLE)
    expect(plan(kernel=WIDE, env={"PT_RENDER_KERNEL": "simple"}), kernel=WIDE)
    expect(plan(kernel=WAVEFRONT, env={"PT_RENDER_KERNEL": "simple"}), kernel=WAVEFRONT)


def test_thresholds_options_then_environment_then_default():
    expect(plan(leaf_batch=100), leafBatch=64)
    expect(plan(leaf_batch=5, env={"PT_LEAF_BATCH": "12"}), leafBatch=5)
    expect(plan(leaf_batch=0, env={"PT_LEAF_BATCH": "12"}), leafBatch=12)
    expect(plan(leaf_batch=0, env={"PT_LEAF_BATCH": "0"}), leafBatch=28)
    expect(plan(leaf_batch=0, env={"PT_LEAF_BATCH": "200"}), leafBatch=64)


def test_resolve_and_accumulation():
    expect(plan(out_format=RGBA8), resolve=1, rawOut=1)
    expect(plan(flags=ACCUMULATE), resolve=1, rawOut=1)
    expect(plan(flags=ACCUMULATE, rng=SAMPLE, accumSamples=512), sampleBase=512)
    expect(plan(flags=ACCUMULATE, accumSamples=512), sampleBase=0)


MSG = {
    "format": "pt_render_ex: unknown output format",
    "accum": "pt_render_ex: accumulated samples must stay below 2^24",
    "kernel": "pt_render_ex: unknown kernel",
    "inst_kernel": "pt_render_ex: instanced scenes render with the wide kernel (PT_KERNEL_WIDE)",
    "mis_inst": "pt_render_ex: PT_RENDER_MIS is not available on instanced scenes (flat scenes only)",
    "mis_wf": "pt_render_ex: PT_RENDER_MIS is not available with PT_KERNEL_WAVEFRONT "
              "(PT_KERNEL_WIDE, PT_KERNEL_DEFAULT or PT_KERNEL_SIMPLE)",
    "nee_inst": "pt_render_ex: PT_RENDER_NEE is not available on instanced scenes (flat scenes only)",
    "nee_wf": "pt_render_ex: PT_RENDER_NEE is not available with PT_KERNEL_WAVEFRONT "
              "(PT_KERNEL_WIDE, PT_KERNEL_DEFAULT or PT_KERNEL_SIMPLE)",
    "rng": "pt_render_ex: unknown rng mode",
    "width": "sample mode: frame width and rows must be < 65536",
    "tasks": "sample mode: too many (pixel, block) tasks (tiles x blocks x 64 must stay below 2^32 - 2^26); "
             "raise the block size (chunk)",
}
OVERFLOW = dict(accumSamples=(1 << 24) - 4)   # with ACCUMULATE and the base's 4 spp: 2^24
WIDE_FILM = dict(width=65536, nrows=8, npix=65536 * 8)
BIG_FILM = dict(width=8192, height=8192, nrows=8192, npix=8192 * 8192, rng=SAMPLE, chunk=1)

ERRORS = [
    # each alone ...
    ("format", dict(out_format=7)),
    ("accum", dict(OVERFLOW, flags=ACCUMULATE)),
    ("kernel", dict(kernel=9)),
    ("inst_kernel", dict(instanced=1, kernel=SIMPLE)),
    ("inst_kernel", dict(instanced=1, kernel=WAVEFRONT)),
    ("mis_inst", dict(instanced=1, flags=MIS)),
    ("mis_wf", dict(kernel=WAVEFRONT, flags=MIS)),
    ("nee_inst", dict(instanced=1, flags=NEE)),
    ("nee_wf", dict(kernel=WAVEFRONT, flags=NEE)),
    ("rng", dict(rng=5)),
    ("width", dict(WIDE_FILM, rng=SAMPLE)),
    ("tasks", dict(BIG_FILM, spp=63)),
    # ... and before the ones that follow it
    ("format", dict(OVERFLOW, out_format=7, flags=ACCUMULATE | MIS, kernel=9, instanced=1, rng=5)),
    ("accum", dict(OVERFLOW, flags=ACCUMULATE | MIS, kernel=9, instanced=1, rng=5)),
    ("kernel", dict(kernel=9, instanced=1, flags=MIS, rng=5)),
    ("inst_kernel", dict(instanced=1, kernel=WAVEFRONT, flags=MIS, rng=5)),
    ("mis_inst", dict(instanced=1, flags=MIS | NEE, rng=5)),
    ("mis_wf", dict(kernel=WAVEFRONT, flags=MIS | NEE, rng=5)),
    ("nee_inst", dict(instanced=1, flags=NEE, rng=5)),
    ("nee_wf", dict(WIDE_FILM, kernel=WAVEFRONT, flags=NEE, rng=5)),
    ("rng", dict(WIDE_FILM, rng=5)),
    ("width", dict(width=65536, nrows=65536, npix=1 << 32, rng=SAMPLE, chunk=1, spp=64)),
]


@pytest.mark.parametrize("name,facts", ERRORS, ids=[f"{i}-{n}" for i, (n, _) in enumerate(ERRORS)])
def test_errors_in_order(name, facts):
    got = plan(facts)
    assert got == {"error": ERR_INVALID, "message": MSG[name]}


def test_instanced_lights_lift_the_refusal():
    expect(plan(instanced=1, instLights=1, flags=MIS, nLights=3), nee=1, mis=1)
    expect(plan(instanced=1, instLights=1, flags=NEE, nLights=3), nee=1, mis=0)


def test_task_limit():
    expect(plan(BIG_FILM, spp=62), ntasks=62 << 26, ngroups=62, ntiles=1 << 20)
    assert plan(BIG_FILM, spp=63) == {"error": ERR_INVALID, "message": MSG["tasks"]}
