"""The wide render kernels' triangle-only instantiations (renderKernelWF<.., TRI>) on the GPU.

A triangle-only, non-instanced scene launches kernels in which the scene's hasSpheres flag is a
compile-time 0; PT_WIDE_TRI=0 launches the generic kernels, which read the flag at run time, on the
same scene.  Nothing may differ between the two, nor from the binary wavefront kernel and the oracle:
pixels, RNG states, rays and paths are compared bit for bit, at 48 x 40, 4 spp, depth 50, in sample
mode and over two compat launches on one film (depth 50 > 16: the second launch runs critical-pixel
waves, the per-lane loop under TRI).  The knob is read when a launch is enqueued, so each setting is
recorded by a child process of its own (tests/tri_kernel_scenes.py lists the scenes), once per session.

Node visits and primitive tests are compared between the knob settings in the compat launches, whose
waves are fixed (a lane per pixel of a tile, or per listed critical pixel).  In sample mode the lanes
take tasks from a shared counter, so which lanes share a wave -- and with it what a speculating lane
visits -- varies from run to run of one build (tests/test_gpu_leaf_edges.py notes the same); there the
comparison is of pixels, states, rays and paths.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  before libpt.so loads (the two must share torch's HIP runtime)

import tri_kernel_scenes as tk
from node_step_scenes import CHUNK, DEPTH, H, SEED, SPP, W

pytestmark = pytest.mark.gpu

VARIANTS = ("sample", "compat1", "compat2")
RAYS, PATHS, VISITS, TRIS, SPHERES = range(5)
FLAT = sorted(tk.flat_cases())
FLAT_TREES = FLAT + [f"{n}@{t}" for n in tk.TREES for t in ("device", "rebuilt")]
EVERY = FLAT_TREES + ["lit", "lit/nee", "lit/mis", "hidden_sphere", "was_sphere", "instanced"]


@pytest.fixture(scope="module")
def recorded(gpu, tmp_path_factory):
    """{knob: arrays}: tri_kernel_scenes.record() under PT_WIDE_TRI=1 and =0, a fresh process each."""
    out = {}
    d = tmp_path_factory.mktemp("tri_kernels")
    for knob in ("1", "0"):
        path = str(d / f"wide_tri_{knob}.npz")
        r = subprocess.run([sys.executable, os.path.abspath(tk.__file__), path], env=dict(os.environ, PT_WIDE_TRI=knob),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"PT_WIDE_TRI={knob}: {r.stdout[-1000:]}\n{r.stderr[-3000:]}"
        with np.load(path) as z:
            out[knob] = {k: z[k] for k in z.files}
    return out


_oracle = {}


def oracle_frames(pt, orc, key, objs, mats, campar):
    """Sample mode, and two successive compat launches (the second starts from the first's states); once per scene."""
    if key not in _oracle:
        nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
        c = pt.camera_to_array(pt.camera_make(*campar))
        rows = np.arange(H, dtype=np.int32)
        ref = {"sample": orc.render_sample(objs, mats, nodes, c, W, H, rows, SPP, DEPTH, SEED, CHUNK, nthreads=8)}
        states = orc.film_states(SEED, W, rows)
        for launch in (1, 2):
            ref[f"compat{launch}"] = orc.render(objs, mats, nodes, c, W, H, rows, SPP, DEPTH, states, nthreads=8)
            ref[f"states{launch}"] = states.copy()
        _oracle[key] = ref
    return _oracle[key]


def assert_equals_oracle(rec, name, ref):
    for v in VARIANTS:
        msg = f"{name}, {v}"
        rgb, st = ref[v]
        np.testing.assert_array_equal(rec[f"{name}|{v}|rgb"], np.ascontiguousarray(rgb).view(np.uint32), err_msg=msg)
        n = rec[f"{name}|{v}|n"]
        assert (int(n[RAYS]), int(n[PATHS])) == (st.rays, W * H * SPP), msg
        if v != "sample":
            np.testing.assert_array_equal(rec[f"{name}|{v}|rng"], ref["states" + v[-1]], err_msg=msg)


@pytest.mark.parametrize("name", EVERY)
def test_both_knob_settings_render_the_same(recorded, name):
    """PT_WIDE_TRI=1 against =0: the TRI kernels against the generic ones on the triangle-only scenes
    (LIT, NEE and MIS ones on `lit`); the scenes with a sphere, with a sphere once, and the instanced
    one take the same kernels under both settings."""
    on, off = recorded["1"], recorded["0"]
    for v in VARIANTS:
        msg = f"{name}, {v}"
        np.testing.assert_array_equal(on[f"{name}|{v}|rgb"], off[f"{name}|{v}|rgb"], err_msg=msg)
        np.testing.assert_array_equal(on[f"{name}|{v}|rng"], off[f"{name}|{v}|rng"], err_msg=msg)
        a, b = on[f"{name}|{v}|n"], off[f"{name}|{v}|n"]
        print(msg, "counters", a.tolist(), b.tolist())
        assert (a[RAYS], a[PATHS]) == (b[RAYS], b[PATHS]), msg
        if v != "sample":   # fixed waves: the same visits and tests (see the module's docstring)
            np.testing.assert_array_equal(a, b, err_msg=msg)
        assert a[PATHS] == W * H * SPP and a[TRIS] > 0, msg


@pytest.mark.parametrize("name", FLAT)
def test_tri_kernels_equal_wavefront_kernel_and_oracle(pt, orc, recorded, name):
    objs, mats, campar = tk.flat_cases()[name]
    ref = oracle_frames(pt, orc, name, objs, mats, campar)
    for knob in ("1", "0"):
        rec = recorded[knob]
        assert_equals_oracle(rec, name, ref)
        assert_equals_oracle(rec, name + "/wavefront", ref)
        for v in VARIANTS:
            assert rec[f"{name}|{v}|n"][SPHERES] == 0
            if len(objs) > 1:   # (a single primitive is the root: the binary kernels count no test of it)
                assert rec[f"{name}/wavefront|{v}|n"][TRIS] == ref[v][1].tri_tests, f"{name}, {v}"


@pytest.mark.parametrize("tree,source", [("device", 2), ("rebuilt", 1)])
@pytest.mark.parametrize("name", tk.TREES)
def test_device_built_and_rebuilt_trees(pt, orc, recorded, name, tree, source):
    objs, mats, campar = tk.flat_cases()[name]
    ref = oracle_frames(pt, orc, name, objs, mats, campar)
    for knob in ("1", "0"):
        assert_equals_oracle(recorded[knob], f"{name}@{tree}", ref)
        assert recorded[knob][f"{name}@{tree}|tree"][0] == source
        assert recorded[knob][f"{name}|tree"][0] == 1


def test_scenes_select_every_stack_size(recorded):
    """wideStackFor: 8, 16 and 24 entries for trees of depth <= 8, <= 16, <= 24 (each its own kernel)."""
    stack = {n: next(s for s in (8, 16, 24) if recorded["1"][f"{n}|tree"][1] <= s) for n in FLAT}
    assert stack["stack16"] == 16 and stack["stack24"] == 24
    assert all(stack[n] == 8 for n in FLAT if not n.startswith("stack")), stack


def test_lit_scene_runs_the_nee_and_mis_kernels(recorded):
    """`lit` has sampled lights: the flags change the frame (so the NEE and MIS instantiations ran),
    and MIS traces the NEE frame's rays."""
    rec = recorded["1"]
    assert rec["lit|lights"][0] > 0
    for v in VARIANTS:
        assert (rec[f"lit|{v}|rgb"] != rec[f"lit/nee|{v}|rgb"]).any()
        assert (rec[f"lit/nee|{v}|rgb"] != rec[f"lit/mis|{v}|rgb"]).any()
        assert rec[f"lit/nee|{v}|n"][RAYS] == rec[f"lit/mis|{v}|n"][RAYS] > rec[f"lit|{v}|n"][RAYS]
        assert rec[f"lit|{v}|rgb"].view(np.float32).max() > 1.0   # the lamp is seen


def test_hidden_sphere_takes_the_generic_kernel(recorded):
    """`shadow` plus a sphere no ray reaches: the same pixels, states and rays from another tree
    (other visits and tests), by the generic kernel -- the TRI kernels count no sphere test -- whatever
    the knob says (test_both_knob_settings_render_the_same: equal counters)."""
    for knob in ("1", "0"):
        rec = recorded[knob]
        for v in VARIANTS:
            np.testing.assert_array_equal(rec[f"hidden_sphere|{v}|rgb"], rec[f"shadow|{v}|rgb"])
            np.testing.assert_array_equal(rec[f"hidden_sphere|{v}|rng"], rec[f"shadow|{v}|rng"])
            a, b = rec[f"hidden_sphere|{v}|n"], rec[f"shadow|{v}|n"]
            assert (a[RAYS], a[PATHS]) == (b[RAYS], b[PATHS])
            assert a[SPHERES] > 0 and b[SPHERES] == 0
        for v in ("compat1", "compat2"):
            assert rec[f"hidden_sphere|{v}|n"][VISITS:].tolist() != rec[f"shadow|{v}|n"][VISITS:].tolist()


def test_scene_that_held_a_sphere_stays_generic_and_matches_the_oracle(pt, orc, recorded):
    """hasSpheres is sticky: the sphere overwritten by a triangle, the scene rebuilt."""
    objs, mats = tk.was_sphere_objects()
    ref = oracle_frames(pt, orc, "was_sphere", objs, mats, tk.shadow_scene()[2])
    for knob in ("1", "0"):
        assert_equals_oracle(recorded[knob], "was_sphere", ref)
        for v in VARIANTS:
            assert recorded[knob][f"was_sphere|{v}|n"][SPHERES] == 0
