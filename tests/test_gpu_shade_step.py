"""The step kernels' SHADE step on the GPU, on the inputs where its slimmed parts can go wrong.

Scalar wave counters, 32-bit record offsets, the 24-bit pixel index of a finished task, one range
check for a ray's three reciprocals, the TRI kernels' hit record without the sphere normal, and
Philox's first two rounds written out change no result: pixels, film
RNG states, rays, paths and primitive tests are compared bit for bit between the wide, wavefront and
simple kernels and the oracle -- sample mode and two compat launches on one film (the second runs
critical-pixel waves), host-built and device-built trees.  The wide kernel's node visits and primitive
tests of the compat launches, whose waves are fixed, are those of the build before the change
(tests/golden/shade_step.npz); in sample mode they vary with lane placement from run to run and are
not compared.  tests/shade_step_scenes.py describes the cases.
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401  before libpt.so loads (the two must share torch's HIP runtime)

import shade_step_scenes as ss
from node_step_scenes import CHUNK, DEPTH, H, SEED, SPP, W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade_step.npz")
ORACLE_CASES = ["edges", "depth0", "depth1", "bunny", "wide_film", "tall_film", "slit_y", "slit_x", "slit_xy",
                "slit_yz", "materials", "lamp0", "cornell"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def cases(pt):
    return ss.cases(pt)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def oracle_frames(pt, orc, case, seed=SEED):
    objs, mats, cam, w, h, spp, depth = case
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    c = pt.camera_to_array(cam)
    rows = np.arange(h, dtype=np.int32)
    ref = {"sample": orc.render_sample(objs, mats, nodes, c, w, h, rows, spp, depth, seed, CHUNK, nthreads=8)}
    states = orc.film_states(seed, w, rows)
    ref["compat"], ref["states"] = [], []
    for _ in range(2):
        ref["compat"].append(orc.render(objs, mats, nodes, c, w, h, rows, spp, depth, states, nthreads=8))
        ref["states"].append(states.copy())
    return ref


def check_kernel(pt, gpu, scene, case, kernel, ref, what):
    """One kernel's sample-mode frame and two compat launches against the oracle's; returns the compat launches."""
    objs, _, cam, w, h, spp, depth = case
    counted = len(objs) > 1   # (a single primitive is the root: the binary kernels count no test of it)
    f = pt.Film(w, h, SEED, device=gpu)
    rgb, st = pt.render(scene, f, cam, spp, depth, kernel=kernel, rng=pt.RNG_SAMPLE, chunk=CHUNK)
    oref, ost = ref["sample"]
    print(what, "sample", st.rays, st.paths, st.node_visits, st.tri_tests, "oracle", ost.rays, ost.tri_tests)
    np.testing.assert_array_equal(bits(rgb), bits(oref), err_msg=f"{what}, sample mode")
    assert (st.rays, st.paths) == (ost.rays, w * h * spp), f"{what}, sample mode"
    if kernel == pt.KERNEL_WAVEFRONT and counted:
        assert (st.tri_tests, st.sphere_tests) == (ost.tri_tests, ost.sphere_tests), what
    launches = ss.compat_launches(pt, gpu, scene, case, kernel)
    for k, (rgb, st, rng) in enumerate(launches):
        oref, ost = ref["compat"][k]
        msg = f"{what}, compat launch {k + 1}"
        print(msg, st.rays, st.paths, st.node_visits, st.tri_tests, "oracle", ost.rays, ost.tri_tests)
        np.testing.assert_array_equal(bits(rgb), bits(oref), err_msg=msg)
        np.testing.assert_array_equal(rng, ref["states"][k], err_msg=msg)
        assert (st.rays, st.paths) == (ost.rays, w * h * spp), msg
        if kernel == pt.KERNEL_WAVEFRONT and counted:
            assert (st.tri_tests, st.sphere_tests) == (ost.tri_tests, ost.sphere_tests), msg
    return launches


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_every_kernel_equals_the_oracle_and_the_recorded_work(pt, orc, gpu, cases, golden, name):
    case = cases[name]
    ref = oracle_frames(pt, orc, case)
    scenes = ss.scenes_of(pt, gpu, case)
    for kernel in (pt.KERNEL_WAVEFRONT, pt.KERNEL_SIMPLE):
        check_kernel(pt, gpu, scenes["host"], case, kernel, ref, f"{name}, host tree, kernel {kernel}")
    for tree, s in scenes.items():
        launches = check_kernel(pt, gpu, s, case, pt.KERNEL_WIDE, ref, f"{name}, {tree} tree, wide kernel")
        np.testing.assert_array_equal(ss.wide_work(launches), golden[f"{name}|{tree}"], err_msg=f"{name}, {tree} tree")
    assert ss.tree_sources(scenes) == (1, 2)


def test_cases_are_what_they_claim(pt, cases):
    lamb = pt.Preset("cornell", W, H).materials
    assert (lamb["type"] == 1).all() and (cases["bunny"][1]["type"] == 1).all()
    assert len(cases["bunny"][0]) == 5000
    assert sorted(set(cases["materials"][1]["type"][cases["materials"][0]["mat"]].tolist())) == [1, 2, 4]
    assert pt.PT_EMISSIVE in cases["lamp0"][1]["type"][cases["lamp0"][0]["mat"]]
    for name, zero_axes in ss.SLITS.items():
        c = pt.camera_to_array(cases[name][2])
        for a in zero_axes:
            assert c[3 + a] == c[a] and c[6 + a] == 0.0 and c[9 + a] == 0.0   # lower_left = origin, no extent


def test_lamp_lights_the_same_frame_in_every_kernel(pt, gpu, cases, golden):
    """An emitter of radiance (4, 3, 0.5) among Lambertian, metal and dielectric walls (no oracle: it
    absorbs at an emitter): the three kernels agree, and the wide kernel's compat work is the recorded one."""
    case = cases["lamp"]
    _, _, cam, w, h, spp, depth = case
    scenes = ss.scenes_of(pt, gpu, case)
    frames = {}
    for what, s, kernel in (("wavefront", scenes["host"], pt.KERNEL_WAVEFRONT), ("simple", scenes["host"], pt.KERNEL_SIMPLE),
                            ("wide", scenes["host"], pt.KERNEL_WIDE), ("wide/device", scenes["device"], pt.KERNEL_WIDE)):
        f = pt.Film(w, h, SEED, device=gpu)
        rgb, st = pt.render(s, f, cam, spp, depth, kernel=kernel, rng=pt.RNG_SAMPLE, chunk=CHUNK)
        launches = ss.compat_launches(pt, gpu, s, case, kernel)
        frames[what] = [(bits(rgb), st.rays, st.paths, None)] + [(bits(r), t.rays, t.paths, g) for r, t, g in launches]
        if kernel == pt.KERNEL_WIDE:
            tree = "device" if what.endswith("device") else "host"
            np.testing.assert_array_equal(ss.wide_work(launches), golden[f"lamp|{tree}"], err_msg=what)
    assert frames["wavefront"][0][0].view(np.float32).max() > 1.0   # the lamp is seen
    for what in ("simple", "wide", "wide/device"):
        for k, (a, b) in enumerate(zip(frames["wavefront"], frames[what])):
            np.testing.assert_array_equal(a[0], b[0], err_msg=f"{what}, frame {k}")
            assert a[1:3] == b[1:3] and a[2] == w * h * spp, (what, k)
            if a[3] is not None:
                np.testing.assert_array_equal(a[3], b[3], err_msg=f"{what}, states {k}")


@pytest.mark.parametrize("seed", [1, 0xFFFFFFFF])
def test_sample_streams_and_a_second_accumulating_launch(pt, orc, gpu, cases, seed):
    """Sample mode's stream is its definition: frames against the oracle's restatement for two seeds,
    and a second launch that accumulates on the same film (sampleBase > 0: the samples go on from the
    first launch's count)."""
    objs, mats, cam, w, h, _, depth = cases["cornell"]
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    c = pt.camera_to_array(cam)
    rows = np.arange(h, dtype=np.int32)
    spps = [3, 5]
    sums, base, rays = [], 0, []
    for spp in spps:
        _, s, ost = orc.render_sample_sums(objs, mats, nodes, c, w, h, rows, spp, depth, seed, CHUNK, sample_base=base,
                                           nthreads=8)
        sums.append(s)
        rays.append(ost.rays)
        base += spp
    want = orc.accumulate(sums, spps)
    plain, pst = orc.render_sample(objs, mats, nodes, c, w, h, rows, spps[0], depth, seed, CHUNK, nthreads=8)
    for tree, s in ss.scenes_of(pt, gpu, cases["cornell"]).items():
        for kernel in (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT, pt.KERNEL_SIMPLE):
            if tree == "device" and kernel != pt.KERNEL_WIDE:
                continue
            msg = f"seed {seed:#x}, {tree} tree, kernel {kernel}"
            f = pt.Film(w, h, seed, device=gpu)
            rgb, st = pt.render(s, f, cam, spps[0], depth, kernel=kernel, rng=pt.RNG_SAMPLE, chunk=CHUNK)
            np.testing.assert_array_equal(bits(rgb), bits(plain), err_msg=msg)
            assert (st.rays, st.paths) == (pst.rays, w * h * spps[0]), msg
            f = pt.Film(w, h, seed, device=gpu)
            for k, spp in enumerate(spps):
                rgb, st = pt.render(s, f, cam, spp, depth, kernel=kernel, rng=pt.RNG_SAMPLE, chunk=CHUNK, accumulate=True)
                np.testing.assert_array_equal(bits(rgb), bits(want[k]), err_msg=f"{msg}, accumulated frame {k}")
                assert (st.rays, st.paths) == (rays[k], w * h * spp), f"{msg}, accumulated frame {k}"
            assert f.accumulated == sum(spps)
