"""The wide sample kernels that draw scatter vectors one bounce ahead (renderKernelWF<.., AHEAD>) on the GPU.

A triangle-only flat scene without a metal or dielectric material, a pinhole camera, sample mode and no
light sampling select them; PT_SHADE_AHEAD=0 launches the kernels without the slot on the same scene.
A sample's stream is read by the unit-sphere loop alone there, so the k-th accepted vector is the k-th
scatter's whenever it is drawn, and nothing may differ: f32 pixels, rays and paths are compared bit for
bit between the two knob values and with the oracle's sample-mode restatement.  The knob is read when
a launch is enqueued, so each value is recorded by a child process of its own (tests/shade_ahead_scenes.py
lists the cases), once per session, with PT_KERNEL_LOG=1: the library names the instantiation of every
launch on stderr, and the eligible cases must name an AHEAD kernel under knob 1 and its twin under knob 0
-- a selection that is never taken fails here -- while the fallback cases name one kernel under both.

Node visits and primitive tests are not compared: in sample mode which lanes share a wave varies from
run to run (tests/test_gpu_tri_kernels.py notes the same).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  before libpt.so loads (the two must share torch's HIP runtime)

import pathloop
import pathloop_nee
import shade_ahead_scenes as sa

pytestmark = pytest.mark.gpu

RAYS, PATHS = range(2)
KERNEL = re.compile(r"^\[pt\] kernel (\S.*)$")


def parse_log(text):
    """{case: [instantiation per launch]} from the recorder's stderr."""
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("[case] "):
            cur = line[len("[case] "):].strip()
            out[cur] = []
        elif cur is not None and KERNEL.match(line):
            out[cur].append(KERNEL.match(line).group(1))
    return out


@pytest.fixture(scope="module")
def recorded(gpu, tmp_path_factory):
    """{knob: (arrays, {case: kernels})}: shade_ahead_scenes.record() under PT_SHADE_AHEAD=1 and =0."""
    out = {}
    d = tmp_path_factory.mktemp("shade_ahead")
    for knob in ("1", "0"):
        path = str(d / f"shade_ahead_{knob}.npz")
        r = subprocess.run([sys.executable, os.path.abspath(sa.__file__), path],
                           env=dict(os.environ, PT_SHADE_AHEAD=knob, PT_KERNEL_LOG="1"), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, f"PT_SHADE_AHEAD={knob}: {r.stdout[-1000:]}\n{r.stderr[-3000:]}"
        with np.load(path) as z:
            out[knob] = ({k: z[k] for k in z.files}, parse_log(r.stderr))
    return out


@pytest.fixture(scope="module")
def cases(pt):
    return sa.cases(pt)


def oracle_launches(pt, orc, case):
    """[(rgb, rays)] per launch of the case: the oracle's sample-mode frames (accumulating launches resolved
    as pt_render_ex does)."""
    objs, mats = case["objs"], case["mats"]
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    c = pt.camera_to_array(case["cam"])
    parts = case.get("parts", (1, 0))
    rows = pt.Film(case["w"], case["h"], case["seed"], n_parts=parts[0], part=parts[1]).rows
    w, h, depth, seed = case["w"], case["h"], case["depth"], case["seed"]
    if not case["launches"][0][2]:
        (spp, chunk, _), = case["launches"]
        rgb, st = orc.render_sample(objs, mats, nodes, c, w, h, rows, spp, depth, seed, chunk, nthreads=8)
        return [(rgb, st.rays)]
    sums, rays, base = [], [], 0
    for spp, chunk, _ in case["launches"]:
        _, s, st = orc.render_sample_sums(objs, mats, nodes, c, w, h, rows, spp, depth, seed, chunk, sample_base=base,
                                          nthreads=8)
        sums.append(s)
        rays.append(st.rays)
        base += spp
    return list(zip(orc.accumulate(sums, [l[0] for l in case["launches"]]), rays))


def assert_knobs_equal(recorded, name, case):
    on, off = recorded["1"][0], recorded["0"][0]
    for k, (spp, _, _) in enumerate(case["launches"]):
        msg = f"{name}, launch {k}"
        a, b = on[f"{name}|{k}|n"], off[f"{name}|{k}|n"]
        print(msg, "rays, paths", a.tolist(), b.tolist())
        np.testing.assert_array_equal(on[f"{name}|{k}|rgb"], off[f"{name}|{k}|rgb"], err_msg=msg)
        assert a.tolist() == b.tolist(), msg
        assert a[PATHS] == len(on[f"{name}|{k}|rgb"]) * spp and a[RAYS] >= a[PATHS], msg


def assert_equals_pathloop(recorded, name, ref):
    """Both knob values' one launch against a pathloop / pathloop_nee sample-mode reference."""
    for knob in ("1", "0"):
        rec = recorded[knob][0]
        msg = f"{name}, knob {knob}"
        np.testing.assert_array_equal(rec[f"{name}|0|rgb"], np.ascontiguousarray(ref["image"]).view(np.uint32), err_msg=msg)
        assert rec[f"{name}|0|n"].tolist() == [ref["rays"], ref["paths"]], msg


@pytest.mark.parametrize("name", sa.ELIGIBLE)
def test_ahead_kernels_equal_their_twins_and_the_oracle(pt, orc, recorded, cases, name):
    case = cases[name]
    assert_knobs_equal(recorded, name, case)
    # teeth: the two logs name different instantiations, an AHEAD kernel and its twin, for every launch
    stack, lit = sa.STACK_LIT[name]
    twin = f"renderKernelWF<{stack}, true, true, false, {'true' if lit else 'false'}, false, false, true, "
    on, off = recorded["1"][1][name], recorded["0"][1][name]
    print(name, on, off)
    assert on == [twin + "true>"] * len(case["launches"]), name
    assert off == [twin + "false>"] * len(case["launches"]), name
    assert recorded["1"][0][f"{name}|tree"][0] == (2 if case.get("device") else 1)
    if name == "lit":   # (an emitter that shines: oracle/ absorbs there; the render loop restated in Python)
        ref = pathloop.lit_reference_sample("L1")
        assert_equals_pathloop(recorded, name, ref)
        assert recorded["1"][0][f"{name}|0|rgb"].view(np.float32).max() > 1.0   # the lamp is seen
        return
    ref = oracle_launches(pt, orc, case)
    for knob in ("1", "0"):
        rec = recorded[knob][0]
        for k, (rgb, rays) in enumerate(ref):
            msg = f"{name}, knob {knob}, launch {k}"
            np.testing.assert_array_equal(rec[f"{name}|{k}|rgb"], np.ascontiguousarray(rgb).view(np.uint32), err_msg=msg)
            assert int(rec[f"{name}|{k}|n"][RAYS]) == rays, msg


@pytest.mark.parametrize("name", sa.FALLBACKS)
def test_fallbacks_take_one_kernel_under_both_knob_values(pt, orc, recorded, cases, name):
    case = cases[name]
    assert_knobs_equal(recorded, name, case)
    on, off = recorded["1"][1][name], recorded["0"][1][name]
    print(name, on, off)
    assert on == off and len(on) == len(case["launches"]), name
    assert all(k.startswith("renderKernelWF<") and k.endswith(", false>") for k in on), on
    if name == "nee":   # NEE on the lit box: the restatement with the rule of include/pt.h
        assert on[0] == "renderKernelWF<8, true, true, false, true, true, false, true, false>"
        assert_equals_pathloop(recorded, name, pathloop_nee.nee_reference_sample("N1"))
        assert (recorded["1"][0]["nee|0|rgb"] != recorded["1"][0]["lit|0|rgb"]).any()   # (the rule was on)
        return
    if name == "instanced":   # one identity instance: the flat Cornell box's frame, so d50s5's oracle frame
        assert on[0] == "renderKernelWF<8, true, true, true, false, false, false, false, false>"
        case = cases["d50s5"]
    else:
        assert on[0] == "renderKernelWF<8, true, true, false, false, false, false, true, false>"
    ref = oracle_launches(pt, orc, case)
    for knob in ("1", "0"):
        rec = recorded[knob][0]
        np.testing.assert_array_equal(rec[f"{name}|0|rgb"], np.ascontiguousarray(ref[0][0]).view(np.uint32), err_msg=name)
        assert int(rec[f"{name}|0|n"][RAYS]) == ref[0][1], name


def test_cases_are_what_they_claim(pt, recorded, cases):
    for name in sa.ELIGIBLE:
        c = cases[name]
        used = set(c["mats"]["type"][c["objs"]["mat"]].tolist())
        assert used <= {1, pt.PT_EMISSIVE} and (c["objs"]["type"] == 3).all() and c["cam"].lens_radius == 0.0, name
    assert 2 in cases["metal"]["mats"]["type"] and 4 in cases["glass"]["mats"]["type"]
    assert cases["lens"]["cam"].lens_radius > 0.0
    assert len(cases["bunny"]["objs"]) == 5000
    assert pt.PT_EMISSIVE in cases["lit"]["mats"]["type"] and pt.PT_EMISSIVE in cases["lamp0"]["mats"]["type"]
    assert cases["nee"]["objs"] is cases["lit"]["objs"] and cases["nee"]["nee"]
    ip = pt.InstancedPreset("cornell", sa.W, sa.H)   # the instanced case: d50s5's camera and one instance
    assert bytes(ip.camera) == bytes(cases["d50s5"]["cam"]) and len(ip.instances) == 1
    assert (cases["lamp0"]["mats"]["albedo"][cases["lamp0"]["mats"]["type"] == pt.PT_EMISSIVE] == 0).all()
    assert cases["tiny"]["w"] * cases["tiny"]["h"] < 64
    depth = {n: int(recorded["1"][0][f"{n}|tree"][1]) for n in sa.ELIGIBLE}
    assert 8 < depth["chain16"] <= 16 and all(d <= 8 for n, d in depth.items() if n != "chain16"), depth
    # at max_depth 1 and 2 a path traces at most that many rays: every scattering path ends out of bounces
    for d in (1, 2):
        n = recorded["1"][0][f"d{d}s5|0|n"]
        assert n[RAYS] <= d * n[PATHS]
    # the two film parts are the two halves of the frame's rows
    assert len(recorded["1"][0]["part0|0|rgb"]) + len(recorded["1"][0]["part1|0|rgb"]) == sa.W * sa.H
