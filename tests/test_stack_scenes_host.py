"""The inputs of tests/test_gpu_render_stacks.py, host side (no GPU): the scenes of tests/stack_scenes.py
have the tree depths that select the traversal-stack sizes they are named for, the lighting rules have
teeth on their frames, and with the rules off the restatement that serves as their reference is the
oracle bit for bit.  Conditions on inputs, not tolerances; each test prints what it found
(tests/stack_scenes.py's docstring holds the table)."""
import numpy as np
import pytest

import many_lights
import pathloop
import pathloop_mis as pm
import pathloop_nee as pn
import stack_scenes as ss
import wide_tree
from pathloop import DEFAULT_SKY, SEED

RNGS = ("compat", "sample")
SCENES = tuple(ss.WIDE) + tuple(ss.BINARY)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def wide_depth(tmp_path, objects):
    """The host builder's (pt::buildWide8) depth, through tools/micro/wide_tree_check's build mode."""
    return wide_tree.build_host(tmp_path, wide_tree.write_objects(tmp_path, objects))[2]


# ---------------------------------------------------------------- 0. the gap these scenes close
def test_earlier_lit_scenes_select_the_smallest_kernels(orc, tmp_path):
    """Every scene with a pinned lit, NEE or MIS frame before these -- N1 (cornell_lit), N2, clamp / rim,
    open, the many-lights soup -- has a wide tree of depth <= 8 (the 8-entry wide kernels) and a binary
    tree of depth <= 23 (the 16- or 24-entry simple kernels)."""
    found = {}
    for sc in (pn.nee_scene("N1"), pn.nee_scene("N2"), pn.clamp_scene(), pm.open_scene(), many_lights.flat_scene()):
        found[sc.name] = (wide_depth(tmp_path, sc.objects), orc.bvh_depth(sc.nodes, len(sc.objects)))
    print("(wide depth, binary depth):", found)
    assert all(ss.wide_stack(w) == 8 and ss.bin_stack(b) <= 24 for w, b in found.values()), found


# ---------------------------------------------------------------- 1. depths
@pytest.mark.parametrize("name", list(ss.WIDE))
def test_wide_scene_selects_its_stack(tmp_path, name):
    sc = ss.scene(name)
    depth = wide_depth(tmp_path, sc.objects)
    lo, hi = ss.wide_interval(sc.stack)
    print(name, "objects", len(sc.objects), "wide depth", depth, "stack", ss.wide_stack(depth), "instanced depth",
          depth + 3, "stack", ss.wide_stack(depth + 3))
    assert lo <= depth <= hi and lo <= depth + 3 <= hi   # (an instance adds top level, marker and root)
    spheres = (sc.objects["type"] == 1).sum()
    assert (spheres > 0) == ss.WIDE[name][2] and set(sc.objects["type"]) <= {1, 3}
    if spheres:   # the generic kernels' scenes: every material on a sphere
        assert set(sc.materials["type"][sc.objects["mat"][sc.objects["type"] == 1]]) == {1, 2, 4}


@pytest.mark.parametrize("name", list(ss.BINARY))
def test_binary_scene_selects_its_stack(orc, name):
    sc = ss.scene(name)
    depth = orc.bvh_depth(sc.nodes, len(sc.objects))
    lo, hi = ss.bin_interval(sc.stack)
    print(name, "objects", len(sc.objects), "binary depth", depth, "stack", ss.bin_stack(depth))
    assert lo <= depth <= hi and ss.bin_stack(depth) == sc.stack


# ---------------------------------------------------------------- 2. teeth
def lit_terms(ref, kind):
    return sum(1 for w in ref["weights"] if w[0] == kind and (w[2] > 0).any())


@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("name", SCENES)
def test_the_rules_have_teeth(name, rng):
    """Per frame: at least 20 unoccluded light samples that add light, 20 occluded ones, 5 scatter rays
    that land on a sampled light (suppressed under NEE, weighted under MIS); the sphere scenes' paths go
    through glass and metal; the blind, lit, NEE and MIS frames all differ."""
    sc = ss.scene(name)
    ref = {m: ss.reference(name, m, rng)[0] for m in ss.MODES}
    nee, mis = ref["nee"], ref["mis"]
    print(name, rng, "rays lit / nee", ref["lit"]["rays"], nee["rays"], "events", nee["events"], "light terms > 0",
          lit_terms(nee, "light"), lit_terms(mis, "light"), "weighted emitter hits > 0", lit_terms(mis, "emitter"),
          "scatters by material type", nee["scattered"])
    for r in (nee, mis):
        e = r["events"]
        assert lit_terms(r, "light") >= 20 and e["direct_unoccluded"] >= 20 and e["direct_occluded"] >= 20
        assert e["emitter_suppressed"] >= 5
        assert e["clamped"] == 0
    assert lit_terms(mis, "emitter") >= 5
    assert not ref["lit"]["weights"] and ref["lit"]["events"] == dict.fromkeys(pn.EVENTS, 0)
    assert mis["events"] == nee["events"] and mis["rays"] == nee["rays"] > ref["lit"]["rays"]
    if name in ("S16", "S24") or name == "B24":
        for r in ref.values():
            assert r["scattered"].get(4, 0) > 0 and r["scattered"].get(2, 0) > 0   # glass and metal
    modes = list(ref)
    for i, a in enumerate(modes):
        for b in modes[i + 1:]:
            assert (bits(ref[a]["image"]) != bits(ref[b]["image"])).any(), (a, b)
    assert len(pn.light_list(sc.objects, sc.materials)[0]) >= 2


@pytest.mark.parametrize("name", list(ss.WIDE))
def test_the_two_launch_case_has_teeth(name):
    """Max depth 20, two NEE launches on one film: both frames add light and they differ.  (What the second
    launch of a film does differently at max depth > 16 depends on the launch, not on the paths' lengths:
    the open chains' longest path has a handful of bounces.)"""
    refs = ss.reference(name, "nee", "compat", max_depth=ss.LONG_DEPTH, frames=2, spp=ss.LONG_SPP)
    for r in refs:
        assert lit_terms(r, "light") >= 20 and r["events"]["direct_occluded"] >= 20
    print(name, "longest path of the first launch:", max(b for _, b in refs[0]["kinds"]), "bounces")
    assert (refs[0]["states"] != refs[1]["states"]).any()
    assert (bits(refs[0]["image"]) != bits(refs[1]["image"])).any()


# ---------------------------------------------------------------- 3. the reference with the rules off
@pytest.mark.parametrize("name", SCENES)
def test_nee_frames_are_pathloop_nees(name):
    """stack_scenes.reference renders through pathloop_mis; its NEE frame is pathloop_nee.render's."""
    sc = ss.scene(name)
    states = pn.orc.film_states(SEED, ss.W, range(ss.H))
    want = pn.render(sc.objects, sc.materials, sc.nodes, sc.camera, ss.W, ss.H, range(ss.H), ss.SPP, ss.DEPTH, states,
                     sky=sc.sky, nee=True)
    got = ss.reference(name, "nee", "compat")[0]
    np.testing.assert_array_equal(bits(got["image"]), bits(want["image"]))
    np.testing.assert_array_equal(got["states"], want["states"])
    assert got["rays"] == want["rays"] and got["events"] == want["events"]


@pytest.mark.parametrize("name", SCENES)
def test_rules_off_is_the_oracle(orc, name):
    """The blind frames (emitters Lambertian, default sky) are orc.render / orc.render_sample bit for
    bit: image, streams, rays.  The lit frames differ from them by the two rules of pathloop.py only."""
    sc = ss.scene(name)
    states = orc.film_states(SEED, ss.W, range(ss.H))
    mine = ss.reference(name, "blind", "compat")[0]
    ref, rst = orc.render(sc.objects, sc.blind_materials, sc.nodes, sc.camera, ss.W, ss.H, range(ss.H), ss.SPP, ss.DEPTH,
                          states)   # advances states
    np.testing.assert_array_equal(bits(mine["image"]), bits(ref))
    np.testing.assert_array_equal(mine["states"], states)
    assert mine["rays"] == rst.rays and mine["paths"] == rst.paths == ss.W * ss.H * ss.SPP
    smine = ss.reference(name, "blind", "sample")[0]
    sref, srst = orc.render_sample(sc.objects, sc.blind_materials, sc.nodes, sc.camera, ss.W, ss.H, range(ss.H),
                                   ss.SAMPLE_SPP, ss.DEPTH, SEED, chunk=ss.SAMPLE_CHUNK)
    np.testing.assert_array_equal(bits(smine["image"]), bits(sref))
    assert smine["rays"] == srst.rays and smine["paths"] == srst.paths


def test_flagged_frames_without_lights_are_the_blind_ones():
    """nee / mis on the blind materials: no sampled light, so the flags change nothing."""
    sc = ss.scene("S16")
    states = pn.orc.film_states(SEED, ss.W, range(ss.H))
    a = pm.render(sc.objects, sc.blind_materials, sc.nodes, sc.camera, ss.W, ss.H, range(ss.H), ss.SPP, ss.DEPTH, states,
                  sky=DEFAULT_SKY, mis=True)
    b = ss.reference("S16", "blind", "compat")[0]
    np.testing.assert_array_equal(bits(a["image"]), bits(b["image"]))
    assert pathloop.EMITTER not in {k for k, _ in b["kinds"]}
