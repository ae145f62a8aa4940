"""CPU test of the wide render kernels' deferred leaf-box rule (triangle-only scenes).

tests/cpp/wide8_deferred_check.cpp (test infrastructure, built here with g++, the recipe of
test_wide_builder.py) traces rays through scalar restatements of the render kernels' new loop
(wideTestTri: plain minimum of (t, rank) and the second-smallest distance t2) with the SHADE step's
single box test of the final hit (deferredRedo), and of the per-candidate rule the sphere scenes
keep (wideTest).  Every ray the new rule decides (no `redo`) must give the oracle's reference-order
closest hit bit for bit, object and t; `redo` rays are re-traced by the kernels in the reference's
order (tests/test_gpu_deferred_leafbox.py covers that path).  Where both rules decide they agree.
"""
import os
import subprocess

import numpy as np
import pytest

from helpers import random_rays, random_soup
from wall_box import wall_box, wall_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("w8d")
    exe = str(d / "wide8_deferred_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "path-tracer-cuda-opengl_amd", "host"),
                    os.path.join(ROOT, "tests", "cpp", "wide8_deferred_check.cpp"),
                    os.path.join(ROOT, "path-tracer-cuda-opengl_amd", "host", "pt_wide8.cpp"),
                    "-L", os.path.join(ROOT, "oracle"), "-loracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
                    "-o", exe], check=True)
    return exe, d


def run(harness, objs, rays):
    exe, d = harness
    objs = np.ascontiguousarray(objs)
    ob, rb, out = str(d / "o.bin"), str(d / "r.bin"), str(d / "out.bin")
    objs.tofile(ob)
    np.ascontiguousarray(rays, np.float32).tofile(rb)
    r = subprocess.run([exe, ob, rb, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = np.fromfile(out, np.float32).reshape(-1, 6)
    new = res[:, 0].astype(np.int64), res[:, 1], res[:, 2] != 0
    old = res[:, 3].astype(np.int64), res[:, 4], res[:, 5] != 0
    return new, old


def compare(orc, harness, objs, rays, max_redo):
    """test_wide_builder.py's compare() for the new rule; returns (redo count, rays hit)."""
    (leaf, t, redo), (oleaf, ot, oredo) = run(harness, objs, rays)
    keys = orc.morton_keys(objs)
    obj = np.where(leaf >= 0, (keys[np.maximum(leaf, 0)] & 0xffffffff).astype(np.int64), -1)
    ref, _ = orc.trace(objs, orc.build_lbvh(objs, keys, tight=True), rays)
    ok = ~redo
    np.testing.assert_array_equal(obj[ok], np.where(ref["hit"] == 1, ref["obj"], -1)[ok])
    h = ok & (ref["hit"] == 1)
    np.testing.assert_array_equal(t[h].view(np.uint32), ref["t"][h].view(np.uint32))
    # the old rule's answers, wherever both rules decide
    both = ~redo & ~oredo
    np.testing.assert_array_equal(leaf[both], oleaf[both])
    bh = both & (leaf >= 0)
    np.testing.assert_array_equal(t[bh].view(np.uint32), ot[bh].view(np.uint32))
    print(f"rays {len(rays)} hit {int((ref['hit'] == 1).sum())} redo new {int(redo.sum())} old {int(oredo.sum())}")
    if max_redo is not None:
        assert redo.mean() <= max_redo, (redo.mean(), int(redo.sum()))
    return int(redo.sum()), int((ref["hit"] == 1).sum())


@pytest.mark.parametrize("name", ["cornell", "bunny_cornell", "triangle_world"])
def test_deferred_rule_presets(pt, orc, harness, name):
    p = pt.Preset(name)
    # triangle_world also holds spheres (295 of its 601 objects), and a scene with spheres keeps the
    # per-candidate rule: its 306 triangles alone are the triangle-only input here
    objects = p.objects[p.objects["type"] == 3]
    assert len(objects) == len(p.objects) or name == "triangle_world"
    p.objects = objects
    lo, hi = p.objects["v"][:, :3].min(0), p.objects["v"][:, :3].max(0)
    center = np.clip((lo + hi) / 2, -1e3, 1e3)
    radius = float(min(np.linalg.norm(hi - lo), 3000.0)) * 0.75 + 1.0
    rays = random_rays(4096, seed=2, center=center, radius=radius, objects=p.objects)
    compare(orc, harness, p.objects, rays, max_redo=0.001)


@pytest.mark.parametrize("seed", [0, 1])
def test_deferred_rule_soup_and_exact_duplicates(orc, harness, seed):
    objs, _ = random_soup(1500, 0, seed=seed)
    compare(orc, harness, objs, random_rays(4096, seed=seed + 20, objects=objs), max_redo=0.001)
    dup = np.concatenate([objs, objs, objs])   # exact ties: identical copies
    dup = dup[np.random.default_rng(seed).permutation(len(dup))]
    compare(orc, harness, dup, random_rays(4096, seed=seed + 30, objects=dup), max_redo=0.01)


def test_deferred_rule_wall_box_grazing_finals(orc, harness):
    """Rays from wall to wall: about half of the final hits graze their flat box (t < lo), and
    alone in their window they are decided without a redo."""
    objs, _ = wall_box()
    redo, hit = compare(orc, harness, objs, wall_rays(4096, seed=3), max_redo=0.001)
    assert hit > 3000


def test_deferred_rule_doubled_walls_fire_the_window(orc, harness):
    """Every wall twice: a grazing final hit has its twin at the same t, inside its window, so the
    window branch must fire (exempt from the redo cap); the decided rays still equal the reference."""
    objs, _ = wall_box(doubled=True)
    redo, hit = compare(orc, harness, objs, wall_rays(4096, seed=3), max_redo=None)
    assert redo > 0 and hit > 3000


@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_deferred_rule_tiny_scenes(orc, harness, n):
    objs, _ = random_soup(n, 0, seed=n)
    compare(orc, harness, objs, random_rays(1024, seed=n, objects=objs), max_redo=0.01)
