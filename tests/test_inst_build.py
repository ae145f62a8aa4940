"""CPU test of the instanced scene's host tree build (host/pt_instancing.cpp).

tests/cpp/inst_build_check.cpp (test infrastructure, built here with g++) runs
pt::buildInstancedTree, the pure part of an instanced scene's full build, on the shapes of
test_tree_shapes (tests/test_gpu_instance_update.py) -- a mesh that enters at its root (two
triangles), a re-braided one (a soup) and an instance of an empty mesh, under 1, 2, 9 and 65
instances of the first two -- and checks the two-level tree it returns: every (instance, mesh
primitive) pair reachable from slot 0 exactly once, the instance records, the top-level entries'
boxes around the fp64 world image of what lies below them, the layout for instance updates
(`dynamic`), the scalars, and that two builds of one input are byte-identical.
"""
import os
import subprocess

import numpy as np
import pytest

from helpers import tree_shape_instances, tree_shape_meshes, write_instanced_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "path-tracer-cuda-opengl_amd", "host")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("inst")
    exe = str(d / "inst_build_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "inst_build_check.cpp"), os.path.join(HOST, "pt_instancing.cpp"),
                    os.path.join(HOST, "pt_wide8.cpp"), "-o", exe], check=True)
    return exe, d


@pytest.fixture(scope="module")
def meshes():
    return tree_shape_meshes()


def run(harness, meshes, m, mesh, dynamic=False, rebraid=1, budget=0):
    exe, d = harness
    files = write_instanced_scene(d, meshes[0], meshes[1], m, mesh)
    return subprocess.run([exe, *files, str(int(dynamic)), str(rebraid), str(budget)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("knobs", [(0, 0), (1, 0), (3, 0), (1, 4)], ids=lambda k: "rebraid%d-entries%d" % k)
@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
@pytest.mark.parametrize("count", [1, 2, 9, 65])
def test_tree_shapes(harness, meshes, count, dynamic, knobs):
    m, mesh, _ = tree_shape_instances(count, seed=31)
    r = run(harness, meshes, m, mesh, dynamic, rebraid=knobs[0], budget=knobs[1])
    assert r.returncode == 0, r.stdout + r.stderr


def test_transform_classes(harness, meshes):
    """An identity, a translation and general matrices in one scene: the class dwords of their records."""
    m, mesh, _ = tree_shape_instances(9, seed=31)
    m[0] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    m[1] = [1, 0, 0, 5.5, 0, 1, 0, -7.25, 0, 0, 1, 3.0]
    r = run(harness, meshes, m, mesh, dynamic=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_singular_matrix(harness, meshes):
    m, mesh, _ = tree_shape_instances(9, seed=31)
    m[5] = 0.0
    r = run(harness, meshes, m, mesh)
    assert r.returncode == 3, r.stdout + r.stderr
    assert r.stdout.strip() == "rc 1: instanced scene: instance 5 has a singular transform"   # PT_ERR_INVALID


def test_only_empty_mesh_instances(harness, meshes):
    m, _, _ = tree_shape_instances(2, seed=31)
    r = run(harness, meshes, m, np.full(len(m), 2))
    assert r.returncode == 3, r.stdout + r.stderr
    assert r.stdout.strip() == "rc 6: instanced scene: no instance of a non-empty mesh"   # PT_ERR_STATE
