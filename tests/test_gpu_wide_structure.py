"""The wide trees the device builds, checked as trees.

tests/test_gpu_wide.py and its neighbours judge a device-built tree by the hits of random rays; a
plane that keeps less than the outward margin, a box that is wrong in a rarely taken branch, an
understated depth or a leaf range referenced twice would pass them.  Here every builder's arrays
are read back (pt_scene_download_wide) and walked by tools/micro/wide_tree_check
(tests/cpp/wide_tree_checks.hpp: the checks tests/test_wide_tree_check.py shows to reject damaged
trees), at the sizes where the builders change their code path: the leaf group size, one wide
node, kWaveTask = 64, kChunk = 2,048 (above it a task's blocks merge their bins in global memory)
and, for PLOC, kTailMax = 16,384 (above it the multi-pass clustering runs).  The record arrays that
do not depend on the builder are compared byte for byte with a host-built scene of the same
objects.  An instanced scene's top level, rebuilt on the device after pt_scene_update_instances, is
walked by tools/micro/inst_build_check against the new matrices.  Nothing is rendered.

Every check is exact; a failure is a finding about the builder named in the test id."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  before libpt.so loads (the two must share torch's HIP runtime)

import wide_tree as wt
from helpers import (OBJECT_DTYPE, MATERIAL_DTYPE, random_soup, tree_shape_instances, tree_shape_meshes,
                     write_instanced_scene)
from test_gpu_dynamic import moved
from test_gpu_wide import edge_scene, tie_scene
from tri_kernel_scenes import hidden_sphere_scene, replacement_triangle, was_sphere_objects

pytestmark = pytest.mark.gpu

BUILDERS = ["host", "device", "device_ploc"]
SIZES = [1, 2, 3, 4, 8, 9, 25, 64, 65, 2048, 2049, 4097, 6145]
PLOC_SIZES = [16384, 16385, 20000]
INST_CHECK = os.path.join(wt.REPO, "tools", "micro", "inst_build_check")


def select(pt, monkeypatch, builder):
    """The builder of the scenes made from here on (tests/test_gpu_wide.py's `wb`); returns the build flags."""
    if builder == "device_ploc":
        monkeypatch.setenv("PT_WIDE_DEVICE_BUILDER", "ploc")
    else:
        monkeypatch.delenv("PT_WIDE_DEVICE_BUILDER", raising=False)
    if builder == "host":
        monkeypatch.setenv("PT_WIDE_BUILD", "host")   # (an updated scene would otherwise build on the device)
    else:
        monkeypatch.delenv("PT_WIDE_BUILD", raising=False)
    return pt.PT_BVH_ORIGIN_BOUNDS | (pt.PT_BVH_WIDE_DEVICE if builder != "host" else 0)


def dev_slots(n):
    """pt::wideDevNodeSlots: the node slots a device build may use."""
    return 1 + 8 * ((n - 1 if n > 1 else 0) // 7 + 1)


def arrays_of(pt, s):
    a = {k: s.download_wide(k) for k in (pt.WIDE_NODES, pt.WIDE_PRIMS, pt.WIDE_SHADE, pt.WIDE_BOXES, pt.WIDE_RANKS,
                                         pt.WIDE_EDGE_PRIMS, pt.WIDE_INSTANCES)}
    a["info"] = s.wide_info()
    return a


def assert_structure(pt, tmp, objs, a, builder):
    """The downloaded tree passes the structural checker."""
    info, n = a["info"], len(objs)
    assert info["source"] == (1 if builder == "host" else 2)
    assert a[pt.WIDE_NODES].shape == (info["slots"], wt.NODE_DWORDS) and a[pt.WIDE_PRIMS].shape == (n, 12)
    assert a[pt.WIDE_SHADE].shape == (n, 12) and a[pt.WIDE_BOXES].shape == (n, 8) and a[pt.WIDE_RANKS].shape == (n,)
    assert len(a[pt.WIDE_INSTANCES]) == 0
    rc, out = wt.run_check(tmp, wt.write_objects(tmp, objs), a[pt.WIDE_NODES], a[pt.WIDE_PRIMS], info["depth"],
                           info["slots"], wt.HOST_CAPACITY if builder == "host" else dev_slots(n))
    assert rc == 0, f"{builder}, n = {n}: {out}"
    assert f"n {n} " in out and "failures 0" in out, out


def assert_edge_form(pt, a, ever_sphere):
    """PT_WIDE_EDGE_PRIMS against pt::edgeTriRecords' rule on the same scene's PT_WIDE_PRIMS."""
    prims, edges = a[pt.WIDE_PRIMS], a[pt.WIDE_EDGE_PRIMS]
    if ever_sphere:
        assert edges.size == 0   # only a scene that never held a sphere has the array
        return
    assert edges.shape == prims.shape
    f = prims.view(np.float32)
    want = prims.copy()
    want.view(np.float32)[:, 4:7] = f[:, 4:7] - f[:, 0:3]      # one IEEE fp32 subtraction per component
    want.view(np.float32)[:, 8:11] = f[:, 8:11] - f[:, 0:3]
    np.testing.assert_array_equal(edges, want)                 # (dwords 3, 7, 11 copied)


def assert_records_equal(pt, dev, host):
    """What does not depend on the builder, byte for byte against the host-built scene's."""
    np.testing.assert_array_equal(dev[pt.WIDE_RANKS], host[pt.WIDE_RANKS], err_msg="ranks")
    np.testing.assert_array_equal(dev[pt.WIDE_SHADE], host[pt.WIDE_SHADE], err_msg="shading records")
    hp, dp = host[pt.WIDE_PRIMS], dev[pt.WIDE_PRIMS]
    hs, ds = hp[np.argsort(hp[:, 3], kind="stable")], dp[np.argsort(dp[:, 3], kind="stable")]
    np.testing.assert_array_equal(ds, hs, err_msg="primitive records by rank")
    tri = hs[hs[:, 11] == 0, 3]   # ranks of the triangle records (a sphere's box record is nobody's input)
    np.testing.assert_array_equal(dev[pt.WIDE_BOXES].view(np.uint32)[tri], host[pt.WIDE_BOXES].view(np.uint32)[tri],
                                  err_msg="exact boxes")


@pytest.fixture(scope="module")
def host_arrays(pt, gpu):
    """name -> the arrays of a host-built scene (source 1) of the objects: built once per scene."""
    made = {}

    def get(name, objs, mats):
        if name not in made:
            assert os.environ.get("PT_WIDE_BUILD", "host") == "host"
            s = pt.Scene(objs, mats, device=gpu, flags=pt.PT_BVH_ORIGIN_BOUNDS)
            made[name] = arrays_of(pt, s)
            assert made[name]["info"]["source"] == 1
        return made[name]
    return get


def check_scene(pt, gpu, monkeypatch, tmp, host_arrays, builder, name, objs, mats):
    flags = select(pt, monkeypatch, builder)
    s = pt.Scene(objs, mats, device=gpu, flags=flags)
    a = arrays_of(pt, s)
    assert_structure(pt, tmp, objs, a, builder)
    assert_edge_form(pt, a, bool((objs["type"] == pt.PT_SPHERE).any()))
    if builder != "host":
        monkeypatch.delenv("PT_WIDE_BUILD", raising=False)
        assert_records_equal(pt, a, host_arrays(name, objs, mats))
    return a


def soup(n):
    return random_soup(n - n // 4, n // 4, seed=100 + n)


@pytest.mark.parametrize("builder,n", [(b, n) for b in BUILDERS for n in SIZES] + [("device_ploc", n) for n in PLOC_SIZES])
def test_random_soups(pt, gpu, monkeypatch, tmp_path, host_arrays, builder, n):
    objs, mats = soup(n)
    check_scene(pt, gpu, monkeypatch, tmp_path, host_arrays, builder, f"soup{n}", objs, mats)


def identical_objects(pt):
    """tests/test_gpu_dynamic.py test_wide_device_identical_objects: every centroid and every distance ties."""
    objs, mats = random_soup(1, 1, seed=50, n_mat=4)
    rep = np.concatenate([np.repeat(objs[:1], 5000), np.repeat(objs[1:2], 3000)])
    rep["mat"] = np.arange(len(rep)) % 4
    return rep, mats


def flat_triangles():
    """Triangles in the plane z = 0: a zero-extent axis (the planes' e = emin branch)."""
    objs, mats = random_soup(900, 0, seed=77)
    objs["v"][:, [2, 5, 8]] = 0.0
    return objs, mats


def edge(kind):
    return edge_scene(kind)[:2]


SCENES = {
    "identical": identical_objects,
    "tripled": lambda pt: tie_scene(),
    "tiny": lambda pt: edge("tiny"), "huge": lambda pt: edge("huge"), "degenerate": lambda pt: edge("degenerate"),
    "one_point": lambda pt: edge("one_point"), "ground": lambda pt: edge("ground"), "slivers": lambda pt: edge("slivers"),
    "flat_z0": lambda pt: flat_triangles(),
    "cornell": lambda pt: (pt.Preset("cornell").objects, pt.Preset("cornell").materials),
    "bunny_cornell": lambda pt: (pt.Preset("bunny_cornell").objects, pt.Preset("bunny_cornell").materials),
    "rtiow": lambda pt: (pt.Preset("rtiow").objects, pt.Preset("rtiow").materials),
}


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("builder", BUILDERS)
def test_ties_edges_and_presets(pt, gpu, monkeypatch, tmp_path, host_arrays, builder, name):
    objs, mats = SCENES[name](pt)
    check_scene(pt, gpu, monkeypatch, tmp_path, host_arrays, builder, name, objs, mats)


@pytest.mark.parametrize("builder", ["device", "device_ploc"])
def test_rebuilds_reuse_the_scratch(pt, gpu, monkeypatch, tmp_path, host_arrays, builder):
    """6,145 objects moved and rebuilt twice in place: every rebuild's arrays pass on their own."""
    flags = select(pt, monkeypatch, builder)
    objs0, mats = soup(6145)
    s = pt.Scene(objs0, mats, device=gpu, flags=flags)
    for frame in (1, 2):
        objs = moved(pt, objs0, frame, np.random.default_rng(60 + frame))
        s.update_objects(objs)
        with pytest.raises(pt.PtError):   # stale until the build
            s.download_wide(pt.WIDE_NODES)
        s.build_bvh(flags)
        a = arrays_of(pt, s)
        assert_structure(pt, tmp_path, objs, a, builder)
        assert_edge_form(pt, a, True)
        assert_records_equal(pt, a, host_arrays(f"moved{frame}", objs, mats))


@pytest.mark.parametrize("builder", BUILDERS)
def test_scene_that_once_held_a_sphere(pt, gpu, monkeypatch, tmp_path, host_arrays, builder):
    """tests/tri_kernel_scenes.py `was_sphere`: the sphere overwritten by a triangle.  The tree is the
    triangle scene's; the edge-form records stay absent (hasSpheres is sticky)."""
    flags = select(pt, monkeypatch, builder)
    before, mats = hidden_sphere_scene()
    s = pt.Scene(before, mats, device=gpu, flags=flags)
    s.update_objects(replacement_triangle(), first=len(before) - 1)
    s.build_bvh(flags)
    objs, _ = was_sphere_objects()
    a = arrays_of(pt, s)
    assert_structure(pt, tmp_path, objs, a, builder)
    assert_edge_form(pt, a, True)
    monkeypatch.delenv("PT_WIDE_BUILD", raising=False)
    fresh = host_arrays("was_sphere", objs, mats)
    assert_records_equal(pt, a, fresh)
    assert_edge_form(pt, fresh, False)   # (a scene of these objects that never held the sphere has them)


def test_download_returns_what_the_host_build_wrote(pt, gpu, monkeypatch, tmp_path):
    """The download itself: a host-built tree's nodes and primitive records equal, byte for byte, what
    pt::buildWide8 produces for the scene in the checker's build mode; and the call's contract."""
    import ctypes as C
    select(pt, monkeypatch, "host")
    objs, mats = soup(4097)
    s = pt.Scene(objs, mats, device=gpu, flags=pt.PT_BVH_ORIGIN_BOUNDS)
    assert s.wide_info()["source"] == 0          # not built yet: the download builds it, like a wide query
    nodes = s.download_wide(pt.WIDE_NODES)
    info = s.wide_info()
    assert info["source"] == 1
    want_nodes, want_prims, depth, slots = wt.build_host(tmp_path, wt.write_objects(tmp_path, objs))
    assert (info["depth"], info["slots"]) == (depth, slots)
    np.testing.assert_array_equal(nodes, want_nodes)
    np.testing.assert_array_equal(s.download_wide(pt.WIDE_PRIMS), want_prims)
    # size only; a capacity below the size writes nothing; an absent array has 0 bytes
    size = C.c_int64(-1)
    assert pt.lib.pt_scene_download_wide(s.h, pt.WIDE_RANKS, None, 0, C.byref(size)) == 0 and size.value == 4 * len(objs)
    buf = np.full(len(objs), 0xdeadbeef, np.uint32)
    size.value = -1
    assert pt.lib.pt_scene_download_wide(s.h, pt.WIDE_RANKS, buf.ctypes.data, buf.nbytes - 1, C.byref(size)) == 1
    assert size.value == 4 * len(objs) and (buf == 0xdeadbeef).all()
    assert pt.lib.pt_scene_download_wide(s.h, pt.WIDE_RANKS, buf.ctypes.data, buf.nbytes, None) == 0
    np.testing.assert_array_equal(np.sort(buf), np.arange(len(objs)))
    for absent in (pt.WIDE_EDGE_PRIMS, pt.WIDE_INSTANCES):
        size.value = -1
        assert pt.lib.pt_scene_download_wide(s.h, absent, buf.ctypes.data, buf.nbytes, C.byref(size)) == 0
        assert size.value == 0
    assert pt.lib.pt_scene_download_wide(s.h, 7, buf.ctypes.data, buf.nbytes, C.byref(size)) == 1
    unbuilt = pt.Scene(objs, mats, device=gpu, build=False)
    assert pt.lib.pt_scene_download_wide(unbuilt.h, pt.WIDE_NODES, None, 0, C.byref(size)) == 6   # PT_ERR_STATE
    assert size.value == 0
    empty = pt.Scene(np.zeros(0, OBJECT_DTYPE), np.zeros(1, MATERIAL_DTYPE), device=gpu)
    assert all(empty.download_wide(k).size == 0 for k in range(7))


# ------------------------------------------------------------------ the instanced top level
def run_inst_check(tmp, files, nodes, winst, info, mode):
    assert os.path.exists(INST_CHECK), "tools/micro/inst_build_check not built (make -C path-tracer-cuda-opengl_amd)"
    nb, wb = os.path.join(str(tmp), f"{mode}_nodes.bin"), os.path.join(str(tmp), f"{mode}_winst.bin")
    nodes.tofile(nb)
    winst.tofile(wb)
    r = subprocess.run([INST_CHECK, *files, "1", "1", "0", nb, wb, str(info["depth"]), str(info["slots"]), mode],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"slots (\d+) top (\d+) entries (\d+) depth (\d+) .*failures 0", r.stdout)
    assert m, r.stdout
    return int(m.group(2))


@pytest.mark.parametrize("count", [1, 2, 9, 65, 600])
def test_instanced_top_level_rebuilt_on_the_device(pt, gpu, monkeypatch, tmp_path, count):
    """tests/test_gpu_instance_update.py test_tree_shapes' scenes, laid out for updates: the full build's
    arrays are the host build's; after update_instances and a rebuild (twice: the scratch is reused)
    the mesh trees are untouched and the top level passes the host build's walk against the new
    matrices -- every entry once, no leaf child, slots inside the region, the records' class dwords,
    mesh roots and rows, each entry's decoded box around the fp64 world image below it with the
    top level's margin -- and the reported depth and slots are the walk's."""
    for knob in ("PT_INST_REBRAID", "PT_INST_ENTRIES", "PT_WIDE_DEVICE_BUILDER"):
        monkeypatch.delenv(knob, raising=False)
    meshes, mats = tree_shape_meshes()
    world = np.concatenate(meshes)
    mcount = np.array([len(m) for m in meshes], np.int64)
    mfirst = np.concatenate([[0], np.cumsum(mcount)[:-1]]).astype(np.int64)

    def instances(seed):
        m, mesh, _ = tree_shape_instances(count, seed)
        inst = np.zeros(len(m), pt.INSTANCE_DTYPE)
        inst["m"] = m
        inst["mesh"] = mesh
        return inst, m, mesh

    inst, m, mesh = instances(31)
    s = pt.Scene.instanced(world, mfirst, mcount, inst, mats, device=gpu, flags=pt.PT_BVH_WIDE_DEVICE)
    info = s.wide_info()
    assert info["source"] == 3
    nodes, winst = s.download_wide(pt.WIDE_NODES), s.download_wide(pt.WIDE_INSTANCES)
    assert nodes.shape == (info["slots"], wt.NODE_DWORDS) and winst.shape == (len(inst), 16)
    assert s.download_wide(pt.WIDE_PRIMS).shape == (max(1, len(world)), 12)
    assert all(s.download_wide(k).size == 0 for k in (pt.WIDE_BOXES, pt.WIDE_RANKS, pt.WIDE_EDGE_PRIMS))
    top_cap = run_inst_check(tmp_path, write_instanced_scene(tmp_path, meshes, mats, m, mesh), nodes, winst, info, "full")

    second, m2, _ = instances(32)
    files2 = write_instanced_scene(tmp_path, meshes, mats, m2, mesh)
    sources = []
    for _ in range(3):
        s.update_instances(second)
        with pytest.raises(pt.PtError):   # stale until the build
            s.download_wide(pt.WIDE_NODES)
        s.build_bvh()
        info2 = s.wide_info()
        sources.append(info2["source"])
        nodes2, winst2 = s.download_wide(pt.WIDE_NODES), s.download_wide(pt.WIDE_INSTANCES)
        if info2["source"] == 3:
            # the new matrices reach farther into a mesh's object space than its tree was quantised for (more
            # than twice the first build's reach; it happens with few instances, count = 2): pt.h's rule makes
            # this build the full one again.  Only the first may be; its arrays are the host's for the new matrices
            assert sources == [3]
            top_cap = run_inst_check(tmp_path, files2, nodes2, winst2, info2, "full")
            nodes = nodes2
            continue
        assert info2["source"] == 4
        assert nodes2.shape == nodes.shape and 1 <= top_cap <= len(nodes)
        np.testing.assert_array_equal(nodes2[top_cap:], nodes[top_cap:], err_msg="the rebuild keeps the mesh trees")
        assert run_inst_check(tmp_path, files2, nodes2, winst2, info2, "top") == top_cap
    assert sources[1:] == [4, 4], sources   # (the second of them reuses the first one's scratch)
