"""The instanced scene's builds pinned to recorded results (tests/golden/instanced_build_counters.json).

The 9- and 65-instance worlds of test_tree_shapes (tests/test_gpu_instance_update.py), each in three
states -- a fresh scene (wide_info source 3), a fresh scene built with PT_BVH_WIDE_DEVICE (the full
build in the layout for instance updates) and a scene after update_instances plus two builds (source
4: the top level rebuilt on the device) -- traced with 4,096 rays by the wide kernel.  Per state the
tree's depth, slots and source, the scene's device bytes, the CRC32 of the hit records and the work
counters must equal what the library gave when the fixture was recorded: the host tree build
(host/pt_instancing.cpp) decides every one of them, so a change there that alters the tree in any way
shows here.  The fixture holds only fields that were reproducible between two recordings.
"""
import json
import os
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  before libpt.so loads (the two must share torch's HIP runtime)

from helpers import OBJECT_DTYPE, random_soup, tree_shape_instances, two_triangles
from test_gpu_instance_update import World

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instanced_build_counters.json")
COUNTS = (9, 65)


def record(pt, scene, rays):
    hits, st = scene.trace(rays, kernel=pt.KERNEL_WIDE)
    wi = scene.wide_info()
    return {"depth": wi["depth"], "slots": wi["slots"], "source": wi["source"],
            "device_bytes": scene.bvh_info()["device_bytes"], "hit_crc32": zlib.crc32(hits.tobytes()),
            "rays": st.rays, "node_visits": st.node_visits, "tri_tests": st.tri_tests, "sphere_tests": st.sphere_tests}


def measure(pt, gpu, count):
    """{state: record} of the `count`-instance world."""
    soup, mats = random_soup(600, 60, seed=21, spread=4.0)
    w = World(pt, gpu, [two_triangles(), soup, np.zeros(0, OBJECT_DTYPE)], mats)
    m1, mesh, reach = tree_shape_instances(count, 31)
    m2, _, _ = tree_shape_instances(count, 32)
    first, second = w.instances(m1, mesh), w.instances(m2, mesh)
    rays1, rays2 = (w.rays(i, 4096, seed=33, radius=2.0 * reach) for i in (first, second))
    out = {}
    s = w.scene(first)
    out["fresh"] = record(pt, s, rays1)
    d = pt.Scene.instanced(w.objs, w.first, w.count, first, w.mats, device=gpu, build=False)
    d.build_bvh(pt.PT_BVH_WIDE_DEVICE)
    out["fresh_dynamic"] = record(pt, d, rays1)
    s.update_instances(second)
    s.build_bvh()
    s.build_bvh()
    out["updated"] = record(pt, s, rays2)
    return out


@pytest.mark.parametrize("count", COUNTS)
def test_recorded_builds(pt, gpu, count):
    want = json.load(open(GOLDEN))[str(count)]
    assert set(want) == {"fresh", "fresh_dynamic", "updated"}
    assert all({"depth", "slots", "source", "device_bytes", "hit_crc32"} <= set(f) for f in want.values())
    got = measure(pt, gpu, count)
    assert got["fresh"]["source"] == 3 and got["fresh_dynamic"]["source"] == 3 and got["updated"]["source"] == 4
    for state, fields in want.items():
        assert {k: got[state][k] for k in fields} == fields, state
