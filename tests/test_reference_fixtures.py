"""tests/golden/reference_fixtures.npz -- outputs of the reference's OWN code, recorded by
tools/make_reference_fixtures.py -- against the CPU restatement: the oracle reproduces every array
of the file, bit for bit.  Needs no reference tree and never skips; where the reference programs
are built (oracle/_ref/), they reproduce the file too.  The GPU counterpart is
tests/test_gpu_reference_fixtures.py.

A NaN equals any NaN (its sign and payload are the host's, not the reference's: see
tests/test_reference_parity.py); pixel 0 of a frame is left out (main.cu:286)."""
import os

import numpy as np
import pytest

import refharness as rh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(REPO, "tests", "golden", "reference_fixtures.npz")
LBVH = [(k, n) for k in ("soup", "dup") for n in (1, 2, 3, 7, 64, 65, 1000)]
DEG = ("soup_negr", "one_sphere", "one_sphere_negr", "one_triangle")
FRAMES = ("rtiow", "triangle_world", "cornell", "l2")
COMPILER_OF = {"xyz": "clang", "zyx": "gxx"}


@pytest.fixture(scope="module")
def fx():
    with np.load(FIX) as d:
        return {k: d[k] for k in d.files}


def canon(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def assert_bits(got, want, what=""):
    np.testing.assert_array_equal(canon(got), canon(want), err_msg=what)


def assert_hits(got, want, what="", fields=("hit", "mat", "front_face")):
    for f in fields:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what} {f}")
    h = want["hit"] == 1
    for f in ("t", "p", "n"):
        assert_bits(got[f][h], want[f][h], f"{what} {f}")


def test_file_is_plain_data_and_small(fx):
    assert os.path.getsize(FIX) < 1 << 20
    assert bytes(fx["draw_order"]) == b"xyz"
    for k, a in fx.items():
        assert a.dtype != object, k


@pytest.mark.parametrize("kind,n", LBVH)
def test_lbvh(orc, fx, kind, n):
    objs = fx[f"lbvh_{kind}_{n}_objects"]
    keys, nodes = fx[f"lbvh_{kind}_{n}_keys"], fx[f"lbvh_{kind}_{n}_nodes"]
    assert len(objs) == n and len(nodes) == 2 * n - 1
    np.testing.assert_array_equal(orc.morton_keys(objs), keys)
    o = orc.build_lbvh(objs, keys, tight=False)
    assert o.tobytes() == nodes.tobytes()
    tight = orc.build_lbvh(objs, keys, tight=True)   # the box rule: recorded box == tight box U {origin}
    assert_bits(np.minimum(tight["bmin"][:n - 1], np.float32(0)), nodes["bmin"][:n - 1])
    assert_bits(np.maximum(tight["bmax"][:n - 1], np.float32(0)), nodes["bmax"][:n - 1])
    if rh.available():
        for comp in rh.COMPILERS:
            k2, n2 = rh.build_lbvh(comp, objs)
            assert np.array_equal(k2, keys) and n2.tobytes() == nodes.tobytes(), comp


@pytest.mark.parametrize("scene", DEG)
def test_degenerate_hits(orc, fx, scene):
    objs, rays, hits = fx[f"deg_{scene}_objects"], fx[f"deg_{scene}_rays"], fx[f"deg_{scene}_hits"]
    lib, via = fx[f"deg_{scene}_lib_hits"], fx[f"deg_{scene}_via_nan"]
    assert len(rays) == len(fx["deg_classes"]) * int(fx["deg_class_size"][0]) and np.isnan(rays).any()
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=False)
    got, _ = orc.trace(objs, nodes, rays, nan_miss=False)   # hitBvh, as recorded (on these rays the brute-force
    assert_hits(got, hits, scene)                           # loop legitimately differs: no box ever culls a NaN)
    # lib_hits is the reference's record under pt.h's one change: a NaN t is the miss record
    ruled, _ = orc.trace(objs, nodes, rays, nan_miss=True)
    assert_hits(ruled, lib, scene + " lib", fields=("hit", "obj", "mat", "front_face"))
    nan_t = (hits["hit"] == 1) & np.isnan(hits["t"])
    assert nan_t.any() and (lib["hit"][nan_t] == 0).all() and (lib["obj"][nan_t] == -1).all()
    keep = ~nan_t & ~via
    assert_hits(lib[keep], hits[keep], scene + " unchanged records")
    if rh.available():
        for comp in rh.COMPILERS:
            assert_hits(rh.trace(comp, objs, rays), hits, f"{comp} {scene}")


@pytest.mark.parametrize("order", ["xyz", "zyx"])
def test_scatter_edges(orc, fx, order):
    mats, cm, rays, hits, tapes = (fx[k] for k in ("sc_materials", "sc_case_mat", "sc_case_ray", "sc_case_hit", "sc_tapes"))
    orc.set_draw_order(order == "zyx")
    try:
        for i in range(len(cm)):
            ok, out, att, used = orc.scatter_tape(mats[cm[i]], rays[i], hits[i], tapes[i])
            what = str(fx["sc_labels"][i])
            assert int(ok) == fx[f"sc_ok_{order}"][i] and used == fx[f"sc_used_{order}"][i], what
            assert_bits(out, fx[f"sc_out_{order}"][i], what)
            assert_bits(att, fx[f"sc_att_{order}"][i], what)
    finally:
        orc.set_draw_order(False)
    if rh.available():
        ok, out, att, used = rh.scatter(COMPILER_OF[order], mats, cm, rays, hits, tapes)
        np.testing.assert_array_equal(ok, fx[f"sc_ok_{order}"])
        np.testing.assert_array_equal(used, fx[f"sc_used_{order}"])
        assert_bits(out, fx[f"sc_out_{order}"])
        assert_bits(att, fx[f"sc_att_{order}"])


@pytest.mark.parametrize("name", FRAMES)
def test_frames(orc, fx, name):
    objs, mats, cam = fx[f"fr_{name}_objects"], fx[f"fr_{name}_materials"], fx[f"fr_{name}_camera"]
    w, h, spp, depth, seed, launches = (int(v) for v in fx[f"fr_{name}_params"])
    assert w >= 24 and h >= 16 and fx[f"fr_{name}_rgb"].shape == (launches, w * h, 3)
    rows = np.arange(h, dtype=np.int32)
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    states = orc.film_states(seed, w, rows)
    for launch in range(launches):
        rgb, _ = orc.render(objs, mats, nodes, cam, w, h, rows, spp, depth, states, nthreads=4)
        assert_bits(rgb[1:], fx[f"fr_{name}_rgb"][launch][1:], f"{name} launch {launch}")
        np.testing.assert_array_equal(states[1:], fx[f"fr_{name}_states"][launch][1:])
    if rh.available():
        order = bytes(fx["draw_order"]).decode()
        rgb, st = rh.render(COMPILER_OF[order], objs, mats, cam, w, h, spp, depth, seed, launches=launches)
        assert_bits(rgb, fx[f"fr_{name}_rgb"], name)            # pixel 0 included: the same program
        np.testing.assert_array_equal(st, fx[f"fr_{name}_states"])
