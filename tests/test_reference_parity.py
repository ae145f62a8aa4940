"""The oracle against the reference's OWN code, compiled for the CPU (oracle/ref/, `make -C oracle ref`).

Every parity claim of this project is "bit-identical to oracle/", and the oracle is a hand
restatement of the reference.  These tests close the remaining link: the reference's utils/ and
simulation/ headers and rayTracing / initRandom / render cut out of its main.cu, built as two host
programs (g++ and the ROCm clang++, -O2 -ffp-contract=off) behind a small shim, run on the same
arrays as the oracle.  Comparisons are by bits, tolerance 0, on every field the reference defines
(hit_record has no object id; u, v and the ray's time are ignored).  Where random draws are involved
both programs run: clang++ draws vec3(u, u, u)'s coordinates x, y, z -- the oracle's default -- and
g++ z, y, x -- orc.set_draw_order(True).

The oracle's documented deviations are named switches of the harness (oracle/refharness.py): powf
and camera_draws.  Pixel 0 is the one pixel left out of frame comparisons (camera::get_ray draws
from randState[0], main.cu:286).

Without the reference tree oracle/_ref/ is empty and this module skips; tests/test_reference_fixtures.py
(which needs no reference) then still checks the oracle against what the reference recorded."""
import os

import numpy as np
import pytest

import reference_cases as rc
import refharness as rh

pytestmark = pytest.mark.skipif(not rh.available(),
                                reason="oracle/_ref/ holds no reference programs (no reference tree at build time)")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(REPO, "tests", "golden", "oracle_fixtures.npz")
HIT_FIELDS = ("hit", "mat", "front_face")   # + t, p, n where hit: what hit_record defines


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def canon(a):
    """Bit patterns with every NaN mapped to one pattern.  Which NaN an operation returns -- sign and
    payload -- is outside the reference's semantics: IEEE 754 leaves it to the implementation, SSE
    hands on its first operand's and the compiler picks the operand order of a commutative operation,
    and the GPU the reference was written for returns one canonical NaN.  A NaN therefore equals
    any NaN here; everything else, the signs of zeros and infinities included, is compared by bits."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def assert_bits(got, want, what=""):
    np.testing.assert_array_equal(canon(got), canon(want), err_msg=what)


def assert_hits(got, want, what=""):
    for f in HIT_FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what} {f}")
    h = want["hit"] == 1
    for f in ("t", "p", "n"):
        assert_bits(got[f][h], want[f][h], f"{what} {f}")


def assert_nodes(got, want, what=""):
    for f in ("left", "right", "parent", "objid"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what} {f}")
    assert_bits(got["bmin"], want["bmin"], what + " bmin")
    assert_bits(got["bmax"], want["bmax"], what + " bmax")


@pytest.fixture(scope="module")
def fx():
    with np.load(FIX) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(params=rh.COMPILERS)
def compiler(request, orc):
    """One of the two programs, with the oracle switched to the draw order that program pins."""
    orc.set_draw_order(rh.DRAW_ORDER_ZYX[request.param])
    yield request.param
    orc.set_draw_order(False)


# ------------------------------------------------------- the committed fixture, re-derived
@pytest.mark.parametrize("key", ["c2", "c3"])
def test_fixture_f1_keys(fx, key):
    """computeMortonOnHost gives the committed keys (no draws: one program is enough, both run)."""
    for comp in rh.COMPILERS:
        np.testing.assert_array_equal(rh.morton_keys(comp, fx[f"{key}_objects"]), fx[f"f1_{key}_keys"], err_msg=comp)


@pytest.mark.parametrize("key", ["c2", "tw", "c3"])
def test_fixture_f2_lbvh(orc, fx, key):
    """buildBVH: the committed topology; the committed origin-seeded boxes where the file has them
    (C3: the oracle's tight=False boxes, and the tight file's topology)."""
    objs = fx[f"{key}_objects"]
    for comp in rh.COMPILERS:
        _, nodes = rh.build_lbvh(comp, objs)
        for f in ("left", "right", "parent", "objid"):
            np.testing.assert_array_equal(nodes[f], fx[f"f2_{key}_tight"][f], err_msg=f"{comp} {f}")
        want = fx[f"f2_{key}_ref"] if f"f2_{key}_ref" in fx else orc.build_lbvh(objs, orc.morton_keys(objs), tight=False)
        assert_nodes(nodes, want, comp)


@pytest.mark.parametrize("brute", [False, True], ids=["hitBvh", "hit"])
@pytest.mark.parametrize("key", ["c2", "c3", "tw"])
def test_fixture_f3_hits(fx, key, brute):
    for comp in rh.COMPILERS:
        assert_hits(rh.trace(comp, fx[f"{key}_objects"], fx[f"f3_{key}_rays"], brute=brute), fx[f"f3_{key}_hits"], comp)


def test_fixture_f4_scatter(fx):
    """The committed tapes were recorded under the default order (x, y, z): the clang++ program."""
    rays, hits = fx["f3_c3_rays"], fx["f3_c3_hits"]
    i = fx["f4_case"]
    ok, out, att, used = rh.scatter("clang", fx["f4_materials"], fx["f4_mat"], rays[i], hits[i], fx["f4_tape"])
    np.testing.assert_array_equal(ok, fx["f4_ok"])
    np.testing.assert_array_equal(used, fx["f4_used"])
    assert_bits(out, fx["f4_out"])
    assert_bits(att, fx["f4_att"])


@pytest.mark.parametrize("key", ["c1", "c2"])
def test_fixture_f5_frames(fx, key):
    """initRandom + render give the committed frames (and C2's streams afterwards), pixel 0 excluded."""
    w, h = (int(v) for v in fx[f"{key}_size"])
    spp, depth, seed = (int(v) for v in fx[f"f5_{key}_params"])
    rgb, st = rh.render("clang", fx[f"{key}_objects"], fx[f"{key}_materials"], fx[f"{key}_camera"], w, h, spp, depth, seed)
    assert_bits(rgb[0][1:], fx[f"f5_{key}_rgb"][1:])
    if f"f5_{key}_rng_after" in fx:
        np.testing.assert_array_equal(st[0][1:], fx[f"f5_{key}_rng_after"][1:])


# --------------------------------------------------------------------------- small LBVHs
@pytest.mark.parametrize("n", rc.LBVH_SIZES)
@pytest.mark.parametrize("kind", rc.LBVH_KINDS)
def test_lbvh_small_sizes(orc, kind, n):
    objs = rc.lbvh_objects(kind, n)
    assert len(objs) == n
    okeys = orc.morton_keys(objs)
    want = orc.build_lbvh(objs, okeys, tight=False)
    tight = orc.build_lbvh(objs, okeys, tight=True)
    if kind == "dup":
        assert len(set((okeys >> np.uint64(32)).tolist())) == 1
    for comp in rh.COMPILERS:
        keys, nodes = rh.build_lbvh(comp, objs)
        np.testing.assert_array_equal(keys, okeys, err_msg=comp)
        assert_nodes(nodes, want, f"{comp} {kind} n={n}")
        # the box rule everything rests on: reference box == tight box U {origin}, every internal node
        k = n - 1
        assert_bits(nodes["bmin"][:k], np.minimum(tight["bmin"][:k], np.float32(0)), "box rule min")
        assert_bits(nodes["bmax"][:k], np.maximum(tight["bmax"][:k], np.float32(0)), "box rule max")
        assert_bits(nodes["bmin"][k:], tight["bmin"][k:])   # leaves: the objects' own boxes
        assert_bits(nodes["bmax"][k:], tight["bmax"][k:])


# --------------------------------------------------------------- degenerate rays and scenes
@pytest.fixture(scope="module")
def degenerate():
    scenes = rc.degenerate_scenes()
    return {name: (objs,) + rc.degenerate_batch(objs) for name, objs in scenes.items()}


@pytest.mark.parametrize("brute", [False, True], ids=["hitBvh", "hit"])
@pytest.mark.parametrize("scene", ["soup_negr", "one_sphere", "one_sphere_negr", "one_triangle"])
def test_degenerate_rays(orc, degenerate, scene, brute):
    """NaN, +-inf, zero and denormal directions, overflowing magnitudes, negative radii, a one-primitive
    scene, every interval of tests/degenerate_rays.py: the reference itself against orc.trace with
    nan_miss=False -- include/pt.h's account of what the reference does with a NaN candidate."""
    from degenerate_rays import INTERVALS
    objs, rays, where = degenerate[scene]
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=False)
    nan_hits = 0
    for tmin, tmax in INTERVALS:
        want, _ = orc.trace(objs, nodes, rays, tmin=tmin, tmax=tmax, brute=brute, nan_miss=False)
        nan_hits += int(np.isnan(want["t"][want["hit"] == 1]).sum())
        for comp in rh.COMPILERS:
            got = rh.trace(comp, objs, rays, tmin=tmin, tmax=tmax, brute=brute)
            assert_hits(got, want, f"{comp} {scene} [{tmin}, {tmax}]")
    if scene == "soup_negr":
        assert nan_hits > 0   # the reference does return records of NaNs: the case pt.h changes


# ------------------------------------------------------------------------------- scatter
def oracle_scatter(orc, mats, case_mat, rays, hits, tapes):
    k = len(case_mat)
    ok, out, att, used = np.zeros(k, np.int32), np.zeros((k, 6), np.float32), np.zeros((k, 3), np.float32), np.zeros(k, np.int32)
    for i in range(k):
        o, r, a, u = orc.scatter_tape(mats[case_mat[i]], rays[i], hits[i], tapes[i])
        ok[i], out[i], att[i], used[i] = int(o), r, a, u
    return ok, out, att, used


def assert_scatter(got, want, labels=None):
    for name, g, w in zip(("ok", "out_ray", "atten", "used"), got, want):
        if g.dtype == np.float32:
            g, w = bits(g), bits(w)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert not len(bad), f"{name}: {len(bad)} cases differ, first {bad[:5]}" + (
            f" ({[labels[i] for i in bad[:5]]})" if labels else "")


def test_scatter_bulk(orc, compiler):
    """20,000 seeded cases per material type on real hits of a soup, front and back faces."""
    mats, cm, rays, hits, tapes = rc.scatter_bulk(orc)
    for t in (1, 2, 4):
        assert (mats["type"][cm] == t).sum() == 20000
    want = oracle_scatter(orc, mats, cm, rays, hits, tapes)
    assert 0 < want[0].sum() < len(cm)                     # metal absorbs some
    assert want[3].max() > 12                              # rejection loops of several rounds
    assert_scatter(rh.scatter(compiler, mats, cm, rays, hits, tapes), want)


def test_scatter_edges(orc, compiler):
    """The constructed edges: ir in {1, 1.5, 1/1.5, 2.4}, total internal reflection, cos_theta clamped
    by the fminf, fuzz {0, 0.3, 1} at grazing incidence (the absorb exit), near_zero, an unknown
    material type, long rejection loops."""
    mats, cm, rays, hits, tapes, labels = rc.scatter_edges()
    want = oracle_scatter(orc, mats, cm, rays, hits, tapes)
    ok, out, att, used = want
    lab = np.array(labels)
    sel = lambda s: np.array([s in x for x in labels])   # noqa: E731
    # the cases reach what they were built for (under either draw order)
    assert (ok[sel("metal fuzz")] == 0).any() and (ok[sel("metal fuzz")] == 1).any()
    assert (ok[sel("unknown type")] == 0).all() and (used[sel("unknown type")] == 0).all()
    assert (used[sel("TIR")] == 0).all()                   # cannot_refract short-circuits the draw
    nz = sel("near_zero")
    assert (bits(out[nz][:, 3:]) == bits(hits["n"][nz])).all(axis=1).any(), "no case drove near_zero"
    th = sel("near_zero threshold")   # both sides of the 1e-7 threshold, under this draw order
    fell_back = (bits(out[th][:, 3:]) == bits(hits["n"][th])).all(axis=1)
    assert fell_back.any() and (~fell_back & (used[th] == 3)).any()
    assert used[sel("k=52")].max() >= 3 * 53
    both = used[sel("dielectric")]
    assert (both == 1).any() and (both == 0).any()
    assert_scatter(rh.scatter(compiler, mats, cm, rays, hits, tapes), want, list(lab))


def test_powf_switch(orc):
    """Deviation 1 of the oracle: powf(x, 5) as ((x*x)*(x*x))*x.  With the switch off (libm's powf)
    the reference's reflectance differs from the oracle's in some cases -- the switch is not vacuous
    -- and with it on, never (test_scatter_bulk).  Prints the measurement DESIGN.md §3 records."""
    mats, cm, rays, hits, tapes = rc.scatter_bulk(orc)
    d = mats["type"][cm] == 4
    cm, rays, hits, tapes = cm[d], rays[d], hits[d], tapes[d]
    m = measure_powf(mats, cm, rays, hits, tapes)
    print(f"powf deviation on {d.sum()} dielectric cases: max |reflectance ulp| = {m['max_ulp']}, "
          f"{m['ulp_nonzero']} reflectances differ, {m['decisions']} reflect/refract decisions differ "
          f"({m['decisions'] / d.sum():.2e})")
    assert m["max_ulp"] > 0


def measure_powf(mats, cm, rays, hits, tapes, comp="clang"):
    """Reflectance under libm's powf against the multiply form, on dielectric scatter cases: the
    inputs of reflectance() are recomputed here in float32 in material.h:47-49's order."""
    f = np.float32
    d = rays[:, 3:].astype(f)
    ln = np.sqrt(((d[:, 0] * d[:, 0]).astype(f) + (d[:, 1] * d[:, 1]).astype(f)).astype(f) + (d[:, 2] * d[:, 2]).astype(f))
    ud = ((f(1.0) / ln)[:, None] * d).astype(f)
    n = hits["n"]
    dot = ((-ud[:, 0] * n[:, 0]).astype(f) + (-ud[:, 1] * n[:, 1]).astype(f)).astype(f) + (-ud[:, 2] * n[:, 2]).astype(f)
    cos = np.minimum(dot.astype(f), f(1.0))
    ir = mats["ir"][cm]
    ratio = np.where(hits["front_face"] == 1, (f(1.0) / ir).astype(f), ir).astype(f)
    r_mul = rh.reflectance(comp, cos, ratio, powf="mul")
    r_lib = rh.reflectance(comp, cos, ratio, powf="libm")
    ulp = np.abs(r_mul.view(np.int32).astype(np.int64) - r_lib.view(np.int32).astype(np.int64))
    a = rh.scatter(comp, mats, cm, rays, hits, tapes, powf="mul")
    b = rh.scatter(comp, mats, cm, rays, hits, tapes, powf="libm")
    decisions = int((bits(a[1]) != bits(b[1])).any(axis=1).sum())
    return {"max_ulp": int(ulp.max()), "ulp_nonzero": int((ulp > 0).sum()), "decisions": decisions, "cases": len(cm)}


# -------------------------------------------------------------------------------- cameras
def test_camera_constructor_and_moves(pt, orc):
    """camera's constructor and processKeyboard against orc.camera_make and pt_camera_make /
    pt_camera_move: the presets' cameras and off-axis ones (a straight-down and a from == at one
    among them, where normalize() returns zeros)."""
    args = rc.CAMERA_ARGS
    k = len(args)
    mdir = np.tile(rc.CAMERA_MOVE_DIR, (k, 1))
    mdt = np.tile(rc.CAMERA_MOVE_DT, (k, 1))
    for i, (name, (w, h)) in enumerate(rc.CAMERA_PRESETS.items()):   # the first rows ARE the presets' cameras
        a = args[i]
        cam = pt.camera_make(a[0:3], a[3:6], *[float(x) for x in a[6:12]])
        assert_bits(pt.camera_to_array(pt.Preset(name, w, h).camera), pt.camera_to_array(cam), name)
    for comp in rh.COMPILERS:
        cams, moved = rh.camera(comp, args, mdir, mdt)
        for i, a in enumerate(args):
            rest = [float(x) for x in a[6:12]]
            assert_bits(orc.camera_make(a[0:3], a[3:6], *rest), cams[i], f"{comp} orc camera {i}")
            cam = pt.camera_make(a[0:3], a[3:6], *rest)
            assert_bits(pt.camera_to_array(cam), cams[i], f"{comp} pt camera {i}")
            for j in range(mdir.shape[1]):
                pt.camera_move(cam, int(mdir[i, j]), float(mdt[i, j]))
                assert_bits(pt.camera_to_array(cam), moved[i, j], f"{comp} camera {i} move {j}")


# --------------------------------------------------------------------------------- frames
@pytest.fixture(scope="module")
def frames(pt, orc):
    return rc.frame_cases(pt, orc)


@pytest.mark.parametrize("name", ["rtiow", "triangle_world", "cornell", "l2", "rtiow_depth0", "rtiow_depth1"])
def test_whole_frames(orc, frames, compiler, name):
    """rayTracing and render over whole frames against orc.render, with the stream states after
    every launch; l2 launches twice (the second continues the streams).  Pixel 0 excluded."""
    c = frames[name]
    want_rgb, want_st = rc.oracle_frames(orc, c)
    rgb, st = rh.render(compiler, c["objects"], c["materials"], c["camera"], c["width"], c["height"], c["spp"],
                        c["depth"], c["seed"], launches=c["launches"])
    for launch in range(c["launches"]):
        assert_bits(rgb[launch][1:], want_rgb[launch][1:], f"{name} launch {launch} image")
        np.testing.assert_array_equal(st[launch][1:], want_st[launch][1:], err_msg=f"{name} launch {launch} streams")
    if c["depth"] > 1:
        assert not np.array_equal(want_st[0][1:, 0], orc.film_states(c["seed"], c["width"], np.arange(c["height"]))[1:, 0])


def test_camera_draws_switch(orc, frames):
    """Deviation 2 of the oracle: camera::get_ray draws from randState[0] (main.cu:286).  With the
    harness switch on "shared" (the reference untouched) pixel 0 -- and only pixel 0 -- differs from
    the isolated run: the deviation is there, and it is confined to the pixel the comparisons leave out."""
    c = frames["rtiow_depth0"]   # no bounce, no scatter draw: every pixel's draw count is known
    args = (c["objects"], c["materials"], c["camera"], c["width"], c["height"], c["spp"], c["depth"], c["seed"])
    iso_rgb, iso_st = rh.render("clang", *args, camera_draws="isolated")
    sh_rgb, sh_st = rh.render("clang", *args, camera_draws="shared")
    assert_bits(sh_rgb[0][1:], iso_rgb[0][1:])
    np.testing.assert_array_equal(sh_st[0][1:], iso_st[0][1:])
    assert not np.array_equal(sh_st[0][0], iso_st[0][0])
    want_rgb, want_st = rc.oracle_frames(orc, c)
    # pixel 0's own camera draws (2 lens + 1 time per sample; the oracle takes none): 5 * spp draws, not 2 * spp
    assert not np.array_equal(iso_st[0][0], want_st[0][0])
    s0 = orc.xorwow_init(c["seed"], 0)
    orc.curand_uniform(s0, 5 * c["spp"])
    np.testing.assert_array_equal(iso_st[0][0], s0)
