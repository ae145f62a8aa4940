"""CPU checks of tests/affine_ref.py: the float64 instanced reference against the oracle where the
two must agree (identity and translation instances), and the conditions every transform class has
to meet for the GPU tests of test_gpu_instance_affine.py to mean something (enough clear hits, few
ambiguous rays, mirrored instances present).  The caps are conditions on the inputs, not
measurements of a kernel: if a seed change breaks one, change the inputs, not the cap.

Measured with the generators of affine_ref.py (matrices seed 70, stretch4's 73; rays seed 71,
4,096 rays):

    class      ambiguous  clear hits  of them sphere  clear misses  det < 0  largest es
    mirror       1.98 %      2604         1188            1411         8       0.0092
    ellipsoid    2.03 %      2431         1006            1582         8       0.0201
    shear        2.61 %      2382         1033            1607         6       0.0394
    stretch4     2.17 %      2272            -            1735         8          -
    pancake      4.15 %      1877            -            2049         8          -
    needle       4.39 %      1807            -            2109         8          -

Between 30 % and 60 % of a class's ambiguous rays are clear but for |cos(ray, normal)| < 0.05 on the
nearest triangle (squashed soups turn their triangles edge-on to the rays across the squashed axis);
with seed 70 that put stretch4 at 3.17 %, above its cap, hence its own seed.
"""
import numpy as np
import pytest

import affine_ref as ar
from helpers import random_rays, random_soup


def test_reference_matches_oracle_on_translations(orc):
    """Identity and translation instances: on clear rays the reference names the oracle's hit of the
    flattened objects (the world vertices differ only by their rounding to float, 2e-6 at 30 units,
    far inside the margins)."""
    a, _ = random_soup(200, 20, seed=21, spread=4.0)
    rng = np.random.default_rng(5)
    m = np.zeros((6, 12), np.float32)
    m[:, [0, 5, 10]] = 1.0
    m[1:, 3], m[1:, 7], m[1:, 11] = rng.uniform(-30.0, 30.0, (3, 5)).astype(np.float32)
    ids = np.zeros(6, np.int64)
    flat = ar.flatten([a], m, ids)
    assert len(flat) == 6 * len(a)
    rays = random_rays(4096, seed=6, radius=60.0, objects=flat)
    ref = ar.reference([a], m, ids, rays)
    got, _ = orc.trace(flat, orc.build_lbvh(flat, orc.morton_keys(flat), tight=True), rays, ar.TMIN, np.inf)
    miss, hit = ref["kind"] == ar.MISS, ref["kind"] == ar.HIT
    assert hit.sum() >= 1000 and miss.sum() >= 500 and ref["sphere"][hit].sum() >= 100
    assert (ref["kind"] == ar.AMBIGUOUS).mean() <= 0.03
    assert (got["hit"][miss] == 0).all()
    assert (got["hit"][hit] == 1).all()
    for f in ("obj", "mat", "front_face"):
        np.testing.assert_array_equal(got[f][hit], ref[f][hit], err_msg=f)
    t = ref["t"][hit]
    assert (np.abs(got["t"][hit] - t) <= 2e-4 * t + 1e-4).all()
    cos = (got["n"][hit].astype(np.float64) * ref["n"][hit]).sum(1) / np.linalg.norm(got["n"][hit], axis=1)
    assert cos[ref["sphere"][hit] == 0].min() >= 0.9999
    assert np.median(cos) >= 0.99999 and cos.min() >= 0.995


def test_flatten_swaps_mirrored_windings():
    tri = np.zeros(1, ar.OBJECT_DTYPE)
    tri["type"] = 3
    tri["v"][0] = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    m = np.zeros((2, 12), np.float32)
    m[:, [0, 5]] = 1.0
    m[0, 10], m[1, 10] = 1.0, -1.0
    flat = ar.flatten([tri], m, [0, 0])
    np.testing.assert_array_equal(flat["v"][0], [0, 0, 0, 1, 0, 0, 0, 1, 0])
    np.testing.assert_array_equal(flat["v"][1], [0, 0, 0, 0, 1, 0, 1, 0, 0])
    # the reference's front side is the mesh's own under both: a ray coming down the object's +z
    rays = np.array([[0.2, 0.2, 5, 0, 0, -1], [0.2, 0.2, -5, 0, 0, 1]], np.float32)
    ref = ar.reference([tri], m[:1], [0], rays)
    assert list(ref["kind"]) == [ar.HIT, ar.HIT] and list(ref["front_face"]) == [1, 0]
    ref = ar.reference([tri], m[1:], [0], rays)     # mirrored in z: object +z is world -z
    assert list(ref["kind"]) == [ar.HIT, ar.HIT] and list(ref["front_face"]) == [0, 1]
    np.testing.assert_allclose(ref["n"], [[0, 0, 1], [0, 0, -1]], atol=1e-15)
    np.testing.assert_allclose(ref["t"], [5, 5], rtol=1e-15)


def test_sphere_margins_and_roots():
    """One unit sphere stretched 2 x along x: the near root from outside (front), the far root from
    inside (back), a silhouette ray ambiguous, and the hollow sphere's flipped front side."""
    for r, front in ((1.0, [1, 0]), (-1.0, [0, 1])):
        s = np.zeros(1, ar.OBJECT_DTYPE)
        s["type"] = 1
        s["v"][0, :4] = [0, 0, 0, r]
        m = np.zeros((1, 12), np.float32)
        m[0, [0, 5, 10]] = [2.0, 1.0, 1.0]
        es = 4.0 * 2.0 ** -24 * 26.0    # the farthest origin, (5, 1, 0) in object space: D^2 = 26 r^2
        rays = np.array([[10, 0, 0, -1, 0, 0], [0.5, 0, 0, 0, 1, 0], [10, 1.0 + 0.5 * es, 0, -1, 0, 0],
                         [10, 1.0 + 2.0 * es, 0, -1, 0, 0]], np.float32)
        ref = ar.reference([s], m, [0], rays)
        assert list(ref["kind"]) == [ar.HIT, ar.HIT, ar.AMBIGUOUS, ar.MISS]
        assert list(ref["front_face"][:2]) == front
        np.testing.assert_allclose(ref["t"][:2], [8.0, np.sqrt(1 - 0.0625)], rtol=1e-12)
        y = np.sqrt(1 - 0.0625)         # object-space hit (0.25, y, 0): A^-T halves the normal's x
        inner = -np.array([0.125, y, 0]) / np.hypot(0.125, y)
        np.testing.assert_allclose(ref["n"][:2], [[1, 0, 0], inner], atol=1e-12)
        assert abs(ar.reference.last_es_max - es) <= 1e-3 * es


@pytest.mark.parametrize("name", ar.CLASSES)
def test_class_conditions(name):
    c = ar.case(name)
    ref = c.ref
    hit, amb = ref["kind"] == ar.HIT, ref["kind"] == ar.AMBIGUOUS
    n_sph = int(ref["sphere"][hit].sum())
    neg = int((c.dets() < 0).sum())
    print(f"{name}: ambiguous {100 * amb.mean():.2f} % clear hits {hit.sum()} sphere {n_sph} det<0 {neg} "
          f"es_max {c.es_max:.4f} clear misses {(ref['kind'] == ar.MISS).sum()}")
    assert amb.mean() <= (0.03 if name in ar.MODERATE else 0.06)
    assert hit.sum() >= 1000
    has_spheres = any((m["type"] == 1).any() for m in c.meshes)
    assert has_spheres == (name in ("mirror", "ellipsoid", "shear"))
    if has_spheres:
        assert n_sph >= 150
        assert c.es_max <= 0.04
    assert neg >= 5 and (c.dets() > 0).sum() >= 5
    assert (ref["kind"] == ar.MISS).sum() >= 500
    assert ref["obj"][hit].max() < c.n_flat() and len(c.flat) == c.n_flat()
    assert len(set(ref["inst"][hit])) == ar.N_INSTANCES       # every instance is hit
    if name == "mirror":
        assert sum((m["v"][m["type"] == 1, 3] < 0).sum() for m in c.meshes) == 1
    if name in ar.EXTREME:
        s = np.array([np.linalg.svd(m.reshape(3, 4)[:, :3].astype(np.float64), compute_uv=False) for m in c.matrices])
        np.testing.assert_allclose(s[:, 0] / s[:, 2], 32.0, rtol=1e-5)
        np.testing.assert_allclose(s[:, 1] / s[:, 2], 32.0 if name == "pancake" else 1.0, rtol=1e-5)


def records_of(orc, case):
    """Hit records that agree with the reference: its own, rounded to float, misses elsewhere."""
    ref = case.ref
    got = np.zeros(len(ref), orc.HIT_DTYPE)
    h = ref["kind"] == ar.HIT
    got["hit"] = h
    for f in ("obj", "mat", "front_face", "t", "p", "n"):
        got[f][h] = ref[f][h]
    return got


def test_checker_tells_wrong_records(orc):
    """check_closest, the GPU tests' comparison, on records that are wrong the ways a kernel could be:
    each of these must fail, and the reference's own records must pass."""
    mirror, ell = ar.case("mirror"), ar.case("ellipsoid")
    for c in (mirror, ell):
        ar.check_closest(c, records_of(orc, c))

    def fails(case, got, what):
        with pytest.raises(AssertionError) as e:
            ar.check_closest(case, got)
        assert what in str(e.value), (what, str(e.value)[:200])

    ref = mirror.ref
    hit = ref["kind"] == ar.HIT
    # the flattened scene's front side on mirrored instances' triangles
    got = records_of(orc, mirror)
    flip = hit & (ref["sphere"] == 0) & (mirror.dets()[ref["inst"]] < 0)
    assert flip.sum() > 300
    got["front_face"][flip] ^= 1
    fails(mirror, got, "front_face")
    # a box that drops 0.3 % of the true hits
    got = records_of(orc, mirror)
    got["hit"][np.flatnonzero(hit)[::333]] = 0
    fails(mirror, got, "clear hits lost")
    # a false hit, the neighbouring object, a t beyond the bar
    got = records_of(orc, mirror)
    got["hit"][np.flatnonzero(ref["kind"] == ar.MISS)[0]] = 1
    fails(mirror, got, "hits on clear misses")
    got = records_of(orc, mirror)
    got["obj"][np.flatnonzero(hit)[5]] += 1
    fails(mirror, got, "obj")
    got = records_of(orc, mirror)
    k = np.flatnonzero(hit)[7]
    got["t"][k] = np.float32(ref["t"][k] * (1.0 + 3e-4) + 1.5e-4)     # 1.5 bars
    fails(mirror, got, "")
    # normals taken through A instead of A^-T: the same for a similarity, wrong for a stretch
    for c, wrong in ((mirror, False), (ell, True)):
        got = records_of(orc, c)
        r = c.ref
        h = np.flatnonzero(r["kind"] == ar.HIT)
        a = c.matrices.reshape(-1, 3, 4)[:, :, :3].astype(np.float64)[r["inst"][h]]
        n = np.einsum("kij,klj,kl->ki", a, a, r["n"][h])          # A A^T n
        got["n"][h] = n / np.linalg.norm(n, axis=1, keepdims=True)
        if wrong:
            fails(c, got, "")
        else:
            ar.check_closest(c, got)
