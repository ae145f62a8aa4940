"""Next-event estimation (PT_RENDER_NEE), host side (no GPU): the Python restatement of the rule
(tests/pathloop_nee.py) against the loop it extends, the conditions the NEE GPU tests' scenes have to
meet (tests/test_gpu_nee.py), the sampling arithmetic's edge cases, and the estimator against a
quadrature that shares no code with it."""
import numpy as np
import pytest

import pathloop
import pathloop_nee as pn
from pathloop import SEED

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, states=True):
    np.testing.assert_array_equal(bits(a["image"]), bits(b["image"]))
    np.testing.assert_array_equal(bits(a["sums"]), bits(b["sums"]))
    if states:
        np.testing.assert_array_equal(a["states"], b["states"])
    assert a["rays"] == b["rays"] and a["paths"] == b["paths"] and a["kinds"] == b["kinds"]


# ---------------------------------------------------------------- 1. the rule off is pathloop
@pytest.mark.parametrize("name", ["L1", "L2"])
def test_nee_off_is_pathloop(name):
    """nee=False: the restatement is pathloop.render / render_sample bit for bit -- image, sums, streams,
    rays, paths and endings.  (pathloop itself is held to the oracle by test_emission_host.py.)"""
    sc = pathloop.lit_scene(name)
    mine = pn.render(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), sc.spp,
                     sc.max_depth, pn.orc.film_states(SEED, sc.width, range(sc.height)), sky=sc.sky, nee=False)
    _same(mine, pathloop.lit_reference(name)[0])
    assert not any(mine["events"].values()) and not mine["shadow"]
    smine = pn.render_sample(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), 5,
                             sc.max_depth, SEED, 2, sky=sc.sky, nee=False)
    _same(smine, pathloop.lit_reference_sample(name), states=False)


def test_nee_without_emissive_triangles_changes_nothing():
    """nL == 0: N2's soup with its emissive triangles given another material (the emitter lives on in
    the soup's emissive spheres, which are not sampled) -- nee=True is nee=False, streams included."""
    sc = pn.nee_scene("N2")
    objs = sc.objects.copy()
    em = int(np.flatnonzero(sc.materials["type"] == pathloop.PT_EMISSIVE)[0])
    objs["mat"][(objs["type"] == pn.PT_TRIANGLE) & (objs["mat"] == em)] = 0
    assert ((objs["type"] == 1) & (objs["mat"] == em)).any(), "an emissive sphere must remain"
    assert len(pn.light_list(objs, sc.materials)[0]) == 0
    nodes = pn.orc.build_lbvh(objs, pn.orc.morton_keys(objs), tight=True)
    res = []
    for nee in (False, True):
        st = pn.orc.film_states(SEED, sc.width, range(sc.height))
        res.append(pn.render(objs, sc.materials, nodes, sc.camera, sc.width, sc.height, range(sc.height), sc.spp,
                             sc.max_depth, st, sky=sc.sky, nee=nee))
    _same(res[1], res[0])
    assert any(k == pathloop.EMITTER for k, _ in res[1]["kinds"])
    sres = [pn.render_sample(objs, sc.materials, nodes, sc.camera, sc.width, sc.height, range(sc.height), 5,
                             sc.max_depth, SEED, 2, sky=sc.sky, nee=nee) for nee in (False, True)]
    _same(sres[1], sres[0], states=False)


# ---------------------------------------------------------------- 2. what the NEE scenes show
def _shown(events):
    return {k for k, v in events.items() if v > 0}


def test_nee_scenes_show_every_case_but_clamped():
    """The references the GPU tests compare with (compat and sample mode): N1 and N2 together show
    every event of the rule except `clamped`, which neither shows in any of them."""
    n1, n2 = pn.nee_reference("N1")[0], pn.nee_reference("N2")[0]
    assert _shown(n1["events"]) == {"direct_unoccluded", "direct_occluded", "direct_backfacing", "emitter_suppressed"}
    assert _shown(n2["events"]) == set(pn.EVENTS) - {"clamped"}
    assert pathloop.ending_kinds(n2["kinds"]) == pathloop.ALL_ENDINGS
    for name in ("N1", "N2"):
        for r in (pn.nee_reference(name)[0], pn.nee_reference_sample(name)):
            assert r["events"]["clamped"] == 0
            assert len(r["shadow"]) == r["events"]["direct_unoccluded"] + r["events"]["direct_occluded"] > 0
        # the rule changed the frame, and spent rays on it
        off = pn.nee_reference(name, nee=False)[0]
        on = pn.nee_reference(name)[0]
        assert (bits(on["image"]) != bits(off["image"])).any() and on["rays"] > off["rays"]
        assert on["paths"] == off["paths"]
    sc = pn.nee_scene("N2")
    assert len(pn.light_list(sc.objects, sc.materials)[0]) == 9
    assert ((sc.objects["type"] == 1) & (sc.materials["type"][sc.objects["mat"]] == 8)).sum() == 3


def test_clamp_scene_clamps():
    sc = pn.clamp_scene()
    st = pn.orc.film_states(3, sc.width, range(sc.height))
    r = pn.render(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), sc.spp,
                  sc.max_depth, st, sky=sc.sky, nee=True)
    assert r["events"]["clamped"] > 0 and r["events"]["direct_unoccluded"] > 0
    assert r["sums"].max() <= sc.spp * 1024.0   # no sample above PT_MAX_RADIANCE
    # a clamped sample is exactly 1024 in the clamped channel: some pixel's sum holds one
    assert (r["sums"] >= 1024.0).any()


# ---------------------------------------------------------------- 3. the sampling arithmetic
def test_folded_points_lie_inside_their_triangle():
    """Barycentrics >= 0 and their sum <= 1 in float64, for random pairs and for the pairs whose fp32 sum
    rounds to exactly 1 from above (the fold alone leaves those 2^-24 outside; the two minima of the
    rule bring them onto the edge)."""
    rng = np.random.default_rng(5)
    u = rng.random((4000, 2)).astype(F)
    u[:8] = [(1, 1), (1, 0), (0, 1), (0.5, 0.5), (F(2.0 ** -24), 1), (1, F(2.0 ** -24)), (0.75, 0.25), (1, 0.5)]
    u[8:12] = [(F(0.25 + 2.0 ** -26), 0.75), (0.75, F(0.25 + 2.0 ** -26)), (F(0.25 + 2.0 ** -26), F(0.75 + 2.0 ** -24)),
               (F(2.0 ** -33), 1)]
    for ua, ub in u:   # curand_uniform's range is (0, 1]
        if ua == 0 or ub == 0:
            continue
        a, b = pn.fold(ua, ub)
        assert float(a) >= 0.0 and float(b) >= 0.0 and float(a) + float(b) <= 1.0, (ua, ub, a, b)


def test_light_index_stays_in_range():
    for nL in (1, 2, 3, 9, 1000, 2 ** 24 + 1):
        assert pn.pick_light(F(1.0), nL) == nL - 1
        assert pn.pick_light(F(2.0 ** -24), nL) in (0, 1)
        assert 0 <= pn.pick_light(F(0.99999994), nL) <= nL - 1


def test_light_list_order_and_records():
    sc = pn.nee_scene("N1")
    v0, e1, e2, E = pn.light_list(sc.objects, sc.materials)
    lamp = np.flatnonzero(sc.materials["type"][sc.objects["mat"]] == 8)
    assert len(v0) == len(lamp) == 2
    for k, i in enumerate(lamp):
        v = sc.objects["v"][i]
        np.testing.assert_array_equal(v0[k], v[0:3])
        np.testing.assert_array_equal(bits(e1[k]), bits((v[3:6] - v[0:3]).astype(F)))
        np.testing.assert_array_equal(bits(e2[k]), bits((v[6:9] - v[0:3]).astype(F)))
        np.testing.assert_array_equal(E[k], np.array([17, 12, 4], F))


# ---------------------------------------------------------------- 4. the estimator against a quadrature
def test_direct_term_mean_equals_the_form_factor_integral():
    """One emissive triangle over a Lambertian point, no occluder.  The rule's direct term, averaged over
    N samples of a XORWOW stream, against a float64 midpoint quadrature of
        (albedo / pi) * E * integral over the triangle of cos_s cos_l / d^2 dA
    (no code shared: the quadrature knows nothing of G, the fold or the cross product's length).
    Bound: 4 standard errors, the standard error from the samples themselves.  N = 20,000: about a
    second of Python."""
    tri = np.array([[-0.6, 1.0, -0.4], [0.9, 1.3, -0.2], [0.1, 0.8, 0.7]], F)
    lights = (tri[0:1].copy(), (tri[1:2] - tri[0:1]).astype(F), (tri[2:3] - tri[0:1]).astype(F), np.array([[5, 3, 2]], F))
    p, n, albedo = np.array([0.1, 0.0, 0.05], F), np.array([0.0, 1.0, 0.0], F), np.array([0.8, 0.5, 0.25], F)
    N = 20000
    state = pn.orc.sample_stream(12345, 0, 7)
    u = pn.orc.curand_uniform(state, 3 * N).reshape(N, 3)
    terms = np.zeros((N, 3), np.float64)
    for i in range(N):
        go, _, t = pn.light_sample(lights, p, n, albedo, u[i, 0], u[i, 1], u[i, 2])
        assert go   # the whole triangle is above the point and faces it
        terms[i] = t
    # quadrature: m^2 congruent subtriangles, the integrand at their centroids
    m = 300
    T = tri.astype(np.float64)
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    up = (i + j < m)
    cu = np.concatenate([((i + 1 / 3) / m)[up], ((i + 2 / 3) / m)[i + j < m - 1]])
    cv = np.concatenate([((j + 1 / 3) / m)[up], ((j + 2 / 3) / m)[i + j < m - 1]])
    assert len(cu) == m * m
    q = T[0] + cu[:, None] * (T[1] - T[0]) + cv[:, None] * (T[2] - T[0])
    nl = np.cross(T[1] - T[0], T[2] - T[0])
    area = 0.5 * np.linalg.norm(nl)
    nl /= np.linalg.norm(nl)
    w = q - p.astype(np.float64)
    d = np.linalg.norm(w, axis=1)
    integrand = (w @ n.astype(np.float64) / d) * np.abs(w @ nl / d) / d ** 2
    integral = integrand.mean() * area
    want = albedo.astype(np.float64) / np.pi * lights[3][0].astype(np.float64) * integral
    mean, se = terms.mean(0), terms.std(0, ddof=1) / np.sqrt(N)
    print("mean", mean, "quadrature", want, "standard error", se, "deviation / se", (mean - want) / se)
    assert (np.abs(mean - want) <= 4 * se).all(), (mean, want, se)
    assert (se < 0.02 * want).all()   # (the check has teeth: a standard error of 2 % at most)


def test_binding_constants(pt):
    assert pt.NEE == 4 and "pt_scene_light_count" in pt.EXPORTS
