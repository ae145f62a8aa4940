"""Next-event estimation with multiple importance sampling (PT_RENDER_MIS), host side (no GPU): the
Python restatement of the rule (tests/pathloop_mis.py) against the loop it extends
(tests/pathloop_nee.py), the rule's bounds, the agreement of its two pdfs, and its expectation against
the blind integrator's where plain NEE's clamp is biased."""
import functools

import numpy as np
import pytest

import pathloop_mis as pm
import pathloop_nee as pn
from pathloop import SEED

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_paths(a, b, states=True):
    if states:
        np.testing.assert_array_equal(a["states"], b["states"])
    assert a["rays"] == b["rays"] and a["paths"] == b["paths"] and a["kinds"] == b["kinds"]
    assert len(a["shadow"]) == len(b["shadow"])
    for (ra, oa), (rb, ob) in zip(a["shadow"], b["shadow"]):
        assert oa == ob and np.array_equal(bits(ra), bits(rb))


# ---------------------------------------------------------------- 1. the weights off is pathloop_nee
@pytest.mark.parametrize("name", ["N1", "N2"])
def test_mis_off_is_pathloop_nee(name):
    """mis=False: pathloop_nee.render / render_sample bit for bit -- image, sums, streams, rays, paths,
    endings, events and shadow rays -- with the rule on and with it off."""
    for nee in (True, False):
        mine, ref = pm.mis_reference(name, nee=nee, mis=False)[0], pn.nee_reference(name, nee=nee)[0]
        np.testing.assert_array_equal(bits(mine["image"]), bits(ref["image"]))
        np.testing.assert_array_equal(bits(mine["sums"]), bits(ref["sums"]))
        _same_paths(mine, ref)
        assert mine["events"] == ref["events"]
    smine, sref = pm.mis_reference_sample(name, mis=False), pn.nee_reference_sample(name)
    np.testing.assert_array_equal(bits(smine["image"]), bits(sref["image"]))
    np.testing.assert_array_equal(bits(smine["sums"]), bits(sref["sums"]))
    _same_paths(smine, sref, states=False)
    assert smine["events"] == sref["events"]


# ---------------------------------------------------------------- 2. the weights on: the same paths
@pytest.mark.parametrize("name", ["N1", "N2"])
def test_mis_traces_the_nee_frames_paths(name):
    """mis=True: the NEE reference's streams, rays, paths, endings and shadow rays exactly; another image.
    nee=False with mis=True is the same frame (the bit implies the rule)."""
    mine, ref = pm.mis_reference(name)[0], pn.nee_reference(name)[0]
    _same_paths(mine, ref)
    assert {k: v for k, v in mine["events"].items() if k != "clamped"} == \
           {k: v for k, v in ref["events"].items() if k != "clamped"}
    assert (bits(mine["image"]) != bits(ref["image"])).any()
    assert (bits(mine["image"]) != bits(pn.nee_reference(name, nee=False)[0]["image"])).any()
    alone = pm.mis_reference(name, nee=False, mis=True)[0]
    np.testing.assert_array_equal(bits(alone["image"]), bits(mine["image"]))
    np.testing.assert_array_equal(alone["states"], mine["states"])
    smine, sref = pm.mis_reference_sample(name), pn.nee_reference_sample(name)
    _same_paths(smine, sref, states=False)
    assert (bits(smine["image"]) != bits(sref["image"])).any()


# ---------------------------------------------------------------- 3. bounds
@functools.lru_cache(maxsize=None)
def _clamp_run():
    """clamp_scene() in sample mode, seed 5, 64 spp (4,096 samples; 512 spp show 285 clamped of 32,768)."""
    sc = pn.clamp_scene()
    return pm.render_sample(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), 64,
                            sc.max_depth, 5, 64, sky=sc.sky, mis=True)


def test_mis_weights_and_terms_are_bounded():
    """0 <= wl, wb <= 1 and every light term <= (att * albedo) * E per channel, over every light sample and
    weighted emitter hit of N1, N2, the rim scene and clamp_scene(); both kinds occur."""
    runs = [pm.mis_reference("N1")[0], pm.mis_reference("N2")[0], pm.mis_reference_sample("N1"),
            pm.mis_reference_sample("N2"), _rim_runs()["mis"][0], _clamp_run()]
    kinds = set()
    n = 0
    for r in runs:
        for kind, wt, term, bound in r["weights"]:
            kinds.add(kind)
            n += 1
            assert 0.0 <= float(wt) <= 1.0, (kind, wt)
            assert (term >= 0).all() and (term <= bound).all(), (kind, wt, term, bound)
    assert kinds == {"light", "emitter"} and n > 1000


def test_mis_clamps_only_where_the_emitter_itself_is_beyond_the_clamp():
    """No clamped sample under the weights in N1, N2 and the rim scene (max E / (1 - max albedo) <
    PT_MAX_RADIANCE in N1 and rim: 17 / 0.27 and 17 / 0.2); clamp_scene(), E = 900 on albedo 0.8, still
    clamps -- the clamp's code path stays tested."""
    for r in (pm.mis_reference("N1")[0], pm.mis_reference("N2")[0], pm.mis_reference_sample("N1"),
              pm.mis_reference_sample("N2"), _rim_runs()["mis"][0]):
        assert r["events"]["clamped"] == 0
    assert _rim_runs()["nee"][0]["events"]["clamped"] > 0   # (what plain NEE does in the rim scene)
    r = _clamp_run()
    assert r["events"]["clamped"] > 0
    assert r["sums"].max() <= 64 * 1024.0


def test_gpu_fixtures_show_the_weighted_emitter_and_the_clamp():
    """What the fixtures of tests/test_gpu_mis.py show: weighted emitter hits in N1, N2 and
    the rim scene, and clamped samples under the weights in the clamp scene."""
    for name in ("N1", "N2", "rim"):
        assert any(k == "emitter" for k, *_ in pm.mis_reference(name)[0]["weights"]), name
    assert pm.mis_reference("clamp")[0]["events"]["clamped"] + pm.mis_reference_sample("clamp")["events"]["clamped"] > 0


# ---------------------------------------------------------------- 4. the two pdfs agree
def test_light_pdf_from_either_side():
    """The light sample's pdf of a direction, as the light sample computes it (pl, from w) and as a scatter
    ray that lands on the light does (pls, from t * d), at N1's shaded points (the origins of its
    reference's shadow rays) and N1's two lights, 400 samples.
    d = w, t = 1: t * d is w exactly, so the two are the same bits (measured and asserted: 0 ulp).
    d = s * w, t = fl(1 / s) for s = 0.37 and 3.3 (the scatter ray has another length than w): t * d
    carries two roundings per component (up to 1.5 ulp relative), D2 and clh follow; measured at most
    6 ulp, asserted with a factor 4: 24 ulp."""
    sc = pn.nee_scene("N1")
    lights = pn.light_list(sc.objects, sc.materials)
    nL = len(lights[0])
    shadow = pm.mis_reference("N1")[0]["shadow"]
    pick = shadow[::max(1, len(shadow) // 400)][:400]
    assert len(pick) >= 300
    u = pn.orc.curand_uniform(pn.orc.sample_stream(77, 0, 3), 2 * len(pick)).reshape(-1, 2)
    worst = 0
    for i, (ray, _) in enumerate(pick):
        p, k = ray[:3].astype(F), i % nL
        ua, ub = pn.fold(u[i, 0], u[i, 1])
        w = (pn.light_point(lights, k, ua, ub) - p).astype(F)
        d2 = pn.dot(w, w)
        cl = F(abs(pn.dot(pn.cross(lights[1][k], lights[2][k]), w)))
        if cl == 0 or d2 == 0:
            continue
        pl = pm.light_pdf(nL, d2, cl)
        assert np.isfinite(pl) and pl > 0

        def pls_of(t, d):
            wv = (F(t) * d).astype(F)
            return pm.light_pdf(nL, pn.dot(wv, wv), F(abs(pn.dot(pn.cross(lights[1][k], lights[2][k]), wv))))
        assert bits(pls_of(1.0, w))[0] == bits(pl)[0]
        for s in (F(0.37), F(3.3)):
            pls = pls_of(F(F(1.0) / s), (s * w).astype(F))
            worst = max(worst, abs(int(bits(pls)[0]) - int(bits(pl)[0])))
    print("largest difference of pls (scaled ray) and pl:", worst, "ulp")
    assert worst <= 24


# ---------------------------------------------------------------- 5. expectation
EXP_SEED, EXP_SPP = 5, 512


def _exp_run(sc, **kw):
    samples = []
    r = pm.render_sample(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), EXP_SPP,
                         sc.max_depth, EXP_SEED, EXP_SPP, sky=sc.sky, samples=samples, **kw)
    return r, np.array(samples, np.float64)


@functools.lru_cache(maxsize=None)
def _rim_runs():
    sc = pm.rim_scene()
    return {"blind": _exp_run(sc), "nee": _exp_run(sc, nee=True), "mis": _exp_run(sc, mis=True)}


def _in_standard_errors(a, b):
    """(mean of a) - (mean of b) per channel, in standard errors of that difference."""
    se = np.sqrt(a.var(0, ddof=1) / len(a) + b.var(0, ddof=1) / len(b))
    return (a.mean(0) - b.mean(0)) / se


def test_mis_has_the_blind_expectation_where_nee_is_biased():
    """The rim scene (the lamp 0.05 above the floor, E = (17, 12, 4)), sample streams, seed 5, 8 x 8, 512 spp,
    depth 3; the statistic is the mean of all 32,768 samples.  MIS - blind lies within 4 standard errors
    of the difference per channel; NEE - blind lies beyond 4 on red, where the clamp cuts the most (the
    teeth: this test tells a biased rule from an unbiased one).  The standard error of the MIS mean is
    the blind integrator's here, a fifth of NEE's."""
    runs = _rim_runs()
    blind, nee, mis = runs["blind"][1], runs["nee"][1], runs["mis"][1]
    zm, zn = _in_standard_errors(mis, blind), _in_standard_errors(nee, blind)
    print("blind mean", blind.mean(0), "NEE mean", nee.mean(0), "MIS mean", mis.mean(0))
    print("MIS - blind", zm, "NEE - blind", zn, "standard errors;  se of the means: blind",
          blind.std(0, ddof=1) / np.sqrt(len(blind)), "NEE", nee.std(0, ddof=1) / np.sqrt(len(nee)), "MIS",
          mis.std(0, ddof=1) / np.sqrt(len(mis)))
    assert len(blind) == len(nee) == len(mis) == 8 * 8 * EXP_SPP
    assert (np.abs(zm) <= 4).all(), zm
    assert abs(zn[0]) > 4, zn
    assert runs["mis"][0]["events"]["clamped"] == 0 and runs["nee"][0]["events"]["clamped"] > 0


def test_mis_has_the_blind_expectation_in_the_open_scene():
    """The open scene (the lamp 1.0 above the floor, a Lambertian blocker halfway, depth 4): nothing near
    the singularity, occluded and unoccluded samples.  MIS - blind within 4 standard errors per channel."""
    sc = pm.open_scene()
    (_, blind), (rm, mis) = _exp_run(sc), _exp_run(sc, mis=True)
    z = _in_standard_errors(mis, blind)
    print("blind mean", blind.mean(0), "MIS mean", mis.mean(0), "MIS - blind", z, "standard errors")
    assert (np.abs(z) <= 4).all(), z
    assert rm["events"]["direct_occluded"] > 0 and rm["events"]["direct_unoccluded"] > 0
    assert rm["events"]["emitter_suppressed"] > 0 and rm["events"]["clamped"] == 0


def test_binding_constants(pt):
    assert pt.MIS == 8 and pt.NEE == 4
    import inspect
    assert "mis" in inspect.signature(pt.render).parameters
