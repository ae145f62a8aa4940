"""CPU tests of the oracle's nan_miss mode (oracle.trace(..., nan_miss=True)): the reference's closest
hit with the library's one change, "a candidate whose t is NaN is not a hit" (include/pt.h,
pt_trace_closest), on the degenerate ray classes of degenerate_rays.py.

With the mode off the oracle is the reference as before: its records on every class and interval are
pinned by tests/golden/degenerate_rays_reference.json, SHA-256 digests recorded from the oracle as it
was before the mode existed.

Reference counts on random_soup(300, 60, seed=1), mode off, the 2048-ray base batch:
  NaN-t hits, directions x1e18, tmin 0: 655      +inf-t hits, directions x1e-30: 564
  negative-t hits at tmin -5: 237                hits among the ordinary rays: 1459
Mode on, hits per class of 256 rays, interval (0.001, inf) / (0, inf) (every other interval of
degenerate_rays.INTERVALS: 0 hits in every class):
  control 186 / 186      d_1e-42 255 / 255 (all at t = +inf)      d_1e18  0 / 136
  d_1e-38 200 / 200 (79 at +inf)      d_1e-30 198 / 198 (67 at +inf)      d_1e30  0 / 131
  o_1e6_aimed 89 / 89 (the brute-force loop, which has no boxes, reports 167 other records)
  every NaN, infinity and zero-direction class and the un-aimed far origins: 0 / 0
(mode off, the same classes report up to 256 "hits" whose t is NaN.)
"""
import hashlib
import json
import os

import numpy as np
import pytest

import degenerate_rays as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "degenerate_rays_reference.json")


class Soup:
    def __init__(self, orc):
        self.objs, _ = dr.soup()
        self.nodes = orc.build_lbvh(self.objs, orc.morton_keys(self.objs), tight=True)
        self.base = dr.base_rays(self.objs)
        self.classes = dr.ray_classes(self.objs, self.base)


@pytest.fixture(scope="module")
def soup(orc):
    return Soup(orc)


def key(name, interval):
    return f"{name} [{interval[0]!r}, {interval[1]!r}]"


def test_mode_off_is_the_reference_as_recorded(orc, soup):
    golden = json.load(open(GOLDEN))
    assert orc.bvh_depth(soup.nodes, len(soup.objs)) == 13
    seen = 0
    for interval in dr.INTERVALS + [(-5.0, np.inf), (0.001, np.nan)]:
        for name, rays in soup.classes.items():
            for brute in (False, True):
                h, _ = orc.trace(soup.objs, soup.nodes, rays, *interval, brute=brute)
                k = key(name, interval) + (" brute" if brute else "")
                assert hashlib.sha256(h.tobytes()).hexdigest() == golden[k], k
                seen += 1
    assert seen == len(golden)


def test_mode_on_nan_rays_miss(orc, soup):
    miss = np.zeros(1, orc.HIT_DTYPE)
    miss["obj"] = miss["mat"] = -1
    for interval in dr.INTERVALS:
        for name in dr.nan_classes():
            off, _ = orc.trace(soup.objs, soup.nodes, soup.classes[name], *interval)
            for brute in (False, True):
                on, _ = orc.trace(soup.objs, soup.nodes, soup.classes[name], *interval, brute=brute, nan_miss=True)
                assert (on == miss).all(), (name, interval, brute)
            if interval[0] <= interval[1]:   # the reference does report these: the mode matters
                assert (off["hit"] == 1).sum() > 0 and np.isnan(off["t"][off["hit"] == 1]).all(), (name, interval)


def test_mode_on_never_returns_a_nan_t(orc, soup):
    for interval in dr.INTERVALS:
        for name, rays in soup.classes.items():
            for brute in (False, True):
                on, _ = orc.trace(soup.objs, soup.nodes, rays, *interval, brute=brute, nan_miss=True)
                assert not np.isnan(on["t"][on["hit"] == 1]).any(), (name, interval, brute)
                assert set(np.unique(on["hit"])) <= {0, 1}


def test_mode_on_keeps_ordinary_rays(orc, soup):
    for rays in (soup.base, soup.classes["control"]):
        for interval in dr.INTERVALS:
            for brute in (False, True):
                off, _ = orc.trace(soup.objs, soup.nodes, rays, *interval, brute=brute)
                on, _ = orc.trace(soup.objs, soup.nodes, rays, *interval, brute=brute, nan_miss=True)
                assert off.tobytes() == on.tobytes(), (interval, brute)


def test_classes_show_what_they_are_for(orc, soup):
    """Conditions, not measurements: each class meets the case it was built for (the counts measured
    when this was written are in the module docstring)."""
    def trace(rays, tmin, tmax=np.inf, **kw):
        return orc.trace(soup.objs, soup.nodes, rays, tmin, tmax, **kw)[0]

    def hits(h):
        return h["hit"] == 1

    names = {1e18: "d_1e18", 1e-30: "d_1e-30"}
    for rays_of in (lambda f: dr.scaled(soup.base, 3, f), lambda f: soup.classes[names[f]]):
        h = trace(rays_of(1e18), 0.0)
        nan_t = int((hits(h) & np.isnan(h["t"])).sum())
        h = trace(rays_of(1e-30), 0.001)
        inf_t = int((hits(h) & np.isposinf(h["t"])).sum())
        print(f"x1e18 at tmin 0: {nan_t} NaN-t hits; x1e-30: {inf_t} +inf-t hits")
        assert nan_t > 0 and inf_t > 0
    for rays in (soup.base, soup.classes["control"]):
        h = trace(rays, -5.0)
        neg = int((hits(h) & (h["t"] < 0)).sum())
        h = trace(rays, 0.001)
        print(f"tmin -5: {neg} negative-t hits; ordinary rays: {int(hits(h).sum())} of {len(rays)} hit")
        assert neg > 0 and 0 < hits(h).sum() < len(rays)
    # the overflowing directions still have real hits under the rule: x1e18 is not a class of misses
    on = trace(soup.classes["d_1e18"], 0.0, nan_miss=True)
    assert hits(on).sum() > 0 and np.isfinite(on["t"][hits(on)]).any()
    # a NaN tmax is no upper bound in the reference
    a, b = trace(soup.base, 0.001, np.nan), trace(soup.base, 0.001, np.inf)
    assert a.tobytes() == b.tobytes()
    # zero directions start both outside and inside spheres
    sph = soup.objs[soup.objs["type"] == 1]
    z = soup.classes["zero_d"]
    inside = (np.linalg.norm(z[:, None, :3] - sph["v"][None, :, :3], axis=2) < np.abs(sph["v"][None, :, 3])).any(1)
    assert inside[1::2].all() and 0 < (~inside).sum()


def test_small_scenes_and_poisoned_batch(orc, soup):
    """The one-primitive scenes have no box test: an empty interval still misses; the helper's mixed
    batch keeps the control rays where it says."""
    for make in (dr.one_sphere, dr.one_triangle):
        objs, _ = make()
        assert len(objs) == 1
        nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
        cl = dr.ray_classes(objs, dr.base_rays(objs, reach=0.75))
        h, _ = orc.trace(objs, nodes, cl["control"], 0.001, np.inf, nan_miss=True)
        assert h["hit"].sum() > 0
        for interval in dr.INTERVALS[2:]:
            for rays in cl.values():
                h, _ = orc.trace(objs, nodes, rays, *interval, nan_miss=True)
                assert h["hit"].sum() == 0
    batch, at = dr.poisoned(soup.classes)
    assert len(batch) == 4 * dr.CLASS_RAYS and np.array_equal(batch[at], soup.classes["control"])
    assert np.isnan(batch[at + 1]).any(axis=1).all() and not batch[at + 2][:, 3:].any()
    rt, plain = dr.mixed_ray_tmax(512)
    assert np.isnan(rt).sum() > 0 and np.isposinf(plain[np.isnan(rt)]).all()
