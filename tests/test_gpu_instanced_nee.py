"""Next-event estimation and MIS (PT_RENDER_NEE, PT_RENDER_MIS) on instanced scenes built with
PT_BVH_LIGHTS: the world-space light list per (instance, emissive triangle) and the instanced
NEE / MIS instantiations of the wide kernel.

The bars are the project's own.  An identity instance is the flat scene bit for bit, so the pinned flat
references of tests/pathloop_nee.py and tests/pathloop_mis.py hold the instanced frames; the light
records are held bit for bit to the float64 restatement of tests/instanced_lights_ref.py; transformed
instances are held to the flattened scene within test_instanced_render_close_to_flattened's tolerance
and to the blind integrator's expectation; a rebuilt scene is a fresh scene bit for bit.
Without the feature PT_BVH_LIGHTS is ignored, the scene lists no light and refuses the render flags.
"""
import numpy as np
import pytest

import instanced_lights_ref as ilr
import pathloop_mis as pm
import pathloop_nee as pn
from pathloop import SEED

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def instanced(pt, gpu, ip, flags):
    s = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, ip.instances, ip.materials, device=gpu, flags=flags)
    s.set_sky(*ip.sky)
    return s


def lamp(pt, gpu, flags, inst=None):
    objs, first, count, inst0, mats = ilr.lamp_scene()
    s = pt.Scene.instanced(objs, first, count, inst0 if inst is None else inst, mats, device=gpu, flags=flags)
    s.set_sky((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    return s


def lamp_camera(pt, aspect=1.0):
    return pt.camera_make(np.array(ilr.LAMP_CAMERA_FROM, np.float32), np.array(ilr.LAMP_CAMERA_AT, np.float32),
                          ilr.LAMP_CAMERA_VFOV, aspect)


@pytest.fixture(scope="module")
def n1(pt, gpu):
    """InstancedPreset("cornell_lit", 24, 24) built with PT_BVH_LIGHTS, and its camera."""
    ip = pt.InstancedPreset("cornell_lit", 24, 24)
    return instanced(pt, gpu, ip, pt.PT_BVH_LIGHTS), ip.camera


# ---------------------------------------------------------------- 1. identity instance = the pinned flat frame
@pytest.mark.parametrize("mis", [False, True], ids=["nee", "mis"])
def test_identity_instance_is_the_flat_frame(pt, gpu, n1, mis):
    s, cam = n1
    sc = pn.nee_scene("N1")
    assert s.n_lights == 2
    np.testing.assert_array_equal(bits(s.lights()), bits(ilr.records(pn.light_list(sc.objects, sc.materials))))
    ref = pm.mis_reference("N1")[0] if mis else pn.nee_reference("N1")[0]
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth, nee=not mis, mis=mis)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"] and st.paths == ref["paths"]
    sref = pm.mis_reference_sample("N1") if mis else pn.nee_reference_sample("N1")
    srgb, sst = pt.render(s, f, cam, 5, sc.max_depth, rng=pt.RNG_SAMPLE, chunk=2, nee=not mis, mis=mis)
    np.testing.assert_array_equal(bits(srgb), bits(sref["image"]))
    assert sst.rays == sref["rays"] and sst.paths == sref["paths"]


# ---------------------------------------------------------------- 2. transformed lights: the records
def test_transformed_light_records(pt, gpu):
    """Five placements of one emissive quad -- identity, rotation x uniform scale, mirror, stretch, shear,
    translations of order 10 -- against the rule written out: each world coordinate
    ((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3] in float64, rounded to float32 once, the edges
    float32 differences of the rounded vertices (instanced_lights_ref.world_vertex / light_list)."""
    objs, first, count, inst, mats = ilr.lamp_scene()
    s = lamp(pt, gpu, pt.PT_BVH_LIGHTS)
    assert s.n_lights == 10
    got = s.lights()
    assert got.shape == (10, 4, 3) and got.dtype == np.float32
    np.testing.assert_array_equal(bits(got), bits(ilr.records(ilr.light_list(objs, first, count, inst, mats))))
    assert np.linalg.det(inst["m"][2].reshape(3, 4)[:, :3].astype(np.float64)) < 0   # (the mirror is one)
    # the same scene laid out for updates lists the same records
    s2 = lamp(pt, gpu, pt.PT_BVH_LIGHTS | pt.PT_BVH_WIDE_DEVICE)
    np.testing.assert_array_equal(bits(s2.lights()), bits(got))


# ---------------------------------------------------------------- 3. the same expectation
STAT_W = STAT_H = 16
STAT_DEPTH = 8
STAT_SEEDS = tuple(range(101, 109))
STAT_SPP = 64


@pytest.fixture(scope="module")
def lamp_lit(pt, gpu):
    return lamp(pt, gpu, pt.PT_BVH_LIGHTS), lamp_camera(pt)


def _stat_frames(pt, gpu, scene, spp, **kw):
    """Linear images (the output squared), one per film seed: float64 (8, npix, 3)."""
    s, cam = scene
    out = []
    for seed in STAT_SEEDS:
        f = pt.Film(STAT_W, STAT_H, seed, device=gpu)
        rgb, _ = pt.render(s, f, cam, spp, STAT_DEPTH, rng=pt.RNG_SAMPLE, **kw)
        out.append(rgb.astype(np.float64) ** 2)
    return np.array(out)


def test_instanced_nee_and_mis_have_the_blind_expectation(pt, gpu, lamp_lit):
    """The lamp scene, 16 x 16, depth 8, sample mode, black sky, eight film seeds a side: blind, NEE and
    MIS, all instanced.  Per channel the difference of the NEE (and MIS) mean image mean from the blind
    one lies within 4 standard errors of that difference, each side's standard error from its own eight
    seeds' spread (test_nee_has_the_blind_integrators_expectation's statistic); teeth: every side's
    standard error is below 5 % of its mean.
    64 spp, chosen on the GPU from a ladder of 16 to 2048: the blind side's standard error over its mean
    is 1.6 % at 16 spp, 0.74 % at 64, 0.40 % at 128 -- 64 is the first rung with more than five times the
    room the 5 % condition asks for, and there 4 standard errors of the difference are 3.9 % of the mean,
    so a rule that lost or double-counted a few percent of the light fails (the three channels are
    proportional in this scene -- grey walls, one lamp colour -- so they are one check, not three).
    Measured at 64 spp: blind 0.98526 / 0.69548 / 0.23183, NEE 0.98469 / 0.69508 / 0.23169 (standard
    error 0.65 % of the mean, difference -0.06 standard errors), MIS 0.98539 / 0.69557 / 0.23186 (0.63 %,
    +0.01).  At 2048 spp the differences are -0.05 and +0.06 standard errors of 0.18 % of the mean."""
    blind = _stat_frames(pt, gpu, lamp_lit, STAT_SPP).mean(axis=1)   # (8, 3) image means
    n = len(STAT_SEEDS)
    se_b = np.sqrt(blind.var(0, ddof=1) / n)
    print("spp", STAT_SPP, "blind means", blind.mean(0), "standard error / mean", se_b / blind.mean(0))
    assert (se_b < 0.05 * blind.mean(0)).all()
    for kw in ({"nee": True}, {"mis": True}):
        side = _stat_frames(pt, gpu, lamp_lit, STAT_SPP, **kw).mean(axis=1)
        se_s = np.sqrt(side.var(0, ddof=1) / n)
        diff = side.mean(0) - blind.mean(0)
        se = np.sqrt(se_b ** 2 + se_s ** 2)
        print(kw, "means", side.mean(0), "difference", diff, "standard error", se, "difference / se", diff / se)
        assert (se_s < 0.05 * side.mean(0)).all()
        assert (np.abs(diff) <= 4 * se).all(), (kw, diff, se)


def test_instanced_nee_has_less_noise(pt, gpu, lamp_lit):
    """The same scene at 16 spp, eight seeds: the mean per-pixel variance across seeds (of the linear
    values) is lower with NEE than blind.  No threshold.  Measured: blind 0.2932, NEE 0.2154, a ratio of 1.36 (MIS: 0.1907,
    1.54)."""
    blind = _stat_frames(pt, gpu, lamp_lit, 16)
    nee = _stat_frames(pt, gpu, lamp_lit, 16, nee=True)
    vb, vn = blind.var(0, ddof=1).mean(), nee.var(0, ddof=1).mean()
    print("mean per-pixel variance: blind", vb, "NEE", vn, "ratio", vb / vn)
    assert vn < vb


# ---------------------------------------------------------------- 4. instanced against flattened
@pytest.mark.parametrize("mis", [False, True], ids=["nee", "mis"])
def test_instanced_close_to_flattened(pt, gpu, mis):
    """bunny_cornell_lit, 64 x 64, 8 spp, sample mode, seed 7: the instanced scene (with the list) against
    the flat preset, both with the render flag; test_instanced_render_close_to_flattened's bars."""
    w = h = 64
    ip, fp = pt.InstancedPreset("bunny_cornell_lit", w, h), pt.Preset("bunny_cornell_lit", w, h)
    si = instanced(pt, gpu, ip, pt.PT_BVH_LIGHTS)
    sf = pt.Scene(fp.objects, fp.materials, device=gpu)
    sf.set_sky(*fp.sky)
    assert si.n_lights == sf.n_lights > 0
    kw = dict(kernel=pt.KERNEL_WIDE, rng=pt.RNG_SAMPLE, nee=not mis, mis=mis)
    ri, sti = pt.render(si, pt.Film(w, h, 7, device=gpu), ip.camera, 8, ip.max_depth, **kw)
    rf, stf = pt.render(sf, pt.Film(w, h, 7, device=gpu), fp.camera, 8, fp.max_depth, **kw)
    assert np.isfinite(ri).all()
    mi, mf = ri.mean(0), rf.mean(0)
    assert (np.abs(mi - mf) <= 0.01 * mf + 1e-4).all(), (mi, mf)
    assert (np.abs(ri - rf).mean(0) <= 0.02).all(), np.abs(ri - rf).mean(0)
    assert abs(sti.rays - stf.rays) <= 0.01 * stf.rays


# ---------------------------------------------------------------- 5. lights follow update_instances
def test_lights_follow_update_instances(pt, gpu):
    objs, first, count, inst, mats = ilr.lamp_scene()
    flags = pt.PT_BVH_WIDE_DEVICE | pt.PT_BVH_LIGHTS
    s = lamp(pt, gpu, flags)
    before = s.lights()
    moved = ilr.moved_instances(inst)
    s.update_instances(moved[1:2], first=1)
    s.update_instances(moved[3:4], first=3)
    with pytest.raises(pt.PtError) as e:
        s.lights()
    assert e.value.code == 6   # stale
    s.build_bvh(flags)
    s.build_bvh(flags)
    assert s.wide_info()["source"] == 4
    fresh = lamp(pt, gpu, flags, inst=moved)
    assert fresh.wide_info()["source"] == 3 and s.n_lights == fresh.n_lights == 10
    got = s.lights()
    np.testing.assert_array_equal(bits(got), bits(fresh.lights()))
    np.testing.assert_array_equal(bits(got), bits(ilr.records(ilr.light_list(objs, first, count, moved, mats))))
    assert (bits(got) != bits(before)).any()
    cam = lamp_camera(pt)
    for kw in (dict(rng=pt.RNG_SAMPLE, nee=True), dict(mis=True)):
        frames = []
        for scene in (s, fresh):
            f = pt.Film(16, 16, 3, device=gpu)
            rgb, st = pt.render(scene, f, cam, 4, 8, **kw)
            frames.append((rgb, st.rays, f.get_rng()))
        np.testing.assert_array_equal(bits(frames[0][0]), bits(frames[1][0]), err_msg=str(kw))
        assert frames[0][1] == frames[1][1]
        np.testing.assert_array_equal(frames[0][2], frames[1][2])
        assert frames[0][0].max() > 0
    # a later build without the bit lists none, and the flags are refused as on any instanced scene
    s.build_bvh(pt.PT_BVH_WIDE_DEVICE)
    assert s.wide_info()["source"] == 4 and s.n_lights == 0 and s.lights().shape == (0, 4, 3)
    f = pt.Film(16, 16, 3, device=gpu)
    out = np.full((f.n_pixels, 3), -7.0, np.float32)
    with pytest.raises(pt.PtError) as e:
        pt.render(s, f, cam, 1, 4, out=out, nee=True)
    assert e.value.code == 1 and "instanced" in str(e.value)
    assert (out == -7.0).all()
    pt.render(s, f, cam, 1, 4, out=out)
    assert (out >= 0.0).all()
    s.build_bvh(flags)   # and with it again: the list is back, from the same tables
    np.testing.assert_array_equal(bits(s.lights()), bits(got))


# ---------------------------------------------------------------- 6. scheduling independence
@pytest.mark.parametrize("rng", ["sample", "compat"])
def test_instanced_mis_frame_independent_of_scheduling(pt, gpu, rng):
    """bunny_cornell_lit instanced, 48 x 32, 4 spp, MIS: other LEAF / SHADE thresholds, the identity
    launch order and a 2-way partition of 8-row stripes give the same bits and rays
    (test_instanced_frame_independent_of_scheduling's form)."""
    w, h, spp = 48, 32, 4
    ip = pt.InstancedPreset("bunny_cornell_lit", w, h)
    s = instanced(pt, gpu, ip, pt.PT_BVH_LIGHTS)
    r = pt.RNG_SAMPLE if rng == "sample" else pt.RNG_COMPAT

    def frame(film_kw=None, **kw):
        f = pt.Film(w, h, 7, device=gpu, **(film_kw or {}))
        img, st = pt.render(s, f, ip.camera, spp, ip.max_depth, kernel=pt.KERNEL_WIDE, rng=r, mis=True, **kw)
        return img, st, f

    a, sa, _ = frame()
    blind, _ = pt.render(s, pt.Film(w, h, 7, device=gpu), ip.camera, spp, ip.max_depth, kernel=pt.KERNEL_WIDE, rng=r)
    assert (bits(a) != bits(blind)).any()
    for kw in ({"leaf_batch": 5, "shade_batch": 40}, {"leaf_batch": 40, "shade_batch": 6},
               {"flags": pt.IDENTITY_ORDER}):
        b, sb, _ = frame(**kw)
        np.testing.assert_array_equal(bits(b), bits(a), err_msg=str(kw))
        assert sb.rays == sa.rays, kw
    full = a.reshape(h, w, 3)
    rays = 0
    for part in (0, 1):
        img, st, f = frame({"stripe_height": 8, "n_parts": 2, "part": part})
        np.testing.assert_array_equal(bits(img.reshape(-1, w, 3)), bits(full[f.rows]))
        rays += st.rays
    assert rays == sa.rays


# ---------------------------------------------------------------- 7. no sampled light: nothing changes
@pytest.mark.parametrize("rng", ["compat", "sample"])
def test_bit_without_lights_changes_nothing(pt, gpu, rng):
    w, h = 32, 32
    ip = pt.InstancedPreset("cornell", w, h)
    s = instanced(pt, gpu, ip, pt.PT_BVH_LIGHTS)
    assert s.n_lights == 0 and s.lights().shape == (0, 4, 3)
    mode = pt.RNG_COMPAT if rng == "compat" else pt.RNG_SAMPLE
    frames = []
    for kw in ({}, {"nee": True}, {"mis": True}):
        f = pt.Film(w, h, 9, device=gpu)
        rgb, st = pt.render(s, f, ip.camera, 4, 12, kernel=pt.KERNEL_WIDE, rng=mode, chunk=2, **kw)
        frames.append((rgb, f.get_rng(), (st.rays, st.paths, st.node_visits, st.tri_tests, st.sphere_tests)))
    for fr in frames[1:]:
        np.testing.assert_array_equal(bits(fr[0]), bits(frames[0][0]))
        np.testing.assert_array_equal(fr[1], frames[0][1])
        assert fr[2] == frames[0][2]


# ---------------------------------------------------------------- 8. rules
def test_rules(pt, orc, gpu, n1):
    s, cam = n1
    sc = pn.nee_scene("N1")
    for k in (pt.KERNEL_SIMPLE, pt.KERNEL_WAVEFRONT):
        for kw in ({}, {"nee": True}, {"mis": True}):
            f = pt.Film(sc.width, sc.height, SEED, device=gpu)
            out = np.full((f.n_pixels, 3), -7.0, np.float32)
            with pytest.raises(pt.PtError) as e:
                pt.render(s, f, cam, 1, 4, out=out, kernel=k, **kw)
            assert e.value.code == 1 and (out == -7.0).all()
    ip = pt.InstancedPreset("cornell_lit", 24, 24)
    unbuilt = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, ip.instances, ip.materials, device=gpu,
                                 build=False)
    buf = np.full(24, -7.0, np.float32)
    assert pt.lib.pt_scene_download_lights(unbuilt.h, buf.ctypes.data) == 6
    assert "pt_scene_download_lights" in pt.lib.pt_last_error().decode() and (buf == -7.0).all()
    assert pt.lib.pt_scene_download_lights(s.h, None) == 1   # NULL records with nL > 0
    # the flat path of the new call
    s2 = pn.nee_scene("N2")
    flat = pt.Scene(s2.objects, s2.materials, device=gpu)
    np.testing.assert_array_equal(bits(flat.lights()), bits(ilr.records(pn.light_list(s2.objects, s2.materials))))
    assert pt.Scene(s2.objects, s2.materials, device=gpu, flags=pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_LIGHTS).n_lights \
        == flat.n_lights == 9   # (ignored on a flat scene)


def test_two_accumulated_nee_frames(pt, orc, gpu, n1):
    """test_nee_two_accumulated_frames' form on the identity-instanced N1."""
    s, cam = n1
    sc = pn.nee_scene("N1")
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    refs = pn.nee_reference("N1", spp=2, frames=2)
    want = orc.accumulate([r["sums"] for r in refs], [2, 2])
    for k in range(2):
        rgb, st = pt.render(s, f, cam, 2, sc.max_depth, accumulate=True, nee=True)
        np.testing.assert_array_equal(bits(rgb), bits(want[k]))
        assert st.rays == refs[k]["rays"]
    np.testing.assert_array_equal(f.get_rng(), refs[-1]["states"])
    assert f.accumulated == 4


def test_rgba8_output(pt, orc, gpu, n1):
    s, cam = n1
    sc = pn.nee_scene("N1")
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    q, _ = pt.render(s, f, cam, sc.spp, sc.max_depth, out_format=pt.OUT_RGBA8, nee=True)
    np.testing.assert_array_equal(q, orc.quantize_png(pn.nee_reference("N1")[0]["image"]))
