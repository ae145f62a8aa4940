"""Next-event estimation (PT_RENDER_NEE) on the GPU.

The reference of an NEE frame is tests/pathloop_nee.py, the render loop restated in Python with the
rule of include/pt.h added; tests/test_nee_host.py holds that restatement to pathloop.py (the rule
off), to a quadrature (the estimator) and to the list of cases its scenes must show.  The bar is the
project's usual one: bit-exact images, sums, RNG streams and counters, in PT_KERNEL_SIMPLE (the rule
as a nested query) and PT_KERNEL_WIDE (the shadow ray as a query of the step machine).

  N1 = the cornell_lit preset, 24 x 24, 4 spp, depth 8, black sky: 2 sampled lights.
  N2 = a dense soup of triangles and spheres, every material, 9 sampled lights and 3 emissive spheres,
       its own sky, 24 x 16, 3 spp, depth 12.
Without the feature the flag is ignored and every NEE frame below is the blind one: the bit-exact
tests fail there.
"""
import numpy as np
import pytest

import pathloop_nee as pn
from pathloop import SEED

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(params=["simple", "wide"])
def kernel(request, pt):
    return {"simple": pt.KERNEL_SIMPLE, "wide": pt.KERNEL_WIDE}[request.param]


def camera_of(pt, sc):
    return pt.Camera.from_buffer_copy(sc.camera.tobytes())


def device_scene(pt, gpu, sc):
    s = pt.Scene(sc.objects, sc.materials, device=gpu)
    s.set_sky(*sc.sky)
    return s


# ---------------------------------------------------------------- 1. NEE frames, both kernels, both modes
@pytest.mark.parametrize("name", ["N1", "N2"])
def test_nee_frames_bit_exact(pt, gpu, kernel, name):
    sc = pn.nee_scene(name)
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    assert s.n_lights == len(pn.light_list(sc.objects, sc.materials)[0]) > 0
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    ref = pn.nee_reference(name)[0]
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel, nee=True)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"] and st.paths == ref["paths"]
    blind = pn.nee_reference(name, nee=False)[0]
    assert (bits(rgb) != bits(blind["image"])).any()   # (what the parent commit renders under the flag)
    before = f.get_rng()
    sref = pn.nee_reference_sample(name)
    srgb, sst = pt.render(s, f, cam, 5, sc.max_depth, kernel=kernel, rng=pt.RNG_SAMPLE, chunk=2, nee=True)
    np.testing.assert_array_equal(bits(srgb), bits(sref["image"]))
    assert sst.rays == sref["rays"] and sst.paths == sref["paths"]
    np.testing.assert_array_equal(f.get_rng(), before)   # sample mode leaves the film's streams alone


def test_nee_off_is_the_blind_frame(pt, gpu, kernel):
    """The same scene without the flag: the frame, streams and counters of before."""
    sc = pn.nee_scene("N2")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    ref = pn.nee_reference("N2", nee=False)[0]
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"]


def test_nee_clamped_samples_bit_exact(pt, gpu, kernel):
    """The clamp scene: samples far above PT_MAX_RADIANCE, each clamped with one fminf."""
    sc = pn.clamp_scene()
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, 3, device=gpu)
    st0 = pn.orc.film_states(3, sc.width, range(sc.height))
    ref = pn.render(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), sc.spp,
                    sc.max_depth, st0, sky=sc.sky, nee=True)
    assert ref["events"]["clamped"] > 0
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel, nee=True)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"]
    sref = pn.render_sample(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), 5,
                            sc.max_depth, 3, 2, sky=sc.sky, nee=True)
    srgb, sst = pt.render(s, f, cam, 5, sc.max_depth, kernel=kernel, rng=pt.RNG_SAMPLE, chunk=2, nee=True)
    np.testing.assert_array_equal(bits(srgb), bits(sref["image"]))
    assert sst.rays == sref["rays"]


# ---------------------------------------------------------------- 2. partitioned film, accumulation, 8-bit output
def test_nee_partitioned_film_bit_exact(pt, gpu, kernel):
    sc = pn.nee_scene("N1")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu, stripe_height=3, n_parts=2, part=1)
    assert 0 < f.n_rows < sc.height
    ref = pn.nee_reference("N1", rows=tuple(int(r) for r in f.rows))[0]
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel, nee=True)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"]


def test_nee_two_accumulated_frames(pt, orc, gpu, kernel):
    """The raw per-pixel sums of two frames, through the film's accumulator."""
    sc = pn.nee_scene("N1")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    refs = pn.nee_reference("N1", spp=2, frames=2)
    want = orc.accumulate([r["sums"] for r in refs], [2, 2])
    for k in range(2):
        rgb, st = pt.render(s, f, cam, 2, sc.max_depth, kernel=kernel, accumulate=True, nee=True)
        np.testing.assert_array_equal(bits(rgb), bits(want[k]))
        assert st.rays == refs[k]["rays"]
    np.testing.assert_array_equal(f.get_rng(), refs[-1]["states"])
    assert f.accumulated == 4


def test_nee_rgba8_output(pt, orc, gpu, kernel):
    sc = pn.nee_scene("N2")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    ref = pn.nee_reference("N2")[0]["image"]
    q, _ = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel, out_format=pt.OUT_RGBA8, nee=True)
    np.testing.assert_array_equal(q, orc.quantize_png(ref))


def test_nee_second_compat_launch_at_long_depth(pt, gpu):
    """Compat mode, wide kernel, depth > 16: a film's second launch would run the first one's longest
    chains in critical-pixel waves, whose per-lane loop knows no shadow query -- NEE launches go
    without them (they only schedule).  Then a blind launch on the same film, which has them again."""
    sc = pn.nee_scene("N2")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    refs = pn.nee_reference("N2", spp=2, max_depth=20, frames=2)
    for ref in refs:
        rgb, st = pt.render(s, f, cam, 2, 20, kernel=pt.KERNEL_WIDE, nee=True)
        np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
        np.testing.assert_array_equal(f.get_rng(), ref["states"])
        assert st.rays == ref["rays"] and st.paths == ref["paths"]
    for _ in range(2):   # blind again: the second of these has critical-pixel waves
        before = f.get_rng()
        rgb, st = pt.render(s, f, cam, 2, 20, kernel=pt.KERNEL_WIDE)
        want = pn.render(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), 2, 20,
                         before, sky=sc.sky, nee=False)
        np.testing.assert_array_equal(bits(rgb), bits(want["image"]))
        assert st.rays == want["rays"]


# ---------------------------------------------------------------- 3. the shadow query's definition
def test_shadow_query_is_pt_trace_occluded(pt, gpu):
    """The shadow rays the restatement traced on N1 (a few hundred, evenly picked): occluded exactly when
    pt_trace_occluded(tmin = 0.001, tmax = 0.999) says so, on either tree."""
    sc = pn.nee_scene("N1")
    s = device_scene(pt, gpu, sc)
    shadow = pn.nee_reference("N1")[0]["shadow"]
    pick = shadow[::max(1, len(shadow) // 400)]
    rays = np.zeros(len(pick), pt.RAY_DTYPE)
    rays["o"] = [r[:3] for r, _ in pick]
    rays["d"] = [r[3:] for r, _ in pick]
    want = np.array([occ for _, occ in pick], np.uint8)
    assert 300 <= len(pick) and 0 < want.sum() < len(want)
    for k in (pt.KERNEL_DEFAULT, pt.KERNEL_SIMPLE):
        occ, _ = s.occluded(rays, tmin=0.001, tmax=0.999, kernel=k)
        np.testing.assert_array_equal(occ, want)


# ---------------------------------------------------------------- 4. no sampled light: nothing changes
@pytest.mark.parametrize("rng", ["compat", "sample"])
def test_nee_flag_without_lights_changes_nothing(pt, gpu, kernel, rng):
    w, h = 32, 18
    p = pt.Preset("rtiow", w, h)
    mode = pt.RNG_COMPAT if rng == "compat" else pt.RNG_SAMPLE
    s = pt.Scene(p.objects, p.materials, device=gpu)
    assert s.n_lights == 0
    frames = []
    for nee in (False, True):
        f = pt.Film(w, h, 9, device=gpu)
        rgb, st = pt.render(s, f, p.camera, 4, 50, kernel=kernel, rng=mode, chunk=2, nee=nee)
        frames.append((rgb, f.get_rng(), st))
    np.testing.assert_array_equal(bits(frames[0][0]), bits(frames[1][0]))
    np.testing.assert_array_equal(frames[0][1], frames[1][1])
    a, b = frames[0][2], frames[1][2]
    assert (a.rays, a.paths, a.node_visits, a.tri_tests, a.sphere_tests) == \
           (b.rays, b.paths, b.node_visits, b.tri_tests, b.sphere_tests)


# ---------------------------------------------------------------- 5. the light list follows a rebuild
def test_light_list_follows_update_objects(pt, gpu, kernel):
    sc = pn.nee_scene("N1")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    assert s.n_lights == 2
    em = int(np.flatnonzero(sc.materials["type"] == pt.PT_EMISSIVE)[0])
    i = int(np.flatnonzero(sc.objects["mat"] != em)[0])   # a Lambertian triangle of the box
    lit = sc.objects[i:i + 1].copy()
    lit["mat"] = em
    s.update_objects(lit, first=i)
    with pytest.raises(pt.PtError) as e:
        s.n_lights
    assert e.value.code == 6
    s.build_bvh()
    assert s.n_lights == 3
    objs = sc.objects.copy()
    objs[i] = lit[0]
    nodes = pn.orc.build_lbvh(objs, pn.orc.morton_keys(objs), tight=True)
    st0 = pn.orc.film_states(SEED, sc.width, range(sc.height))
    ref = pn.render(objs, sc.materials, nodes, sc.camera, sc.width, sc.height, range(sc.height), 2, sc.max_depth, st0,
                    sky=sc.sky, nee=True)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    rgb, st = pt.render(s, f, cam, 2, sc.max_depth, kernel=kernel, nee=True)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"]
    s.update_objects(sc.objects[i:i + 1], first=i)   # and back
    s.build_bvh()
    assert s.n_lights == 2
    f.reset()
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel, nee=True)
    np.testing.assert_array_equal(bits(rgb), bits(pn.nee_reference("N1")[0]["image"]))


# ---------------------------------------------------------------- 6. errors
def test_nee_errors(pt, gpu):
    sc = pn.nee_scene("N1")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    out = np.full((f.n_pixels, 3), -7.0, np.float32)
    before = f.get_rng()
    with pytest.raises(pt.PtError) as e:
        pt.render(s, f, cam, 1, 4, out=out, kernel=pt.KERNEL_WAVEFRONT, nee=True)
    assert e.value.code == 1 and "PT_RENDER_NEE" in str(e.value) and "WAVEFRONT" in str(e.value)
    assert (out == -7.0).all()
    np.testing.assert_array_equal(f.get_rng(), before)
    ip = pt.InstancedPreset("cornell_lit", 16, 16)
    si = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, ip.instances, ip.materials, device=gpu)
    assert si.n_lights == 0
    fi = pt.Film(16, 16, 1, device=gpu)
    outi = np.full((fi.n_pixels, 3), -7.0, np.float32)
    with pytest.raises(pt.PtError) as e:
        pt.render(si, fi, ip.camera, 1, 4, out=outi, kernel=pt.KERNEL_WIDE, nee=True)
    assert e.value.code == 1 and "instanced" in str(e.value)
    assert (outi == -7.0).all()
    pt.render(si, fi, ip.camera, 1, 4, out=outi, kernel=pt.KERNEL_WIDE)   # (without the flag it renders)
    assert (outi >= 0.0).all()
    unbuilt = pt.Scene(sc.objects, sc.materials, device=gpu, build=False)
    with pytest.raises(pt.PtError) as e:
        unbuilt.n_lights
    assert e.value.code == 6 and "pt_scene_light_count" in str(e.value)


# ---------------------------------------------------------------- 7. the same expectation, less noise
STAT_W = STAT_H = 16
STAT_DEPTH = 8
STAT_SEEDS = tuple(range(101, 109))


def _stat_frames(pt, gpu, spp, nee):
    """Linear images (the output squared), one per film seed: float64 (8, npix, 3)."""
    p = pt.Preset("cornell_lit", STAT_W, STAT_H)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    s.set_sky(*p.sky)
    out = []
    for seed in STAT_SEEDS:
        f = pt.Film(STAT_W, STAT_H, seed, device=gpu)
        rgb, _ = pt.render(s, f, p.camera, spp, STAT_DEPTH, rng=pt.RNG_SAMPLE, nee=nee)
        out.append(rgb.astype(np.float64) ** 2)
    return np.array(out)


def test_nee_has_the_blind_integrators_expectation(pt, gpu):
    """cornell_lit, 16 x 16, depth 8, sample mode, eight film seeds each for blind and NEE at 1024 spp
    (262,144 paths per frame; chosen on the GPU: the blind side's eight image means then spread by
    about 1 % and the standard error of the difference is 0.5 % of the mean, so a rule that lost or
    double-counted a few percent of the light would fail).  Per channel, the difference of the two
    mean image means lies within 4 standard errors of that difference, each side's standard error
    taken from the spread of its own eight seeds.  Measured: blind 0.18842 / 0.12275 / 0.03514, NEE
    0.18800 / 0.12236 / 0.03506, differences of -0.47, -0.66 and -0.50 standard errors.  (None of N1's
    reference samples clamps -- test_nee_host.py; the clamp's bias next to the lamp, DESIGN.md section
    10b, is far below this test's resolution at 16 x 16.)"""
    spp = 1024
    blind = _stat_frames(pt, gpu, spp, False).mean(axis=1)   # (8, 3) image means
    nee = _stat_frames(pt, gpu, spp, True).mean(axis=1)
    n = len(STAT_SEEDS)
    diff = nee.mean(0) - blind.mean(0)
    se = np.sqrt(blind.var(0, ddof=1) / n + nee.var(0, ddof=1) / n)
    print("blind means", blind.mean(0), "NEE means", nee.mean(0), "difference", diff, "standard error", se,
          "difference / se", diff / se)
    assert (np.abs(diff) <= 4 * se).all(), (diff, se)
    assert (se < 0.05 * blind.mean(0)).all()   # (teeth: the two sides are pinned to 5 % or better)


def test_nee_has_less_noise(pt, gpu):
    """The same scene at 16 spp, eight seeds: the mean per-pixel variance across seeds (of the linear
    values) is lower with NEE.  (The measured ratio, 1.51, is in DESIGN.md section 10b; no threshold here.)"""
    blind = _stat_frames(pt, gpu, 16, False)
    nee = _stat_frames(pt, gpu, 16, True)
    vb, vn = blind.var(0, ddof=1).mean(), nee.var(0, ddof=1).mean()
    print("mean per-pixel variance: blind", vb, "NEE", vn, "ratio", vb / vn)
    assert vn < vb


# ---------------------------------------------------------------- 8. the command-line app
def test_render_png_app_nee(pt, gpu, tmp_path):
    """pt_render_png --nee: the PNG is the library's RGBA8 frame of the same preset with the flag; without
    --nee the app's output is what it was."""
    import os
    import subprocess
    from helpers import read_png
    app = os.path.join(os.path.dirname(pt.LIB_PATH), "pt_render_png")
    w, h, spp = 32, 32, 4
    pngs = []
    for extra in (["--nee"], []):
        out = str(tmp_path / f"nee{len(extra)}.png")
        r = subprocess.run([app, "--scene", "cornell_lit", "--models", pt.MODELS_DIR, "--width", str(w), "--height",
                            str(h), "--spp", str(spp), "--out", out] + extra, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        pngs.append(read_png(out))
    p = pt.Preset("cornell_lit", w, h)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    s.set_sky(*p.sky)
    for png, nee in zip(pngs, (True, False)):
        f = pt.Film(w, h, seed=1, device=gpu)
        rgba, _ = pt.render(s, f, p.camera, spp, p.max_depth, out_format=pt.OUT_RGBA8, nee=nee)
        np.testing.assert_array_equal(png, rgba.reshape(h, w, 4)[::-1])
    assert (pngs[0] != pngs[1]).any()
