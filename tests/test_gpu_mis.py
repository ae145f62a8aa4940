"""Next-event estimation with multiple importance sampling (PT_RENDER_MIS) on the GPU.

The reference of a MIS frame is tests/pathloop_mis.py, pathloop_nee's loop with the weights of
include/pt.h as a parameter; tests/test_mis_host.py holds that restatement to pathloop_nee.py (the
weights off), to the rule's bounds and to the blind integrator's expectation.  The bar is the project's
usual one: bit-exact images, sums, RNG streams and counters, in PT_KERNEL_SIMPLE and PT_KERNEL_WIDE.

  N1, N2 = pathloop_nee's scenes (the cornell_lit preset 24 x 24; a dense soup 24 x 16).
  clamp  = pathloop_nee.clamp_scene(): E = 900, the lamp 0.05 above the floor, 8 x 8.
  rim    = the same geometry with E = (17, 12, 4): plain NEE clamps there, the weights do not.
Without the feature bit 8 is ignored and every MIS frame below is the blind one: the bit-exact tests
fail there.
"""
import numpy as np
import pytest

import pathloop_mis as pm
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


def counters(st):
    return (st.rays, st.paths, st.node_visits, st.tri_tests, st.sphere_tests)


# ---------------------------------------------------------------- 1. MIS frames, both kernels, both modes
@pytest.mark.parametrize("name", ["N1", "N2", "clamp", "rim"])
def test_mis_frames_bit_exact(pt, gpu, kernel, name):
    sc = pm.mis_scene(name)
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    assert s.n_lights > 0
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    ref = pm.mis_reference(name)[0]
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel, mis=True)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"] and st.paths == ref["paths"]
    # (what the parent commit renders under the bit, and what plain NEE renders)
    for nee in (False, True):
        other = pn.nee_reference(name, nee=nee) if name in ("N1", "N2") else pm.mis_reference(name, nee=nee, mis=False)
        assert (bits(rgb) != bits(other[0]["image"])).any()
    before = f.get_rng()
    sref = pm.mis_reference_sample(name)
    srgb, sst = pt.render(s, f, cam, 5, sc.max_depth, kernel=kernel, rng=pt.RNG_SAMPLE, chunk=2, mis=True)
    np.testing.assert_array_equal(bits(srgb), bits(sref["image"]))
    assert sst.rays == sref["rays"] and sst.paths == sref["paths"]
    np.testing.assert_array_equal(f.get_rng(), before)   # sample mode leaves the film's streams alone


def test_mis_partitioned_film_bit_exact(pt, gpu, kernel):
    sc = pn.nee_scene("N1")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu, stripe_height=3, n_parts=2, part=1)
    assert 0 < f.n_rows < sc.height
    ref = pm.mis_reference("N1", rows=tuple(int(r) for r in f.rows))[0]
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel, mis=True)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"]


def test_mis_two_accumulated_frames(pt, orc, gpu, kernel):
    sc = pn.nee_scene("N1")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    refs = pm.mis_reference("N1", spp=2, frames=2)
    want = orc.accumulate([r["sums"] for r in refs], [2, 2])
    for k in range(2):
        rgb, st = pt.render(s, f, cam, 2, sc.max_depth, kernel=kernel, accumulate=True, mis=True)
        np.testing.assert_array_equal(bits(rgb), bits(want[k]))
        assert st.rays == refs[k]["rays"]
    np.testing.assert_array_equal(f.get_rng(), refs[-1]["states"])
    assert f.accumulated == 4


def test_mis_rgba8_output(pt, orc, gpu, kernel):
    sc = pn.nee_scene("N2")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    ref = pm.mis_reference("N2")[0]["image"]
    q, _ = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel, out_format=pt.OUT_RGBA8, mis=True)
    np.testing.assert_array_equal(q, orc.quantize_png(ref))


def test_mis_second_compat_launch_at_long_depth(pt, gpu):
    """Compat mode, wide kernel, depth > 16: MIS launches, like NEE ones, go without critical-pixel waves."""
    sc = pn.nee_scene("N2")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    refs = pm.mis_reference("N2", spp=2, max_depth=20, frames=2)
    for ref in refs:
        rgb, st = pt.render(s, f, cam, 2, 20, kernel=pt.KERNEL_WIDE, mis=True)
        np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
        np.testing.assert_array_equal(f.get_rng(), ref["states"])
        assert st.rays == ref["rays"] and st.paths == ref["paths"]


# ---------------------------------------------------------------- 2, 3. the bit's value; the NEE frame's counters
@pytest.mark.parametrize("rng", ["compat", "sample"])
def test_mis_bit_implies_nee_and_keeps_its_counters(pt, gpu, kernel, rng):
    """mis=True alone and mis=True, nee=True: the same frame.  Against the nee=True frame of the same
    arguments: the same rays, paths, node, triangle and sphere counters and advanced streams; another image."""
    sc = pn.nee_scene("N2")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    mode = pt.RNG_COMPAT if rng == "compat" else pt.RNG_SAMPLE
    res = []
    for kw in ({"mis": True}, {"mis": True, "nee": True}, {"nee": True}):
        f = pt.Film(sc.width, sc.height, SEED, device=gpu)
        rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel, rng=mode, chunk=2, **kw)
        res.append((rgb, f.get_rng(), counters(st)))
    np.testing.assert_array_equal(bits(res[0][0]), bits(res[1][0]))
    for k in (1, 2):
        np.testing.assert_array_equal(res[0][1], res[k][1])
        assert res[0][2] == res[k][2]
    assert (bits(res[0][0]) != bits(res[2][0])).any()


# ---------------------------------------------------------------- 4. the light slots follow a rebuild
def test_mis_light_slots_follow_update_objects(pt, gpu, kernel):
    """A box triangle turns emissive -- object 0, ahead of the lamp's triangles (objects 10 and 11), whose
    slots the rebuild's scan moves from 0, 1 to 1, 2: the MIS frame is the restatement of the new
    objects, and of the old ones after turning it back."""
    sc = pn.nee_scene("N1")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    em = int(np.flatnonzero(sc.materials["type"] == pt.PT_EMISSIVE)[0])
    i = int(np.flatnonzero(sc.objects["mat"] != em)[0])   # a Lambertian triangle of the box
    lit = sc.objects[i:i + 1].copy()
    lit["mat"] = em
    s.update_objects(lit, first=i)
    s.build_bvh()
    assert s.n_lights == 3
    objs = sc.objects.copy()
    objs[i] = lit[0]
    assert pm.light_slots(objs, sc.materials)[sc.objects["mat"] == em].tolist() == [1, 2]
    nodes = pn.orc.build_lbvh(objs, pn.orc.morton_keys(objs), tight=True)
    st0 = pn.orc.film_states(SEED, sc.width, range(sc.height))
    ref = pm.render(objs, sc.materials, nodes, sc.camera, sc.width, sc.height, range(sc.height), 2, sc.max_depth, st0,
                    sky=sc.sky, mis=True)
    assert any(k == "emitter" for k, *_ in ref["weights"])
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    rgb, st = pt.render(s, f, cam, 2, sc.max_depth, kernel=kernel, mis=True)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"]
    s.update_objects(sc.objects[i:i + 1], first=i)   # and back
    s.build_bvh()
    assert s.n_lights == 2
    f.reset()
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=kernel, mis=True)
    np.testing.assert_array_equal(bits(rgb), bits(pm.mis_reference("N1")[0]["image"]))


# ---------------------------------------------------------------- 5. no sampled light: nothing changes
@pytest.mark.parametrize("rng", ["compat", "sample"])
def test_mis_flag_without_lights_changes_nothing(pt, gpu, kernel, rng):
    w, h = 32, 18
    p = pt.Preset("rtiow", w, h)
    mode = pt.RNG_COMPAT if rng == "compat" else pt.RNG_SAMPLE
    s = pt.Scene(p.objects, p.materials, device=gpu)
    assert s.n_lights == 0
    frames = []
    for mis in (False, True):
        f = pt.Film(w, h, 9, device=gpu)
        rgb, st = pt.render(s, f, p.camera, 4, 50, kernel=kernel, rng=mode, chunk=2, mis=mis)
        frames.append((rgb, f.get_rng(), st))
    np.testing.assert_array_equal(bits(frames[0][0]), bits(frames[1][0]))
    np.testing.assert_array_equal(frames[0][1], frames[1][1])
    assert counters(frames[0][2]) == counters(frames[1][2])


# ---------------------------------------------------------------- 6. errors
def test_mis_errors(pt, gpu):
    sc = pn.nee_scene("N1")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    out = np.full((f.n_pixels, 3), -7.0, np.float32)
    before = f.get_rng()
    with pytest.raises(pt.PtError) as e:
        pt.render(s, f, cam, 1, 4, out=out, kernel=pt.KERNEL_WAVEFRONT, mis=True)
    assert e.value.code == 1 and "PT_RENDER_MIS" in str(e.value) and "WAVEFRONT" in str(e.value)
    assert (out == -7.0).all()
    np.testing.assert_array_equal(f.get_rng(), before)
    ip = pt.InstancedPreset("cornell_lit", 16, 16)
    si = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, ip.instances, ip.materials, device=gpu)
    fi = pt.Film(16, 16, 1, device=gpu)
    outi = np.full((fi.n_pixels, 3), -7.0, np.float32)
    beforei = fi.get_rng()
    with pytest.raises(pt.PtError) as e:
        pt.render(si, fi, ip.camera, 1, 4, out=outi, kernel=pt.KERNEL_WIDE, mis=True)
    assert e.value.code == 1 and "PT_RENDER_MIS" in str(e.value) and "instanced" in str(e.value)
    assert (outi == -7.0).all()
    np.testing.assert_array_equal(fi.get_rng(), beforei)


# ---------------------------------------------------------------- 7. statistics, the rim scene
RIM_SEEDS = tuple(range(201, 209))


def _rim_means(pt, gpu, spp, **kw):
    """Image means of the linear frame (the output squared), one per film seed: float64 (8, 3)."""
    sc = pm.rim_scene()
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    out = []
    for seed in RIM_SEEDS:
        f = pt.Film(sc.width, sc.height, seed, device=gpu)
        rgb, _ = pt.render(s, f, cam, spp, sc.max_depth, rng=pt.RNG_SAMPLE, **kw)
        out.append((rgb.astype(np.float64) ** 2).mean(0))
    return np.array(out)


def test_mis_has_the_blind_expectation_where_nee_is_biased(pt, gpu):
    """The rim scene, 8 x 8, depth 3, sample mode, eight film seeds x 4096 spp a side (262,144 paths per
    frame).  Per channel MIS - blind lies within 4 standard errors of the difference, each side's
    standard error from the spread of its own eight seeds, and each side is pinned to 5 % or better;
    NEE - blind lies beyond 4 on red (the clamp's bias: the teeth).  The host test at 512 spp measures
    +0.12 and -8.4 standard errors."""
    spp, n = 4096, len(RIM_SEEDS)
    blind, nee, mis = _rim_means(pt, gpu, spp), _rim_means(pt, gpu, spp, nee=True), _rim_means(pt, gpu, spp, mis=True)

    def z(a, b):
        se = np.sqrt(a.var(0, ddof=1) / n + b.var(0, ddof=1) / n)
        return (a.mean(0) - b.mean(0)) / se, se
    zm, sem = z(mis, blind)
    zn, _ = z(nee, blind)
    print("blind means", blind.mean(0), "NEE means", nee.mean(0), "MIS means", mis.mean(0))
    print("MIS - blind", zm, "NEE - blind", zn, "standard errors; standard error of MIS - blind", sem)
    assert (np.abs(zm) <= 4).all(), zm
    assert (sem < 0.05 * blind.mean(0)).all()
    assert abs(zn[0]) > 4, zn


# ---------------------------------------------------------------- 8, 9. statistics, cornell_lit
STAT_W = STAT_H = 16
STAT_DEPTH = 8
STAT_SEEDS = tuple(range(101, 109))


def _stat_frames(pt, gpu, spp, **kw):
    """Linear images (the output squared), one per film seed: float64 (8, npix, 3)."""
    p = pt.Preset("cornell_lit", STAT_W, STAT_H)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    s.set_sky(*p.sky)
    out = []
    for seed in STAT_SEEDS:
        f = pt.Film(STAT_W, STAT_H, seed, device=gpu)
        rgb, _ = pt.render(s, f, p.camera, spp, STAT_DEPTH, rng=pt.RNG_SAMPLE, **kw)
        out.append(rgb.astype(np.float64) ** 2)
    return np.array(out)


def test_mis_has_the_blind_integrators_expectation(pt, gpu):
    """cornell_lit, 16 x 16, depth 8, sample mode, eight film seeds each for blind and MIS at 1024 spp, as in
    test_gpu_nee.py: per channel the difference of the two mean image means lies within 4 standard errors
    of that difference, each side pinned to 5 % or better."""
    spp = 1024
    blind = _stat_frames(pt, gpu, spp).mean(axis=1)
    mis = _stat_frames(pt, gpu, spp, mis=True).mean(axis=1)
    n = len(STAT_SEEDS)
    diff = mis.mean(0) - blind.mean(0)
    se = np.sqrt(blind.var(0, ddof=1) / n + mis.var(0, ddof=1) / n)
    print("blind means", blind.mean(0), "MIS means", mis.mean(0), "difference", diff, "standard error", se,
          "difference / se", diff / se)
    assert (np.abs(diff) <= 4 * se).all(), (diff, se)
    assert (se < 0.05 * blind.mean(0)).all()


def test_mis_has_less_noise(pt, gpu):
    """The same scene at 16 spp, eight seeds: the mean per-pixel variance across seeds (of the linear
    values) is lower with MIS than blind.  No threshold; the ratio to NEE's is printed."""
    blind = _stat_frames(pt, gpu, 16)
    nee = _stat_frames(pt, gpu, 16, nee=True)
    mis = _stat_frames(pt, gpu, 16, mis=True)
    vb, vn, vm = (x.var(0, ddof=1).mean() for x in (blind, nee, mis))
    print("mean per-pixel variance: blind", vb, "NEE", vn, "MIS", vm, "blind / MIS", vb / vm, "NEE / MIS", vn / vm)
    assert vm < vb


# ---------------------------------------------------------------- 10. the command-line app
def test_render_png_app_mis(pt, gpu, tmp_path):
    """pt_render_png --mis: the PNG is the library's RGBA8 frame of the same preset with the bit; without
    --mis the app's output is what it was."""
    import os
    import subprocess
    from helpers import read_png
    app = os.path.join(os.path.dirname(pt.LIB_PATH), "pt_render_png")
    w, h, spp = 32, 32, 4
    pngs = []
    for extra in (["--mis"], []):
        out = str(tmp_path / f"mis{len(extra)}.png")
        r = subprocess.run([app, "--scene", "cornell_lit", "--models", pt.MODELS_DIR, "--width", str(w), "--height",
                            str(h), "--spp", str(spp), "--out", out] + extra, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        pngs.append(read_png(out))
    p = pt.Preset("cornell_lit", w, h)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    s.set_sky(*p.sky)
    for png, mis in zip(pngs, (True, False)):
        f = pt.Film(w, h, seed=1, device=gpu)
        rgba, _ = pt.render(s, f, p.camera, spp, p.max_depth, out_format=pt.OUT_RGBA8, mis=mis)
        np.testing.assert_array_equal(png, rgba.reshape(h, w, 4)[::-1])
    assert (pngs[0] != pngs[1]).any()
