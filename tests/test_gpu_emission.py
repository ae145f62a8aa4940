"""Emissive materials (PT_EMISSIVE) and the per-scene sky (pt_scene_set_sky) on the GPU.

The reference of a lit frame is tests/pathloop.py: the oracle's render loop restated out of oracle
parts with the two new rules added; tests/test_emission_host.py proves that restatement against the
oracle itself and that the two lit scenes' paths end in every way.  The bar is the project's usual
one: bit-exact images, RNG streams and counters, in every render kernel.

  L1 = the cornell_lit preset, 24 x 24, 4 spp, depth 8, black sky (the lamp is the only light).
  L2 = a soup of triangles and spheres -- Lambertian, metal, dielectric and an emitter E = (4, 3, 0.5) --
       under the sky H = (0.2, 0.1, 0.3), Z = (0.9, 0.8, 0.1), 24 x 16, 3 spp, depth 12.
"""
import numpy as np
import pytest

import pathloop
from pathloop import SEED, lit_reference, lit_reference_sample, lit_scene

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(params=["wide", "wavefront", "simple"])
def kernel(request, monkeypatch):
    monkeypatch.setenv("PT_RENDER_KERNEL", request.param)
    return request.param


def camera_of(pt, sc):
    return pt.Camera.from_buffer_copy(sc.camera.tobytes())


def device_scene(pt, gpu, sc, sky=None):
    s = pt.Scene(sc.objects, sc.materials, device=gpu)
    s.set_sky(*(sc.sky if sky is None else sky))
    return s


# ---------------------------------------------------------------- 5. lit frames, every kernel
@pytest.mark.parametrize("name", ["L1", "L2"])
def test_lit_frames_bit_exact(pt, gpu, kernel, name):
    """Fails without the feature: type 8 absorbs there (every path that ends on an emitter is black)
    and pt_scene_set_sky does not exist."""
    sc = lit_scene(name)
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    ref = lit_reference(name)[0]
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"] and st.paths == ref["paths"]
    assert rgb.max() > 1.0   # (light was emitted: a frame of absorbers would not get here)
    before = f.get_rng()
    sref = lit_reference_sample(name)
    srgb, sst = pt.render(s, f, cam, 5, sc.max_depth, rng=pt.RNG_SAMPLE, chunk=2)
    np.testing.assert_array_equal(bits(srgb), bits(sref["image"]))
    assert sst.rays == sref["rays"] and sst.paths == sref["paths"]
    np.testing.assert_array_equal(f.get_rng(), before)   # sample mode leaves the film's streams alone


# ---------------------------------------------------------------- 6. critical-pixel waves
def test_lit_critical_pixel_waves_bit_exact(pt, gpu):
    """Compat mode, wide kernel, depth > 16: the second launch on a film runs the first one's longest
    chains in critical-pixel waves (the per-lane traversal loop, then the same SHADE step)."""
    sc = lit_scene("L2")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    refs = lit_reference("L2", spp=2, max_depth=20, frames=2)
    for ref in refs:
        rgb, st = pt.render(s, f, cam, 2, 20, kernel=pt.KERNEL_WIDE)
        np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
        np.testing.assert_array_equal(f.get_rng(), ref["states"])
        assert st.rays == ref["rays"] and st.paths == ref["paths"]


# ---------------------------------------------------------------- 7. a partitioned film
def test_lit_partitioned_film_bit_exact(pt, gpu):
    sc = lit_scene("L1")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu, stripe_height=3, n_parts=2, part=1)
    assert 0 < f.n_rows < sc.height
    ref = lit_reference("L1", rows=tuple(int(r) for r in f.rows))[0]
    rgb, st = pt.render(s, f, cam, sc.spp, sc.max_depth)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref["states"])
    assert st.rays == ref["rays"]


# ---------------------------------------------------------------- 8. nothing existing moved
@pytest.mark.parametrize("rng", ["compat", "sample"])
def test_default_sky_set_explicitly_is_the_sky_never_set(pt, gpu, rng):
    w, h = 32, 18
    p = pt.Preset("rtiow", w, h)
    mode = pt.RNG_COMPAT if rng == "compat" else pt.RNG_SAMPLE
    frames = []
    for set_it in (False, True):
        s = pt.Scene(p.objects, p.materials, device=gpu)
        if set_it:
            s.set_sky((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))
        f = pt.Film(w, h, 9, device=gpu)
        rgb, st = pt.render(s, f, p.camera, 4, 50, rng=mode, chunk=2)
        frames.append((rgb, f.get_rng(), st.rays))
    np.testing.assert_array_equal(bits(frames[0][0]), bits(frames[1][0]))
    np.testing.assert_array_equal(frames[0][1], frames[1][1])
    assert frames[0][2] == frames[1][2]
    assert bits(p.sky[0]).tolist() == bits(np.ones(3, np.float32)).tolist()


def test_zero_radiance_emitter_equals_the_oracle(pt, orc, gpu, kernel):
    """The oracle absorbs type 8, so an emitter of radiance 0 under the default sky has a whole-frame
    oracle: image, streams (no draw at an emitter) and rays.  (Passes without the feature too.)"""
    sc = lit_scene("L2")
    w, h, spp, depth = 64, 36, 4, 50
    mats = sc.materials.copy()
    mats["albedo"][mats["type"] == pt.PT_EMISSIVE] = 0.0
    cam = pt.camera_make(pathloop.L2_CAMERA_FROM, pathloop.L2_CAMERA_AT, pathloop.L2_CAMERA_VFOV, w / h)
    s = pt.Scene(sc.objects, mats, device=gpu)
    f = pt.Film(w, h, 4, device=gpu)
    rgb, st = pt.render(s, f, cam, spp, depth)
    states = orc.film_states(4, w, f.rows)
    ref, rst = orc.render(sc.objects, mats, sc.nodes, pt.camera_to_array(cam), w, h, f.rows, spp, depth, states,
                          nthreads=8)
    np.testing.assert_array_equal(bits(rgb), bits(ref))
    np.testing.assert_array_equal(f.get_rng(), states)
    assert st.rays == rst.rays and st.paths == rst.paths


# ---------------------------------------------------------------- 9. progressive and 8-bit output
def test_lit_progressive_frames(pt, orc, gpu):
    sc = lit_scene("L1")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    refs = lit_reference("L1", spp=2, frames=3)
    want = orc.accumulate([r["sums"] for r in refs], [2, 2, 2])
    for k in range(3):
        rgb, _ = pt.render(s, f, cam, 2, sc.max_depth, accumulate=True)
        np.testing.assert_array_equal(bits(rgb), bits(want[k]))
    np.testing.assert_array_equal(f.get_rng(), refs[-1]["states"])
    assert f.accumulated == 6


def test_lit_rgba8_output_clamps(pt, orc, gpu):
    sc = lit_scene("L2")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    ref = lit_reference("L2")[0]["image"]
    q, _ = pt.render(s, f, cam, sc.spp, sc.max_depth, out_format=pt.OUT_RGBA8)
    np.testing.assert_array_equal(q, orc.quantize_png(ref))
    assert (ref > 1.0).any() and q[:, :3].max() == 255   # radiance above 1 clamps to 0.999 * 256


# ---------------------------------------------------------------- 10. instanced scenes
def _instanced_and_flat(pt, gpu, name, w, h, spp):
    ip, fp = pt.InstancedPreset(name, w, h), pt.Preset(name, w, h)
    si = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, ip.instances, ip.materials, device=gpu)
    sf = pt.Scene(fp.objects, fp.materials, device=gpu)
    si.set_sky(*ip.sky)
    sf.set_sky(*fp.sky)
    ri, sti = pt.render(si, pt.Film(w, h, 7, device=gpu), ip.camera, spp, ip.max_depth, kernel=pt.KERNEL_WIDE,
                        rng=pt.RNG_SAMPLE)
    rf, stf = pt.render(sf, pt.Film(w, h, 7, device=gpu), fp.camera, spp, fp.max_depth, kernel=pt.KERNEL_WIDE,
                        rng=pt.RNG_SAMPLE)
    return ri, sti, rf, stf


def test_instanced_cornell_lit_equals_flat(pt, gpu):
    ri, sti, rf, stf = _instanced_and_flat(pt, gpu, "cornell_lit", 48, 48, 4)
    np.testing.assert_array_equal(ri, rf)
    assert sti.rays == stf.rays and rf.max() > 1.0


def test_instanced_bunny_cornell_lit_close_to_flat(pt, gpu):
    """test_gpu_instancing.py::test_instanced_render_close_to_flattened's three inequalities, with its
    constants."""
    ri, sti, rf, stf = _instanced_and_flat(pt, gpu, "bunny_cornell_lit", 64, 64, 4)
    assert np.isfinite(ri).all()
    mi, mf = ri.mean(0), rf.mean(0)
    print("means", mi, mf, "mean abs diff", np.abs(ri - rf).mean(0), "rays", sti.rays, stf.rays)
    assert (np.abs(mi - mf) <= 0.01 * mf + 1e-4).all(), (mi, mf)
    assert (np.abs(ri - rf).mean(0) <= 0.02).all(), np.abs(ri - rf).mean(0)
    assert abs(sti.rays - stf.rays) <= 0.01 * stf.rays


# ---------------------------------------------------------------- 11. pt_scene_set_sky's rules
def test_set_sky_rules(pt, gpu):
    sc = lit_scene("L2")
    s, cam = device_scene(pt, gpu, sc), camera_of(pt, sc)
    f = pt.Film(sc.width, sc.height, SEED, device=gpu)
    ref = lit_reference("L2")[0]
    rgb, _ = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=pt.KERNEL_WIDE)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    source = s.wide_info()["source"]
    assert source != 0
    ok = (0.5, 0.5, 0.5)
    for h, z in ((None, ok), (ok, None), ((float("nan"), 0.5, 0.5), ok), (ok, (0.5, float("inf"), 0.5)),
                 ((0.5, -0.25, 0.5), ok), (ok, (0.5, 0.5, 1025.0)), ((2000.0, 0.0, 0.0), (2000.0, 0.0, 0.0))):
        with pytest.raises(pt.PtError) as e:
            s.set_sky(h, z)
        assert e.value.code == 1 and "pt_scene_set_sky" in str(e.value)
    f.reset()
    again, _ = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=pt.KERNEL_WIDE)   # the sky is what it was
    np.testing.assert_array_equal(bits(again), bits(rgb))
    # a valid change: the next render has it, without a rebuild
    new_sky = ((0.5, 0.25, 1.0), (0.0, 2.0, 0.125))
    s.set_sky(*new_sky)
    assert s.wide_info()["source"] == source
    f.reset()
    changed, st = pt.render(s, f, cam, sc.spp, sc.max_depth, kernel=pt.KERNEL_WIDE)
    ref2 = lit_reference("L2", sky=new_sky)[0]
    np.testing.assert_array_equal(bits(changed), bits(ref2["image"]))
    np.testing.assert_array_equal(f.get_rng(), ref2["states"])
    assert st.rays == ref2["rays"] and (bits(changed) != bits(rgb)).any()
    assert s.wide_info()["source"] == source


# ---------------------------------------------------------------- 12. the command-line app
def test_render_png_app_lit(pt, gpu, tmp_path):
    """pt_render_png --scene cornell_lit renders under the preset's own (black) sky: its PNG is the
    library's RGBA8 frame of the same preset, sky, seed and RNG mode; --sky default overrides."""
    import os
    import subprocess
    from helpers import read_png
    app = os.path.join(os.path.dirname(pt.LIB_PATH), "pt_render_png")
    w, h, spp = 32, 32, 4
    pngs = []
    for extra in ([], ["--sky", "default"]):
        out = str(tmp_path / f"lit{len(extra)}.png")
        r = subprocess.run([app, "--scene", "cornell_lit", "--models", pt.MODELS_DIR, "--width", str(w), "--height",
                            str(h), "--spp", str(spp), "--out", out] + extra, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        pngs.append(read_png(out))
    p = pt.Preset("cornell_lit", w, h)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    s.set_sky(*p.sky)
    f = pt.Film(w, h, seed=1, device=gpu)   # the app's default seed, RNG mode (compat) and depth (the preset's)
    rgba, _ = pt.render(s, f, p.camera, spp, p.max_depth, out_format=pt.OUT_RGBA8)
    np.testing.assert_array_equal(pngs[0], rgba.reshape(h, w, 4)[::-1])   # (the PNG's row 0 is the top row)
    assert (pngs[1] != pngs[0]).any()
    s.set_sky((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))
    f.reset()
    rgba, _ = pt.render(s, f, p.camera, spp, p.max_depth, out_format=pt.OUT_RGBA8)
    np.testing.assert_array_equal(pngs[1], rgba.reshape(h, w, 4)[::-1])
