"""Emissive materials and the per-scene sky, host side (no GPU): the Python restatement of the render
loop that serves as the exact reference of lit frames (tests/pathloop.py) against the oracle it is
built from, the "_lit" presets, the argument checks that run before any device call, and the
conditions the lit GPU tests' inputs have to meet (tests/test_gpu_emission.py)."""
import numpy as np
import pytest

import pathloop


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- 1. the restatement itself
@pytest.mark.parametrize("name,w,h,spp,depth", [
    ("rtiow", 16, 9, 2, 50),     # spheres: metal and dielectric draws
    ("cornell", 12, 12, 2, 8),   # triangles; paths that run out of bounces
])
def test_pathloop_equals_oracle_render(pt, orc, name, w, h, spp, depth):
    """No emissive material, the default sky: the restated loop is orc.render, bit for bit -- image,
    final RNG states, rays and paths.  Without this the lit GPU tests prove nothing."""
    p = pt.Preset(name, w, h)
    nodes = orc.build_lbvh(p.objects, orc.morton_keys(p.objects), tight=True)
    cam = pt.camera_to_array(p.camera)
    states = orc.film_states(3, w, range(h))
    mine = pathloop.render(p.objects, p.materials, nodes, cam, w, h, range(h), spp, depth, states)
    ref, rst = orc.render(p.objects, p.materials, nodes, cam, w, h, range(h), spp, depth, states)   # advances states
    np.testing.assert_array_equal(bits(mine["image"]), bits(ref))
    np.testing.assert_array_equal(mine["states"], states)
    assert mine["rays"] == rst.rays and mine["paths"] == rst.paths == w * h * spp
    assert len(mine["kinds"]) == w * h * spp


def test_pathloop_equals_oracle_render_on_a_partition(pt, orc):
    """`rows` like orc.render: the rows of one part of a striped film."""
    w, h = 16, 9
    p = pt.Preset("rtiow", w, h)
    nodes = orc.build_lbvh(p.objects, orc.morton_keys(p.objects), tight=True)
    cam = pt.camera_to_array(p.camera)
    rows = [2, 3, 6, 7]
    states = orc.film_states(3, w, rows)
    mine = pathloop.render(p.objects, p.materials, nodes, cam, w, h, rows, 2, 50, states)
    ref, rst = orc.render(p.objects, p.materials, nodes, cam, w, h, rows, 2, 50, states)
    np.testing.assert_array_equal(bits(mine["image"]), bits(ref))
    np.testing.assert_array_equal(mine["states"], states)
    assert mine["rays"] == rst.rays


def test_pathloop_equals_oracle_render_sample(pt, orc):
    """Sample mode, 5 spp in blocks of 2 (a short last block)."""
    w, h = 16, 9
    p = pt.Preset("rtiow", w, h)
    nodes = orc.build_lbvh(p.objects, orc.morton_keys(p.objects), tight=True)
    cam = pt.camera_to_array(p.camera)
    mine = pathloop.render_sample(p.objects, p.materials, nodes, cam, w, h, range(h), 5, 50, 11, 2)
    ref, rst = orc.render_sample(p.objects, p.materials, nodes, cam, w, h, range(h), 5, 50, 11, chunk=2)
    np.testing.assert_array_equal(bits(mine["image"]), bits(ref))
    assert mine["rays"] == rst.rays and mine["paths"] == rst.paths


def test_pathloop_zero_radiance_emitter_is_the_oracles_absorber(pt, orc):
    """The oracle absorbs type 8; an emitter of radiance 0 under the default sky is that, exactly:
    same image, and -- no draw at an emitter -- the same streams."""
    sc = pathloop.lit_scene("L2")
    mats = sc.materials.copy()
    mats["albedo"][mats["type"] == pt.PT_EMISSIVE] = 0.0
    states = orc.film_states(5, sc.width, range(sc.height))
    mine = pathloop.render(sc.objects, mats, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), 2, 12, states)
    ref, rst = orc.render(sc.objects, mats, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), 2, 12, states)
    np.testing.assert_array_equal(bits(mine["image"]), bits(ref))
    np.testing.assert_array_equal(mine["states"], states)
    assert mine["rays"] == rst.rays
    assert any(k == pathloop.EMITTER for k, _ in mine["kinds"])


# ---------------------------------------------------------------- 2. presets
@pytest.mark.parametrize("name", ["cornell", "bunny_cornell"])
def test_lit_presets_are_the_unlit_ones_with_an_emissive_lamp(pt, name):
    lit, unlit = pt.Preset(name + "_lit"), pt.Preset(name)
    assert lit.name == name + "_lit"
    assert (lit.width, lit.height, lit.spp, lit.max_depth) == (unlit.width, unlit.height, unlit.spp, unlit.max_depth)
    assert bytes(lit.camera) == bytes(unlit.camera)
    np.testing.assert_array_equal(lit.objects["type"], unlit.objects["type"])
    np.testing.assert_array_equal(bits(lit.objects["v"]), bits(unlit.objects["v"]))
    # the lamp: exactly the triangles of light.obj, in place, now of the appended emissive material
    lamp = pt.load_obj(pt.MODELS_DIR + "/cornellbox/light.obj")
    moved = np.flatnonzero(lit.objects["mat"] != unlit.objects["mat"])
    assert len(moved) == len(lamp) > 0
    np.testing.assert_array_equal(bits(lit.objects["v"][moved]), bits(lamp["v"]))
    assert len(lit.materials) == len(unlit.materials) + 1
    np.testing.assert_array_equal(lit.materials[:-1], unlit.materials)
    assert (lit.objects["mat"][moved] == len(lit.materials) - 1).all()
    m = lit.materials[-1]
    assert m["type"] == pt.PT_EMISSIVE == 8
    np.testing.assert_array_equal(m["albedo"], np.array([17, 12, 4], np.float32))
    assert (lit.materials["type"] == pt.PT_EMISSIVE).sum() == 1


def test_preset_sky(pt):
    default = (np.array([1, 1, 1], np.float32), np.array([0.5, 0.7, 1.0], np.float32))
    for name in ("triangle_world", "random_world", "test_world", "rtiow", "cornell", "bunny_cornell"):
        h, z = pt.Preset(name, 8, 8).sky
        np.testing.assert_array_equal(h, default[0])
        np.testing.assert_array_equal(z, default[1])
    for name in ("bunny_field", "bunny_field_x4"):   # (not built here: a million triangles)
        h, z = pt.preset_sky(name)
        np.testing.assert_array_equal(h, default[0])
        np.testing.assert_array_equal(z, default[1])
    for name in ("cornell_lit", "bunny_cornell_lit"):
        for p in (pt.Preset(name, 8, 8), pt.InstancedPreset(name, 8, 8)):
            assert not p.sky[0].any() and not p.sky[1].any()
    np.testing.assert_array_equal(pt.InstancedPreset("cornell", 8, 8).sky[1], default[1])
    for bad in ("nonesuch", "cornell_lit_lit", ""):
        with pytest.raises(pt.PtError) as e:
            pt.preset_sky(bad)
        assert e.value.code == 1 and "pt_preset_sky" in str(e.value)
    with pytest.raises(pt.PtError):
        pt.Preset("nonesuch_lit")
    assert pt.PT_MAX_RADIANCE == 1024.0


@pytest.mark.parametrize("name", ["cornell_lit", "bunny_cornell_lit"])
def test_instanced_lit_presets_flatten_to_the_flat_presets(pt, name):
    """As test_host.py::test_instanced_presets_flatten_to_the_flat_presets, for the lit names."""
    ip, fp = pt.InstancedPreset(name), pt.Preset(name)
    parts = []
    for inst in ip.instances:
        m = inst["m"].reshape(3, 4)
        np.testing.assert_array_equal(m[:, :3], np.eye(3, dtype=np.float32))
        f, c = ip.mesh_first[inst["mesh"]], ip.mesh_count[inst["mesh"]]
        o = ip.objects[f:f + c].copy()
        o["v"] = (o["v"].reshape(-1, 3, 3) + m[:, 3]).reshape(-1, 9)
        parts.append(o)
    flat = np.concatenate(parts)
    assert ip.flattened_count() == len(fp.objects) == len(flat)
    np.testing.assert_array_equal(flat["v"], fp.objects["v"])
    np.testing.assert_array_equal(flat["mat"], fp.objects["mat"])
    np.testing.assert_array_equal(ip.materials, fp.materials)
    assert bytes(ip.camera) == bytes(fp.camera)
    assert ip.name == fp.name == name
    np.testing.assert_array_equal(ip.instances[0]["m"].reshape(3, 4)[:, 3], 0)   # the box: identity


# ---------------------------------------------------------------- 3. checks before any device call
def _one_triangle(pt, mat_type, albedo):
    objs = np.zeros(1, pt.OBJECT_DTYPE)
    objs["type"] = pt.PT_TRIANGLE
    objs["v"][0] = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    mats = np.zeros(2, pt.MATERIAL_DTYPE)
    mats["type"] = [pt.PT_LAMBERTIAN, mat_type]
    mats["albedo"][0] = 0.5
    mats["albedo"][1] = albedo
    return objs, mats


def _create_codes(pt, objs, mats):
    """Status of pt_scene_create and pt_scene_create_instanced (one mesh, one identity instance)."""
    codes = []
    inst = np.zeros(1, pt.INSTANCE_DTYPE)
    inst["m"][0] = np.eye(3, 4, dtype=np.float32).ravel()
    for make in (lambda: pt.Scene(objs, mats, build=False),
                 lambda: pt.Scene.instanced(objs, [0], [len(objs)], inst, mats, build=False)):
        try:
            make().close()
            codes.append(0)
        except pt.PtError as e:
            codes.append(e.code)
    return codes


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -0.5, 1025.0])
@pytest.mark.parametrize("channel", [0, 2])
def test_emissive_radiance_is_checked_before_the_device(pt, bad, channel):
    albedo = [1.0, 2.0, 3.0]
    albedo[channel] = bad
    objs, mats = _one_triangle(pt, pt.PT_EMISSIVE, albedo)
    for make in (lambda: pt.Scene(objs, mats, build=False),
                 lambda: pt.Scene.instanced(objs, [0], [1], np.zeros(1, pt.INSTANCE_DTYPE), mats, build=False)):
        with pytest.raises(pt.PtError) as e:
            make()
        assert e.value.code == 1, str(e.value)   # PT_ERR_INVALID
    assert _create_codes(pt, objs, mats) == [1, 1]
    with pytest.raises(pt.PtError) as e:
        pt.Scene(objs, mats, build=False)
    assert "emissive material 1" in str(e.value) and f"radiance[{channel}]" in str(e.value)


def test_valid_radiance_and_other_materials_pass_the_checks(pt):
    """PT_MAX_RADIANCE itself is allowed, and a Lambertian's albedo is not a radiance (today's
    non-validation stays): neither is PT_ERR_INVALID.  Without a GPU both calls get as far as the
    device and report PT_ERR_NODEVICE (5); with one they succeed."""
    expect = [0, 0] if pt.device_count() > 0 else [5, 5]
    for objs, mats in (_one_triangle(pt, pt.PT_EMISSIVE, [pt.PT_MAX_RADIANCE, 0.0, pt.PT_MAX_RADIANCE]),
                       _one_triangle(pt, pt.PT_LAMBERTIAN, [2.0, 2.0, 2.0]),
                       _one_triangle(pt, 16, [float("nan"), -1.0, 5000.0])):   # an unknown type: absorbs, unchecked
        assert _create_codes(pt, objs, mats) == expect


def test_set_sky_rejects_a_null_scene(pt):
    one = np.ones(3, np.float32)
    rc = pt.lib.pt_scene_set_sky(None, one.ctypes.data, one.ctypes.data)
    assert rc == 1 and b"pt_scene_set_sky" in pt.lib.pt_last_error()


# ---------------------------------------------------------------- 4. the lit GPU tests' inputs
def test_L2_paths_end_in_every_way():
    """A condition on the inputs of tests/test_gpu_emission.py, not a tolerance: L2's frame holds
    at least one path of every ending -- sky, absorbed, out of bounces, an emitter seen directly and
    an emitter reached after a bounce -- so each exit of the kernels' SHADE step is compared."""
    ref = pathloop.lit_reference("L2")[0]
    assert pathloop.ending_kinds(ref["kinds"]) == pathloop.ALL_ENDINGS
    sc = pathloop.lit_scene("L2")
    types = set(int(t) for t in sc.materials["type"])
    assert types == {1, 2, 4, 8} and set(int(t) for t in sc.objects["type"]) == {1, 3}
    assert ref["image"].max() > 1.0   # radiance above 1: the 8-bit output has something to clamp


def test_L1_paths_end_in_every_way_its_materials_allow():
    """L1 is the cornell_lit preset: Lambertian walls and the lamp.  A Lambertian never absorbs
    (material.h:28-36 always scatters; only a metal whose fuzzed reflection points into the surface
    does), so "absorbed" cannot occur in L1, whatever the seed; L2 covers it.  Every other ending
    occurs: sky (black here), out of bounces, the lamp seen directly and after a bounce."""
    ref = pathloop.lit_reference("L1")[0]
    sc = pathloop.lit_scene("L1")
    assert set(int(t) for t in sc.materials["type"]) == {1, 8}
    assert pathloop.ending_kinds(ref["kinds"]) == pathloop.ALL_ENDINGS - {"absorbed"}
    assert sc.sky == ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    # black sky: all light in the frame comes from the lamp
    dark = [i for i, (k, _) in enumerate(ref["kinds"]) if k != pathloop.EMITTER]
    assert ref["image"].max() > 1.0 and len(dark) > 0
