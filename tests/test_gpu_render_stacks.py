"""The lit, NEE, MIS and instanced render kernels at every traversal-stack size a small scene can reach.

Every render kernel is compiled once per stack size and the host picks the copy from the tree's depth
(pt_device.hip: wideStackFor, stackFor).  The scenes of the other lit tests have wide trees of depth <= 8
(tests/test_stack_scenes_host.py shows it), so they only ever run the 8-entry wide copies; the scenes of
tests/stack_scenes.py select the others, and that file's docstring holds the table of scene -> depth,
stack and kernel family.  Each case first checks that its scene does select the size it names.

The bar is the project's usual one, tolerance 0: image bits, film.get_rng() after compat launches
(unchanged after sample-mode ones), rays and paths, against the restatement of tests/pathloop_mis.py,
which tests/test_stack_scenes_host.py holds to the oracle with the rules off.  An identity instance is
the flat scene bit for bit (include/pt.h), so the flat references hold the instanced frames too --
as long as no ray finds two primitives at exactly the same t, which a flat scene decides in the
reference's order and an instanced one by (instance, primitive): the wide scenes have no two triangles in
one plane for that reason (stack_scenes.chains; a first version with a coplanar chain differed from the
flat frame in 15 to 24 pixels, each through such a tie, at every stack size, 8 entries included).
"""
import numpy as np
import pytest

import pathloop_mis as pm
import stack_scenes as ss
from pathloop import DEFAULT_SKY, SEED

pytestmark = pytest.mark.gpu

W, H = ss.W, ss.H
RNGS = ("compat", "sample")
FLAGS = {"blind": {}, "lit": {}, "nee": {"nee": True}, "mis": {"mis": True}}
IDENTITY = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)

# The depth PT_BVH_WIDE_DEVICE's builder reports per scene (found on the GPU): on these chains the same as
# the host builder's (tests/stack_scenes.py), so the device-built trees select the same stack sizes.
DEVICE_DEPTH = {"T16": 12, "S16": 11, "T24": 19, "S24": 19}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def camera_of(pt, sc):
    return pt.Camera.from_buffer_copy(sc.camera.tobytes())


@pytest.fixture(scope="module")
def scenes(pt, gpu):
    """Device scenes, built once per (name, kind, blind): kind 'flat', 'device' (PT_BVH_WIDE_DEVICE),
    'instanced' (one mesh, one identity instance, PT_BVH_LIGHTS) or 'updated' (the same laid out for
    updates, then update_instances to the same matrix and a rebuild of the top level: source 4)."""
    made = {}

    def get(name, kind="flat", blind=False):
        key = (name, kind, blind)
        if key in made:
            return made[key]
        sc = ss.scene(name)
        mats = sc.blind_materials if blind else sc.materials
        if kind in ("flat", "device"):
            flags = pt.PT_BVH_ORIGIN_BOUNDS | (pt.PT_BVH_WIDE_DEVICE if kind == "device" else 0)
            s = pt.Scene(sc.objects, mats, device=gpu, flags=flags)
        else:
            inst = np.zeros(1, pt.INSTANCE_DTYPE)
            inst["m"][0] = IDENTITY
            flags = pt.PT_BVH_LIGHTS | (pt.PT_BVH_WIDE_DEVICE if kind == "updated" else 0)
            s = pt.Scene.instanced(sc.objects, [0], [len(sc.objects)], inst, mats, device=gpu, flags=flags)
            assert s.wide_info()["source"] == 3
            if kind == "updated":
                s.update_instances(inst)
                s.build_bvh(flags)
                s.build_bvh(flags)
                assert s.wide_info()["source"] == 4
        s.set_sky(*(DEFAULT_SKY if blind else sc.sky))
        assert s.n_lights == (0 if blind else len(pm.light_list(sc.objects, sc.materials)[0]))
        made[key] = s
        return s

    return get


def render_and_compare(pt, gpu, s, name, mode, rng, kernel, before_compare=None):
    """One frame of `mode` in `rng` on a fresh film against stack_scenes.reference; returns the stats."""
    sc = ss.scene(name)
    cam = camera_of(pt, sc)
    f = pt.Film(W, H, SEED, device=gpu)
    ref = ss.reference(name, mode, rng)[0]
    if rng == "compat":
        rgb, st = pt.render(s, f, cam, ss.SPP, ss.DEPTH, kernel=kernel, **FLAGS[mode])
    else:
        before = f.get_rng()
        rgb, st = pt.render(s, f, cam, ss.SAMPLE_SPP, ss.DEPTH, kernel=kernel, rng=pt.RNG_SAMPLE, chunk=ss.SAMPLE_CHUNK,
                            **FLAGS[mode])
    if before_compare:
        before_compare()
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    if rng == "compat":
        np.testing.assert_array_equal(f.get_rng(), ref["states"])
    else:
        np.testing.assert_array_equal(f.get_rng(), before)   # sample mode leaves the film's streams alone
    assert st.rays == ref["rays"] and st.paths == ref["paths"]
    return st


def selects_wide(s, stack, depth=None):
    d = s.wide_info()["depth"]
    assert ss.wide_stack(d) == stack, d
    assert depth is None or d == depth, d


def sphere_counter(name, st):
    if ss.WIDE[name][2]:
        assert st.sphere_tests > 0    # the generic kernels
    else:
        assert st.sphere_tests == 0   # the TRI kernels' scenes hold no sphere


# ---------------------------------------------------------------- 1. wide kernels, flat scenes
@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("mode", list(FLAGS))
@pytest.mark.parametrize("name", list(ss.WIDE))
def test_wide_flat(pt, gpu, scenes, name, mode, rng):
    """renderKernelWF<16 | 24, rng, WIDE, blind / LIT / NEE / MIS, TRI (T16, T24) | generic (S16, S24)>."""
    s = scenes(name, blind=mode == "blind")
    # (a flat scene's wide tree is built by the first wide launch: its depth is known after it)
    st = render_and_compare(pt, gpu, s, name, mode, rng, pt.KERNEL_WIDE,
                            before_compare=lambda: selects_wide(s, ss.WIDE[name][0]))
    assert s.wide_info()["source"] == 1
    sphere_counter(name, st)


@pytest.mark.parametrize("name", list(ss.WIDE))
def test_wide_flat_two_compat_launches_at_long_depth(pt, gpu, scenes, name):
    """Compat mode, max depth 20, one film: two NEE launches, then two lit ones.  At max depth > 16 a
    film's second launch is scheduled from the first one's costs -- its longest tiles split over two
    waves; the critical-pixel waves of test_nee_second_compat_launch_at_long_depth exist in the 8-entry
    kernels only (pt_device.hip: critFor)."""
    sc = ss.scene(name)
    s, cam = scenes(name), camera_of(pt, sc)
    f = pt.Film(W, H, SEED, device=gpu)
    for ref in ss.reference(name, "nee", "compat", max_depth=ss.LONG_DEPTH, frames=2, spp=ss.LONG_SPP):
        rgb, st = pt.render(s, f, cam, ss.LONG_SPP, ss.LONG_DEPTH, kernel=pt.KERNEL_WIDE, nee=True)
        selects_wide(s, ss.WIDE[name][0])
        np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
        np.testing.assert_array_equal(f.get_rng(), ref["states"])
        assert st.rays == ref["rays"] and st.paths == ref["paths"]
    for _ in range(2):
        before = f.get_rng()
        rgb, st = pt.render(s, f, cam, ss.LONG_SPP, ss.LONG_DEPTH, kernel=pt.KERNEL_WIDE)
        want = pm.render(sc.objects, sc.materials, sc.nodes, sc.camera, W, H, range(H), ss.LONG_SPP, ss.LONG_DEPTH, before,
                         sky=sc.sky)
        np.testing.assert_array_equal(bits(rgb), bits(want["image"]))
        np.testing.assert_array_equal(f.get_rng(), want["states"])
        assert st.rays == want["rays"]


@pytest.mark.parametrize("part", [0, 1])
def test_wide_partitioned_film(pt, gpu, scenes, part):
    """The 24-entry MIS kernel, sample mode, on one part of a film of 3-row stripes dealt to two parts."""
    sc = ss.scene("S24")
    s, cam = scenes("S24"), camera_of(pt, sc)
    f = pt.Film(W, H, SEED, device=gpu, stripe_height=3, n_parts=2, part=part)
    assert 0 < f.n_rows < H
    ref = ss.reference("S24", "mis", "sample", rows=tuple(int(r) for r in f.rows))[0]
    rgb, st = pt.render(s, f, cam, ss.SAMPLE_SPP, ss.DEPTH, kernel=pt.KERNEL_WIDE, rng=pt.RNG_SAMPLE, chunk=ss.SAMPLE_CHUNK,
                        mis=True)
    selects_wide(s, 24)
    np.testing.assert_array_equal(bits(rgb), bits(ref["image"]))
    assert st.rays == ref["rays"] and st.paths == ref["paths"] == f.n_pixels * ss.SAMPLE_SPP
    full = ss.reference("S24", "mis", "sample")[0]["image"].reshape(H, W, 3)
    np.testing.assert_array_equal(bits(rgb.reshape(-1, W, 3)), bits(full[f.rows]))


# ---------------------------------------------------------------- 2. device-built wide trees
@pytest.mark.parametrize("mode,rng", [("nee", "compat"), ("mis", "sample")])
@pytest.mark.parametrize("name", list(ss.WIDE))
def test_wide_device_built_tree(pt, gpu, scenes, name, mode, rng):
    """The same frames from the tree PT_BVH_WIDE_DEVICE builds (source 2): another tree, the same bits."""
    s = scenes(name, "device")
    assert s.wide_info()["source"] == 2
    depth = s.wide_info()["depth"]
    print(name, "device-built wide depth", depth, "stack", ss.wide_stack(depth))
    assert depth == DEVICE_DEPTH[name] and ss.wide_stack(depth) == ss.WIDE[name][0]
    st = render_and_compare(pt, gpu, s, name, mode, rng, pt.KERNEL_WIDE)
    assert s.wide_info()["source"] == 2
    sphere_counter(name, st)


# ---------------------------------------------------------------- 3. instanced wide kernels
@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("mode", list(FLAGS))
@pytest.mark.parametrize("kind", ["instanced", "updated"])
@pytest.mark.parametrize("name", list(ss.WIDE))
def test_wide_instanced(pt, gpu, scenes, name, kind, mode, rng):
    """The scene as one mesh placed once by the identity: the instanced kernels (blind, LIT, NEE, MIS) at
    16 and 24 entries -- the instance adds three levels (top level, marker, mesh root) -- from the full
    host build and from the layout for updates after update_instances and a top-level rebuild."""
    s = scenes(name, kind, blind=mode == "blind")
    selects_wide(s, ss.WIDE[name][0])
    st = render_and_compare(pt, gpu, s, name, mode, rng, pt.KERNEL_WIDE)
    sphere_counter(name, st)


# ---------------------------------------------------------------- 4. binary kernels
def selects_binary(s, stack):
    d = s.bvh_info()["depth"]
    assert ss.bin_stack(d) == stack, d


@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("mode", list(FLAGS))
@pytest.mark.parametrize("name", list(ss.BINARY))
def test_simple_kernel(pt, gpu, scenes, name, mode, rng):
    """renderKernel<24 | 32 | 48, rng, blind / LIT / NEE / MIS>: the rule as a nested query on the binary tree."""
    s = scenes(name, blind=mode == "blind")
    selects_binary(s, ss.BINARY[name])
    render_and_compare(pt, gpu, s, name, mode, rng, pt.KERNEL_SIMPLE)


@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("mode", ["blind", "lit"])
@pytest.mark.parametrize("name", list(ss.BINARY))
def test_wavefront_kernel(pt, gpu, scenes, name, mode, rng):
    """renderKernelWF<24 | 32 | 48, rng, WIDE = false, .., blind / LIT>; at 48 entries the sample-mode kernel
    keeps the entries above 32 in the global spill buffer, and leaves it through the emissive exit too."""
    s = scenes(name, blind=mode == "blind")
    selects_binary(s, ss.BINARY[name])
    st = render_and_compare(pt, gpu, s, name, mode, rng, pt.KERNEL_WAVEFRONT)
    assert st.node_visits > 0


def test_wavefront_kernel_refuses_nee(pt, gpu, scenes):
    sc = ss.scene("B32")
    f = pt.Film(W, H, SEED, device=gpu)
    out = np.full((f.n_pixels, 3), -7.0, np.float32)
    with pytest.raises(pt.PtError) as e:
        pt.render(scenes("B32"), f, camera_of(pt, sc), 1, 4, out=out, kernel=pt.KERNEL_WAVEFRONT, nee=True)
    assert e.value.code == 1 and (out == -7.0).all()   # PT_ERR_INVALID, nothing launched
