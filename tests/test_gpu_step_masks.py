"""The render kernels' step scheduling by wave masks, on the GPU.

renderKernelWF keeps its scheduler predicates (lanes on a path, lanes waiting for a task, lanes
with NODE / LEAF / SHADE work) as 64-bit wave masks combined with scalar logic, and takes the
lane's bit back where a step needs it.  A wrong mask loses or repeats a lane's step, so every
check here compares bits: pixels, ray and path counts, and the films' RNG states, between the wide
kernel, the binary wavefront kernel, the one-lane-per-pixel kernel and (bunny_cornell) the oracle.
The cases are the ones mask code can get wrong: fewer tasks than lanes and lanes off the frame
edge, spp that is no multiple of the chunk, paths without a bounce, a film that holds one part of
a frame, step thresholds that force every branch of the kind selection, and both RNG modes (compat
mode twice on one film, so that the critical-pixel waves run).
"""
import numpy as np
import pytest
import torch  # before libpt.so loads (the two must share torch's HIP runtime)

from wall_box import wall_box

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, SEED, CHUNK = 48, 40, 5, 50, 11, 2   # spp is no multiple of the chunk


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame(pt, gpu, s, cam, w, h, spp, depth, kernel, rng, launches=1, film_kw=None, **kw):
    """`launches` renders on one film: the last frame, its stats, the film's RNG states, its rows."""
    f = pt.Film(w, h, SEED, device=gpu, **(film_kw or {}))
    for _ in range(launches):
        rgb, st = pt.render(s, f, cam, spp, depth, kernel=kernel, rng=rng, chunk=CHUNK if rng == pt.RNG_SAMPLE else 0,
                            **kw)
    return rgb, st, f.get_rng(), f.rows


def same_on_all_kernels(pt, gpu, s, cam, w, h, spp, depth, rng, launches=1):
    """The wide kernel's frame against the wavefront and the simple kernel's; returns the wide one."""
    wide = frame(pt, gpu, s, cam, w, h, spp, depth, pt.KERNEL_WIDE, rng, launches)
    for kernel in (pt.KERNEL_WAVEFRONT, pt.KERNEL_SIMPLE):
        other = frame(pt, gpu, s, cam, w, h, spp, depth, kernel, rng, launches)
        np.testing.assert_array_equal(bits(wide[0]), bits(other[0]), err_msg=f"kernel {kernel}")
        np.testing.assert_array_equal(wide[2], other[2], err_msg=f"kernel {kernel}")
        assert (wide[1].rays, wide[1].paths) == (other[1].rays, other[1].paths), kernel
    assert wide[1].paths == w * h * spp
    return wide


@pytest.fixture(scope="module")
def bunny(pt, gpu):
    p = pt.Preset("bunny_cornell", W, H)
    return p, pt.Scene(p.objects, p.materials, device=gpu)


@pytest.fixture(scope="module")
def bunny_oracle(pt, orc):
    """The oracle's frames of bunny_cornell, computed once: sample mode, and two successive compat
    launches (the second starts from the first's RNG states)."""
    p = pt.Preset("bunny_cornell", W, H)
    nodes = orc.build_lbvh(p.objects, orc.morton_keys(p.objects), tight=True)
    cam = pt.camera_to_array(p.camera)
    rows = np.arange(H, dtype=np.int32)
    sample = orc.render_sample(p.objects, p.materials, nodes, cam, W, H, rows, SPP, DEPTH, SEED, CHUNK, nthreads=8)
    states = orc.film_states(SEED, W, rows)
    first = orc.render(p.objects, p.materials, nodes, cam, W, H, rows, SPP, DEPTH, states, nthreads=8)
    second = orc.render(p.objects, p.materials, nodes, cam, W, H, rows, SPP, DEPTH, states, nthreads=8)
    return {"sample": sample, "compat": (first, second), "states": states.copy()}


def test_bunny_cornell_sample_equals_oracle(pt, gpu, bunny, bunny_oracle):
    p, s = bunny
    wide, wst, _, rows = same_on_all_kernels(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.RNG_SAMPLE)
    np.testing.assert_array_equal(rows, np.arange(H))
    ref, rst = bunny_oracle["sample"]
    np.testing.assert_array_equal(bits(wide), bits(ref))
    assert wst.rays == rst.rays


def test_bunny_cornell_compat_two_launches_equal_oracle(pt, gpu, bunny, bunny_oracle):
    p, s = bunny
    for launches in (1, 2):
        wide, wst, wrng, _ = same_on_all_kernels(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.RNG_COMPAT, launches)
        ref, rst = bunny_oracle["compat"][launches - 1]
        np.testing.assert_array_equal(bits(wide), bits(ref))
        assert wst.rays == rst.rays
    np.testing.assert_array_equal(wrng, bunny_oracle["states"])


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (13, 9)])
@pytest.mark.parametrize("rng", ["sample", "compat"])
def test_frames_smaller_than_a_wave_or_a_tile(pt, gpu, rng, w, h):
    """One task, fewer tasks than lanes, and tiles that hang over the right and lower edge."""
    p = pt.Preset("bunny_cornell", w, h)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    r = pt.RNG_SAMPLE if rng == "sample" else pt.RNG_COMPAT
    same_on_all_kernels(pt, gpu, s, p.camera, w, h, SPP, 8, r, launches=1 if rng == "sample" else 2)


@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("rng", ["sample", "compat"])
def test_paths_without_a_bounce(pt, gpu, bunny, rng, depth):
    """max_depth 0: no step loop at all (sample mode hands the tasks out before it); 1: every path
    ends in its first SHADE step."""
    p = pt.Preset("bunny_cornell", 13, 9)
    r = pt.RNG_SAMPLE if rng == "sample" else pt.RNG_COMPAT
    wide, wst, _, _ = same_on_all_kernels(pt, gpu, bunny[1], p.camera, 13, 9, SPP, depth, r)
    assert wst.rays == (13 * 9 * SPP if depth else 0)


@pytest.mark.parametrize("rng", ["sample", "compat"])
def test_one_part_of_a_frame(pt, gpu, bunny, rng):
    """A film with n_parts=3, part=1 renders its rows of the full frame, on every kernel."""
    p, s = bunny
    r = pt.RNG_SAMPLE if rng == "sample" else pt.RNG_COMPAT
    full, _, _, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_WIDE, r)
    kw = {"stripe_height": 8, "n_parts": 3, "part": 1}
    part, pst, prng, rows = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_WIDE, r, film_kw=kw)
    assert 0 < len(rows) < H
    np.testing.assert_array_equal(bits(part).reshape(-1, W, 3), bits(full).reshape(H, W, 3)[rows])
    for kernel in (pt.KERNEL_WAVEFRONT, pt.KERNEL_SIMPLE):
        other, ost, orng, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, kernel, r, film_kw=kw)
        np.testing.assert_array_equal(bits(part), bits(other))
        np.testing.assert_array_equal(prng, orng)
        assert (pst.rays, pst.paths) == (ost.rays, ost.paths) == (ost.rays, len(rows) * W * SPP)


@pytest.mark.parametrize("name", ["bunny_cornell", "rtiow"])
@pytest.mark.parametrize("rng", ["sample", "compat"])
def test_every_branch_of_the_kind_selection(pt, gpu, name, rng):
    """leaf_batch / shade_batch at 1 and 64: LEAF as soon as one lane has a primitive or only when
    no lane has a node left, SHADE likewise: the same frame, rays and RNG states."""
    p = pt.Preset(name, W, H)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    r = pt.RNG_SAMPLE if rng == "sample" else pt.RNG_COMPAT
    ref, rst, rrng, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, pt.KERNEL_SIMPLE, r)
    for kernel in (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT):
        for lb, sb in ((1, 1), (1, 64), (64, 1), (64, 64)):
            img, st, rg, _ = frame(pt, gpu, s, p.camera, W, H, SPP, DEPTH, kernel, r, leaf_batch=lb, shade_batch=sb)
            np.testing.assert_array_equal(bits(img), bits(ref), err_msg=f"kernel {kernel} batches {lb} {sb}")
            np.testing.assert_array_equal(rg, rrng, err_msg=f"kernel {kernel} batches {lb} {sb}")
            assert (st.rays, st.paths) == (rst.rays, rst.paths), (kernel, lb, sb)


@pytest.mark.parametrize("rng", ["sample", "compat"])
def test_sphere_branch_of_leaf(pt, gpu, rng):
    p = pt.Preset("rtiow", W, H)
    s = pt.Scene(p.objects, p.materials, device=gpu)
    r = pt.RNG_SAMPLE if rng == "sample" else pt.RNG_COMPAT
    _, st, _, _ = same_on_all_kernels(pt, gpu, s, p.camera, W, H, SPP, DEPTH, r, launches=1 if rng == "sample" else 2)
    assert st.sphere_tests > 0   # (counted from the step's masks)


@pytest.mark.parametrize("rng", ["sample", "compat"])
def test_redo_branch(pt, gpu, rng):
    """The box of doubled walls (tests/test_gpu_deferred_leafbox.py): about a third of the queries
    are repeated in the reference's order inside the SHADE step."""
    objs, mats = wall_box(doubled=True)
    s = pt.Scene(objs, mats, device=gpu)
    cam = pt.camera_make((270.0, 280.0, 40.0), (200.0, 250.0, 500.0), 70.0, 1.0)
    r = pt.RNG_SAMPLE if rng == "sample" else pt.RNG_COMPAT
    _, st, _, _ = same_on_all_kernels(pt, gpu, s, cam, 32, 32, 3, 12, r, launches=1 if rng == "sample" else 2)
    assert st.rays > 32 * 32 * 3 * 6   # a closed box: paths run to their depth


@pytest.mark.parametrize("rng", ["sample", "compat"])
def test_instanced_kernel(pt, gpu, rng):
    """The instanced instantiation: cornell's one identity instance gives the flattened scene's frame
    bit for bit (tests/test_gpu_instancing.py), and bunny_cornell's frame does not depend on the
    step thresholds."""
    r = pt.RNG_SAMPLE if rng == "sample" else pt.RNG_COMPAT
    ip, fp = pt.InstancedPreset("cornell", W, H), pt.Preset("cornell", W, H)
    si = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, ip.instances, ip.materials, device=gpu)
    sf = pt.Scene(fp.objects, fp.materials, device=gpu)
    a, ast, arng, _ = frame(pt, gpu, si, ip.camera, W, H, SPP, ip.max_depth, pt.KERNEL_WIDE, r)
    b, bst, brng, _ = frame(pt, gpu, sf, fp.camera, W, H, SPP, fp.max_depth, pt.KERNEL_WIDE, r)
    np.testing.assert_array_equal(bits(a), bits(b))
    np.testing.assert_array_equal(arng, brng)
    assert (ast.rays, ast.paths) == (bst.rays, bst.paths) == (bst.rays, W * H * SPP)
    ip = pt.InstancedPreset("bunny_cornell", W, H)
    si = pt.Scene.instanced(ip.objects, ip.mesh_first, ip.mesh_count, ip.instances, ip.materials, device=gpu)
    a, ast, arng, _ = frame(pt, gpu, si, ip.camera, W, H, SPP, ip.max_depth, pt.KERNEL_WIDE, r)
    for lb, sb in ((1, 64), (64, 1)):
        b, bst, brng, _ = frame(pt, gpu, si, ip.camera, W, H, SPP, ip.max_depth, pt.KERNEL_WIDE, r, leaf_batch=lb,
                                shade_batch=sb)
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"batches {lb} {sb}")
        np.testing.assert_array_equal(arng, brng)
        assert (ast.rays, ast.paths) == (bst.rays, bst.paths)
