"""GPU tests: occlusion ("any hit") queries, pt_trace_occluded / pt_trace_occluded_device.

The contract: occluded[i] == 1 exactly when the closest-hit query of the same ray, tmin and tmax on
the same scene reports hit == 1.  Expected flags come from the CPU oracle's closest-hit trace on
the tight LBVH, or from Scene.trace -- never from the occlusion query itself.  Bar: exact.
"""
import numpy as np
import pytest
import torch  # before libpt.so loads (the two must share torch's HIP runtime)

from helpers import deep_stack_scene, duplicate_centroids, random_rays, random_soup, rays_to_struct

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_ERR_STATE = 1, 6
TMAXES = (np.inf, 12.0, 1.0, 0.5)


def grazing_rays(objs):
    """20,000 rays through triangle vertices, edge points and sphere tangent points (the hits whose
    rounded leaf-box entry can lie beyond the hit), plus 20,000 of helpers.random_rays."""
    rng = np.random.default_rng(3); N = 20000; n = len(objs)
    o = rng.normal(size=(N, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * 15
    k = rng.integers(0, n, N); v = objs["v"][k]; typ = objs["type"][k]
    w = rng.random((N, 1)); w[::3] = 1.0
    edge = v[:, 0:3] * w + v[:, 3:6] * (1 - w)            # triangle vertices and edge points
    perp = np.cross(v[:, :3] - o, rng.normal(size=(N, 3))); perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    tgt = np.where((typ == 1)[:, None], v[:, :3] + perp * v[:, 3:4], edge)   # sphere tangents
    g = np.zeros((N, 6), np.float32); g[:, :3] = o; g[:, 3:] = (tgt - o) * rng.uniform(0.3, 3, (N, 1))
    return np.concatenate([g, random_rays(20000, 7, objects=objs)])


class Soup:
    """The shared scene: objects, oracle LBVH, the grazing ray set and the oracle's closest hits per
    tmax (computed once, never modified)."""

    def __init__(self, pt, orc, gpu):
        self.objs, self.mats = random_soup(300, 40, seed=5)
        self.nodes = orc.build_lbvh(self.objs, orc.morton_keys(self.objs), tight=True)
        self.rays = grazing_rays(self.objs)
        self.rs = rays_to_struct(self.rays, pt.RAY_DTYPE)
        self.scene = pt.Scene(self.objs, self.mats, device=gpu)
        self.ref = {}
        for tmax in TMAXES:
            h, _ = orc.trace(self.objs, self.nodes, self.rays, 0.001, tmax)
            h.setflags(write=False)
            self.ref[tmax] = h
        lo, hi = self.objs["v"][:, :3].min(0), self.objs["v"][:, :3].max(0)
        self.center, self.ext = (lo + hi) / 2, float((hi - lo).max())


@pytest.fixture(scope="module")
def soup(pt, orc, gpu):
    return Soup(pt, orc, gpu)


def all_kernels(pt):
    return (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT, pt.KERNEL_SIMPLE, pt.KERNEL_DEFAULT)


def assert_flags(occ, want_hit, msg=""):
    assert occ.dtype == np.uint8 and occ.shape == want_hit.shape
    bad = np.flatnonzero(occ != (want_hit == 1))
    assert len(bad) == 0, f"{msg}: {len(bad)} flags differ, first rays {bad[:8]}"
    assert set(np.unique(occ)) <= {0, 1}


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tmax", TMAXES)
def test_grazing_set_equals_oracle(pt, orc, soup, tmax):
    want = soup.ref[tmax]["hit"]
    for k in all_kernels(pt):
        occ, st = soup.scene.occluded(soup.rs, 0.001, tmax, kernel=k)
        assert_flags(occ, want, f"tmax {tmax} kernel {k}")
        assert st.rays == len(soup.rs)


def test_grazing_set_needs_the_leaf_box_rule(orc, soup):
    """The set keeps rays whose answer depends on condition (b): the oracle's traversal and its
    brute-force loop over every primitive (no boxes) disagree on them (43 rays on the CPU)."""
    brute, _ = orc.trace(soup.objs, soup.nodes, soup.rays, 0.001, np.inf, brute=True)
    differ = int((brute["hit"] != soup.ref[np.inf]["hit"]).sum())
    print(f"oracle vs brute force: {differ} rays differ")
    assert differ >= 10


# 2 ---------------------------------------------------------------------------------------------
def test_per_ray_tmax_at_the_hit(pt, orc, soup):
    """ray_tmax = the hit's own t, one ulp above and one ulp below: a triangle at exactly tmax does
    not occlude (t < tmax), a sphere root at exactly tmax does (root <= tmax)."""
    ref = soup.ref[np.inf]
    idx = np.flatnonzero(ref["hit"] == 1)[:600]
    assert len(idx) == 600
    rays, rs = soup.rays[idx], soup.rs[idx]
    t = ref["t"][idx].astype(np.float32)
    sph = soup.objs["type"][ref["obj"][idx]] == pt.PT_SPHERE
    assert sph.sum() >= 100 and (~sph).sum() >= 100
    batches = {"at": t, "above": np.nextafter(t, np.float32(np.inf)), "below": np.nextafter(t, np.float32(0))}
    want = {}
    for name, rt in batches.items():   # one single-ray oracle query per (ray, tmax)
        want[name] = np.array([orc.trace(soup.objs, soup.nodes, rays[i:i + 1], 0.001, float(rt[i]))[0]["hit"][0]
                               for i in range(len(idx))])
    print("triangles occluded at t / above: %d / %d of %d; spheres at t / below: %d / %d of %d" % (
        want["at"][~sph].sum(), want["above"][~sph].sum(), (~sph).sum(),
        want["at"][sph].sum(), want["below"][sph].sum(), sph.sum()))
    # both outcomes occur, and the tie rules are the ones stated
    assert want["at"][~sph].sum() == 0 and want["at"][sph].all()
    assert want["above"][~sph].sum() >= 0.9 * (~sph).sum() and want["below"][sph].sum() <= 0.1 * sph.sum()
    assert 0 < want["at"].sum() < len(idx)
    for name, rt in batches.items():
        for k in (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT, pt.KERNEL_SIMPLE):
            # (the scalar tmax is ignored when ray_tmax is given)
            occ, _ = soup.scene.occluded(rs, 0.001, 1e-3, ray_tmax=rt, kernel=k)
            assert_flags(occ, want[name], f"ray_tmax {name} kernel {k}")


# 3 ---------------------------------------------------------------------------------------------
def smallest_scenes(pt):
    objs, mats = random_soup(300, 40, seed=5)
    tri, sph = objs[objs["type"] == pt.PT_TRIANGLE], objs[objs["type"] == pt.PT_SPHERE]
    return [("empty", objs[:0], mats), ("one triangle", tri[:1], mats), ("one sphere", sph[:1], mats),
            ("two primitives", np.concatenate([tri[:1], sph[:1]]), mats), ("duplicates",) + duplicate_centroids(64)]


@pytest.mark.parametrize("which", range(5))
def test_smallest_scenes(pt, orc, gpu, which):
    name, objs, mats = smallest_scenes(pt)[which]
    rays = random_rays(257, seed=11 + which, radius=6.0 if name == "duplicates" else 15.0,
                       objects=objs if len(objs) else None)
    if name == "duplicates":   # aim at points of the shared triangle, not only its centroid
        rays[64:, 3:] = np.random.default_rng(1).dirichlet((1, 1, 1), 193) @ objs["v"][0].reshape(3, 3) - rays[64:, :3]
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True) if len(objs) else np.zeros(0, pt.NODE_DTYPE)
    want = orc.trace(objs, nodes, rays, 0.001, np.inf)[0]["hit"]
    assert (want.sum() > 0) == (len(objs) > 0), name   # (no objects: nothing occludes)
    s = pt.Scene(objs, mats, device=gpu)
    for k in all_kernels(pt):
        occ, st = s.occluded(rays_to_struct(rays, pt.RAY_DTYPE), 0.001, np.inf, kernel=k)
        assert_flags(occ, want, f"{name} kernel {k}")
        assert st.rays == 257


# 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 65, 255, 257, 4099])
def test_ragged_batches(pt, soup, n):
    rs = soup.rs[20000 - n // 2:20000 - n // 2 + n]   # across both halves of the set
    for k in (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT):
        hits, _ = soup.scene.trace(rs, 0.001, np.inf, kernel=k)
        occ, st = soup.scene.occluded(rs, 0.001, np.inf, kernel=k)
        assert_flags(occ, hits["hit"], f"n {n} kernel {k}")
        assert st.rays == n
        if n == 0:
            assert (st.node_visits, st.tri_tests, st.sphere_tests) == (0, 0, 0)


# 5 ---------------------------------------------------------------------------------------------
def test_fallback_rays(pt, orc, soup):
    """Rays the wide kernel answers in the reference's order: origins beyond wideFar's 8 extents, a
    direction component too small for the MIX planes (mixUnsafe), axis-aligned directions."""
    far = random_rays(256, seed=31, center=soup.center, radius=20 * soup.ext, objects=soup.objs)
    tiny = random_rays(256 + 64, seed=32, objects=soup.objs)[64:]   # (without its axis-aligned head)
    tiny[np.arange(256), 3 + np.arange(256) % 3] = np.where(np.arange(256) % 2, 1e-30, -1e-30)
    axis = np.zeros((64, 6), np.float32)
    axis[np.arange(64), 3 + np.arange(64) % 3] = np.where(np.arange(64) % 2, 1.0, -1.0)
    assert (np.count_nonzero(axis[:, 3:], axis=1) == 1).all()
    # aim the axis-aligned rays at primitives: origin = a point of the primitive moved back along the axis
    pick = np.arange(64) * 5 % len(soup.objs)
    v, sph = soup.objs["v"][pick], soup.objs["type"][pick] == pt.PT_SPHERE
    inside = np.where(sph[:, None], v[:, :3], (v[:, 0:3] + v[:, 3:6] + v[:, 6:9]) / 3)
    axis[:, :3] = inside - 20 * axis[:, 3:]
    for name, rays in (("far", far), ("tiny", tiny), ("axis", axis)):
        want = orc.trace(soup.objs, soup.nodes, rays, 0.001, np.inf)[0]["hit"]
        assert 0 < want.sum(), name
        for k in (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT):
            occ, _ = soup.scene.occluded(rays_to_struct(rays, pt.RAY_DTYPE), 0.001, np.inf, kernel=k)
            assert_flags(occ, want, f"{name} kernel {k}")


# 6 ---------------------------------------------------------------------------------------------
def test_work_never_exceeds_closest_hit(pt, soup):
    """The two walks are the same until the first accepted hit, where the occlusion query stops."""
    hit = soup.ref[np.inf]["hit"] == 1
    for k in (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT):
        for name, rs in (("all", soup.rs), ("hitting", soup.rs[hit])):
            _, c = soup.scene.trace(rs, 0.001, np.inf, kernel=k)
            _, a = soup.scene.occluded(rs, 0.001, np.inf, kernel=k)
            cp, ap = c.tri_tests + c.sphere_tests, a.tri_tests + a.sphere_tests
            print(f"kernel {k} {name}: visits {a.node_visits} vs {c.node_visits}, primitive tests {ap} vs {cp}")
            assert a.node_visits <= c.node_visits and ap <= cp
            if name == "hitting":   # more than half of the rays hit (all do)
                assert a.node_visits < c.node_visits and ap < cp


# 7 ---------------------------------------------------------------------------------------------
def test_real_tree(pt, gpu):
    p = pt.Preset("bunny_cornell")
    s = pt.Scene(p.objects, p.materials, device=gpu)
    rng = np.random.default_rng(1)
    n = 20000
    lo, hi = p.objects["v"][:, :3].min(0), p.objects["v"][:, :3].max(0)
    rays = np.zeros(n, pt.RAY_DTYPE)
    rays["o"] = rng.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    rays["d"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    for tmax in (np.inf, 100.0):
        for k in (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT):
            want, _ = s.trace(rays, 0.001, tmax, kernel=k)
            occ, _ = s.occluded(rays, 0.001, tmax, kernel=k)
            assert_flags(occ, want["hit"], f"tmax {tmax} kernel {k}")
    assert 0 < want["hit"].sum() < n   # (tmax = 100: some rays end before the wall)


def test_deep_stack_binary_kernel(pt, orc, gpu):
    """A binary LBVH deeper than 32: the kernel's larger stack sizes are instantiated and used."""
    objs, mats = deep_stack_scene(256)
    s = pt.Scene(objs, mats, device=gpu)
    assert s.bvh_info()["depth"] + 1 > 32
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    rays = np.zeros((64, 6), np.float32)
    rays[:, :3] = 1024.0
    d = np.random.default_rng(2).normal(size=(64, 3))
    rays[:, 3:] = d / np.linalg.norm(d, axis=1, keepdims=True)
    for tmax in (np.inf, 1.0):   # every ray leaves a sphere; or ends before any surface, after the whole tree
        want = orc.trace(objs, nodes, rays, 0.001, tmax)[0]["hit"]
        assert want.all() if tmax == np.inf else not want.any()
        for k in (pt.KERNEL_WAVEFRONT, pt.KERNEL_SIMPLE, pt.KERNEL_WIDE):
            occ, _ = s.occluded(rays_to_struct(rays, pt.RAY_DTYPE), 0.001, tmax, kernel=k)
            assert_flags(occ, want, f"tmax {tmax} kernel {k}")


# 8 ---------------------------------------------------------------------------------------------
def random_transforms(n, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 12), np.float32)
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        s = rng.uniform(0.5, 2.0)
        out[i] = np.concatenate([q * s, rng.uniform(-30, 30, (3, 1))], 1).reshape(-1)
    return out


def flatten(objects, mesh_first, mesh_count, instances):
    """World-space objects of an instanced description (float64 transform, rounded once): targets for the rays."""
    parts = []
    for inst in instances:
        m = inst["m"].astype(np.float64).reshape(3, 4)
        f, c = int(mesh_first[inst["mesh"]]), int(mesh_count[inst["mesh"]])
        o = objects[f:f + c].copy()
        v = o["v"].astype(np.float64)
        out = (v.reshape(-1, 3, 3) @ m[:, :3].T + m[:, 3]).reshape(-1, 9)
        sph = o["type"] == 1
        out[sph, :3] = v[sph, :3] @ m[:, :3].T + m[:, 3]
        out[sph, 3] = v[sph, 3] * np.cbrt(abs(np.linalg.det(m[:, :3])))
        out[sph, 4:] = 0
        o["v"] = out.astype(np.float32)
        parts.append(o)
    return np.concatenate(parts)


def test_instanced(pt, gpu):
    """The 40-instance rotated and scaled scene: flags equal the instanced closest-hit query's."""
    a, mats = random_soup(600, 60, seed=21, spread=4.0)
    b, _ = random_soup(300, 30, seed=22, spread=3.0)
    objs = np.concatenate([a, b])
    inst = np.zeros(40, pt.INSTANCE_DTYPE)
    inst["m"] = random_transforms(40, seed=23)
    inst["mesh"] = np.arange(40) % 2
    si = pt.Scene.instanced(objs, [0, len(a)], [len(a), len(b)], inst, mats, device=gpu)
    flat = flatten(objs, [0, len(a)], [len(a), len(b)], inst)
    lo, hi = flat["v"][:, :3].min(0), flat["v"][:, :3].max(0)
    ext = float((hi - lo).max())
    near = random_rays(16384, seed=24, radius=60.0, objects=flat)
    far = random_rays(2048, seed=25, center=(lo + hi) / 2, radius=50 * ext, objects=flat)   # instEntry
    for name, rays in (("near", near), ("far", far)):
        rs = rays_to_struct(rays, pt.RAY_DTYPE)
        want, _ = si.trace(rs, 0.001, np.inf, kernel=pt.KERNEL_WIDE)
        assert 0 < want["hit"].sum() < len(rs), name
        for k in (pt.KERNEL_WIDE, pt.KERNEL_DEFAULT):
            occ, st = si.occluded(rs, 0.001, np.inf, kernel=k)
            assert_flags(occ, want["hit"], f"{name} kernel {k}")
            assert st.rays == len(rs)
        # a scalar tmax inside the scene, then a per-ray tmax drawn from 8 values (one trace call each)
        t = want["t"][want["hit"] == 1]
        values = np.quantile(t, np.linspace(0.1, 0.9, 8)).astype(np.float32)
        assert len(set(values)) == 8
        w4, _ = si.trace(rs, 0.001, float(values[4]), kernel=pt.KERNEL_WIDE)
        occ, _ = si.occluded(rs, 0.001, float(values[4]), kernel=pt.KERNEL_WIDE)
        assert 0 < w4["hit"].sum() < want["hit"].sum()
        assert_flags(occ, w4["hit"], f"{name} scalar tmax")
        pick = np.random.default_rng(26).integers(0, 8, len(rs))
        wantr = np.zeros(len(rs), np.int32)
        for j, vj in enumerate(values):
            wantr[pick == j] = si.trace(rs, 0.001, float(vj), kernel=pt.KERNEL_WIDE)[0]["hit"][pick == j]
        occ, _ = si.occluded(rs, 0.001, np.inf, ray_tmax=values[pick], kernel=pt.KERNEL_WIDE)
        assert_flags(occ, wantr, f"{name} per-ray tmax")
    with pytest.raises(pt.PtError) as e:
        si.occluded(rs, kernel=pt.KERNEL_WAVEFRONT)
    assert e.value.code == PT_ERR_INVALID


# 9 ---------------------------------------------------------------------------------------------
def test_dynamic_scene(pt, orc, gpu):
    objs, mats = random_soup(300, 40, seed=5)
    rays = random_rays(4099, seed=41, objects=objs)
    rs = rays_to_struct(rays, pt.RAY_DTYPE)
    s = pt.Scene(objs, mats, device=gpu)
    s.occluded(rs)
    new = objs.copy()
    new["v"][:, :3] += np.random.default_rng(42).normal(size=(len(objs), 3)).astype(np.float32)
    tri = new["type"] == pt.PT_TRIANGLE
    new["v"][tri, 3:] += (new["v"][tri, :3] - objs["v"][tri, :3])[:, [0, 1, 2, 0, 1, 2]]
    s.update_objects(new)
    for k in (pt.KERNEL_DEFAULT, pt.KERNEL_WAVEFRONT):   # a stale hierarchy
        with pytest.raises(pt.PtError) as e:
            s.occluded(rs, kernel=k)
        assert e.value.code == PT_ERR_STATE
    s.build_bvh(pt.PT_BVH_WIDE_DEVICE | pt.PT_BVH_ORIGIN_BOUNDS)
    want = orc.trace(new, orc.build_lbvh(new, orc.morton_keys(new), tight=True), rays, 0.001, np.inf)[0]["hit"]
    old = orc.trace(objs, orc.build_lbvh(objs, orc.morton_keys(objs), tight=True), rays, 0.001, np.inf)[0]["hit"]
    assert (want != old).sum() > 0   # the move matters
    for k in (pt.KERNEL_DEFAULT, pt.KERNEL_WAVEFRONT):
        occ, _ = s.occluded(rs, kernel=k)
        assert_flags(occ, want, f"rebuilt, kernel {k}")
    with pytest.raises(pt.PtError) as e:
        s.occluded(rs, kernel=7)
    assert e.value.code == PT_ERR_INVALID


# 10 --------------------------------------------------------------------------------------------
def test_device_arrays(pt, soup, gpu):
    """occluded_device on torch tensors and a non-default stream writes exactly n bytes and equals
    the host-pointer call."""
    n = 4099
    rs = soup.rs[20000 - n // 2:20000 - n // 2 + n]
    rt = np.random.default_rng(51).uniform(0.1, 2.0, n).astype(np.float32)
    dev = torch.device("cuda", gpu)
    rd = torch.from_numpy(rs.view(np.uint8).copy()).to(dev)
    td = torch.from_numpy(rt).to(dev)
    stream = torch.cuda.Stream(dev)
    for k in (pt.KERNEL_WIDE, pt.KERNEL_WAVEFRONT):
        for tmax_ptr, host_rt in ((None, None), (td.data_ptr(), rt)):
            want, wst = soup.scene.occluded(rs, 0.001, 0.8, ray_tmax=host_rt, kernel=k)
            out = torch.full((n + 2,), 0xAA, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            st = soup.scene.occluded_device(rd.data_ptr(), n, out.data_ptr(), 0.001, 0.8, ray_tmax_ptr=tmax_ptr,
                                            kernel=k, stream=stream.cuda_stream)
            got = out.cpu().numpy()
            np.testing.assert_array_equal(got[:n], want)
            assert (got[n:] == 0xAA).all()
            assert 0 < want.sum() < n
            assert (st.rays, st.node_visits, st.tri_tests, st.sphere_tests) == \
                (wst.rays, wst.node_visits, wst.tri_tests, wst.sphere_tests)
    # the per-ray interval matters on this batch
    a, _ = soup.scene.occluded(rs, 0.001, 0.8)
    b, _ = soup.scene.occluded(rs, 0.001, 0.8, ray_tmax=rt)
    assert (a != b).any()
