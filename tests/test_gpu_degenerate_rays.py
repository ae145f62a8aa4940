"""GPU tests: the ray queries on degenerate rays and intervals (the contract next to pt_trace_closest
in include/pt.h).  Any bit pattern is a legal ray; the result is the reference's closest hit except
that a candidate whose t is NaN is not a hit (oracle.trace(..., nan_miss=True)); tmin < 0, a NaN tmin
and a NaN scalar tmax are PT_ERR_INVALID; a NaN ray_tmax[i] is no upper bound.  Bar: exact -- every
field of every record, t / p / n compared as bit patterns -- wherever the oracle is the reference;
the instanced scene (no oracle: its rays are transformed) is held to the rule's consequences only.

Why every walk ends whatever the float values are (read before the first run of these inputs):
  trace<> / binVisit: an internal node is pushed at most once, by its parent's visit, so a query
    makes at most nprims - 1 visits; the guard counter (> nprims: PT_ERR_STATE) cannot trip on a
    sound tree.  A ray that passes every box (NaN: the min / max of the slab test drop NaN planes)
    holds at most one pending sibling per level: depth + 1 entries, what stackFor allots.
  traceRefStackless: a state machine over parent links, no stack.  A node is entered from its parent
    once and left once; the float tests only choose which children are entered, never whether the
    walk returns.  2 (nprims - 1) steps at most, inside its bound of 4 nprims + 1 (which reports a
    corrupt tree through the guard word, never loops).
  wideStep: each step clears one bit of the current node's child mask or pops; a node's remaining
    children are pushed once, so the stack holds one entry per level (wideStackFor), and a ray that
    passes every plane test visits every node once.
  instanced: entering an instance pushes one marker, popped once on the way back (it restores the
    world ray); the mesh tree's walk above it is wideStep's.  Top-level depth + 1 + mesh depth entries.
  No loop's exit depends on a float comparison.

What these tests found when they were written (each is fixed and stays covered here):
  - no entry point validated the interval (a negative or NaN tmin returned PT_OK);
  - a one-primitive scene, wide kernel: the root's box test dropped the reference's box-free hits at
    t = +inf of x1e18 directions (9 of 256 rays, both trees, closest hit and occlusion);
  - a signalling NaN in ray_tmax made the wide occlusion kernel miss everything for that ray (33 of the
    soup batch's 4864 flags at tmin 0.001, 64 at tmin 0), and any NaN there differed from +inf on an
    instanced scene's rays with denormal directions (2 of 4864).
"""
import ctypes as C

import numpy as np
import pytest
import torch  # before libpt.so loads (the two must share torch's HIP runtime)

import degenerate_rays as dr

pytestmark = pytest.mark.gpu

PT_ERR_INVALID = 1
SCENES = {"soup": dr.soup, "one_sphere": dr.one_sphere, "one_triangle": dr.one_triangle, "empty": dr.empty}
FIELDS = ("hit", "obj", "mat", "front_face", "t", "p", "n")


def structs(pt, rays):
    """(n, 6) float32 -> pt_ray records, bit for bit (NaN payloads included)."""
    return np.ascontiguousarray(rays, np.float32).view(pt.RAY_DTYPE).reshape(-1)


def miss_record(pt, n=1):
    m = np.zeros(n, pt.HIT_DTYPE)
    m["obj"] = m["mat"] = -1
    return m


def assert_records_equal(got, want, msg):
    """Every field of every record; floats as bit patterns (inf, NaN payloads and the sign of zero count)."""
    for f in FIELDS:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        if f in ("t", "p", "n"):
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero((g != w).reshape(len(got), -1).any(axis=1))
        assert len(bad) == 0, f"{msg}: `{f}` differs on {len(bad)} rays, first {bad[:6]}: got {got[bad[:3]]} want {want[bad[:3]]}"


class Flat:
    """One flat scene: its ray classes in one batch, a host-built and a device-built wide tree, and
    the oracle's records under the rule per interval (computed once, read-only)."""

    def __init__(self, pt, orc, gpu, name):
        self.name = name
        self.objs, self.mats = SCENES[name]()
        self.nodes = (orc.build_lbvh(self.objs, orc.morton_keys(self.objs), tight=True) if len(self.objs)
                      else np.zeros(0, pt.NODE_DTYPE))
        self.classes = dr.ray_classes(self.objs, dr.base_rays(self.objs, reach=0.25 if name == "soup" else 0.75))
        self.batch, self.where = dr.concat(self.classes)
        assert len(self.batch) % 64 == 0
        self.rs = structs(pt, self.batch)
        self.host = pt.Scene(self.objs, self.mats, device=gpu)
        self.dev = pt.Scene(self.objs, self.mats, device=gpu, flags=pt.PT_BVH_ORIGIN_BOUNDS | pt.PT_BVH_WIDE_DEVICE)
        self.orc, self.refs = orc, {}

    def ref(self, interval, rays=None):
        if rays is not None:
            return self.orc.trace(self.objs, self.nodes, rays, *interval, nan_miss=True)[0]
        if interval not in self.refs:
            h = self.orc.trace(self.objs, self.nodes, self.batch, *interval, nan_miss=True)[0]
            h.setflags(write=False)
            self.refs[interval] = h
        return self.refs[interval]


_flats = {}


@pytest.fixture
def flat(request, pt, orc, gpu, monkeypatch):
    monkeypatch.delenv("PT_WIDE_BUILD", raising=False)
    monkeypatch.delenv("PT_TRACE_STRIDE", raising=False)
    name = request.param
    if name not in _flats:
        _flats[name] = Flat(pt, orc, gpu, name)
    return _flats[name]


def closest_configs(pt, flat):
    """(label, scene, kernel, PT_TRACE_STRIDE): the binary kernels and the wide kernel on both trees,
    each as the queued and as the grid-stride kernel."""
    for stride in ("0", "1"):
        for kernel, kn in ((pt.KERNEL_SIMPLE, "simple"), (pt.KERNEL_WAVEFRONT, "wavefront")):
            yield f"{kn} stride={stride}", flat.host, kernel, stride
        for scene, tn in ((flat.host, "host tree"), (flat.dev, "device tree")):
            yield f"wide {tn} stride={stride}", scene, pt.KERNEL_WIDE, stride


def occluded_configs(pt, flat):
    for kernel, kn in ((pt.KERNEL_SIMPLE, "simple"), (pt.KERNEL_WAVEFRONT, "wavefront")):
        yield kn, flat.host, kernel
    for scene, tn in ((flat.host, "host tree"), (flat.dev, "device tree")):
        for kernel, kn in ((pt.KERNEL_WIDE, "wide"), (pt.KERNEL_DEFAULT, "default")):
            yield f"{kn} {tn}", scene, kernel


def check_trees(flat):
    if len(flat.objs):
        assert flat.host.wide_info()["source"] == 1 and flat.dev.wide_info()["source"] == 2


# ------------------------------------------------------------------------------- flat scenes
@pytest.mark.parametrize("interval", dr.INTERVALS, ids=lambda iv: f"{iv[0]}..{iv[1]}")
@pytest.mark.parametrize("flat", list(SCENES), indirect=True)
def test_closest_hit_is_the_rule(pt, flat, interval, monkeypatch):
    want = flat.ref(interval)
    for label, scene, kernel, stride in closest_configs(pt, flat):
        monkeypatch.setenv("PT_TRACE_STRIDE", stride)
        hits, st = scene.trace(flat.rs, *interval, kernel=kernel)
        for name, sl in flat.where.items():
            assert_records_equal(hits[sl], want[sl], f"{flat.name} {interval} {label} class {name}")
        assert st.rays == len(flat.rs), label
        for name in dr.nan_classes():
            assert (hits[flat.where[name]] == miss_record(pt)).all(), (label, name)
    check_trees(flat)
    if flat.name != "empty" and interval == dr.INTERVALS[0]:   # the batch is not a batch of misses
        assert want["hit"][flat.where["control"]].sum() > 0
    if flat.name == "soup" and interval == dr.INTERVALS[1]:
        assert want["hit"][flat.where["d_1e18"]].sum() > 0 and np.isposinf(want["t"][flat.where["d_1e-30"]]).sum() > 0
    if interval[1] < interval[0]:
        assert want["hit"].sum() == 0


@pytest.mark.parametrize("interval", dr.INTERVALS, ids=lambda iv: f"{iv[0]}..{iv[1]}")
@pytest.mark.parametrize("flat", list(SCENES), indirect=True)
def test_occlusion_is_the_closest_hit_flag(pt, flat, interval):
    want = flat.ref(interval)["hit"]
    for label, scene, kernel in occluded_configs(pt, flat):
        occ, st = scene.occluded(flat.rs, *interval, kernel=kernel)
        bad = np.flatnonzero(occ != want)
        assert len(bad) == 0, f"{flat.name} {interval} {label}: {len(bad)} flags differ, first rays {bad[:8]}"
        assert occ.dtype == np.uint8 and st.rays == len(flat.rs)


@pytest.mark.parametrize("flat", list(SCENES), indirect=True)
def test_ragged_batch(pt, flat, monkeypatch):
    """The batch without its first 37 rays: not a multiple of 64, and every class boundary inside a wave."""
    interval = dr.INTERVALS[1]
    rs, want = flat.rs[37:], flat.ref(interval)[37:]
    assert len(rs) % 64 != 0
    for label, scene, kernel, stride in closest_configs(pt, flat):
        monkeypatch.setenv("PT_TRACE_STRIDE", stride)
        hits, st = scene.trace(rs, *interval, kernel=kernel)
        assert_records_equal(hits, want, f"{flat.name} ragged {label}")
        assert st.rays == len(rs)
    for label, scene, kernel in occluded_configs(pt, flat):
        occ, _ = scene.occluded(rs, *interval, kernel=kernel)
        assert np.array_equal(occ, want["hit"]), label


@pytest.mark.parametrize("tmin", [0.001, 0.0])
@pytest.mark.parametrize("flat", list(SCENES), indirect=True)
def test_nan_ray_tmax_is_no_upper_bound(pt, flat, tmin):
    """ray_tmax with NaN (quiet and signalling) and inf entries among four finite values: a NaN entry
    gives the tmax = inf answer, every other ray the oracle's answer for its own tmax."""
    rt, plain = dr.mixed_ray_tmax(len(flat.rs))
    want = np.zeros(len(flat.rs), np.int32)
    for v in np.unique(plain):
        want[plain == v] = flat.ref((tmin, float(v)))["hit"][plain == v]
    nan = np.isnan(rt)
    assert np.array_equal(want[nan], flat.ref((tmin, np.inf))["hit"][nan])
    if flat.name == "soup":   # the finite values cut hits off: the per-ray bound is in use
        assert want[~nan].sum() < flat.ref((tmin, np.inf))["hit"][~nan].sum() and want[nan].sum() > 0
    for label, scene, kernel in occluded_configs(pt, flat):
        for name, values in (("with NaN", rt), ("NaN as inf", plain)):
            occ, _ = scene.occluded(flat.rs, tmin, 1e-3, ray_tmax=values, kernel=kernel)   # (the scalar is ignored)
            bad = np.flatnonzero(occ != want)
            assert len(bad) == 0, (f"{flat.name} {label} ray_tmax {name}: {len(bad)} flags differ, first rays {bad[:8]}, "
                                   f"their ray_tmax bits {[hex(b) for b in values.view(np.uint32)[bad[:8]]]}, got {occ[bad[:8]]}")


@pytest.mark.parametrize("flat", ["soup", "one_sphere"], indirect=True)
def test_poisoned_batch(pt, flat, monkeypatch):
    """Ordinary rays interleaved lane by lane with NaN, zero-direction and x1e18 rays: their records
    are those of the same rays traced alone, and the oracle's."""
    batch, at = dr.poisoned(flat.classes)
    alone = structs(pt, flat.classes["control"])
    for interval in dr.INTERVALS[:2]:
        want = flat.ref(interval, batch)
        assert want["hit"][at].sum() > 0
        for n in (len(batch), len(batch) - 37):
            keep = at[at < n]
            for label, scene, kernel, stride in closest_configs(pt, flat):
                monkeypatch.setenv("PT_TRACE_STRIDE", stride)
                mixed, _ = scene.trace(structs(pt, batch[:n]), *interval, kernel=kernel)
                solo, _ = scene.trace(alone, *interval, kernel=kernel)
                assert mixed[keep].tobytes() == solo[:len(keep)].tobytes(), f"{flat.name} {interval} {label} n={n}"
                assert_records_equal(mixed, want[:n], f"{flat.name} poisoned {interval} {label} n={n}")
            for label, scene, kernel in occluded_configs(pt, flat):
                occ, _ = scene.occluded(structs(pt, batch[:n]), *interval, kernel=kernel)
                assert np.array_equal(occ, want["hit"][:n]), label


def on_device(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def device_closest(pt, scene, rs, interval, kernel, dev, stream):
    rd = on_device(rs, dev)
    out = torch.full((len(rs) * pt.HIT_DTYPE.itemsize + 64,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    st = scene.trace_device(rd.data_ptr(), len(rs), out.data_ptr(), *interval, kernel=kernel, stream=stream.cuda_stream)
    got = out.cpu().numpy()
    assert (got[-64:] == 0xAA).all()
    return got[:-64].view(pt.HIT_DTYPE), st


def device_occluded(pt, scene, rs, interval, kernel, dev, stream, ray_tmax=None):
    rd = on_device(rs, dev)
    td = None if ray_tmax is None else on_device(ray_tmax, dev)
    out = torch.full((len(rs) + 64,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    st = scene.occluded_device(rd.data_ptr(), len(rs), out.data_ptr(), *interval,
                               ray_tmax_ptr=None if td is None else td.data_ptr(), kernel=kernel,
                               stream=stream.cuda_stream)
    got = out.cpu().numpy()
    assert (got[-64:] == 0xAA).all()
    return got[:-64], st


def work(st):
    return (st.rays, st.node_visits, st.tri_tests, st.sphere_tests)


@pytest.mark.parametrize("flat", list(SCENES), indirect=True)
def test_device_pointer_entries(pt, flat, gpu):
    """pt_trace_closest_device / pt_trace_occluded_device on torch tensors and a stream of their own:
    the host-pointer calls' results and work counters."""
    dev = torch.device("cuda", gpu)
    stream = torch.cuda.Stream(dev)
    rt, _ = dr.mixed_ray_tmax(len(flat.rs))
    for interval in (dr.INTERVALS[1], dr.INTERVALS[3]):
        want = flat.ref(interval)
        for label, scene, kernel in occluded_configs(pt, flat):
            if kernel != pt.KERNEL_DEFAULT:
                hits, hst = scene.trace(flat.rs, *interval, kernel=kernel)
                got, st = device_closest(pt, scene, flat.rs, interval, kernel, dev, stream)
                assert got.tobytes() == hits.tobytes() and work(st) == work(hst), label
                assert_records_equal(got, want, f"{flat.name} device pointers {interval} {label}")
            for values in (None, rt):
                occ, ost = scene.occluded(flat.rs, *interval, ray_tmax=values, kernel=kernel)
                got, st = device_occluded(pt, scene, flat.rs, interval, kernel, dev, stream, values)
                assert np.array_equal(got, occ) and work(st) == work(ost), label
                if values is None:
                    assert np.array_equal(got, want["hit"]), label


# ------------------------------------------------------------------------------- the instanced scene
class Instanced:
    def __init__(self, pt, gpu):
        self.objs, self.mats, self.inst = dr.two_instances()
        self.scene = pt.Scene.instanced(self.objs, [0], [len(self.objs)], self.inst, self.mats, device=gpu)
        self.classes = dr.ray_classes(self.objs, dr.instanced_base(self.objs, self.inst))
        self.batch, self.where = dr.concat(self.classes)
        self.rs = structs(pt, self.batch)


@pytest.fixture(scope="module")
def instanced(pt, gpu):
    return Instanced(pt, gpu)


def instanced_trace(pt, si, rs, interval, monkeypatch):
    """Both kernels (queued, grid-stride); each call returning at all is PT_OK with the guard word clear
    (ptamd raises on anything else).  They agree bit for bit."""
    monkeypatch.setenv("PT_TRACE_STRIDE", "1")
    a, ast = si.scene.trace(rs, *interval, kernel=pt.KERNEL_WIDE)
    monkeypatch.delenv("PT_TRACE_STRIDE")
    b, bst = si.scene.trace(rs, *interval, kernel=pt.KERNEL_DEFAULT)
    assert a.tobytes() == b.tobytes() and ast.rays == bst.rays == len(rs)
    assert set(np.unique(a["hit"])) <= {0, 1}
    return a


@pytest.mark.parametrize("interval", dr.INTERVALS, ids=lambda iv: f"{iv[0]}..{iv[1]}")
def test_instanced_scene(pt, instanced, interval, gpu, monkeypatch):
    si = instanced
    hits = instanced_trace(pt, si, si.rs, interval, monkeypatch)
    for name in dr.nan_classes():
        assert (hits[si.where[name]] == miss_record(pt)).all(), name
    h = hits["hit"] == 1
    assert (hits[~h] == miss_record(pt)).all() and not np.isnan(hits["t"][h]).any()
    n = len(si.objs)
    assert ((hits["obj"][h] >= 0) & (hits["obj"][h] < 2 * n)).all()
    if interval == dr.INTERVALS[0]:   # the ordinary rays meet both instances
        c = hits[si.where["control"]]
        assert ((c["hit"] == 1) & (c["obj"] < n)).sum() > 10 and ((c["hit"] == 1) & (c["obj"] >= n)).sum() > 10
    if interval[1] < interval[0]:
        assert h.sum() == 0
    dev = torch.device("cuda", gpu)
    stream = torch.cuda.Stream(dev)
    for kernel in (pt.KERNEL_WIDE, pt.KERNEL_DEFAULT):
        occ, st = si.scene.occluded(si.rs, *interval, kernel=kernel)
        assert np.array_equal(occ, hits["hit"]) and st.rays == len(si.rs), kernel
    got, _ = device_closest(pt, si.scene, si.rs, interval, pt.KERNEL_WIDE, dev, stream)
    assert got.tobytes() == hits.tobytes()
    got, _ = device_occluded(pt, si.scene, si.rs, interval, pt.KERNEL_WIDE, dev, stream)
    assert np.array_equal(got, hits["hit"])


def test_instanced_nan_ray_tmax_and_poisoned_batch(pt, instanced, monkeypatch):
    si = instanced
    rt, plain = dr.mixed_ray_tmax(len(si.rs))
    for tmin in (0.001, 0.0):
        a, _ = si.scene.occluded(si.rs, tmin, 1e-3, ray_tmax=rt)
        b, _ = si.scene.occluded(si.rs, tmin, 1e-3, ray_tmax=plain)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, (f"tmin {tmin}: {len(bad)} flags differ, first rays {bad[:8]}, their ray_tmax bits "
                               f"{[hex(x) for x in rt.view(np.uint32)[bad[:8]]]}, with NaN {a[bad[:8]]}")
        want = np.zeros(len(si.rs), np.int32)
        for v in np.unique(plain):   # each ray's own interval, by the closest-hit query
            want[plain == v] = si.scene.trace(si.rs, tmin, float(v), kernel=pt.KERNEL_WIDE)[0]["hit"][plain == v]
        assert np.array_equal(a, want) and 0 < want.sum() < len(want)
    batch, at = dr.poisoned(si.classes)
    alone = structs(pt, si.classes["control"])
    for interval in dr.INTERVALS[:2]:
        for n in (len(batch), len(batch) - 37):
            keep = at[at < n]
            mixed = instanced_trace(pt, si, structs(pt, batch[:n]), interval, monkeypatch)
            solo = instanced_trace(pt, si, alone, interval, monkeypatch)
            assert mixed[keep].tobytes() == solo[:len(keep)].tobytes(), (interval, n)
            assert solo["hit"].sum() > 0
            assert (mixed[keep + 1] == miss_record(pt)).all()   # the NaN rays between them
            occ, _ = si.scene.occluded(structs(pt, batch[:n]), *interval)
            assert np.array_equal(occ, mixed["hit"])


# ------------------------------------------------------------------------------- validation
BAD = [("tmin", -1.0, np.inf), ("tmin", -1e-45, np.inf), ("tmin", np.nan, np.inf), ("tmax", 0.001, np.nan)]


def sentinel_stats(pt):
    st = pt.Stats()
    for k, _ in st._fields_:
        setattr(st, k, 77)
    return st


def entry_points(pt, scene, rs, dev):
    """name -> (call(stats, tmin, tmax) -> status, unchanged() -> bool): the five entry points, each on
    buffers of its own that hold a sentinel."""
    n = len(rs)
    hits = np.full(n * pt.HIT_DTYPE.itemsize, 0xAB, np.uint8)
    hits_ex = hits.copy()
    occ = np.full(n, 0xAB, np.uint8)
    rd = on_device(rs, dev)
    dhits = torch.full((n * pt.HIT_DTYPE.itemsize,), 0xAA, dtype=torch.uint8, device=dev)
    docc = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
    L, P = pt.lib, C.c_void_p
    host = lambda a: (a == 0xAB).all()   # noqa: E731
    devb = lambda t: bool((t == 0xAA).all().item())   # noqa: E731
    return {
        "pt_trace_closest": (lambda st, a, b: L.pt_trace_closest(scene.h, rs.ctypes.data, n, a, b, hits.ctypes.data, st),
                             lambda: host(hits)),
        "pt_trace_closest_ex": (lambda st, a, b: L.pt_trace_closest_ex(scene.h, rs.ctypes.data, n, a, b, pt.KERNEL_WIDE,
                                                                       hits_ex.ctypes.data, st), lambda: host(hits_ex)),
        "pt_trace_closest_device": (lambda st, a, b: L.pt_trace_closest_device(scene.h, P(rd.data_ptr()), n, a, b,
                                                                               pt.KERNEL_WIDE, P(dhits.data_ptr()), None, st),
                                    lambda: devb(dhits)),
        "pt_trace_occluded": (lambda st, a, b: L.pt_trace_occluded(scene.h, rs.ctypes.data, n, a, b, None, pt.KERNEL_WIDE,
                                                                   occ.ctypes.data, st), lambda: host(occ)),
        "pt_trace_occluded_device": (lambda st, a, b: L.pt_trace_occluded_device(scene.h, P(rd.data_ptr()), n, a, b, None,
                                                                                 pt.KERNEL_WIDE, P(docc.data_ptr()), None, st),
                                     lambda: devb(docc)),
    }


@pytest.mark.parametrize("which", ["flat", "instanced"])
def test_interval_validation(pt, orc, gpu, which, instanced):
    if which == "flat":
        objs, mats = dr.soup()
        scene = pt.Scene(objs, mats, device=gpu)
        rs = structs(pt, dr.class_base(dr.base_rays(objs)))
    else:
        scene, rs = instanced.scene, np.ascontiguousarray(instanced.rs[instanced.where["control"]])
    dev = torch.device("cuda", gpu)
    good, _ = scene.trace(rs, 0.0, np.inf, kernel=pt.KERNEL_WIDE)
    assert good["hit"].sum() > 0
    for fn, (call, unchanged) in entry_points(pt, scene, rs, dev).items():
        for arg, tmin, tmax in BAD:
            st = sentinel_stats(pt)
            rc = call(C.byref(st), tmin, tmax)
            msg = pt.lib.pt_last_error().decode()
            assert rc == PT_ERR_INVALID, (fn, tmin, tmax, rc, msg)
            assert msg.startswith(fn + ": " + arg + " must"), (fn, msg)
            assert unchanged(), (fn, tmin, tmax)
            assert all(getattr(st, k) == 77 for k, _ in st._fields_), (fn, tmin, tmax)
        # a valid call follows and works; -0.0 counts as 0
        st = sentinel_stats(pt)
        assert call(C.byref(st), -0.0, np.inf) == pt.PT_OK and st.rays == len(rs) and not unchanged(), fn
    for tmin in (0.0, -0.0):
        h, _ = scene.trace(rs, tmin, np.inf, kernel=pt.KERNEL_WIDE)
        assert h.tobytes() == good.tobytes()
    # with ray_tmax given the scalar tmax is ignored, whatever it holds
    rt = np.full(len(rs), np.inf, np.float32)
    a, _ = scene.occluded(rs, 0.0, np.nan, ray_tmax=rt, kernel=pt.KERNEL_WIDE)
    assert np.array_equal(a, good["hit"])
    with pytest.raises(pt.PtError) as e:
        scene.occluded(rs, -1.0, np.nan, ray_tmax=rt)
    assert e.value.code == PT_ERR_INVALID
