"""Degenerate rays and intervals for the ray-query contract (include/pt.h, pt_trace_closest): the ray
classes, intervals and scenes shared by test_degenerate_rays_host.py and test_gpu_degenerate_rays.py.

Every class is CLASS_RAYS rays built from a base batch of ordinary rays (helpers.random_rays around
the scene's box), so a class differs from the control in exactly the property its name states.
"""
import numpy as np

from helpers import INSTANCE_DTYPE, random_rays, random_soup

CLASS_RAYS = 256
BASE_RAYS = 2048
FLT_MAX = float(np.finfo(np.float32).max)
QNAN, SNAN, NEG_QNAN, NEG_SNAN = 0x7FC00000, 0x7F800001, 0xFFC00000, 0xFFBFFFFF   # any bit pattern is legal

# (tmin, tmax): the renderer's interval, tmin = 0, a one-point interval, two empty ones
INTERVALS = [(0.001, np.inf), (0.0, np.inf), (0.001, 0.001), (5.0, 1.0), (0.001, -1.0)]


def soup():
    """300 triangles and 60 spheres: binary depth 13, wide depth 4."""
    return random_soup(300, 60, seed=1)


def one_sphere():
    objs, mats = soup()
    return objs[objs["type"] == 1][:1].copy(), mats


def one_triangle():
    objs, mats = soup()
    return objs[objs["type"] == 3][:1].copy(), mats


def empty():
    objs, mats = soup()
    return objs[:0].copy(), mats


def box(objs):
    """The exact box of the objects (a sphere: centre -/+ |r|)."""
    v = objs["v"].astype(np.float64)
    sph = objs["type"] == 1
    r = np.abs(v[sph, 3:4])
    lo = np.concatenate([v[~sph].reshape(-1, 3), v[sph, :3] - r])
    hi = np.concatenate([v[~sph].reshape(-1, 3), v[sph, :3] + r])
    return lo.min(0), hi.max(0)


def base_rays(objs, n=BASE_RAYS, seed=5, reach=0.25):
    """Ordinary rays: origins on a sphere of `reach` box diagonals around the box's centre (0.25: inside
    the soup, among its primitives), half of them aimed at object centres."""
    if not len(objs):
        return random_rays(n, seed=seed)
    lo, hi = box(objs)
    return random_rays(n, seed=seed, center=(lo + hi) / 2, radius=float(np.linalg.norm(hi - lo)) * reach, objects=objs)


def class_base(base):
    """CLASS_RAYS of the base batch, evenly spread: axis-aligned, aimed and unaimed rays alike."""
    assert len(base) % CLASS_RAYS == 0
    return base[::len(base) // CLASS_RAYS].copy()


def _put(rays, first_col, bits):
    """Overwrite one component (column first_col + i % 3 of ray i) with the bit patterns `bits`."""
    out = rays.copy()
    u = out.view(np.uint32)
    i = np.arange(len(out))
    u[i, first_col + i % 3] = np.resize(np.asarray(bits, np.uint32), len(out))
    return out


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def scaled(rays, first_col, factor):
    """Three columns times `factor`: the product in double precision, rounded once to float32."""
    out = rays.copy()
    with np.errstate(over="ignore", under="ignore"):
        out[:, first_col:first_col + 3] = (rays[:, first_col:first_col + 3].astype(np.float64) * factor).astype(np.float32)
    return out


def _zero_dir(rays, objs, zero):
    """Direction (zero, zero, zero); the odd rays start inside a sphere (at its centre, and between
    centre and surface), the even ones keep their origin (outside, mostly)."""
    out = rays.copy()
    out[:, 3:] = zero
    sph = objs[objs["type"] == 1] if len(objs) else objs
    if len(sph):
        k = np.arange(1, len(out), 2)
        c = sph["v"][k % len(sph)]
        out[k, :3] = c[:, :3]
        out[k[::2], 0] += 0.5 * np.abs(c[::2, 3])
    return out


def nan_classes():
    """The classes whose every ray has a NaN component: each must miss everything."""
    return ("nan_o", "nan_d", "nan_all")


def ray_classes(objs, base):
    """name -> (CLASS_RAYS, 6) float32, in a fixed order."""
    b = class_base(base)
    nan4 = [QNAN, SNAN, NEG_QNAN, NEG_SNAN]
    c = {"control": b}
    c["nan_o"] = _put(b, 0, nan4)
    c["nan_d"] = _put(b, 3, nan4)
    c["nan_all"] = b.copy()
    c["nan_all"].view(np.uint32)[:] = np.resize(np.asarray(nan4 + [0x7FFFFFFF, 0xFF800001, 0x7FA00000], np.uint32),
                                                b.size).reshape(b.shape)
    c["pinf_o"] = _put(b, 0, _bits([np.inf]))
    c["ninf_o"] = _put(b, 0, _bits([-np.inf]))
    c["pinf_d"] = _put(b, 3, _bits([np.inf]))
    c["ninf_d"] = _put(b, 3, _bits([-np.inf]))
    c["inf_d3"] = b.copy()
    c["inf_d3"][:, 3:] = np.where(b[:, 3:] < 0, -np.inf, np.inf).astype(np.float32)
    c["zero_d"] = _zero_dir(b, objs, 0.0)
    c["negzero_d"] = _zero_dir(b, objs, -0.0)
    for name, f in (("d_1e-42", 1e-42), ("d_1e-38", 1e-38), ("d_1e-30", 1e-30), ("d_1e18", 1e18), ("d_1e30", 1e30)):
        c[name] = scaled(b, 3, f)
    c["o_1e6"] = scaled(b, 0, 1e6)
    # the same far origins aimed back at the scene (at the point o + d of the base ray): the x1e6 origins
    # alone all miss; these hit, with an origin whose ulp is the size of a primitive
    c["o_1e6_aimed"] = c["o_1e6"].copy()
    c["o_1e6_aimed"][:, 3:] = ((b[:, :3] + b[:, 3:]).astype(np.float64) - c["o_1e6"][:, :3].astype(np.float64)).astype(np.float32)
    c["o_1e30"] = scaled(b, 0, 1e30)
    c["o_fltmax"] = _put(b, 0, _bits([FLT_MAX, -FLT_MAX]))
    for name, r in c.items():
        assert r.shape == (CLASS_RAYS, 6) and r.dtype == np.float32, name
    assert np.signbit(c["negzero_d"][:, 3:]).all() and not c["negzero_d"][:, 3:].any()
    den = np.abs(c["d_1e-42"][:, 3:])   # denormal, not flushed by the helper
    assert den.max() < np.finfo(np.float32).tiny and (den > 0).any(axis=1).all()
    for name in nan_classes():
        assert np.isnan(c[name]).any(axis=1).all(), name
    return c


def concat(classes):
    """All classes in one batch (a multiple of 64 rays) and each class's slice of it."""
    where, at = {}, 0
    for name, r in classes.items():
        where[name] = slice(at, at + len(r))
        at += len(r)
    return np.concatenate(list(classes.values())), where


def poisoned(classes):
    """The control rays interleaved lane by lane with NaN, zero-direction and x1e18 rays: every wave of
    64 mixes the four.  Returns (batch, the control rays' positions in it)."""
    parts = [classes["control"], classes["nan_d"], classes["zero_d"], classes["d_1e18"]]
    batch = np.stack(parts, axis=1).reshape(-1, 6)
    return np.ascontiguousarray(batch), np.arange(0, len(batch), len(parts))


def mixed_ray_tmax(n, seed=7):
    """Per-ray tmax values: four finite ones (a reference needs one trace per value) with NaN (quiet
    and signalling, either sign) and inf entries mixed in.  Returns (ray_tmax, the same with every NaN
    replaced by inf)."""
    rng = np.random.default_rng(seed)
    rt = rng.choice(np.array([0.25, 0.5, 1.0, 2.0], np.float32), n)
    kind = rng.integers(0, 4, n)
    rt[kind == 1] = np.inf
    nan = kind == 2
    rt.view(np.uint32)[nan] = np.resize(np.asarray([QNAN, SNAN, NEG_QNAN, NEG_SNAN], np.uint32), int(nan.sum()))
    plain = rt.copy()
    plain[nan] = np.inf
    assert np.isnan(rt).sum() == nan.sum() > 0 and (kind == 0).sum() > 0
    return rt, plain


def two_instances():
    """The soup as one mesh placed twice: the identity, and a rotation about (1, 2, 3) with scales
    (0.5, 1.25, 2) and a translation -- every row of its inverse mixes the ray's components."""
    objs, mats = soup()
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    rot = np.eye(3) + np.sin(0.9) * k + (1 - np.cos(0.9)) * (k @ k)
    m = np.concatenate([rot @ np.diag([0.5, 1.25, 2.0]), [[31.0], [-7.0], [12.0]]], axis=1)
    inst = np.zeros(2, INSTANCE_DTYPE)
    inst["m"][0] = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(-1)
    inst["m"][1] = m.reshape(-1)
    assert (np.abs(m[:, :3]) > 0.05).all()
    return objs, mats, inst


def instanced_base(objs, inst, n=BASE_RAYS):
    """Ordinary rays for the two-instance scene: the soup's base batch, every other run of 8 rays
    moved by the second instance's matrix (they meet that instance as the rest meet the first;
    class_base's stride of 8 then alternates between the two)."""
    rays = base_rays(objs, n)
    m = inst["m"][1].astype(np.float64).reshape(3, 4)
    odd = np.flatnonzero(np.arange(n) % 16 >= 8)
    rays[odd, :3] = (rays[odd, :3].astype(np.float64) @ m[:, :3].T + m[:, 3]).astype(np.float32)
    rays[odd, 3:] = (rays[odd, 3:].astype(np.float64) @ m[:, :3].T).astype(np.float32)
    return rays
