"""Small triangle-only scenes for the wide LEAF step's triangle test (shared by
test_leaf_edge_scenes.py, on the CPU, and test_gpu_leaf_edges.py).

The wide render kernels test edge-form records with straight-line code: the decisions `det != 0`,
the barycentric tests, `t > tmin` and the (t, rank) minimum are lane masks, and the reciprocal's
IEEE-division fallback is the one branch.  Each scene here puts camera rays on one of those:

  degenerate  a point triangle and an axis-aligned needle (zero area: det == 0 exactly for every
              ray -- the needle is what a triangle seen edge-on comes to; with jittered camera rays
              no triangle that has an area gives an exact zero), a triangle at the origin whose
              determinant underflows to zero (edges 2^-80), and two whose determinant is denormal
              (edges 2^-65, 2^-66: the division fallback; the first has a finite reciprocal)
  huge        a triangle with edges 1.5 * 2^61 behind a small quad: |det| >= 2^126, the fallback on
              the other side, on rays that hit it
  ties        coincident triangles with different materials (same vertex order, and rotated), and a
              fan of four triangles with the camera aimed at the vertex all its edges share
  one, two, three   scenes of exactly 1, 2 and 3 triangles
  box         tests/wall_box.py's closed box: every bounce starts on a surface (t <= tmin)

`first_camera_rays` restates PT_NEW_PATH (pt_device.hip) for sample 0 of every pixel in compat mode
in numpy fp32, `tri_terms` the triangle test in the kernels' operation order; `conditions` says how
many of those rays meet each scene's condition.
"""
import numpy as np

from helpers import MATERIAL_DTYPE, OBJECT_DTYPE
from wall_box import wall_box

W = H = 32
SPP, DEPTH, SEED, CHUNK = 3, 50, 5, 2
F = np.float32


def _objs(tris, mats):
    o = np.zeros(len(tris), OBJECT_DTYPE)
    o["type"] = 3
    o["v"] = np.array(tris, np.float32).reshape(len(tris), 9)
    o["mat"] = mats
    return o


def _mats():
    m = np.zeros(3, MATERIAL_DTYPE)
    m["type"] = 1   # Lambertian
    m["albedo"] = [(0.8, 0.3, 0.2), (0.2, 0.7, 0.3), (0.3, 0.4, 0.9)]
    return m


def _wall(z=6.0, r=8.0):
    a, b, c, d = (-r, -r, z), (r, -r, z), (r, r, z), (-r, r, z)
    return [(a, b, c), (a, c, d)]


CAM = ((0.3, 0.2, -4.0), (0.0, 0.0, 6.0), 60.0, 1.0)   # (from, at, vfov, aspect)


def scenes():
    """name -> (objects, materials, camera parameters)."""
    out = {}
    z = (0.0, 0.0, 0.0)
    e80, e65, e66 = 2.0 ** -80, 2.0 ** -65, 2.0 ** -66
    deg = _wall() + [
        ((0.5, 0.5, 1.0),) * 3,                                      # a point
        ((-1.0, 0.25, 1.0), (0.0, 0.25, 1.0), (1.0, 0.25, 1.0)),     # a needle along x
        (z, (e80, 0.0, 0.0), (0.0, e80, 0.0)),                       # det underflows to zero
        (z, (e65, 0.0, 0.0), (0.0, e65, 0.0)),                       # det denormal, 1 / det finite
        (z, (e66, 0.0, 0.0), (0.0, e66, 0.0)),                       # det denormal, 1 / det infinite
    ]
    out["degenerate"] = (_objs(deg, [0, 1, 2, 2, 2, 2, 2]), _mats(), CAM)
    b, e = -(2.0 ** 60), 1.5 * 2.0 ** 61
    huge = [((b, b, 8.0), (b + e, b, 8.0), (b, b + e, 8.0)),
            ((-0.5, -0.5, 3.0), (0.5, -0.5, 3.0), (0.5, 0.5, 3.0)), ((-0.5, -0.5, 3.0), (0.5, 0.5, 3.0), (-0.5, 0.5, 3.0))]
    out["huge"] = (_objs(huge, [0, 1, 2]), _mats(), CAM)
    big = ((-2.0, -2.0, 3.0), (2.0, -2.0, 3.0), (0.0, 2.0, 3.0))
    small = ((-1.0, -1.0, 2.0), (1.0, -1.0, 2.0), (0.0, 1.0, 2.0))
    c, k = (0.0, 0.0, 1.0), [(-0.6, -0.6, 1.0), (0.6, -0.6, 1.0), (0.6, 0.6, 1.0), (-0.6, 0.6, 1.0)]
    fan = [(c, k[i], k[(i + 1) % 4]) for i in range(4)]
    ties = _wall() + [big, big, small, (small[1], small[2], small[0])] + fan
    out["ties"] = (_objs(ties, [0, 1, 0, 1, 2, 0, 1, 2, 0, 1]), _mats(), ((0.3, 0.2, -4.0), c, 60.0, 1.0))
    few = [((-6.0, -6.0, 5.0), (6.0, -6.0, 5.0), (0.0, 7.0, 5.0)), big, small]
    for n, name in ((1, "one"), (2, "two"), (3, "three")):
        out[name] = (_objs(few[:n], [0, 1, 2][:n]), _mats(), CAM)
    bo, bm = wall_box()
    out["box"] = (bo, bm, ((270.0, 280.0, 40.0), (200.0, 250.0, 500.0), 70.0, 1.0))
    return out


def first_camera_rays(orc, cam, seed=SEED, w=W, h=H):
    """Origin (3,) and directions (w * h, 3) of sample 0 of every pixel in compat mode: PT_NEW_PATH's
    arithmetic, the pixel's first two XORWOW uniforms.  cam: the camera as a float32 array."""
    cam = np.asarray(cam, np.float32)
    pos, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    rows = np.arange(h, dtype=np.int32)
    states = orc.film_states(seed, w, rows)
    u = np.zeros((h * w, 2), np.float32)
    for i in range(h * w):
        st = np.ascontiguousarray(states[i])
        u[i] = orc.curand_uniform(st, 2)
    col = np.tile(np.arange(w, dtype=np.float32), h)
    row = np.repeat(rows.astype(np.float32), w)
    inv_w, inv_h = F(1.0) / F(w), F(1.0) / F(h)
    s = ((col + u[:, 0]) * inv_w).astype(np.float32)[:, None]
    t = ((row + u[:, 1]) * inv_h).astype(np.float32)[:, None]
    d = ((ll[None, :] + s * hor[None, :]) + t * ver[None, :]) - pos[None, :]
    assert d.dtype == np.float32
    return pos.copy(), d


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def tri_terms(o, d, tri, tmin=F(0.001)):
    """primHitAny's triangle form (pt_device.hip) for rays (o, d[i]) in its operation order, fp32:
    det, t, and whether the triangle is a candidate."""
    v = np.asarray(tri, np.float32).reshape(3, 3)
    with np.errstate(all="ignore"):
        e1, e2 = v[1] - v[0], v[2] - v[0]
        s1 = _cross(d, e2[None, :])
        det = _dot(s1, e1[None, :])
        s = (o - v[0])[None, :]
        s2 = _cross(s, e1[None, :])
        inv = F(1.0) / det
        t = _dot(s2, e2[None, :]) * inv
        b1 = _dot(s1, s) * inv
        b2 = _dot(s2, d) * inv
        rej = (b1 >= 1) | (b1 <= 0) | (b2 >= 1) | (b2 <= 0) | (b1 + b2 >= 1)
        hit = (det != 0) & ~rej & (t > tmin)
    assert det.dtype == np.float32 and t.dtype == np.float32
    return det, t, hit


def conditions(orc, name, objs, cam):
    """name of a condition -> number of first camera rays that meet it, for the scene `name`."""
    o, d = first_camera_rays(orc, cam)
    tiny = np.float32(2.0 ** -126)
    tri = lambda i: objs["v"][i]
    out = {}
    if name == "degenerate":
        out["point: det == 0"] = int((tri_terms(o, d, tri(2))[0] == 0).sum())
        out["needle: det == 0"] = int((tri_terms(o, d, tri(3))[0] == 0).sum())
        out["underflow: det == 0"] = int((tri_terms(o, d, tri(4))[0] == 0).sum())
        for i, finite, what in ((5, True, "denormal det, finite reciprocal"), (6, False, "denormal det, infinite reciprocal")):
            det = tri_terms(o, d, tri(i))[0]
            with np.errstate(all="ignore"):
                fin = np.isfinite(F(1.0) / det)
            den = (det != 0) & (np.abs(det) < tiny)
            out[what] = int((den & (fin if finite else ~fin)).sum())
    elif name == "huge":
        det, _, hit = tri_terms(o, d, tri(0))
        out["|det| >= 2^126 on a candidate"] = int((np.isfinite(det) & (np.abs(det) >= F(2.0 ** 126)) & hit).sum())
    elif name == "ties":
        for a, b, what in ((2, 3, "same order"), (4, 5, "rotated")):
            _, ta, ha = tri_terms(o, d, tri(a))
            _, tb, hb = tri_terms(o, d, tri(b))
            out[f"coincident, {what}: equal t on two candidates"] = int((ha & hb & (ta == tb)).sum())
        out["fan: rays on it"] = int(np.any([tri_terms(o, d, tri(i))[2] for i in range(6, 10)], axis=0).sum())
    return out
