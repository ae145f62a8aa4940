"""Inputs of the reference-parity cases (a helper module, not a test file), shared by
tests/test_reference_parity.py (the reference's own code, compiled for the CPU, against the oracle)
and tools/make_reference_fixtures.py (which records the reference's outputs on a subset of them
into tests/golden/reference_fixtures.npz for the GPU tests).  Everything is seeded."""
import numpy as np

import degenerate_rays as dg
from helpers import MATERIAL_DTYPE, duplicate_centroids, random_soup

F = np.float32
HIT_DTYPE = np.dtype([("hit", "<i4"), ("obj", "<i4"), ("mat", "<i4"), ("front_face", "<i4"),
                      ("t", "<f4"), ("p", "<f4", (3,)), ("n", "<f4", (3,))])

# ------------------------------------------------------------------------------------- LBVH
# the sizes at which Karras ranges go wrong: a leaf root, one internal node, odd counts, a full
# block of 64 lanes and one lane more, and a few blocks
LBVH_SIZES = (1, 2, 3, 7, 64, 65, 1000)
LBVH_KINDS = ("soup", "dup")


def lbvh_objects(kind, n):
    if kind == "dup":   # all Morton codes equal: the object id alone orders the keys
        return duplicate_centroids(n)[0]
    return random_soup(n - n // 4, n // 4, seed=100 + n)[0]


# --------------------------------------------------------------------------- degenerate rays
def degenerate_scenes():
    """name -> objects: the soup of tests/degenerate_rays.py with every third sphere's radius
    negated (the reference's hollow-glass trick, main.cu:233), and the one-primitive scenes (no box
    test in the reference)."""
    soup = dg.soup()[0].copy()
    sph = np.flatnonzero(soup["type"] == 1)
    soup["v"][sph[::3], 3] *= -1
    one_neg = dg.one_sphere()[0].copy()
    one_neg["v"][:, 3] *= -1
    return {"soup_negr": soup, "one_sphere": dg.one_sphere()[0], "one_sphere_negr": one_neg,
            "one_triangle": dg.one_triangle()[0]}


def degenerate_batch(objs, stride=1):
    """All ray classes of tests/degenerate_rays.py in one batch (every `stride`-th ray of each class)
    and each class's slice."""
    classes = dg.ray_classes(objs, dg.base_rays(objs))
    return dg.concat({k: v[::stride].copy() for k, v in classes.items()})


# ------------------------------------------------------------------------------- scatter
def _hit(p, n, front, t=1.0, mat=0):
    h = np.zeros(1, HIT_DTYPE)[0]
    h["hit"], h["obj"], h["mat"], h["front_face"], h["t"] = 1, 0, mat, int(front), t
    h["p"], h["n"] = p, n
    return h


def scatter_edges(tape_len=160):
    """Constructed Material::scatter cases: (materials, case_mat, case_ray (k, 6), case_hit (k,),
    tapes (k, tape_len), labels).  A tape is in the order the draws are TAKEN, so which coordinate a
    draw lands in depends on the draw order; the cases that aim a vector come in both orders."""
    mats, cm, rays, hits, tapes, labels = [], [], [], [], [], []

    def material(t, albedo=(0.8, 0.6, 0.4), fuzz=0.0, ir=0.0):
        m = np.zeros(1, MATERIAL_DTYPE)[0]
        m["type"], m["albedo"], m["fuzz"], m["ir"] = t, albedo, fuzz, ir
        mats.append(m)
        return len(mats) - 1

    def case(label, mat, d, hit, tape):
        t = np.full(tape_len, 0.5, F)
        tape = np.asarray(tape, F).reshape(-1)
        assert len(tape) <= tape_len
        t[:len(tape)] = tape
        cm.append(mat)
        rays.append(np.concatenate([np.asarray(hit["p"], F) - np.asarray(d, F), np.asarray(d, F)]).astype(F))
        hits.append(hit)
        tapes.append(t)
        labels.append(label)

    p = (1.5, -2.25, 3.0)
    n = np.array([0.0, 1.0, 0.0], F)
    tilt = np.array([0.6, 0.8, 0.0], F)   # an exact unit vector off the axes
    # dielectric: ir x face x incidence (cos from normal to grazing) x the uniform the reflectance meets
    for ir in (1.0, 1.5, 1.0 / 1.5, 2.4):
        m = material(4, ir=ir)
        for front in (1, 0):
            for nrm in (n, tilt):
                for c in (1.0, 0.9, 0.5, 0.2, 0.05, 1e-3, 1e-6):
                    s = np.sqrt(1.0 - c * c)
                    # a direction at angle acos(c) to -nrm, unnormalised (scaled by 3.7)
                    tang = np.array([0.0, 0.0, 1.0]) if nrm is n else np.array([-0.8, 0.6, 0.0])
                    d = (3.7 * (-c * nrm.astype(np.float64) + s * tang)).astype(F)
                    for u in (1e-9, 0.04, 0.5, 1.0):
                        case(f"dielectric ir={ir:.3g} front={front} cos={c:g} u={u:g}", m, d, _hit(p, nrm, front), [u])
    # total internal reflection by construction: leaving glass (back face, ratio 1.5) at 60 degrees,
    # and entering "anti-glass" (front face, ir = 1/1.5)
    for ir, front in ((1.5, 0), (1.0 / 1.5, 1), (2.4, 0)):
        m = material(4, ir=ir)
        d = np.array([np.sin(np.pi / 3), -np.cos(np.pi / 3), 0.0], F)
        case(f"TIR ir={ir:.3g}", m, d, _hit(p, n, front), [0.999])
    # cos_theta above 1, clamped by the fminf: a hit normal longer than 1 (the record is an input)
    m15 = material(4, ir=1.5)
    for scale in (1.0000001, 2.0, 1e3):
        case(f"cos clamp |n|={scale:g}", m15, (0.0, -2.0, 0.0), _hit(p, n * F(scale), 1), [0.3])
    case("cos clamp, rounding", m15, (-0.6 * 7, -0.8 * 7, 0.0), _hit(p, tilt, 1), [0.3])
    # metal: fuzz x grazing incidence, the fuzz vector aimed below and above the surface in either
    # draw order (y is the middle draw in both; x and z swap) -> the absorb exit and its neighbour
    for fuzz in (0.0, 0.3, 1.0):
        m = material(2, fuzz=fuzz)
        for graze in (1e-1, 1e-3, 1e-6, 0.0):
            d = np.array([1.0, -graze, 0.25], F)
            for vy in (0.05, 0.5, 0.95):
                for vx, vz in ((0.5, 0.5), (0.3, 0.6), (0.6, 0.3)):
                    case(f"metal fuzz={fuzz} graze={graze:g} v=({vx},{vy},{vz})", m, d, _hit(p, n, 1), [vx, vy, vz])
    m = material(2, fuzz=1.0)
    case("metal zero direction", m, (0.0, 0.0, 0.0), _hit(p, n, 1), [0.5, 0.5, 0.5])
    # Lambertian: a unit vector opposite to the normal -> near_zero; along every axis, in both orders
    lam = material(1)
    for axis in range(3):
        nrm = np.zeros(3, F)
        nrm[axis] = 1.0
        for u in (0.05, 0.1, 0.2, 0.25, 0.3, 0.4, 0.45, 0.0500001):
            for order in (0, 1):
                t = [0.5, 0.5, 0.5]
                t[axis if order == 0 else 2 - axis] = u
                case(f"lambertian near_zero axis={axis} u={u:g} order={order}", lam, (0.3, -1.0, 0.2), _hit(p, nrm, 1), t)
    # the near_zero threshold itself (1e-7): u = 0.25 on the axis gives the unit vector -axis exactly,
    # so normal + vector = |normal| - 1 exactly: 2^-21, 2^-22, 2^-23 (1.19e-7, just not near zero),
    # -2^-24 (5.96e-8, near zero), -2^-23
    for axis in range(3):
        for excess in (2.0 ** -21, 2.0 ** -22, 2.0 ** -23, -2.0 ** -24, -2.0 ** -23):
            nrm = np.zeros(3, F)
            nrm[axis] = F(1.0 + excess)
            assert float(nrm[axis]) == 1.0 + excess
            for order in (0, 1):
                t = [0.5, 0.5, 0.5]
                t[axis if order == 0 else 2 - axis] = 0.25
                case(f"lambertian near_zero threshold axis={axis} excess={excess:g} order={order}", lam,
                     (0.3, -1.0, 0.2), _hit(p, nrm, 1), t)
    case("lambertian zero candidate", lam, (0.3, -1.0, 0.2), _hit(p, n, 1), [0.5, 0.5, 0.5])
    # a type the reference does not know: no draw, false
    for t in (0, 3, 8, -1):
        case(f"unknown type {t}", material(t, fuzz=0.5, ir=1.5), (0.3, -1.0, 0.2), _hit(p, n, 1), [0.25, 0.75, 0.25])
    # long rejection loops: k rejected candidates (corners of the cube, |v|^2 = 3 ... just outside
    # the sphere), then an accepted one
    outside = 0.5 + 0.5 / np.sqrt(3.0) + 1e-4   # |2 (u - 0.5)|^2 * 3 just above 1
    for mat in (lam, material(2, fuzz=0.3)):
        for k in (1, 7, 52):
            for rej in (1.0, outside, 1e-9):
                case(f"rejections mat={mat} k={k} rej={rej:g}", mat, (0.3, -1.0, 0.2), _hit(p, tilt, 1),
                     [rej] * (3 * k) + [0.7, 0.6, 0.4])
    # exactly on the sphere: rejected (>= 1): 2 (1 - 0.5) = 1, 0, 0
    case("rejection boundary", lam, (0.3, -1.0, 0.2), _hit(p, n, 1), [1.0, 0.5, 0.5, 0.5, 1.0, 0.5, 0.7, 0.6, 0.4])
    return (np.array(mats, MATERIAL_DTYPE), np.array(cm, np.int32), np.stack(rays), np.array(hits, HIT_DTYPE),
            np.stack(tapes), labels)


def scatter_bulk(orc, per_type=20000, tape_len=48, seed=11):
    """per_type seeded cases for each material type on real hits of the degenerate-ray soup (front
    and back faces): (materials, case_mat, case_ray, case_hit, tapes)."""
    objs = dg.soup()[0]
    rays = dg.base_rays(objs, n=8192, seed=9)
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    hits, _ = orc.trace(objs, nodes, rays)
    idx = np.flatnonzero(hits["hit"] == 1)
    assert len(idx) > 1000 and (hits["front_face"][idx] == 1).sum() > 300 and (hits["front_face"][idx] == 0).sum() > 300
    rng = np.random.default_rng(seed)
    mats = np.zeros(12, MATERIAL_DTYPE)
    mats["type"] = [1] * 4 + [2] * 4 + [4] * 4
    mats["albedo"] = rng.uniform(0.05, 0.95, (12, 3))
    mats["fuzz"][4:8] = [0.0, 0.3, 1.0, 0.07]
    mats["ir"][8:12] = [1.5, 1.0 / 1.5, 2.4, 1.0]
    k = 3 * per_type
    case_mat = np.repeat(np.arange(3), per_type) * 4 + rng.integers(0, 4, k)
    pick = idx[rng.integers(0, len(idx), k)]
    tapes = rng.uniform(0.0, 1.0, (k, tape_len)).astype(F)
    tapes[tapes == 0] = F(1.0)   # curand_uniform's range is (0, 1]
    return mats, case_mat.astype(np.int32), rays[pick], hits[pick], tapes


# -------------------------------------------------------------------------------- cameras
# from, at, vfov, aspect, aperture, focus, t0, t1 -- the presets' (pt_host.cpp) first, then off-axis ones
CAMERA_PRESETS = {"triangle_world": (0, 0), "random_world": (0, 0), "test_world": (0, 0), "rtiow": (400, 225),
                  "cornell": (64, 64)}
CAMERA_ARGS = np.array([
    [0, 0, 25, 0, 0, 0, 40, 16.0 / 9.0, 0, 10, 0, 1],            # triangle_world (main.cu:438-442)
    [0, 30, 0.1, 0, 0, 0, 20, 16.0 / 9.0, 0, 10, 0, 1],          # random_world (main.cu:412-416)
    [0, 0, 15, 0, 0, 0, 20, 16.0 / 9.0, 0, 10, 0, 1],            # test_world (main.cu:430-434)
    [13, 2, 3, 0, 0, 0, 20, 400.0 / 225.0, 0, 10, 0, 1],         # rtiow
    [278, 273, -800, 278, 273, 0, 40, 1.0, 0, 10, 0, 1],         # cornell
    [-0.7606797218322754, -3.7550902366638184, 9.920369148254395, -0.7577590346336365, -4.791014194488525,
     9.05327320098877, 90.0, 1.5, 0, 10, 0, 1],                   # tests/pathloop.py L2
    [3.3, -7.1, 2.9, -1.2, 0.4, 8.8, 63.5, 1.85, 0.3, 4.2, 0.25, 0.75],
    [0.001, 50, 0, 0, 0, 0, 35, 4.0 / 3.0, 0.05, 50, 0, 0],       # nearly straight down
    [0, 5, 0, 0, 0, 0, 35, 1.0, 0, 5, 0, 1],                      # straight down: cross((0,1,0), front) = 0
    [1e6, -2e6, 3e6, 1e6 + 1, -2e6, 3e6 - 2, 1.0, 2.39, 2.0, 1e3, 1, 0],
    [2, 2, 2, 2, 2, 2, 179.0, 0.5, 0, 1, 0, 1],                   # from == at: a zero front
], F)
CAMERA_MOVE_DIR = np.array([0, 1, 2, 3, 4, 5, 0, 3, 4, 4], np.int32)
CAMERA_MOVE_DT = np.array([0.016, 0.5, 0.033, 1.0, 0.25, 2.0, 1e-4, 3.5, 0.0, 100.0], F)


# --------------------------------------------------------------------------------- frames
def frame_cases(pt, orc):
    """name -> dict(objects, materials, camera (25 floats), width, height, spp, depth, seed, launches)."""
    import pathloop
    out = {}
    for name, preset, w, h, spp, depth, seed, launches in (
            ("rtiow", "rtiow", 64, 36, 4, 50, 3, 1), ("triangle_world", "triangle_world", 48, 27, 2, 50, 5, 1),
            ("cornell", "cornell", 32, 32, 4, 8, 7, 1)):
        if preset == "triangle_world":   # the camera is the reference's 16:9 one (main.cu:438-442), whatever the frame
            p = pt.Preset(preset)
            cam = orc.camera_make((0, 0, 25), (0, 0, 0), 40, 16.0 / 9.0)
        else:
            p = pt.Preset(preset, w, h)
            cam = pt.camera_to_array(p.camera)
        out[name] = dict(objects=p.objects, materials=p.materials, camera=cam, width=w, height=h, spp=spp,
                         depth=depth, seed=seed, launches=launches)
    # L2 of tests/pathloop.py under the reference's sky, its emissive material made Lambertian: the
    # camera sits inside a glass sphere (TIR, depth exhaustion), with metal and dielectric triangles
    sc = pathloop.lit_scene("L2")
    mats = sc.materials.copy()
    mats[4]["type"] = 1
    mats[4]["albedo"] = (0.8, 0.6, 0.5)
    out["l2"] = dict(objects=sc.objects, materials=mats, camera=sc.camera, width=24, height=16, spp=3, depth=12,
                     seed=21, launches=2)   # the second launch continues the streams
    r = out["rtiow"]
    for depth in (0, 1):
        out[f"rtiow_depth{depth}"] = dict(r, width=32, height=18, spp=2, depth=depth, seed=11 + depth,
                                          camera=pt.camera_to_array(pt.Preset("rtiow", 32, 18).camera))
    return out


def oracle_frames(orc, c):
    """orc.render on a frame case: (rgb (launches, npix, 3), states (launches, npix, 6))."""
    w, h = c["width"], c["height"]
    rows = np.arange(h, dtype=np.int32)
    nodes = orc.build_lbvh(c["objects"], orc.morton_keys(c["objects"]), tight=True)
    states = orc.film_states(c["seed"], w, rows)
    rgb, after = [], []
    for _ in range(c["launches"]):
        img, _ = orc.render(c["objects"], c["materials"], nodes, c["camera"], w, h, rows, c["spp"], c["depth"], states,
                            nthreads=4)
        rgb.append(img)
        after.append(states.copy())
    return np.stack(rgb), np.stack(after)
