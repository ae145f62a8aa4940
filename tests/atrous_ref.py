"""numpy restatements of pt_render_aov and pt_film_denoise (include/pt.h states both rules).

Every line of the filter is one float32 array operation per operation of the contract, in its order
(numpy neither contracts nor reorders, and keeps denormals), so the device output is held bit for bit.
A skipped tap is excluded with np.where: it is never added, so 0 x inf cannot appear.  The AOV rule is
computed from the oracle's closest hits (oracle.trace(..., nan_miss=True)) of pixel-centre rays made
here, plus the material lookup.  A helper, not a test module.
"""
import numpy as np

from helpers import MATERIAL_DTYPE, random_soup

AOV_DTYPE = np.dtype([("albedo", "<f4", (3,)), ("depth", "<f4"), ("n", "<f4", (3,)), ("obj", "<i4"),
                      ("p", "<f4", (3,)), ("mat", "<i4")])
F = np.float32
KERNEL = (F(0.375), F(0.25), F(0.0625))
DEFAULTS = dict(iterations=5, sigma_color=0.6, sigma_albedo=0.1, sigma_plane=0.02)


def sigma_for(spp):
    """ptamd.denoise's default colour tolerance for a frame of spp samples per pixel."""
    return 1.2 / float(np.sqrt(max(1, spp)))


def pixel_rays(camera, width, height, rows):
    """The camera rays through the pixel centres of the global rows `rows`, (len(rows) * width, 6)
    float32, in the render kernels' operation order.  camera: the pt_camera as float32 words."""
    c = np.asarray(camera, F)
    org, ll, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    rows = np.asarray(rows, np.int64)
    col = np.tile(np.arange(width), len(rows)).astype(F)
    row = np.repeat(rows, width).astype(F)
    u = ((col + F(0.5)) * (F(1.0) / F(width)))[:, None]
    v = ((row + F(0.5)) * (F(1.0) / F(height)))[:, None]
    rays = np.zeros((len(col), 6), F)
    rays[:, :3] = org
    rays[:, 3:] = ((ll + u * hor) + v * ver) - org
    assert rays.dtype == F
    return rays


def aov_from_hits(hits, rays, materials):
    """The pt_aov records of closest-hit records `hits` (HIT_DTYPE fields) of `rays` ((n, 6) float32)."""
    out = np.zeros(len(hits), AOV_DTYPE)
    hit = hits["hit"] == 1
    d = np.asarray(rays, F)[:, 3:]
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert length.dtype == F
    out["depth"] = np.where(hit, hits["t"] * length, F(0))
    out["n"] = np.where(hit[:, None], hits["n"], F(0))
    out["p"] = np.where(hit[:, None], hits["p"], F(0))
    out["obj"] = np.where(hit, hits["obj"], -1)
    out["mat"] = np.where(hit, hits["mat"], -1)
    alb = np.ones((len(hits), 3), F)
    if len(materials):
        m = materials[np.clip(hits["mat"], 0, len(materials) - 1)]
        typ = np.where(hit, m["type"], 0)
        plain = (typ == 1) | (typ == 2)   # PT_LAMBERTIAN, PT_METAL
        alb = np.where(plain[:, None], m["albedo"], alb)
        alb = np.where((typ == 8)[:, None], np.minimum(m["albedo"], F(1)), alb)   # PT_EMISSIVE: fminf(E, 1)
    out["albedo"] = alb
    return out


def aov_ref(orc, objects, materials, camera, width, height, rows=None):
    """pt_render_aov's records from the oracle: the rows `rows` (default: all) of a width x height frame."""
    rows = np.arange(height) if rows is None else rows
    rays = pixel_rays(camera, width, height, rows)
    nodes = orc.build_lbvh(objects)
    hits, _ = orc.trace(objects, nodes, rays, tmin=0.001, tmax=float("inf"), nan_miss=True)
    return aov_from_hits(hits, rays, materials)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def atrous_pass(c, aov, step, isa2, isc2, sigma_plane):
    """One pass: c (H, W, 3) float32, aov (H, W) records -> the filtered (H, W, 3) float32."""
    H, W = aov.shape
    ys, xs = np.mgrid[0:H, 0:W]
    P = aov
    hit_p = P["obj"] >= 0
    plane_den = F(sigma_plane) * P["depth"]
    acc = np.zeros((H, W, 3), F)
    ws = np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * step, xs + dx * step
                keep = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                cq = c[qy, qx]
                h = KERNEL[abs(dx)] * KERNEL[abs(dy)]
                if dx == 0 and dy == 0:
                    w = np.full((H, W), h, F)
                else:
                    Q = aov[qy, qx]
                    keep &= (Q["obj"] >= 0) == hit_p
                    wn = np.fmax(F(0), _dot(P["n"], Q["n"]))
                    for _ in range(6):
                        wn = wn * wn
                    dp = Q["p"] - P["p"]
                    dist = np.abs(_dot(P["n"], dp))
                    xx = dist / plane_den
                    wp = F(1) / (F(1) + xx * xx)
                    wn = np.where(hit_p, wn, F(1))
                    wp = np.where(hit_p, wp, F(1))
                    da = Q["albedo"] - P["albedo"]
                    wa = F(1) / (F(1) + _dot(da, da) * F(isa2))
                    dc = cq - c
                    wc = F(1) / (F(1) + _dot(dc, dc) * F(isc2))
                    w = (((h * wn) * wp) * wa) * wc
                    keep &= w > 0
                assert w.dtype == F
                acc = np.where(keep[..., None], acc + w[..., None] * cq, acc)
                ws = np.where(keep, ws + w, ws)
        out = acc / ws[..., None]
    assert out.dtype == F
    return out


def atrous(rgb, aov, width, height, iterations=5, sigma_color=0.6, sigma_albedo=0.1, sigma_plane=0.02):
    """pt_film_denoise: rgb (n_pixels, 3) float32 and aov (n_pixels,) records in film order -> (n_pixels, 3)."""
    c = np.ascontiguousarray(rgb, F).reshape(height, width, 3).copy()
    g = np.ascontiguousarray(aov, AOV_DTYPE).reshape(height, width)
    isa2 = F(1.0) / (F(sigma_albedo) * F(sigma_albedo))
    with np.errstate(all="ignore"):
        for i in range(iterations):
            sc = F(sigma_color) * (F(1.0) / F(1 << i))
            isc2 = F(1.0) / (sc * sc)
            c = atrous_pass(c, g, 1 << i, isa2, isc2, sigma_plane)
    return c.reshape(-1, 3)


# ------------------------------------------------------------------------------------ shared test inputs
def lit_soup(seed=5):
    """random_soup(60, 12) with a fifth, emissive material whose E has components above and below 1."""
    objs, mats = random_soup(60, 12, seed)
    mats = np.concatenate([mats, np.zeros(1, MATERIAL_DTYPE)])
    mats[4]["type"] = 8
    mats[4]["albedo"] = (3.0, 0.4, 1.0)
    objs["mat"][::4] = 4
    return objs, mats


def synthetic_guides(W, H, seed):
    """Random guides: unit normals of every angle around a few directions (so that wn = cos^64 passes
    through the denormals: 0.2^64 ~ 1e-45), hit / miss mixes, two albedos with noise, positions near
    a few planes, and one hit with depth 0."""
    rng = np.random.default_rng(seed)
    g = np.zeros(W * H, AOV_DTYPE)
    n = rng.normal(size=(W * H, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    base = np.array([0.0, 0.0, 1.0])
    t = rng.choice([0.0, 0.02, 0.3, 0.8, 0.98, 1.0], W * H)[:, None]   # blends: cosines from 1 down through 0.2 to < 0
    n = base * (1 - t) + n * t
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    g["n"] = n
    g["p"] = rng.uniform(-2, 2, (W * H, 3)) * np.array([1.0, 1.0, 0.05])
    g["depth"] = rng.uniform(1.0, 6.0, W * H)
    g["albedo"] = rng.choice([0.2, 0.8], (W * H, 1)) + rng.uniform(-0.03, 0.03, (W * H, 3))
    g["obj"] = rng.integers(0, 50, W * H)
    g["mat"] = rng.integers(0, 4, W * H)
    miss = rng.random(W * H) < 0.25
    g["obj"][miss] = -1
    g["mat"][miss] = -1
    g["n"][miss] = 0
    g["p"][miss] = 0
    g["depth"][miss] = 0
    g["albedo"][miss] = 1
    hits = np.flatnonzero(~miss)
    if len(hits) > 1:
        g["depth"][hits[len(hits) // 2]] = 0   # a hit at depth 0: its plane term divides by 0
        g["n"][hits[1]] = g["n"][hits[0]] * F(0.2)   # |n| = 0.2: dot = 0.2 -> wn = 0.2^64 ~ 1e-45, a denormal
    return g


def synthetic_image(W, H, seed, special=True):
    rng = np.random.default_rng(seed + 100)
    c = rng.uniform(0, 1, (W * H, 3)).astype(F)
    if special:
        c[W + 2, 1] = np.nan
        c[2 * W + 1] = np.inf
    return c
